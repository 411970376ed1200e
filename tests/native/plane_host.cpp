// Test-only host simulation of the dominant-plane extraction (parsenet_codebase_amd/csrc/plane.hip): the launches of its
// schedule run serially, one after the other, on the SAME definitions the kernels compile (csrc/plane_math.h on
// csrc/outlier_math.h and csrc/normal_math.h): bounds, hypotheses, scores per tile of 1 024 points with a flush of the
// tile's counters into the cloud's, selection, then per round mean partials, mean, moment partials, moments + Jacobi, the
// refit's count and the decision, then inlier and dist.  The tiles flush their counters — the scores' and the refit's —
// in ascending order or, with order = 1, in descending order: integer sums, which must not change a bit.  The sums of
// the refinement go through the tree of outlier_math.h exactly as the workgroups run it (ol_lane_sum of the lane's four
// points, ol_butterfly per run of 64 lanes, ol_wave_sum, the tile sums in ascending order).  tests/test_plane_abi.py
// holds the result against an independent numpy restatement in every bit.  Not part of the product.
//
// As a program (it has a main): without an argument it runs its own list of clouds in both orders against a brute force
// (every hypothesis against every point, one after the other) and prints "<cases> cases, <d> differences" (exit 1 when
// d > 0); with a file of cases, each `n t H seed refine has_axis ax ay az min_cos` + n lines `x y z`, it runs every case
// in both orders and prints count, best, the four numbers of the plane, then per point inlier and dist (exit 1 when the
// orders differ).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../parsenet_codebase_amd/csrc/plane_math.h"
#include "../../parsenet_codebase_amd/csrc/ragged.h"

// The sum of the 1 024 terms of a tile as a workgroup of 256 lanes forms it.
static double plh_tile_sum(const double* v) {
  double w[OL_WAVES];
  for (int wave = 0; wave < OL_WAVES; ++wave) {
    double s[OL_WAVE];
    for (int l = 0; l < OL_WAVE; ++l) {
      const int lane = wave * OL_WAVE + l;
      s[l] = ol_lane_sum(v[lane], v[lane + OL_LANES], v[lane + 2 * OL_LANES], v[lane + 3 * OL_LANES]);
    }
    ol_butterfly(s);
    w[wave] = s[0];
  }
  return ol_wave_sum(w[0], w[1], w[2], w[3]);
}

static int plh_point_inlier(const double* q, const float* p, double t) {
  return pl_inlier(pl_signed(q[0], q[1], q[2], q[3], (double)p[0], (double)p[1], (double)p[2]), t);
}

// The inliers of plane q over the segment, counted tile by tile, the tiles' counts added in `order`.
static int plh_count(const float* P, int n, const double* q, double t, int order) {
  const int nt = ol_cloud_tiles(n);
  std::vector<int> tcount(nt, 0);
  for (int b = 0; b < nt; ++b)
    for (int i = b * PL_TILE; i < std::min(n, (b + 1) * PL_TILE); ++i) tcount[b] += plh_point_inlier(q, P + 3 * i, t);
  int s = 0;
  for (int c = 0, b = order ? nt - 1 : 0; c < nt; ++c, b += order ? -1 : 1) s += tcount[b];
  return s;
}

// One valid segment.
static void plh_segment(const float* P, int n, float tf, int H, unsigned long long seed, int refine, const double* axis,
                        double min_cos, int order, double* plane, int32_t* count, int32_t* best, uint8_t* inlier,
                        float* dist) {
  const int nt = ol_cloud_tiles(n);
  // bounds
  int bad = 0;
  for (int i = 0; i < 3 * n; ++i) bad |= !kg_finite(P[i]);
  // hypotheses
  std::vector<PlPlane> hyp(H);
  for (int h = 0; h < H; ++h) hyp[h] = pl_hypothesis(P, n, seed, h, axis, min_cos);
  const int status = pl_status(bad, tf);
  const double t = (double)tf;
  // scores: the counters of a tile, then their flush
  std::vector<uint32_t> hcount(H, 0u), tile(H);
  if (pl_threshold_ok(tf))
    for (int c = 0, b = order ? nt - 1 : 0; c < nt; ++c, b += order ? -1 : 1) {
      std::fill(tile.begin(), tile.end(), 0u);
      for (int h = 0; h < H; ++h) {
        if (!hyp[h].valid) continue;
        const double q[4] = {hyp[h].nx, hyp[h].ny, hyp[h].nz, hyp[h].d};
        for (int i = b * PL_TILE; i < std::min(n, (b + 1) * PL_TILE); ++i)
          tile[h] += (uint32_t)plh_point_inlier(q, P + 3 * i, t);
      }
      for (int h = 0; h < H; ++h)
        if (tile[h]) hcount[h] += tile[h];
    }
  // selection
  unsigned long long key = 0ull;
  for (int h = 0; h < H; ++h)
    if (hyp[h].valid) key = std::max(key, pl_key(hcount[h], (uint32_t)h));
  const int win = status == 0 ? pl_key_h(key) : -1;
  plane[0] = plane[1] = plane[2] = plane[3] = 0.0;
  *count = status;
  *best = win;
  if (win >= 0) {
    plane[0] = hyp[win].nx, plane[1] = hyp[win].ny, plane[2] = hyp[win].nz, plane[3] = hyp[win].d;
    *count = pl_key_count(key);
  }
  // refinement
  std::vector<double> part(PL_MOMENTS * (size_t)nt), v(PL_TILE);
  for (int r = 0; r < refine && win >= 0; ++r) {
    double mean[3] = {0.0, 0.0, 0.0}, sums[PL_MOMENTS];
    for (int stage = 0; stage < 2; ++stage) {
      const int K = stage == 0 ? 3 : PL_MOMENTS;
      for (int b = 0; b < nt; ++b)
        for (int k = 0; k < K; ++k) {
          std::fill(v.begin(), v.end(), 0.0);                                  // an absent point enters as 0.0
          for (int i = b * PL_TILE; i < std::min(n, (b + 1) * PL_TILE); ++i) {
            const float* p = P + 3 * i;
            const int in = plh_point_inlier(plane, p, t);
            double term = (double)p[k % 3];
            if (stage == 1) {
              double prod[PL_MOMENTS];
              pl_products((double)p[0], (double)p[1], (double)p[2], mean, prod);
              term = prod[k];
            }
            v[i - b * PL_TILE] = pl_term(in, term);
          }
          part[(size_t)k * nt + b] = plh_tile_sum(v.data());
        }
      for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int b = 0; b < nt; ++b) s = ol_add(s, part[(size_t)k * nt + b]);
        if (stage == 0) mean[k] = pl_mean(s, *count);
        else sums[k] = s;
      }
    }
    const PlPlane cand = pl_refit(mean, sums, *count, axis, min_cos);
    if (!cand.valid) continue;
    const double q[4] = {cand.nx, cand.ny, cand.nz, cand.d};
    const int m = plh_count(P, n, q, t, order);
    if (!pl_take(1, m, *count)) continue;
    plane[0] = q[0], plane[1] = q[1], plane[2] = q[2], plane[3] = q[3];
    *count = m;
  }
  // inlier and dist
  for (int i = 0; i < n; ++i) {
    const float* p = P + 3 * i;
    const double s =
        win >= 0 ? pl_signed(plane[0], plane[1], plane[2], plane[3], (double)p[0], (double)p[1], (double)p[2]) : ol_nan();
    inlier[i] = (uint8_t)(win >= 0 && pl_inlier(s, t));
    if (dist) dist[i] = (float)s;
  }
}

// A ragged batch: pts (total,3), off (S+1), threshold (S); axis and dist may be null.  Returns pl_launches(refine).
extern "C" int plh_plane(const float* pts, const int* off, int S, int total, const float* threshold, int H,
                         unsigned long long seed, int refine, const double* axis, double min_cos, int order,
                         double* plane, int32_t* count, int32_t* best, uint8_t* inlier, float* dist) {
  for (int s = 0; s < S; ++s) {
    const int o0 = off[s], o1 = off[s + 1];
    if (!rg_valid_segment(o0, o1, total)) {
      for (int k = 0; k < 4; ++k) plane[4 * s + k] = 0.0;
      count[s] = 0, best[s] = -1;
      continue;
    }
    plh_segment(pts + 3 * (size_t)o0, o1 - o0, threshold[s], H, seed, refine, axis, min_cos, order, plane + 4 * s,
                count + s, best + s, inlier + o0, dist ? dist + o0 : nullptr);
  }
  return pl_launches(refine);
}

extern "C" int plh_launches(int refine) { return pl_launches(refine); }
extern "C" int plh_constant(int which) {
  const int c[] = {PL_TILE, PL_MAX_H, PL_MAX_REFINE, NM_SWEEPS, PL_MOMENTS};
  return which >= 0 && which < 5 ? c[which] : -1;
}
extern "C" unsigned long long plh_mix(unsigned long long z) { return pl_mix(z); }
extern "C" int plh_draw(unsigned long long seed, int h, int s, int n) { return pl_draw(seed, h, s, n); }
// The refit of given mean (3) and moment sums (6) over m points -> out (4); returns its validity.
extern "C" int plh_refit(const double* mean, const double* sums, int m, const double* axis, double min_cos, double* out) {
  const PlPlane p = pl_refit(mean, sums, m, axis, min_cos);
  out[0] = p.nx, out[1] = p.ny, out[2] = p.nz, out[3] = p.d;
  return p.valid;
}

// ---- the program ------------------------------------------------------------------------------------------------------
static uint32_t plh_state = 12345u;
static float plh_uniform(void) {
  plh_state = plh_state * 1664525u + 1013904223u;
  return (float)(plh_state >> 8) / 8388608.0f - 1.0f;                  // [-1, 1)
}

struct PlhResult {
  double plane[4];
  int32_t count, best;
  std::vector<uint8_t> inlier;
  std::vector<float> dist;
};

static PlhResult plh_run(const std::vector<float>& P, int n, float t, int H, unsigned long long seed, int refine,
                         const double* axis, double min_cos, int order) {
  PlhResult r;
  r.inlier.assign(n + 1, 9);
  r.dist.assign(n + 1, -9.0f);
  const int off[2] = {0, n};
  plh_plane(P.data(), off, 1, n, &t, H, seed, refine, axis, min_cos, order, r.plane, &r.count, &r.best, r.inlier.data(),
            r.dist.data());
  return r;
}

static int plh_same(const PlhResult& a, const PlhResult& b) {
  return a.count == b.count && a.best == b.best && !memcmp(a.plane, b.plane, sizeof a.plane) && a.inlier == b.inlier &&
         !memcmp(a.dist.data(), b.dist.data(), a.dist.size() * sizeof(float));
}

// The definition without refinement by brute force, and what must hold with it.
static int plh_check(const std::vector<float>& P, int n, float t, int H, unsigned long long seed, const double* axis,
                     double min_cos) {
  int diff = 0, bad = 0;
  for (int i = 0; i < 3 * n; ++i) bad |= !kg_finite(P[i]);
  int want_best = -1, want_count = pl_status(bad, t);
  if (want_count == 0)
    for (int h = 0; h < H; ++h) {
      const PlPlane p = pl_hypothesis(P.data(), n, seed, h, axis, min_cos);
      if (!p.valid) continue;
      const double q[4] = {p.nx, p.ny, p.nz, p.d};
      int m = 0;
      for (int i = 0; i < n; ++i) m += plh_point_inlier(q, &P[3 * i], (double)t);
      if (want_best < 0 || m > want_count) want_best = h, want_count = m;
    }
  int before = -1;
  for (int refine = 0; refine <= PL_MAX_REFINE; ++refine) {
    const PlhResult a = plh_run(P, n, t, H, seed, refine, axis, min_cos, 0);
    const PlhResult b = plh_run(P, n, t, H, seed, refine, axis, min_cos, 1);
    diff += !plh_same(a, b);
    diff += a.best != want_best;
    if (refine == 0) diff += a.count != want_count;
    int m = 0;
    for (int i = 0; i < n; ++i) m += a.inlier[i];
    diff += a.best >= 0 ? m != a.count : (m != 0 || a.count > 0);
    diff += a.best >= 0 && a.count < before;                           // refinement never loses inliers
    before = a.count;
    diff += a.inlier[n] != 9 || a.dist[n] != -9.0f;                    // nothing is written behind the segment
  }
  return diff;
}

int main(int argc, char** argv) {
  if (argc > 1) {
    FILE* f = fopen(argv[1], "r");
    if (!f) {
      fprintf(stderr, "plane_host: cannot open %s\n", argv[1]);
      return 2;
    }
    int n = 0, H = 0, refine = 0, has_axis = 0, rc = 0, got = 0;
    unsigned long long seed = 0ull;
    float t = 0.0f;
    double axis[3], min_cos = 0.0;
    while ((got = fscanf(f, "%d %f %d %llu %d %d %lf %lf %lf %lf", &n, &t, &H, &seed, &refine, &has_axis, &axis[0],
                         &axis[1], &axis[2], &min_cos)) == 10) {
      if (n < 0 || n > (1 << 20) || H < 1 || H > PL_MAX_H || refine < 0 || refine > PL_MAX_REFINE) {
        fprintf(stderr, "plane_host: expected `n t H seed refine has_axis ax ay az min_cos`\n");
        fclose(f);
        return 2;
      }
      std::vector<float> P(3 * (size_t)n + 1);
      for (int i = 0; i < n; ++i)
        if (fscanf(f, "%f %f %f", &P[3 * i], &P[3 * i + 1], &P[3 * i + 2]) != 3) {
          fprintf(stderr, "plane_host: %d points announced, point %d is missing\n", n, i);
          fclose(f);
          return 2;
        }
      const PlhResult a = plh_run(P, n, t, H, seed, refine, has_axis ? axis : nullptr, min_cos, 0);
      const PlhResult b = plh_run(P, n, t, H, seed, refine, has_axis ? axis : nullptr, min_cos, 1);
      printf("%d %d %.17g %.17g %.17g %.17g\n", a.count, a.best, a.plane[0], a.plane[1], a.plane[2], a.plane[3]);
      for (int i = 0; i < n; ++i) printf("%d %.9g\n", (int)a.inlier[i], a.dist[i]);
      if (!plh_same(a, b)) rc = 1;
    }
    fclose(f);
    if (got != EOF) {
      fprintf(stderr, "plane_host: expected `n t H seed refine has_axis ax ay az min_cos`\n");
      return 2;
    }
    return rc;
  }
  int cases = 0, diff = 0;
  const int sizes[] = {0, 1, 2, 3, 4, 65, 700, 1025, 2049};
  const double up[3] = {0.0, 0.0, 1.0};
  for (int n : sizes)
    for (int H : {1, 65, 200})
      for (float t : {0.02f, 0.3f}) {
        std::vector<float> P(3 * (size_t)n + 1);
        for (int i = 0; i < n; ++i) {                                  // two thirds on a noisy plane, the rest anywhere
          P[3 * i] = plh_uniform(), P[3 * i + 1] = plh_uniform();
          P[3 * i + 2] = i % 3 ? 0.01f * plh_uniform() + 0.25f * P[3 * i] : plh_uniform();
        }
        diff += plh_check(P, n, t, H, 7ull + (unsigned)n, nullptr, 0.0), ++cases;
        diff += plh_check(P, n, t, H, 0xFEDCBA9876543210ull, up, 0.9), ++cases;
      }
  {                                                                    // a lattice plane: every valid hypothesis holds all
    const int m = 20;
    std::vector<float> P;
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) P.push_back(0.125f * i), P.push_back(0.125f * j), P.push_back(1.0f);
    diff += plh_check(P, m * m, 0.25f, 64, 3ull, nullptr, 0.0), ++cases;
    for (float t : {0.0f, -1.0f, kg_inf(), kg_inf() - kg_inf()}) diff += plh_check(P, m * m, t, 64, 3ull, nullptr, 0.0), ++cases;
    P[3 * 77 + 1] = kg_inf();                                          // a non-finite coordinate
    diff += plh_check(P, m * m, 0.25f, 64, 3ull, nullptr, 0.0), ++cases;
  }
  {                                                                    // collinear and coincident clouds: no plane
    std::vector<float> P(3 * 300), Q(3 * 300, 0.5f);
    for (int i = 0; i < 300; ++i) P[3 * i] = 0.01f * i, P[3 * i + 1] = 0.02f * i, P[3 * i + 2] = -0.01f * i;
    diff += plh_check(P, 300, 0.1f, 100, 5ull, nullptr, 0.0), ++cases;
    diff += plh_check(Q, 300, 0.1f, 100, 5ull, nullptr, 0.0), ++cases;
  }
  printf("%d cases, %d differences\n", cases, diff);
  return diff ? 1 : 0;
}
