// Test-only host simulation of the rigid registration (parsenet_codebase_amd/csrc/register.hip): the launches of its
// schedule run serially on the SAME definitions the kernels compile (csrc/register_math.h on csrc/outlier_math.h and
// csrc/normal_math.h; the search on csrc/knn3_grid_math.h: the target's grid built once, every iteration the moved points
// searched in it by rings with the termination bound, selection by (d, j)): init, then per iteration move, pair, the mean
// sums per tile, the means, the centred sums per tile, the solve with the stopping rule, then the final evaluation.  The
// sums go through the tree of outlier_math.h exactly as the workgroups run it; the tiles are visited in ascending order
// or, with order = 1, in descending order — the partials land in their slots and the counts are integers, so no bit may
// change.  tests/test_register_abi.py holds every output against an independent numpy restatement.  Not part of the
// product.
//
// As a program (it has a main) it reads cases from the file named by its argument, each
//     S mode max_dist max_iter tol_rot tol_trans has_normals has_init
//     per segment:  ns nt, [16 numbers of init], ns lines x y z, nt lines x y z [nx ny nz]
// runs every case in both orders (exit 1 when they differ) and prints per segment the 16 numbers of the transform,
// iterations, status, count, rmse, then per source point idx and dist.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../parsenet_codebase_amd/csrc/knn3_grid_math.h"
#include "../../parsenet_codebase_amd/csrc/register_math.h"

// ---- the target's grid and the k = 1 query in it (the restatement of tests/native/knn3_query_host.cpp) ----------------
struct RrhGrid {
  KgGrid g;
  bool flagged;
  std::vector<int> start, order;
};

static RrhGrid rrh_build(const float* R, int n, int ppc) {
  RrhGrid s;
  s.flagged = false;
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const float x = R[3 * i + a];
      if (!kg_finite(x)) s.flagged = true;
      if (i == 0 || x < lo[a]) lo[a] = x;
      if (i == 0 || x > hi[a]) hi[a] = x;
    }
  if (s.flagged || n == 0) return s;
  s.g = kg_grid(n, lo, hi, ppc);
  const int cells = kg_cells(s.g);
  s.start.assign(cells + 1, 0);
  std::vector<int> of(n);
  for (int i = 0; i < n; ++i) {
    of[i] = kg_cell_index(s.g, kg_cell(s.g, 0, R[3 * i]), kg_cell(s.g, 1, R[3 * i + 1]), kg_cell(s.g, 2, R[3 * i + 2]));
    ++s.start[of[i] + 1];
  }
  for (int c = 0; c < cells; ++c) s.start[c + 1] += s.start[c];
  s.order.resize(n);
  std::vector<int> fill(s.start.begin(), s.start.end() - 1);
  for (int i = 0; i < n; ++i) s.order[fill[of[i]]++] = i;
  return s;
}

// The nearest target point of q under the key (d, j): idx and dist as pn_knn3_query_f32 writes them for k = 1.
static void rrh_nearest(const float* R, int n, const RrhGrid& s, const float* q, int32_t* idx, float* dist) {
  if (s.flagged || !kg_finite(q[0]) || !kg_finite(q[1]) || !kg_finite(q[2])) {
    *idx = -1, *dist = (float)ol_nan();
    return;
  }
  if (n == 0) {
    *idx = -1, *dist = kg_inf();
    return;
  }
  const KgGrid& g = s.g;
  int c[3];
  for (int a = 0; a < 3; ++a) c[a] = kg_cell(g, a, q[a]);
  bool have = false;
  std::pair<float, int> best(0.0f, -1);
  const int rmax = std::max(g.dim[0], std::max(g.dim[1], g.dim[2]));
  for (int r = 0; r <= rmax; ++r) {
    for (int z = std::max(c[2] - r, 0); z <= std::min(c[2] + r, g.dim[2] - 1); ++z)
      for (int y = std::max(c[1] - r, 0); y <= std::min(c[1] + r, g.dim[1] - 1); ++y)
        for (int x = std::max(c[0] - r, 0); x <= std::min(c[0] + r, g.dim[0] - 1); ++x) {
          if (std::max(std::abs(x - c[0]), std::max(std::abs(y - c[1]), std::abs(z - c[2]))) != r) continue;
          const int cell = kg_cell_index(g, x, y, z);
          for (int t = s.start[cell]; t < s.start[cell + 1]; ++t) {
            const int j = s.order[t];
            const std::pair<float, int> key(kg_dist(q[0], q[1], q[2], R[3 * j], R[3 * j + 1], R[3 * j + 2]), j);
            if (!have || key < best) best = key, have = true;
          }
        }
    if (kg_covers(g, c, r)) break;
    if (have && best.first < kg_bound(g, c, r, q)) break;
  }
  *idx = have ? best.second : -1;
  *dist = have ? (float)sqrt((double)best.first) : kg_inf();
}

// ---- the sums ------------------------------------------------------------------------------------------------------------
static double rrh_tile_sum(const double* v) {
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

struct RrhSegment {
  const float *src, *tgt, *normals;
  int ns, nt, mode;
  float max_dist;
  std::vector<float> moved, dist;
  std::vector<int32_t> idx;
};

static void rrh_move_pair(RrhSegment& g, const RrhGrid& grid, const RrState& st) {
  double R[9];
  rr_rotation(st.q, R);
  for (int i = 0; i < g.ns; ++i) {
    rr_move(R, st.t, g.src + 3 * i, &g.moved[3 * i]);
    rrh_nearest(g.tgt, g.nt, grid, &g.moved[3 * i], &g.idx[i], &g.dist[i]);
  }
}

static int rrh_accepted(const RrhSegment& g, int i) {
  const int j = g.idx[i];
  return rr_accept(j, g.dist[i], g.max_dist, g.mode == RR_PLANE && j >= 0 ? g.normals + 3 * j : nullptr);
}

// K sums of stage 0 (means), 1 (centred) or 2 (residuals) over the segment, and the accepted pairs.
static int rrh_sums(const RrhSegment& g, int stage, const double* mean, int order, double* out) {
  const int K = stage == 0 ? RR_SUMS_MEAN : stage == 1 ? rr_second_sums(g.mode) : 1;
  const int tiles = ol_cloud_tiles(g.ns);
  std::vector<double> part((size_t)K * std::max(tiles, 1)), v((size_t)K * RR_TILE);
  std::vector<int> tcount(std::max(tiles, 1), 0);
  for (int c = 0, b = order ? tiles - 1 : 0; c < tiles; ++c, b += order ? -1 : 1) {
    std::fill(v.begin(), v.end(), 0.0);                                    // a rejected or absent point enters as 0.0
    for (int i = b * RR_TILE; i < std::min(g.ns, (b + 1) * RR_TILE); ++i) {
      if (!rrh_accepted(g, i)) continue;
      ++tcount[b];
      double term[RR_MAX_SUMS];
      const float *p = &g.moved[3 * i], *q = g.tgt + 3 * g.idx[i];
      if (stage == 0) rr_mean_terms(p, q, term);
      else if (stage == 2) term[0] = rr_residual_term(g.dist[i]);
      else if (g.mode == RR_PLANE) rr_plane_terms(p, q, g.normals + 3 * g.idx[i], mean, term);
      else rr_point_terms(p, q, mean, term);
      for (int k = 0; k < K; ++k) v[(size_t)k * RR_TILE + (i - b * RR_TILE)] = term[k];
    }
    for (int k = 0; k < K; ++k) part[(size_t)k * tiles + b] = rrh_tile_sum(&v[(size_t)k * RR_TILE]);
  }
  int m = 0;
  for (int c = 0, b = order ? tiles - 1 : 0; c < tiles; ++c, b += order ? -1 : 1) m += tcount[b];
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
    for (int b = 0; b < tiles; ++b) s = ol_add(s, part[(size_t)k * tiles + b]);
    out[k] = s;
  }
  return m;
}

extern "C" {

// A ragged batch.  normals, init (S,16), idx and dist may be null.  Returns rr_launches(max_iter).
int rrh_register(const float* src, const int* off_s, const float* tgt, const int* off_t, const float* normals, int S,
                 int mode, float max_dist, int max_iter, double tol_rot, double tol_trans, const double* init,
                 int sweeps, int order, int ppc, double* transform, int32_t* iterations, int32_t* status, int32_t* count,
                 double* rmse, int32_t* idx, float* dist) {
  for (int s = 0; s < S; ++s) {
    RrhSegment g;
    g.ns = off_s[s + 1] - off_s[s], g.nt = off_t[s + 1] - off_t[s], g.mode = mode, g.max_dist = max_dist;
    g.src = src + 3 * (size_t)off_s[s], g.tgt = tgt + 3 * (size_t)off_t[s];
    g.normals = normals ? normals + 3 * (size_t)off_t[s] : nullptr;
    g.moved.assign(3 * (size_t)g.ns + 1, 0.0f), g.dist.assign(g.ns + 1, 0.0f), g.idx.assign(g.ns + 1, 0);
    const RrhGrid grid = rrh_build(g.tgt, g.nt, ppc);
    RrState st = init ? rr_from_matrix(init + 16 * (size_t)s) : rr_identity();
    int stop = RR_RUNNING, its = 0;
    for (int it = 1; it <= max_iter && stop == RR_RUNNING; ++it) {
      rrh_move_pair(g, grid, st);
      double sums[RR_MAX_SUMS], mean[RR_SUMS_MEAN];
      const int m = rrh_sums(g, 0, nullptr, order, sums);
      for (int k = 0; k < RR_SUMS_MEAN; ++k) mean[k] = rr_mean(sums[k], m);
      rrh_sums(g, 1, mean, order, sums);
      stop = rr_step(mode, grid.flagged, m, mean, sums, tol_rot, tol_trans, sweeps, &st);
      its = it;
    }
    rrh_move_pair(g, grid, st);
    double res = 0.0;
    const int m = rrh_sums(g, 2, nullptr, order, &res);
    rr_matrix(st, transform + 16 * (size_t)s);
    iterations[s] = its;
    status[s] = stop == RR_RUNNING ? RR_MAX_ITER : stop;
    count[s] = m;
    rmse[s] = rr_rmse(res, m);
    for (int i = 0; i < g.ns; ++i) {
      if (idx) idx[off_s[s] + i] = g.idx[i];
      if (dist) dist[off_s[s] + i] = g.dist[i];
    }
  }
  return rr_launches(max_iter);
}

// The move step alone: T (S,16).
void rrh_apply(const float* src, const int* off_s, int S, const double* T, float* out) {
  for (int s = 0; s < S; ++s) {
    const RrState st = rr_from_matrix(T + 16 * (size_t)s);
    double R[9];
    rr_rotation(st.q, R);
    for (int i = off_s[s]; i < off_s[s + 1]; ++i) rr_move(R, st.t, src + 3 * (size_t)i, out + 3 * (size_t)i);
  }
}

int rrh_launches(int max_iter) { return rr_launches(max_iter); }
int rrh_constant(int which) {
  const int c[] = {RR_TILE, RR_SWEEPS, RR_MAX_ITERATIONS, RR_CONVERGED, RR_MAX_ITER, RR_TOO_FEW, RR_DEGENERATE, RR_NON_FINITE};
  return which >= 0 && which < 8 ? c[which] : -1;
}
double rrh_pivot(void) { return RR_PIVOT; }

}  // extern "C"

// ---- the program ------------------------------------------------------------------------------------------------------
struct RrhOut {
  std::vector<double> transform, rmse;
  std::vector<int32_t> iterations, status, count, idx;
  std::vector<float> dist;
};

static int rrh_fail(FILE* f, const char* what) {
  fprintf(stderr, "register_host: %s\n", what);
  fclose(f);
  return 2;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "register_host: a file of cases\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    fprintf(stderr, "register_host: cannot open %s\n", argv[1]);
    return 2;
  }
  int S = 0, mode = 0, max_iter = 0, has_normals = 0, has_init = 0, got = 0, rc = 0;
  float max_dist = 0.0f;
  double tol_rot = 0.0, tol_trans = 0.0;
  while ((got = fscanf(f, "%d %d %f %d %lf %lf %d %d", &S, &mode, &max_dist, &max_iter, &tol_rot, &tol_trans, &has_normals,
                       &has_init)) == 8) {
    if (S < 0 || S > 64 || mode < 0 || mode > 1 || max_iter < 1 || max_iter > RR_MAX_ITERATIONS || (mode == 1 && !has_normals))
      return rrh_fail(f, "expected `S mode max_dist max_iter tol_rot tol_trans has_normals has_init`");
    std::vector<int> off_s(S + 1, 0), off_t(S + 1, 0);
    std::vector<float> src, tgt, nrm;
    std::vector<double> init;
    for (int s = 0; s < S; ++s) {
      int ns = 0, nt = 0;
      if (fscanf(f, "%d %d", &ns, &nt) != 2 || ns < 0 || nt < 0 || ns > (1 << 20) || nt > (1 << 20))
        return rrh_fail(f, "expected `ns nt`");
      off_s[s + 1] = off_s[s] + ns, off_t[s + 1] = off_t[s] + nt;
      for (int k = 0; k < 16 * has_init; ++k) {
        double x;
        if (fscanf(f, "%lf", &x) != 1) return rrh_fail(f, "init is short");
        init.push_back(x);
      }
      for (int i = 0; i < 3 * ns; ++i) {
        float x;
        if (fscanf(f, "%f", &x) != 1) return rrh_fail(f, "the source is short");
        src.push_back(x);
      }
      for (int i = 0; i < nt; ++i)
        for (int k = 0; k < (has_normals ? 6 : 3); ++k) {
          float x;
          if (fscanf(f, "%f", &x) != 1) return rrh_fail(f, "the target is short");
          (k < 3 ? tgt : nrm).push_back(x);
        }
    }
    src.push_back(0.0f), tgt.push_back(0.0f), nrm.push_back(0.0f), init.push_back(0.0);
    RrhOut o[2];
    for (int order = 0; order < 2; ++order) {
      RrhOut& r = o[order];
      r.transform.assign(16 * (size_t)S + 1, -9.0), r.rmse.assign(S + 1, -9.0);
      r.iterations.assign(S + 1, -9), r.status.assign(S + 1, -9), r.count.assign(S + 1, -9);
      r.idx.assign(off_s[S] + 1, -9), r.dist.assign(off_s[S] + 1, -9.0f);
      rrh_register(src.data(), off_s.data(), tgt.data(), off_t.data(), has_normals ? nrm.data() : nullptr, S, mode,
                   max_dist, max_iter, tol_rot, tol_trans, has_init ? init.data() : nullptr, RR_SWEEPS, order, KG_PPC,
                   r.transform.data(), r.iterations.data(), r.status.data(), r.count.data(), r.rmse.data(), r.idx.data(),
                   r.dist.data());
    }
    if (memcmp(o[0].transform.data(), o[1].transform.data(), o[0].transform.size() * 8) ||
        memcmp(o[0].rmse.data(), o[1].rmse.data(), o[0].rmse.size() * 8) || o[0].iterations != o[1].iterations ||
        o[0].status != o[1].status || o[0].count != o[1].count || o[0].idx != o[1].idx ||
        memcmp(o[0].dist.data(), o[1].dist.data(), o[0].dist.size() * 4))
      rc = 1;
    if (o[0].idx[off_s[S]] != -9 || o[0].dist[off_s[S]] != -9.0f || o[0].count[S] != -9) rc = 1;      // nothing behind
    for (int s = 0; s < S; ++s) {
      for (int k = 0; k < 16; ++k) printf("%.17g ", o[0].transform[16 * s + k]);
      printf("\n%d %d %d %.17g\n", o[0].iterations[s], o[0].status[s], o[0].count[s], o[0].rmse[s]);
      for (int i = off_s[s]; i < off_s[s + 1]; ++i) printf("%d %.9g\n", o[0].idx[i], o[0].dist[i]);
    }
  }
  fclose(f);
  if (got != EOF) {
    fprintf(stderr, "register_host: expected `S mode max_dist max_iter tol_rot tol_trans has_normals has_init`\n");
    return 2;
  }
  return rc;
}
