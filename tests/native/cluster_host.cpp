// Test-only host simulation of the Euclidean cluster extraction (parsenet_codebase_amd/csrc/cluster.hip): the launches of
// its schedule run serially, one after the other, on the SAME definitions the kernels compile (csrc/cluster_math.h on
// csrc/knn3_grid_math.h): bounds, cells, scan, scatter, then per round offers (every record searches its ball ring by
// ring until cl_stop), hooks and cl_passes compress passes with the walk cap CL_WALK, then sizes, numbers and labels.
// The rounds and passes are exactly cl_rounds / cl_passes of the largest segment, the numbers pn_cluster_launches
// reports; the exit flags are the kernels'.  Inside a launch the elements are visited in ascending order or, with
// order = 1, in descending order: the ranks inside a cell, the arrival of the minima and the stale words of the
// in-place compress pass then come the other way round, which must not change a bit.  tests/test_cluster_abi.py holds
// the result against an independent numpy restatement in every bit and reads the report.  Not part of the product.
//
// report[0]  1 when the schedule sufficed: the last scheduled round found no entry, and after the passes of every round
//            every vertex pointed at a root (no cap was hit)
// report[1]  rounds in which a component found an entry (largest over the segments)   report[2]  cl_rounds(max_n)
// report[3]  the most compress passes that moved a word in one round                  report[4]  cl_passes(max_n)
// report[5]  the most rings one query looked at          report[6]  the largest depth met before the passes of a round
// report[7]  the cells of the last searched segment's grid
//
// As a program (it has a main): without an argument it runs its own list of clouds in both orders against a brute-force
// union-find and prints "<cases> cases, <d> differences" (exit 1 when d > 0); with a file of clouds, each `n r min_size`
// + n lines `x y z`, it runs every cloud in both orders and prints ncomp and the n labels of each (exit 1 when the
// orders differ or the schedule did not suffice).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../parsenet_codebase_amd/csrc/cluster_math.h"
#include "../../parsenet_codebase_amd/csrc/ragged.h"

struct ClhRec {
  float x, y, z;
  int j;
};

// The order-preserving integer image of common.h, by which the kernels take the bounds: -0 lies below +0.
static uint32_t clh_ord(float f) {
  const uint32_t u = kg_bits(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static float clh_unord(uint32_t o) { return kg_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

static int clh_depth(const std::vector<uint32_t>& P, const std::vector<uint32_t>& H, uint32_t v, int first, int cap) {
  int d = 0;
  uint32_t x = v;
  while (d <= cap) {
    const uint32_t p = cl_word(P.data(), H.data(), x, first);
    if (p == x) return d;
    x = p, ++d;
  }
  return d;                                                            // a cycle: above every bound
}

// One valid segment.  Returns 1 when the schedule sufficed.
static int clh_segment(const float* pts, int n, float rad, int min_size, int rounds, int passes, int order,
                       int32_t* label, int32_t* ncomp, int32_t* count, int32_t* first_out, int32_t* ndrop,
                       int* report) {
  const int v0 = order ? n - 1 : 0, dv = order ? -1 : 1;
  // bounds
  uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u}, bad = 0u;
  for (int c = 0, i = v0; c < n; ++c, i += dv)
    for (int a = 0; a < 3; ++a) {
      const float x = pts[3 * i + a];
      bad |= kg_finite(x) ? 0u : 1u;
      mn[a] = std::min(mn[a], clh_ord(x));
      mx[a] = std::max(mx[a], clh_ord(x));
    }
  const int status = cl_status(bad, rad);
  if (status != 0 || n == 0) {
    for (int i = 0; i < n; ++i) {
      label[i] = -1;
      if (count) count[i] = -1;
      if (first_out) first_out[i] = -1;
    }
    *ncomp = n == 0 && status == 0 ? 0 : status;
    if (ndrop) *ndrop = n;
    return 1;
  }
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) lo[a] = clh_unord(mn[a]), hi[a] = clh_unord(mx[a]);
  const KgGrid g = cl_grid(n, lo, hi, rad);
  const float r2 = cl_r2(rad);
  const int ncell = kg_cells(g);
  report[7] = ncell;
  if (ncell > std::max(1, n)) return 0;
  // cells, scan, scatter
  std::vector<int> start(ncell + 1, 0), pcell(n), prank(n);
  for (int c = 0, i = v0; c < n; ++c, i += dv) {
    pcell[i] = kg_cell_index(g, kg_cell(g, 0, pts[3 * i]), kg_cell(g, 1, pts[3 * i + 1]), kg_cell(g, 2, pts[3 * i + 2]));
    prank[i] = start[pcell[i]]++;
  }
  for (int c = 0, run = 0; c <= ncell; ++c) {
    const int v = c < ncell ? start[c] : 0;
    start[c] = run;
    run += v;
  }
  std::vector<ClhRec> rec(n);
  for (int i = 0; i < n; ++i) rec[start[pcell[i]] + prank[i]] = ClhRec{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], i};
  // rounds
  std::vector<uint32_t> P(n), H(n, CL_NO_HOOK);
  std::vector<unsigned long long> best(n, CL_NO_ENTRY);
  std::vector<int> any(rounds + 1, 0);
  for (int v = 0; v < n; ++v) P[v] = (uint32_t)v;
  const int rmax = std::max(g.dim[0], std::max(g.dim[1], g.dim[2]));
  int ok = 1, worked = 0;
  for (int r = 0; r < rounds; ++r) {
    if (r > 0 && !any[r - 1]) break;                                   // (the launches exit at the flag)
    for (int cnt = 0, p = v0; cnt < n; ++cnt, p += dv) {               // offers: one query per record
      const ClhRec me = rec[p];
      const uint32_t ci = P[me.j];
      const float q[3] = {me.x, me.y, me.z};
      int c[3];
      for (int a = 0; a < 3; ++a) c[a] = kg_cell(g, a, q[a]);
      unsigned long long key = CL_NO_ENTRY;
      int ring = 0;
      for (; ring <= rmax; ++ring) {
        for (int z = std::max(c[2] - ring, 0); z <= std::min(c[2] + ring, g.dim[2] - 1); ++z)
          for (int y = std::max(c[1] - ring, 0); y <= std::min(c[1] + ring, g.dim[1] - 1); ++y)
            for (int x = std::max(c[0] - ring, 0); x <= std::min(c[0] + ring, g.dim[0] - 1); ++x) {
              if (std::max(abs(x - c[0]), std::max(abs(y - c[1]), abs(z - c[2]))) != ring) continue;      // the shell
              const int cell = kg_cell_index(g, x, y, z);
              for (int t = start[cell]; t < start[cell + 1]; ++t) {
                const ClhRec o = rec[t];
                if (o.j == me.j || !cl_is_edge(kg_dist(q[0], q[1], q[2], o.x, o.y, o.z), r2)) continue;
                if (P[o.j] == ci) continue;
                key = std::min(key, cl_key((uint32_t)me.j, (uint32_t)o.j));
              }
            }
        if (cl_stop(g, c, ring, q, r2)) break;
      }
      report[5] = std::max(report[5], ring + 1);
      if (key < best[ci]) best[ci] = key;
    }
    for (int c = 0, v = v0; c < n; ++c, v += dv) {                     // hooks: reads only, the word goes to H
      H[v] = CL_NO_HOOK;
      if (P[v] == (uint32_t)v) H[v] = cl_hook(P.data(), best.data(), n, (uint32_t)v, &any[r]);
    }
    if (!any[r]) break;
    ++worked;
    for (int v = 0; v < n; ++v) report[6] = std::max(report[6], clh_depth(P, H, (uint32_t)v, 1, n));
    int changed = 1, used = 0;
    for (int p = 0; p < passes && changed; ++p) {                      // compress passes, in place
      changed = 0;
      for (int c = 0, v = v0; c < n; ++c, v += dv) {
        const uint32_t now = cl_walk(P.data(), H.data(), n, (uint32_t)v, p == 0);
        if (now != P[v]) P[v] = now, changed = 1;
        if (p == 0) best[v] = CL_NO_ENTRY;
      }
      used += changed;
    }
    report[3] = std::max(report[3], used);
    for (int v = 0; v < n; ++v)
      if (clh_depth(P, H, (uint32_t)v, 0, n) > 1) ok = 0;              // the passes did not reach the roots
  }
  if (any[rounds - 1]) ok = 0;                                         // the last scheduled round still found an entry
  report[1] = std::max(report[1], worked);
  // sizes
  std::vector<uint32_t> cnt(n, 0u), first(n, 0xffffffffu);
  for (int c = 0, i = v0; c < n; ++c, i += dv) {
    cnt[P[i]] += 1u;
    first[P[i]] = std::min(first[P[i]], (uint32_t)i);
  }
  // numbers: the kept heads in ascending order
  int C = 0, points = 0;
  for (int i = 0; i < n; ++i) {
    const uint32_t root = P[i];
    if (first[root] != (uint32_t)i) continue;
    if (cl_kept(cnt[root], min_size)) {
      label[i] = C;
      if (count) count[C] = (int32_t)cnt[root];
      if (first_out) first_out[C] = i;
      points += (int)cnt[root];
      ++C;
    } else {
      label[i] = -1;
    }
  }
  for (int i = C; i < n; ++i) {
    if (count) count[i] = -1;
    if (first_out) first_out[i] = -1;
  }
  *ncomp = C;
  if (ndrop) *ndrop = n - points;
  // labels: every other point takes the label of its head
  for (int c = 0, i = v0; c < n; ++c, i += dv) {
    const uint32_t root = P[i], f = first[root];
    if (f == (uint32_t)i) continue;
    label[i] = cl_kept(cnt[root], min_size) ? label[f] : -1;
  }
  return ok;
}

// A ragged batch: pts (total,3), off (S+1), radius (S); count, first_out (total) and ndrop (S) may be null; report: 8
// ints (above).  Returns cl_launches of the largest segment.
extern "C" int clh_cluster(const float* pts, const int* off, int S, int total, const float* radius, int min_size,
                           int order, int32_t* label, int32_t* ncomp, int32_t* count, int32_t* first_out, int32_t* ndrop,
                           int* report) {
  int max_n = 0;
  for (int s = 0; s < S; ++s) max_n = std::max(max_n, off[s + 1] - off[s]);
  const int rounds = cl_rounds(max_n), passes = cl_passes(max_n);
  for (int t = 0; t < 8; ++t) report[t] = 0;
  report[0] = 1, report[2] = rounds, report[4] = passes;
  for (int s = 0; s < S; ++s) {
    const int o0 = off[s], o1 = off[s + 1];
    if (!rg_valid_segment(o0, o1, total)) {
      ncomp[s] = 0;
      if (ndrop) ndrop[s] = 0;
      continue;
    }
    if (!clh_segment(pts + 3 * (size_t)o0, o1 - o0, radius[s], min_size, rounds, passes, order, label + o0, ncomp + s,
                     count ? count + o0 : nullptr, first_out ? first_out + o0 : nullptr, ndrop ? ndrop + s : nullptr,
                     report))
      report[0] = 0;
  }
  return cl_launches(max_n);
}

extern "C" int clh_rounds(int max_n) { return cl_rounds(max_n); }
extern "C" int clh_passes(int max_n) { return cl_passes(max_n); }
extern "C" int clh_launches(int max_n) { return cl_launches(max_n); }
extern "C" int clh_constant(int which) {
  const int c[] = {CL_WALK, CL_MAX_ROUNDS, CL_MAX_PASSES, CL_CTRL_WORDS, CL_CTRL_ANY, CL_CTRL_CHANGED};
  return which >= 0 && which < 6 ? c[which] : -1;
}
// The grid of a cloud: dim (3), and the cell edge; returns the cells.
extern "C" int clh_grid(const float* pts, int n, float rad, int* dim, float* h) {
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      lo[a] = i ? std::min(lo[a], pts[3 * i + a]) : pts[a];
      hi[a] = i ? std::max(hi[a], pts[3 * i + a]) : pts[a];
    }
  const KgGrid g = cl_grid(n, lo, hi, rad);
  for (int a = 0; a < 3; ++a) dim[a] = g.dim[a];
  *h = g.h;
  return kg_cells(g);
}

// ---- the program ------------------------------------------------------------------------------------------------------
static uint32_t clh_state = 12345u;
static float clh_uniform(void) {
  clh_state = clh_state * 1664525u + 1013904223u;
  return (float)(clh_state >> 8) / 8388608.0f - 1.0f;                  // [-1, 1)
}

static int clh_find(std::vector<int>& up, int x) {
  while (up[x] != x) x = up[x] = up[up[x]];
  return x;
}

// The definition by brute force: all pairs, a union-find, the numbering.
static void clh_brute(const std::vector<float>& P, int n, float rad, int min_size, std::vector<int32_t>& label,
                      int* ncomp) {
  label.assign(n, -1);
  uint32_t bad = 0u;
  for (int i = 0; i < 3 * n; ++i) bad |= kg_finite(P[i]) ? 0u : 1u;
  const int status = cl_status(bad, rad);
  if (status != 0) {
    *ncomp = status;
    return;
  }
  const float r2 = cl_r2(rad);
  std::vector<int> up(n), size(n, 0), number(n, -1);
  for (int i = 0; i < n; ++i) up[i] = i;
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (kg_dist(P[3 * i], P[3 * i + 1], P[3 * i + 2], P[3 * j], P[3 * j + 1], P[3 * j + 2]) <= r2) {
        const int a = clh_find(up, i), b = clh_find(up, j);
        if (a != b) up[std::max(a, b)] = std::min(a, b);
      }
  for (int i = 0; i < n; ++i) size[clh_find(up, i)] += 1;
  int C = 0;
  for (int i = 0; i < n; ++i) {
    const int root = clh_find(up, i);                                  // the lowest index of the component
    if (size[root] < min_size) continue;
    if (root == i) number[i] = C++;
    label[i] = number[root];
  }
  *ncomp = C;
}

static int clh_check(const std::vector<float>& P, int n, float rad, int min_size) {
  std::vector<int32_t> want;
  int wantC = 0, diff = 0;
  clh_brute(P, n, rad, min_size, want, &wantC);
  for (int order = 0; order < 2; ++order) {
    std::vector<int32_t> label(n + 1, -9), count(n + 1, -9), first(n + 1, -9);
    int32_t ncomp = -9, ndrop = -9;
    const int off[2] = {0, n};
    int report[8];
    clh_cluster(P.data(), off, 1, n, &rad, min_size, order, label.data(), &ncomp, count.data(), first.data(), &ndrop,
                report);
    diff += ncomp != wantC || !report[0];
    int dropped = 0;
    for (int i = 0; i < n; ++i) diff += label[i] != want[i], dropped += want[i] < 0;
    diff += ndrop != dropped;
    for (int c = 0; c < n; ++c) {
      if (c < wantC) {
        int size = 0;
        for (int i = 0; i < n; ++i) size += want[i] == c;
        diff += count[c] != size || first[c] < 0 || first[c] >= n || want[first[c]] != c;
      } else {
        diff += count[c] != -1 || first[c] != -1;
      }
    }
  }
  return diff;
}

int main(int argc, char** argv) {
  if (argc > 1) {
    FILE* f = fopen(argv[1], "r");
    if (!f) {
      fprintf(stderr, "cluster_host: cannot open %s\n", argv[1]);
      return 2;
    }
    int n = 0, min_size = 0, rc = 0, got = 0;
    float rad = 0.0f;
    while ((got = fscanf(f, "%d %f %d", &n, &rad, &min_size)) == 3) {      // one cloud after the other
      if (n < 0 || n > (1 << 20) || min_size < 1) {
        fprintf(stderr, "cluster_host: expected `n r min_size`\n");
        fclose(f);
        return 2;
      }
      std::vector<float> P(3 * (size_t)n + 1);
      for (int i = 0; i < n; ++i)
        if (fscanf(f, "%f %f %f", &P[3 * i], &P[3 * i + 1], &P[3 * i + 2]) != 3) {
          fprintf(stderr, "cluster_host: %d points announced, point %d is missing\n", n, i);
          fclose(f);
          return 2;
        }
      std::vector<int32_t> label(n + 1), other(n + 1);
      int32_t ncomp = 0, ncomp1 = 0;
      const int off[2] = {0, n};
      int report[8], report1[8];
      clh_cluster(P.data(), off, 1, n, &rad, min_size, 0, label.data(), &ncomp, nullptr, nullptr, nullptr, report);
      clh_cluster(P.data(), off, 1, n, &rad, min_size, 1, other.data(), &ncomp1, nullptr, nullptr, nullptr, report1);
      printf("%d\n", ncomp);
      for (int i = 0; i < n; ++i) printf("%d\n", label[i]);
      if (!report[0] || !report1[0] || ncomp != ncomp1 || !std::equal(label.begin(), label.end(), other.begin())) rc = 1;
    }
    fclose(f);
    if (got != EOF) {
      fprintf(stderr, "cluster_host: expected `n r min_size`\n");
      return 2;
    }
    return rc;
  }
  int cases = 0, diff = 0;
  const int sizes[] = {0, 1, 2, 3, 65, 700, 1025};
  const float radii[] = {1e-5f, 0.05f, 0.12f, 0.3f, 4.0f};
  for (int n : sizes)
    for (float rad : radii)
      for (int min_size : {1, 3}) {
        std::vector<float> P(3 * (size_t)n + 1);
        for (int i = 0; i < 3 * n; ++i) P[i] = clh_uniform();
        diff += clh_check(P, n, rad, min_size), ++cases;
      }
  {                                                                    // a chain in bit-reversed order: the deep forest
    const int n = 512;
    std::vector<float> P(3 * n, 0.0f);
    for (int i = 0; i < n; ++i) {
      int rev = 0;
      for (int b = 0; b < 9; ++b) rev |= ((i >> b) & 1) << (8 - b);
      P[3 * i] = 0.01f * (float)rev;
    }
    diff += clh_check(P, n, 0.011f, 1), ++cases;
    diff += clh_check(P, n, 0.0099f, 1), ++cases;
    P[3 * 77 + 1] = kg_inf();                                          // a non-finite coordinate
    diff += clh_check(P, n, 0.011f, 1), ++cases;
  }
  {                                                                    // a planar lattice, the radius exactly the spacing
    const int m = 20;
    std::vector<float> P;
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) P.push_back(0.25f * i), P.push_back(0.25f * j), P.push_back(1.0f);
    diff += clh_check(P, m * m, 0.25f, 1), ++cases;
    diff += clh_check(P, m * m, kg_prev(0.25f), 1), ++cases;
    for (float rad : {0.0f, -1.0f, 1e-30f, kg_inf(), kg_inf() - kg_inf()}) diff += clh_check(P, m * m, rad, 1), ++cases;
  }
  printf("%d cases, %d differences\n", cases, diff);
  return diff ? 1 : 0;
}
