// Test-only host harness around parsenet_codebase_amd/csrc/knn3_grid_math.h (the definition knn3_grid.hip implements):
// the WHOLE search restated serially — bounding box and flag, grid, cell function, counting sort into cell order, rings,
// the termination bound, selection by (d, j) — so that tests/test_knn3_grid_abi.py can hold it against brute force
// without a GPU, and check the two properties the exactness rests on directly.  Not part of the product.
//
// As a shared object it exports the kgh_* functions below.  As a program (it has a main) it reads one cloud as text
// from the file named by its first argument, or from stdin:
//     n k ppc                      the number of points, of neighbours, and the points per cell
//     n lines  x y z               the points
// and prints one line of k indices per point.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../parsenet_codebase_amd/csrc/knn3_grid_math.h"

struct KghSegment {
  KgGrid g;
  bool flagged;
  std::vector<int> cell;       // (n,3) cell of every point
  std::vector<int> start;      // (cells + 1) first record of every cell
  std::vector<int> order;      // records: the points in cell order (stable)
};

static KghSegment kgh_build(const float* P, int n, int ppc) {
  KghSegment s;
  s.flagged = false;
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const float x = P[3 * i + a];
      if (!kg_finite(x)) s.flagged = true;
      if (i == 0 || x < lo[a]) lo[a] = x;
      if (i == 0 || x > hi[a]) hi[a] = x;
    }
  if (s.flagged) return s;
  s.g = kg_grid(n, lo, hi, ppc);
  const int cells = kg_cells(s.g);
  s.cell.resize((size_t)3 * n);
  s.start.assign(cells + 1, 0);
  std::vector<int> of(n);
  for (int i = 0; i < n; ++i) {
    for (int a = 0; a < 3; ++a) s.cell[3 * i + a] = kg_cell(s.g, a, P[3 * i + a]);
    of[i] = kg_cell_index(s.g, s.cell[3 * i], s.cell[3 * i + 1], s.cell[3 * i + 2]);
    ++s.start[of[i] + 1];
  }
  for (int c = 0; c < cells; ++c) s.start[c + 1] += s.start[c];
  s.order.resize(n);
  std::vector<int> fill(s.start.begin(), s.start.end() - 1);
  for (int i = 0; i < n; ++i) s.order[fill[of[i]]++] = i;
  return s;
}

typedef std::pair<float, int> KghKey;      // (d, j): the order of the neighbours

// One query: its k best in ``best`` (sorted), the ring it stopped at as the return value.
static int kgh_query(const float* P, const KghSegment& s, int i, int k, std::vector<KghKey>& best) {
  const KgGrid& g = s.g;
  const float* q = P + 3 * i;
  const int* c = &s.cell[3 * i];
  best.clear();
  const int rmax = std::max(g.dim[0], std::max(g.dim[1], g.dim[2]));
  for (int r = 0; r <= rmax; ++r) {
    for (int z = std::max(c[2] - r, 0); z <= std::min(c[2] + r, g.dim[2] - 1); ++z)
      for (int y = std::max(c[1] - r, 0); y <= std::min(c[1] + r, g.dim[1] - 1); ++y)
        for (int x = std::max(c[0] - r, 0); x <= std::min(c[0] + r, g.dim[0] - 1); ++x) {
          if (std::max(std::abs(x - c[0]), std::max(std::abs(y - c[1]), std::abs(z - c[2]))) != r) continue;   // the shell
          const int cell = kg_cell_index(g, x, y, z);
          for (int t = s.start[cell]; t < s.start[cell + 1]; ++t) {
            const int j = s.order[t];
            best.push_back(KghKey(kg_dist(q[0], q[1], q[2], P[3 * j], P[3 * j + 1], P[3 * j + 2]), j));
          }
        }
    std::sort(best.begin(), best.end());
    if ((int)best.size() > k) best.resize(k);
    if (kg_covers(g, c, r)) return r;
    if ((int)best.size() == k && best[k - 1].first < kg_bound(g, c, r, q)) return r;
  }
  return -1;      // not reached: the cube of ring rmax covers the grid
}

extern "C" {

// The search of one segment: idx (n,k), dist (n,k) or null, ring (n) or null: the ring every query stopped at.
int kgh_search(const float* P, int n, int k, int ppc, int32_t* idx, float* dist, int32_t* ring) {
  if (n < 0 || k < KG_MIN_K || k > KG_MAX_K) return -1;
  const KghSegment s = kgh_build(P, n, ppc);
  std::vector<KghKey> best;
  for (int i = 0; i < n; ++i) {
    int r = 0;
    if (!s.flagged) r = kgh_query(P, s, i, k, best);
    if (r < 0) return -2;
    if (ring) ring[i] = r;
    for (int t = 0; t < k; ++t) {
      const bool have = !s.flagged && t < (int)best.size();
      idx[(size_t)i * k + t] = have ? best[t].second : i;
      if (dist) dist[(size_t)i * k + t] = s.flagged ? NAN : (float)sqrt((double)(have ? best[t].first : 0.0f));
    }
  }
  return 0;
}

// The grid of a segment: dim (3), cell (n,3), h; returns the number of cells, 0 for a flagged segment.
int kgh_cells(const float* P, int n, int ppc, int32_t* dim, int32_t* cell, float* h) {
  const KghSegment s = kgh_build(P, n, ppc);
  if (s.flagged) return 0;
  for (int a = 0; a < 3; ++a) dim[a] = s.g.dim[a];
  for (size_t t = 0; t < s.cell.size(); ++t) cell[t] = s.cell[t];
  *h = s.g.h;
  return kg_cells(s.g);
}

// The bound's property, directly: over every query and every ring before the cube covers the grid, the number of
// points outside the cube with fp32 d < b(r).  It must be 0.  ``finite`` counts the (query, ring) pairs whose bound is
// positive and finite, so that the caller sees the check was not vacuous.
long long kgh_bound_violations(const float* P, int n, int ppc, long long* finite) {
  const KghSegment s = kgh_build(P, n, ppc);
  *finite = 0;
  if (s.flagged) return 0;
  long long bad = 0;
  const int rmax = std::max(s.g.dim[0], std::max(s.g.dim[1], s.g.dim[2]));
  for (int i = 0; i < n; ++i) {
    const float* q = P + 3 * i;
    const int* c = &s.cell[3 * i];
    for (int r = 0; r <= rmax && !kg_covers(s.g, c, r); ++r) {
      const float b = kg_bound(s.g, c, r, q);
      if (b > 0.0f && kg_finite(b)) ++*finite;
      for (int j = 0; j < n; ++j) {
        const int* cj = &s.cell[3 * j];
        if (std::max(std::abs(cj[0] - c[0]), std::max(std::abs(cj[1] - c[1]), std::abs(cj[2] - c[2]))) <= r) continue;
        if (kg_dist(q[0], q[1], q[2], P[3 * j], P[3 * j + 1], P[3 * j + 2]) < b) ++bad;
      }
    }
  }
  return bad;
}

int kgh_resolution(int n, int ppc) { return kg_resolution(n, ppc); }
int kgh_default_ppc(void) { return KG_PPC; }

}  // extern "C"

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return 2;
  int n, k, ppc;
  if (fscanf(f, "%d %d %d", &n, &k, &ppc) != 3 || n < 0 || k < KG_MIN_K || k > KG_MAX_K) return 2;
  std::vector<float> P((size_t)3 * n);
  for (size_t t = 0; t < P.size(); ++t)
    if (fscanf(f, "%f", &P[t]) != 1) return 2;
  std::vector<int32_t> idx((size_t)n * k);
  if (kgh_search(P.data(), n, k, ppc, idx.data(), nullptr, nullptr) != 0) return 1;
  for (int i = 0; i < n; ++i) {
    for (int t = 0; t < k; ++t) printf(t ? " %d" : "%d", idx[(size_t)i * k + t]);
    printf("\n");
  }
  return 0;
}
