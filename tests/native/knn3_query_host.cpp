// Test-only host harness around parsenet_codebase_amd/csrc/knn3_grid_math.h and knn_lift_math.h (the definitions
// knn3_query.hip and knn_lift.hip implement): the WHOLE cross-cloud query restated serially — bounding box and flag of
// the reference, its grid, the counting sort into cell order, the query's cell in that grid (clamped when the query is
// outside), rings, the termination bound, selection by (d, j), padding — and the two lifting rules, so that
// tests/test_knn3_query_abi.py can hold them against brute force without a GPU.  Not part of the product.
//
// As a shared object it exports the kqh_* functions below.  As a program (it has a main) it reads one pair of clouds
// as text from the file named by its first argument, or from stdin:
//     nr nq k ppc                  the reference points, the queries, the neighbours, the points per cell
//     nr lines  x y z              the reference
//     nq lines  x y z              the queries
// runs the query and both lifting rules (values = the reference's x, labels = j % 3) and prints one line per query:
// k indices, the interpolated value as the integer image of its bits, the voted label.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../parsenet_codebase_amd/csrc/knn3_grid_math.h"
#include "../../parsenet_codebase_amd/csrc/knn_lift_math.h"

struct KqhGrid {
  KgGrid g;
  bool flagged;
  std::vector<int> start;      // (cells + 1) first record of every cell
  std::vector<int> order;      // records: the reference points in cell order (stable)
};

static KqhGrid kqh_build(const float* R, int n, int ppc) {
  KqhGrid s;
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

typedef std::pair<float, int> KqhKey;      // (d, j): the order of the neighbours

// One query q against the grid of R: its k best in ``best`` (sorted), the ring it stopped at as the return value.
static int kqh_one(const float* R, const KqhGrid& s, const float* q, int k, std::vector<KqhKey>& best) {
  const KgGrid& g = s.g;
  int c[3];
  for (int a = 0; a < 3; ++a) c[a] = kg_cell(g, a, q[a]);      // clamped into a border cell when q is outside
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
            best.push_back(KqhKey(kg_dist(q[0], q[1], q[2], R[3 * j], R[3 * j + 1], R[3 * j + 2]), j));
          }
        }
    std::sort(best.begin(), best.end());
    if ((int)best.size() > k) best.resize(k);
    if (kg_covers(g, c, r)) return r;
    // (never on "k held" while the reference has fewer than k points: then best.size() stays below k)
    if ((int)best.size() == k && best[k - 1].first < kg_bound(g, c, r, q)) return r;
  }
  return -1;      // not reached: the cube of ring rmax covers the grid
}

extern "C" {

// The query of one segment: idx (nq,k), dist (nq,k) or null, ring (nq) or null: the ring every query stopped at
// (-1 for a row that is not searched).
int kqh_query(const float* R, int nr, const float* Q, int nq, int k, int ppc, int32_t* idx, float* dist, int32_t* ring) {
  if (nr < 0 || nq < 0 || k < KG_MIN_K || k > KG_MAX_K) return -1;
  const KqhGrid s = kqh_build(R, nr, ppc);
  std::vector<KqhKey> best;
  for (int i = 0; i < nq; ++i) {
    const float* q = Q + 3 * i;
    const bool nan_row = s.flagged || !kg_finite(q[0]) || !kg_finite(q[1]) || !kg_finite(q[2]);
    best.clear();
    int r = -1;
    if (!nan_row && nr > 0) {
      r = kqh_one(R, s, q, k, best);
      if (r < 0) return -2;
    }
    if (ring) ring[i] = r;
    for (int t = 0; t < k; ++t) {
      const bool have = t < (int)best.size();
      idx[(size_t)i * k + t] = have ? best[t].second : -1;
      if (dist) dist[(size_t)i * k + t] = nan_row ? kl_nan() : have ? (float)sqrt((double)best[t].first) : kg_inf();
    }
  }
  return 0;
}

// The bound's property for queries that are not points of the grid's cloud: over every query and every ring before
// the cube covers the grid, the number of reference points outside the cube with fp32 d < b(r).  It must be 0.
// ``finite`` counts the (query, ring) pairs whose bound is positive and finite.
long long kqh_bound_violations(const float* R, int nr, const float* Q, int nq, int ppc, long long* finite) {
  const KqhGrid s = kqh_build(R, nr, ppc);
  *finite = 0;
  if (s.flagged || nr == 0) return 0;
  long long bad = 0;
  const int rmax = std::max(s.g.dim[0], std::max(s.g.dim[1], s.g.dim[2]));
  for (int i = 0; i < nq; ++i) {
    const float* q = Q + 3 * i;
    int c[3];
    for (int a = 0; a < 3; ++a) c[a] = kg_cell(s.g, a, q[a]);
    for (int r = 0; r <= rmax && !kg_covers(s.g, c, r); ++r) {
      const float b = kg_bound(s.g, c, r, q);
      if (b > 0.0f && kg_finite(b)) ++*finite;
      for (int j = 0; j < nr; ++j) {
        int cj[3];
        for (int a = 0; a < 3; ++a) cj[a] = kg_cell(s.g, a, R[3 * j + a]);
        if (std::max(std::abs(cj[0] - c[0]), std::max(std::abs(cj[1] - c[1]), std::abs(cj[2] - c[2]))) <= r) continue;
        if (kg_dist(q[0], q[1], q[2], R[3 * j], R[3 * j + 1], R[3 * j + 2]) < b) ++bad;
      }
    }
  }
  return bad;
}

// The two lifting rules over nq rows of one segment of n reference points.
void kqh_interpolate(const float* values, int n, int C, const int32_t* idx, const float* dist, int nq, int k, float* out) {
  for (int i = 0; i < nq; ++i)
    for (int c = 0; c < C; ++c)
      out[(size_t)i * C + c] = kl_interpolate(values, C, c, idx + (size_t)i * k, dist + (size_t)i * k, k, n);
}

void kqh_vote(const int32_t* labels, int n, const int32_t* idx, int nq, int k, int32_t* out) {
  for (int i = 0; i < nq; ++i) out[i] = kl_vote(labels, idx + (size_t)i * k, k, n);
}

}  // extern "C"

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return 2;
  int nr, nq, k, ppc;
  if (fscanf(f, "%d %d %d %d", &nr, &nq, &k, &ppc) != 4 || nr < 0 || nq < 0 || k < KG_MIN_K || k > KG_MAX_K) return 2;
  std::vector<float> R((size_t)3 * nr), Q((size_t)3 * nq);
  for (size_t t = 0; t < R.size(); ++t)
    if (fscanf(f, "%f", &R[t]) != 1) return 2;
  for (size_t t = 0; t < Q.size(); ++t)
    if (fscanf(f, "%f", &Q[t]) != 1) return 2;
  if (f != stdin) fclose(f);
  std::vector<int32_t> idx((size_t)nq * k), labels(nr), vote(nq);
  std::vector<float> dist((size_t)nq * k), values(nr), out(nq);
  if (kqh_query(R.data(), nr, Q.data(), nq, k, ppc, idx.data(), dist.data(), nullptr) != 0) return 1;
  for (int j = 0; j < nr; ++j) {
    values[j] = R[3 * j];
    labels[j] = j % 3;
  }
  kqh_interpolate(values.data(), nr, 1, idx.data(), dist.data(), nq, k, out.data());
  kqh_vote(labels.data(), nr, idx.data(), nq, k, vote.data());
  for (int i = 0; i < nq; ++i) {
    for (int t = 0; t < k; ++t) printf("%d ", idx[(size_t)i * k + t]);
    printf("%u %d\n", kg_bits(out[i]), vote[i]);
  }
  return 0;
}
