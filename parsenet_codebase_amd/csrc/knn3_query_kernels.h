// The cross-cloud search of knn3_query.hip as kernels that more than one translation unit compiles: the workspace of the
// query (the reference's grid, then the queries' cell order), the row rule, and the three launches that bin the queries
// into the reference's cells and search them — what knn3_query.hip (one search per call) and register.hip (one search
// per iteration on a grid built once) share, so that the two cannot drift apart; each translation unit that includes
// this header gets its own copy of the kernels (anonymous namespace), as with knn3_grid_build.h.
//
// `stop` (S) is null, or one word per segment: the rows of a segment whose word is not 0 take no position in the cell
// order, so the waves of the search exit at their empty positions, and keep what idx and dist held.  pn_knn3_query_f32 passes
// null; register.hip passes the stop flags of its segments.
#pragma once
#include "knn3_grid_build.h"

struct KqWs {
  KgWs g;           // the grid of the reference
  int* qord;        // (totalQ) the rows of the binned queries in cell order, -1 where a position is empty
  int* qcell;       // (totalQ) the query's cell in the reference's grid, -1: not searched
  int* qrank;       // (totalQ)
  int* qstart;      // (totalR + 2 S) histogram of the queries over the reference's cells, then starts
};

static inline long long kq_carve(void* base, long long totalR, long long totalQ, long long S, KqWs* w) {
  RgCarver c = {(uintptr_t)base, 0};
  kg_take(c, totalR, S, &w->g);
  w->qord = c.take<int>(totalQ);
  w->qcell = c.take<int>(totalQ);
  w->qrank = c.take<int>(totalQ);
  w->qstart = c.take<int>(totalR + 2 * S);
  return c.bytes;
}

// PN_KNN3_QUERY_BIN: developer hook of tools/knn3_query_ab.py — 0 searches the queries in the order they came.
static inline int kq_bin(void) {
  const char* e = getenv("PN_KNN3_QUERY_BIN");
  return !(e && e[0] == '0' && e[1] == 0);
}

// What a query row is: its segment and whether it is searched.
struct KqRow {
  int s, o0, o1;      // the segment and its REFERENCE rows [o0, o1)
  int state;          // 0: searched, 1: -1 / NaN, 2: -1 / +inf
};

__device__ static inline KqRow kq_row(const int* __restrict__ off_r, const int* __restrict__ off_q, int S, int totalR,
                                      int totalQ, const KgWs& g, int row, const float* q) {
  KqRow r;
  r.s = kg_segment(off_q, S, row);
  r.o0 = off_r[r.s];
  r.o1 = off_r[r.s + 1];
  const bool finite = kg_finite(q[0]) && kg_finite(q[1]) && kg_finite(q[2]);
  if (!rg_segment_holds(off_q[r.s], off_q[r.s + 1], totalQ, row) || !rg_valid_segment(r.o0, r.o1, totalR) || !finite ||
      g.flag[r.s])
    r.state = 1;
  else
    r.state = r.o1 == r.o0 ? 2 : 0;
  return r;
}

namespace {

// ---- 5: the cell of every query in the reference's grid; the rows that are not searched ---------------------------------
// STOPS: the caller has stop flags (false: the argument is not read, and the kernel is the one it was without it).
template <bool STOPS>
__global__ __launch_bounds__(256) void pn_knn3_query_cells_kernel(const float* __restrict__ qry,
                                                                  const int* __restrict__ off_r,
                                                                  const int* __restrict__ off_q, int S, int totalR,
                                                                  int totalQ, int k, int ppc, int bin, KqWs w,
                                                                  int* __restrict__ idx, float* __restrict__ dist,
                                                                  const uint32_t* __restrict__ stop) {
  const long long row64 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row64 >= totalQ) return;
  const int row = (int)row64;
  const float q[3] = {qry[(size_t)row * 3], qry[(size_t)row * 3 + 1], qry[(size_t)row * 3 + 2]};
  const KqRow r = kq_row(off_r, off_q, S, totalR, totalQ, w.g, row, q);
  w.qcell[row] = -1;
  if (STOPS && stop && stop[r.s]) return;      // a stopped segment: no position, and the row keeps what it held
  if (r.state) {
    const float fill = r.state == 1 ? __builtin_nanf("") : kg_inf();
    for (int t = 0; t < k; ++t) {
      idx[(size_t)row * k + t] = -1;
      if (dist) dist[(size_t)row * k + t] = fill;
    }
    return;
  }
  if (!bin) {
    w.qord[row] = row;
    return;
  }
  const KgGrid g = kg_segment_grid(w.g, r.s, r.o1 - r.o0, ppc);
  const int cell = kg_cell_index(g, kg_cell(g, 0, q[0]), kg_cell(g, 1, q[1]), kg_cell(g, 2, q[2]));
  w.qcell[row] = cell;
  w.qrank[row] = atomicAdd(&w.qstart[(size_t)r.o0 + 2 * (size_t)r.s + cell], 1);      // cell < max(1, n_r)
}

// ---- 7: the queries in the cell order of the reference --------------------------------------------------------------------
__global__ __launch_bounds__(256) void pn_knn3_query_scatter_kernel(const int* __restrict__ off_r,
                                                                    const int* __restrict__ off_q, int S, int totalQ,
                                                                    KqWs w) {      // (a stopped row has cell -1)
  const long long row64 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row64 >= totalQ) return;
  const int row = (int)row64;
  const int cell = w.qcell[row];
  if (cell < 0) return;
  const int s = kg_segment(off_q, S, row);
  const int pos = w.qstart[(size_t)off_r[s] + 2 * (size_t)s + cell] + w.qrank[row];
  if (pos < off_q[s] || pos >= off_q[s + 1] || pos >= totalQ) return;      // (cannot happen; never write out of the segment)
  w.qord[pos] = row;
}

// ---- 8: the search ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pn_knn3_query_search_kernel(const float* __restrict__ qry,
                                                                   const int* __restrict__ off_r,
                                                                   const int* __restrict__ off_q, int S, int totalR,
                                                                   int totalQ, int k, int ppc, KqWs w,
                                                                   int* __restrict__ idx, float* __restrict__ dist,
                                                                   const uint32_t* __restrict__ stop) {
  const int lane = threadIdx.x & 63;
  const long long p64 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p64 >= totalQ) return;
  const int row = w.qord[(int)p64];
  if ((unsigned)row >= (unsigned)totalQ) return;      // an empty position: the row was finished by the cells kernel
  const float q[3] = {qry[(size_t)row * 3], qry[(size_t)row * 3 + 1], qry[(size_t)row * 3 + 2]};
  const KqRow r = kq_row(off_r, off_q, S, totalR, totalQ, w.g, row, q);
  if (r.state) return;                                // (cannot happen: such a row has no position)
  if (stop && stop[r.s]) return;                      // (cannot happen either: a stopped row has no position)
  const int n = r.o1 - r.o0;
  const KgGrid g = kg_segment_grid(w.g, r.s, n, ppc);
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = kg_cell(g, a, q[a]);
  const u64 best = kg_ring_search(w.g, w.g.start + (size_t)r.o0 + 2 * (size_t)r.s, g, r.o0, r.o1, n, k, q, c);
  if (lane < k) {
    const size_t o = (size_t)row * k + lane;
    const bool have = best != 0ull;                   // fewer than k points in the reference: -1 / +inf from n_r on
    idx[o] = have ? (int)knn_key_index(best) : -1;
    if (dist) dist[o] = have ? kg_key_dist(best) : kg_inf();
  }
}

}  // namespace
