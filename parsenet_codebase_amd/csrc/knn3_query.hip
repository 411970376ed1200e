// Exact k nearest neighbours ACROSS two clouds, for a ragged batch of (reference, query) pairs of any size: segment s
// of the queries is searched in segment s of the reference.  The grid, its cell function, the rings and the termination
// bound are those of knn3_grid_math.h as they stand, and the build phases, the workspace of the grid and the ring loop
// are those of knn3_grid.hip (knn3_grid_build.h): the grid is built on the REFERENCE, and a query starts in the cell
// kg_cell gives it in that grid — clamped into a border cell when it lies outside, which keeps the cell function
// monotone, all the bound relies on ("Neighbours across two clouds").
//
// Eight stream-ordered launches (pn_knn3_query_launches; four memsets on top), no cooperative launch, no grid-wide
// barrier, no host synchronisation:
//   1 - 4      bbox, cells, scan, scatter of the reference (knn3_grid_build.h)
//   5 qcells   the cell of every query in the reference's grid, the histogram of the queries over those cells and the
//              query's rank in its cell.  A row that is not searched is finished here: no valid segment, a non-finite
//              query or a flagged reference (-1 / NaN), an empty reference (-1 / +inf).
//   6 scan     the same scan kernel, on the queries' histogram, positions starting at the queries' offsets
//   7 qscatter the row of every binned query to start[cell] + rank: the queries in the cell order of the reference
//   8 search   one wave per position of that order, kg_ring_search, the row written to the query's ORIGINAL position.
//              Waves of a workgroup search from the same or neighbouring cells and read the same records.
// PN_KNN3_QUERY_BIN=0 (developer hook of tools/knn3_query_ab.py) skips 6 and 7 and searches the queries in the order
// they came; it moves the speed and no output.  profiles/knn3_query.txt holds the comparison: on shuffled tori the
// binning costs 2 - 18 % up to a reference of 10^5 points (its three launches, and the records sit in the cache
// anyway) and wins 1.5 times at 10^6 x 10^6 (4.74 against 7.07 ms), the size no other kernel serves: it stays.
//
// Workspace (pn_knn3_query_workspace_bytes): the grid's arrays over the reference (knn3_grid_build.h) | query order
// 4 totalQ (memset 0xff: an empty position) | query cell 4 totalQ | query rank 4 totalQ | query cell starts
// 4 (totalR + 2 S), laid out like the grid's (memset 0).
//
// Resource report of hipcc --offload-arch=gfx950 -O3 (-Rpass-analysis=kernel-resource-usage):
//   pn_knn3_query_search_kernel  VGPRs: 67  TotalSGPRs: 91  ScratchSize [bytes/lane]: 0  Occupancy [waves/SIMD]: 7
//                                LDS Size [bytes/block]: 0 — no spill
//   qcells 29 / qscatter 14 VGPRs, ScratchSize 0 for both, 8 waves/SIMD; bbox, cells, scan, scatter as in knn3_grid.hip
#include "knn3_grid_build.h"

struct KqWs {
  KgWs g;           // the grid of the reference
  int* qord;        // (totalQ) the rows of the binned queries in cell order, -1 where a position is empty
  int* qcell;       // (totalQ) the query's cell in the reference's grid, -1: not searched
  int* qrank;       // (totalQ)
  int* qstart;      // (totalR + 2 S) histogram of the queries over the reference's cells, then starts
};

static long long kq_carve(void* base, long long totalR, long long totalQ, long long S, KqWs* w) {
  RgCarver c = {(uintptr_t)base, 0};
  kg_take(c, totalR, S, &w->g);
  w->qord = c.take<int>(totalQ);
  w->qcell = c.take<int>(totalQ);
  w->qrank = c.take<int>(totalQ);
  w->qstart = c.take<int>(totalR + 2 * S);
  return c.bytes;
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

// ---- 5: the cell of every query in the reference's grid; the rows that are not searched ---------------------------------
__global__ __launch_bounds__(256) void pn_knn3_query_cells_kernel(const float* __restrict__ qry,
                                                                  const int* __restrict__ off_r,
                                                                  const int* __restrict__ off_q, int S, int totalR,
                                                                  int totalQ, int k, int ppc, int bin, KqWs w,
                                                                  int* __restrict__ idx, float* __restrict__ dist) {
  const long long row64 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row64 >= totalQ) return;
  const int row = (int)row64;
  const float q[3] = {qry[(size_t)row * 3], qry[(size_t)row * 3 + 1], qry[(size_t)row * 3 + 2]};
  const KqRow r = kq_row(off_r, off_q, S, totalR, totalQ, w.g, row, q);
  w.qcell[row] = -1;
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
                                                                    KqWs w) {
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
                                                                   int* __restrict__ idx, float* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const long long p64 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p64 >= totalQ) return;
  const int row = w.qord[(int)p64];
  if ((unsigned)row >= (unsigned)totalQ) return;      // an empty position: the row was finished by the cells kernel
  const float q[3] = {qry[(size_t)row * 3], qry[(size_t)row * 3 + 1], qry[(size_t)row * 3 + 2]};
  const KqRow r = kq_row(off_r, off_q, S, totalR, totalQ, w.g, row, q);
  if (r.state) return;                                // (cannot happen: such a row has no position)
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

// ---- host -------------------------------------------------------------------------------------------------------------------
extern "C" int pn_knn3_query_launches(void) { return 8; }

extern "C" long long pn_knn3_query_workspace_bytes(long long totalR, long long totalQ, int S) {
  if (totalR < 0 || totalQ < 0 || S < 0) return 0;
  KqWs w;
  return kq_carve(nullptr, totalR, totalQ, S, &w) + 16;
}

// PN_KNN3_QUERY_BIN: developer hook of tools/knn3_query_ab.py — 0 searches the queries in the order they came.
static int kq_bin(void) {
  const char* e = getenv("PN_KNN3_QUERY_BIN");
  return !(e && e[0] == '0' && e[1] == 0);
}

extern "C" int pn_knn3_query_f32(const float* ref, const int* off_r, int totalR, const float* qry, const int* off_q,
                                 int totalQ, int S, int k, int32_t* idx, float* dist, void* ws, long long ws_bytes,
                                 void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PN_CHECK_ARG(k >= KG_MIN_K && k <= KG_MAX_K, "pn_knn3_query_f32: k=%d (%d <= k <= %d)", k, KG_MIN_K, KG_MAX_K);
  PN_CHECK_ARG(S >= 0 && totalR >= 0 && totalQ >= 0, "pn_knn3_query_f32: S=%d totalR=%d totalQ=%d", S, totalR, totalQ);
  PN_CHECK_ARG((long long)totalQ * k < (1ll << 31), "pn_knn3_query_f32: totalQ * k = %lld (below 2^31)",
               (long long)totalQ * k);
  if (totalQ == 0 || S == 0) return PN_OK;
  PN_CHECK_ARG((ref || totalR == 0) && off_r && qry && off_q && idx && ws, "pn_knn3_query_f32: null pointer");
  PN_CHECK_ARG(ws_bytes >= pn_knn3_query_workspace_bytes(totalR, totalQ, S),
               "pn_knn3_query_f32: workspace of %lld bytes (%lld)", ws_bytes,
               pn_knn3_query_workspace_bytes(totalR, totalQ, S));
  KqWs w;
  kq_carve((void*)pn_align_up((size_t)ws, 16), totalR, totalQ, S, &w);
  const int ppc = kg_ppc(), bin = kq_bin();
  if (totalR > 0) {
    const int rc = kg_build_launch(ref, off_r, S, totalR, ppc, w.g, stream);
    if (rc != PN_OK) return rc;
  } else {
    PN_CHECK_HIP(hipMemsetAsync(w.g.flag, 0, (size_t)4 * S, stream));      // the one array the fill launch reads
  }
  PN_CHECK_HIP(hipMemsetAsync(w.qord, 0xff, (size_t)4 * totalQ, stream));
  PN_CHECK_HIP(hipMemsetAsync(w.qstart, 0, (size_t)4 * ((size_t)totalR + 2 * (size_t)S), stream));
  const int row_blocks = pn_cdiv(totalQ, 256);
  {
    PN_PROF("knn3_query_cells", stream);
    hipLaunchKernelGGL(pn_knn3_query_cells_kernel, dim3(row_blocks), dim3(256), 0, stream, qry, off_r, off_q, S, totalR,
                       totalQ, k, ppc, bin, w, idx, dist);
  }
  if (totalR > 0 && bin) {
    {
      PN_PROF("knn3_query_scan", stream);
      hipLaunchKernelGGL(pn_knn3_grid_scan_kernel, dim3(S), dim3(1024), 0, stream, off_r, off_q, totalR, ppc, w.g,
                         w.qstart);
    }
    {
      PN_PROF("knn3_query_scatter", stream);
      hipLaunchKernelGGL(pn_knn3_query_scatter_kernel, dim3(row_blocks), dim3(256), 0, stream, off_r, off_q, S, totalQ,
                         w);
    }
  }
  if (totalR > 0) {
    PN_PROF("knn3_query_search", stream);
    hipLaunchKernelGGL(pn_knn3_query_search_kernel, dim3(pn_cdiv(totalQ, 4)), dim3(256), 0, stream, qry, off_r, off_q, S,
                       totalR, totalQ, k, ppc, w, idx, dist);
  }
  PN_CHECK_LAUNCH();
  return PN_OK;
}
