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
// The three kernels and the workspace live in knn3_query_kernels.h, which register.hip compiles too; they take a nullable
// stop-flag argument that this file passes as null (cells<false> does not read it).  The figures above are the same
// before and after that move: cells 29 VGPRs / 42 SGPRs, scatter 14 / 20, search 67 / 91, no scratch, no LDS.
#include "knn3_query_kernels.h"

// ---- host -------------------------------------------------------------------------------------------------------------------
extern "C" int pn_knn3_query_launches(void) { return 8; }

extern "C" long long pn_knn3_query_workspace_bytes(long long totalR, long long totalQ, int S) {
  if (totalR < 0 || totalQ < 0 || S < 0) return 0;
  KqWs w;
  return kq_carve(nullptr, totalR, totalQ, S, &w) + 16;
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
    hipLaunchKernelGGL(pn_knn3_query_cells_kernel<false>, dim3(row_blocks), dim3(256), 0, stream, qry, off_r, off_q, S, totalR,
                       totalQ, k, ppc, bin, w, idx, dist, (const uint32_t*)nullptr);
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
                       totalR, totalQ, k, ppc, w, idx, dist, (const uint32_t*)nullptr);
  }
  PN_CHECK_LAUNCH();
  return PN_OK;
}
