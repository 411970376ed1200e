// Exact k nearest neighbours of 3-D points by a uniform-grid search, for a ragged batch of clouds of ANY size: the
// results of pn_knn3_ragged's fp32 mode (knn3.hip), bit for bit, at cost O(n k) instead of O(n^2) and without its
// limit of 10 240 points per cloud.  The definition — grid, cell function, rings, the termination bound and why it is
// safe — is knn3_grid_math.h, the same source the test suite compiles for the host.
//
// Five stream-ordered phases (plus two memsets), no cooperative launch, no grid-wide barrier, no host synchronisation.
// Phases 1 - 4, the workspace and the ring loop of phase 5 are knn3_grid_build.h, shared with knn3_query.hip:
//   1 bbox     min / max per axis and segment (atomics on the order-preserving integer image, one set per wave where
//              the wave's rows lie in one segment) and the non-finite flag.  Every later phase derives the segment's
//              grid from these six numbers with kg_grid: no table is built, nothing is downloaded.
//   2 cells    the cell of every point and its rank inside the cell (the value the histogram's atomic returned).
//   3 scan     exclusive scan of a segment's histogram to global record positions, one workgroup per segment.
//   4 scatter  (x, y, z, local index) as one 16-byte record per point to start[cell] + rank.  The order inside a cell
//              is the order of the atomics; no output depends on it, because selection is by the key (d, j) alone.
//   5 search   one wave per record (queries in cell order: the waves of a workgroup read the same cells).  The wave
//              keeps its best 64 keys knn_key(-d, j), one per lane, sorted.  Ring by ring (knn3_grid_math.h) the
//              rows of the shell — a row of cells along x is one contiguous range of records — are handed out one
//              per lane; a batch of 64 records is one 16-byte load per lane; a ballot of "beats the k-th" skips the
//              merge (knn_wave_sort128 of the list and the batch) for most batches.  No capacity anywhere: a cell of
//              thousands of coincident points is slow, not wrong.  The row goes to the query's ORIGINAL position.
//
// Workspace (pn_knn3_grid_workspace_bytes): records 16 total | cell 4 total | rank 4 total | box max 12 S | flag 4 S |
// cell starts 4 (total + 2 S) | box min 12 S.  Segment s owns the cell slots [off[s] + 2 s, off[s + 1] + 2 s + 2):
// at most max(1, n_s) cells and the end sentinel.
//
// Resource report of hipcc --offload-arch=gfx950 -O3 (-Rpass-analysis=kernel-resource-usage):
//   pn_knn3_grid_search_kernel  VGPRs: 67  TotalSGPRs: 97  ScratchSize [bytes/lane]: 0  Occupancy [waves/SIMD]: 7
//                               LDS Size [bytes/block]: 0 — no spill
//   bbox 23 / cells 26 / scan 35 / scatter 12 VGPRs, ScratchSize 0 for all four, 8 waves/SIMD
#include "knn3_grid_build.h"

// ---- 5: the search --------------------------------------------------------------------------------------------------------
// (phases 1 - 4, the workspace and the ring loop: knn3_grid_build.h, shared with knn3_query.hip)
__global__ __launch_bounds__(256) void pn_knn3_grid_search_kernel(const int* __restrict__ off, int S, int total, int k,
                                                                  int ppc, KgWs w, int* __restrict__ idx,
                                                                  float* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const long long p64 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p64 >= total) return;
  const int p = (int)p64;
  const int s = kg_segment(off, S, p);
  const int o0 = off[s], o1 = off[s + 1], n = o1 - o0;
  if (p < o0 || p >= o1) return;
  if (w.flag[s]) {      // a non-finite coordinate in the segment: the point itself k times, dist NaN
    if (lane < k) {
      idx[(size_t)p * k + lane] = p - o0;
      if (dist) dist[(size_t)p * k + lane] = __builtin_nanf("");
    }
    return;
  }
  const float4 me = w.rec[p];
  const int self = __float_as_int(me.w);
  if ((unsigned)self >= (unsigned)n) return;
  const KgGrid g = kg_segment_grid(w, s, n, ppc);
  const float q[3] = {me.x, me.y, me.z};
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = kg_cell(g, a, q[a]);
  const u64 best = kg_ring_search(w, w.start + (size_t)o0 + 2 * (size_t)s, g, o0, o1, n, k, q, c);
  if (lane < k) {
    const size_t o = ((size_t)o0 + self) * k + lane;
    const bool have = best != 0ull;                                // fewer than k points in the segment: pad with self
    idx[o] = have ? (int)knn_key_index(best) : self;
    if (dist) dist[o] = have ? kg_key_dist(best) : 0.0f;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
extern "C" long long pn_knn3_grid_workspace_bytes(long long total, int S) {
  if (total < 0 || S < 0) return 0;
  KgWs w;
  return kg_carve(nullptr, total, S, &w) + 16;
}

extern "C" int pn_knn3_grid_f32(const float* pts, const int* off, int S, int total, int max_n, int k, int32_t* idx,
                                float* dist, void* ws, long long ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PN_CHECK_ARG(k >= KG_MIN_K && k <= KG_MAX_K, "pn_knn3_grid_f32: k=%d (%d <= k <= %d)", k, KG_MIN_K, KG_MAX_K);
  PN_CHECK_ARG(S >= 0 && total >= 0 && max_n >= 0, "pn_knn3_grid_f32: S=%d total=%d max_n=%d", S, total, max_n);
  PN_CHECK_ARG((long long)total * k < (1ll << 31), "pn_knn3_grid_f32: total * k = %lld (below 2^31)",
               (long long)total * k);
  if (total == 0 || S == 0) return PN_OK;
  PN_CHECK_ARG(pts && off && idx && ws, "pn_knn3_grid_f32: null pointer");
  PN_CHECK_ARG(ws_bytes >= pn_knn3_grid_workspace_bytes(total, S), "pn_knn3_grid_f32: workspace of %lld bytes (%lld)",
               ws_bytes, pn_knn3_grid_workspace_bytes(total, S));
  KgWs w;
  kg_carve((void*)pn_align_up((size_t)ws, 16), total, S, &w);
  const int ppc = kg_ppc();
  const int rc = kg_build_launch(pts, off, S, total, ppc, w, stream);
  if (rc != PN_OK) return rc;
  {
    PN_PROF("knn3_grid_search", stream);
    hipLaunchKernelGGL(pn_knn3_grid_search_kernel, dim3(pn_cdiv(total, 4)), dim3(256), 0, stream, off, S, total, k, ppc,
                       w, idx, dist);
  }
  PN_CHECK_LAUNCH();
  return PN_OK;
}
