// Point normals of a ragged batch of 3-D clouds from the clouds themselves, for gfx950: the eigenvector of the
// smallest eigenvalue of the covariance of the k nearest neighbours of every point (k-NN PCA), with the surface
// variation and the eigenvalue gap that says how well that normal is defined.  The neighbours are those
// pn_knn3_ragged (knn3.hip) returns; the arithmetic is normal_math.h, the same source the test suite compiles for the
// host.
//
// One launch for all segments.  A workgroup is ONE wave and owns NR_POINTS = 64 consecutive points of one segment
// (flat tile table tile -> (segment, first point) as in cover.hip and tridist.hip); a lane owns one point and its
// work is serial: 2 k gathered rows of 12 bytes (one pass for the mean, one for the covariance; the rows of a
// neighbourhood are near each other in a cloud ordered along a curve and sit in the cache the second time), then the
// five sweeps of the 3 x 3 Jacobi iteration, about 200 fp64 operations.  The kernel is latency-bound, and what hides
// latency is the number of waves in flight across the machine: 10 000 points are 157 one-wave workgroups, which the
// dispatcher spreads over 157 of the 256 CUs, where 256-point workgroups would stack four waves on each of 40 CUs and
// leave the rest idle.  No LDS, no scratch, no atomics; every sum runs in neighbour order in one lane, so a point's
// result depends on its neighbourhood alone: the same bits from run to run, alone and inside a batch, for every
// tiling.  Plain vector stores only.
// A segment with fewer than k points arrives padded with the point itself (knn3's contract): the padding entries
// count as copies of the point.  A segment of fewer than 3 points gets zero normals and zero scalars.
#include "common.h"
#include "normal_math.h"

#define NR_POINTS 64      // points per workgroup, one per lane

__global__ __launch_bounds__(NR_POINTS) void pn_point_normals_kernel(
    const float* __restrict__ pts, const int* __restrict__ off, int S, int total, const int* __restrict__ idx, int k,
    const float* __restrict__ view, const int* __restrict__ tile_seg, const int* __restrict__ tile_first,
    float* __restrict__ normals, float* __restrict__ variation, float* __restrict__ gap) {
  const int s = tile_seg[blockIdx.x];
  if (s < 0 || s >= S) return;   // (a table that does not belong to these offsets reads nothing)
  const int o0 = off[s], o1 = off[s + 1];
  const int p = tile_first[blockIdx.x] + (int)threadIdx.x;
  if (o0 < 0 || o1 > total || p < o0 || p >= o1) return;
  float n[3], var, g;
  nm_point(pts + 3 * (size_t)o0, o1 - o0, idx + (size_t)p * k, k, NM_SWEEPS, n, &var, &g);
  if (view) nm_orient(n, pts + 3 * (size_t)p, view + 3 * (size_t)s);
  normals[3 * (size_t)p] = n[0], normals[3 * (size_t)p + 1] = n[1], normals[3 * (size_t)p + 2] = n[2];
  if (variation) variation[p] = var;
  if (gap) gap[p] = g;
}

extern "C" int pn_point_normals_tile(void) { return NR_POINTS; }

extern "C" int pn_point_normals_f32(const float* pts, const int* off, int S, int total, const int32_t* idx, int k,
                                    const float* viewpoints, const int* tile_seg, const int* tile_first,
                                    int total_tiles, float* normals, float* variation, float* gap, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PN_CHECK_ARG(k >= NM_MIN_K && k <= NM_MAX_K, "pn_point_normals_f32: k=%d (%d <= k <= %d)", k, NM_MIN_K, NM_MAX_K);
  PN_CHECK_ARG(S >= 0 && total >= 0 && total_tiles >= 0, "pn_point_normals_f32: S=%d total=%d tiles=%d", S, total,
               total_tiles);
  if (total == 0 || S == 0) return PN_OK;
  PN_CHECK_ARG(pts && off && idx && normals && tile_seg && tile_first, "pn_point_normals_f32: null pointer");
  PN_CHECK_ARG(total_tiles > 0, "pn_point_normals_f32: %d points in %d tiles", total, total_tiles);
  PN_PROF("point_normals", stream);
  hipLaunchKernelGGL(pn_point_normals_kernel, dim3(total_tiles), dim3(NR_POINTS), 0, stream, pts, off, S, total, idx,
                     k, viewpoints, tile_seg, tile_first, normals, variation, gap);
  PN_CHECK_LAUNCH();
  return PN_OK;
}
