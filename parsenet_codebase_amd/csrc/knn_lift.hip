// k-nearest-sample lifting over a ragged batch: per-sample values carried to every point through the neighbours
// pn_knn3_query_f32 found (idx LOCAL to the reference segment, dist).  The two rules — inverse-distance interpolation
// in fp64 and the majority vote — are knn_lift_math.h, the same source the test suite compiles for the host.
//
// One launch each, no workspace, no atomics, no host synchronisation:
//   interpolate  one lane per (row, channel), channels fastest: the lanes of a wave read consecutive floats of the same
//                row of `values`, and the k (idx, dist) pairs of their row from the cache.
//   vote         one lane per row.
// A row that no valid segment holds is NaN / -1.
//
// Resource report of hipcc --offload-arch=gfx950 -O3 (-Rpass-analysis=kernel-resource-usage):
//   pn_knn_interpolate_kernel  VGPRs: 26  TotalSGPRs: 28  ScratchSize [bytes/lane]: 0  Occupancy [waves/SIMD]: 8
//   pn_knn_vote_kernel         VGPRs: 15  TotalSGPRs: 24  ScratchSize [bytes/lane]: 0  Occupancy [waves/SIMD]: 8
#include "common.h"
#include "knn_lift_math.h"
#include "ragged.h"

// The reference rows [o0, o1) of the segment that holds query row `row`; 0 when no valid segment does.
__device__ static inline int kl_segment(const int* __restrict__ off_r, const int* __restrict__ off_q, int S, int totalR,
                                        int totalQ, int row, int* o0, int* o1) {
  const int s = rg_row_segment(off_q, S, row);
  *o0 = off_r[s];
  *o1 = off_r[s + 1];
  return rg_segment_holds(off_q[s], off_q[s + 1], totalQ, row) && rg_valid_segment(*o0, *o1, totalR);
}

__global__ __launch_bounds__(256) void pn_knn_interpolate_kernel(const float* __restrict__ values,
                                                                 const int* __restrict__ off_r, int totalR,
                                                                 const int32_t* __restrict__ idx,
                                                                 const float* __restrict__ dist,
                                                                 const int* __restrict__ off_q, int totalQ, int S, int k,
                                                                 long long C, float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)totalQ * C) return;
  const int row = (int)(e / C);
  const long long c = e - (long long)row * C;
  int o0, o1;
  if (!kl_segment(off_r, off_q, S, totalR, totalQ, row, &o0, &o1)) {
    out[e] = kl_nan();
    return;
  }
  out[e] = kl_interpolate(values + (size_t)o0 * C, C, c, idx + (size_t)row * k, dist + (size_t)row * k, k, o1 - o0);
}

__global__ __launch_bounds__(256) void pn_knn_vote_kernel(const int32_t* __restrict__ labels,
                                                          const int* __restrict__ off_r, int totalR,
                                                          const int32_t* __restrict__ idx,
                                                          const int* __restrict__ off_q, int totalQ, int S, int k,
                                                          int32_t* __restrict__ out) {
  const long long row64 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row64 >= totalQ) return;
  const int row = (int)row64;
  int o0, o1;
  if (!kl_segment(off_r, off_q, S, totalR, totalQ, row, &o0, &o1)) {
    out[row] = -1;
    return;
  }
  out[row] = kl_vote(labels + o0, idx + (size_t)row * k, k, o1 - o0);
}

// What the two entry points check alike.
static int kl_check(const char* who, int totalR, int totalQ, int S, int k) {
  PN_CHECK_ARG(k >= KL_MIN_K && k <= KL_MAX_K, "%s: k=%d (%d <= k <= %d)", who, k, KL_MIN_K, KL_MAX_K);
  PN_CHECK_ARG(S >= 0 && totalR >= 0 && totalQ >= 0, "%s: S=%d totalR=%d totalQ=%d", who, S, totalR, totalQ);
  PN_CHECK_ARG((long long)totalQ * k < (1ll << 31), "%s: totalQ * k = %lld (below 2^31)", who, (long long)totalQ * k);
  return PN_OK;
}

extern "C" int pn_knn_interpolate_f32(const float* values, const int* off_r, int totalR, const int32_t* idx,
                                      const float* dist, const int* off_q, int totalQ, int S, int k, int C, float* out,
                                      void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = kl_check("pn_knn_interpolate_f32", totalR, totalQ, S, k);
  if (rc != PN_OK) return rc;
  PN_CHECK_ARG(C >= 1, "pn_knn_interpolate_f32: C=%d (at least 1)", C);
  PN_CHECK_ARG((long long)totalQ * C < (1ll << 39), "pn_knn_interpolate_f32: totalQ * C = %lld (below 2^39)",
               (long long)totalQ * C);      // (one lane per element, 256 per workgroup, an int of workgroups)
  if (totalQ == 0 || S == 0) return PN_OK;
  PN_CHECK_ARG((values || totalR == 0) && off_r && idx && dist && off_q && out, "pn_knn_interpolate_f32: null pointer");
  {
    PN_PROF("knn_interpolate", stream);
    hipLaunchKernelGGL(pn_knn_interpolate_kernel, dim3(pn_cdiv((long long)totalQ * C, 256)), dim3(256), 0, stream, values,
                       off_r, totalR, idx, dist, off_q, totalQ, S, k, (long long)C, out);
  }
  PN_CHECK_LAUNCH();
  return PN_OK;
}

extern "C" int pn_knn_vote_i32(const int32_t* labels, const int* off_r, int totalR, const int32_t* idx,
                               const int* off_q, int totalQ, int S, int k, int32_t* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = kl_check("pn_knn_vote_i32", totalR, totalQ, S, k);
  if (rc != PN_OK) return rc;
  if (totalQ == 0 || S == 0) return PN_OK;
  PN_CHECK_ARG((labels || totalR == 0) && off_r && idx && off_q && out, "pn_knn_vote_i32: null pointer");
  {
    PN_PROF("knn_vote", stream);
    hipLaunchKernelGGL(pn_knn_vote_kernel, dim3(pn_cdiv(totalQ, 256)), dim3(256), 0, stream, labels, off_r, totalR, idx,
                       off_q, totalQ, S, k, out);
  }
  PN_CHECK_LAUNCH();
  return PN_OK;
}
