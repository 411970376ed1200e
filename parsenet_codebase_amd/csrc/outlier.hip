// Statistical outlier removal over a ragged batch of clouds of ANY size, for gfx950: the definition of outlier_math.h,
// the same source the test suite compiles for the host.  Per point the mean distance to its k nearest (from the
// distances of knn3_ragged / knn3_grid), per cloud mean, standard deviation and threshold of that statistic, the mask
// of the points below the threshold and their indices in ascending order — the cleaner in front of the farthest-point
// sampling, which otherwise spends its first samples on the strays.
//
// Workspace (pn_outlier_workspace_bytes, linear in total):            tiles = total / OL_TILE + S
//   part 8 tiles | count 4 tiles | tile_seg 4 tiles | tile_first 4 tiles
//   part[b]         the sum of tile b by the tree of outlier_math.h: of the terms (launch 1), then of the squared
//                   deviations (launch 3, after launch 2 has read the first)
//   count[b]        the kept points of tile b
//   tile_seg/first  the flat table tile -> (cloud, first LOCAL point); -1 for a tile number that holds nothing
// Launches, all stream-ordered, pn_outlier_launches() = 6 of them; no memset, no cooperative launch, no flag anybody
// waits for, no workgroup waits for another, no atomic of any kind:
//   1 stat    per tile: the table entry, a_i of its points, part[b].  Workgroup b also looks at rows 1024 b .. of the
//             flat array and marks those that no valid segment of off holds: avg NaN, keep 0, index -1.
//   2 mean    per cloud: the tile sums in ascending order -> stats[c][0]; kept[c] = 0.  An invalid segment: stats NaN.
//   3 dev     per tile: part[b] of the squared deviations from the cloud's mean; a NaN mean goes into avg of its cloud.
//   4 thr     per cloud: the tile sums in ascending order -> std and thr in stats[c][1], stats[c][2].
//   5 mask    per tile: keep of its points, count[b] (ballots and popcounts: integers).
//   6 index   per tile: the kept points of the cloud's tiles before it and in all of them (integer sums of count, in any
//             order), kept[c] from the cloud's first tile; the rank of a kept point inside the tile from the ballots of
//             the 16 runs of 64 points in index order, wave offsets in LDS; -1 into the entries from kept[c] on.
// Visibility: a launch reads what earlier launches wrote (stream order); nothing is handed over inside a launch.
// The two per-cloud launches add sequentially — that is the definition — from LDS, 256 tile sums staged per round.
#include "common.h"
#include "outlier_math.h"

struct OlWs {
  double* part;
  int* count;
  int* tile_seg;
  int* tile_first;
};

// The arrays of the workspace in order, cut from `base` (0: measure only); returns their bytes.
static long long ol_carve(void* base, long long total, int S, OlWs* w) {
  RgCarver c = {(uintptr_t)base, 0};
  const long long tiles = ol_tiles(total, S);
  w->part = c.take<double>(tiles);
  w->count = c.take<int>(tiles);
  w->tile_seg = c.take<int>(tiles);
  w->tile_first = c.take<int>(tiles);
  return c.bytes;
}

// The sum of the tile's 1 024 terms (v: the four of this lane) by the tree of outlier_math.h; every lane gets it.
__device__ static inline double ol_block_sum(const double* v, double* sh) {
  double s = ol_lane_sum(v[0], v[1], v[2], v[3]);
#pragma unroll
  for (int h = OL_WAVE / 2; h > 0; h >>= 1) s = ol_add(s, __shfl_xor(s, h, OL_WAVE));
  if (pn_lane() == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  return ol_wave_sum(sh[0], sh[1], sh[2], sh[3]);
}

// VEC: k is a multiple of 4 and dist is 16-byte aligned, so a row is read as float4.
template <bool VEC>
__device__ static inline double ol_row(const float* __restrict__ row, int kc) {
  if (!VEC) return ol_point(row, kc);
  double s = 0.0;
  int j = 0;
  for (; j + 4 <= kc; j += 4) {
    const float4 q = *reinterpret_cast<const float4*>(row + j);
    const float x[4] = {q.x, q.y, q.z, q.w};
    s = ol_accumulate(s, x, 4);
  }
  return ol_average(ol_accumulate(s, row + j, kc - j), kc);
}

template <bool VEC>
__global__ __launch_bounds__(OL_LANES) void pn_outlier_stat_kernel(const float* __restrict__ dist,
                                                                   const int* __restrict__ off, int S, int total, int k,
                                                                   OlWs w, double* __restrict__ avg,
                                                                   uint8_t* __restrict__ keep,
                                                                   int32_t* __restrict__ index) {
  __shared__ double sh[OL_WAVES];
  const long long b = blockIdx.x;
#pragma unroll
  for (int p = 0; p < OL_PER_LANE; ++p) {                    // rows of the flat array that no valid segment holds
    const long long g = b * OL_TILE + p * OL_LANES + (long long)threadIdx.x;
    if (g >= total) continue;
    const int s = rg_row_segment(off, S, (int)g);
    if (rg_segment_holds(off[s], off[s + 1], total, (int)g)) continue;
    avg[g] = ol_nan();
    keep[g] = 0;
    if (index) index[g] = -1;
  }
  const int c = rg_segment(S, b, [off](int s) { return ol_tile_base(off[s], s); });
  const int o0 = off[c], o1 = off[c + 1];
  const long long first = (b - ol_tile_base(o0, c)) * OL_TILE;
  const int n = o1 - o0;
  const bool live = rg_valid_segment(o0, o1, total) && first >= 0 && first < n;       // uniform over the workgroup
  if (threadIdx.x == 0) {
    w.tile_seg[b] = live ? c : -1;
    w.tile_first[b] = live ? (int)first : 0;
  }
  if (!live) return;
  const int kc = ol_count(k, n);
  double v[OL_PER_LANE];
#pragma unroll
  for (int p = 0; p < OL_PER_LANE; ++p) {
    const int i = (int)first + p * OL_LANES + (int)threadIdx.x;
    v[p] = 0.0;
    if (i >= n) continue;
    const size_t g = (size_t)o0 + i;
    const double a = ol_row<VEC>(dist + g * (size_t)k, kc);
    avg[g] = a;
    v[p] = ol_mean_term(a);
  }
  const double s = ol_block_sum(v, sh);
  if (threadIdx.x == 0) w.part[b] = s;
}

// Launches 2 (stage 0) and 4 (stage 1): one workgroup per cloud adds the cloud's tile sums in ascending order.
__global__ __launch_bounds__(OL_LANES) void pn_outlier_cloud_kernel(const int* __restrict__ off, int total, int stage,
                                                                    double std_ratio, OlWs w,
                                                                    double* __restrict__ stats,
                                                                    int32_t* __restrict__ kept) {
  __shared__ double buf[OL_LANES];
  const int c = blockIdx.x;
  const int o0 = off[c], o1 = off[c + 1];
  if (!rg_valid_segment(o0, o1, total)) {
    if (threadIdx.x == 0 && stage == 0) {
      stats[3 * (size_t)c] = stats[3 * (size_t)c + 1] = stats[3 * (size_t)c + 2] = ol_nan();
      kept[c] = 0;
    }
    return;
  }
  const int n = o1 - o0, nt = ol_cloud_tiles(n);
  const double* part = w.part + ol_tile_base(o0, c);
  double s = 0.0;
  for (int base = 0; base < nt; base += OL_LANES) {
    if (base + (int)threadIdx.x < nt) buf[threadIdx.x] = part[base + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = nt - base < OL_LANES ? nt - base : OL_LANES;
#pragma unroll 8
      for (int j = 0; j < m; ++j) s = ol_add(s, buf[j]);
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (stage == 0) {
    stats[3 * (size_t)c] = ol_mean(s, n);
    kept[c] = 0;
  } else {
    const double sd = ol_std(s, n);
    stats[3 * (size_t)c + 1] = sd;
    stats[3 * (size_t)c + 2] = ol_threshold(stats[3 * (size_t)c], sd, std_ratio);
  }
}

__global__ __launch_bounds__(OL_LANES) void pn_outlier_dev_kernel(const int* __restrict__ off, OlWs w,
                                                                  double* __restrict__ avg,
                                                                  const double* __restrict__ stats) {
  __shared__ double sh[OL_WAVES];
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0) return;
  const int o0 = off[c], n = off[c + 1] - o0, first = w.tile_first[blockIdx.x];
  const double mean = stats[3 * (size_t)c];
  double v[OL_PER_LANE];
#pragma unroll
  for (int p = 0; p < OL_PER_LANE; ++p) {
    const int i = first + p * OL_LANES + (int)threadIdx.x;
    v[p] = 0.0;
    if (i >= n) continue;
    if (ol_poisoned(mean)) avg[(size_t)o0 + i] = mean;
    v[p] = ol_dev_term(ol_poisoned(mean) ? mean : avg[(size_t)o0 + i], mean);
  }
  const double s = ol_block_sum(v, sh);
  if (threadIdx.x == 0) w.part[blockIdx.x] = s;
}

__global__ __launch_bounds__(OL_LANES) void pn_outlier_mask_kernel(const int* __restrict__ off, OlWs w,
                                                                   const double* __restrict__ avg,
                                                                   const double* __restrict__ stats,
                                                                   uint8_t* __restrict__ keep) {
  __shared__ int sh[OL_WAVES];
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0) return;
  const int o0 = off[c], n = off[c + 1] - o0, first = w.tile_first[blockIdx.x];
  const double thr = stats[3 * (size_t)c + 2];
  int count = 0;                                                              // of this wave: the same in all its lanes
#pragma unroll
  for (int p = 0; p < OL_PER_LANE; ++p) {
    const int i = first + p * OL_LANES + (int)threadIdx.x;
    int kp = 0;
    if (i < n) {
      kp = ol_keep(avg[(size_t)o0 + i], thr);
      keep[(size_t)o0 + i] = (uint8_t)kp;
    }
    count += __popcll(__ballot(kp));
  }
  if (pn_lane() == 0) sh[threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x == 0) w.count[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(OL_LANES) void pn_outlier_index_kernel(const int* __restrict__ off, OlWs w,
                                                                    const uint8_t* __restrict__ keep,
                                                                    int32_t* __restrict__ kept,
                                                                    int32_t* __restrict__ index) {
  __shared__ unsigned sums[2 * OL_WAVES];
  __shared__ unsigned runs[OL_PER_LANE * OL_WAVES];
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0) return;
  const int o0 = off[c], n = off[c + 1] - o0, first = w.tile_first[blockIdx.x];
  const int nt = ol_cloud_tiles(n), mine = first / OL_TILE;
  const int* count = w.count + ol_tile_base(o0, c);
  unsigned before = 0, all = 0;                               // kept points of the cloud's tiles before this one, of all
  for (int t = threadIdx.x; t < nt; t += OL_LANES) {
    const unsigned q = (unsigned)count[t];
    all += q;
    before += t < mine ? q : 0u;
  }
  before = (unsigned)pn_wave_sum_i((int)before);
  all = (unsigned)pn_wave_sum_i((int)all);
  const int wave = threadIdx.x >> 6;
  if (pn_lane() == 0) {
    sums[wave] = before;
    sums[OL_WAVES + wave] = all;
  }
  int kp[OL_PER_LANE];
  unsigned long long ballot[OL_PER_LANE];
#pragma unroll
  for (int p = 0; p < OL_PER_LANE; ++p) {
    const int i = first + p * OL_LANES + (int)threadIdx.x;
    kp[p] = i < n ? (int)keep[(size_t)o0 + i] : 0;
    ballot[p] = __ballot(kp[p]);
    if (pn_lane() == 0) runs[p * OL_WAVES + wave] = (unsigned)__popcll(ballot[p]);
  }
  __syncthreads();
  before = ((sums[0] + sums[1]) + sums[2]) + sums[3];
  all = ((sums[OL_WAVES] + sums[OL_WAVES + 1]) + sums[OL_WAVES + 2]) + sums[OL_WAVES + 3];
  if (first == 0 && threadIdx.x == 0) kept[c] = (int32_t)all;
  if (!index) return;
#pragma unroll
  for (int p = 0; p < OL_PER_LANE; ++p) {
    const int i = first + p * OL_LANES + (int)threadIdx.x;
    unsigned pos = before + (unsigned)pn_mbcnt(ballot[p]);
    for (int r = 0; r < p * OL_WAVES + wave; ++r) pos += runs[r];
    if (kp[p] && pos < (unsigned)n) index[(size_t)o0 + pos] = i;      // (pos < n always, unless off changed under us)
    if (i < n && (unsigned)i >= all) index[(size_t)o0 + i] = -1;
  }
}

extern "C" long long pn_outlier_workspace_bytes(long long total, int S) {
  if (total < 0 || S < 0) return 0;
  OlWs w;
  return ol_carve(nullptr, total, S, &w) + 16;
}

extern "C" int pn_outlier_launches(void) { return ol_launches(); }

extern "C" int pn_outlier_stat_f32(const float* dist, const int* off, int S, int total, int k, double std_ratio,
                                   double* avg, double* stats, uint8_t* keep, int32_t* kept, int32_t* index, void* ws,
                                   long long ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "pn_outlier_stat_f32";
  PN_CHECK_ARG(k >= OL_MIN_K && k <= OL_MAX_K, "%s: k=%d (%d .. %d)", who, k, OL_MIN_K, OL_MAX_K);
  PN_CHECK_ARG(S >= 0 && total >= 0, "%s: S=%d total=%d (total below 2^31)", who, S, total);
  PN_CHECK_ARG((long long)total * k < (1ll << 31), "%s: total * k = %lld (below 2^31)", who, (long long)total * k);
  PN_CHECK_ARG(std_ratio >= 0.0 && std_ratio <= 1.7976931348623157e308, "%s: std_ratio=%g (finite, not negative)", who,
               std_ratio);
  if (S == 0 || total == 0) return PN_OK;
  PN_CHECK_ARG(dist && off && avg && stats && keep && kept && ws,
               "%s: null pointer (dist, off, avg, stats, keep, kept and ws are required)", who);
  PN_CHECK_ARG(ws_bytes >= pn_outlier_workspace_bytes(total, S), "%s: workspace of %lld bytes (%lld)", who, ws_bytes,
               pn_outlier_workspace_bytes(total, S));
  OlWs w;
  ol_carve((void*)pn_align_up((size_t)ws, 16), total, S, &w);
  const dim3 block(OL_LANES), tiles((unsigned)ol_tiles(total, S)), clouds((unsigned)S);
  PN_PROF("outlier", stream);
  if (k % 4 == 0 && ((uintptr_t)dist & 15) == 0)
    hipLaunchKernelGGL(pn_outlier_stat_kernel<true>, tiles, block, 0, stream, dist, off, S, total, k, w, avg, keep,
                       index);
  else
    hipLaunchKernelGGL(pn_outlier_stat_kernel<false>, tiles, block, 0, stream, dist, off, S, total, k, w, avg, keep,
                       index);
  hipLaunchKernelGGL(pn_outlier_cloud_kernel, clouds, block, 0, stream, off, total, 0, std_ratio, w, stats, kept);
  hipLaunchKernelGGL(pn_outlier_dev_kernel, tiles, block, 0, stream, off, w, avg, (const double*)stats);
  hipLaunchKernelGGL(pn_outlier_cloud_kernel, clouds, block, 0, stream, off, total, 1, std_ratio, w, stats, kept);
  hipLaunchKernelGGL(pn_outlier_mask_kernel, tiles, block, 0, stream, off, w, (const double*)avg, (const double*)stats,
                     keep);
  hipLaunchKernelGGL(pn_outlier_index_kernel, tiles, block, 0, stream, off, w, (const uint8_t*)keep, kept, index);
  PN_CHECK_LAUNCH();
  return PN_OK;
}
