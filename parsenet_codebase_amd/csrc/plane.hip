// Dominant-plane extraction over a ragged batch of clouds of ANY size, for gfx950: the definition of plane_math.h, the
// same source the test suite compiles for the host.  H sampled planes per cloud are scored against every point of the
// cloud, the one with the most inliers wins and is refined by least squares through its inliers — the step between the
// downsampling and the Euclidean clusters that takes the table, the floor or the fixture plate out of a scan.
//
// Workspace (pn_plane_workspace_bytes, known from (total, S, H) alone):            tiles = total / PL_TILE + S
//   hyp 32 S H | part 48 tiles | mean 24 S | cand 32 S | hcount 4 S H | tcount, tile_seg, tile_first, tile_bad 4 tiles
//   each | cand_ok 4 S
//   hyp[c][h]       the plane of hypothesis h of cloud c, nx a NaN where the hypothesis is invalid
//   hcount[c][h]    its inliers: integer sums of the tiles' counts, in any order
//   part[q][b]      sum q of tile b by the tree of outlier_math.h: the coordinates of the inliers (q < 3), then their six
//                   centred products
//   mean, cand      per cloud: the mean of the inliers, the refit; cand_ok: the refit is valid
//   tcount[b]       the inliers of the refit in tile b
//   tile_seg/first  the flat table tile -> (cloud, first LOCAL point); -1 for a tile number that holds nothing
//   tile_bad[b]     tile b holds a non-finite coordinate
// Launches, all stream-ordered, pn_plane_launches(refine) = 5 + 6 refine of them; no memset, no cooperative launch, no
// workgroup waits for another:
//   1 bounds    per tile: the table entry and tile_bad; the rows of the flat array that no valid segment holds get
//               inlier 0 and dist NaN; hcount is zeroed by all workgroups together.
//   2 hyp       one lane per (cloud, h): pl_hypothesis.
//   3 score     the hot path.  Per tile: its 1 024 points in registers as fp64, four per lane (an absent point as NaN,
//               which is no inlier of anything); the cloud's H planes one after the other from a wave-uniform address;
//               the inliers of a wave counted by four ballots and population counts, kept by lane h % 64 of the wave in
//               a register, and every 64 hypotheses added to the H counters in LDS; at the end one integer atomicAdd
//               per non-zero counter to hcount.
//   4 select    per cloud: the status, the maximum of pl_key over the valid hypotheses -> plane, count, best.
//   per round   5 mean partials (tile) | 6 mean (cloud) | 7 moment partials (tile) | 8 moments, pl_refit (cloud) |
//               9 the refit's count (tile) | 10 decision (cloud).  A cloud without a plane, or without a valid refit,
//               exits in the first instructions.
//   last        per tile: inlier and dist of its points against the final plane.
// Visibility: a launch reads what earlier launches wrote (stream order); nothing is handed over inside a launch.  The
// per-cloud launches add the tile sums sequentially — that is the definition — from LDS, 256 tiles staged per round.
#include "common.h"
#include "plane_math.h"

struct PlWs {
  double* hyp;
  double* part;
  double* mean;
  double* cand;
  uint32_t* hcount;
  int* tcount;
  int* tile_seg;
  int* tile_first;
  int* tile_bad;
  int* cand_ok;
  long long tiles;
};

struct PlAxis {
  double a[3];
  double min_cos;
  int on;
};

// The arrays of the workspace in order, cut from `base` (0: measure only); returns their bytes.
static long long pl_carve(void* base, long long total, int S, int H, PlWs* w) {
  RgCarver c = {(uintptr_t)base, 0};
  const long long tiles = ol_tiles(total, S), SH = (long long)S * H;
  w->tiles = tiles;
  w->hyp = c.take<double>(4 * SH);
  w->part = c.take<double>(PL_MOMENTS * tiles);
  w->mean = c.take<double>(3ll * S);
  w->cand = c.take<double>(4ll * S);
  w->hcount = c.take<uint32_t>(SH);
  w->tcount = c.take<int>(tiles);
  w->tile_seg = c.take<int>(tiles);
  w->tile_first = c.take<int>(tiles);
  w->tile_bad = c.take<int>(tiles);
  w->cand_ok = c.take<int>(S);
  return c.bytes;
}

// The sum of the tile's 1 024 terms (v: the four of this lane) by the tree of outlier_math.h into sh[0 .. 3]; the caller
// reads ol_wave_sum(sh) behind a barrier.  Every sum of a launch has its own sh.
__device__ static inline void pl_wave_part(const double* v, double* sh) {
  double s = ol_lane_sum(v[0], v[1], v[2], v[3]);
#pragma unroll
  for (int h = OL_WAVE / 2; h > 0; h >>= 1) s = ol_add(s, __shfl_xor(s, h, OL_WAVE));
  if (pn_lane() == 0) sh[threadIdx.x >> 6] = s;
}

__device__ static inline double pl_nan(void) { return ol_nan(); }

__global__ __launch_bounds__(PL_LANES) void pn_plane_bounds_kernel(const float* __restrict__ pts,
                                                                   const int* __restrict__ off, int S, int total, int H,
                                                                   PlWs w, uint8_t* __restrict__ inlier,
                                                                   float* __restrict__ dist) {
  const long long b = blockIdx.x;
  const long long SH = (long long)S * H, step = (long long)gridDim.x * PL_LANES;
  for (long long g = b * PL_LANES + threadIdx.x; g < SH; g += step) w.hcount[g] = 0u;
#pragma unroll
  for (int p = 0; p < PL_PER_LANE; ++p) {                    // rows of the flat array that no valid segment holds
    const long long g = b * PL_TILE + p * PL_LANES + (long long)threadIdx.x;
    if (g >= total) continue;
    const int s = rg_row_segment(off, S, (int)g);
    if (rg_segment_holds(off[s], off[s + 1], total, (int)g)) continue;
    inlier[g] = 0;
    if (dist) dist[g] = (float)pl_nan();
  }
  const int c = rg_segment(S, b, [off](int s) { return ol_tile_base(off[s], s); });
  const int o0 = off[c], o1 = off[c + 1];
  const long long first = (b - ol_tile_base(o0, c)) * PL_TILE;
  const int n = o1 - o0;
  const bool live = rg_valid_segment(o0, o1, total) && first >= 0 && first < n;       // uniform over the workgroup
  int bad = 0;
  if (live) {
#pragma unroll
    for (int p = 0; p < PL_PER_LANE; ++p) {
      const int i = (int)first + p * PL_LANES + (int)threadIdx.x;
      if (i >= n) continue;
      const float* q = pts + 3 * ((size_t)o0 + i);
      bad |= !(kg_finite(q[0]) && kg_finite(q[1]) && kg_finite(q[2]));
    }
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    w.tile_seg[b] = live ? c : -1;
    w.tile_first[b] = live ? (int)first : 0;
    w.tile_bad[b] = bad ? 1 : 0;
  }
}

__global__ __launch_bounds__(PL_LANES) void pn_plane_hyp_kernel(const float* __restrict__ pts,
                                                                const int* __restrict__ off, int S, int total, int H,
                                                                unsigned long long seed, PlAxis axis, PlWs w) {
  const long long g = (long long)blockIdx.x * PL_LANES + threadIdx.x;
  if (g >= (long long)S * H) return;
  const int c = (int)(g / H), h = (int)(g % H);
  const int o0 = off[c], o1 = off[c + 1];
  PlPlane p = pl_none();
  if (rg_valid_segment(o0, o1, total))
    p = pl_hypothesis(pts + 3 * (size_t)o0, o1 - o0, seed, h, axis.on ? axis.a : nullptr, axis.min_cos);
  double* out = w.hyp + 4 * (size_t)g;
  out[0] = p.valid ? p.nx : pl_nan();
  out[1] = p.ny;
  out[2] = p.nz;
  out[3] = p.d;
}

// The fp64 coordinates of the four points of this lane; an absent point is NaN throughout.
__device__ static inline void pl_load(const float* __restrict__ pts, int o0, int n, int first, double* x, double* y,
                                      double* z) {
#pragma unroll
  for (int p = 0; p < PL_PER_LANE; ++p) {
    const int i = first + p * PL_LANES + (int)threadIdx.x;
    x[p] = y[p] = z[p] = pl_nan();
    if (i >= n) continue;
    const float* q = pts + 3 * ((size_t)o0 + i);
    x[p] = (double)q[0], y[p] = (double)q[1], z[p] = (double)q[2];
  }
}

__global__ __launch_bounds__(PL_LANES) void pn_plane_score_kernel(const float* __restrict__ pts,
                                                                  const int* __restrict__ off,
                                                                  const float* __restrict__ threshold, int H, PlWs w) {
  __shared__ uint32_t sh[PL_MAX_H];
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0) return;
  const float tf = threshold[c];
  if (!pl_threshold_ok(tf)) return;                                           // status -2: nothing is read from hcount
  const double t = (double)tf;
  const int o0 = off[c], n = off[c + 1] - o0, first = w.tile_first[blockIdx.x];
  for (int h = threadIdx.x; h < H; h += PL_LANES) sh[h] = 0u;
  double x[PL_PER_LANE], y[PL_PER_LANE], z[PL_PER_LANE];
  pl_load(pts, o0, n, first, x, y, z);
  __syncthreads();
  const double* __restrict__ hyp = w.hyp + 4 * (size_t)c * H;
  const int lane = pn_lane();
  for (int h0 = 0; h0 < H; h0 += OL_WAVE) {
    const int m = H - h0 < OL_WAVE ? H - h0 : OL_WAVE;
    uint32_t acc = 0u;                                                        // of hypothesis h0 + lane, this wave
    for (int j = 0; j < m; ++j) {
      const double* q = hyp + 4 * (size_t)(h0 + j);                           // the same address in every lane
      const double nx = q[0], ny = q[1], nz = q[2], d = q[3];
      if (nx != nx) continue;                                                 // invalid: uniform
      uint32_t cnt = 0u;
#pragma unroll
      for (int p = 0; p < PL_PER_LANE; ++p)
        cnt += (uint32_t)__popcll(__ballot(pl_inlier(pl_signed(nx, ny, nz, d, x[p], y[p], z[p]), t)));
      acc += lane == j ? cnt : 0u;
    }
    if (lane < m && acc) atomicAdd(&sh[h0 + lane], acc);
  }
  __syncthreads();
  uint32_t* hcount = w.hcount + (size_t)c * H;
  for (int h = threadIdx.x; h < H; h += PL_LANES)
    if (sh[h]) atomicAdd(&hcount[h], sh[h]);
}

__global__ __launch_bounds__(PL_LANES) void pn_plane_select_kernel(const int* __restrict__ off, int total,
                                                                   const float* __restrict__ threshold, int H, PlWs w,
                                                                   double* __restrict__ plane,
                                                                   int32_t* __restrict__ count,
                                                                   int32_t* __restrict__ best) {
  __shared__ unsigned long long keys[OL_WAVES];
  const int c = blockIdx.x;
  const int o0 = off[c], o1 = off[c + 1];
  const bool seg = rg_valid_segment(o0, o1, total);                           // uniform
  int bad = 0;
  unsigned long long key = 0ull;
  if (seg) {
    const int nt = ol_cloud_tiles(o1 - o0);
    const int* tile_bad = w.tile_bad + ol_tile_base(o0, c);
    for (int t = threadIdx.x; t < nt; t += PL_LANES) bad |= tile_bad[t];
    const double* hyp = w.hyp + 4 * (size_t)c * H;
    const uint32_t* hcount = w.hcount + (size_t)c * H;
    for (int h = threadIdx.x; h < H; h += PL_LANES) {
      const double nx = hyp[4 * (size_t)h];
      const unsigned long long k = nx == nx ? pl_key(hcount[h], (uint32_t)h) : 0ull;
      key = k > key ? k : key;
    }
  }
  bad = __syncthreads_or(bad);
  key = pn_wave_max_u64(key);
  if (pn_lane() == 0) keys[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int v = 0; v < OL_WAVES; ++v) key = keys[v] > key ? keys[v] : key;
  const int status = seg ? pl_status(bad, threshold[c]) : 0;
  const int h = seg && status == 0 ? pl_key_h(key) : -1;
  double* out = plane + 4 * (size_t)c;
  if (h < 0) {
    out[0] = out[1] = out[2] = out[3] = 0.0;
    count[c] = status;
    best[c] = -1;
    return;
  }
  const double* q = w.hyp + 4 * ((size_t)c * H + h);
  out[0] = q[0], out[1] = q[1], out[2] = q[2], out[3] = q[3];
  count[c] = pl_key_count(key);
  best[c] = h;
}

// Launches 5 (STAGE 0: the coordinates of the inliers of the current plane) and 7 (STAGE 1: their centred products).
template <int STAGE>
__global__ __launch_bounds__(PL_LANES) void pn_plane_sums_kernel(const float* __restrict__ pts,
                                                                 const int* __restrict__ off,
                                                                 const float* __restrict__ threshold, PlWs w,
                                                                 const double* __restrict__ plane,
                                                                 const int32_t* __restrict__ best) {
  constexpr int K = STAGE == 0 ? 3 : PL_MOMENTS;
  __shared__ double sh[K][OL_WAVES];
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0 || best[c] < 0) return;
  const int o0 = off[c], n = off[c + 1] - o0, first = w.tile_first[blockIdx.x];
  const double t = (double)threshold[c];
  const double* q = plane + 4 * (size_t)c;
  const double nx = q[0], ny = q[1], nz = q[2], d = q[3];
  double x[PL_PER_LANE], y[PL_PER_LANE], z[PL_PER_LANE];
  pl_load(pts, o0, n, first, x, y, z);
  double v[K][PL_PER_LANE];
  double mean[3] = {0.0, 0.0, 0.0};
  if (STAGE == 1) mean[0] = w.mean[3 * (size_t)c], mean[1] = w.mean[3 * (size_t)c + 1], mean[2] = w.mean[3 * (size_t)c + 2];
#pragma unroll
  for (int p = 0; p < PL_PER_LANE; ++p) {
    const int in = pl_inlier(pl_signed(nx, ny, nz, d, x[p], y[p], z[p]), t);
    if (STAGE == 0) {
      v[0][p] = pl_term(in, x[p]), v[1][p] = pl_term(in, y[p]), v[2][p] = pl_term(in, z[p]);
    } else {
      double prod[PL_MOMENTS];
      pl_products(x[p], y[p], z[p], mean, prod);
#pragma unroll
      for (int k = 0; k < K; ++k) v[k][p] = pl_term(in, prod[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) pl_wave_part(v[k], sh[k]);
  __syncthreads();
  if (threadIdx.x < K)
    w.part[(size_t)threadIdx.x * w.tiles + blockIdx.x] =
        ol_wave_sum(sh[threadIdx.x][0], sh[threadIdx.x][1], sh[threadIdx.x][2], sh[threadIdx.x][3]);
}

// Launches 6 (STAGE 0: the mean) and 8 (STAGE 1: the moments and the refit): one workgroup per cloud adds the cloud's
// tile sums in ascending order, lane k those of sum k.
template <int STAGE>
__global__ __launch_bounds__(PL_LANES) void pn_plane_cloud_kernel(const int* __restrict__ off, PlAxis axis, PlWs w,
                                                                  const int32_t* __restrict__ count,
                                                                  const int32_t* __restrict__ best) {
  constexpr int K = STAGE == 0 ? 3 : PL_MOMENTS;
  __shared__ double buf[K][PL_LANES];
  __shared__ double sums[PL_MOMENTS];
  const int c = blockIdx.x;
  if (best[c] < 0) {                                                          // no plane (an invalid segment included)
    if (STAGE == 1 && threadIdx.x == 0) w.cand_ok[c] = 0;
    return;
  }
  const int o0 = off[c], nt = ol_cloud_tiles(off[c + 1] - o0);
  const long long tb = ol_tile_base(o0, c);
  double s = 0.0;
  for (int base = 0; base < nt; base += PL_LANES) {
    if (base + (int)threadIdx.x < nt) {
#pragma unroll
      for (int k = 0; k < K; ++k) buf[k][threadIdx.x] = w.part[(size_t)k * w.tiles + tb + base + threadIdx.x];
    }
    __syncthreads();
    if (threadIdx.x < K) {
      const int m = nt - base < PL_LANES ? nt - base : PL_LANES;
#pragma unroll 8
      for (int j = 0; j < m; ++j) s = ol_add(s, buf[threadIdx.x][j]);
    }
    __syncthreads();
  }
  const int m = count[c];
  if (STAGE == 0) {
    if (threadIdx.x < K) w.mean[3 * (size_t)c + threadIdx.x] = pl_mean(s, m);
    return;
  }
  if (threadIdx.x < K) sums[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const PlPlane p = pl_refit(w.mean + 3 * (size_t)c, sums, m, axis.on ? axis.a : nullptr, axis.min_cos);
  double* out = w.cand + 4 * (size_t)c;
  out[0] = p.nx, out[1] = p.ny, out[2] = p.nz, out[3] = p.d;
  w.cand_ok[c] = p.valid;
}

// Launch 9: the inliers of the refit in every tile (ballots and popcounts: integers).
__global__ __launch_bounds__(PL_LANES) void pn_plane_count_kernel(const float* __restrict__ pts,
                                                                  const int* __restrict__ off,
                                                                  const float* __restrict__ threshold, PlWs w,
                                                                  const int32_t* __restrict__ best) {
  __shared__ int sh[OL_WAVES];
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0 || best[c] < 0 || !w.cand_ok[c]) return;
  const int o0 = off[c], n = off[c + 1] - o0, first = w.tile_first[blockIdx.x];
  const double t = (double)threshold[c];
  const double* q = w.cand + 4 * (size_t)c;
  const double nx = q[0], ny = q[1], nz = q[2], d = q[3];
  double x[PL_PER_LANE], y[PL_PER_LANE], z[PL_PER_LANE];
  pl_load(pts, o0, n, first, x, y, z);
  int cnt = 0;                                                                // of this wave: the same in all its lanes
#pragma unroll
  for (int p = 0; p < PL_PER_LANE; ++p)
    cnt += __popcll(__ballot(pl_inlier(pl_signed(nx, ny, nz, d, x[p], y[p], z[p]), t)));
  if (pn_lane() == 0) sh[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) w.tcount[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// Launch 10: the refit replaces the plane iff it is valid and holds at least as many inliers.
__global__ __launch_bounds__(PL_LANES) void pn_plane_decide_kernel(const int* __restrict__ off, PlWs w,
                                                                   double* __restrict__ plane,
                                                                   int32_t* __restrict__ count,
                                                                   const int32_t* __restrict__ best) {
  __shared__ int sh[OL_WAVES];
  const int c = blockIdx.x;
  if (best[c] < 0 || !w.cand_ok[c]) return;
  const int o0 = off[c], nt = ol_cloud_tiles(off[c + 1] - o0);
  const int* tcount = w.tcount + ol_tile_base(o0, c);
  int s = 0;
  for (int t = threadIdx.x; t < nt; t += PL_LANES) s += tcount[t];
  s = pn_wave_sum_i(s);
  if (pn_lane() == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  s = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  if (!pl_take(1, s, count[c])) return;
  const double* q = w.cand + 4 * (size_t)c;
  double* out = plane + 4 * (size_t)c;
  out[0] = q[0], out[1] = q[1], out[2] = q[2], out[3] = q[3];
  count[c] = s;
}

__global__ __launch_bounds__(PL_LANES) void pn_plane_final_kernel(const float* __restrict__ pts,
                                                                  const int* __restrict__ off,
                                                                  const float* __restrict__ threshold, PlWs w,
                                                                  const double* __restrict__ plane,
                                                                  const int32_t* __restrict__ best,
                                                                  uint8_t* __restrict__ inlier,
                                                                  float* __restrict__ dist) {
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0) return;
  const int o0 = off[c], n = off[c + 1] - o0, first = w.tile_first[blockIdx.x];
  const bool found = best[c] >= 0;
  const double t = (double)threshold[c];
  const double* q = plane + 4 * (size_t)c;
  const double nx = q[0], ny = q[1], nz = q[2], d = q[3];
#pragma unroll
  for (int p = 0; p < PL_PER_LANE; ++p) {
    const int i = first + p * PL_LANES + (int)threadIdx.x;
    if (i >= n) continue;
    const size_t g = (size_t)o0 + i;
    const float* r = pts + 3 * g;
    const double s = found ? pl_signed(nx, ny, nz, d, (double)r[0], (double)r[1], (double)r[2]) : pl_nan();
    inlier[g] = (uint8_t)(found && pl_inlier(s, t));
    if (dist) dist[g] = (float)s;
  }
}

extern "C" long long pn_plane_workspace_bytes(long long total, int S, int H) {
  if (total < 0 || total >= (1ll << 31) || S < 0 || H < 1 || H > PL_MAX_H) return 0;
  PlWs w;
  return pl_carve(nullptr, total, S, H, &w) + 16;
}

extern "C" int pn_plane_launches(int refine) { return pl_launches(refine); }

extern "C" int pn_plane_f32(const float* pts, const int* off, int S, int total, const float* threshold, int H,
                            long long seed, int refine, const double* axis, double min_cos, double* plane,
                            int32_t* count, int32_t* best, uint8_t* inlier, float* dist, void* ws, long long ws_bytes,
                            void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "pn_plane_f32";
  PN_CHECK_ARG(S >= 0 && total >= 0, "%s: S=%d total=%d (total below 2^31)", who, S, total);
  PN_CHECK_ARG(H >= 1 && H <= PL_MAX_H, "%s: H=%d (1 .. %d)", who, H, PL_MAX_H);
  PN_CHECK_ARG(refine >= 0 && refine <= PL_MAX_REFINE, "%s: refine=%d (0 .. %d)", who, refine, PL_MAX_REFINE);
  PN_CHECK_ARG(!axis || (min_cos >= 0.0 && min_cos <= 1.0), "%s: min_cos=%g (0 .. 1 with an axis)", who, min_cos);
  PN_CHECK_ARG((long long)S * H < (1ll << 31), "%s: S * H = %lld (below 2^31)", who, (long long)S * H);
  if (S == 0 || total == 0) return PN_OK;
  PN_CHECK_ARG(pts && off && threshold && plane && count && best && inlier && ws,
               "%s: null pointer (pts, off, threshold, plane, count, best, inlier and ws are required)", who);
  PN_CHECK_ARG(ws_bytes >= pn_plane_workspace_bytes(total, S, H), "%s: workspace of %lld bytes (%lld)", who, ws_bytes,
               pn_plane_workspace_bytes(total, S, H));
  PlWs w;
  pl_carve((void*)pn_align_up((size_t)ws, 16), total, S, H, &w);
  PlAxis ax = {{0.0, 0.0, 0.0}, 0.0, 0};
  if (axis) ax = PlAxis{{axis[0], axis[1], axis[2]}, min_cos, 1};
  const dim3 block(PL_LANES), tiles((unsigned)w.tiles), clouds((unsigned)S);
  const dim3 hyps((unsigned)pn_cdiv((long long)S * H, PL_LANES));
  PN_PROF("plane", stream);
  hipLaunchKernelGGL(pn_plane_bounds_kernel, tiles, block, 0, stream, pts, off, S, total, H, w, inlier, dist);
  hipLaunchKernelGGL(pn_plane_hyp_kernel, hyps, block, 0, stream, pts, off, S, total, H, (unsigned long long)seed, ax,
                     w);
  {
    PN_PROF("plane_score", stream);
    hipLaunchKernelGGL(pn_plane_score_kernel, tiles, block, 0, stream, pts, off, threshold, H, w);
  }
  hipLaunchKernelGGL(pn_plane_select_kernel, clouds, block, 0, stream, off, total, threshold, H, w, plane, count, best);
  for (int r = 0; r < refine; ++r) {
    hipLaunchKernelGGL(pn_plane_sums_kernel<0>, tiles, block, 0, stream, pts, off, threshold, w, (const double*)plane,
                       (const int32_t*)best);
    hipLaunchKernelGGL(pn_plane_cloud_kernel<0>, clouds, block, 0, stream, off, ax, w, (const int32_t*)count,
                       (const int32_t*)best);
    hipLaunchKernelGGL(pn_plane_sums_kernel<1>, tiles, block, 0, stream, pts, off, threshold, w, (const double*)plane,
                       (const int32_t*)best);
    hipLaunchKernelGGL(pn_plane_cloud_kernel<1>, clouds, block, 0, stream, off, ax, w, (const int32_t*)count,
                       (const int32_t*)best);
    hipLaunchKernelGGL(pn_plane_count_kernel, tiles, block, 0, stream, pts, off, threshold, w, (const int32_t*)best);
    hipLaunchKernelGGL(pn_plane_decide_kernel, clouds, block, 0, stream, off, w, plane, count, (const int32_t*)best);
  }
  hipLaunchKernelGGL(pn_plane_final_kernel, tiles, block, 0, stream, pts, off, threshold, w, (const double*)plane,
                     (const int32_t*)best, inlier, dist);
  PN_CHECK_LAUNCH();
  return PN_OK;
}
