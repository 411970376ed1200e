// Farthest-point sampling of a ragged batch of 3-D clouds of ANY size, for gfx950: the definition of fps_math.h, the
// same source the test suite compiles for the host.  m samples per cloud in selection order, their radii, and for every
// point the rank of the nearest sample ("owner") and the distance to it — the reducer in front of the network and the
// lift of its per-sample results back to every scanned point.
//
// Workspace (pn_fps_workspace_bytes, linear in total and in S m):
//   slot 8 S (m + 2) | D 4 total | tile_seg 4 tiles | tile_first 4 tiles          tiles = total / FPS_TILE + S
//   slot[c][t]      the key (radius_t, s_t) of step t; slot[c][m + 1] nonzero: the cloud holds a non-finite coordinate
//   D[g]            the working distance of point g, FPS_CHOSEN once it is a sample
//   tile_seg/first  the flat table tile -> (cloud, first LOCAL point); -1 for a tile number that holds nothing
// Launches, all stream-ordered, m + 2 of them (pn_fps_launches) after one memset of the slots; no cooperative launch, no
// flag anybody waits for, no workgroup waits for another:
//   init     per tile: the table entry, D = +inf and owner = -1 over the tile, the cloud's non-finite flag (a 64-bit
//            atomicMax of 1), and from the first tile of a cloud the start slot (+inf, start).
//   step t   ONE kernel: a workgroup decodes s_t from slot (c, t), loads that row, updates D and owner of its tile,
//            reduces the tile's best candidate key (wave shuffles, 4 words of LDS) and issues one 64-bit integer
//            atomicMax on slot (c, t + 1) — behind a plain read that is never above the slot, so it only ever saves an
//            atomic.  A workgroup of a cloud with t >= m_c, of a flagged cloud or of a spare tile exits at once.
//   outputs  sample / radius decoded from the slots (grid-stride over S m), -1 / NaN past m_c and on flagged clouds;
//            dist from D over the tile, owner = -1 and dist = NaN on flagged clouds.
// Visibility: a launch reads what earlier launches wrote (stream order); inside a step launch slot (c, t) is only read
// and slot (c, t + 1) only takes atomics.  Every store is a plain vector store or that integer atomic.
// Tile shape: 256 lanes x 4 points.  A step is one dependent chain (slot -> sample row -> distances -> key -> atomic),
// so a lane keeps four independent 12-byte rows and four D in flight to cover the latency of one; 1 024 points per
// workgroup puts a million-point cloud at 977 workgroups (under four per CU, one wave of atomics per step) and a
// 10 000-point cloud at 10, where the step is launch-bound whatever the shape.
#include "common.h"
#include "fps_math.h"

struct FpsWs {
  unsigned long long* slot;
  float* D;
  int* tile_seg;
  int* tile_first;
};

// The arrays of the workspace in order, cut from `base` (0: measure only); returns their bytes.
static long long fps_carve(void* base, long long total, int S, int m, FpsWs* w) {
  RgCarver c = {(uintptr_t)base, 0};
  w->slot = c.take<unsigned long long>(fps_slots(m) * S);
  w->D = c.take<float>(total);
  w->tile_seg = c.take<int>(fps_tiles(total, S));
  w->tile_first = c.take<int>(fps_tiles(total, S));
  return c.bytes;
}

// The cloud whose tile numbers hold tile b: the last c with fps_tile_base(off[c], c) <= b.
__device__ static inline int fps_find_segment(const int* __restrict__ off, int S, long long b) {
  return rg_segment(S, b, [off](int c) { return fps_tile_base(off[c], c); });
}

__device__ static inline unsigned long long fps_block_max(unsigned long long v, unsigned long long* sh) {
  v = pn_wave_max_u64(v);
  if (pn_lane() == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long r = sh[0];
#pragma unroll
  for (int w = 1; w < FPS_LANES / PN_WAVE; ++w) r = sh[w] > r ? sh[w] : r;
  return r;
}

__global__ __launch_bounds__(FPS_LANES) void pn_fps_init_kernel(const float* __restrict__ pts,
                                                                const int* __restrict__ off, int S, int total, int m,
                                                                const int* __restrict__ start, FpsWs w,
                                                                int* __restrict__ owner) {
  const int b = blockIdx.x;
  const int c = fps_find_segment(off, S, b);
  const int o0 = off[c], o1 = off[c + 1];
  const long long first = ((long long)b - fps_tile_base(o0, c)) * FPS_TILE;
  const int n = o1 - o0;
  const bool live = fps_valid_segment(o0, o1, total) && first >= 0 && first < n;      // uniform over the workgroup
  if (threadIdx.x == 0) {
    w.tile_seg[b] = live ? c : -1;
    w.tile_first[b] = live ? (int)first : 0;
  }
  if (!live) return;
  int bad = 0;
#pragma unroll
  for (int p = 0; p < FPS_PER_LANE; ++p) {
    const int i = (int)first + p * FPS_LANES + (int)threadIdx.x;
    if (i >= n) continue;
    const size_t g = (size_t)o0 + i;
    bad |= !(kg_finite(pts[3 * g]) && kg_finite(pts[3 * g + 1]) && kg_finite(pts[3 * g + 2]));
    w.D[g] = kg_inf();
    if (owner) owner[g] = -1;
  }
  unsigned long long* slot = w.slot + fps_slots(m) * c;
  if (__syncthreads_or(bad) && threadIdx.x == 0) atomicMax(&slot[fps_flag_slot(m)], 1ull);
  if (first == 0 && threadIdx.x == 0) slot[0] = fps_key(kg_inf(), (uint32_t)fps_clamp_start(start ? start[c] : 0, n));
}

__global__ __launch_bounds__(FPS_LANES) void pn_fps_step_kernel(const float* __restrict__ pts,
                                                                const int* __restrict__ off, int m, int t, FpsWs w,
                                                                int* __restrict__ owner) {
  __shared__ unsigned long long sh[FPS_LANES / PN_WAVE];
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0) return;
  const int o0 = off[c], n = off[c + 1] - o0;
  if (t >= (m < n ? m : n)) return;
  unsigned long long* slot = w.slot + fps_slots(m) * c;
  if (slot[fps_flag_slot(m)] != 0) return;
  const uint32_t s = fps_key_index(slot[t]);                 // below n: the start was clamped, a candidate is a point
  if (s >= (uint32_t)n) return;                              // (an empty slot: only if off changed under the launches)
  const size_t gs = (size_t)o0 + s;
  const float q[3] = {pts[3 * gs], pts[3 * gs + 1], pts[3 * gs + 2]};
  const int first = w.tile_first[blockIdx.x];
  unsigned long long best = FPS_NO_KEY;
#pragma unroll
  for (int p = 0; p < FPS_PER_LANE; ++p) {
    const int i = first + p * FPS_LANES + (int)threadIdx.x;
    if (i >= n) continue;
    const size_t g = (size_t)o0 + i;
    const float x[3] = {pts[3 * g], pts[3 * g + 1], pts[3 * g + 2]};
    float D = w.D[g];
    int owned;
    const unsigned long long key = fps_point_step(x, q, (uint32_t)i, s, &D, &owned);
    if (owned) {
      w.D[g] = D;
      if (owner) owner[g] = t;
    }
    best = key > best ? key : best;
  }
  best = fps_block_max(best, sh);
  if (threadIdx.x == 0 && best > slot[t + 1]) atomicMax(&slot[t + 1], best);
}

__global__ __launch_bounds__(FPS_LANES) void pn_fps_output_kernel(const int* __restrict__ off, int S, int total, int m,
                                                                  FpsWs w, int* __restrict__ sample,
                                                                  float* __restrict__ radius, int* __restrict__ owner,
                                                                  float* __restrict__ dist) {
  const long long E = (long long)S * m;
  for (long long e = (long long)blockIdx.x * FPS_LANES + threadIdx.x; e < E; e += (long long)gridDim.x * FPS_LANES) {
    const int c = (int)(e / m), t = (int)(e - (long long)c * m);
    const int o0 = off[c], o1 = off[c + 1];
    const unsigned long long* slot = w.slot + fps_slots(m) * c;
    const int n = fps_valid_segment(o0, o1, total) ? o1 - o0 : 0;
    const bool have = t < n && slot[fps_flag_slot(m)] == 0;
    const unsigned long long key = slot[t];
    sample[e] = have ? (int)fps_key_index(key) : -1;
    if (radius) radius[e] = have ? fps_key_dist(key) : __builtin_nanf("");
  }
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0 || (!owner && !dist)) return;
  const int o0 = off[c], n = off[c + 1] - o0;
  const bool bad = w.slot[fps_slots(m) * c + fps_flag_slot(m)] != 0;
  const int first = w.tile_first[blockIdx.x];
#pragma unroll
  for (int p = 0; p < FPS_PER_LANE; ++p) {
    const int i = first + p * FPS_LANES + (int)threadIdx.x;
    if (i >= n) continue;
    const size_t g = (size_t)o0 + i;
    if (dist) dist[g] = bad ? __builtin_nanf("") : fps_final_dist(w.D[g]);
    if (bad && owner) owner[g] = -1;
  }
}

extern "C" long long pn_fps_workspace_bytes(long long total, int S, int m) {
  if (total < 0 || S < 0 || m < 1 || fps_slots(m) * S >= (1ll << 59)) return 0;
  FpsWs w;
  return fps_carve(nullptr, total, S, m, &w) + 16;
}

extern "C" int pn_fps_launches(int m) { return fps_launches(m < 0 ? 0 : m); }

extern "C" int pn_fps_f32(const float* pts, const int* off, int S, int total, int max_n, int m, const int32_t* start,
                          int32_t* sample, float* radius, int32_t* owner, float* dist, void* ws, long long ws_bytes,
                          void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "pn_fps_f32";
  PN_CHECK_ARG(m >= 1, "%s: m=%d (m >= 1)", who, m);
  PN_CHECK_ARG(S >= 0 && total >= 0 && max_n >= 0, "%s: S=%d total=%d max_n=%d (total below 2^31)", who, S, total,
               max_n);
  PN_CHECK_ARG(fps_slots(m) * S < (1ll << 59), "%s: S * (m + 2) = %lld (below 2^59)", who, fps_slots(m) * S);
  if (S == 0) return PN_OK;
  PN_CHECK_ARG(off && sample && ws && (pts || total == 0), "%s: null pointer (pts, off, sample and ws are required)",
               who);
  PN_CHECK_ARG(ws_bytes >= pn_fps_workspace_bytes(total, S, m), "%s: workspace of %lld bytes (%lld)", who, ws_bytes,
               pn_fps_workspace_bytes(total, S, m));
  FpsWs w;
  fps_carve((void*)pn_align_up((size_t)ws, 16), total, S, m, &w);
  const dim3 block(FPS_LANES), grid((unsigned)fps_tiles(total, S));
  PN_CHECK_HIP(hipMemsetAsync(w.slot, 0, (size_t)((char*)w.D - (char*)w.slot), stream));
  PN_PROF("fps", stream);
  hipLaunchKernelGGL(pn_fps_init_kernel, grid, block, 0, stream, pts, off, S, total, m, start, w, owner);
  for (int t = 0; t < m; ++t)
    hipLaunchKernelGGL(pn_fps_step_kernel, grid, block, 0, stream, pts, off, m, t, w, owner);
  hipLaunchKernelGGL(pn_fps_output_kernel, grid, block, 0, stream, off, S, total, m, w, sample, radius, owner, dist);
  PN_CHECK_LAUNCH();
  return PN_OK;
}
