// Voxel-grid downsampling of a ragged batch of 3-D clouds of ANY size, for gfx950: the definition of voxel_math.h, the
// same source the test suite compiles for the host.  Per occupied cell of a cubic grid the exact centroid of its
// points, their count, the lowest point index and the scanned point nearest to the centroid; per point the number of
// its voxel ("owner") — the first reduction of a raw scan, in front of the farthest-point sampling, and the lift of
// per-voxel results back to every scanned point.
//
// Workspace (pn_voxel_workspace_bytes, linear in total):     cap = 2 total, tiles = total / VX_TILE + S
//   key 8 cap | repkey 8 total | first 4 cap | bmin 16 S          one memset 0xff
//   U 24 cap | count 4 cap | bmax 16 S | flag 4 S (+ 4 S)         one memset 0
//   cent 12 total | slot 4 total | tile_seg, tile_first, tile_heads 4 tiles each
//   key/first/count/U  the open-addressing table: segment c owns the slots 2 off[c] .. 2 off[c + 1] - 1
//   repkey[g]       row v of a segment: the smallest (d to the centroid, index) among the points of voxel v
//   bmin/bmax/flag  per segment: the order-preserving integer image of the bounds; non-finite and out-of-range bits
//   cent[g]         row v of a segment: the centroid of voxel v (the output may be NULL; the rep launch reads this one)
//   slot[g]         the LOCAL slot of point g, VX_NONE for a point whose cell is out of range
//   tile_heads[b]   the heads of tile b, then (scan launch) the heads of the segment's tiles before b
// Launches, all stream-ordered, pn_voxel_launches() = 7 of them after the two memsets (6 when rep is NULL); no
// cooperative launch, no flag anybody waits for, no workgroup waits for another:
//   1 bounds  per tile: the table entry tile -> (cloud, first LOCAL point); min / max per axis (integer atomics, one
//             set per workgroup) and the non-finite bit.
//   2 table   per point: the cell key, the out-of-range bit, the slot of the key (an agent-scope read, then a 64-bit
//             atomicCAS on VX_EMPTY; linear probing inside the segment's slots), atomicMin of the index into first,
//             atomicAdd into count and the three U.
//   3 heads   per tile: the points with first[slot] == i, counted by ballots.
//   4 scan    per cloud, one workgroup: the exclusive sums of its tile counts in tile order; nvox[c] = V or the status.
//   5 rows    per tile: a head's voxel number = heads of the tiles before + heads before it in the tile (ballots of
//             the 16 runs of 64 points in index order); the head writes owner, centroid (and cent), count and first
//             of its voxel; every point i >= V of the cloud writes NaN / -1 into row i; a cloud with a status: owner
//             -1, every row NaN / -1.
//   6 owner   per point that is no head: owner = owner of first[slot] (heads are not written in this launch); with rep:
//             d to the centroid of its voxel and a 64-bit atomicMin on repkey, behind an agent-scope read that is
//             never below the slot, so it only ever saves an atomic.
//   7 rep     row v < V: the index of repkey.
// Visibility: a launch reads what earlier launches wrote (stream order).  Inside launch 2 a slot's key only ever
// changes from VX_EMPTY to its final value, by compare-and-swap, and every other word of the table only takes atomics.
// Every store is a plain vector store or an integer atomic.  A voxel of thousands of coincident points serialises its
// atomics on one slot: slow, not wrong.
//
// Resource report of hipcc --offload-arch=gfx950 -O3 (-Rpass-analysis=kernel-resource-usage):
//   pn_voxel_table_kernel  VGPRs: 66  ScratchSize [bytes/lane]: 0  Occupancy [waves/SIMD]: 7  LDS Size [bytes/block]: 256
//                          (the probe loop with its 64-bit key, the fp64 cells and three 64-bit sums in flight) — no spill
//   bounds 19 / heads 8 / scan 24 / rows 38 / owner 16 / rep 6 VGPRs, ScratchSize 0 for all six, 8 waves/SIMD,
//   LDS 112 / 16 / 16 / 64 / 0 / 0 bytes per block.  The fp64 divisions of voxel_math.h compile to the IEEE sequence
//   (v_div_scale_f64, v_rcp_f64, v_div_fmas_f64, v_div_fixup_f64): correctly rounded under the build's flags.
#include "common.h"
#include "voxel_math.h"

struct VxWs {
  unsigned long long* key;
  unsigned long long* repkey;
  uint32_t* first;
  uint32_t* bmin;
  unsigned long long* U;
  uint32_t* count;
  uint32_t* bmax;
  uint32_t* flag;
  float* cent;
  uint32_t* slot;
  int* tile_seg;
  int* tile_first;
  int* tile_heads;
};

// The arrays of the workspace in order, cut from `base` (0: measure only); returns their bytes.
static long long vx_carve(void* base, long long total, long long S, VxWs* w) {
  RgCarver c = {(uintptr_t)base, 0};
  const long long cap = 2 * total, tiles = vx_tiles(total, (int)S);
  w->key = c.take<unsigned long long>(cap);
  w->repkey = c.take<unsigned long long>(total);
  w->first = c.take<uint32_t>(cap);
  w->bmin = c.take<uint32_t>(4 * S);
  w->U = c.take<unsigned long long>(3 * cap);      // (the zero memset starts here)
  w->count = c.take<uint32_t>(cap);
  w->bmax = c.take<uint32_t>(4 * S);
  w->flag = c.take<uint32_t>(2 * S);
  w->cent = c.take<float>(3 * total);
  w->slot = c.take<uint32_t>(total);
  w->tile_seg = c.take<int>(tiles);
  w->tile_first = c.take<int>(tiles);
  w->tile_heads = c.take<int>(tiles);
  return c.bytes;
}

// What every launch after the first knows of a segment.
struct VxSeg {
  float lo[3], hi[3], o[3];
  float h;
  int shift;
  uint32_t flag;
};

__device__ static inline VxSeg vx_segment(const VxWs& w, int c, const float* __restrict__ voxel,
                                          const float* __restrict__ origin) {
  VxSeg g;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    g.lo[a] = pn_ord2f(w.bmin[4 * (size_t)c + a]);
    g.hi[a] = pn_ord2f(w.bmax[4 * (size_t)c + a]);
    g.o[a] = origin ? origin[3 * (size_t)c + a] : g.lo[a];
  }
  g.h = voxel[c];
  g.flag = w.flag[c];
  g.shift = (g.flag & VX_NON_FINITE) ? 0 : vx_shift(g.lo, g.hi);
  return g;
}

__device__ static inline unsigned long long vx_peek(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(VX_LANES) void pn_voxel_bounds_kernel(const float* __restrict__ pts,
                                                                   const int* __restrict__ off, int S, int total,
                                                                   VxWs w) {
  __shared__ uint32_t sh[VX_WAVES][7];
  const long long b = blockIdx.x;
  const int c = rg_segment(S, b, [off](int s) { return vx_tile_base(off[s], s); });
  const int o0 = off[c], o1 = off[c + 1];
  const long long first = (b - vx_tile_base(o0, c)) * VX_TILE;
  const int n = o1 - o0;
  const bool live = rg_valid_segment(o0, o1, total) && first >= 0 && first < n;       // uniform over the workgroup
  if (threadIdx.x == 0) {
    w.tile_seg[b] = live ? c : -1;
    w.tile_first[b] = live ? (int)first : 0;
    w.tile_heads[b] = 0;
  }
  if (!live) return;
  uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u}, bad = 0u;
#pragma unroll
  for (int p = 0; p < VX_PER_LANE; ++p) {
    const int i = (int)first + p * VX_LANES + (int)threadIdx.x;
    if (i >= n) continue;
    const size_t g = (size_t)o0 + i;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float x = pts[3 * g + a];
      bad |= kg_finite(x) ? 0u : 1u;
      const uint32_t o = pn_f2ord(x);
      mn[a] = o < mn[a] ? o : mn[a];
      mx[a] = o > mx[a] ? o : mx[a];
    }
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mn[a] = pn_wave_min_u32(mn[a]);
    mx[a] = pn_wave_max_u32(mx[a]);
  }
  bad = __ballot(bad != 0u) != 0ull ? 1u : 0u;
  if (pn_lane() == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      sh[wave][a] = mn[a];
      sh[wave][3 + a] = mx[a];
    }
    sh[wave][6] = bad;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    uint32_t lo = sh[0][a], hi = sh[0][3 + a];
#pragma unroll
    for (int v = 1; v < VX_WAVES; ++v) {
      lo = sh[v][a] < lo ? sh[v][a] : lo;
      hi = sh[v][3 + a] > hi ? sh[v][3 + a] : hi;
    }
    atomicMin(&w.bmin[4 * (size_t)c + a], lo);
    atomicMax(&w.bmax[4 * (size_t)c + a], hi);
  }
  if (threadIdx.x == 3 && (sh[0][6] | sh[1][6] | sh[2][6] | sh[3][6])) atomicOr(&w.flag[c], VX_NON_FINITE);
}

__global__ __launch_bounds__(VX_LANES) void pn_voxel_table_kernel(const float* __restrict__ pts,
                                                                  const int* __restrict__ off,
                                                                  const float* __restrict__ voxel,
                                                                  const float* __restrict__ origin, VxWs w) {
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0) return;
  const VxSeg sg = vx_segment(w, c, voxel, origin);
  if ((sg.flag & VX_NON_FINITE) || !vx_good_size(sg.h)) return;
  const int o0 = off[c], n = off[c + 1] - o0, first = w.tile_first[blockIdx.x];
  const uint32_t cap = 2u * (uint32_t)n;
  const size_t base = 2 * (size_t)o0;
  unsigned long long* tkey = w.key + base;
  int out = 0;
#pragma unroll 1
  for (int p = 0; p < VX_PER_LANE; ++p) {
    const int i = first + p * VX_LANES + (int)threadIdx.x;
    if (i >= n) continue;
    const size_t g = (size_t)o0 + i;
    const float x[3] = {pts[3 * g], pts[3 * g + 1], pts[3 * g + 2]};
    int ok;
    const unsigned long long key = vx_key(x, sg.o, sg.h, &ok);
    uint32_t at = VX_NONE;
    if (ok) {
      uint32_t s = vx_home(key, cap);
      for (uint32_t probe = 0; probe < cap; ++probe) {      // (ends long before: the table is at most half full)
        unsigned long long cur = vx_peek(&tkey[s]);
        if (cur == VX_EMPTY) cur = atomicCAS(&tkey[s], VX_EMPTY, key);
        if (cur == VX_EMPTY || cur == key) {
          at = s;
          break;
        }
        s = s + 1u == cap ? 0u : s + 1u;
      }
    }
    w.slot[g] = at;
    if (at == VX_NONE) {
      out = 1;
      continue;
    }
    const size_t t = base + at;
    atomicMin(&w.first[t], (uint32_t)i);
    atomicAdd(&w.count[t], 1u);
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicAdd(&w.U[3 * t + a], vx_quantise(x[a], sg.lo[a], sg.shift));
  }
  if (__syncthreads_or(out) && threadIdx.x == 0) atomicOr(&w.flag[c], VX_RANGE);
}

// Is point i (slot at) the head of its voxel?
__device__ static inline int vx_is_head(const VxWs& w, size_t base, uint32_t at, int i) {
  return at != VX_NONE && w.first[base + at] == (uint32_t)i;
}

__global__ __launch_bounds__(VX_LANES) void pn_voxel_heads_kernel(const int* __restrict__ off,
                                                                  const float* __restrict__ voxel, VxWs w) {
  __shared__ int sh[VX_WAVES];
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0) return;
  if (vx_status(w.flag[c], voxel[c]) != 0) return;                                    // (tile_heads stays 0)
  const int o0 = off[c], n = off[c + 1] - o0, first = w.tile_first[blockIdx.x];
  const size_t base = 2 * (size_t)o0;
  int count = 0;                                                              // of this wave: the same in all its lanes
#pragma unroll
  for (int p = 0; p < VX_PER_LANE; ++p) {
    const int i = first + p * VX_LANES + (int)threadIdx.x;
    const int head = i < n ? vx_is_head(w, base, w.slot[(size_t)o0 + i], i) : 0;
    count += __popcll(__ballot(head));
  }
  if (pn_lane() == 0) sh[threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x == 0) w.tile_heads[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// One workgroup per cloud: tile_heads becomes the exclusive sum over the cloud's tiles, nvox the total or the status.
__global__ __launch_bounds__(VX_LANES) void pn_voxel_scan_kernel(const int* __restrict__ off, int total,
                                                                 const float* __restrict__ voxel, VxWs w,
                                                                 int32_t* __restrict__ nvox) {
  __shared__ int waves[VX_WAVES];
  const int c = blockIdx.x;
  const int o0 = off[c], o1 = off[c + 1];
  if (!rg_valid_segment(o0, o1, total)) {
    if (threadIdx.x == 0) nvox[c] = 0;
    return;
  }
  const int status = vx_status(w.flag[c], voxel[c]);
  if (status != 0) {
    if (threadIdx.x == 0) nvox[c] = status;
    return;
  }
  const int nt = vx_cloud_tiles(o1 - o0);
  int* heads = w.tile_heads + vx_tile_base(o0, c);
  const int lane = pn_lane(), wave = threadIdx.x >> 6;
  int carry = 0;
  for (int t0 = 0; t0 < nt; t0 += VX_LANES) {
    const int t = t0 + (int)threadIdx.x;
    const int v = t < nt ? heads[t] : 0;
    int incl = v;                                                             // inclusive sum over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(incl, d, 64);
      if (lane >= d) incl += u;
    }
    if (lane == 63) waves[wave] = incl;
    __syncthreads();
    int before = carry;
    for (int v2 = 0; v2 < wave; ++v2) before += waves[v2];
    if (t < nt) heads[t] = before + incl - v;
    carry += ((waves[0] + waves[1]) + waves[2]) + waves[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) nvox[c] = carry;
}

__global__ __launch_bounds__(VX_LANES) void pn_voxel_rows_kernel(const int* __restrict__ off,
                                                                 const float* __restrict__ voxel,
                                                                 const float* __restrict__ origin, VxWs w,
                                                                 const int32_t* __restrict__ nvox,
                                                                 int32_t* __restrict__ owner,
                                                                 float* __restrict__ centroid,
                                                                 int32_t* __restrict__ count,
                                                                 int32_t* __restrict__ first_out,
                                                                 int32_t* __restrict__ rep) {
  __shared__ unsigned runs[VX_PER_LANE * VX_WAVES];
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0) return;
  const int o0 = off[c], n = off[c + 1] - o0, first = w.tile_first[blockIdx.x];
  const int V = nvox[c];
  const size_t base = 2 * (size_t)o0;
  const int wave = threadIdx.x >> 6;
  int head[VX_PER_LANE];
  uint32_t at[VX_PER_LANE];
  unsigned long long ballot[VX_PER_LANE];
#pragma unroll
  for (int p = 0; p < VX_PER_LANE; ++p) {
    const int i = first + p * VX_LANES + (int)threadIdx.x;
    at[p] = i < n && V >= 0 ? w.slot[(size_t)o0 + i] : VX_NONE;
    head[p] = i < n && V >= 0 ? vx_is_head(w, base, at[p], i) : 0;
    ballot[p] = __ballot(head[p]);
    if (pn_lane() == 0) runs[p * VX_WAVES + wave] = (unsigned)__popcll(ballot[p]);
  }
  __syncthreads();
  const VxSeg sg = vx_segment(w, c, voxel, origin);
  const unsigned before = (unsigned)w.tile_heads[blockIdx.x];
#pragma unroll
  for (int p = 0; p < VX_PER_LANE; ++p) {
    const int i = first + p * VX_LANES + (int)threadIdx.x;
    if (i >= n) continue;
    const size_t g = (size_t)o0 + i;
    if (V < 0) owner[g] = -1;
    if (i >= V) {                                       // (V < 0: every row)
      if (centroid) centroid[3 * g] = centroid[3 * g + 1] = centroid[3 * g + 2] = __builtin_nanf("");
      if (count) count[g] = -1;
      if (first_out) first_out[g] = -1;
      if (rep) rep[g] = -1;
    }
    if (!head[p]) continue;
    unsigned v = before + (unsigned)pn_mbcnt(ballot[p]);
    for (int r = 0; r < p * VX_WAVES + wave; ++r) v += runs[r];
    if (v >= (unsigned)V) continue;                     // (never, unless off changed under the launches)
    owner[g] = (int32_t)v;
    const size_t t = base + at[p], row = (size_t)o0 + v;
    const uint32_t cnt = w.count[t];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float m = vx_centroid(sg.lo[a], w.U[3 * t + a], cnt, sg.shift);
      w.cent[3 * row + a] = m;
      if (centroid) centroid[3 * row + a] = m;
    }
    if (count) count[row] = (int32_t)cnt;
    if (first_out) first_out[row] = i;
  }
}

__global__ __launch_bounds__(VX_LANES) void pn_voxel_owner_kernel(const float* __restrict__ pts,
                                                                  const int* __restrict__ off, VxWs w,
                                                                  const int32_t* __restrict__ nvox,
                                                                  int32_t* __restrict__ owner, int want_rep) {
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0) return;
  const int V = nvox[c];
  if (V < 0) return;
  const int o0 = off[c], n = off[c + 1] - o0, first = w.tile_first[blockIdx.x];
  const size_t base = 2 * (size_t)o0;
#pragma unroll
  for (int p = 0; p < VX_PER_LANE; ++p) {
    const int i = first + p * VX_LANES + (int)threadIdx.x;
    if (i >= n) continue;
    const size_t g = (size_t)o0 + i;
    const uint32_t at = w.slot[g];
    if (at == VX_NONE) continue;                        // (never: V >= 0)
    const uint32_t f = w.first[base + at];
    if (f >= (uint32_t)n) continue;                     // (never)
    const int v = owner[(size_t)o0 + f];                // the head's entry: written by launch 5, by nobody here
    if (f != (uint32_t)i) owner[g] = v;
    if (!want_rep || v < 0 || v >= V) continue;
    const size_t row = (size_t)o0 + v;
    const float d = kg_dist(pts[3 * g], pts[3 * g + 1], pts[3 * g + 2], w.cent[3 * row], w.cent[3 * row + 1],
                            w.cent[3 * row + 2]);
    const unsigned long long key = vx_rep_key(d, (uint32_t)i);
    if (key < vx_peek(&w.repkey[row])) atomicMin(&w.repkey[row], key);
  }
}

__global__ __launch_bounds__(VX_LANES) void pn_voxel_rep_kernel(const int* __restrict__ off, VxWs w,
                                                                const int32_t* __restrict__ nvox,
                                                                int32_t* __restrict__ rep) {
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0) return;
  const int V = nvox[c];
  const int o0 = off[c], n = off[c + 1] - o0, first = w.tile_first[blockIdx.x];
#pragma unroll
  for (int p = 0; p < VX_PER_LANE; ++p) {
    const int i = first + p * VX_LANES + (int)threadIdx.x;
    if (i >= n || i >= V) continue;
    const uint32_t r = vx_rep_index(w.repkey[(size_t)o0 + i]);
    rep[(size_t)o0 + i] = r < (uint32_t)n ? (int32_t)r : -1;
  }
}

extern "C" long long pn_voxel_workspace_bytes(long long total, int S) {
  if (total < 0 || total >= (1ll << 31) || S < 0) return 0;
  VxWs w;
  return vx_carve(nullptr, total, S, &w) + 16;
}

extern "C" int pn_voxel_launches(void) { return vx_launches(); }

extern "C" int pn_voxel_f32(const float* pts, const int* off, int S, int total, const float* voxel,
                            const float* origin, int32_t* owner, int32_t* nvox, float* centroid, int32_t* count,
                            int32_t* first, int32_t* rep, void* ws, long long ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "pn_voxel_f32";
  PN_CHECK_ARG(S >= 0, "%s: S=%d (S >= 0)", who, S);
  PN_CHECK_ARG(total >= 0, "%s: total=%d (0 <= total, below 2^31)", who, total);
  if (S == 0 || total == 0) return PN_OK;
  PN_CHECK_ARG(pts && off && voxel && owner && nvox && ws,
               "%s: null pointer (pts, off, voxel, owner, nvox and ws are required)", who);
  PN_CHECK_ARG(ws_bytes >= pn_voxel_workspace_bytes(total, S), "%s: workspace of %lld bytes (%lld)", who, ws_bytes,
               pn_voxel_workspace_bytes(total, S));
  VxWs w;
  vx_carve((void*)pn_align_up((size_t)ws, 16), total, S, &w);
  const dim3 block(VX_LANES), tiles((unsigned)vx_tiles(total, S)), clouds((unsigned)S);
  PN_CHECK_HIP(hipMemsetAsync(w.key, 0xff, (size_t)((char*)w.U - (char*)w.key), stream));
  PN_CHECK_HIP(hipMemsetAsync(w.U, 0, (size_t)((char*)w.cent - (char*)w.U), stream));
  PN_PROF("voxel", stream);
  hipLaunchKernelGGL(pn_voxel_bounds_kernel, tiles, block, 0, stream, pts, off, S, total, w);
  hipLaunchKernelGGL(pn_voxel_table_kernel, tiles, block, 0, stream, pts, off, voxel, origin, w);
  hipLaunchKernelGGL(pn_voxel_heads_kernel, tiles, block, 0, stream, off, voxel, w);
  hipLaunchKernelGGL(pn_voxel_scan_kernel, clouds, block, 0, stream, off, total, voxel, w, nvox);
  hipLaunchKernelGGL(pn_voxel_rows_kernel, tiles, block, 0, stream, off, voxel, origin, w, (const int32_t*)nvox, owner,
                     centroid, count, first, rep);
  hipLaunchKernelGGL(pn_voxel_owner_kernel, tiles, block, 0, stream, pts, off, w, (const int32_t*)nvox, owner,
                     rep ? 1 : 0);
  if (rep) hipLaunchKernelGGL(pn_voxel_rep_kernel, tiles, block, 0, stream, off, w, (const int32_t*)nvox, rep);
  PN_CHECK_LAUNCH();
  return PN_OK;
}
