// Consistent orientation of point normals without a viewpoint on clouds of ANY size, for gfx950: the definition and the
// outputs of pn_orient_normals_f32 (orient.hip, orient_math.h), bit for bit, with the Boruvka state in global memory and
// every step spread over many workgroups.  The per-element steps and the schedule with its bounds are
// orient_global_math.h, the same source the test suite compiles for the host.
//
// Workspace (pn_orient_normals_global_workspace_bytes, linear in total):
//   ctrl  OG_CTRL_WORDS words | best 8 total | P 4 total | H 4 total | seg 4 total
//   P[g]    parent LOCAL to the segment in the low 31 bits, parity to it in the top bit
//   best[g] smallest key offered to the root g this round; the seed keys in the tail
//   H[g]    the hook a root decided on, OG_NO_HOOK otherwise
//   seg[g]  the segment of point g (found once, by a search in off), -1 for a point no valid segment holds
// Launches, all stream-ordered, their number fixed by the host from max_n alone (og_launches); no cooperative launch,
// no grid-wide barrier, no kernel ever waits for another workgroup, every loop has a fixed cap:
//   init     seg, P[v] = v, best = no entry                                       (over points)
//   per round r = 0 .. og_rounds - 1:
//     offers   grid-stride over all (point, slot) entries of all segments, coalesced idx reads; an entry between two
//              components takes a 64-bit integer atomicMin of its key on both roots' slots, after a plain read (a
//              stale read is never below the slot: it only costs an atomic).  Integer minima do not depend on the
//              order of arrival: the round is deterministic.
//     hooks    every root with an entry writes its new word to H and raises any[r]; it reads P and best of other
//              roots, which nobody writes in this launch.
//     passes   og_passes compress launches.  The first reads a hooked root's word from H while P still shows it as a
//              root, stores the walked word over it, and resets best; the later ones read P alone.  A pass that moves
//              a word raises changed[r][p], and pass p + 1 exits at once when pass p raised nothing (every vertex then
//              points at its root).
//   Every launch of round r after the hooks exits in its first instructions when any[r] is not raised, and every
//   launch of a later round when any[r - 1] is not: once no component found an entry the rest of the schedule is idle.
//   tail     best = 0 (a memset); a 64-bit atomicMax of om_zkey per root; then flip = par(v) ^ par(seed) ^
//            om_seed_flip(n_z(seed)) and plain vector stores of normals, flip and seed.
// Visibility: a launch reads what earlier launches wrote (stream order).  Inside a launch only the compress passes read
// words that the same launch writes, and og_walk is correct for any mix of old and new words.
// Block size and entries per lane: 256 threads and at most OG_MAX_BLOCKS workgroups (16 waves per CU, enough loads in
// flight to cover the dependent P[j] read behind each idx read); a lane strides by OG_STRIDE over what is left.  The
// cost of the 64-bit atomics is bounded by the plain read in front of them: after the first offers to a root only
// lower keys reach the atomic unit.
#include "common.h"
#include "orient_global_math.h"
#include "ragged.h"

struct OgWs {
  uint32_t* ctrl;
  unsigned long long* best;
  uint32_t* P;
  uint32_t* H;
  int* seg;
};

// The arrays of the workspace in order, cut from `base` (0: measure only); returns their bytes.
static long long og_carve(void* base, long long total, OgWs* w) {
  RgCarver c = {(uintptr_t)base, 0};
  w->ctrl = c.take<uint32_t>(OG_CTRL_WORDS);
  w->best = c.take<unsigned long long>(total);
  w->P = c.take<uint32_t>(total);
  w->H = c.take<uint32_t>(total);
  w->seg = c.take<int>(total);
  return c.bytes;
}

// The segment of point g: the last s with off[s] <= g, accepted only if g lies inside a segment inside 0 .. total.
__device__ static inline int og_find_segment(const int* __restrict__ off, int S, int total, int g) {
  const int s = rg_row_segment(off, S, g);
  return rg_segment_holds(off[s], off[s + 1], total, g) ? s : -1;
}

__global__ __launch_bounds__(OG_BLOCK) void pn_orient_global_init_kernel(const int* __restrict__ off, int S, int total,
                                                                         OgWs w) {
  for (long long t = (long long)blockIdx.x * OG_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * OG_BLOCK) {
    const int g = (int)t;                                              // (t itself may pass 2^31 on its last step)
    const int s = og_find_segment(off, S, total, g);
    w.seg[g] = s;
    w.P[g] = s >= 0 ? (uint32_t)(g - off[s]) : 0u;
    w.H[g] = OG_NO_HOOK;
    w.best[g] = OM_NO_ENTRY;
  }
}

__global__ __launch_bounds__(OG_BLOCK) void pn_orient_global_offer_kernel(
    const int* __restrict__ off, int total, const int* __restrict__ idx, int k, const float* __restrict__ nin, int round,
    OgWs w) {
  if (round > 0 && w.ctrl[OG_CTRL_ANY + round - 1] == 0) return;
  const int E = total * k;                                             // < 2^31 (checked by the host)
  for (long long e = (long long)blockIdx.x * OG_BLOCK + threadIdx.x; e < E; e += (long long)gridDim.x * OG_BLOCK) {
    const int g = (int)(e / k), s = (int)(e - (long long)g * k);
    const int sg = w.seg[g];
    if (sg < 0) continue;
    const int o0 = off[sg], n = off[sg + 1] - o0;
    uint32_t ci, cj;
    unsigned long long key;
    if (!og_offer(w.P + o0, nin + 3 * (size_t)o0, n, k, g - o0, s, idx[e], &ci, &cj, &key)) continue;
    unsigned long long* best = w.best + o0;
    if (key < best[ci]) atomicMin(&best[ci], key);
    if (key < best[cj]) atomicMin(&best[cj], key);
  }
}

__global__ __launch_bounds__(OG_BLOCK) void pn_orient_global_hook_kernel(
    const int* __restrict__ off, int total, const int* __restrict__ idx, int k, const float* __restrict__ nin, int round,
    OgWs w) {
  if (round > 0 && w.ctrl[OG_CTRL_ANY + round - 1] == 0) return;
  int any = 0;
  for (long long t = (long long)blockIdx.x * OG_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * OG_BLOCK) {
    const int g = (int)t;                                              // (t itself may pass 2^31 on its last step)
    const int sg = w.seg[g];
    if (sg < 0) continue;
    const int o0 = off[sg];
    const uint32_t v = (uint32_t)(g - o0);
    uint32_t h = OG_NO_HOOK;
    if (w.P[g] == v)
      h = og_hook(w.P + o0, w.best + o0, idx + (size_t)o0 * k, nin + 3 * (size_t)o0, k, v, &any);
    w.H[g] = h;
  }
  if (__syncthreads_or(any) && threadIdx.x == 0) atomicOr(&w.ctrl[OG_CTRL_ANY + round], 1u);
}

__global__ __launch_bounds__(OG_BLOCK) void pn_orient_global_compress_kernel(const int* __restrict__ off, int total,
                                                                             int round, int pass, OgWs w) {
  if (w.ctrl[OG_CTRL_ANY + round] == 0) return;
  uint32_t* changed = w.ctrl + OG_CTRL_CHANGED + round * OG_MAX_PASSES;
  if (pass > 0 && changed[pass - 1] == 0) return;
  const int first = pass == 0;
  int moved = 0;
  for (long long t = (long long)blockIdx.x * OG_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * OG_BLOCK) {
    const int g = (int)t;                                              // (t itself may pass 2^31 on its last step)
    const int sg = w.seg[g];
    if (sg < 0) continue;
    const int o0 = off[sg];
    const uint32_t old = w.P[g];
    const uint32_t now = og_walk(w.P + o0, w.H + o0, (uint32_t)(g - o0), first);
    if (now != old) {
      w.P[g] = now;
      moved = 1;
    }
    if (first) w.best[g] = OM_NO_ENTRY;
  }
  if (__syncthreads_or(moved) && threadIdx.x == 0) atomicOr(&changed[pass], 1u);
}

__global__ __launch_bounds__(OG_BLOCK) void pn_orient_global_seedkey_kernel(const float* __restrict__ pts,
                                                                            const int* __restrict__ off, int total,
                                                                            OgWs w) {
  for (long long t = (long long)blockIdx.x * OG_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * OG_BLOCK) {
    const int g = (int)t;                                              // (t itself may pass 2^31 on its last step)
    const int sg = w.seg[g];
    if (sg < 0) continue;
    const int o0 = off[sg];
    const uint32_t r = w.P[g] & ~OM_PARITY;
    const unsigned long long zk = om_zkey(pts[3 * (size_t)g + 2], (uint32_t)(g - o0));
    unsigned long long* slot = w.best + o0 + r;
    if (zk > *slot) atomicMax(slot, zk);
  }
}

__global__ __launch_bounds__(OG_BLOCK) void pn_orient_global_output_kernel(
    const int* __restrict__ off, int total, const float* __restrict__ nin, OgWs w, float* __restrict__ nout,
    int* __restrict__ flip, int* __restrict__ seed) {
  for (long long t = (long long)blockIdx.x * OG_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * OG_BLOCK) {
    const int g = (int)t;                                              // (t itself may pass 2^31 on its last step)
    const int sg = w.seg[g];
    if (sg < 0) {                                                      // offsets that do not hold the point: loud
      nout[3 * (size_t)g] = nout[3 * (size_t)g + 1] = nout[3 * (size_t)g + 2] = __builtin_nanf("");
      if (flip) flip[g] = -1;
      if (seed) seed[g] = -1;
      continue;
    }
    const int o0 = off[sg], n = off[sg + 1] - o0;
    const uint32_t v = (uint32_t)(g - o0), wv = w.P[g];
    uint32_t sd = om_zkey_vertex(w.best[o0 + (wv & ~OM_PARITY)]);      // a vertex of this component: below n
    if (sd >= (uint32_t)n) sd = v;                                     // (only if max_n was below the largest segment)
    const int f = (int)((wv ^ w.P[o0 + sd]) >> 31) ^ om_seed_flip(nin[3 * ((size_t)o0 + sd) + 2]);
    nout[3 * (size_t)g] = om_apply(nin[3 * (size_t)g], f);
    nout[3 * (size_t)g + 1] = om_apply(nin[3 * (size_t)g + 1], f);
    nout[3 * (size_t)g + 2] = om_apply(nin[3 * (size_t)g + 2], f);
    if (flip) flip[g] = f;
    if (seed) seed[g] = (int)sd;
  }
}

extern "C" long long pn_orient_normals_global_workspace_bytes(long long total, int S) {
  if (total < 0 || S < 0) return 0;
  OgWs w;
  return og_carve(nullptr, total, &w) + 16;
}

extern "C" int pn_orient_normals_global_launches(int max_n) { return og_launches(max_n < 0 ? 0 : max_n); }

extern "C" int pn_orient_normals_global_f32(const float* pts, const int* off, int S, int total, int max_n,
                                            const int32_t* idx, int k, const float* normals_in, float* normals_out,
                                            int32_t* flip, int32_t* seed, void* ws, long long ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "pn_orient_normals_global_f32";
  PN_CHECK_ARG(k >= OM_MIN_K && k <= OM_MAX_K, "%s: k=%d (%d <= k <= %d)", who, k, OM_MIN_K, OM_MAX_K);
  PN_CHECK_ARG(S >= 0 && total >= 0 && max_n >= 0, "%s: S=%d total=%d max_n=%d", who, S, total, max_n);
  PN_CHECK_ARG((long long)total * k < (1ll << 31), "%s: total * k = %lld (below 2^31)", who, (long long)total * k);
  if (total == 0 || S == 0) return PN_OK;
  PN_CHECK_ARG(pts && off && idx && normals_in && normals_out && ws, "%s: null pointer", who);
  PN_CHECK_ARG(normals_in != normals_out, "%s: normals_out must not be normals_in", who);
  PN_CHECK_ARG(ws_bytes >= pn_orient_normals_global_workspace_bytes(total, S), "%s: workspace of %lld bytes (%lld)", who,
               ws_bytes, pn_orient_normals_global_workspace_bytes(total, S));
  OgWs w;
  og_carve((void*)pn_align_up((size_t)ws, 16), total, &w);
  const int rounds = og_rounds(max_n), passes = og_passes(max_n);
  const dim3 block(OG_BLOCK);
  const int vb = pn_cdiv(total, OG_BLOCK), eb = pn_cdiv((long long)total * k, OG_BLOCK);
  const dim3 vgrid(vb < OG_MAX_BLOCKS ? vb : OG_MAX_BLOCKS), egrid(eb < OG_MAX_BLOCKS ? eb : OG_MAX_BLOCKS);
  PN_CHECK_HIP(hipMemsetAsync(w.ctrl, 0, (size_t)OG_CTRL_WORDS * 4, stream));
  PN_PROF("orient_normals_global", stream);
  hipLaunchKernelGGL(pn_orient_global_init_kernel, vgrid, block, 0, stream, off, S, total, w);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(pn_orient_global_offer_kernel, egrid, block, 0, stream, off, total, idx, k, normals_in, r, w);
    hipLaunchKernelGGL(pn_orient_global_hook_kernel, vgrid, block, 0, stream, off, total, idx, k, normals_in, r, w);
    for (int p = 0; p < passes; ++p)
      hipLaunchKernelGGL(pn_orient_global_compress_kernel, vgrid, block, 0, stream, off, total, r, p, w);
  }
  PN_CHECK_HIP(hipMemsetAsync(w.best, 0, (size_t)8 * total, stream));
  hipLaunchKernelGGL(pn_orient_global_seedkey_kernel, vgrid, block, 0, stream, pts, off, total, w);
  hipLaunchKernelGGL(pn_orient_global_output_kernel, vgrid, block, 0, stream, off, total, normals_in, w, normals_out,
                     flip, seed);
  PN_CHECK_LAUNCH();
  return PN_OK;
}
