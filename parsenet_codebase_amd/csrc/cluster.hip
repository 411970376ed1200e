// Euclidean cluster extraction of a ragged batch of 3-D clouds of ANY size, for gfx950: the connected components of the
// graph "no further apart than the radius", numbered by their lowest point, under the definition of cluster_math.h —
// the same source the test suite compiles for the host.  The neighbour search is the exact uniform-grid search of
// knn3_grid_math.h (cell function and bound as they stand, the resolution chosen from the radius); the merge is the
// Boruvka engine of orient_global.hip without the parities, on the schedule the two share (boruvka_schedule.h).
//
// The grid build is NOT shared with knn3_grid.hip: its four kernels derive the grid from a points-per-cell number,
// these derive it from the radius of the segment (cl_grid), and they also set up the merge.  knn3_grid.hip is untouched.
//
// Workspace (pn_cluster_workspace_bytes, linear in total): 56 total + 36 S + 4 CL_CTRL_WORDS + 16
//   ctrl  CL_CTRL_WORDS words, FIRST in the (16-byte aligned) workspace: any[r] at word r — a root found an entry in
//         round r —, changed[r][p] at CL_CTRL_CHANGED + r CL_MAX_PASSES + p                              memset 0
//   rec 16 total | best 8 total | first 4 total | bmin 12 S                      best .. bmin: one memset 0xff
//   cnt 4 total | start 4 (total + 2 S) | bmax 12 S | flag 4 S                   one memset 0
//   pcell, prank, P, H, seg 4 total each
//   rec[p]   (x, y, z, LOCAL index) of the points in cell order; segment s owns the records off[s] .. off[s + 1] - 1 and
//            the cell slots [off[s] + 2 s, off[s + 1] + 2 s + 2): at most max(1, n_s) cells and the end sentinel
//   P[g]     parent LOCAL to the segment; H[g] the hook a root decided on, CL_NO_HOOK otherwise
//   best[g]  the least key offered to the root g this round;  cnt[g], first[g]  size and lowest index of the component
//            with root g;  seg[g]  the segment of point g, -1 for a point that no valid segment holds
// Launches, all stream-ordered, their number fixed by the host from max_n alone (cl_launches); no cooperative launch, no
// grid-wide barrier, no kernel ever waits for another workgroup, every loop has a fixed cap:
//   bounds   min / max per axis and segment, the non-finite flag; seg and P[v] = v of every point
//   cells, scan, scatter   the cell of every point and its rank, the cell starts, the records (as in knn3_grid.hip)
//   per round r = 0 .. cl_rounds - 1:
//     offers   one wave per record: ring by ring the rows of the shell are handed out one per lane, a batch of 64
//              records is one 16-byte load per lane; a lane keeps the least key among its edges to another component.
//              ONE 64-bit atomicMin per wave, on the query's own root, behind a plain read (a stale read is never below
//              the slot: it only costs the atomic).  Integer minima do not depend on the order of arrival.
//     hooks    every root with an entry writes its new parent to H and raises any[r]
//     passes   cl_passes compress launches; the first reads a hooked root's word from H, stores the walked word and
//              resets best; a pass that moves a word raises changed[r][p], pass p + 1 exits when pass p raised nothing
//   Every launch of round r after the hooks exits at once when any[r] is not raised, every launch of a later round when
//   any[r - 1] is not: once no component found an entry the rest of the schedule is idle.
//   sizes    integer atomicAdd / atomicMin on the root, one per run of lanes of a wave that share the root
//   numbers  one workgroup per segment: the kept heads (lowest points of components of min_size points or more) in
//            ascending order get 0 .. C-1 by a scan; label of the heads, the rows of count and first, ncomp, ndrop; a
//            segment with a status: label, count, first -1 throughout
//   labels   every other point takes the label of its head (written by the launch before, by nobody in this one)
// Every store is a plain vector store or an integer atomic.
//
// Resource report of hipcc --offload-arch=gfx950 -O3 (-Rpass-analysis=kernel-resource-usage):
//   pn_cluster_offer_kernel  VGPRs: 66  TotalSGPRs: 43  ScratchSize [bytes/lane]: 0  Occupancy [waves/SIMD]: 7
//                            LDS Size [bytes/block]: 0 — no spill
//   bounds 27 / cells 30 / scan 35 / scatter 18 / hook 22 / compress 24 / sizes 12 / numbers 38 / labels 14 VGPRs,
//   ScratchSize 0 for all nine, 8 waves/SIMD
#include "common.h"
#include "cluster_math.h"
#include "ragged.h"

#define CL_BLOCK 256                    // threads per workgroup of the per-point kernels
#define CL_MAX_BLOCKS 1024              // workgroups per launch at most; a lane strides over what is left
#define CL_ROWS_PER_WAVE 512            // bounds: rows one wave reduces before its six atomics
#define CL_SCAN 1024                    // threads of the one-workgroup-per-segment kernels
#define CL_SHARE_TRIES 4                // sizes: runs of lanes that share a root served by one atomic each

struct ClWs {
  uint32_t* ctrl;
  float4* rec;
  unsigned long long* best;
  uint32_t* first;
  uint32_t* bmin;
  uint32_t* cnt;
  int* start;
  uint32_t* bmax;
  uint32_t* flag;
  int* pcell;
  int* prank;
  uint32_t* P;
  uint32_t* H;
  int* seg;
};

// The arrays of the workspace in order, cut from `base` (0: measure only); returns their bytes.
static long long cl_carve(void* base, long long total, long long S, ClWs* w) {
  RgCarver c = {(uintptr_t)base, 0};
  w->ctrl = c.take<uint32_t>(CL_CTRL_WORDS);          // (a multiple of 16 bytes)
  w->rec = c.take<float4>(total);
  w->best = c.take<unsigned long long>(total);        // (the 0xff memset starts here)
  w->first = c.take<uint32_t>(total);
  w->bmin = c.take<uint32_t>(3 * S);
  w->cnt = c.take<uint32_t>(total);                   // (the zero memset starts here)
  w->start = c.take<int>(total + 2 * S);
  w->bmax = c.take<uint32_t>(3 * S);
  w->flag = c.take<uint32_t>(S);
  w->pcell = c.take<int>(total);                      // (and ends here)
  w->prank = c.take<int>(total);
  w->P = c.take<uint32_t>(total);
  w->H = c.take<uint32_t>(total);
  w->seg = c.take<int>(total);
  return c.bytes;
}

__device__ static inline KgGrid cl_segment_grid(const ClWs& w, int s, int n, float r) {
  float lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = pn_ord2f(w.bmin[3 * s + a]);
    hi[a] = pn_ord2f(w.bmax[3 * s + a]);
  }
  return cl_grid(n, lo, hi, r);
}

// ---- bounding boxes, flags, the segment and the parent of every point ---------------------------------------------------
__global__ __launch_bounds__(256) void pn_cluster_bounds_kernel(const float* __restrict__ pts,
                                                                const int* __restrict__ off, int S, int total,
                                                                ClWs w) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long first = wave * CL_ROWS_PER_WAVE;
  if (first >= total) return;
  const int last = (int)(first + CL_ROWS_PER_WAVE - 1 < total - 1 ? first + CL_ROWS_PER_WAVE - 1 : total - 1);
  const int s0 = rg_row_segment(off, S, (int)first), s1 = rg_row_segment(off, S, last);
  const int b0 = off[s0], e0 = off[s0 + 1];
  const bool one = s0 == s1 && rg_segment_holds(b0, e0, total, (int)first) && last < e0;      // (uniform over the wave)
  uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u}, bad = 0u;
  for (int row = (int)first + lane; row <= last; row += 64) {
    uint32_t o[3];
    uint32_t nf = 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float x = pts[(size_t)row * 3 + a];
      nf |= kg_finite(x) ? 0u : 1u;
      o[a] = pn_f2ord(x);
    }
    if (one) {
      w.seg[row] = s0;
      w.P[row] = (uint32_t)(row - b0);
      bad |= nf;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        mn[a] = o[a] < mn[a] ? o[a] : mn[a];
        mx[a] = o[a] > mx[a] ? o[a] : mx[a];
      }
    } else {
      const int s = rg_row_segment(off, S, row);
      const int o0 = off[s];
      if (!rg_segment_holds(o0, off[s + 1], total, row)) {      // (offsets that do not cover the row: no segment)
        w.seg[row] = -1;
        w.P[row] = 0u;
        continue;
      }
      w.seg[row] = s;
      w.P[row] = (uint32_t)(row - o0);
      if (nf) atomicOr(&w.flag[s], 1u);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        atomicMin(&w.bmin[3 * s + a], o[a]);
        atomicMax(&w.bmax[3 * s + a], o[a]);
      }
    }
  }
  if (!one) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mn[a] = pn_wave_min_u32(mn[a]);
    mx[a] = pn_wave_max_u32(mx[a]);
  }
  bad = __ballot(bad != 0u) != 0ull ? 1u : 0u;
  if (lane == 0) {
    if (bad) atomicOr(&w.flag[s0], 1u);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&w.bmin[3 * s0 + a], mn[a]);
      atomicMax(&w.bmax[3 * s0 + a], mx[a]);
    }
  }
}

// ---- the cell of every point, the histogram and the point's rank in its cell ---------------------------------------------
__global__ __launch_bounds__(CL_BLOCK) void pn_cluster_cells_kernel(const float* __restrict__ pts,
                                                                    const int* __restrict__ off, int total,
                                                                    const float* __restrict__ radius, ClWs w) {
  for (long long t = (long long)blockIdx.x * CL_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * CL_BLOCK) {
    const int row = (int)t;                                            // (t itself may pass 2^31 on its last step)
    const int s = w.seg[row];
    w.pcell[row] = -1;
    if (s < 0) continue;
    const float r = radius[s];
    if (cl_status(w.flag[s], r) != 0) continue;
    const int o0 = off[s], n = off[s + 1] - o0;
    const KgGrid g = cl_segment_grid(w, s, n, r);
    const int cell = kg_cell_index(g, kg_cell(g, 0, pts[(size_t)row * 3]), kg_cell(g, 1, pts[(size_t)row * 3 + 1]),
                                   kg_cell(g, 2, pts[(size_t)row * 3 + 2]));
    if ((unsigned)cell >= (unsigned)(n > 1 ? n : 1)) continue;         // (never: at most max(1, n) cells)
    w.pcell[row] = cell;
    w.prank[row] = atomicAdd(&w.start[(size_t)o0 + 2 * (size_t)s + cell], 1);
  }
}

// ---- exclusive scan of a segment's histogram to record positions ------------------------------------------------------
__global__ __launch_bounds__(CL_SCAN) void pn_cluster_scan_kernel(const int* __restrict__ off, int total,
                                                                  const float* __restrict__ radius, ClWs w) {
  __shared__ int s_wave[16];
  __shared__ int s_carry;
  const int s = blockIdx.x;
  const int o0 = off[s], o1 = off[s + 1], n = o1 - o0;
  if (!rg_valid_segment(o0, o1, total) || n <= 0 || cl_status(w.flag[s], radius[s]) != 0) return;
  const KgGrid g = cl_segment_grid(w, s, n, radius[s]);
  const int ncell = kg_cells(g);                                     // <= n
  if (ncell > n) return;                                             // (never)
  int* __restrict__ st = w.start + (size_t)o0 + 2 * (size_t)s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_carry = o0;
  __syncthreads();
  for (int base = 0; base < ncell; base += 4 * CL_SCAN) {
    const int c0 = base + 4 * (int)threadIdx.x;
    int v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = c0 + e < ncell ? st[c0 + e] : 0;
    const int mine = (v[0] + v[1]) + (v[2] + v[3]);
    int inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = s_carry, all = 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      before += u < wave ? s_wave[u] : 0;
      all += s_wave[u];
    }
    int run = before + inc - mine;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c0 + e < ncell) st[c0 + e] = run;
      run += v[e];
    }
    __syncthreads();
    if (threadIdx.x == 0) s_carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) st[ncell] = s_carry;                         // the end of the last cell: off[s + 1]
}

// ---- the records in cell order -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(CL_BLOCK) void pn_cluster_scatter_kernel(const float* __restrict__ pts,
                                                                      const int* __restrict__ off, int total, ClWs w) {
  for (long long t = (long long)blockIdx.x * CL_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * CL_BLOCK) {
    const int row = (int)t;
    const int cell = w.pcell[row];
    if (cell < 0) continue;
    const int s = w.seg[row];
    const int o0 = off[s], o1 = off[s + 1];
    const int pos = w.start[(size_t)o0 + 2 * (size_t)s + cell] + w.prank[row];
    if (pos < o0 || pos >= o1) continue;                               // (cannot happen; never write out of the segment)
    w.rec[pos] = make_float4(pts[(size_t)row * 3], pts[(size_t)row * 3 + 1], pts[(size_t)row * 3 + 2],
                             __int_as_float(row - o0));
  }
}

// ---- offers: the ball of every point -------------------------------------------------------------------------------------
// One batch: the records [p, min(p + 64, end)) against the query; the lane's least key to another component.
__device__ static inline void cl_batch(const float4* __restrict__ rec, const uint32_t* __restrict__ P, int p, int end,
                                       float qx, float qy, float qz, float r2, int n, int self, uint32_t ci,
                                       unsigned long long& key) {
  const int lane = threadIdx.x & 63;
  if (p + lane >= end) return;
  const float4 c = rec[p + lane];
  const int j = __float_as_int(c.w);
  if ((unsigned)j >= (unsigned)n || j == self) return;
  if (!cl_is_edge(kg_dist(qx, qy, qz, c.x, c.y, c.z), r2)) return;
  if (P[j] == ci) return;
  const unsigned long long k = cl_key((uint32_t)self, (uint32_t)j);
  key = k < key ? k : key;
}

__global__ __launch_bounds__(256) void pn_cluster_offer_kernel(const int* __restrict__ off, int total,
                                                               const float* __restrict__ radius, int round, ClWs w) {
  if (round > 0 && w.ctrl[CL_CTRL_ANY + round - 1] == 0) return;
  const int lane = threadIdx.x & 63;
  const long long p64 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p64 >= total) return;
  const int p = (int)p64;
  const int s = w.seg[p];                                            // the records of a segment stand in its own rows
  if (s < 0) return;
  const float rad = radius[s];
  if (cl_status(w.flag[s], rad) != 0) return;                        // (no records were written)
  const int o0 = off[s], o1 = off[s + 1], n = o1 - o0;
  const float4 me = w.rec[p];
  const int self = __float_as_int(me.w);
  if ((unsigned)self >= (unsigned)n) return;
  const uint32_t* __restrict__ P = w.P + o0;
  const uint32_t ci = P[self];
  if (ci >= (uint32_t)n) return;                                     // (never)
  const float r2 = cl_r2(rad);
  const KgGrid g = cl_segment_grid(w, s, n, rad);
  const float q[3] = {me.x, me.y, me.z};
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = kg_cell(g, a, q[a]);
  const int* __restrict__ st = w.start + (size_t)o0 + 2 * (size_t)s;
  const int rmax = max(g.dim[0], max(g.dim[1], g.dim[2]));          // the cube of ring rmax covers any grid
  unsigned long long key = CL_NO_ENTRY;
  for (int r = 0; r <= rmax; ++r) {
    // the rows (y, z) of the shell, clipped to the grid; a row on the rim of the square contributes its whole x range,
    // a row inside it the two cells at x = c - r and x = c + r
    const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.dim[1] - 1);
    const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.dim[2] - 1);
    const int ny = y1 - y0 + 1, rows = ny * (z1 - z0 + 1);
    const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.dim[0] - 1);
    for (int t0 = 0; t0 < rows; t0 += 64) {
      int b0 = 0, e0 = 0, b1 = 0, e1 = 0;
      const int t = t0 + lane;
      if (t < rows) {
        const int y = y0 + t % ny, z = z0 + t / ny;
        const int row = (z * g.dim[1] + y) * g.dim[0];
        const int dy = y - c[1], dz = z - c[2];
        if (max(dy < 0 ? -dy : dy, dz < 0 ? -dz : dz) == r) {
          b0 = st[row + x0];
          e0 = st[row + x1 + 1];
        } else {
          if (c[0] - r >= 0) {
            b0 = st[row + c[0] - r];
            e0 = st[row + c[0] - r + 1];
          }
          if (c[0] + r <= g.dim[0] - 1) {
            b1 = st[row + c[0] + r];
            e1 = st[row + c[0] + r + 1];
          }
        }
        b0 = max(b0, o0);      // (a range never leaves the segment's records, whatever the table holds)
        e0 = min(e0, o1);
        b1 = max(b1, o0);
        e1 = min(e1, o1);
      }
      unsigned long long m = __ballot(e0 > b0);
      while (m) {
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        const int b = __builtin_amdgcn_readlane(b0, l), e = __builtin_amdgcn_readlane(e0, l);
        for (int pp = b; pp < e; pp += 64) cl_batch(w.rec, P, pp, e, q[0], q[1], q[2], r2, n, self, ci, key);
      }
      m = __ballot(e1 > b1);
      while (m) {
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        const int b = __builtin_amdgcn_readlane(b1, l), e = __builtin_amdgcn_readlane(e1, l);
        for (int pp = b; pp < e; pp += 64) cl_batch(w.rec, P, pp, e, q[0], q[1], q[2], r2, n, self, ci, key);
      }
    }
    if (cl_stop(g, c, r, q, r2)) break;                              // (uniform over the wave)
  }
  key = pn_wave_min_u64(key);
  if (lane == 0 && key != CL_NO_ENTRY) {
    unsigned long long* slot = w.best + o0 + ci;
    if (key < *slot) atomicMin(slot, key);
  }
}

__global__ __launch_bounds__(CL_BLOCK) void pn_cluster_hook_kernel(const int* __restrict__ off, int total, int round,
                                                                   ClWs w) {
  if (round > 0 && w.ctrl[CL_CTRL_ANY + round - 1] == 0) return;
  int any = 0;
  for (long long t = (long long)blockIdx.x * CL_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * CL_BLOCK) {
    const int g = (int)t;
    const int sg = w.seg[g];
    if (sg < 0) continue;
    const int o0 = off[sg], n = off[sg + 1] - o0;
    const uint32_t v = (uint32_t)(g - o0);
    uint32_t h = CL_NO_HOOK;
    if (w.P[g] == v) h = cl_hook(w.P + o0, w.best + o0, n, v, &any);
    w.H[g] = h;
  }
  if (__syncthreads_or(any) && threadIdx.x == 0) atomicOr(&w.ctrl[CL_CTRL_ANY + round], 1u);
}

__global__ __launch_bounds__(CL_BLOCK) void pn_cluster_compress_kernel(const int* __restrict__ off, int total, int round,
                                                                       int pass, ClWs w) {
  if (w.ctrl[CL_CTRL_ANY + round] == 0) return;
  uint32_t* changed = w.ctrl + CL_CTRL_CHANGED + round * CL_MAX_PASSES;
  if (pass > 0 && changed[pass - 1] == 0) return;
  const int first = pass == 0;
  int moved = 0;
  for (long long t = (long long)blockIdx.x * CL_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * CL_BLOCK) {
    const int g = (int)t;
    const int sg = w.seg[g];
    if (sg < 0) continue;
    const int o0 = off[sg], n = off[sg + 1] - o0;
    const uint32_t old = w.P[g];
    const uint32_t now = cl_walk(w.P + o0, w.H + o0, n, (uint32_t)(g - o0), first);
    if (now != old) {
      w.P[g] = now;
      moved = 1;
    }
    if (first) w.best[g] = CL_NO_ENTRY;
  }
  if (__syncthreads_or(moved) && threadIdx.x == 0) atomicOr(&changed[pass], 1u);
}

// ---- sizes and lowest points of the components ----------------------------------------------------------------------------
__global__ __launch_bounds__(CL_BLOCK) void pn_cluster_sizes_kernel(const int* __restrict__ off, int total,
                                                                    const float* __restrict__ radius, ClWs w) {
  const int lane = threadIdx.x & 63;
  // (whole waves enter the loop together: the bound is rounded up to the wave, so that the ballots see all lanes)
  const long long end = ((long long)total + 63) / 64 * 64;
  for (long long t = (long long)blockIdx.x * CL_BLOCK + threadIdx.x; t < end; t += (long long)gridDim.x * CL_BLOCK) {
    long long slot = -1;                                               // the global row of the root, -1: nothing to add
    uint32_t i = 0u;
    if (t < total) {
      const int g = (int)t;
      const int sg = w.seg[g];
      if (sg >= 0 && cl_status(w.flag[sg], radius[sg]) == 0) {
        const int o0 = off[sg], n = off[sg + 1] - o0;
        const uint32_t root = w.P[g];
        if (root < (uint32_t)n) slot = (long long)o0 + root, i = (uint32_t)(g - o0);
      }
    }
    // lanes ascend with the point index: the first lane of a run that shares a root holds its lowest index
    for (int tries = 0; tries < CL_SHARE_TRIES; ++tries) {
      const unsigned long long active = __ballot(slot >= 0);
      if (active == 0ull) break;
      const int leader = __builtin_ctzll(active);
      const long long ls = ((long long)__builtin_amdgcn_readlane((int)(slot >> 32), leader) << 32) |
                           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)slot, leader);
      const unsigned long long share = __ballot(slot == ls);
      if (lane == leader) {
        atomicAdd(&w.cnt[ls], (uint32_t)__popcll(share));
        atomicMin(&w.first[ls], i);
      }
      if (slot == ls) slot = -1;
    }
    if (slot >= 0) {
      atomicAdd(&w.cnt[slot], 1u);
      atomicMin(&w.first[slot], i);
    }
  }
}

// ---- numbers: one workgroup per segment ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(CL_SCAN) void pn_cluster_numbers_kernel(const int* __restrict__ off, int total,
                                                                     const float* __restrict__ radius, int min_size,
                                                                     ClWs w, int32_t* __restrict__ label,
                                                                     int32_t* __restrict__ ncomp,
                                                                     int32_t* __restrict__ count,
                                                                     int32_t* __restrict__ first_out,
                                                                     int32_t* __restrict__ ndrop) {
  __shared__ int s_wave[16];
  __shared__ int s_points;
  const int s = blockIdx.x;
  const int o0 = off[s], o1 = off[s + 1];
  if (!rg_valid_segment(o0, o1, total)) {
    if (threadIdx.x == 0) {
      ncomp[s] = 0;
      if (ndrop) ndrop[s] = 0;
    }
    return;
  }
  const int n = o1 - o0;
  const int status = cl_status(w.flag[s], radius[s]);
  if (status != 0) {
    for (int i = threadIdx.x; i < n; i += CL_SCAN) {
      label[(size_t)o0 + i] = -1;
      if (count) count[(size_t)o0 + i] = -1;
      if (first_out) first_out[(size_t)o0 + i] = -1;
    }
    if (threadIdx.x == 0) {
      ncomp[s] = status;
      if (ndrop) ndrop[s] = n;
    }
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_points = 0;
  int carry = 0;                                                       // kept components before this chunk: uniform
  for (int base = 0; base < n; base += CL_SCAN) {
    const int i = base + (int)threadIdx.x;
    int head = 0, kept = 0;
    uint32_t size = 0u;
    if (i < n) {
      const uint32_t root = w.P[(size_t)o0 + i];
      if (root < (uint32_t)n) {
        head = w.first[(size_t)o0 + root] == (uint32_t)i;
        size = w.cnt[(size_t)o0 + root];
        kept = head && cl_kept(size, min_size);
      }
    }
    const unsigned long long b = __ballot(kept);
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int before = carry, all = 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      before += u < wave ? s_wave[u] : 0;
      all += s_wave[u];
    }
    if (kept) {
      const int c = before + pn_mbcnt(b);                              // <= i: the row is the segment's own
      label[(size_t)o0 + i] = c;
      if (count) count[(size_t)o0 + c] = (int32_t)size;
      if (first_out) first_out[(size_t)o0 + c] = i;
      atomicAdd(&s_points, (int)size);
    } else if (head) {
      label[(size_t)o0 + i] = -1;
    }
    carry += all;
    __syncthreads();
  }
  // (rows carry .. n - 1 were written by nobody above: a kept head writes row c <= carry - 1)
  for (int i = carry + (int)threadIdx.x; i < n; i += CL_SCAN) {
    if (count) count[(size_t)o0 + i] = -1;
    if (first_out) first_out[(size_t)o0 + i] = -1;
  }
  if (threadIdx.x == 0) {
    ncomp[s] = carry;
    if (ndrop) ndrop[s] = n - s_points;
  }
}

__global__ __launch_bounds__(CL_BLOCK) void pn_cluster_labels_kernel(const int* __restrict__ off, int total,
                                                                     const float* __restrict__ radius, int min_size,
                                                                     ClWs w, int32_t* label) {
  for (long long t = (long long)blockIdx.x * CL_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * CL_BLOCK) {
    const int g = (int)t;
    const int sg = w.seg[g];
    if (sg < 0 || cl_status(w.flag[sg], radius[sg]) != 0) continue;   // (a status: the launch before wrote -1)
    const int o0 = off[sg], n = off[sg + 1] - o0;
    const uint32_t root = w.P[g];
    if (root >= (uint32_t)n) continue;                                 // (never)
    const uint32_t f = w.first[(size_t)o0 + root];
    if (f >= (uint32_t)n || f == (uint32_t)(g - o0)) continue;         // the head: written by the launch before
    label[g] = cl_kept(w.cnt[(size_t)o0 + root], min_size) ? label[(size_t)o0 + f] : -1;
  }
}

extern "C" long long pn_cluster_workspace_bytes(long long total, int S) {
  if (total < 0 || total >= (1ll << 31) || S < 0) return 0;
  ClWs w;
  return cl_carve(nullptr, total, S, &w) + 16;
}

extern "C" int pn_cluster_launches(int max_n) { return cl_launches(max_n < 0 ? 0 : max_n); }

extern "C" int pn_cluster_f32(const float* pts, const int* off, int S, int total, int max_n, const float* radius,
                              int min_size, int32_t* label, int32_t* ncomp, int32_t* count, int32_t* first,
                              int32_t* ndrop, void* ws, long long ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "pn_cluster_f32";
  PN_CHECK_ARG(S >= 0, "%s: S=%d (S >= 0)", who, S);
  PN_CHECK_ARG(total >= 0, "%s: total=%d (0 <= total, below 2^31)", who, total);
  PN_CHECK_ARG(max_n >= 0, "%s: max_n=%d (max_n >= 0)", who, max_n);
  PN_CHECK_ARG(min_size >= 1, "%s: min_size=%d (min_size >= 1)", who, min_size);
  if (S == 0 || total == 0) return PN_OK;
  PN_CHECK_ARG(pts && off && radius && label && ncomp && ws,
               "%s: null pointer (pts, off, radius, label, ncomp and ws are required)", who);
  PN_CHECK_ARG(ws_bytes >= pn_cluster_workspace_bytes(total, S), "%s: workspace of %lld bytes (%lld)", who, ws_bytes,
               pn_cluster_workspace_bytes(total, S));
  ClWs w;
  cl_carve((void*)pn_align_up((size_t)ws, 16), total, S, &w);
  const int rounds = cl_rounds(max_n), passes = cl_passes(max_n);
  const dim3 block(CL_BLOCK);
  const int vb = pn_cdiv(total, CL_BLOCK);
  const dim3 vgrid(vb < CL_MAX_BLOCKS ? vb : CL_MAX_BLOCKS);
  PN_CHECK_HIP(hipMemsetAsync(w.ctrl, 0, (size_t)CL_CTRL_WORDS * 4, stream));
  PN_CHECK_HIP(hipMemsetAsync(w.best, 0xff, (size_t)((char*)w.cnt - (char*)w.best), stream));
  PN_CHECK_HIP(hipMemsetAsync(w.cnt, 0, (size_t)((char*)w.pcell - (char*)w.cnt), stream));
  PN_PROF("cluster", stream);
  hipLaunchKernelGGL(pn_cluster_bounds_kernel, dim3(pn_cdiv(total, 4 * CL_ROWS_PER_WAVE)), dim3(256), 0, stream, pts,
                     off, S, total, w);
  hipLaunchKernelGGL(pn_cluster_cells_kernel, vgrid, block, 0, stream, pts, off, total, radius, w);
  hipLaunchKernelGGL(pn_cluster_scan_kernel, dim3(S), dim3(CL_SCAN), 0, stream, off, total, radius, w);
  hipLaunchKernelGGL(pn_cluster_scatter_kernel, vgrid, block, 0, stream, pts, off, total, w);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(pn_cluster_offer_kernel, dim3(pn_cdiv(total, 4)), dim3(256), 0, stream, off, total, radius, r, w);
    hipLaunchKernelGGL(pn_cluster_hook_kernel, vgrid, block, 0, stream, off, total, r, w);
    for (int p = 0; p < passes; ++p)
      hipLaunchKernelGGL(pn_cluster_compress_kernel, vgrid, block, 0, stream, off, total, r, p, w);
  }
  hipLaunchKernelGGL(pn_cluster_sizes_kernel, vgrid, block, 0, stream, off, total, radius, w);
  hipLaunchKernelGGL(pn_cluster_numbers_kernel, dim3(S), dim3(CL_SCAN), 0, stream, off, total, radius, min_size, w,
                     label, ncomp, count, first, ndrop);
  hipLaunchKernelGGL(pn_cluster_labels_kernel, vgrid, block, 0, stream, off, total, radius, min_size, w, label);
  PN_CHECK_LAUNCH();
  return PN_OK;
}
