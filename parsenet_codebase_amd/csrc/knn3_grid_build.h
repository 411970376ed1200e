// The uniform grid of knn3_grid_math.h built on a ragged batch of clouds, and the ring search on it: what knn3_grid.hip
// (every point searches its own cloud) and knn3_query.hip (the points of one cloud search another) share.  One
// definition of the workspace, of the four build phases and of the ring loop, so that the two searches cannot drift
// apart; each translation unit that includes this header gets its own copy of the kernels (anonymous namespace).
//
//   1 bbox     min / max per axis and segment (atomics on the order-preserving integer image, one set per wave where
//              the wave's rows lie in one segment) and the non-finite flag.  Every later phase derives the segment's
//              grid from these six numbers with kg_grid: no table is built, nothing is downloaded.
//   2 cells    the cell of every point and its rank inside the cell (the value the histogram's atomic returned).
//   3 scan     exclusive scan of a segment's histogram to global positions, one workgroup per segment.  The histogram
//              is laid out by the offsets of the cloud that owns the GRID; the positions start at base[s], the offsets
//              of the cloud whose rows are being SORTED (the same cloud in the build; the queries in knn3_query.hip).
//   4 scatter  (x, y, z, local index) as one 16-byte record per point to start[cell] + rank.  The order inside a cell
//              is the order of the atomics; no output depends on it, because selection is by the key (d, j) alone.
//   search     kg_ring_search: one wave keeps its best 64 keys knn_key(-d, j), one per lane, sorted.  Ring by ring
//              (knn3_grid_math.h) the rows of the shell — a row of cells along x is one contiguous range of records —
//              are handed out one per lane; a batch of 64 records is one 16-byte load per lane; a ballot of "beats the
//              k-th" skips the merge (knn_wave_sort128 of the list and the batch) for most batches.  No capacity
//              anywhere: a cell of thousands of coincident points is slow, not wrong.
//
// Workspace (kg_take): records 16 total | cell 4 total | rank 4 total | box max 12 S | flag 4 S | cell starts
// 4 (total + 2 S) | box min 12 S.  Segment s owns the cell slots [off[s] + 2 s, off[s + 1] + 2 s + 2): at most
// max(1, n_s) cells and the end sentinel.
#pragma once
#include <stdlib.h>

#include "knn3_grid_math.h"
#include "knn_common.h"
#include "ragged.h"

#define KG_ROWS_PER_WAVE 512      // bbox: rows one wave reduces before its six atomics

struct KgWs {
  float4* rec;
  int* pcell;
  int* prank;
  uint32_t* bmax;      // (S,3) ord of the maxima            } one memset 0
  uint32_t* flag;      // (S)                                 }
  int* start;          // (total + 2 S) histogram, then starts }
  uint32_t* bmin;      // (S,3) ord of the minima: memset 0xff
};

// The arrays of the grid in order, taken from a carver that may go on to further arrays.
static inline void kg_take(RgCarver& c, long long total, long long S, KgWs* w) {
  w->rec = c.take<float4>(total);
  w->pcell = c.take<int>(total);
  w->prank = c.take<int>(total);
  w->bmax = c.take<uint32_t>(3 * S);
  w->flag = c.take<uint32_t>(S);
  w->start = c.take<int>(total + 2 * S);
  w->bmin = c.take<uint32_t>(3 * S);
}

// The arrays of the workspace in order, cut from `base` (0: measure only); returns their bytes.
static inline long long kg_carve(void* base, long long total, long long S, KgWs* w) {
  RgCarver c = {(uintptr_t)base, 0};
  kg_take(c, total, S, w);
  return c.bytes;
}

// PN_KNN3_GRID_PPC: developer hook of tools/knn3_grid_ab.py — the points per cell, which moves the speed and no output.
static inline int kg_ppc(void) {
  const char* e = getenv("PN_KNN3_GRID_PPC");
  const int v = e ? atoi(e) : 0;
  return v >= 1 && v <= KG_MAX_PPC ? v : KG_PPC;
}

// The segment of a row: the largest s < S with off[s] <= row.  The caller checks off[s] <= row < off[s + 1].
__device__ static inline int kg_segment(const int* __restrict__ off, int S, int row) {
  return rg_row_segment(off, S, row);
}

__device__ static inline KgGrid kg_segment_grid(const KgWs& w, int s, int n, int ppc) {
  float lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = pn_ord2f(w.bmin[3 * s + a]);
    hi[a] = pn_ord2f(w.bmax[3 * s + a]);
  }
  return kg_grid(n, lo, hi, ppc);
}

namespace {

// ---- 1: bounding boxes and flags -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pn_knn3_grid_bbox_kernel(const float* __restrict__ pts,
                                                                const int* __restrict__ off, int S, int total,
                                                                KgWs w) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long first = wave * KG_ROWS_PER_WAVE;
  if (first >= total) return;
  const int last = (int)(first + KG_ROWS_PER_WAVE - 1 < total - 1 ? first + KG_ROWS_PER_WAVE - 1 : total - 1);
  const int s0 = kg_segment(off, S, (int)first), s1 = kg_segment(off, S, last);
  const bool one = s0 == s1 && off[s0] <= (int)first && last < off[s0 + 1];      // (uniform over the wave)
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
      bad |= nf;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        mn[a] = o[a] < mn[a] ? o[a] : mn[a];
        mx[a] = o[a] > mx[a] ? o[a] : mx[a];
      }
    } else {
      const int s = kg_segment(off, S, row);
      if (row < off[s] || row >= off[s + 1]) continue;      // (offsets that do not cover the rows: no segment)
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

// ---- 2: the cell of every point, the histogram and the point's rank in its cell ---------------------------------------
__global__ __launch_bounds__(256) void pn_knn3_grid_cells_kernel(const float* __restrict__ pts,
                                                                 const int* __restrict__ off, int S, int total,
                                                                 int ppc, KgWs w) {
  const long long row64 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row64 >= total) return;
  const int row = (int)row64;
  const int s = kg_segment(off, S, row);
  const int o0 = off[s], n = off[s + 1] - o0;
  w.pcell[row] = -1;
  if (row < o0 || row - o0 >= n || w.flag[s]) return;
  const KgGrid g = kg_segment_grid(w, s, n, ppc);
  const int cell = kg_cell_index(g, kg_cell(g, 0, pts[(size_t)row * 3]), kg_cell(g, 1, pts[(size_t)row * 3 + 1]),
                                 kg_cell(g, 2, pts[(size_t)row * 3 + 2]));
  w.pcell[row] = cell;
  w.prank[row] = atomicAdd(&w.start[(size_t)o0 + 2 * (size_t)s + cell], 1);      // cell < max(1, n)
}

// ---- 3: exclusive scan of a segment's histogram to positions ------------------------------------------------------------
// `off` (total rows) lays out the grid and the histogram `st_all`; the positions of segment s start at base[s].  A
// segment of `off` that does not lie inside 0 .. total owns no slots and is skipped.
__global__ __launch_bounds__(1024) void pn_knn3_grid_scan_kernel(const int* __restrict__ off,
                                                                 const int* __restrict__ base, int total, int ppc,
                                                                 KgWs w, int* __restrict__ st_all) {
  __shared__ int s_wave[16];
  __shared__ int s_carry;
  const int s = blockIdx.x;
  const int o0 = off[s], n = off[s + 1] - o0;
  if (n <= 0 || !rg_valid_segment(o0, o0 + n, total) || w.flag[s]) return;
  const KgGrid g = kg_segment_grid(w, s, n, ppc);
  const int ncell = kg_cells(g);                                     // <= n
  int* __restrict__ st = st_all + (size_t)o0 + 2 * (size_t)s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_carry = base[s];
  __syncthreads();
  for (int b = 0; b < ncell; b += 4096) {
    const int c0 = b + 4 * (int)threadIdx.x;
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
  if (threadIdx.x == 0) st[ncell] = s_carry;                         // the end of the last cell
}

// ---- 4: the records in cell order ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pn_knn3_grid_scatter_kernel(const float* __restrict__ pts,
                                                                   const int* __restrict__ off, int S, int total,
                                                                   KgWs w) {
  const long long row64 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row64 >= total) return;
  const int row = (int)row64;
  const int cell = w.pcell[row];
  if (cell < 0) return;
  const int s = kg_segment(off, S, row);
  const int o0 = off[s], o1 = off[s + 1];
  const int pos = w.start[(size_t)o0 + 2 * (size_t)s + cell] + w.prank[row];
  if (pos < o0 || pos >= o1) return;                                 // (cannot happen; never write out of the segment)
  w.rec[pos] = make_float4(pts[(size_t)row * 3], pts[(size_t)row * 3 + 1], pts[(size_t)row * 3 + 2],
                           __int_as_float(row - o0));
}

}  // namespace

// The two memsets and the four launches that build the grid of every segment of (pts, off) in w.  total, S > 0.
static inline int kg_build_launch(const float* pts, const int* off, int S, int total, int ppc, const KgWs& w,
                                  hipStream_t stream) {
  const size_t zero_bytes = (size_t)((char*)w.bmin - (char*)w.bmax);      // box max, flag and cell starts
  PN_CHECK_HIP(hipMemsetAsync(w.bmax, 0, zero_bytes, stream));
  PN_CHECK_HIP(hipMemsetAsync(w.bmin, 0xff, (size_t)12 * S, stream));
  const int row_blocks = pn_cdiv(total, 256);
  {
    PN_PROF("knn3_grid_bbox", stream);
    hipLaunchKernelGGL(pn_knn3_grid_bbox_kernel, dim3(pn_cdiv(total, 4 * KG_ROWS_PER_WAVE)), dim3(256), 0, stream, pts,
                       off, S, total, w);
  }
  {
    PN_PROF("knn3_grid_cells", stream);
    hipLaunchKernelGGL(pn_knn3_grid_cells_kernel, dim3(row_blocks), dim3(256), 0, stream, pts, off, S, total, ppc, w);
  }
  {
    PN_PROF("knn3_grid_scan", stream);
    hipLaunchKernelGGL(pn_knn3_grid_scan_kernel, dim3(S), dim3(1024), 0, stream, off, off, total, ppc, w, w.start);
  }
  {
    PN_PROF("knn3_grid_scatter", stream);
    hipLaunchKernelGGL(pn_knn3_grid_scatter_kernel, dim3(row_blocks), dim3(256), 0, stream, pts, off, S, total, w);
  }
  return PN_OK;
}

// ---- the search ---------------------------------------------------------------------------------------------------------
// One batch: the records [p, min(p + 64, end)) against the wave's list.
__device__ static inline void kg_batch(const float4* __restrict__ rec, int p, int end, float qx, float qy, float qz,
                                       int n, int k, u64& best, u64& kth) {
  const int lane = threadIdx.x & 63;
  u64 key = 0ull;
  if (p + lane < end) {
    const float4 c = rec[p + lane];
    const int j = __float_as_int(c.w);
    if ((unsigned)j < (unsigned)n) key = knn_key(-kg_dist(qx, qy, qz, c.x, c.y, c.z), j);
  }
  if (__ballot(key > kth) == 0ull) return;
  knn_wave_sort128(best, key);
  kth = readlane_u64(best, k - 1);
}

// The whole wave: the k best keys of the query q, whose cell in g is c (clamped when q lies outside the grid), among the
// records [o0, o1) of a segment of n points with cell starts st.  Returns the wave's sorted list, rank r in lane r; a
// lane beyond the points of the segment holds 0.  The loop ends by kg_covers at an integer limit, or earlier by
// kg_bound once k candidates are held — never on "k held" while the segment has fewer than k points, because then the
// k-th key stays 0.
__device__ static inline u64 kg_ring_search(const KgWs& w, const int* __restrict__ st, const KgGrid& g, int o0, int o1,
                                            int n, int k, const float* q, const int* c) {
  const int lane = threadIdx.x & 63;
  const int rmax = max(g.dim[0], max(g.dim[1], g.dim[2]));      // the cube of ring rmax covers any grid
  u64 best = 0ull, kth = 0ull;
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
      u64 m = __ballot(e0 > b0);
      while (m) {
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        const int b = __builtin_amdgcn_readlane(b0, l), e = __builtin_amdgcn_readlane(e0, l);
        for (int pp = b; pp < e; pp += 64) kg_batch(w.rec, pp, e, q[0], q[1], q[2], n, k, best, kth);
      }
      m = __ballot(e1 > b1);
      while (m) {
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        const int b = __builtin_amdgcn_readlane(b1, l), e = __builtin_amdgcn_readlane(e1, l);
        for (int pp = b; pp < e; pp += 64) kg_batch(w.rec, pp, e, q[0], q[1], q[2], n, k, best, kth);
      }
    }
    if (kg_covers(g, c, r)) break;
    if (kth == 0ull) continue;                                     // fewer than k candidates so far
    const float dk = fabsf(pn_ord2f((uint32_t)(kth >> 32)));      // the key holds -d: |.| gives d, and +0 for d = 0
    if (dk < kg_bound(g, c, r, q)) break;                          // (uniform over the wave)
  }
  return best;
}

// The distance a key holds, as the searches write it: (float) sqrt((double) d).
__device__ static inline float kg_key_dist(u64 key) {
  return (float)sqrt((double)fabsf(pn_ord2f((uint32_t)(key >> 32))));
}
