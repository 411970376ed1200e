// What every kernel over a ragged batch needs besides its own arithmetic: the segment that a row or a tile belongs to,
// and a workspace cut into typed arrays.  Every raw-cloud family takes them from here: knn3_grid.hip, knn3_query.hip
// and register.hip through knn3_grid_build.h; fps.hip, outlier.hip, voxel.hip and plane.hip through fps_math.h;
// cluster.hip, orient_global.hip and knn_lift.hip directly.  Plain C++ behind RG_HD so that the same source is compiled
// into the gfx950 kernels and, by the test suite only (tests/native/ragged_host.cpp), for the host.
//
// A ragged batch is S segments over `total` rows: off[s] .. off[s + 1] - 1 are the rows of segment s, off ascends from
// 0 to total, and a segment may be empty.  The offsets come from the caller, so a kernel never trusts them: it
// searches, then checks what it found with one of the predicates below, and a row that no valid segment holds is
// skipped (or marked), never used as an index.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RG_HD __host__ __device__ static inline __attribute__((always_inline))
#else
#define RG_HD static inline __attribute__((always_inline))
#endif

// The last s in [0, S) with key(s) <= x; 0 when no s has (key(0) is never read) and when S <= 1.  key(s) must not
// decrease with s: off[s] for rows, fps_tile_base(off[s], s) for the tiles of fps.hip.  Among equal keys — a run of
// empty segments — the last one wins, which is the one that can hold x.  At most 32 steps whatever the keys hold.
template <class X, class Key>
RG_HD int rg_segment(int S, X x, Key key) {
  int lo = 0, hi = S;                                   // key(lo) <= x (assumed for lo = 0), key(hi) > x or hi = S
  for (int t = 0; t < 32 && hi - lo > 1; ++t) {
    const int mid = lo + ((hi - lo) >> 1);
    if (key(mid) <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// The segment of a row: rg_segment on the offsets themselves.
RG_HD int rg_row_segment(const int* __restrict__ off, int S, int row) {
  return rg_segment(S, row, [off](int s) { return off[s]; });
}

// Is [o0, o1) a segment inside 0 .. total?
RG_HD int rg_valid_segment(int o0, int o1, int total) { return o0 >= 0 && o0 <= o1 && o1 <= total; }

// Does it hold row x as well?  0 <= o0 <= x < o1 <= total.
RG_HD int rg_segment_holds(int o0, int o1, int total, int x) { return o0 >= 0 && o0 <= x && x < o1 && o1 <= total; }

// A workspace cut into typed arrays: take<T>(count) returns the next array and moves on by count * sizeof(T).  A
// kernel family writes ONE function that takes its arrays in order and returns `bytes`; run on base 0 it measures the
// workspace, run on the real base it yields the pointers, so the two cannot drift apart.  The addresses are formed as
// integers: the measuring pass does no arithmetic on a null pointer, and its pointers are never used.  The order of the
// takes keeps every array aligned to its element (the widest elements first, or counts that keep the next one aligned).
struct RgCarver {
  uintptr_t base;
  long long bytes;
  template <class T>
  T* take(long long count) {
    T* const at = (T*)(base + (uintptr_t)bytes);
    bytes += count * (long long)sizeof(T);
    return at;
  }
};
