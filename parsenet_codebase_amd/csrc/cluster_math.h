// Definition of the Euclidean cluster extraction of cluster.hip: the connected components of the graph that joins two
// points of a cloud when they are no further apart than a radius, numbered by their lowest point.  Plain C++ behind the
// CL_HD qualifier so that the same source is compiled into the gfx950 kernels and, by the test suite only
// (tests/native/cluster_host.cpp), into a serial simulation of the launches.  Contraction is switched off inside every
// function here, whatever the flags of the including file (clang: the pragma inside the functions; g++: the option pushed
// around the whole header).
//
// Everything is per segment (one cloud of a ragged batch) of n points, indices LOCAL to it.
//
//   radius      r, one fp32 per segment; r2 = fl(r * r), rounded once in fp32 (cl_r2).
//   edge        {i, j}, i != j, is an edge iff kg_dist(i, j) <= r2: the expression of knn3_grid_math.h word for word,
//               d = ((x_i - x_j)^2 + (y_i - y_j)^2) + (z_i - z_j)^2, every operation rounded once, no fma.  Swapping the
//               ends negates the three differences exactly and leaves the squares alone: d is symmetric bit for bit, so
//               "j is in the ball of i" and "i is in the ball of j" are one statement.  Equality is an edge.
//   component   a connected component of that graph.  Nothing below depends on how the components are found.
//   numbering   a component is KEPT iff it holds at least min_size points.  Kept components are numbered 0 .. C-1 by
//               their ascending lowest point index; every point of a dropped component has label -1.
//   outputs     label (n) int32; ncomp = C; count, first (n) int32: rows 0 .. C-1 hold the size and the lowest index of
//               the kept components, -1 behind them; ndrop: the points with label -1.
//   status      in ncomp, with label -1 throughout and count / first -1: CL_NON_FINITE (-1) for a segment that holds an
//               inf or a NaN coordinate — flagged while the bounding box is taken and never searched —, CL_BAD_RADIUS
//               (-2) where r or r2 is not a positive finite number (r = 1e-30: r2 underflows to 0).
//
// Neighbour search.  Exact, on the uniform grid of knn3_grid_math.h: its cell function, its monotonicity argument and
// its bound kg_bound are used as they stand, only the resolution is chosen here.  A query in cell c looks at the cube
// of cells within Chebyshev distance ring = 0, 1, ... of c and stops after the first ring whose bound b(ring) is
// STRICTLY above r2, or whose cube covers the grid (cl_stop).  Every point outside the cube has d >= b(ring) > r2: it
// is no neighbour.  With b(ring) == r2 a point outside could still have d == r2, which is an edge: hence strictly.  The
// bound is evaluated, not estimated, so ANY resolution is correct; cl_resolution picks the smaller of
// kg_resolution(n, KG_PPC) and the largest R whose cell edge fl(extent / R) is not below r, so that ring 1 normally
// ends the search (a doubt about that R costs a ring, never a neighbour).
//
// Merging.  Boruvka rounds on a parent word P[v] per point (between rounds every point points at the root of its
// component, initially itself), a 64-bit slot best[v] and a hook word H[v]:
//   offers    every point i searches its ball; of the neighbours j whose root differs from its own it takes the least
//             key cl_key(i, j) = (min(i,j) << 32) | max(i,j) and offers it to ITS OWN root by a 64-bit integer minimum.
//             The key is unique per undirected edge and the same from both ends, and by the symmetry of d the other
//             end finds the same edge in its own ball and offers the same key to the other root: after the launch
//             best[root] is the least key over all edges that leave the component, whatever the order of arrival.
//   hooks     cl_hook: a root with an entry hooks to the root at the other end of its least edge; of a mutual pick (both
//             roots hold the same key) the lower root stays root.  Keys are totally ordered and unique, so the picks
//             form no cycle but the mutual pair (along a cycle of picks the keys would strictly descend).  It only
//             READS P and best; the word goes to H, because P of other roots is read in the same launch.
//   passes    cl_walk: up to CL_WALK further parents from the word of v (P[v], or H[v] while v still stands as a root
//             in P with a hook pending: first pass only).  Every word read is a single load of an ancestor in the hooked
//             forest, whichever of its values a concurrent walk left there: correct under any interleaving.
// The schedule, fixed by the host from the largest segment max_n alone, is boruvka_schedule.h (shared with
// orient_global_math.h): cl_rounds = bv_rounds rounds of offers, hooks and cl_passes = bv_passes compress passes, with
// the proof of both bounds, the control words and the word a pass reads (cl_word = bv_word).
//   cl_launches  4 (bounds and init, cells, scan, scatter) + rounds x (offers + hooks + passes) + 3 (sizes, numbers,
//             labels).
#pragma once
#include "boruvka_schedule.h"
#include "knn3_grid_math.h"
#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

#define CL_HD KG_HD
#define CL_NO_ENTRY 0xffffffffffffffffull
#define CL_NON_FINITE (-1)
#define CL_BAD_RADIUS (-2)
// The shared schedule under the names of this engine, which cluster.hip and the host simulation use.
#define CL_WALK BV_WALK
#define CL_NO_HOOK BV_NO_HOOK
#define CL_MAX_ROUNDS BV_MAX_ROUNDS
#define CL_MAX_PASSES BV_MAX_PASSES
#define CL_CTRL_ANY BV_CTRL_ANY
#define CL_CTRL_CHANGED BV_CTRL_CHANGED
#define CL_CTRL_WORDS BV_CTRL_WORDS      // the first words of the workspace
CL_HD int cl_rounds(int max_n) { return bv_rounds(max_n); }
CL_HD int cl_passes(int max_n) { return bv_passes(max_n); }
CL_HD uint32_t cl_word(const uint32_t* P, const uint32_t* H, uint32_t x, int first) { return bv_word(P, H, x, first); }

CL_HD int cl_launches(int max_n) { return 4 + cl_rounds(max_n) * (2 + cl_passes(max_n)) + 3; }

CL_HD float cl_r2(float r) {
  KG_NO_CONTRACT
  return r * r;
}

// 0, or the status of a segment: `bad` is its non-finite flag, r its radius.
CL_HD int cl_status(uint32_t bad, float r) {
  if (bad) return CL_NON_FINITE;
  const float r2 = cl_r2(r);
  if (!(r > 0.0f) || !kg_finite(r) || !(r2 > 0.0f) || !kg_finite(r2)) return CL_BAD_RADIUS;
  return 0;
}

// The cells per axis of a segment of n points, largest extent em, radius r (positive, finite): at most
// kg_resolution(n, KG_PPC), and the cell edge fl(em / R) not below r where an R > 1 allows it.  Any value >= 1 is
// correct; at most four steps down from the quotient.
CL_HD int cl_resolution(int n, float em, float r) {
  KG_NO_CONTRACT
  int R = kg_resolution(n, KG_PPC);
  if (!(em > 0.0f) || !kg_finite(em)) return 1;
  const float q = em / r;                                  // (inf for a tiny r: R stays)
  if (q < (float)R) R = q >= 1.0f ? (int)q : 1;
  for (int t = 0; t < 4 && R > 1 && em / (float)R < r; ++t) --R;
  return R;
}

// kg_grid with the resolution of cl_resolution: the same cells, faces and clamps, so that kg_cell, kg_covers and
// kg_bound apply as they stand.
CL_HD KgGrid cl_grid(int n, const float* lo, const float* hi, float r) {
  KG_NO_CONTRACT
  KgGrid g;
  float em = 0.0f;
  for (int a = 0; a < 3; ++a) {
    g.lo[a] = lo[a];
    g.dim[a] = 1;
    const float e = hi[a] - lo[a];
    if (!(e <= em)) em = e;
  }
  const int R = cl_resolution(n, em, r);
  g.h = 0.0f;
  g.inv_h = 0.0f;
  if (R > 1 && em > 0.0f && kg_finite(em)) {
    const float h = em / (float)R, inv_h = (float)R / em;
    if (h > 0.0f && kg_finite(h) && inv_h > 0.0f && kg_finite(inv_h)) {
      g.h = h;
      g.inv_h = inv_h;
      for (int a = 0; a < 3; ++a) {
        g.dim[a] = R;                                  // the clamp of kg_cell while the cell of hi is taken
        const int top = kg_cell(g, a, hi[a]) + 1;
        g.dim[a] = top < R ? top : R;
      }
    }
  }
  return g;
}

// Is ring `ring` the last one of the query q in the cells c?  (See "Neighbour search" above.)
CL_HD int cl_stop(const KgGrid& g, const int* c, int ring, const float* q, float r2) {
  return kg_covers(g, c, ring) || kg_bound(g, c, ring, q) > r2;
}

CL_HD int cl_is_edge(float d, float r2) { return d <= r2; }

CL_HD unsigned long long cl_key(uint32_t i, uint32_t j) {
  return i < j ? ((unsigned long long)i << 32) | j : ((unsigned long long)j << 32) | i;
}

// The root v after the offers: its new parent, or CL_NO_HOOK; *any = 1 when it holds an entry at all.  The ends of an
// offered key lie inside the segment; a word outside it (never) is refused.
CL_HD uint32_t cl_hook(const uint32_t* P, const unsigned long long* best, int n, uint32_t v, int* any) {
  const unsigned long long key = best[v];
  if (key == CL_NO_ENTRY) return CL_NO_HOOK;
  const uint32_t a = (uint32_t)(key >> 32), b = (uint32_t)key;
  if (a >= (uint32_t)n || b >= (uint32_t)n) return CL_NO_HOOK;
  const uint32_t ca = P[a], cb = P[b];
  const uint32_t other = ca == v ? cb : ca;
  if (other >= (uint32_t)n || other == v) return CL_NO_HOOK;
  *any = 1;
  if (best[other] == key && v < other) return CL_NO_HOOK;      // the lower root of a mutual pick stays root
  return other;
}

// One compress pass of vertex v: an ancestor up to CL_WALK parents above the word of v.
CL_HD uint32_t cl_walk(const uint32_t* P, const uint32_t* H, int n, uint32_t v, int first) {
  uint32_t w = bv_word(P, H, v, first);
  for (int t = 0; t < CL_WALK; ++t) {
    if (w == v || w >= (uint32_t)n) break;                           // v is a root
    const uint32_t q = bv_word(P, H, w, first);
    if (q == w || q >= (uint32_t)n) break;                           // w is a root
    w = q;
  }
  return w < (uint32_t)n ? w : v;
}

CL_HD int cl_kept(uint32_t count, int min_size) { return count >= (uint32_t)min_size; }

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
