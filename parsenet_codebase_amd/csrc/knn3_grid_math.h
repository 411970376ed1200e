// Definition of the uniform-grid neighbour search of knn3_grid.hip: the SAME exact k nearest neighbours as the
// brute-force kernel of knn3.hip (fp32 mode), found in O(n k) instead of O(n^2).  Plain C++ behind the KG_HD qualifier
// so that the same source is compiled into the gfx950 kernels and, by the test suite only
// (tests/native/knn3_grid_host.cpp), into a serial restatement of the whole search.  Contraction is switched off
// inside every function here, whatever the flags of the including file.
//
// Everything is per segment (one cloud of a ragged batch) of n points, indices LOCAL to it.
//
//   distance    d(i,j) = ((x_i - x_j)^2 + (y_i - y_j)^2) + (z_i - z_j)^2, every operation rounded once in fp32, no fma:
//               kg_dist, word for word the expression of knn3.hip.  Neighbours are ordered by (d, j) ascending.
//   grid        lo, hi: min and max per axis of the fp32 coordinates.  R = kg_resolution(n, ppc): the largest integer
//               with ppc R^3 <= n (at least 1) — integer arithmetic on n alone.  h = fl(max extent / R) is the edge of
//               the cubic cells, inv_h = fl(R / max extent).  An axis has dim = min(R, cell of hi + 1) cells, so the
//               grid has at most R^3 <= max(1, n) cells.  A zero, overflowing or vanishing extent (h or inv_h not a
//               positive finite number) gives ONE cell: nothing is divided by zero, the search is then brute force.
//   cell        kg_cell: t = fl(fl(x - lo) * inv_h); 0 unless t > 0; dim - 1 if t >= dim - 1; else (int) t.
//               fl(x - lo) is non-decreasing in x (rounding to nearest is monotone), so is the product with
//               inv_h > 0, so is the truncation, so is the clamp: the cell is a NON-DECREASING function of the
//               coordinate.  That property — not the position of the cell's faces — is all the search relies on.
//   rings       a query in cell c looks at the cube of cells within Chebyshev distance r of c, r = 0, 1, ...; ring r
//               adds the shell of the cube.  It stops at the first r where it holds k candidates and the k-th d is
//               STRICTLY below b(r), or where the cube covers the whole grid (r <= largest dim: an integer limit).
//   bound b(r)  A point outside the cube has, on some axis, a cell above c + r or below c - r.  Take the upper face of
//               one axis, m = c + r + 1 <= dim - 1 (no such cell: no such point, the face gives +inf).  Let e be ANY
//               fp32 number with kg_cell(e) <= m - 1.  A point with cell >= m has coordinate p > e, because p <= e
//               would give cell(p) <= cell(e) by monotonicity.  e is found by evaluating the cell function itself:
//               start at fl(lo + fl(m h)) and step to the previous fp32 number while the cell is still >= m, at
//               most KG_STEPS times; a face whose e is not found, or whose e does not lie above the query, gives 0.
//               So the rounding of the cell function needs no error analysis: it is evaluated, not estimated.
//               With q < e < p (fp32 numbers, q the query's coordinate):
//                 fl(p - q) >= fl(e - q) = G >= 0     subtraction rounds monotonically, and fl(q - p) = -fl(p - q);
//                 fl(fl(p - q)^2) >= fl(G^2)           the square of a non-negative number rounds monotonically;
//                 d = fl(fl(sx + sy) + sz) >= fl(G^2)  the other two squares are >= 0, and fl(a + b) is monotone in
//                                                     a and b (adding +0 changes nothing), whichever axis it was.
//               Underflow and overflow keep every step monotone.  The lower face is the mirror image (e with
//               cell(e) >= c - r, stepping to the next number).  b(r) = the minimum over the six faces of fl(G^2),
//               computed with the kernel's own operations: every point outside the cube has d >= b(r).  A point
//               with d == b(r) may tie with the k-th and win on its index, hence the strict comparison.  Every doubt
//               is resolved towards a smaller bound, which costs a ring and never a neighbour.
//   non-finite  a segment that holds an inf or a NaN coordinate is flagged while the bounding box is taken: every row
//               of it is the point itself k times, dist NaN.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KG_HD __host__ __device__ static inline __attribute__((always_inline))
#else
#define KG_HD static inline __attribute__((always_inline))
#endif
#if defined(__clang__)
#define KG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define KG_NO_CONTRACT
#if defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
#endif

#define KG_MIN_K 1
#define KG_MAX_K 64
#define KG_PPC 4          // points per cell of a cloud that fills its bounding box: the best of 2 .. 32 in
                          // profiles/knn3_grid.txt (tools/knn3_grid_ab.py), the runner-up is 32
#define KG_MAX_PPC 4096
#define KG_STEPS 8        // fp32 numbers tried on the way from the nominal face of a cell to a verified one

struct KgGrid {
  float lo[3];
  float h, inv_h;
  int dim[3];
};

KG_HD uint32_t kg_bits(float f) {
  uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
  u = __float_as_uint(f);
#else
  memcpy(&u, &f, 4);
#endif
  return u;
}
KG_HD float kg_float(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float f;
  memcpy(&f, &u, 4);
  return f;
#endif
}
KG_HD float kg_inf(void) { return kg_float(0x7f800000u); }
KG_HD int kg_finite(float f) { return (kg_bits(f) & 0x7f800000u) != 0x7f800000u; }

// The fp32 number after and before a finite x.
KG_HD float kg_next(float x) {
  const uint32_t u = kg_bits(x);
  if ((u & 0x7fffffffu) == 0u) return kg_float(1u);
  return kg_float((u & 0x80000000u) ? u - 1u : u + 1u);
}
KG_HD float kg_prev(float x) {
  const uint32_t u = kg_bits(x);
  if ((u & 0x7fffffffu) == 0u) return kg_float(0x80000001u);
  return kg_float((u & 0x80000000u) ? u + 1u : u - 1u);
}

// The largest R >= 1 with ppc R^3 <= n (1 if there is none): bisection on integers, 11 steps.
KG_HD int kg_resolution(int n, int ppc) {
  if (ppc < 1) ppc = 1;
  if (ppc > KG_MAX_PPC) ppc = KG_MAX_PPC;
  int a = 1, b = 1291;      // 1291^3 > 2^31: the answer is in [a, b)
  while (b - a > 1) {
    const int m = (a + b) / 2;
    if ((long long)m * m * m * ppc <= (long long)n)
      a = m;
    else
      b = m;
  }
  return a;
}

KG_HD float kg_dist(float qx, float qy, float qz, float px, float py, float pz) {
  KG_NO_CONTRACT
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

KG_HD int kg_cell(const KgGrid& g, int axis, float x) {
  KG_NO_CONTRACT
  const float t = (x - g.lo[axis]) * g.inv_h;
  const int last = g.dim[axis] - 1;
  if (!(t > 0.0f)) return 0;
  if (t >= (float)last) return last;
  return (int)t;
}

KG_HD KgGrid kg_grid(int n, const float* lo, const float* hi, int ppc) {
  KG_NO_CONTRACT
  KgGrid g;
  float em = 0.0f;
  for (int a = 0; a < 3; ++a) {
    g.lo[a] = lo[a];
    g.dim[a] = 1;
    const float e = hi[a] - lo[a];
    if (!(e <= em)) em = e;      // (a NaN extent — a flagged segment — ends as one cell below)
  }
  const int R = kg_resolution(n, ppc);
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

KG_HD int kg_cells(const KgGrid& g) { return g.dim[0] * g.dim[1] * g.dim[2]; }
KG_HD int kg_cell_index(const KgGrid& g, int cx, int cy, int cz) { return (cz * g.dim[1] + cy) * g.dim[0] + cx; }

// Does the cube of ring r around the cell c cover the grid?
KG_HD int kg_covers(const KgGrid& g, const int* c, int r) {
  for (int a = 0; a < 3; ++a)
    if (c[a] - r > 0 || c[a] + r < g.dim[a] - 1) return 0;
  return 1;
}

// A lower bound of the fp32 d between a query with coordinate q in cell c of ``axis`` and every point whose cell on
// that axis is above c + r (side 1) or below c - r (side 0): see b(r) above.
KG_HD float kg_face_bound(const KgGrid& g, int axis, int side, int c, int r, float q) {
  KG_NO_CONTRACT
  if (side) {
    const int m = c + r + 1;
    if (m > g.dim[axis] - 1) return kg_inf();
    float e = g.lo[axis] + (float)m * g.h;
    if (!kg_finite(e)) return 0.0f;
    for (int s = 0; s < KG_STEPS && kg_cell(g, axis, e) >= m; ++s) e = kg_prev(e);
    if (kg_cell(g, axis, e) >= m || !(e > q)) return 0.0f;
    const float G = e - q;
    return G * G;
  }
  const int m = c - r;
  if (m < 1) return kg_inf();
  float e = g.lo[axis] + (float)m * g.h;
  if (!kg_finite(e)) return 0.0f;
  for (int s = 0; s < KG_STEPS && kg_cell(g, axis, e) < m; ++s) e = kg_next(e);
  if (kg_cell(g, axis, e) < m || !(q > e)) return 0.0f;
  const float G = q - e;
  return G * G;
}

// b(r) of a query q (3 coordinates) in the cells c (3 indices).
KG_HD float kg_bound(const KgGrid& g, const int* c, int r, const float* q) {
  float b = kg_inf();
  for (int a = 0; a < 3; ++a)
    for (int side = 0; side < 2; ++side) {
      const float f = kg_face_bound(g, a, side, c[a], r, q[a]);
      if (f < b) b = f;
    }
  return b;
}

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
