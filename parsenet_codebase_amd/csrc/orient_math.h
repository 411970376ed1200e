// Definition of the consistent orientation of point normals without a viewpoint (orient.hip): signs are propagated
// along the minimum spanning forest of the k-NN graph under the weight 1 - |n_i . n_j| (Hoppe et al. 1992), and one
// rule per connected component fixes the component's sign.  Plain C++ behind the OM_HD qualifier so that the SAME
// source is compiled into the gfx950 kernel and, by the test suite only (tests/native/orient_math_host.cpp), into a
// serial restatement (Kruskal, tree walk, seed rule) the kernel is held against bit for bit.  Contraction is switched
// off inside every function here, whatever the flags of the including file.
//
// All indices are LOCAL to a segment (one cloud of a ragged batch) of n points.  idx (n,k) is what pn_knn3_ragged
// wrote: the point itself first, and padding with the point itself.
//
//   entries     one per (point i, slot s), e = i k + s, with j = idx[i][s].  An entry with j == i (the self entry and
//               every padding entry) or with j outside 0 .. n-1 is dropped.  The graph is undirected: the entry i -> j
//               is incident to i and to j; a pair that lists each other gives two parallel entries, which is harmless.
//   weight      dot = (nx_i nx_j + ny_i ny_j) + nz_i nz_j in fp64 on the fp32 normals, in exactly this order (the
//               products of fp32 values are exact in fp64 and commute, so dot is bitwise symmetric in i, j);
//               d = 1 - |dot|;  w = d > 0 ? (float) d : 0;  neg = dot < 0.  A zero normal gives w = 1, neg = false.
//   order       key = (bits of w as uint32) << 32 | e.  w >= 0, so its bit pattern orders as its value; the order is
//               strict, so the minimum spanning forest under it is unique — which is what makes an exact test possible.
//   propagation flip(j) = flip(i) XOR neg(i,j) along every forest edge: the flips of a component up to one bit.
//   seed        the vertex of a component with the largest om_zkey: the largest fp32 z (-0 counts as +0), the lowest
//               index on equal z.  The component's bit is chosen so that the seed's oriented normal has n_z >= 0:
//               flip(seed) = n_z(seed) < 0.  A seed with n_z == 0 (-0 and the zero normal included) keeps flip = 0.
//   outputs     per point: the oriented normal — the input normal, bit-identical (flip = 0) or with the sign bit of
//               every component inverted (flip = 1); flip (0/1); seed, the local index of the component's seed.
//               All three are functions of the input alone.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#define OM_HD __host__ __device__ static inline __attribute__((always_inline))
#else
#define OM_HD static inline __attribute__((always_inline))
#endif
#if defined(__clang__)
#define OM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define OM_NO_CONTRACT
#if defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
#endif

#define OM_MIN_K 1                    // pn_knn3_ragged's limits (k = 1: the point itself, no entry, n components)
#define OM_MAX_K 64
#define OM_NO_ENTRY (~0ull)           // above every key
#define OM_PARITY 0x80000000u         // the parity bit of a packed (parent, parity) word

OM_HD uint32_t om_bits(float f) {
  uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
  u = __float_as_uint(f);
#else
  memcpy(&u, &f, 4);
#endif
  return u;
}

// Weight and relative sign of the pair of normals a, b.
OM_HD float om_weight(const float* a, const float* b, int* neg) {
  OM_NO_CONTRACT
  const double dot = ((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2];
  const double d = 1.0 - fabs(dot);
  *neg = dot < 0.0 ? 1 : 0;
  return d > 0.0 ? (float)d : 0.0f;
}

OM_HD unsigned long long om_key(float w, uint32_t entry) {
  return ((unsigned long long)om_bits(w) << 32) | (unsigned long long)entry;
}

// Seed order: larger is better.  The high word orders as z does (-0 as +0), the low word prefers the lower index.
OM_HD unsigned long long om_zkey(float z, uint32_t vertex) {
  const uint32_t u = om_bits(z + 0.0f);
  const uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)ord << 32) | (unsigned long long)(~vertex);
}
OM_HD uint32_t om_zkey_vertex(unsigned long long key) { return ~(uint32_t)key; }

// The seed's own flip: its oriented normal has n_z >= 0.
OM_HD int om_seed_flip(float nz) { return nz < 0.0f ? 1 : 0; }

// The oriented component: bit-identical, or the sign bit inverted.
OM_HD float om_apply(float x, int flip) { return flip ? -x : x; }

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
