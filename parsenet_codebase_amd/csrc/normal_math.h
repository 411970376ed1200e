// Arithmetic of the k-NN PCA point normals (normals.hip): the normal of a point is the eigenvector of the smallest
// eigenvalue of the covariance of its k nearest neighbours.  Plain C++ behind the NM_HD qualifier so that the SAME
// source is compiled into the gfx950 kernel and, by the test suite only (tests/native/normal_math_host.cpp), into a
// host harness that checks it against numpy.linalg.eigh in float64.  Everything is fp64 on fp32 inputs; every
// multiply and add is rounded once (contraction is switched off inside every function here, whatever the flags of the
// including file); the only other operations are sqrt, division, fabs and comparisons — no trigonometric call — so
// that a host compile and the device compile perform the same IEEE operations.
//
// Input: the segment's points P (n, 3) fp32 and the k LOCAL neighbour indices of the point as pn_knn3_ragged wrote
// them: nearest first, the point itself first, and — when the segment has fewer than k points — padded with the point
// itself.  A padding entry counts as one more copy of the point: it enters the mean and the covariance like any other
// neighbour.  (An index outside 0 .. n-1 is clamped into the segment: no read leaves it.)
//
//   mean        m = (sum_i x_i) / k, summed in neighbour order.
//   covariance  C_ab = (sum_i (x_i - m)_a (x_i - m)_b) / k, the six entries, summed in neighbour order.
//   eigen       cyclic Jacobi, NM_SWEEPS sweeps, each visiting (0,1), (0,2), (1,2) in that order.  A rotation with
//               a_pq == 0 is skipped; otherwise theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| +
//               sqrt(theta^2 + 1)) (sgn(0) = +1; theta^2 overflowing to inf gives t = 0, no NaN), c = 1 / sqrt(t^2 + 1),
//               s = t c.  Not the closed-form cubic: it loses half the digits when two eigenvalues meet.
//   NM_SWEEPS   = 5.  On the inputs of tests/test_point_normals_abi.py (noisy plane, sphere, cylinder, wavy grid,
//               k = 3, 5, 16, 64: 4 864 neighbourhoods) 4 sweeps are the smallest number for which one more sweep
//               changes no bit of any output (normal, variation, gap), measured on the host compile; plus one.  The
//               test re-checks that 4, 5 and 6 sweeps agree bit for bit.  (Jacobi converges quadratically: the
//               off-diagonal mass of a 3 x 3 matrix is below 1e-8 of the diagonal after sweep 3, below 1e-16 after 4.)
//   eigenvalues sorted l0 <= l1 <= l2; l0 is the diagonal entry of the smallest value, the lowest index on equal
//               values; negative rounding noise in l0 and l1 is clamped to 0 (a covariance is positive semi-definite).
//   normal      the eigenvector (column of the accumulated rotations) of l0, renormalised in fp64, rounded to fp32
//               once; canonical sign: the component of largest magnitude (of the fp32 values; the lowest axis on a
//               tie) is positive.
//   scalars     variation = l0 / (l0 + l1 + l2) and gap = (l1 - l0) / l2, formed in fp64, rounded to fp32 once.
//   degenerate  l2 <= NM_TINY (all k points coincide, or nearly) or n < 3: normal (0,0,0), variation = gap = 0.
//               No NaN leaves nm_point for finite input.
//   viewpoint   nm_orient flips the normal iff n . (v - p) < 0, the dot product in fp64 from the fp32 values,
//               ((nx dx + ny dy) + nz dz); a zero dot keeps the canonical sign.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define NM_HD __host__ __device__ static inline __attribute__((always_inline))
#else
#define NM_HD static inline __attribute__((always_inline))
#endif
#if defined(__clang__)
#define NM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define NM_NO_CONTRACT
#if defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
#endif

#define NM_SWEEPS 5      // see above
#define NM_TINY 1e-30    // largest eigenvalue at or below which a neighbourhood is a point
#define NM_MIN_K 3
#define NM_MAX_K 64

// One Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix; r is the third index.  nm_angle: tangent,
// cosine and sine from the 2 x 2 block (a_pq != 0).  NM_ROTATE applies it — app, aqq, apq: the block; arp, arq: the
// two entries that couple it to r; (v0p, v0q), (v1p, v1q), (v2p, v2q): the rows of the columns p and q of the
// accumulated eigenvector matrix.  (A macro over plain locals, not a function over references: no variable of
// nm_point has its address taken, so all of them live in registers on the device.)
struct NmRot {
  double t, c, s;
};

NM_HD NmRot nm_angle(double app, double aqq, double apq) {
  NM_NO_CONTRACT
  NmRot r;
  const double theta = (aqq - app) / (2.0 * apq);
  const double at = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  r.t = theta < 0.0 ? -at : at;
  r.c = 1.0 / sqrt(r.t * r.t + 1.0);
  r.s = r.t * r.c;
  return r;
}

#define NM_MIX(c_, s_, p_, q_)                                 \
  do {                                                         \
    const double nm_p = (p_), nm_q = (q_);                     \
    (p_) = (c_)*nm_p - (s_)*nm_q, (q_) = (s_)*nm_p + (c_)*nm_q; \
  } while (0)

#define NM_ROTATE(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q) \
  do {                                                                    \
    if ((apq) != 0.0) {                                                   \
      const NmRot nm_r = nm_angle(app, aqq, apq);                         \
      (app) = (app)-nm_r.t * (apq);                                       \
      (aqq) = (aqq) + nm_r.t * (apq);                                     \
      (apq) = 0.0;                                                        \
      NM_MIX(nm_r.c, nm_r.s, arp, arq);                                   \
      NM_MIX(nm_r.c, nm_r.s, v0p, v0q);                                   \
      NM_MIX(nm_r.c, nm_r.s, v1p, v1q);                                   \
      NM_MIX(nm_r.c, nm_r.s, v2p, v2q);                                   \
    }                                                                     \
  } while (0)

// Canonical sign of a normal: the component of largest magnitude positive, the lowest axis on a tie.
NM_HD void nm_canonical(float* n) {
  const float ax = fabsf(n[0]), ay = fabsf(n[1]), az = fabsf(n[2]);
  const float lead = (ax >= ay && ax >= az) ? n[0] : (ay >= az ? n[1] : n[2]);
  if (lead < 0.0f) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
}

// Flip n iff n . (v - p) < 0 (fp64 from the fp32 values); a zero dot, and a zero normal, stay as they are.
NM_HD void nm_orient(float* n, const float* p, const float* v) {
  NM_NO_CONTRACT
  const double dx = (double)v[0] - (double)p[0], dy = (double)v[1] - (double)p[1], dz = (double)v[2] - (double)p[2];
  const double d = ((double)n[0] * dx + (double)n[1] * dy) + (double)n[2] * dz;
  if (d < 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
}

// Normal (canonical sign), surface variation and eigenvalue gap of one neighbourhood: P the segment's n points,
// idx the k neighbour indices (a row of pn_knn3_ragged's output).  sweeps: NM_SWEEPS (a parameter so that the host
// harness can show that one sweep fewer gives the same bits).
NM_HD void nm_point(const float* P, int n, const int32_t* idx, int k, int sweeps, float* normal, float* variation,
                    float* gap) {
  NM_NO_CONTRACT
  normal[0] = normal[1] = normal[2] = 0.0f;
  *variation = 0.0f;
  *gap = 0.0f;
  if (n < 3) return;
  double mx = 0.0, my = 0.0, mz = 0.0;
  for (int i = 0; i < k; ++i) {
    int j = idx[i];
    j = j < 0 ? 0 : (j >= n ? n - 1 : j);
    mx = mx + (double)P[3 * j], my = my + (double)P[3 * j + 1], mz = mz + (double)P[3 * j + 2];
  }
  const double dk = (double)k;
  mx = mx / dk, my = my / dk, mz = mz / dk;
  double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
  for (int i = 0; i < k; ++i) {
    int j = idx[i];
    j = j < 0 ? 0 : (j >= n ? n - 1 : j);
    const double x = (double)P[3 * j] - mx, y = (double)P[3 * j + 1] - my, z = (double)P[3 * j + 2] - mz;
    a00 = a00 + x * x, a01 = a01 + x * y, a02 = a02 + x * z;
    a11 = a11 + y * y, a12 = a12 + y * z, a22 = a22 + z * z;
  }
  a00 = a00 / dk, a01 = a01 / dk, a02 = a02 / dk, a11 = a11 / dk, a12 = a12 / dk, a22 = a22 / dk;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int s = 0; s < sweeps; ++s) {
    NM_ROTATE(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0,1), r = 2
    NM_ROTATE(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0,2), r = 1
    NM_ROTATE(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1,2), r = 0
  }
  // the smallest diagonal entry, the lowest index on equal values, and its column
  double l0 = a00, nx = v00, ny = v10, nz = v20;
  if (a11 < l0) l0 = a11, nx = v01, ny = v11, nz = v21;
  if (a22 < l0) l0 = a22, nx = v02, ny = v12, nz = v22;
  const double lo01 = a00 < a11 ? a00 : a11, hi01 = a00 < a11 ? a11 : a00;
  const double l2 = hi01 < a22 ? a22 : hi01;
  const double rest = hi01 < a22 ? hi01 : a22;      // min(max(a00, a11), a22)
  double l1 = lo01 < rest ? rest : lo01;            // the median
  if (!(l2 > NM_TINY)) return;
  if (l0 < 0.0) l0 = 0.0;
  if (l1 < 0.0) l1 = 0.0;
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);   // 1 up to rounding: the columns stay orthonormal
  normal[0] = (float)(nx / len), normal[1] = (float)(ny / len), normal[2] = (float)(nz / len);
  nm_canonical(normal);
  *variation = (float)(l0 / ((l0 + l1) + l2));
  *gap = (float)((l1 - l0) / l2);
}

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
