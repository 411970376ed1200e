// Definition of the rigid registration of register.hip: iterative closest point (ICP) of a SOURCE cloud, which moves,
// onto a TARGET cloud, with the exact nearest neighbours of knn3_query.hip as correspondences.  Plain C++ behind the
// KG_HD qualifier so that the same source is compiled into the gfx950 kernels and, by the test suite only
// (tests/native/register_host.cpp), into a serial simulation of the launches.  Contraction is switched off inside every
// function here, whatever the flags of the including file; the only operations besides + - * / are sqrt, fabs and
// comparisons — no trigonometric call — so that a host compile and the device compile perform the same IEEE operations.
//
// Everything is per segment pair s of a ragged batch: a source of n_s points, a target of n_t points and, optionally, one
// fp32 normal per target point; mode RR_POINT (point to point) or RR_PLANE (point to plane, linearised); max_dist fp32,
// max_iter 1 .. RR_MAX_ITERATIONS, tol_rot and tol_trans doubles; optionally init, sixteen doubles, a row-major 4 x 4.
//
//   state       a unit quaternion q = (w, x, y, z) and a translation t, fp64.  R is ALWAYS derived from q (rr_rotation:
//               R00 = 1 - 2 (yy + zz), R01 = 2 (xy - wz), R02 = 2 (xz + wy), R10 = 2 (xy + wz), R11 = 1 - 2 (xx + zz),
//               R12 = 2 (yz - wx), R20 = 2 (xz - wy), R21 = 2 (yz + wx), R22 = 1 - 2 (xx + yy) from the nine products
//               xx .. wz), so it stays orthonormal to a few ulp however many steps are composed.
//   start       q = (1, 0, 0, 0), t = 0, or from init: t = (M03, M13, M23) and q by the extraction rule rr_from_matrix —
//               with tr = (R00 + R11) + R22, the largest of (tr, R00, R11, R22), the lowest index on equal values, picks
//                 0: (1 + tr, R21 - R12, R02 - R20, R10 - R01)        1: (R21 - R12, ((1 + R00) - R11) - R22, R01 + R10, R02 + R20)
//                 2: (R02 - R20, R01 + R10, ((1 - R00) + R11) - R22, R12 + R21)        3: (R10 - R01, R02 + R20, R12 + R21, ((1 - R00) - R11) + R22)
//               (Shepperd's rule: four times the chosen component times q), then rr_normalise (division by
//               sqrt(((w w + x x) + y y) + z z)) and the canonical sign: the first non-zero component positive.  A block
//               that is no rotation gives SOME unit quaternion: the last row of init and the block's scale are not read.
//   move        p'_i = (float)(((R00 x + R01 y) + R02 z) + t0) and likewise for the other two rows, every operation
//               rounded once in fp64, the result stored as fp32 (rr_move).
//   pair        j_i, dist_i: what pn_knn3_query_f32 returns for p' against the target with k = 1.  Accepted iff j_i >= 0
//               and dist_i <= max_dist in fp32, equality counts, +inf accepts every found pair (a NaN dist fails); in
//               RR_PLANE also rejected when the target normal has a non-finite component.  m: the accepted pairs.
//   sums        SUM of outlier_math.h (tiles of 1 024 SOURCE points from the segment's first, ol_lane_sum, ol_butterfly,
//               ol_wave_sum, tile sums in ascending order), a rejected point enters as 0.0.  Two passes as in the plane
//               refit: first pbar = SUM p' / m and qbar = SUM q / m over the accepted pairs, then the centred quantities:
//               RR_POINT  S_ab = SUM (p'_a - pbar_a) (q_b - qbar_b), nine sums, index 3 a + b.
//               RR_PLANE  c = p' - pbar, n the normal, d = p' - q, r = (nx dx + ny dy) + nz dz, the row
//                         (cy nz - cz ny, cz nx - cx nz, cx ny - cy nx, nx, ny, nz); the 21 products row_i row_j, i <= j,
//                         in row order, then the 6 products row_k r.
//   RR_POINT    Horn's matrix N00 = (Sxx + Syy) + Szz, N01 = Syz - Szy, N02 = Szx - Sxz, N03 = Sxy - Syx,
//               N11 = (Sxx - Syy) - Szz, N12 = Sxy + Syx, N13 = Szx + Sxz, N22 = (Syy - Sxx) - Szz, N23 = Syz + Szy,
//               N33 = (Szz - Sxx) - Syy; cyclic Jacobi, RR_SWEEPS sweeps over (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) with
//               the rotation of normal_math.h (nm_angle; a zero entry is skipped); dq: the column of the largest
//               diagonal entry, the lowest index on equal values, normalised, the first non-zero component positive;
//               dR = rr_rotation(dq); dt = qbar - dR pbar.  A quaternion is a rotation: never a reflection.
//   RR_SWEEPS   = 5.  On the point-mode cases of tests/test_register_abi.py (every iteration of every case but the
//               collinear one, whose top eigenvalue is double: its eigenvector never settles, it is merely defined) 4
//               sweeps are the smallest number for which one more sweep changes no bit of any output, measured on the
//               host compile; plus one.  The test re-checks that 4, 5 and 6 sweeps agree bit for bit.
//   RR_PLANE    A x = -b with A the 21 sums, b the 6, x = (omega, v), by an unpivoted LDL^T: for j = 0 .. 5
//               d_j = A_jj - SUM_{k<j} (L_jk L_jk) d_k, L_ij = (A_ij - SUM_{k<j} (L_ik L_jk) d_k) / d_j, k ascending, then
//               forward, diagonal and backward substitution.  DEGENERATE when some d_j is not above RR_PIVOT = 1e-12
//               times the largest A_jj (a plane with its normals leaves three such pivots at rounding level, 1e-16).
//               dq = rr_normalise(1, omega / 2): no trigonometry; dR = rr_rotation(dq); the step is
//               x -> dR (x - pbar) + pbar + v, so dt = (pbar + v) - dR pbar.
//   compose     q <- rr_normalise(dq (x) q), the Hamilton product written out in rr_qmul; t <- dR t + dt.
//   stop        per segment, checked in this order after the sums of iteration `it` (1-based; iterations = it):
//               NON_FINITE the target holds an inf or a NaN (the flag of the grid build) | TOO_FEW m < 3 (RR_POINT),
//               m < 6 (RR_PLANE) | DEGENERATE the solve failed or its step is not finite | the step is applied |
//               CONVERGED 2 sqrt((dq1^2 + dq2^2) + dq3^2) <= tol_rot and |((dR pbar) + dt) - pbar| <= tol_trans.
//               Otherwise the segment goes on, and has status MAX_ITER after max_iter iterations.  A stopped segment keeps
//               its state; a step that could not be solved is not applied.
//   final       one more move and pair with the final state: transform (16 doubles: R from q, t, 0 0 0 1), iterations,
//               status, count = the accepted pairs, rmse = sqrt(SUM (dist dist) / count) with dist widened to fp64, NaN
//               when count = 0, and per source point idx and dist as the query wrote them.
// A non-finite source point is never paired.  All outputs are functions of the segment pair and the arguments alone.
#pragma once
#include <math.h>

#include "normal_math.h"
#include "outlier_math.h"

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

// The six pairs of the 4 x 4 Jacobi unrolled on the device, so that its matrix is indexed by constants and lives in
// registers; the host compile keeps the loops: the operations and their order are the same.
#if defined(__HIP_DEVICE_COMPILE__)
#define RR_UNROLL _Pragma("unroll")
#else
#define RR_UNROLL
#endif

#define RR_LANES OL_LANES
#define RR_PER_LANE OL_PER_LANE
#define RR_TILE OL_TILE
#define RR_POINT 0
#define RR_PLANE 1
#define RR_MAX_ITERATIONS 256
#define RR_SWEEPS 5          // see above
#define RR_PIVOT 1e-12       // see above
#define RR_SUMS_MEAN 6       // sums per tile of the first pass
#define RR_SUMS_POINT 9      // of the second pass, RR_POINT
#define RR_SUMS_PLANE 27     // of the second pass, RR_PLANE
#define RR_MAX_SUMS 27

#define RR_CONVERGED 0
#define RR_MAX_ITER 1
#define RR_TOO_FEW 2
#define RR_DEGENERATE 3
#define RR_NON_FINITE 4
#define RR_RUNNING (-1)      // internal: no stop at this iteration

// 4 build + 1 init + per iteration (move, cells, scan, scatter, search, mean sums, means, centred sums, solve) + the
// final evaluation (move, cells, scan, scatter, search, residual sums, outputs); 0 for max_iter out of range.
KG_HD int rr_launches(int max_iter) { return max_iter < 1 || max_iter > RR_MAX_ITERATIONS ? 0 : 12 + 9 * max_iter; }

struct RrState {
  double q[4];      // (w, x, y, z), unit
  double t[3];
};

KG_HD int rr_finite(double x) { return x - x == 0.0; }
KG_HD int rr_min_pairs(int mode) { return mode == RR_PLANE ? 6 : 3; }
KG_HD int rr_second_sums(int mode) { return mode == RR_PLANE ? RR_SUMS_PLANE : RR_SUMS_POINT; }

KG_HD void rr_normalise(double* q) {
  KG_NO_CONTRACT
  const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  q[0] = q[0] / n, q[1] = q[1] / n, q[2] = q[2] / n, q[3] = q[3] / n;
}

// The first non-zero component positive.
KG_HD void rr_canonical(double* q) {
  const double lead = q[0] != 0.0 ? q[0] : (q[1] != 0.0 ? q[1] : (q[2] != 0.0 ? q[2] : q[3]));
  if (lead < 0.0) q[0] = -q[0], q[1] = -q[1], q[2] = -q[2], q[3] = -q[3];
}

KG_HD void rr_rotation(const double* q, double* R) {
  KG_NO_CONTRACT
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  R[0] = 1.0 - 2.0 * (yy + zz), R[1] = 2.0 * (xy - wz), R[2] = 2.0 * (xz + wy);
  R[3] = 2.0 * (xy + wz), R[4] = 1.0 - 2.0 * (xx + zz), R[5] = 2.0 * (yz - wx);
  R[6] = 2.0 * (xz - wy), R[7] = 2.0 * (yz + wx), R[8] = 1.0 - 2.0 * (xx + yy);
}

KG_HD RrState rr_identity(void) {
  RrState s;
  s.q[0] = 1.0, s.q[1] = s.q[2] = s.q[3] = 0.0;
  s.t[0] = s.t[1] = s.t[2] = 0.0;
  return s;
}

// The state of a row-major 4 x 4 (the extraction rule above).
KG_HD RrState rr_from_matrix(const double* M) {
  KG_NO_CONTRACT
  RrState s;
  const double r00 = M[0], r01 = M[1], r02 = M[2], r10 = M[4], r11 = M[5], r12 = M[6], r20 = M[8], r21 = M[9], r22 = M[10];
  const double tr = (r00 + r11) + r22;
  int k = 0;
  double best = tr;
  if (r00 > best) best = r00, k = 1;
  if (r11 > best) best = r11, k = 2;
  if (r22 > best) best = r22, k = 3;
  if (k == 0) {
    s.q[0] = 1.0 + tr, s.q[1] = r21 - r12, s.q[2] = r02 - r20, s.q[3] = r10 - r01;
  } else if (k == 1) {
    s.q[0] = r21 - r12, s.q[1] = ((1.0 + r00) - r11) - r22, s.q[2] = r01 + r10, s.q[3] = r02 + r20;
  } else if (k == 2) {
    s.q[0] = r02 - r20, s.q[1] = r01 + r10, s.q[2] = ((1.0 - r00) + r11) - r22, s.q[3] = r12 + r21;
  } else {
    s.q[0] = r10 - r01, s.q[1] = r02 + r20, s.q[2] = r12 + r21, s.q[3] = ((1.0 - r00) - r11) + r22;
  }
  rr_normalise(s.q);
  rr_canonical(s.q);
  s.t[0] = M[3], s.t[1] = M[7], s.t[2] = M[11];
  return s;
}

// The row-major 4 x 4 of a state.
KG_HD void rr_matrix(const RrState& s, double* M) {
  double R[9];
  rr_rotation(s.q, R);
  for (int a = 0; a < 3; ++a) {
    M[4 * a] = R[3 * a], M[4 * a + 1] = R[3 * a + 1], M[4 * a + 2] = R[3 * a + 2];
    M[4 * a + 3] = s.t[a];
  }
  M[12] = M[13] = M[14] = 0.0;
  M[15] = 1.0;
}

KG_HD void rr_rotate(const double* R, const double* v, double* out) {
  KG_NO_CONTRACT
  for (int a = 0; a < 3; ++a) out[a] = (R[3 * a] * v[0] + R[3 * a + 1] * v[1]) + R[3 * a + 2] * v[2];
}

// The move of one point: R (9) and t (3) of the state.
KG_HD void rr_move(const double* R, const double* t, const float* p, float* out) {
  KG_NO_CONTRACT
  const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
  for (int a = 0; a < 3; ++a) out[a] = (float)(((R[3 * a] * x + R[3 * a + 1] * y) + R[3 * a + 2] * z) + t[a]);
}

// Is the pair (j, dist) of a moved point accepted?  normal: null in RR_POINT, else the fp32 normal of target point j.
KG_HD int rr_accept(int j, float dist, float max_dist, const float* normal) {
  if (!(j >= 0 && dist <= max_dist)) return 0;
  return !normal || (kg_finite(normal[0]) && kg_finite(normal[1]) && kg_finite(normal[2]));
}

// The terms of an accepted pair: p the moved point, q its target point, n the normal (RR_PLANE).
KG_HD void rr_mean_terms(const float* p, const float* q, double* out) {
  out[0] = (double)p[0], out[1] = (double)p[1], out[2] = (double)p[2];
  out[3] = (double)q[0], out[4] = (double)q[1], out[5] = (double)q[2];
}
KG_HD void rr_point_terms(const float* p, const float* q, const double* mean, double* out) {
  KG_NO_CONTRACT
  const double a[3] = {(double)p[0] - mean[0], (double)p[1] - mean[1], (double)p[2] - mean[2]};
  const double b[3] = {(double)q[0] - mean[3], (double)q[1] - mean[4], (double)q[2] - mean[5]};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) out[3 * i + j] = a[i] * b[j];
}
KG_HD void rr_plane_terms(const float* p, const float* q, const float* n, const double* mean, double* out) {
  KG_NO_CONTRACT
  const double cx = (double)p[0] - mean[0], cy = (double)p[1] - mean[1], cz = (double)p[2] - mean[2];
  const double nx = (double)n[0], ny = (double)n[1], nz = (double)n[2];
  const double dx = (double)p[0] - (double)q[0], dy = (double)p[1] - (double)q[1], dz = (double)p[2] - (double)q[2];
  const double r = (nx * dx + ny * dy) + nz * dz;
  const double row[6] = {cy * nz - cz * ny, cz * nx - cx * nz, cx * ny - cy * nx, nx, ny, nz};
  int e = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) out[e++] = row[i] * row[j];
  for (int k = 0; k < 6; ++k) out[21 + k] = row[k] * r;
}
KG_HD double rr_mean(double sum, int m) {
  KG_NO_CONTRACT
  return sum / (double)m;
}
KG_HD double rr_residual_term(float dist) {
  KG_NO_CONTRACT
  return (double)dist * (double)dist;
}
KG_HD double rr_rmse(double sum, int count) {
  KG_NO_CONTRACT
  return count > 0 ? sqrt(sum / (double)count) : ol_nan();
}

// The Hamilton product a (x) b.
KG_HD void rr_qmul(const double* a, const double* b, double* out) {
  KG_NO_CONTRACT
  out[0] = ((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3];
  out[1] = ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2];
  out[2] = ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1];
  out[3] = ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0];
}

// RR_POINT: dq from the nine sums S (sweeps: RR_SWEEPS; a parameter so that the host harness can count them).
KG_HD void rr_horn(const double* S, int sweeps, double* dq) {
  NM_NO_CONTRACT
  const double sxx = S[0], sxy = S[1], sxz = S[2], syx = S[3], syy = S[4], syz = S[5], szx = S[6], szy = S[7], szz = S[8];
  double a[4][4], v[4][4];
  a[0][0] = (sxx + syy) + szz, a[0][1] = syz - szy, a[0][2] = szx - sxz, a[0][3] = sxy - syx;
  a[1][1] = (sxx - syy) - szz, a[1][2] = sxy + syx, a[1][3] = szx + sxz;
  a[2][2] = (syy - sxx) - szz, a[2][3] = syz + szy;
  a[3][3] = (szz - sxx) - syy;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      v[i][j] = i == j ? 1.0 : 0.0;
      if (j < i) a[i][j] = a[j][i];
    }
  for (int s = 0; s < sweeps; ++s)
    RR_UNROLL
    for (int p = 0; p < 3; ++p)
      RR_UNROLL
      for (int q = p + 1; q < 4; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const NmRot r = nm_angle(a[p][p], a[q][q], apq);
        a[p][p] = a[p][p] - r.t * apq;
        a[q][q] = a[q][q] + r.t * apq;
        a[p][q] = a[q][p] = 0.0;
        RR_UNROLL
        for (int k = 0; k < 4; ++k) {
          if (k != p && k != q) {
            NM_MIX(r.c, r.s, a[k][p], a[k][q]);
            a[p][k] = a[k][p], a[q][k] = a[k][q];
          }
          NM_MIX(r.c, r.s, v[k][p], v[k][q]);
        }
      }
  double top = a[0][0];                                  // (selected by moves, not by an index: registers on the device)
  dq[0] = v[0][0], dq[1] = v[1][0], dq[2] = v[2][0], dq[3] = v[3][0];
  RR_UNROLL
  for (int k = 1; k < 4; ++k)
    if (a[k][k] > top) {
      top = a[k][k];
      dq[0] = v[0][k], dq[1] = v[1][k], dq[2] = v[2][k], dq[3] = v[3][k];
    }
  rr_normalise(dq);
  rr_canonical(dq);
}

// RR_PLANE: x (6) = (omega, v) from the 27 sums; 0 when a pivot is not above RR_PIVOT times the largest diagonal entry.
KG_HD int rr_ldlt(const double* sums, double* x) {
  KG_NO_CONTRACT
  double A[6][6], L[6][6], d[6];
  int e = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = sums[e++];
  double top = A[0][0];
  for (int j = 1; j < 6; ++j) top = A[j][j] > top ? A[j][j] : top;
  const double floor_ = RR_PIVOT * top;
  for (int j = 0; j < 6; ++j) {
    double dj = A[j][j];
    for (int k = 0; k < j; ++k) dj = dj - (L[j][k] * L[j][k]) * d[k];
    if (!(dj > floor_)) return 0;
    d[j] = dj;
    for (int i = j + 1; i < 6; ++i) {
      double l = A[i][j];
      for (int k = 0; k < j; ++k) l = l - (L[i][k] * L[j][k]) * d[k];
      L[i][j] = l / dj;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {                       // L z = -b
    double z = -sums[21 + i];
    for (int k = 0; k < i; ++k) z = z - L[i][k] * y[k];
    y[i] = z;
  }
  for (int i = 0; i < 6; ++i) y[i] = y[i] / d[i];
  for (int i = 5; i >= 0; --i) {                      // L^T x = y
    double z = y[i];
    for (int k = i + 1; k < 6; ++k) z = z - L[k][i] * x[k];
    x[i] = z;
  }
  return 1;
}

// One iteration of a running segment behind its sums: the status it stops with, or RR_RUNNING.  bad: the target's
// non-finite flag; m: the accepted pairs; mean: pbar (3), qbar (3); sums: the centred sums of the mode.
KG_HD int rr_step(int mode, int bad, int m, const double* mean, const double* sums, double tol_rot, double tol_trans,
                  int sweeps, RrState* state) {
  KG_NO_CONTRACT
  if (bad) return RR_NON_FINITE;
  if (m < rr_min_pairs(mode)) return RR_TOO_FEW;
  double dq[4], dR[9], dt[3], rp[3];
  if (mode == RR_PLANE) {
    double x[6];
    if (!rr_ldlt(sums, x)) return RR_DEGENERATE;
    dq[0] = 1.0, dq[1] = x[0] / 2.0, dq[2] = x[1] / 2.0, dq[3] = x[2] / 2.0;
    rr_normalise(dq);
    rr_rotation(dq, dR);
    rr_rotate(dR, mean, rp);
    for (int a = 0; a < 3; ++a) dt[a] = (mean[a] + x[3 + a]) - rp[a];
  } else {
    rr_horn(sums, sweeps, dq);
    rr_rotation(dq, dR);
    rr_rotate(dR, mean, rp);
    for (int a = 0; a < 3; ++a) dt[a] = mean[3 + a] - rp[a];
  }
  RrState next;
  rr_qmul(dq, state->q, next.q);
  rr_normalise(next.q);
  double rt[3];
  rr_rotate(dR, state->t, rt);
  int ok = 1;
  for (int a = 0; a < 3; ++a) {
    next.t[a] = rt[a] + dt[a];
    ok &= rr_finite(next.t[a]);
  }
  for (int a = 0; a < 4; ++a) ok &= rr_finite(next.q[a]);
  if (!ok) return RR_DEGENERATE;
  *state = next;
  const double rot = 2.0 * sqrt((dq[1] * dq[1] + dq[2] * dq[2]) + dq[3] * dq[3]);
  const double e0 = (rp[0] + dt[0]) - mean[0], e1 = (rp[1] + dt[1]) - mean[1], e2 = (rp[2] + dt[2]) - mean[2];
  const double shift = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
  return rot <= tol_rot && shift <= tol_trans ? RR_CONVERGED : RR_RUNNING;
}

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
