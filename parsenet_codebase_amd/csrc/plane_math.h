// Definition of the dominant-plane extraction of plane.hip: the plane that holds the most points of a cloud within a
// threshold, found by scoring H sampled planes against every point (RANSAC) and refined by least squares through its
// inliers.  Plain C++ behind the KG_HD qualifier so that the same source is compiled into the gfx950 kernels and, by
// the test suite only (tests/native/plane_host.cpp), into a serial simulation of the launches.  Contraction is switched
// off inside every function here, whatever the flags of the including file.
//
// Everything is per segment (one cloud of a ragged batch) of n points, indices LOCAL to it, and a function of the cloud
// and the call's arguments alone: t (one fp32 threshold per segment), H (1 .. PL_MAX_H hypotheses), seed (64 bits),
// refine (0 .. PL_MAX_REFINE rounds) and, optionally, a unit axis with min_cos (doubles).
//
//   sample      hypothesis h draws i_s = ((pl_mix(seed + PL_GOLD (3 h + s + 1)) >> 32) n) >> 32 for s = 0, 1, 2, all
//               arithmetic mod 2^64; pl_mix is the splitmix64 finaliser.  No re-draw: two equal indices make the
//               hypothesis invalid, and so does n < 3.
//   plane       in fp64 from the fp32 coordinates, every operation rounded once, no fma: a = p1 - p0, b = p2 - p0,
//               c = a x b (each component u v - w z: two products, one subtraction), len2 = (cx^2 + cy^2) + cz^2 —
//               invalid unless len2 > 0 and finite —, n = c / sqrt(len2) with the canonical sign (the component of
//               largest magnitude positive, the lowest axis on a tie), d = -((nx x0 + ny y0) + nz z0).
//   axis        with an axis a hypothesis is invalid unless |((nx ax + ny ay) + nz az)| >= min_cos.
//   inlier      p is an inlier of (n, d) iff |((nx x + ny y) + nz z) + d| <= (double) t.  Equality counts.  The count of
//               a plane is an integer: no order of arrival shows in it.
//   selection   the valid hypothesis with the most inliers, the lowest h on equal counts: the maximum of
//               pl_key(count, h) = (count << 32) | (0xFFFFFFFF - h), which is never 0 for a valid h.  No valid
//               hypothesis: best = -1, count = 0, plane zeros, no inlier.
//   refinement  `refine` rounds.  With the inliers of the current plane and their count m: the mean (three sums / m),
//               then the six centred second moments xx, xy, xz, yy, yz, zz (sums of products of the fp64 differences
//               to the mean, / m).  Every sum is SUM of outlier_math.h — tiles of 1 024 points, ol_lane_sum,
//               ol_butterfly, ol_wave_sum, tile sums in ascending order —, a non-inlier enters as 0.0.  The cyclic
//               Jacobi of normal_math.h with NM_SWEEPS sweeps gives the eigenvector of the smallest eigenvalue,
//               renormalised, canonical sign; d = -((nx mx + ny my) + nz mz).  The refit is taken, with its own inliers,
//               iff m >= 3, the largest eigenvalue is above NM_TINY, it satisfies the axis constraint and it has at
//               least as many inliers as the plane it came from.  Otherwise the plane stays — and, the refit being a
//               function of the plane, so it does in every later round.  Refinement never loses inliers.
//   outputs     per segment plane (4) fp64, count and best int32 — best is the winning h whatever the refinement did —;
//               per point inlier (one byte) and, optionally, dist fp32: ((nx x + ny y) + nz z) + d formed in fp64 and
//               rounded once; NaN where the segment has no plane.
//   status      in count, with best -1, plane zeros, no inlier: PL_NON_FINITE (-1) for a segment that holds an inf or a
//               NaN coordinate, PL_BAD_THRESHOLD (-2) where t is not a positive finite number.
//
// How plane.hip computes it.  A point belongs to one tile of PL_TILE points of its segment (the tiles of fps_math.h:
// PL_LANES lanes, PL_PER_LANE points each, lane-interleaved), a tile to one workgroup.  pl_launches(refine) launches:
// bounds (tile table, non-finite flags, counters zeroed) | hypotheses | scores | selection | per round: mean partials,
// mean, moment partials, moments + Jacobi, the refit's count, the decision | inlier and dist.
#pragma once
#include <math.h>

#include "normal_math.h"
#include "outlier_math.h"

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

#define PL_LANES OL_LANES
#define PL_PER_LANE OL_PER_LANE
#define PL_TILE OL_TILE
#define PL_MAX_H 4096
#define PL_MAX_REFINE 4
#define PL_NON_FINITE (-1)
#define PL_BAD_THRESHOLD (-2)
#define PL_GOLD 0x9E3779B97F4A7C15ull
#define PL_MOMENTS 6                    // sums per tile of a refinement launch: 3 for the mean, 6 for the moments

struct PlPlane {
  double nx, ny, nz, d;
  int valid;
};

KG_HD int pl_launches(int refine) { return refine < 0 || refine > PL_MAX_REFINE ? 0 : 5 + 6 * refine; }

KG_HD unsigned long long pl_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Index s = 0, 1, 2 of hypothesis h in a segment of n >= 1 points: below n, because the hash is below 2^32.
KG_HD int pl_draw(unsigned long long seed, int h, int s, int n) {
  const unsigned long long u = pl_mix(seed + PL_GOLD * (unsigned long long)(3ll * h + s + 1)) >> 32;
  return (int)((u * (unsigned long long)n) >> 32);
}

KG_HD int pl_finite(double x) { return x - x == 0.0; }

KG_HD int pl_threshold_ok(float t) { return t > 0.0f && kg_finite(t); }

// 0, or the status of a segment: `bad` is its non-finite flag, t its threshold.
KG_HD int pl_status(int bad, float t) { return bad ? PL_NON_FINITE : (pl_threshold_ok(t) ? 0 : PL_BAD_THRESHOLD); }

KG_HD PlPlane pl_none(void) {
  PlPlane p;
  p.nx = p.ny = p.nz = p.d = 0.0;
  p.valid = 0;
  return p;
}

// Canonical sign of a normal: the component of largest magnitude positive, the lowest axis on a tie (nm_canonical, on
// the fp64 values).
KG_HD void pl_canonical(double* nx, double* ny, double* nz) {
  const double ax = fabs(*nx), ay = fabs(*ny), az = fabs(*nz);
  const double lead = (ax >= ay && ax >= az) ? *nx : (ay >= az ? *ny : *nz);
  if (lead < 0.0) *nx = -*nx, *ny = -*ny, *nz = -*nz;
}

KG_HD double pl_dot(double nx, double ny, double nz, double x, double y, double z) {
  KG_NO_CONTRACT
  return (nx * x + ny * y) + nz * z;
}

// Does the normal pass the axis constraint?  axis: null, or three doubles.
KG_HD int pl_axis_ok(double nx, double ny, double nz, const double* axis, double min_cos) {
  return !axis || fabs(pl_dot(nx, ny, nz, axis[0], axis[1], axis[2])) >= min_cos;
}

// The plane through three points of the segment.
KG_HD PlPlane pl_from_points(const float* p0, const float* p1, const float* p2, const double* axis, double min_cos) {
  KG_NO_CONTRACT
  PlPlane p = pl_none();
  const double x0 = (double)p0[0], y0 = (double)p0[1], z0 = (double)p0[2];
  const double ax = (double)p1[0] - x0, ay = (double)p1[1] - y0, az = (double)p1[2] - z0;
  const double bx = (double)p2[0] - x0, by = (double)p2[1] - y0, bz = (double)p2[2] - z0;
  const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  const double len2 = (cx * cx + cy * cy) + cz * cz;
  if (!(len2 > 0.0) || !pl_finite(len2)) return p;
  const double len = sqrt(len2);
  double nx = cx / len, ny = cy / len, nz = cz / len;
  pl_canonical(&nx, &ny, &nz);
  if (!pl_axis_ok(nx, ny, nz, axis, min_cos)) return p;
  p.nx = nx, p.ny = ny, p.nz = nz;
  p.d = -pl_dot(nx, ny, nz, x0, y0, z0);
  p.valid = 1;
  return p;
}

// Hypothesis h of a segment of n points P.
KG_HD PlPlane pl_hypothesis(const float* P, int n, unsigned long long seed, int h, const double* axis, double min_cos) {
  if (n < 3) return pl_none();
  const int i0 = pl_draw(seed, h, 0, n), i1 = pl_draw(seed, h, 1, n), i2 = pl_draw(seed, h, 2, n);
  if (i0 == i1 || i0 == i2 || i1 == i2) return pl_none();
  return pl_from_points(P + 3 * (size_t)i0, P + 3 * (size_t)i1, P + 3 * (size_t)i2, axis, min_cos);
}

KG_HD double pl_signed(double nx, double ny, double nz, double d, double x, double y, double z) {
  KG_NO_CONTRACT
  return pl_dot(nx, ny, nz, x, y, z) + d;
}
KG_HD int pl_inlier(double s, double t) { return fabs(s) <= t; }

KG_HD unsigned long long pl_key(uint32_t count, uint32_t h) {
  return ((unsigned long long)count << 32) | (unsigned long long)(0xFFFFFFFFu - h);
}
KG_HD int pl_key_h(unsigned long long key) { return key ? (int)(0xFFFFFFFFu - (uint32_t)key) : -1; }
KG_HD int pl_key_count(unsigned long long key) { return (int)(key >> 32); }

// What a point adds to the sums of a refinement round.
KG_HD double pl_term(int inlier, double x) { return inlier ? x : 0.0; }
KG_HD double pl_mean(double sum, int m) {
  KG_NO_CONTRACT
  return sum / (double)m;
}
// The six centred products of a point in the order xx, xy, xz, yy, yz, zz.
KG_HD void pl_products(double x, double y, double z, const double* mean, double* out) {
  KG_NO_CONTRACT
  const double dx = x - mean[0], dy = y - mean[1], dz = z - mean[2];
  out[0] = dx * dx, out[1] = dx * dy, out[2] = dx * dz;
  out[3] = dy * dy, out[4] = dy * dz, out[5] = dz * dz;
}

// The refit of a round: mean and the six moment SUMS over the m inliers.  Not valid when it is degenerate (m < 3 or the
// largest eigenvalue at or below NM_TINY) or fails the axis constraint.  The rotations are nm_point's, word for word.
KG_HD PlPlane pl_refit(const double* mean, const double* sums, int m, const double* axis, double min_cos) {
  NM_NO_CONTRACT
  PlPlane p = pl_none();
  if (m < 3) return p;
  const double dm = (double)m;
  double a00 = sums[0] / dm, a01 = sums[1] / dm, a02 = sums[2] / dm;
  double a11 = sums[3] / dm, a12 = sums[4] / dm, a22 = sums[5] / dm;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int s = 0; s < NM_SWEEPS; ++s) {
    NM_ROTATE(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0,1), r = 2
    NM_ROTATE(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0,2), r = 1
    NM_ROTATE(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1,2), r = 0
  }
  double l0 = a00, nx = v00, ny = v10, nz = v20;
  if (a11 < l0) l0 = a11, nx = v01, ny = v11, nz = v21;
  if (a22 < l0) l0 = a22, nx = v02, ny = v12, nz = v22;
  const double hi01 = a00 < a11 ? a11 : a00;
  const double l2 = hi01 < a22 ? a22 : hi01;
  if (!(l2 > NM_TINY)) return p;
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  nx = nx / len, ny = ny / len, nz = nz / len;
  pl_canonical(&nx, &ny, &nz);
  if (!pl_axis_ok(nx, ny, nz, axis, min_cos)) return p;
  p.nx = nx, p.ny = ny, p.nz = nz;
  p.d = -pl_dot(nx, ny, nz, mean[0], mean[1], mean[2]);
  p.valid = 1;
  return p;
}

// Is the refit with `refit_count` inliers taken over a plane with `count`?
KG_HD int pl_take(int refit_valid, int refit_count, int count) { return refit_valid && refit_count >= count; }

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
