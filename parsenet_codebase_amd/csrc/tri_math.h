// Arithmetic of the exact point-to-trimmed-surface distance (tridist.hip): the squared distance from a point to a
// triangle and the certified bounds of the distance to a bounding sphere of a group of triangles.  fp32, plain C++
// behind the TM_HD qualifier so that the SAME source is compiled into the gfx950 kernels and, by the test suite only
// (tests/native/tri_math_host.cpp), into a host harness that checks it against a float64 restatement.  Every
// multiply and add is rounded once: contraction is switched off inside every function here, whatever the flags of
// the including file.
//
// The distance.  d(p, T) = min over the three edges of the point-to-segment distance, and, when the projection of p
// onto the plane of T falls inside T, the plane distance — exact for the face interior, the three edges and the
// three vertices, since the nearest point of a triangle lies either inside the face (then it is the projection) or
// on the boundary (then it is the nearest point of some edge).  The point-independent part is formed once per
// triangle (tm_make, a 16-float record): the vertex a, the edges u = b - a, v = c - a, the normal n = u x v and
// the reciprocals of |u|^2, |v|^2, |c - b|^2 and |n|^2.
//   * tm_make first ROTATES (a, b, c) — orientation and triangle unchanged — so that a lies opposite the longest
//     edge: the angle at a is then the largest one, at least 60 degrees, and for a needle (two long edges and a short
//     one: the rings next to a sphere's pole) close to 90: u x v is formed without the cancellation that the
//     product of two nearly parallel long edges suffers.
//   * Degenerate triangles.  A reciprocal is 0 when its denominator is below TM_TINY: an edge of zero length then
//     has t = 0, the distance to its vertex.  The plane term is dropped (in = 0) when |n|^2 <= TM_TOL2 |u|^2 |v|^2,
//     sin(angle at a) <= 2^-11: the three vertices are collinear to within what fp32 can tell (the components of
//     n carry an absolute error of about 2.5e-7 |u||v|, so at the threshold its direction is known to 5e-4 rad;
//     below it it is noise).  Such a triangle is its own boundary to within 2^-11 of an edge length, which the three
//     segments cover.  Two equal vertices, three equal vertices and three collinear vertices give n = 0 exactly.
//     No division by zero, no 0 * inf: every value that reaches the minimum is finite for finite input.
//   * The inside test reads the signs of (u x ap).n, (ap x v).n and (w x bp).n, the three barycentric coordinates
//     times |n|^2.  A sign taken wrongly by rounding moves the result by a second-order amount only: just outside an
//     edge the plane distance and the edge distance differ by the squared in-plane offset.
//
// The bounds.  A group of triangles lies in the ball (c, r): c is the centre of the bounding box of its vertices,
// r = sqrtf(max |vertex - c|^2) (1 + 2^-9) (a triangle is the convex hull of its vertices).  For a point p with
// D = |p - c|, every triangle T of the group has   D - r0 <= d(p, T) <= D + r0   (r0 the true radius).  The bounds
// are compared with COMPUTED distances (skipping must not change a bit of the result), so they allow for the error
// of both sides:
//     D as computed carries a relative error below 4 * 2^-24;
//     a computed segment distance differs from the true one by at most about 4 * 2^-24 (|ap| + |e|) <= 2^-21 (D + 3 r0);
//     a computed plane distance uses a normal whose direction is off by rho <= 5e-4 rad (see above; 1e-6 for a
//     well-shaped triangle): it differs from the true one by at most rho x (in-plane offset <= 2 r0) + D rho^2 / 2
//     <= 2^-10 r0 + 2^-22 D.
//   lower:  lb = max(0, D (1 - 2^-19) - r),  lb2 = lb^2 (1 - 2^-19)  — the 2^-19 D covers the first, second and the D
//           part of the third item with a factor of four to spare, and r - r0 >= 2^-9 r0 covers the r0 parts, so
//           lb2 never exceeds the true nor the computed squared distance to any triangle of the group;
//   upper:  ub = D (1 + 2^-19) + r,  ub2 = ub^2 (1 + 2^-19)  — never below them, by the same items.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define TM_HD __host__ __device__ static inline
#else
#define TM_HD static inline
#endif
#if defined(__clang__)
#define TM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TM_NO_CONTRACT
#if defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
#endif

#define TM_NREC 16                       // floats per triangle record
#define TM_GROUP 8                       // consecutive triangles per bounding sphere
#define TM_TINY 1e-30f                   // denominators below this are treated as zero
#define TM_TOL2 2.384185791015625e-07f   // 2^-22: sin^2 of the angle at a below which the plane term is dropped
#define TM_FAR 3e18f                     // vertex of a padding record: never the minimum of finite input
#define TM_DOWN 0.99999809265136719f     // 1 - 2^-19
#define TM_UP 1.0000019073486328f        // 1 + 2^-19
#define TM_RADIUS_UP 1.001953125f        // 1 + 2^-9

struct TmTri {
  float ax, ay, az;     // vertex a (opposite the longest edge)
  float ux, uy, uz;     // b - a
  float vx, vy, vz;     // c - a
  float nx, ny, nz;     // u x v
  float iu, iv, iw;     // 1 / |u|^2, 1 / |v|^2, 1 / |c - b|^2, or 0
  float in;             // 1 / |n|^2, or 0: no plane term
};

TM_HD float tm_dot(float ax, float ay, float az, float bx, float by, float bz) {
  TM_NO_CONTRACT
  return (ax * bx + ay * by) + az * bz;
}

TM_HD float tm_inv(float x) { return x >= TM_TINY ? 1.0f / x : 0.0f; }

TM_HD TmTri tm_make(const float* p0, const float* p1, const float* p2) {
  TM_NO_CONTRACT
  const float e01 = tm_dot(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2], p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]);
  const float e12 = tm_dot(p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2], p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]);
  const float e20 = tm_dot(p0[0] - p2[0], p0[1] - p2[1], p0[2] - p2[2], p0[0] - p2[0], p0[1] - p2[1], p0[2] - p2[2]);
  // (selected value by value, not through a pointer: the vertices stay in registers)
  const int rot = (e20 > e12 && e20 >= e01) ? 1 : (e01 > e12 && e01 > e20) ? 2 : 0;
  float a[3], b[3], c[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = rot == 0 ? p0[k] : rot == 1 ? p1[k] : p2[k];   // longest edge p1 p2: as given;
    b[k] = rot == 0 ? p1[k] : rot == 1 ? p2[k] : p0[k];   // p2 p0: (p1, p2, p0);
    c[k] = rot == 0 ? p2[k] : rot == 1 ? p0[k] : p1[k];   // p0 p1: (p2, p0, p1)
  }
  TmTri t;
  t.ax = a[0], t.ay = a[1], t.az = a[2];
  t.ux = b[0] - a[0], t.uy = b[1] - a[1], t.uz = b[2] - a[2];
  t.vx = c[0] - a[0], t.vy = c[1] - a[1], t.vz = c[2] - a[2];
  const float wx = c[0] - b[0], wy = c[1] - b[1], wz = c[2] - b[2];
  t.nx = t.uy * t.vz - t.uz * t.vy;
  t.ny = t.uz * t.vx - t.ux * t.vz;
  t.nz = t.ux * t.vy - t.uy * t.vx;
  const float uu = tm_dot(t.ux, t.uy, t.uz, t.ux, t.uy, t.uz);
  const float vv = tm_dot(t.vx, t.vy, t.vz, t.vx, t.vy, t.vz);
  const float nn = tm_dot(t.nx, t.ny, t.nz, t.nx, t.ny, t.nz);
  t.iu = tm_inv(uu);
  t.iv = tm_inv(vv);
  t.iw = tm_inv(tm_dot(wx, wy, wz, wx, wy, wz));
  t.in = nn > TM_TOL2 * (uu * vv) ? tm_inv(nn) : 0.0f;
  return t;
}

// a record no finite point is nearest to (fills a shape's last group)
TM_HD TmTri tm_pad(void) {
  TmTri t;
  t.ax = t.ay = t.az = TM_FAR;
  t.ux = t.uy = t.uz = t.vx = t.vy = t.vz = t.nx = t.ny = t.nz = 0.0f;
  t.iu = t.iv = t.iw = t.in = 0.0f;
  return t;
}

// squared distance from the point at offset (x, y, z) of a segment's start to the segment along e, ie = 1/|e|^2 or 0
TM_HD float tm_seg2(float x, float y, float z, float ex, float ey, float ez, float ie) {
  TM_NO_CONTRACT
  const float t = fminf(fmaxf(tm_dot(x, y, z, ex, ey, ez) * ie, 0.0f), 1.0f);
  const float rx = x - t * ex, ry = y - t * ey, rz = z - t * ez;
  return tm_dot(rx, ry, rz, rx, ry, rz);
}

// (e x q) . n
TM_HD float tm_side(float ex, float ey, float ez, float qx, float qy, float qz, float nx, float ny, float nz) {
  TM_NO_CONTRACT
  return tm_dot(ey * qz - ez * qy, ez * qx - ex * qz, ex * qy - ey * qx, nx, ny, nz);
}

TM_HD float tm_dist2(float px, float py, float pz, const TmTri& t) {
  TM_NO_CONTRACT
  const float ax = px - t.ax, ay = py - t.ay, az = pz - t.az;        // p - a
  const float bx = ax - t.ux, by = ay - t.uy, bz = az - t.uz;        // p - b
  const float wx = t.vx - t.ux, wy = t.vy - t.uy, wz = t.vz - t.uz;  // c - b
  float d = fminf(fminf(tm_seg2(ax, ay, az, t.ux, t.uy, t.uz, t.iu), tm_seg2(ax, ay, az, t.vx, t.vy, t.vz, t.iv)),
                  tm_seg2(bx, by, bz, wx, wy, wz, t.iw));
  const float s_v = tm_side(t.ux, t.uy, t.uz, ax, ay, az, t.nx, t.ny, t.nz);   // coordinate along v, times |n|^2
  const float s_u = tm_side(ax, ay, az, t.vx, t.vy, t.vz, t.nx, t.ny, t.nz);   // along u
  const float s_a = tm_side(wx, wy, wz, bx, by, bz, t.nx, t.ny, t.nz);         // weight of a
  const float h = tm_dot(ax, ay, az, t.nx, t.ny, t.nz);
  const float plane = (h * h) * t.in;
  const bool inside = t.in > 0.0f && s_v >= 0.0f && s_u >= 0.0f && s_a >= 0.0f;
  return inside ? fminf(d, plane) : d;
}

// ---- bounding sphere of a group and the certified bounds (derivation at the head of the file) ----------------------
TM_HD float tm_centre(float lo, float hi) {
  TM_NO_CONTRACT
  return 0.5f * lo + 0.5f * hi;
}

TM_HD float tm_radius(float r2max) { return sqrtf(r2max) * TM_RADIUS_UP; }

TM_HD float tm_sq(float px, float py, float pz, float cx, float cy, float cz) {
  TM_NO_CONTRACT
  const float dx = px - cx, dy = py - cy, dz = pz - cz;
  return tm_dot(dx, dy, dz, dx, dy, dz);
}

TM_HD float tm_centre_dist(float px, float py, float pz, float cx, float cy, float cz) {
  return sqrtf(tm_sq(px, py, pz, cx, cy, cz));
}

// lower bound of the squared distance from p to every triangle inside the ball (c, r)
TM_HD float tm_lower2(float px, float py, float pz, float cx, float cy, float cz, float r) {
  TM_NO_CONTRACT
  const float lb = fmaxf(tm_centre_dist(px, py, pz, cx, cy, cz) * TM_DOWN - r, 0.0f);
  return (lb * lb) * TM_DOWN;
}

// upper bound of the squared distance from p to any triangle inside the ball (c, r)
TM_HD float tm_upper2(float px, float py, float pz, float cx, float cy, float cz, float r) {
  TM_NO_CONTRACT
  const float ub = tm_centre_dist(px, py, pz, cx, cy, cz) * TM_UP + r;
  return (ub * ub) * TM_UP;
}

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
