// Test-only host harness around parsenet_codebase_amd/csrc/tri_math.h (the arithmetic tridist.hip runs per point and
// triangle), so that tests/test_tridist_abi.py can hold it against a float64 restatement without a GPU.  Not part of
// the product library.
#include "../../parsenet_codebase_amd/csrc/tri_math.h"

// out[i * nt + j] = squared distance from point i to triangle j (tri: nt x 9 floats, the three vertices)
extern "C" void tmh_dist2(const float* P, int np, const float* tri, int nt, float* out) {
  for (int j = 0; j < nt; ++j) {
    const TmTri t = tm_make(tri + 9 * j, tri + 9 * j + 3, tri + 9 * j + 6);
    for (int i = 0; i < np; ++i) out[(size_t)i * nt + j] = tm_dist2(P[3 * i], P[3 * i + 1], P[3 * i + 2], t);
  }
}

// the 16-float records themselves
extern "C" void tmh_records(const float* tri, int nt, float* rec) {
  for (int j = 0; j < nt; ++j) {
    const TmTri t = tm_make(tri + 9 * j, tri + 9 * j + 3, tri + 9 * j + 6);
    const float* f = &t.ax;
    for (int k = 0; k < TM_NREC; ++k) rec[(size_t)j * TM_NREC + k] = f[k];
  }
}

// Bounding spheres of the groups of TM_GROUP consecutive triangles (the last group may be short), formed as the record
// pass forms them, and both bounds of every point against every group: sph (ng x 4), lower / upper (np x ng).
extern "C" int tmh_bounds(const float* P, int np, const float* tri, int nt, float* sph, float* lower, float* upper) {
  const int ng = (nt + TM_GROUP - 1) / TM_GROUP;
  for (int g = 0; g < ng; ++g) {
    const int j0 = g * TM_GROUP, j1 = j0 + TM_GROUP < nt ? j0 + TM_GROUP : nt;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int j = j0; j < j1; ++j)
      for (int v = 0; v < 3; ++v)
        for (int k = 0; k < 3; ++k) {
          lo[k] = fminf(lo[k], tri[9 * j + 3 * v + k]);
          hi[k] = fmaxf(hi[k], tri[9 * j + 3 * v + k]);
        }
    const float c[3] = {tm_centre(lo[0], hi[0]), tm_centre(lo[1], hi[1]), tm_centre(lo[2], hi[2])};
    float r2 = 0.0f;
    for (int j = j0; j < j1; ++j)
      for (int v = 0; v < 3; ++v) {
        const float* q = tri + 9 * j + 3 * v;
        r2 = fmaxf(r2, tm_sq(q[0], q[1], q[2], c[0], c[1], c[2]));
      }
    const float r = tm_radius(r2);
    sph[4 * g] = c[0], sph[4 * g + 1] = c[1], sph[4 * g + 2] = c[2], sph[4 * g + 3] = r;
    for (int i = 0; i < np; ++i) {
      lower[(size_t)i * ng + g] = tm_lower2(P[3 * i], P[3 * i + 1], P[3 * i + 2], c[0], c[1], c[2], r);
      upper[(size_t)i * ng + g] = tm_upper2(P[3 * i], P[3 * i + 1], P[3 * i + 2], c[0], c[1], c[2], r);
    }
  }
  return ng;
}

extern "C" int tmh_group(void) { return TM_GROUP; }
