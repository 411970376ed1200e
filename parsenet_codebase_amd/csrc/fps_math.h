// Definition of the farthest-point sampling of fps.hip: an exact, bit-reproducible reduction of a cloud of any size to
// m samples that cover it, and for every point the sample that is nearest to it.  Plain C++ behind KG_HD so that the
// same source is compiled into the gfx950 kernels and, by the test suite only (tests/native/fps_host.cpp), into a serial
// restatement of the whole schedule.  Contraction is switched off inside every function here.
//
// Everything is per segment (one cloud of a ragged batch) of n points, indices LOCAL to it; m_c = min(m, n).
//
//   distance    d(i,j) = ((x_i - x_j)^2 + (y_i - y_j)^2) + (z_i - z_j)^2, every operation rounded once in fp32, no fma:
//               kg_dist of knn3_grid_math.h.  fl(a - b) = -fl(b - a) and the square drops the sign, so d(i,j) and
//               d(j,i) are the same bits.  On finite coordinates d is never NaN and never negative (it can overflow to
//               +inf, which the strict comparison below then never takes).
//   state       D_i = +inf and owner_i = -1 for every point; s_0 = start, clamped into [0, n - 1].
//   step t      (t = 0 .. m_c - 1)  radius_t = D_{s_t} (so radius_0 = +inf); s_t is marked chosen, D = 0, owner = t;
//               every unchosen i takes nd = d(i, s_t) and, if nd < D_i (strict), D_i = nd and owner_i = t;
//               s_{t+1} is the unchosen point with the largest D, the lowest index on equal D.
//   outputs     sample (m) the s_t, -1 from m_c on; radius (m), NaN from m_c on; owner (n) and dist (n) the final state.
//   non-finite  a segment that holds an inf or a NaN coordinate: sample -1, radius NaN, owner -1, dist NaN throughout.
//
// Three properties hold exactly, because the state only ever moves by comparisons of fp32 numbers:
//   (1) radius is non-increasing over t >= 1.  radius_{t+1} is the largest D among the points unchosen after step t.
//       Every one of them was unchosen before step t as well, where its D was no smaller (a D only ever drops) and
//       where the largest D was radius_t.
//   (2) d(s_t, s_u) >= radius_u for t < u.  radius_u is the D of s_u when it is chosen: the minimum of d(s_u, s_v) over
//       v < u (strict updates from +inf keep the exact minimum), hence <= d(s_u, s_t), which is d(s_t, s_u) bit for bit.
//   (3) every final dist <= radius_{m_c - 1} (+inf when m_c = 1).  A chosen point has 0 <= any radius.  A point still
//       unchosen at the end was unchosen before the last step, where the largest D was radius_{m_c - 1}; it has not
//       grown since.
//
// How fps.hip computes it.  A point belongs to one tile of FPS_TILE points of its segment (FPS_LANES lanes, FPS_PER_LANE
// points each, lane-interleaved), a tile to one workgroup.  The working D lives in a workspace and holds FPS_CHOSEN
// (-1) for a chosen point: no d is below it, so a chosen point is never updated, and it offers no candidate.  The
// candidate of a point is the key (bits of D) << 32 | (0xFFFFFFFF - i): D >= 0, so its bits order as its value, and the
// inverted index makes the lowest index win.  A real key is never 0 (i < 2^31); 0 means "no candidate".  s_{t+1} is
// the maximum of the keys — of a tile first, then of the tiles, by a 64-bit integer atomicMax on slot (c, t + 1) —
// and an integer maximum does not depend on the order of arrival.  Slot (c, t) therefore holds (radius_t, s_t), the
// start as (+inf, start), and the last launch only decodes the slots.
//
// Tiles without a prefix sum: segment c owns the tile numbers fps_tile_base(off[c], c) .. fps_tile_base(off[c+1], c+1)
// - 1, with fps_tile_base(o, c) = o / FPS_TILE + c.  floor((o + n) / T) - floor(o / T) + 1 >= ceil(n / T), so the range
// always holds the tiles the segment needs (the spare ones exit at once), the bases strictly increase with c, and the
// whole batch has total / FPS_TILE + S tile numbers — a host integer.  The first launch searches the bases once and
// writes the flat table tile -> (segment, first point) that the m step launches read.
#pragma once
#include "knn3_grid_math.h"
#include "ragged.h"

#define FPS_LANES 256                          // lanes per workgroup
#define FPS_PER_LANE 4                         // points per lane: four independent 12-byte rows in flight
#define FPS_TILE (FPS_LANES * FPS_PER_LANE)    // points per workgroup and step
#define FPS_CHOSEN (-1.0f)                     // the working D of a chosen point
#define FPS_NO_KEY 0ull

KG_HD int fps_launches(int m) { return m + 2; }     // init, the m steps, outputs

// 64-bit slots of one segment: (radius_t, s_t) for t = 0 .. m (slot m takes the candidates of the last step and is
// never read), then the non-finite flag.
KG_HD long long fps_slots(int m) { return (long long)m + 2; }
KG_HD long long fps_flag_slot(int m) { return (long long)m + 1; }

KG_HD long long fps_tile_base(int o, int c) { return (long long)(o / FPS_TILE) + c; }
KG_HD long long fps_tiles(long long total, int S) { return total / FPS_TILE + S; }

KG_HD unsigned long long fps_key(float D, uint32_t i) {
  return ((unsigned long long)kg_bits(D) << 32) | (unsigned long long)(0xFFFFFFFFu - i);
}
KG_HD uint32_t fps_key_index(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)key; }
KG_HD float fps_key_dist(unsigned long long key) { return kg_float((uint32_t)(key >> 32)); }

KG_HD int fps_clamp_start(int s, int n) { return s < 0 ? 0 : (s > n - 1 ? n - 1 : s); }

// Is (o0, o1) a segment inside 0 .. total?
KG_HD int fps_valid_segment(int o0, int o1, int total) { return rg_valid_segment(o0, o1, total); }

// Step t at point i (coordinates p, working distance *D) against the sample s (coordinates q): the new working
// distance in *D, 1 if the point's owner becomes t, and the point's candidate key as the return value.
KG_HD unsigned long long fps_point_step(const float* p, const float* q, uint32_t i, uint32_t s, float* D, int* owned) {
  float d = *D;
  *owned = 0;
  if (i == s) {
    d = FPS_CHOSEN;
    *owned = 1;
  } else {
    const float nd = kg_dist(p[0], p[1], p[2], q[0], q[1], q[2]);
    if (nd < d) {
      d = nd;
      *owned = 1;
    }
  }
  *D = d;
  return d >= 0.0f ? fps_key(d, i) : FPS_NO_KEY;
}

// The final distance of a working D.
KG_HD float fps_final_dist(float D) { return D < 0.0f ? 0.0f : D; }
