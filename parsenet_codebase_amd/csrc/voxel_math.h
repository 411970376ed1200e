// Definition of the voxel-grid downsampling of voxel.hip: one point per occupied cell of a cubic grid — the exact
// centroid of the cell's points and the scanned point nearest to it — and for every point the voxel that holds it, as
// an exact, bit-reproducible function of the cloud, the voxel size and the origin alone, on clouds of any size.  Plain
// C++ behind KG_HD so that the same source is compiled into the gfx950 kernels and, by the test suite only
// (tests/native/voxel_host.cpp), into a serial restatement of the whole schedule.  Contraction is switched off inside
// every function here.
//
// Everything is per segment (one cloud of a ragged batch) of n points, indices LOCAL to it.  Given the voxel size h
// (fp32) and an optional origin o (3 fp32):
//
//   bounds      lo, hi: min and max per axis of the fp32 coordinates.  Without an origin, o = lo.
//   cell        c_a = floor(((double) x_a - (double) o_a) / (double) h): subtraction, division and floor in fp64, each
//               rounded once (IEEE division: the build uses no fast-math flag, and neither hipcc nor g++ relaxes an
//               fp64 division without one).  A point on a face belongs to the upper cell.
//   status      -1  the segment holds an inf or a NaN coordinate;
//               -2  "voxel too small for the extent": some c_a outside [-2^20, 2^20), or h not a positive finite
//                   number, or an origin that is not finite (the quotient is then no number in the range);
//               both give nvox = status, owner = -1 throughout and no voxel rows.  -1 wins over -2.
//   voxels      a voxel is the set of points with the same cell triple.  Voxels are numbered 0 .. V - 1 by the
//               ascending lowest point index they hold (first); owner_i is the number of i's voxel.  Hence
//               owner_0 = 0 and first ascends.  nvox = V.
//   centroid    exact, whatever the order of the summation: E is the binary exponent with
//               max_a((double) hi_a - (double) lo_a) < 2^E (frexp), s = 32 - E, and s = 0 for a zero extent;
//               u_ia = llrint(((double) x_ia - (double) lo_a) 2^s), an integer in [0, 2^32];
//               U_a = SUM u_ia over the voxel in 64-bit integers (n < 2^31: at most 2^63, no overflow) — integer
//               addition is associative, so an atomicAdd in any order gives the same bits;
//               centroid_a = (float) ((double) lo_a + ((double) U_a / (double) count) 2^-s).
//               Accuracy: u_ia 2^-s differs from x_ia - lo_a by at most 2^-s-1 <= extent 2^-33 (2^(E-1) <= extent),
//               plus the rounding of the fp64 difference (2^-53 relative); so does their mean.  The conversion of U,
//               the division and the addition of lo are three fp64 roundings, far below the final rounding to fp32:
//               |centroid_a - true mean_a| <= extent 2^-33 + one fp32 rounding of the result.
//   rep         the member of the voxel with the smallest d = ((dx^2 + dy^2) + dz^2) to the fp32 centroid, every
//               operation rounded once in fp32, no fma (kg_dist); the lowest index on equal d: the minimum of the key
//               bits(d) << 32 | index (d >= 0 or +inf on finite coordinates, so its bits order as its value).
//   count       the points of the voxel.
//   outputs     owner (n); nvox; centroid, count, first, rep in the first V entries of the segment's rows, NaN / -1
//               behind them.
//   determinism every output is a function of the segment's points, h and o alone: the same bits from run to run and
//               for every batching.  Nothing depends on the layout of the table below.
//
// How voxel.hip computes it.  The three cells, each shifted by 2^20 into 21 bits, form a 63-bit key; a segment owns the
// slots 2 off[c] .. 2 off[c + 1] - 1 of one open-addressing table (capacity twice its points, so a probe sequence
// always ends), the home slot of a key is vx_home, probing is linear.  Per slot: the key (64-bit compare-and-swap on
// VX_EMPTY), first (atomicMin of the index), count and U (atomicAdd).  A point whose slot has first == i is the HEAD of
// its voxel.  Tiles of VX_TILE points, numbered as in fps_math.h; the heads of a tile are counted, the tile counts are
// scanned per segment, and a head's voxel number is the heads before it.  Every number that leaves the table went
// through an integer minimum or an integer sum, which do not depend on the order of arrival.
#pragma once
#include "fps_math.h"

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

#define VX_LANES FPS_LANES
#define VX_PER_LANE FPS_PER_LANE
#define VX_TILE FPS_TILE
#define VX_WAVES (VX_LANES / 64)
#define VX_CELL_BITS 21
#define VX_CELL_BIAS 1048576.0                       // 2^20: cells -2^20 .. 2^20 - 1 become 0 .. 2^21 - 1
#define VX_EMPTY 0xFFFFFFFFFFFFFFFFull               // no key (a key has 63 bits) and no rep candidate
#define VX_NONE 0xFFFFFFFFu                          // no slot, no first
#define VX_NON_FINITE 1u                             // flag bits of a segment
#define VX_RANGE 2u
#define VX_STATUS_NON_FINITE (-1)
#define VX_STATUS_RANGE (-2)

// bounds | table | heads per tile | scan, nvox | voxel rows, owner of the heads | owner, rep candidates | rep
KG_HD int vx_launches(void) { return 7; }

KG_HD long long vx_tile_base(int o, int c) { return fps_tile_base(o, c); }
KG_HD long long vx_tiles(long long total, int S) { return fps_tiles(total, S); }
KG_HD int vx_cloud_tiles(int n) { return n / VX_TILE + (n % VX_TILE != 0); }

KG_HD int vx_good_size(float h) { return h > 0.0f && kg_finite(h); }

// The cell of one coordinate, shifted by 2^20; 0 and *ok = 0 when it does not lie in [0, 2^21).
KG_HD uint32_t vx_cell(float x, float o, float h, int* ok) {
  KG_NO_CONTRACT
  const double d = (double)x - (double)o;
  const double q = d / (double)h;
  const double c = floor(q) + VX_CELL_BIAS;         // exact where it matters: |floor(q)| < 2^52 there
  if (!(c >= 0.0 && c < 2.0 * VX_CELL_BIAS)) {      // (a NaN quotient ends here as well)
    *ok = 0;
    return 0u;
  }
  return (uint32_t)c;
}

// The 63-bit key of a point; *ok = 0 if a cell is out of range.
KG_HD unsigned long long vx_key(const float* p, const float* o, float h, int* ok) {
  *ok = 1;
  const unsigned long long cx = vx_cell(p[0], o[0], h, ok), cy = vx_cell(p[1], o[1], h, ok),
                           cz = vx_cell(p[2], o[2], h, ok);
  return (cx << (2 * VX_CELL_BITS)) | (cy << VX_CELL_BITS) | cz;
}
KG_HD int vx_key_cell(unsigned long long key, int axis) {
  return (int)((key >> ((2 - axis) * VX_CELL_BITS)) & ((1u << VX_CELL_BITS) - 1u)) - (1 << 20);
}

// The home slot of a key in a table of cap slots (1 <= cap < 2^32): the upper half of a multiplicative hash, scaled.
KG_HD uint32_t vx_home(unsigned long long key, uint32_t cap) {
  const unsigned long long h = (key * 0x9E3779B97F4A7C15ull) >> 32;
  return (uint32_t)((h * (unsigned long long)cap) >> 32);
}

// s of the definition from the fp32 bounds.
KG_HD int vx_shift(const float* lo, const float* hi) {
  KG_NO_CONTRACT
  double ext = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double e = (double)hi[a] - (double)lo[a];
    if (e > ext) ext = e;
  }
  if (!(ext > 0.0)) return 0;
  int E;
  frexp(ext, &E);
  return 32 - E;
}

KG_HD unsigned long long vx_quantise(float x, float lo, int s) {
  KG_NO_CONTRACT
  const double d = (double)x - (double)lo;
  return (unsigned long long)llrint(ldexp(d, s));
}

KG_HD float vx_centroid(float lo, unsigned long long U, uint32_t count, int s) {
  KG_NO_CONTRACT
  const double mean = (double)U / (double)count;
  const double c = (double)lo + ldexp(mean, -s);
  return (float)c;
}

KG_HD unsigned long long vx_rep_key(float d, uint32_t i) {
  return ((unsigned long long)kg_bits(d) << 32) | (unsigned long long)i;
}
KG_HD uint32_t vx_rep_index(unsigned long long key) { return (uint32_t)key; }

// The status of a segment from its flag bits and its voxel size: -1, -2 or 0.
KG_HD int vx_status(uint32_t flag, float h) {
  if (flag & VX_NON_FINITE) return VX_STATUS_NON_FINITE;
  if ((flag & VX_RANGE) || !vx_good_size(h)) return VX_STATUS_RANGE;
  return 0;
}

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
