// Definition of the statistical outlier removal of outlier.hip: open3d's remove_statistical_outlier statistic (as
// oracle/ref_fitting.remove_outliers restates it) on the fp32 neighbour distances the raw-cloud searches deliver, as an
// exact, bit-reproducible function of the cloud alone, on clouds of any size.  Plain C++ behind KG_HD so that the same
// source is compiled into the gfx950 kernels and, by the test suite only (tests/native/outlier_host.cpp), into a serial
// restatement of the whole schedule.  Contraction is switched off inside every function here.
//
// Everything is per segment (one cloud of a ragged batch) of n points, indices LOCAL to it.  Given dist (n,k) fp32 —
// the distances of knn3_ragged / knn3_grid: nearest first, the point itself first, padded with the point itself when
// n < k —, 1 <= k <= 64 and std_ratio >= 0 (a double):
//
//   count       k_c = min(k, n).
//   statistic   a_i = (((0 + (double) dist[i][0]) + (double) dist[i][1]) + ... ) / (double) k_c over j < k_c, ascending
//               j, every operation rounded once in fp64: the mean distance to the k_c nearest, the point itself included.
//   validity    valid_i = a_i > 0.  A NaN is not valid, and neither is a point whose k_c nearest coincide with it.
//   term        t(x, valid, a) = x if valid, NaN if a is a NaN, else 0.  A NaN statistic — the searches give NaN rows to
//               every point of a cloud that holds a non-finite coordinate — therefore poisons the sums below, whatever
//               their order, and the cloud ends with mean, std and thr NaN, every keep 0 and kept = 0.
//   mean        mean = SUM_i t(a_i) / (double) n                                            (0 / 0 = NaN when n = 0)
//   poison      the terms are non-negative or NaN, so mean is a NaN exactly when some a_i is (or n = 0); then EVERY a_i
//               of the cloud is replaced by NaN.  The brute-force search gives NaN rows only to the non-finite points
//               themselves (their distance to themselves is inf - inf or NaN), the grid search to the whole cloud: with
//               this rule the outputs do not tell the two apart.
//   std         std = sqrt(SUM_i t((a_i - mean) * (a_i - mean)) / (double) (n - 1)), 0 when n <= 1.  Two passes: mean
//               is known before the deviations are formed.  The divisors are n and n - 1, not the count of valid points.
//   threshold   thr = mean + std_ratio * std (two roundings);  keep_i = valid_i && a_i < thr, strict.
//   compaction  index: the LOCAL indices of the kept points in ascending order in the first kept entries of the
//               cloud's rows, -1 behind them.
//
// SUM is ONE fixed tree that depends on the cloud alone — not on the batch, the launch or the run:
//   tile        OL_TILE = 1 024 consecutive points counted from the cloud's first point; an absent point enters as 0.0,
//               whose addition is exact.  With v[0 .. 1023] the terms of a tile:
//   lane        lane l of 256:  s_l = ((v[l] + v[l + 256]) + v[l + 512]) + v[l + 768]                    (ol_lane_sum)
//   wave        each run of 64 lanes: s_l = s_l + s_(l ^ h) for h = 32, 16, 8, 4, 2, 1.  Addition is commutative, so
//               after every step the two partners hold the same bits, and in the end all 64 lanes do     (ol_butterfly)
//   tile sum    ((w0 + w1) + w2) + w3 of the four waves                                                  (ol_wave_sum)
//   cloud       the tile sums one after another in ascending tile order, starting from 0.0.
// In numpy: v.reshape(tiles, 4, 256) -> ((v[:,0] + v[:,1]) + v[:,2]) + v[:,3] -> reshape(tiles, 4, 64) -> six times
// s = s + s[..., arange(64) ^ h] -> w = s[..., 0] -> ((w[:,0] + w[:,1]) + w[:,2]) + w[:,3] -> a loop over the tiles.
//
// Accuracy.  Every term passes through 3 additions in its lane, 6 in the butterfly, 3 over the waves and at most
// `tiles` over the tiles: with the division at the end, at most 13 + tiles roundings.  The terms are non-negative, so
// nothing cancels, and the first-order bound of recursive summation gives |SUM - exact| <= (depth) u |exact| with
// u = 2^-53; (13 + tiles) 2^-52 is that bound with a factor 2 for the higher-order terms (depth u << 1 up to 2^31
// points: tiles <= 2^21).  tests/test_outlier_abi.py holds mean and the deviation sum to it against math.fsum.
//
// How outlier.hip computes it.  A tile is one workgroup of OL_LANES lanes, OL_PER_LANE points per lane, lane-interleaved
// (point first + p * 256 + l is v[l + 256 p]).  Tiles are numbered without a prefix sum as in fps_math.h: segment c owns
// ol_tile_base(off[c], c) .. + ol_cloud_tiles(n) - 1 out of ol_tiles(total, S) numbers — a host integer.  The order of
// the kept points inside a tile comes from ballots: point (p, wave, lane) has p * 4 + wave runs of 64 in front of it.
#pragma once
#include "fps_math.h"

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

#define OL_LANES FPS_LANES
#define OL_PER_LANE FPS_PER_LANE
#define OL_TILE FPS_TILE
#define OL_WAVE 64
#define OL_WAVES (OL_LANES / OL_WAVE)
#define OL_MIN_K 1
#define OL_MAX_K 64

// statistic + tile sums | mean | deviation sums | std, thr | mask + tile counts | kept, index
KG_HD int ol_launches(void) { return 6; }

KG_HD long long ol_tile_base(int o, int c) { return fps_tile_base(o, c); }
KG_HD long long ol_tiles(long long total, int S) { return fps_tiles(total, S); }
KG_HD int ol_cloud_tiles(int n) { return n / OL_TILE + (n % OL_TILE != 0); }

KG_HD double ol_nan(void) {
  const unsigned long long u = 0x7ff8000000000000ull;
  double d;
#if defined(__HIP_DEVICE_COMPILE__)
  d = __longlong_as_double((long long)u);
#else
  memcpy(&d, &u, 8);
#endif
  return d;
}

KG_HD int ol_count(int k, int n) { return k < n ? k : n; }

// The running sum of a row continued over x[0 .. count - 1], and the statistic of a finished sum.
KG_HD double ol_accumulate(double s, const float* x, int count) {
  KG_NO_CONTRACT
  for (int j = 0; j < count; ++j) s = s + (double)x[j];
  return s;
}
KG_HD double ol_average(double s, int kc) {
  KG_NO_CONTRACT
  return s / (double)kc;
}
KG_HD double ol_point(const float* row, int kc) { return ol_average(ol_accumulate(0.0, row, kc), kc); }

KG_HD int ol_valid(double a) { return a > 0.0; }

// What a point adds to a SUM: x if it is valid, NaN if its statistic is a NaN, else 0.
KG_HD double ol_term(double x, double a) { return ol_valid(a) ? x : (a != a ? ol_nan() : 0.0); }
KG_HD double ol_mean_term(double a) { return ol_term(a, a); }
KG_HD int ol_poisoned(double mean) { return mean != mean; }
KG_HD double ol_dev_term(double a, double mean) {
  KG_NO_CONTRACT
  const double d = a - mean;
  return ol_term(d * d, a);
}

KG_HD double ol_add(double a, double b) {
  KG_NO_CONTRACT
  return a + b;
}
KG_HD double ol_lane_sum(double v0, double v1, double v2, double v3) { return ol_add(ol_add(ol_add(v0, v1), v2), v3); }
KG_HD double ol_wave_sum(double w0, double w1, double w2, double w3) { return ol_add(ol_add(ol_add(w0, w1), w2), w3); }

// The butterfly over the OL_WAVE values of s, as the shuffles of the kernel run it: afterwards every entry holds the sum.
KG_HD void ol_butterfly(double* s) {
  double t[OL_WAVE];
  for (int h = OL_WAVE / 2; h > 0; h >>= 1) {
    for (int l = 0; l < OL_WAVE; ++l) t[l] = ol_add(s[l], s[l ^ h]);
    for (int l = 0; l < OL_WAVE; ++l) s[l] = t[l];
  }
}

KG_HD double ol_mean(double sum, int n) {
  KG_NO_CONTRACT
  return sum / (double)n;
}
KG_HD double ol_std(double sum, int n) {
  KG_NO_CONTRACT
  return n <= 1 ? 0.0 : sqrt(sum / (double)(n - 1));
}
KG_HD double ol_threshold(double mean, double std, double std_ratio) {
  KG_NO_CONTRACT
  const double m = std_ratio * std;
  return mean + m;
}
KG_HD int ol_keep(double a, double thr) { return ol_valid(a) && a < thr; }

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
