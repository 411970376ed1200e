// Definition of the two k-nearest-sample lifting rules of knn_lift.hip: what a point takes from the k reference points
// (samples) that pn_knn3_query_f32 found for it.  Plain C++ behind KG_HD so that the same source is compiled into the
// gfx950 kernels and, by the test suite only (tests/native/knn3_query_host.cpp), into a serial restatement.
// Contraction is switched off inside every function here.
//
// Everything is per query row: idx[0 .. k-1] int32 LOCAL to the reference segment of n points, nearest first, -1 behind
// the neighbours that exist; dist[0 .. k-1] fp32.  An entry is VALID when 0 <= idx < n.
//
//   interpolate  inverse-distance weights, PointNet++'s three_interpolate with its 1 / (d + 1e-8):
//                  w_j   = 1.0 / ((double) dist_j + 1e-8)
//                  out_c = (float) ((SUM_j w_j * v[idx_j][c]) / (SUM_j w_j))
//                over the valid entries in ascending rank j, both sums started at 0.0, every operation rounded once in
//                fp64, the product rounded before it is added.  A row with no valid entry, or with a NaN anywhere in
//                dist, is NaN in every channel.  A neighbour at dist = +inf (a squared distance that overflowed fp32)
//                has weight 0; if every weight is 0 the row is 0 / 0 = NaN.  A coincident sample (dist = 0) has
//                weight 1e8 and dominates without a special case.
//   vote         the label that occurs most often among the valid entries with label >= 0; on equal counts the label
//                whose first occurrence has the lowest rank (the one with the nearer member); none: -1.  Integers only.
#pragma once
#include "knn3_grid_math.h"

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

#define KL_MIN_K 1
#define KL_MAX_K 64

KG_HD float kl_nan(void) { return kg_float(0x7fc00000u); }

KG_HD int kl_valid(int j, int n) { return (unsigned)j < (unsigned)n; }

KG_HD double kl_weight(float dist) {
  KG_NO_CONTRACT
  return 1.0 / ((double)dist + 1e-8);
}

// Is the row NaN whatever its values: no valid entry, or a NaN distance?
KG_HD int kl_row_is_nan(const int32_t* idx, const float* dist, int k, int n) {
  int valid = 0;
  for (int j = 0; j < k; ++j) {
    if (dist[j] != dist[j]) return 1;
    valid |= kl_valid(idx[j], n);
  }
  return !valid;
}

// Channel c of one row: values (n,C) are the rows of the reference segment.
KG_HD float kl_interpolate(const float* values, long long C, long long c, const int32_t* idx, const float* dist, int k,
                           int n) {
  KG_NO_CONTRACT
  if (kl_row_is_nan(idx, dist, k, n)) return kl_nan();
  double num = 0.0, den = 0.0;
  for (int j = 0; j < k; ++j) {
    if (!kl_valid(idx[j], n)) continue;
    const double w = kl_weight(dist[j]);
    const double t = w * (double)values[(long long)idx[j] * C + c];
    num = num + t;
    den = den + w;
  }
  return (float)(num / den);
}

// The label of entry j, -1 when the entry is not valid or its label is negative.
KG_HD int kl_label(const int32_t* labels, const int32_t* idx, int j, int n) {
  if (!kl_valid(idx[j], n)) return -1;
  const int l = labels[idx[j]];
  return l < 0 ? -1 : l;
}

// labels (n) are those of the reference segment.  No array of k labels is kept: a label is read again where it is
// needed (k * k reads of a row that sits in the cache), so that the kernel needs no scratch.
KG_HD int kl_vote(const int32_t* labels, const int32_t* idx, int k, int n) {
  int best = -1, most = 0;
  for (int j = 0; j < k; ++j) {
    const int l = kl_label(labels, idx, j, n);
    if (l < 0) continue;
    int count = 0;
    for (int i = 0; i < k; ++i) count += kl_label(labels, idx, i, n) == l;
    if (count > most) {      // strict: an equal count later in rank order does not replace the nearer label
      most = count;
      best = l;
    }
  }
  return best;
}

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
