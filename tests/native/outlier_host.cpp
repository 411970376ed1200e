// Test-only host restatement of the statistical outlier removal of parsenet_codebase_amd/csrc/outlier.hip: the six
// launches of its schedule run serially, in the kernel's own order, on the SAME per-point statistic, terms, summation
// tree and tile numbering the kernels compile (csrc/outlier_math.h): the statistic and the tile sums, the mean, the
// deviation sums, std and thr, the mask and the tile counts, kept and index.  With order = 1 the tiles of a launch are
// visited in descending order: nothing may depend on the order in which workgroups run.  tests/test_outlier_abi.py
// holds every output against an independent numpy restatement of the definition.  Not part of the product.
//
// As a shared object it exports olh_stat and the constants below.  As a program (it has a main) it runs a built-in
// ragged batch — three tiles with strays, coincident points, a short, an empty and a NaN cloud — in both tile orders
// against a plain loop over the definition whose sums are long double (compared within the bound of the header, the
// mask wherever the statistic is not within that bound of the threshold), and returns 1 on any difference.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../parsenet_codebase_amd/csrc/outlier_math.h"

// The sum of one tile's terms v[0 .. OL_TILE - 1] by the tree, as a workgroup forms it.
static double tile_sum(const double* v) {
  double w[OL_WAVES];
  for (int wave = 0; wave < OL_WAVES; ++wave) {
    double s[OL_WAVE];
    for (int lane = 0; lane < OL_WAVE; ++lane) {
      const int l = wave * OL_WAVE + lane;
      s[lane] = ol_lane_sum(v[l], v[l + OL_LANES], v[l + 2 * OL_LANES], v[l + 3 * OL_LANES]);
    }
    ol_butterfly(s);
    w[wave] = s[0];
  }
  return ol_wave_sum(w[0], w[1], w[2], w[3]);
}

extern "C" {

int olh_tile(void) { return OL_TILE; }
int olh_launches(void) { return ol_launches(); }

// The whole batch under the schedule.  dist (total,k), off (S+1); avg (total), stats (S,3), keep (total), kept (S),
// index (total) or null, sums (S,2) or null: the two SUMs of every valid segment before their divisions.  Returns the
// number of launches it ran, -1 on a bad argument.
int olh_stat(const float* dist, const int32_t* off, int S, int total, int k, double std_ratio, int order, double* avg,
             double* stats, uint8_t* keep, int32_t* kept, int32_t* index, double* sums) {
  if (k < OL_MIN_K || k > OL_MAX_K || S < 0 || total < 0 || !(std_ratio >= 0.0)) return -1;
  if (S == 0 || total == 0) return 0;                                    // as the library: nothing is launched
  const long long tiles = ol_tiles(total, S);
  std::vector<double> part((size_t)tiles, -1.0);
  std::vector<int> count((size_t)tiles, -1), tile_seg((size_t)tiles, -1), tile_first((size_t)tiles, 0);
  std::vector<double> v(OL_TILE);
  int launches = 0;
  const auto visit = [&](long long bb) { return order ? tiles - 1 - bb : bb; };
  // 1: statistic and tile sums; rows that no valid segment holds
  for (int g = 0; g < total; ++g) {
    const int s = rg_row_segment(off, S, g);
    if (S > 0 && rg_segment_holds(off[s], off[s + 1], total, g)) continue;
    avg[g] = ol_nan(), keep[g] = 0;
    if (index) index[g] = -1;
  }
  for (long long bb = 0; bb < tiles; ++bb) {
    const long long b = visit(bb);
    const int c = rg_segment(S, b, [off](int s) { return ol_tile_base(off[s], s); });
    const int o0 = off[c], o1 = off[c + 1], n = o1 - o0;
    const long long first = (b - ol_tile_base(o0, c)) * OL_TILE;
    if (!(rg_valid_segment(o0, o1, total) && first >= 0 && first < n)) continue;
    tile_seg[b] = c, tile_first[b] = (int)first;
    const int kc = ol_count(k, n);
    for (int e = 0; e < OL_TILE; ++e) {
      const int i = (int)first + e;
      v[e] = 0.0;
      if (i >= n) continue;
      const size_t g = (size_t)o0 + i;
      avg[g] = ol_point(dist + g * (size_t)k, kc);
      v[e] = ol_mean_term(avg[g]);
    }
    part[b] = tile_sum(v.data());
  }
  ++launches;
  for (int stage = 0; stage < 2; ++stage) {
    // 2 and 4: the tile sums of a cloud in ascending order
    for (int c = 0; c < S; ++c) {
      const int o0 = off[c], o1 = off[c + 1];
      if (!rg_valid_segment(o0, o1, total)) {
        if (stage == 0) stats[3 * c] = stats[3 * c + 1] = stats[3 * c + 2] = ol_nan(), kept[c] = 0;
        continue;
      }
      const int n = o1 - o0, nt = ol_cloud_tiles(n);
      double s = 0.0;
      for (int t = 0; t < nt; ++t) s = ol_add(s, part[ol_tile_base(o0, c) + t]);
      if (sums) sums[2 * c + stage] = s;
      if (stage == 0) {
        stats[3 * c] = ol_mean(s, n), kept[c] = 0;
      } else {
        stats[3 * c + 1] = ol_std(s, n);
        stats[3 * c + 2] = ol_threshold(stats[3 * c], stats[3 * c + 1], std_ratio);
      }
    }
    ++launches;
    // 3: deviation sums; 5: mask and tile counts
    for (long long bb = 0; bb < tiles; ++bb) {
      const long long b = visit(bb);
      const int c = tile_seg[b];
      if (c < 0) continue;
      const int o0 = off[c], n = off[c + 1] - o0, first = tile_first[b];
      int cnt = 0;
      for (int e = 0; e < OL_TILE; ++e) {
        const int i = first + e;
        v[e] = 0.0;
        if (i >= n) continue;
        const size_t g = (size_t)o0 + i;
        if (stage == 0) {
          if (ol_poisoned(stats[3 * c])) avg[g] = stats[3 * c];
          v[e] = ol_dev_term(avg[g], stats[3 * c]);
        } else {
          keep[g] = (uint8_t)ol_keep(avg[g], stats[3 * c + 2]);
          cnt += keep[g];
        }
      }
      if (stage == 0) part[b] = tile_sum(v.data()); else count[b] = cnt;
    }
    ++launches;
  }
  // 6: kept and index
  for (long long bb = 0; bb < tiles; ++bb) {
    const long long b = visit(bb);
    const int c = tile_seg[b];
    if (c < 0) continue;
    const int o0 = off[c], n = off[c + 1] - o0, first = tile_first[b], nt = ol_cloud_tiles(n), mine = first / OL_TILE;
    unsigned before = 0, all = 0;
    for (int t = 0; t < nt; ++t) {
      const unsigned q = (unsigned)count[ol_tile_base(o0, c) + t];
      all += q;
      if (t < mine) before += q;
    }
    if (first == 0) kept[c] = (int32_t)all;
    if (!index) continue;
    // the kernel's index order inside a tile: p, then wave, then lane — which is ascending i
    unsigned pos = before;
    for (int e = 0; e < OL_TILE; ++e) {
      const int i = first + e;
      if (i >= n) break;
      if (keep[(size_t)o0 + i]) {
        if (pos >= (unsigned)n) return -2;
        index[(size_t)o0 + pos++] = i;
      }
    }
    for (int e = 0; e < OL_TILE; ++e) {
      const int i = first + e;
      if (i < n && (unsigned)i >= all) index[(size_t)o0 + i] = -1;
    }
  }
  return launches + 1;
}

}  // extern "C"

// The definition as a plain loop over one cloud, the two sums in long double: (mean, std, thr) and the statistic.
static void plain(const float* dist, int n, int k, double ratio, std::vector<double>* a, double* stats) {
  const int kc = ol_count(k, n);
  a->assign((size_t)n, 0.0);
  long double sum = 0.0L, dev = 0.0L;
  for (int i = 0; i < n; ++i) {
    double s = 0.0;
    for (int j = 0; j < kc; ++j) s += (double)dist[(size_t)i * k + j];
    (*a)[i] = s / (double)kc;
    if ((*a)[i] > 0.0) sum += (*a)[i]; else if ((*a)[i] != (*a)[i]) sum += (long double)NAN;
  }
  const long double mean = sum / (long double)n;
  if (mean != mean) a->assign((size_t)n, NAN);
  for (int i = 0; i < n; ++i) {
    const long double d = (long double)(*a)[i] - mean;
    if ((*a)[i] > 0.0) dev += d * d; else if ((*a)[i] != (*a)[i]) dev += (long double)NAN;
  }
  stats[0] = (double)mean;
  stats[1] = n <= 1 ? 0.0 : (double)sqrtl(dev / (long double)(n - 1));
  stats[2] = stats[0] + ratio * stats[1];
}

static bool close_to(double got, double want, double rel) {
  if (got != got || want != want) return got != got && want != want;
  return fabs(got - want) <= rel * fabs(want);
}

static int self_check(void) {
  const int k = 20;
  const double ratio = 1.5;
  // the clouds: 2 500 points with distances that grow slowly and 12 strays, 40 coincident points, 3 points, none, 30 NaN
  const int sizes[5] = {2500, 40, 3, 0, 30};
  std::vector<int32_t> off(1, 0);
  for (int c = 0; c < 5; ++c) off.push_back(off.back() + sizes[c]);
  const int S = 5, total = off[S];
  std::vector<float> dist((size_t)total * k, 0.0f);
  unsigned r = 2463534242u;
  for (int c = 0; c < S; ++c)
    for (int i = 0; i < sizes[c]; ++i) {
      float* row = dist.data() + ((size_t)off[c] + i) * k;
      float d = 0.0f;
      for (int j = 1; j < k; ++j) {
        r = r * 1664525u + 1013904223u;
        if (c == 0) d += (i % 211 == 7 ? 0.5f : 0.01f) * (1.0f + (float)(r >> 8) / (float)(1 << 24));
        if (c == 2) d = j < 3 ? 0.25f * j : 0.0f;              // n < k: the pad is the point itself
        row[j] = c == 4 ? NAN : (c == 1 ? 0.0f : d);
      }
      if (c == 4) row[0] = NAN;
    }
  std::vector<double> avg[2] = {std::vector<double>(total), std::vector<double>(total)};
  std::vector<double> stats[2] = {std::vector<double>(3 * S), std::vector<double>(3 * S)};
  std::vector<uint8_t> keep[2] = {std::vector<uint8_t>(total), std::vector<uint8_t>(total)};
  std::vector<int32_t> kept[2] = {std::vector<int32_t>(S), std::vector<int32_t>(S)};
  std::vector<int32_t> index[2] = {std::vector<int32_t>(total), std::vector<int32_t>(total)};
  for (int order = 0; order < 2; ++order)
    if (olh_stat(dist.data(), off.data(), S, total, k, ratio, order, avg[order].data(), stats[order].data(),
                 keep[order].data(), kept[order].data(), index[order].data(), nullptr) != ol_launches())
      return 1;
  int differ = 0;
  for (int g = 0; g < total; ++g)
    differ += memcmp(&avg[0][g], &avg[1][g], 8) != 0 || keep[0][g] != keep[1][g] || index[0][g] != index[1][g];
  for (int e = 0; e < 3 * S; ++e) differ += memcmp(&stats[0][e], &stats[1][e], 8) != 0;
  for (int c = 0; c < S; ++c) {
    const int n = sizes[c];
    differ += kept[0][c] != kept[1][c];
    std::vector<double> a;
    double want[3];
    plain(dist.data() + (size_t)off[c] * k, n, k, ratio, &a, want);
    const double rel = (13.0 + ol_cloud_tiles(n)) * ldexp(1.0, -52);
    differ += !close_to(stats[0][3 * c], want[0], rel) || !close_to(stats[0][3 * c + 1], want[1], 4 * rel) ||
              !close_to(stats[0][3 * c + 2], want[2], 4 * rel);
    int pos = 0;
    for (int i = 0; i < n; ++i) {
      const size_t g = (size_t)off[c] + i;
      differ += memcmp(&avg[0][g], &a[i], 8) != 0;
      const int near = fabs(a[i] - want[2]) <= 8 * rel * fabs(want[2]);
      if (!near) differ += keep[0][g] != (a[i] > 0.0 && a[i] < want[2]);
      if (keep[0][g]) differ += index[0][(size_t)off[c] + pos++] != i;
    }
    differ += pos != kept[0][c];
    for (int i = pos; i < n; ++i) differ += index[0][(size_t)off[c] + i] != -1;
  }
  differ += !(kept[0][0] > 2400 && kept[0][0] <= 2488) || kept[0][1] != 0 || kept[0][3] != 0 || kept[0][4] != 0;
  printf("outlier_host: %d clouds, %d points, k = %d, %d launches, kept %d %d %d %d %d: %d differences from the plain "
         "loop\n", S, total, k, ol_launches(), kept[0][0], kept[0][1], kept[0][2], kept[0][3], kept[0][4], differ);
  return differ != 0;
}

int main(void) { return self_check(); }
