// Test-only host restatement of the farthest-point sampling of parsenet_codebase_amd/csrc/fps.hip: the launches of its
// schedule run serially, in the kernel's own order, on the SAME per-point step, keys and tile numbering the kernels
// compile (csrc/fps_math.h): init (tile table, D = +inf, non-finite flags, start slots), then per step every tile's
// candidate and the maximum over the tiles' keys on slot (c, t + 1), then the decoding of the slots.  With order = 1 the
// tiles of a launch are visited in descending order: an integer maximum must not depend on the order of arrival.
// tests/test_fps_abi.py holds every output against an independent numpy restatement of the definition.  Not part of
// the product.
//
// As a shared object it exports fph_fps and the constants below.  As a program (it has a main) it runs built-in
// clouds — ties on a lattice over several tiles, duplicates, a short, an empty and a non-finite cloud in one batch —
// against a plain loop over the definition and in both tile orders, and returns 1 on any difference; with a file name
// as its first argument it reads  n m start  and n lines  x y z  and prints the m samples.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../parsenet_codebase_amd/csrc/fps_math.h"

extern "C" {

int fph_tile(void) { return FPS_TILE; }
int fph_launches(int m) { return fps_launches(m); }

// The whole batch under the schedule.  P (total,3), off (S+1), start (S) or null; sample, radius (S,m), owner, dist
// (total).  Returns the number of launches it ran, -1 on a bad argument.
int fph_fps(const float* P, const int32_t* off, int S, int total, int m, const int32_t* start, int order,
            int32_t* sample, float* radius, int32_t* owner, float* dist) {
  if (m < 1 || S < 0 || total < 0) return -1;
  const long long tiles = fps_tiles(total, S), ns = fps_slots(m);
  std::vector<unsigned long long> slot((size_t)(ns * S), 0ull);                      // the memset
  std::vector<float> D((size_t)total, 0.0f);
  std::vector<int> tile_seg((size_t)tiles, -1), tile_first((size_t)tiles, 0);
  int launches = 0;
  // init
  for (long long b = 0; b < tiles; ++b) {
    int lo = 0, hi = S;
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      if (fps_tile_base(off[mid], mid) <= b) lo = mid; else hi = mid;
    }
    const int c = lo, o0 = off[c], o1 = off[c + 1], n = o1 - o0;
    const long long first = (b - fps_tile_base(o0, c)) * FPS_TILE;
    if (!(fps_valid_segment(o0, o1, total) && first >= 0 && first < n)) continue;
    tile_seg[b] = c;
    tile_first[b] = (int)first;
    for (int i = (int)first; i < n && i < first + FPS_TILE; ++i) {
      const size_t g = (size_t)o0 + i;
      if (!(kg_finite(P[3 * g]) && kg_finite(P[3 * g + 1]) && kg_finite(P[3 * g + 2]))) slot[ns * c + fps_flag_slot(m)] = 1;
      D[g] = kg_inf();
      owner[g] = -1;
    }
    if (first == 0) slot[ns * c] = fps_key(kg_inf(), (uint32_t)fps_clamp_start(start ? start[c] : 0, n));
  }
  ++launches;
  // the m steps
  for (int t = 0; t < m; ++t, ++launches)
    for (long long bb = 0; bb < tiles; ++bb) {
      const long long b = order ? tiles - 1 - bb : bb;
      const int c = tile_seg[b];
      if (c < 0) continue;
      const int o0 = off[c], n = off[c + 1] - o0;
      if (t >= (m < n ? m : n) || slot[ns * c + fps_flag_slot(m)] != 0) continue;
      const uint32_t s = fps_key_index(slot[ns * c + t]);
      if (s >= (uint32_t)n) return -2;
      const float* q = P + 3 * ((size_t)o0 + s);
      unsigned long long best = FPS_NO_KEY;
      for (int i = tile_first[b]; i < n && i < tile_first[b] + FPS_TILE; ++i) {
        const size_t g = (size_t)o0 + i;
        int owned;
        const unsigned long long key = fps_point_step(P + 3 * g, q, (uint32_t)i, s, &D[g], &owned);
        if (owned) owner[g] = t;
        if (key > best) best = key;
      }
      if (best > slot[ns * c + t + 1]) slot[ns * c + t + 1] = best;
    }
  // outputs
  for (int c = 0; c < S; ++c) {
    const int o0 = off[c], o1 = off[c + 1];
    const int n = fps_valid_segment(o0, o1, total) ? o1 - o0 : 0;
    const bool bad = slot[ns * c + fps_flag_slot(m)] != 0;
    for (int t = 0; t < m; ++t) {
      const bool have = t < n && !bad;
      const unsigned long long key = slot[ns * c + t];
      sample[(size_t)c * m + t] = have ? (int32_t)fps_key_index(key) : -1;
      radius[(size_t)c * m + t] = have ? fps_key_dist(key) : NAN;
    }
  }
  for (long long b = 0; b < tiles; ++b) {
    const int c = tile_seg[b];
    if (c < 0) continue;
    const int o0 = off[c], n = off[c + 1] - o0;
    const bool bad = slot[ns * c + fps_flag_slot(m)] != 0;
    for (int i = tile_first[b]; i < n && i < tile_first[b] + FPS_TILE; ++i) {
      const size_t g = (size_t)o0 + i;
      dist[g] = bad ? NAN : fps_final_dist(D[g]);
      if (bad) owner[g] = -1;
    }
  }
  return launches + 1;
}

}  // extern "C"

// The definition, as a plain loop over one cloud.
static void plain(const float* P, int n, int m, int start, int32_t* sample, float* radius, int32_t* owner, float* dist) {
  bool bad = false;
  for (int i = 0; i < 3 * n; ++i) bad = bad || !kg_finite(P[i]);
  for (int t = 0; t < m; ++t) sample[t] = -1, radius[t] = NAN;
  for (int i = 0; i < n; ++i) owner[i] = -1, dist[i] = bad ? NAN : kg_inf();
  if (bad || n == 0) return;
  std::vector<char> chosen(n, 0);
  int s = fps_clamp_start(start, n);
  for (int t = 0; t < (m < n ? m : n); ++t) {
    sample[t] = s;
    radius[t] = dist[s];
    chosen[s] = 1, dist[s] = 0.0f, owner[s] = t;
    int next = -1;
    for (int i = 0; i < n; ++i) {
      if (chosen[i]) continue;
      const float nd = kg_dist(P[3 * i], P[3 * i + 1], P[3 * i + 2], P[3 * s], P[3 * s + 1], P[3 * s + 2]);
      if (nd < dist[i]) dist[i] = nd, owner[i] = t;
      if (next < 0 || dist[i] > dist[next]) next = i;
    }
    s = next;
  }
}

static bool same(float a, float b) { return kg_bits(a) == kg_bits(b) || (a != a && b != b); }

static int self_check(void) {
  // five clouds: a 13^3 dyadic lattice (2 197 points, three tiles, all ties), 600 copies of one point among 400 others,
  // three points (shorter than m), an empty cloud, a cloud with one NaN
  std::vector<float> P;
  std::vector<int32_t> off(1, 0);
  for (int x = 0; x < 13; ++x)
    for (int y = 0; y < 13; ++y)
      for (int z = 0; z < 13; ++z) P.push_back(0.25f * x), P.push_back(0.25f * y), P.push_back(0.25f * z);
  off.push_back((int32_t)(P.size() / 3));
  unsigned r = 12345u;
  for (int i = 0; i < 1000; ++i)
    for (int a = 0; a < 3; ++a) {
      r = r * 1664525u + 1013904223u;
      P.push_back(i % 5 < 3 ? 0.125f * (a + 1) : (float)(r >> 8) / (float)(1 << 24) - 0.5f);
    }
  off.push_back((int32_t)(P.size() / 3));
  for (int i = 0; i < 9; ++i) P.push_back(0.5f * i);
  off.push_back((int32_t)(P.size() / 3));
  off.push_back((int32_t)(P.size() / 3));
  for (int i = 0; i < 30; ++i) P.push_back(i == 7 ? NAN : 0.1f * i);
  off.push_back((int32_t)(P.size() / 3));
  const int S = (int)off.size() - 1, total = off[S], m = 40;
  const int32_t start[5] = {5, -3, 99, 0, 2};
  std::vector<int32_t> sa((size_t)S * m), sb(sa), sc(sa), oa(total), ob(total), oc(total);
  std::vector<float> ra((size_t)S * m), rb(ra), rc(ra), da(total), db(total), dc(total);
  if (fph_fps(P.data(), off.data(), S, total, m, start, 0, sa.data(), ra.data(), oa.data(), da.data()) != m + 2) return 1;
  if (fph_fps(P.data(), off.data(), S, total, m, start, 1, sb.data(), rb.data(), ob.data(), db.data()) != m + 2) return 1;
  for (int c = 0; c < S; ++c)
    plain(P.data() + 3 * (size_t)off[c], off[c + 1] - off[c], m, start[c], sc.data() + (size_t)c * m,
          rc.data() + (size_t)c * m, oc.data() + off[c], dc.data() + off[c]);
  int differ = 0;
  for (size_t e = 0; e < sa.size(); ++e)
    differ += sa[e] != sc[e] || sb[e] != sc[e] || !same(ra[e], rc[e]) || !same(rb[e], rc[e]);
  for (int g = 0; g < total; ++g)
    differ += oa[g] != oc[g] || ob[g] != oc[g] || !same(da[g], dc[g]) || !same(db[g], dc[g]);
  printf("fps_host: %d clouds, %d points, m = %d, %d launches: %d differences from the plain loop\n", S, total, m,
         fps_launches(m), differ);
  return differ != 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return self_check();
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int n, m, start;
  if (fscanf(f, "%d %d %d", &n, &m, &start) != 3 || n < 0 || m < 1) return 2;
  std::vector<float> P((size_t)3 * n);
  for (size_t t = 0; t < P.size(); ++t)
    if (fscanf(f, "%f", &P[t]) != 1) return 2;
  fclose(f);
  const int32_t off[2] = {0, n};
  std::vector<int32_t> sample(m), owner(n);
  std::vector<float> radius(m), dist(n);
  if (fph_fps(P.data(), off, 1, n, m, &start, 0, sample.data(), radius.data(), owner.data(), dist.data()) < 0) return 1;
  for (int t = 0; t < m; ++t) printf(t ? " %d" : "%d", sample[t]);
  printf("\n");
  return 0;
}
