// Test-only host restatement of the voxel-grid downsampling of parsenet_codebase_amd/csrc/voxel.hip: the launches of
// its schedule run serially, in the kernel's own order, on the SAME cell key, home slot, quantisation, centroid and rep
// key the kernels compile (csrc/voxel_math.h): bounds and flags, the open-addressing table (key, first, count, U per
// slot), the heads per tile, the scan of the tile counts, the voxel rows, owner and the rep candidates, the decoding.
// cap_mul sets the capacity of a segment's table to cap_mul * n slots (the kernels use 2), and with order = 1 the
// points of a launch are visited in descending order: no output may depend on the layout of the table or on the order
// of arrival.  tests/test_voxel_abi.py holds every output against an independent numpy restatement of the definition.
// Not part of the product.
//
// As a shared object it exports vxh_voxel and the constants below.  As a program (it has a main) it runs built-in
// clouds — a lattice on the faces of its cells over several tiles, duplicates, a short, an empty, a non-finite and an
// out-of-range cloud in one batch — against a plain loop over the definition, with two capacities and both orders, and
// returns 1 on any difference; with a file name as its first argument it reads  n h  and n lines  x y z  and prints
// nvox and the n owners.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <vector>

#include "../../parsenet_codebase_amd/csrc/voxel_math.h"

extern "C" {

int vxh_tile(void) { return VX_TILE; }
int vxh_launches(void) { return vx_launches(); }

// The whole batch under the schedule.  P (total,3), off (S+1), voxel (S), origin (S,3) or null; owner (total), nvox (S),
// centroid (total,3), count, first, rep (total).  Rows that no valid segment holds are not written.  Returns the number
// of launches it ran, -1 on a bad argument, -2 if a probe sequence did not end.
int vxh_voxel(const float* P, const int32_t* off, int S, int total, const float* voxel, const float* origin,
              int cap_mul, int order, int32_t* owner, int32_t* nvox, float* centroid, int32_t* count, int32_t* first,
              int32_t* rep) {
  if (S < 0 || total < 0 || cap_mul < 2) return -1;
  const long long tiles = vx_tiles(total, S);
  const size_t slots = (size_t)cap_mul * (size_t)total;
  std::vector<unsigned long long> key(slots, VX_EMPTY), repkey((size_t)total, VX_EMPTY), U(3 * slots, 0ull);
  std::vector<uint32_t> tfirst(slots, VX_NONE), tcount(slots, 0u), slot((size_t)total, VX_NONE), flag((size_t)S, 0u);
  std::vector<float> lo(3 * (size_t)S, 0.0f), hi(3 * (size_t)S, 0.0f), org(3 * (size_t)S, 0.0f), cent(3 * (size_t)total);
  std::vector<int> tile_seg((size_t)tiles, -1), tile_first((size_t)tiles, 0), tile_heads((size_t)tiles, 0), shift(S, 0);
  std::vector<char> seen((size_t)S, 0);
  // 1 bounds
  for (long long b = 0; b < tiles; ++b) {
    int l = 0, h = S;
    while (h - l > 1) {
      const int mid = l + ((h - l) >> 1);
      if (vx_tile_base(off[mid], mid) <= b) l = mid; else h = mid;
    }
    const int c = l, o0 = off[c], o1 = off[c + 1], n = o1 - o0;
    const long long f = (b - vx_tile_base(o0, c)) * VX_TILE;
    if (!(rg_valid_segment(o0, o1, total) && f >= 0 && f < n)) continue;
    tile_seg[b] = c;
    tile_first[b] = (int)f;
    for (int i = (int)f; i < n && i < f + VX_TILE; ++i)
      for (int a = 0; a < 3; ++a) {
        const float x = P[3 * ((size_t)o0 + i) + a];
        if (!kg_finite(x)) flag[c] |= VX_NON_FINITE;
        if (!seen[c] || x < lo[3 * c + a]) lo[3 * c + a] = x;
        if (!seen[c] || x > hi[3 * c + a]) hi[3 * c + a] = x;
        if (a == 2) seen[c] = 1;
      }
  }
  for (int c = 0; c < S; ++c) {
    for (int a = 0; a < 3; ++a) org[3 * c + a] = origin ? origin[3 * c + a] : lo[3 * c + a];
    shift[c] = (flag[c] & VX_NON_FINITE) ? 0 : vx_shift(&lo[3 * c], &hi[3 * c]);
  }
  // the points of a tile in the order of this run
  auto visit = [&](long long b, auto&& body) {
    const int c = tile_seg[b];
    if (c < 0) return;
    const int n = off[c + 1] - off[c], f = tile_first[b], e = n < f + VX_TILE ? n : f + VX_TILE;
    for (int t = f; t < e; ++t) body(c, order ? e - 1 - (t - f) : t);
  };
  auto tile_of = [&](long long bb) { return order ? tiles - 1 - bb : bb; };
  // 2 table
  int stuck = 0;
  for (long long bb = 0; bb < tiles; ++bb)
    visit(tile_of(bb), [&](int c, int i) {
      if ((flag[c] & VX_NON_FINITE) || !vx_good_size(voxel[c])) return;
      const int o0 = off[c], n = off[c + 1] - o0;
      const size_t g = (size_t)o0 + i, base = (size_t)cap_mul * o0;
      const uint32_t cap = (uint32_t)cap_mul * (uint32_t)n;
      int ok;
      const unsigned long long k = vx_key(P + 3 * g, &org[3 * c], voxel[c], &ok);
      if (!ok) {
        flag[c] |= VX_RANGE;
        return;
      }
      uint32_t s = vx_home(k, cap), probe = 0;
      while (probe < cap && key[base + s] != VX_EMPTY && key[base + s] != k) s = s + 1u == cap ? 0u : s + 1u, ++probe;
      if (probe == cap) {
        stuck = 1;
        return;
      }
      key[base + s] = k;
      slot[g] = s;
      if ((uint32_t)i < tfirst[base + s]) tfirst[base + s] = (uint32_t)i;
      tcount[base + s] += 1u;
      for (int a = 0; a < 3; ++a) U[3 * (base + s) + a] += vx_quantise(P[3 * g + a], lo[3 * c + a], shift[c]);
    });
  if (stuck) return -2;
  auto is_head = [&](int c, int i) {
    const size_t g = (size_t)off[c] + i;
    return slot[g] != VX_NONE && tfirst[(size_t)cap_mul * off[c] + slot[g]] == (uint32_t)i;
  };
  // 3 heads
  for (long long b = 0; b < tiles; ++b)
    visit(b, [&](int c, int i) {
      if (vx_status(flag[c], voxel[c]) == 0 && is_head(c, i)) tile_heads[b] += 1;
    });
  // 4 scan
  for (int c = 0; c < S; ++c) {
    const int o0 = off[c], o1 = off[c + 1];
    if (!rg_valid_segment(o0, o1, total)) {
      nvox[c] = 0;
      continue;
    }
    const int status = vx_status(flag[c], voxel[c]);
    if (status != 0) {
      nvox[c] = status;
      continue;
    }
    int carry = 0;
    for (int t = 0; t < vx_cloud_tiles(o1 - o0); ++t) {
      int& h = tile_heads[vx_tile_base(o0, c) + t];
      const int v = h;
      h = carry;
      carry += v;
    }
    nvox[c] = carry;
  }
  // 5 rows (a head's rank inside its tile: the heads of the tile below it, whatever the order of the visit)
  for (long long bb = 0; bb < tiles; ++bb)
    visit(tile_of(bb), [&](int c, int i) {
      const int o0 = off[c], V = nvox[c];
      const size_t g = (size_t)o0 + i;
      if (V < 0) owner[g] = -1;
      if (i >= V) {
        centroid[3 * g] = centroid[3 * g + 1] = centroid[3 * g + 2] = NAN;
        count[g] = first[g] = rep[g] = -1;
      }
      if (V < 0 || !is_head(c, i)) return;
      const long long b = vx_tile_base(o0, c) + i / VX_TILE;
      int v = tile_heads[b];
      for (int j = tile_first[b]; j < i; ++j) v += is_head(c, j);
      owner[g] = v;
      const size_t t = (size_t)cap_mul * o0 + slot[g], row = (size_t)o0 + v;
      for (int a = 0; a < 3; ++a)
        centroid[3 * row + a] = cent[3 * row + a] = vx_centroid(lo[3 * c + a], U[3 * t + a], tcount[t], shift[c]);
      count[row] = (int32_t)tcount[t];
      first[row] = i;
    });
  // 6 owner and the rep candidates
  for (long long bb = 0; bb < tiles; ++bb)
    visit(tile_of(bb), [&](int c, int i) {
      const int o0 = off[c], V = nvox[c];
      if (V < 0) return;
      const size_t g = (size_t)o0 + i;
      const uint32_t f = tfirst[(size_t)cap_mul * o0 + slot[g]];
      const int v = owner[(size_t)o0 + f];
      if (f != (uint32_t)i) owner[g] = v;
      const size_t row = (size_t)o0 + v;
      const float d = kg_dist(P[3 * g], P[3 * g + 1], P[3 * g + 2], cent[3 * row], cent[3 * row + 1], cent[3 * row + 2]);
      const unsigned long long k = vx_rep_key(d, (uint32_t)i);
      if (k < repkey[row]) repkey[row] = k;
    });
  // 7 rep
  for (long long b = 0; b < tiles; ++b)
    visit(b, [&](int c, int i) {
      if (i < nvox[c]) rep[(size_t)off[c] + i] = (int32_t)vx_rep_index(repkey[(size_t)off[c] + i]);
    });
  return vx_launches();
}

}  // extern "C"

// The definition, as a plain loop over one cloud: a map from the cell triple to the voxel number.
static int plain(const float* P, int n, float h, const float* origin, int32_t* owner, float* centroid, int32_t* count,
                 int32_t* first, int32_t* rep) {
  for (int i = 0; i < n; ++i) {
    owner[i] = count[i] = first[i] = rep[i] = -1;
    centroid[3 * i] = centroid[3 * i + 1] = centroid[3 * i + 2] = NAN;
  }
  for (int i = 0; i < 3 * n; ++i)
    if (!kg_finite(P[i])) return -1;
  if (!(h > 0.0f) || !kg_finite(h)) return -2;
  if (n == 0) return 0;
  float lo[3], hi[3], o[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = hi[a] = P[a];
    for (int i = 1; i < n; ++i) lo[a] = fminf(lo[a], P[3 * i + a]), hi[a] = fmaxf(hi[a], P[3 * i + a]);
    o[a] = origin ? origin[a] : lo[a];
  }
  std::map<std::vector<long long>, int> number;
  std::vector<std::vector<int>> members;
  for (int i = 0; i < n; ++i) {
    std::vector<long long> cell(3);
    for (int a = 0; a < 3; ++a) {
      const double q = floor(((double)P[3 * i + a] - (double)o[a]) / (double)h);
      if (!(q >= -1048576.0 && q < 1048576.0)) return -2;
      cell[a] = (long long)q;
    }
    auto at = number.find(cell);
    if (at == number.end()) {
      at = number.emplace(cell, (int)members.size()).first;
      members.emplace_back();
    }
    members[at->second].push_back(i);
  }
  const int s = vx_shift(lo, hi);
  for (size_t v = 0; v < members.size(); ++v) {
    unsigned long long U[3] = {0, 0, 0};
    for (int i : members[v]) {
      owner[i] = (int)v;
      for (int a = 0; a < 3; ++a) U[a] += vx_quantise(P[3 * i + a], lo[a], s);
    }
    float* c = centroid + 3 * v;
    for (int a = 0; a < 3; ++a) c[a] = vx_centroid(lo[a], U[a], (uint32_t)members[v].size(), s);
    count[v] = (int)members[v].size();
    first[v] = members[v][0];
    float best = 0.0f;
    for (int i : members[v]) {
      const float d = kg_dist(P[3 * i], P[3 * i + 1], P[3 * i + 2], c[0], c[1], c[2]);
      if (rep[v] < 0 || d < best) best = d, rep[v] = i;
    }
  }
  return (int)members.size();
}

static bool same(float a, float b) { return kg_bits(a) == kg_bits(b) || (a != a && b != b); }

static int self_check(void) {
  // six clouds: a 13^3 dyadic lattice on the faces of its cells (2 197 points, three tiles), 600 copies of one point
  // among 400 others, three points, an empty cloud, a cloud with one NaN, a cloud too wide for its voxel
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
  for (int i = 0; i < 30; ++i) P.push_back(100.0f * i);
  off.push_back((int32_t)(P.size() / 3));
  const int S = (int)off.size() - 1, total = off[S];
  const float voxel[6] = {0.5f, 0.07f, 1.0f, 1.0f, 0.3f, 1e-3f};
  std::vector<float> origin(3 * S, 0.0f);
  for (int a = 0; a < 3; ++a) origin[a] = -0.75f, origin[3 + a] = 0.3f;      // cells below zero
  std::vector<int32_t> ow(total), cw(total), fw(total), rw(total), nw(S);
  std::vector<float> mw(3 * (size_t)total);
  for (int c = 0; c < S; ++c)
    nw[c] = plain(P.data() + 3 * (size_t)off[c], off[c + 1] - off[c], voxel[c], origin.data() + 3 * c, ow.data() + off[c],
                  mw.data() + 3 * (size_t)off[c], cw.data() + off[c], fw.data() + off[c], rw.data() + off[c]);
  int differ = nw[0] != 7 * 7 * 7 || nw[4] != -1 || nw[5] != -2 || nw[3] != 0;
  for (int cap_mul = 2; cap_mul <= 3; ++cap_mul)
    for (int order = 0; order < 2; ++order) {
      std::vector<int32_t> o(total), c(total), f(total), rp(total), nv(S);
      std::vector<float> m(3 * (size_t)total);
      if (vxh_voxel(P.data(), off.data(), S, total, voxel, origin.data(), cap_mul, order, o.data(), nv.data(), m.data(),
                    c.data(), f.data(), rp.data()) != vx_launches())
        return 1;
      for (int s = 0; s < S; ++s) differ += nv[s] != nw[s];
      for (int g = 0; g < total; ++g)
        differ += o[g] != ow[g] || c[g] != cw[g] || f[g] != fw[g] || rp[g] != rw[g] || !same(m[3 * g], mw[3 * g]) ||
                  !same(m[3 * g + 1], mw[3 * g + 1]) || !same(m[3 * g + 2], mw[3 * g + 2]);
    }
  printf("voxel_host: %d clouds, %d points, %d launches: %d differences from the plain loop\n", S, total, vx_launches(),
         differ);
  return differ != 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return self_check();
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int n;
  float h;
  if (fscanf(f, "%d %f", &n, &h) != 2 || n < 0) return 2;
  std::vector<float> P((size_t)3 * n);
  for (size_t t = 0; t < P.size(); ++t)
    if (fscanf(f, "%f", &P[t]) != 1) return 2;
  fclose(f);
  const int32_t off[2] = {0, n};
  std::vector<int32_t> owner(n), count(n), first(n), rep(n);
  std::vector<float> centroid((size_t)3 * n);
  int32_t nvox = 0;
  if (vxh_voxel(P.data(), off, 1, n, &h, nullptr, 2, 0, owner.data(), &nvox, centroid.data(), count.data(), first.data(),
                rep.data()) < 0)
    return 1;
  printf("%d\n", nvox);
  for (int i = 0; i < n; ++i) printf(i ? " %d" : "%d", owner[i]);
  printf("\n");
  return 0;
}
