// Test-only program over parsenet_codebase_amd/csrc/ragged.h, the segment search and the workspace carver that
// knn3_grid.hip, orient_global.hip and fps.hip share, compiled for the host.  Not part of the product.
//
// Search: every offsets vector of S <= 6 segments with sizes from {0, 1, 2, 3} (5 461 of them), every x from -1 to
// total (and on to the last tile number): rg_segment under the row key off[s] and under the tile key off[s] / 2 + s
// (fps_tile_base with a tile of 2) against a linear scan for the last s whose key is <= x; every row of a batch lies in
// the segment found and passes rg_segment_holds, and no other x does.  The two predicates against their definitions
// written out one comparison at a time, over every (o0, o1, total, x) in -2 .. 4.
// Carver: six typed takes, one of them empty.  On base 0 it returns the sum of the bytes and hands out offsets; on a
// buffer every pointer lies at the offset the sum predicts, and every array, filled with a value of its own to its
// last element, still holds it after the others were filled (no overlap, nothing past the end: the sanitizer build
// of this program checks the latter).
// Returns 1 on any difference and prints the counts.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../parsenet_codebase_amd/csrc/ragged.h"

static const int TILE = 2;
static long long tile_key(const int* off, int s) { return (long long)(off[s] / TILE) + s; }

static int linear_rows(const int* off, int S, int x) {
  int found = 0;
  for (int s = 0; s < S; ++s)
    if (off[s] <= x) found = s;
  return found;
}

static int linear_tiles(const int* off, int S, long long b) {
  int found = 0;
  for (int s = 0; s < S; ++s)
    if (tile_key(off, s) <= b) found = s;
  return found;
}

static long long check_search(long long* vectors) {
  long long differ = 0;
  for (int S = 0; S <= 6; ++S) {
    int combos = 1;
    for (int s = 0; s < S; ++s) combos *= 4;
    for (int code = 0; code < combos; ++code) {
      int off[7] = {0, 0, 0, 0, 0, 0, 0};
      for (int s = 0, c = code; s < S; ++s, c /= 4) off[s + 1] = off[s] + c % 4;
      const int total = off[S];
      ++*vectors;
      for (int x = -1; x <= total; ++x) {
        const int s = rg_row_segment(off, S, x);
        differ += s != linear_rows(off, S, x);
        if (S == 0) continue;
        const int inside = x >= 0 && x < total;      // the offsets are valid: a row of the batch lies in the segment found
        differ += rg_segment_holds(off[s], off[s + 1], total, x) != inside;
        differ += !rg_valid_segment(off[s], off[s + 1], total);
      }
      const long long tiles = total / TILE + S;
      for (long long b = -1; b <= (tiles > total ? tiles : total); ++b)
        differ += rg_segment(S, b, [&off](int s) { return tile_key(off, s); }) != linear_tiles(off, S, b);
    }
  }
  return differ;
}

static long long check_predicates(void) {
  long long differ = 0;
  for (int o0 = -2; o0 <= 4; ++o0)
    for (int o1 = -2; o1 <= 4; ++o1)
      for (int total = -2; total <= 4; ++total) {
        int valid = 1;
        if (o0 < 0) valid = 0;
        if (o1 < o0) valid = 0;
        if (total < o1) valid = 0;
        differ += (rg_valid_segment(o0, o1, total) != 0) != (valid != 0);
        for (int x = -2; x <= 4; ++x) {
          int holds = valid;
          if (x < o0) holds = 0;
          if (x >= o1) holds = 0;
          differ += (rg_segment_holds(o0, o1, total, x) != 0) != (holds != 0);
        }
      }
  return differ;
}

struct Wide {
  unsigned char b[16];
};
struct Arrays {
  Wide* wide;
  double* d;
  int* i;
  unsigned long long* none;
  short* s;
  char* c;
};
static const long long COUNTS[6] = {2, 3, 5, 0, 3, 7};
static const long long SIZES[6] = {16, 8, 4, 8, 2, 1};

// The one function a kernel family writes: its arrays in order.
static long long carve(void* base, Arrays* a) {
  RgCarver c = {(uintptr_t)base, 0};
  a->wide = c.take<Wide>(COUNTS[0]);
  a->d = c.take<double>(COUNTS[1]);
  a->i = c.take<int>(COUNTS[2]);
  a->none = c.take<unsigned long long>(COUNTS[3]);
  a->s = c.take<short>(COUNTS[4]);
  a->c = c.take<char>(COUNTS[5]);
  return c.bytes;
}

static long long check_carver(void) {
  long long differ = 0, sum = 0, at[6];
  for (int t = 0; t < 6; ++t) at[t] = sum, sum += COUNTS[t] * SIZES[t];
  Arrays m;
  differ += carve(nullptr, &m) != sum;
  const uintptr_t measured[6] = {(uintptr_t)m.wide, (uintptr_t)m.d, (uintptr_t)m.i,
                                 (uintptr_t)m.none, (uintptr_t)m.s, (uintptr_t)m.c};
  for (int t = 0; t < 6; ++t) differ += measured[t] != (uintptr_t)at[t];
  std::vector<Wide> buffer((size_t)(sum + 15) / 16);      // exactly the bytes, rounded up to the alignment of Wide
  char* const base = (char*)buffer.data();
  Arrays a;
  differ += carve(base, &a) != sum;
  char* const got[6] = {(char*)a.wide, (char*)a.d, (char*)a.i, (char*)a.none, (char*)a.s, a.c};
  for (int t = 0; t < 6; ++t) {
    differ += got[t] != base + at[t];
    for (int u = t + 1; u < 6; ++u)      // [got[t], +bytes) and [got[u], +bytes) do not overlap
      differ += got[t] + COUNTS[t] * SIZES[t] > got[u] && COUNTS[t] > 0 && COUNTS[u] > 0;
  }
  for (long long e = 0; e < COUNTS[0]; ++e) memset(a.wide[e].b, 0x11, 16);
  for (long long e = 0; e < COUNTS[1]; ++e) a.d[e] = 2.5;
  for (long long e = 0; e < COUNTS[2]; ++e) a.i[e] = 0x33333333;
  for (long long e = 0; e < COUNTS[4]; ++e) a.s[e] = 0x5555;
  for (long long e = 0; e < COUNTS[5]; ++e) a.c[e] = 0x66;
  for (long long e = 0; e < COUNTS[0]; ++e)
    for (int b = 0; b < 16; ++b) differ += a.wide[e].b[b] != 0x11;
  for (long long e = 0; e < COUNTS[1]; ++e) differ += a.d[e] != 2.5;
  for (long long e = 0; e < COUNTS[2]; ++e) differ += a.i[e] != 0x33333333;
  for (long long e = 0; e < COUNTS[4]; ++e) differ += a.s[e] != 0x5555;
  for (long long e = 0; e < COUNTS[5]; ++e) differ += a.c[e] != 0x66;
  return differ;
}

int main(void) {
  long long vectors = 0;
  const long long search = check_search(&vectors), predicates = check_predicates(), carver = check_carver();
  printf("ragged_host: %lld offsets vectors; differences: search %lld, predicates %lld, carver %lld\n", vectors, search,
         predicates, carver);
  return search != 0 || predicates != 0 || carver != 0;
}
