// The per-element steps and the launch schedule of the global-memory engine of the consistent normal orientation
// (orient_global.hip), built on the definition in orient_math.h.  Plain C++ behind OM_HD so that the SAME source is
// compiled into the gfx950 kernels and, by the test suite only (tests/native/orient_global_host.cpp), into a serial
// simulation of the launches that is held against the Kruskal restatement bit for bit.
//
// All pointers and indices here are LOCAL to one segment of n points: P, H (n) packed words (parent | parity << 31),
// best (n) 64-bit keys, I (n,k) neighbour lists, N (n,3) normals.
//
//   og_offer   an entry (i, s) -> j: dropped (0), or the two components it is offered to and its key.
//   og_hook    a root's decision once every offer has arrived: OG_NO_HOOK (no entry, or the lower root of a mutual pick
//              stays root), or its new word (the other root, parity to it).  It only READS: the word goes to the
//              separate buffer H, because P[a], P[b] and best[other] belong to vertices that may be roots deciding in
//              the same launch.
//   og_word    the word of x as the FIRST compress pass of a round sees it: P[x], or H[x] while x still stands as a
//              root in P with a hook pending.  Both are (an ancestor of x in the hooked forest, the parity to it), so
//              a reader may see either.  Later passes read P alone: the first pass has stored a word over every hooked
//              root (its own thread walks from H[x], which is not x).
//   og_walk    up to OG_WALK further parents from the word of v; returns (ancestor, parity to it).  Every word read on
//              the way is a single load of a pair (ancestor, parity), whichever of its values a concurrent walk left
//              there, so the result is correct under any interleaving and under stale reads.
//
// The schedule, fixed by the host from the largest segment max_n alone:
//   og_rounds  ceil(log2 max_n) + 1.  A component that finds an entry is merged with at least one other, and one that
//              finds none never finds one again (it is a whole connected component of the graph), so the number of
//              components that can still find an entry at least halves per round: after ceil(log2 n) rounds it is at
//              most one, which has no partner.  One more round sees "no entry" and raises no flag.
//   og_passes  the smallest C with OG_WALK^C >= max_n.  Before the hooks every vertex is at depth <= 1; the hooks of a
//              round can line the components up in one chain, depth <= n - 1.  A pass takes a vertex at depth d to an
//              ancestor at least min(d, OG_WALK) levels up (a stale or a fresher word is never lower), and roots do not
//              move during the passes, so by induction over d the new depth is at most ceil(d / OG_WALK): 1 for
//              d <= OG_WALK, else 1 + ceil((d - OG_WALK) / OG_WALK).  After C passes the depth is at most
//              ceil((n - 1) / OG_WALK^C) = 1: every vertex points at its root, which the next round's offers need.
//   og_launches  1 (init) + rounds x (offers + hooks + passes) + 2 (seed keys, outputs).
#pragma once
#include "orient_math.h"

#define OG_BLOCK 256                    // threads per workgroup of every kernel
#define OG_MAX_BLOCKS 1024              // workgroups per launch at most: 16 waves on each of the 256 CUs
#define OG_STRIDE (OG_BLOCK * OG_MAX_BLOCKS)   // entries (or vertices) one launch covers before its lanes stride on
#define OG_WALK 64                      // parents a vertex walks per compress pass
#define OG_NO_HOOK 0xffffffffu          // no packed word: a parent is below 2^31 - 1
#define OG_MAX_ROUNDS 32                // og_rounds(2^31 - 1)
#define OG_MAX_PASSES 8                 // > og_passes(2^31 - 1) = 6
// control words (zeroed before the first launch): any[r] — a root found an entry in round r;
// changed[r][p] — pass p of round r moved a word
#define OG_CTRL_ANY 0
#define OG_CTRL_CHANGED 64
#define OG_CTRL_WORDS (OG_CTRL_CHANGED + OG_MAX_ROUNDS * OG_MAX_PASSES)

OM_HD int og_rounds(int max_n) {
  int r = 0;
  while (r < 31 && (1ll << r) < (long long)max_n) ++r;
  return r + 1;
}

OM_HD int og_passes(int max_n) {
  int c = 1;
  long long reach = OG_WALK;
  while (reach < (long long)max_n) reach *= OG_WALK, ++c;
  return c;
}

OM_HD int og_launches(int max_n) { return 1 + og_rounds(max_n) * (2 + og_passes(max_n)) + 2; }

// Entry e = i k + s of point i with j = I[e]: 0 if it is dropped (self, padding, outside the segment, both ends in one
// component), else 1 with the roots of both ends and the key.  Between rounds every vertex points at its root.
OM_HD int og_offer(const uint32_t* P, const float* N, int n, int k, int i, int s, int j, uint32_t* ci, uint32_t* cj,
                   unsigned long long* key) {
  if (j == i || (unsigned)j >= (unsigned)n) return 0;
  *ci = P[i] & ~OM_PARITY;
  *cj = P[j] & ~OM_PARITY;
  if (*ci == *cj) return 0;
  int neg;
  const float w = om_weight(N + 3 * i, N + 3 * j, &neg);
  *key = om_key(w, (uint32_t)(i * k + s));
  return 1;
}

// Of a mutual pick (both roots hold the same key: keys are unique) the lower root stays root.
OM_HD int og_stays_root(unsigned long long key, unsigned long long best_other, uint32_t v, uint32_t other) {
  return best_other == key && v < other;
}

// The root v after the offers: its new word, or OG_NO_HOOK; *any = 1 when it holds an entry at all.
OM_HD uint32_t og_hook(const uint32_t* P, const unsigned long long* best, const int32_t* I, const float* N, int k,
                       uint32_t v, int* any) {
  const unsigned long long key = best[v];
  if (key == OM_NO_ENTRY) return OG_NO_HOOK;
  *any = 1;
  const int e = (int)(uint32_t)key, a = e / k, b = I[e];              // (offered: b is inside the segment)
  const uint32_t wa = P[a], wb = P[b];
  const uint32_t ca = wa & ~OM_PARITY, cb = wb & ~OM_PARITY;
  const uint32_t other = ca == v ? cb : ca;
  if (og_stays_root(key, best[other], v, other)) return OG_NO_HOOK;
  int neg;
  om_weight(N + 3 * a, N + 3 * b, &neg);
  return other | (((wa ^ wb) & OM_PARITY) ^ ((uint32_t)neg << 31));
}

OM_HD uint32_t og_word(const uint32_t* P, const uint32_t* H, uint32_t x, int first) {
  const uint32_t w = P[x];
  if (first && w == x) {
    const uint32_t h = H[x];
    if (h != OG_NO_HOOK) return h;
  }
  return w;
}

// One compress pass of vertex v: (ancestor, parity to it) up to OG_WALK parents above the word of v.
OM_HD uint32_t og_walk(const uint32_t* P, const uint32_t* H, uint32_t v, int first) {
  uint32_t w = og_word(P, H, v, first);
  for (int t = 0; t < OG_WALK; ++t) {
    const uint32_t p = w & ~OM_PARITY;
    if (p == v) break;                                                 // v is a root
    const uint32_t wp = og_word(P, H, p, first), q = wp & ~OM_PARITY;
    if (q == p) break;                                                 // p is a root
    w = q | ((w ^ wp) & OM_PARITY);
  }
  return w;
}
