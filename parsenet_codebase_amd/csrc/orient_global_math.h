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
//   og_walk    up to OG_WALK further parents from the word of v; returns (ancestor, parity to it).  Every word read on
//              the way is a single load of a pair (ancestor, parity), whichever of its values a concurrent walk left
//              there, so the result is correct under any interleaving and under stale reads.
//
// The schedule — og_rounds = bv_rounds rounds of offers, hooks and og_passes = bv_passes compress passes, with the proof
// of both bounds —, the control words and the word a pass reads (og_word = bv_word) are boruvka_schedule.h, shared with
// cluster_math.h.
//   og_launches  1 (init) + rounds x (offers + hooks + passes) + 2 (seed keys, outputs).
#pragma once
#include "boruvka_schedule.h"
#include "orient_math.h"

#define OG_BLOCK 256                    // threads per workgroup of every kernel
#define OG_MAX_BLOCKS 1024              // workgroups per launch at most: 16 waves on each of the 256 CUs
#define OG_STRIDE (OG_BLOCK * OG_MAX_BLOCKS)   // entries (or vertices) one launch covers before its lanes stride on
// The shared schedule under the names of this engine, which orient_global.hip and the host simulation use.  The walk
// width stands here as a figure, because the test suite reads it from this file; it is held to BV_WALK below.
#define OG_WALK 64
static_assert(OG_WALK == BV_WALK, "OG_WALK is the walk width of boruvka_schedule.h");
#define OG_NO_HOOK BV_NO_HOOK
#define OG_MAX_ROUNDS BV_MAX_ROUNDS
#define OG_MAX_PASSES BV_MAX_PASSES
#define OG_CTRL_ANY BV_CTRL_ANY
#define OG_CTRL_CHANGED BV_CTRL_CHANGED
#define OG_CTRL_WORDS BV_CTRL_WORDS
OM_HD int og_rounds(int max_n) { return bv_rounds(max_n); }
OM_HD int og_passes(int max_n) { return bv_passes(max_n); }
OM_HD uint32_t og_word(const uint32_t* P, const uint32_t* H, uint32_t x, int first) { return bv_word(P, H, x, first); }

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

// One compress pass of vertex v: (ancestor, parity to it) up to OG_WALK parents above the word of v.
OM_HD uint32_t og_walk(const uint32_t* P, const uint32_t* H, uint32_t v, int first) {
  uint32_t w = bv_word(P, H, v, first);
  for (int t = 0; t < OG_WALK; ++t) {
    const uint32_t p = w & ~OM_PARITY;
    if (p == v) break;                                                 // v is a root
    const uint32_t wp = bv_word(P, H, p, first), q = wp & ~OM_PARITY;
    if (q == p) break;                                                 // p is a root
    w = q | ((w ^ wp) & OM_PARITY);
  }
  return w;
}
