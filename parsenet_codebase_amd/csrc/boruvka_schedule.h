// The launch schedule of the Boruvka engines that merge components in global memory: cluster.hip (cluster_math.h) and
// orient_global.hip (orient_global_math.h).  Plain C++ behind BV_HD so that the same source is compiled into the
// gfx950 kernels and, by the test suite only (tests/native/cluster_host.cpp, tests/native/orient_global_host.cpp), into
// the serial simulations of the launches.
//
// Both engines keep a parent word P[v] per vertex (between rounds every vertex points at the root of its component,
// initially itself), a 64-bit slot best[v] and a hook word H[v].  A round is: offers (the least key over the edges that
// leave a component arrives in best[root]), hooks (a root with an entry writes its new parent to H; of a mutual pick the
// lower root stays root), and compress passes (every vertex walks up to BV_WALK parents).  What an edge, a key and a
// word are — the offers, cl_hook / og_hook, cl_walk / og_walk and the hook and compress kernels — stays with each
// engine: the words of orient_global carry a parity bit where those of cluster carry range guards, and one shared
// version of any of them would branch on its caller.
//
// The schedule, fixed by the host from the largest segment max_n alone:
//   bv_rounds  ceil(log2 max_n) + 1.  A component that finds an entry (an edge that leaves it) is merged with at least
//              one other, and one that finds none never finds one again (it is a whole connected component of the
//              graph), so the number of components that can still find an entry at least halves per round: after
//              ceil(log2 n) rounds it is at most one, which has no partner.  One more round sees "no entry" and raises
//              no flag.
//   bv_passes  the smallest C with BV_WALK^C >= max_n.  Before the hooks every vertex is at depth <= 1; the hooks of a
//              round can line the components up in one chain, depth <= n - 1.  A pass takes a vertex at depth d to an
//              ancestor at least min(d, BV_WALK) levels up (a stale or a fresher word is never lower), and roots do not
//              move during the passes, so by induction over d the new depth is at most ceil(d / BV_WALK): 1 for
//              d <= BV_WALK, else 1 + ceil((d - BV_WALK) / BV_WALK).  After C passes the depth is at most
//              ceil((n - 1) / BV_WALK^C) = 1: every vertex points at its root, which the next round's offers need.
// A per-round control word any[r] — a root found an entry in round r — lets every launch behind the last merge exit in
// its first instructions; changed[r][p] — pass p of round r moved a word — does the same for the passes behind the one
// that moved nothing.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BV_HD __host__ __device__ static inline __attribute__((always_inline))
#else
#define BV_HD static inline __attribute__((always_inline))
#endif

#define BV_WALK 64                      // parents a vertex walks per compress pass
#define BV_NO_HOOK 0xffffffffu          // no word in H: a parent is below 2^31 - 1
#define BV_MAX_ROUNDS 32                // bv_rounds(2^31 - 1)
#define BV_MAX_PASSES 8                 // > bv_passes(2^31 - 1) = 6
// control words (zeroed before the first launch): any[r] at BV_CTRL_ANY + r, changed[r][p] at
// BV_CTRL_CHANGED + r BV_MAX_PASSES + p
#define BV_CTRL_ANY 0
#define BV_CTRL_CHANGED 64
#define BV_CTRL_WORDS (BV_CTRL_CHANGED + BV_MAX_ROUNDS * BV_MAX_PASSES)

BV_HD int bv_rounds(int max_n) {
  int r = 0;
  while (r < 31 && (1ll << r) < (long long)max_n) ++r;
  return r + 1;
}

BV_HD int bv_passes(int max_n) {
  int c = 1;
  long long reach = BV_WALK;
  while (reach < (long long)max_n) reach *= BV_WALK, ++c;
  return c;
}

// The word of x as the FIRST compress pass of a round sees it: P[x], or H[x] while x still stands as a root in P with a
// hook pending.  Both are an ancestor of x in the hooked forest (with whatever the engine packs beside it), so a reader
// may see either.  Later passes read P alone: the first pass has stored a word over every hooked root (its own thread
// walks from H[x], which is not x).
BV_HD uint32_t bv_word(const uint32_t* P, const uint32_t* H, uint32_t x, int first) {
  const uint32_t w = P[x];
  if (first && w == x) {
    const uint32_t h = H[x];
    if (h != BV_NO_HOOK) return h;
  }
  return w;
}
