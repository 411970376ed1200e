// Test-only host simulation of the global-memory orientation engine (parsenet_codebase_amd/csrc/orient_global.hip): the
// launches of its schedule run serially, one after the other, on the SAME per-element steps the kernels compile
// (csrc/orient_global_math.h): init, then per round offers, hooks and og_passes compress passes with the walk cap
// OG_WALK, then the seed keys and the outputs.  The rounds and passes are exactly og_rounds / og_passes of the largest
// segment, the numbers pn_orient_normals_global_launches reports; the exit flags are the kernels'.  Inside a launch the
// elements are visited in ascending order or, with order = 1, in descending order: two of the interleavings a GPU
// may produce, which must not change a bit.  tests/test_orient_global_abi.py holds the result against the Kruskal
// restatement (orient_math_host.cpp) in every bit and reads the report.  Not part of the product.
//
// report[0]  1 when the schedule sufficed: the last scheduled round found no entry, and after the passes of every round
//            every vertex pointed at a root (no cap was hit)
// report[1]  rounds in which a component found an entry          report[2]  og_rounds(max_n)
// report[3]  the most compress passes that moved a word in one round   report[4]  og_passes(max_n)
// report[5]  og_launches(max_n)          report[6]  the largest depth met before the passes of a round
//
// As a program (it has a main) it reads one cloud in the text format of orient_math_host.cpp from the file named by its
// first argument, or from stdin, prints one line  nx ny nz flip seed  per point, and the report on stderr; it returns
// 1 when the schedule did not suffice.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../parsenet_codebase_amd/csrc/orient_global_math.h"

static int ogh_depth(const std::vector<uint32_t>& P, const std::vector<uint32_t>& H, uint32_t v, int first, int cap) {
  int d = 0;
  uint32_t x = v;
  while (d <= cap) {
    const uint32_t p = og_word(P.data(), H.data(), x, first) & ~OM_PARITY;
    if (p == x) return d;
    x = p, ++d;
  }
  return d;                                                            // a cycle: above every bound
}

// One segment under the schedule (rounds, passes).  Returns 1 when the schedule sufficed.
static int ogh_segment(const float* pts, int n, const int32_t* I, int k, const float* N, int rounds, int passes,
                       int order, float* nout, int32_t* flip, int32_t* seed, int* report) {
  std::vector<uint32_t> P(n), H(n, OG_NO_HOOK);
  std::vector<unsigned long long> best(n, OM_NO_ENTRY);
  std::vector<int> any(rounds + 1, 0);
  int ok = 1;
  const int v0 = order ? n - 1 : 0, dv = order ? -1 : 1;
  for (int v = 0; v < n; ++v) P[v] = (uint32_t)v;
  for (int r = 0; r < rounds; ++r) {
    if (r > 0 && !any[r - 1]) break;                                   // (the launches exit at the flag)
    for (int c = 0, i = v0; c < n; ++c, i += dv)                       // offers
      for (int s = 0; s < k; ++s) {
        uint32_t ci, cj;
        unsigned long long key;
        if (!og_offer(P.data(), N, n, k, i, s, I[(size_t)i * k + s], &ci, &cj, &key)) continue;
        if (key < best[ci]) best[ci] = key;
        if (key < best[cj]) best[cj] = key;
      }
    for (int c = 0, v = v0; c < n; ++c, v += dv) {                     // hooks: reads only, the word goes to H
      H[v] = OG_NO_HOOK;
      if (P[v] == (uint32_t)v) H[v] = og_hook(P.data(), best.data(), I, N, k, (uint32_t)v, &any[r]);
    }
    if (!any[r]) break;
    report[1] += 1;
    for (int v = 0; v < n; ++v) report[6] = std::max(report[6], ogh_depth(P, H, (uint32_t)v, 1, n));
    int changed = 1, used = 0;
    for (int p = 0; p < passes && changed; ++p) {                      // compress passes, in place
      changed = 0;
      for (int c = 0, v = v0; c < n; ++c, v += dv) {
        const uint32_t now = og_walk(P.data(), H.data(), (uint32_t)v, p == 0);
        if (now != P[v]) P[v] = now, changed = 1;
        if (p == 0) best[v] = OM_NO_ENTRY;
      }
      used += changed;
    }
    report[3] = std::max(report[3], used);
    for (int v = 0; v < n; ++v)
      if (ogh_depth(P, H, (uint32_t)v, 0, n) > 1) ok = 0;              // the passes did not reach the roots
  }
  if (any[rounds - 1]) ok = 0;                                         // the last scheduled round still found an entry
  std::fill(best.begin(), best.end(), 0ull);
  for (int v = 0; v < n; ++v) {
    const uint32_t r = P[v] & ~OM_PARITY;
    best[r] = std::max(best[r], om_zkey(pts[3 * v + 2], (uint32_t)v));
  }
  for (int v = 0; v < n; ++v) {
    const uint32_t w = P[v];
    uint32_t sd = om_zkey_vertex(best[w & ~OM_PARITY]);
    if (sd >= (uint32_t)n) sd = (uint32_t)v;
    const int f = (int)((w ^ P[sd]) >> 31) ^ om_seed_flip(N[3 * sd + 2]);
    for (int c = 0; c < 3; ++c) nout[3 * v + c] = om_apply(N[3 * v + c], f);
    flip[v] = f;
    seed[v] = (int)sd;
  }
  return ok;
}

// A ragged batch: pts (total,3), off (S+1), idx (total,k) local indices, nin (total,3); report: 7 ints (above).
extern "C" void ogh_orient(const float* pts, const int* off, int S, const int32_t* idx, int k, const float* nin, int order,
                           float* nout, int32_t* flip, int32_t* seed, int* report) {
  int max_n = 0;
  for (int s = 0; s < S; ++s) max_n = std::max(max_n, off[s + 1] - off[s]);
  const int rounds = og_rounds(max_n), passes = og_passes(max_n);
  for (int t = 0; t < 7; ++t) report[t] = 0;
  report[0] = 1, report[2] = rounds, report[4] = passes, report[5] = og_launches(max_n);
  for (int s = 0; s < S; ++s) {
    const size_t o = (size_t)off[s];
    if (!ogh_segment(pts + 3 * o, off[s + 1] - off[s], idx + o * k, k, nin + 3 * o, rounds, passes, order, nout + 3 * o,
                     flip + o, seed + o, report))
      report[0] = 0;
  }
}

extern "C" int ogh_constant(int which) {
  const int c[] = {OG_BLOCK, OG_MAX_BLOCKS, OG_STRIDE, OG_WALK, OG_MAX_ROUNDS, OG_MAX_PASSES, OG_CTRL_WORDS};
  return which >= 0 && which < 7 ? c[which] : -1;
}
extern "C" int ogh_rounds(int max_n) { return og_rounds(max_n); }
extern "C" int ogh_passes(int max_n) { return og_passes(max_n); }
extern "C" int ogh_launches(int max_n) { return og_launches(max_n); }

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) {
    fprintf(stderr, "orient_global_host: cannot open %s\n", argv[1]);
    return 2;
  }
  int n = 0, k = 0, rc = 0;
  if (fscanf(f, "%d %d", &n, &k) != 2 || n < 0 || n > (1 << 20) || k < OM_MIN_K || k > OM_MAX_K) {
    fprintf(stderr, "orient_global_host: expected `n k` with %d <= k <= %d\n", OM_MIN_K, OM_MAX_K);
    return 2;
  }
  std::vector<float> P(3 * (size_t)n + 1), N(3 * (size_t)n + 1), out(3 * (size_t)n + 1);
  std::vector<int32_t> idx((size_t)n * k + 1), flip(n + 1), seed(n + 1);
  for (int i = 0; i < n && rc == 0; ++i)
    if (fscanf(f, "%f %f %f %f %f %f", &P[3 * i], &P[3 * i + 1], &P[3 * i + 2], &N[3 * i], &N[3 * i + 1], &N[3 * i + 2]) != 6) {
      fprintf(stderr, "orient_global_host: %d points announced, point %d is missing\n", n, i);
      rc = 2;
    }
  for (int e = 0; e < n * k && rc == 0; ++e)
    if (fscanf(f, "%d", &idx[e]) != 1) {
      fprintf(stderr, "orient_global_host: %d x %d indices announced, index %d is missing\n", n, k, e);
      rc = 2;
    }
  if (rc == 0) {
    const int off[2] = {0, n};
    int report[7];
    ogh_orient(P.data(), off, 1, idx.data(), k, N.data(), 0, out.data(), flip.data(), seed.data(), report);
    for (int i = 0; i < n; ++i)
      printf("%.9g %.9g %.9g %d %d\n", out[3 * i], out[3 * i + 1], out[3 * i + 2], flip[i], seed[i]);
    fprintf(stderr, "sufficed %d, rounds %d of %d, passes %d of %d, launches %d, depth %d\n", report[0], report[1],
            report[2], report[3], report[4], report[5], report[6]);
    rc = report[0] ? 0 : 1;
  }
  if (f != stdin) fclose(f);
  return rc;
}
