// Consistent orientation of the point normals of a ragged batch of clouds without a viewpoint, for gfx950: the signs
// are propagated along the minimum spanning forest of the k-NN graph under the weight 1 - |n_i . n_j| and one rule per
// connected component (the topmost point looks up) fixes the component's sign.  The definition — entries, weight,
// the strict order that makes the forest unique, the seed rule — is orient_math.h, the same source the test suite
// compiles for the host; the neighbours are those pn_knn3_ragged (knn3.hip) returns.
//
// ONE workgroup of 16 waves per cloud, Boruvka rounds, everything in LDS: no grid-wide synchronisation, no global
// atomic, no workspace, no floating-point atomic anywhere.
//   state   P[v], one 32-bit word per vertex: the parent in the low 31 bits, the parity (relative flip) to the
//           parent in the top bit.  Between rounds every vertex points at the root of its component.
//   offers  the lanes stride over the (point, slot) entries (coalesced idx reads, components looked up in LDS); an
//           entry whose ends lie in different components takes a 64-bit integer minimum of its key on BOTH
//           components' slots best[root] (a plain read first: a key that is not below the slot needs no atomic).
//           Both components must see the entry: the argument that Boruvka's picks close no cycle longer than a
//           mutual pick needs every component to choose among ALL entries incident to it — hence no transposed
//           lists.  An integer minimum does not depend on the order of arrival: the round is deterministic.
//   hooks   every root with an entry computes its new word (other root, parity = par(i) ^ par(j) ^ neg) into a
//           register while nobody writes, and stores it after the barrier; of a mutual pick (both slots hold the
//           same key: keys are unique) the lower root stays root.
//   jumps   P[v] = (parent(P[p]), par(v) ^ par(p)) for every vertex until nothing changes.  A word is read in a
//           single load, so whichever of its values a concurrent jump of p leaves is (an ancestor of p, the
//           parity to it): the step is correct under any interleaving and its fixed point (root, parity to the root)
//           is unique.
//   The rounds end when no component found an entry: at most ceil(log2 n) + 1 of them, each with at most
//   ceil(log2 n) + 1 jump passes (both loops carry a fixed cap above that, so that no input can spin a workgroup).
//   tail    a 64-bit integer maximum per root of (order-preserving map of z, inverted index) selects the seed; the
//           flip of v is par(v) ^ par(seed) ^ (n_z(seed) < 0); plain vector stores of normals, flip and seed.
// LDS: 8 bytes (slot) + 4 bytes (word) per vertex of the largest cloud the call can hold, min(total, 10 240):
// 120 KB of the CU's 160 KB at the limit, which needs the dynamic-LDS attribute.
// A segment above pn_orient_normals_max_points() is not truncated: its normals come out NaN and its flip and seed -1
// (the Python layer raises before the launch).
#include "common.h"
#include "orient_math.h"

#define ON_THREADS 1024
#define ON_MAX_POINTS 10240
#define ON_PER_THREAD (ON_MAX_POINTS / ON_THREADS)
#define ON_LDS_PER_POINT 12
#define ON_MAX_ROUNDS 32        // > ceil(log2 10 240) + 1 = 15
#define ON_MAX_JUMPS 32
#define ON_NO_HOOK 0xffffffffu  // (no packed word: a parent is below 10 240)

__global__ __launch_bounds__(ON_THREADS) void pn_orient_normals_kernel(
    const float* __restrict__ pts, const int* __restrict__ off, int total, const int* __restrict__ idx, int k,
    const float* __restrict__ nin, int cap, float* __restrict__ nout, int* __restrict__ flip, int* __restrict__ seed) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long on_lds[];
  unsigned long long* best = on_lds;                          // [cap] smallest key offered to a root; then seed keys
  uint32_t* P = reinterpret_cast<uint32_t*>(best + cap);      // [cap] parent | parity << 31
  const int tid = threadIdx.x;
  const int o0 = off[blockIdx.x], o1 = off[blockIdx.x + 1];
  if (o0 < 0 || o1 > total || o1 <= o0) return;               // (uniform: an empty segment, or offsets of another batch)
  const int n = o1 - o0;
  if (n > cap) {                                              // only above ON_MAX_POINTS: loud, never truncated
    for (int v = tid; v < n; v += ON_THREADS) {
      const size_t g = (size_t)o0 + v;
      nout[3 * g] = nout[3 * g + 1] = nout[3 * g + 2] = __builtin_nanf("");
      if (flip) flip[g] = -1;
      if (seed) seed[g] = -1;
    }
    return;
  }
  const float* __restrict__ N = nin + 3 * (size_t)o0;
  const int* __restrict__ I = idx + (size_t)o0 * k;
  const int E = n * k;                                        // <= 10 240 x 64

  for (int v = tid; v < n; v += ON_THREADS) {
    P[v] = (uint32_t)v;
    best[v] = OM_NO_ENTRY;
  }
  __syncthreads();

  const int di = ON_THREADS / k, ds = ON_THREADS - di * k;    // entry e + ON_THREADS is (i + di, s + ds), carried
  for (int round = 0; round < ON_MAX_ROUNDS; ++round) {
    int i = tid / k, s = tid - i * k;
    for (int e = tid; e < E; e += ON_THREADS) {
      const int j = I[e];
      if (j != i && (unsigned)j < (unsigned)n) {
        const uint32_t ci = P[i] & ~OM_PARITY, cj = P[j] & ~OM_PARITY;
        if (ci != cj) {
          int neg;
          const float w = om_weight(N + 3 * i, N + 3 * j, &neg);
          const unsigned long long key = om_key(w, (uint32_t)e);
          if (key < best[ci]) atomicMin(&best[ci], key);
          if (key < best[cj]) atomicMin(&best[cj], key);
        }
      }
      i += di, s += ds;
      if (s >= k) s -= k, ++i;
    }
    __syncthreads();

    uint32_t hook[ON_PER_THREAD];
    int any = 0;
#pragma unroll
    for (int t = 0; t < ON_PER_THREAD; ++t) {
      const int v = tid + t * ON_THREADS;
      hook[t] = ON_NO_HOOK;
      if (v < n && P[v] == (uint32_t)v) {
        const unsigned long long key = best[v];
        if (key != OM_NO_ENTRY) {
          const int e = (int)(uint32_t)key, a = e / k, b = I[e];       // (offered: b is inside the segment)
          const uint32_t wa = P[a], wb = P[b];
          const uint32_t ca = wa & ~OM_PARITY, cb = wb & ~OM_PARITY;
          const uint32_t other = ca == (uint32_t)v ? cb : ca;
          if (!(best[other] == key && (uint32_t)v < other)) {
            int neg;
            om_weight(N + 3 * a, N + 3 * b, &neg);
            hook[t] = other | (((wa ^ wb) & OM_PARITY) ^ ((uint32_t)neg << 31));
          }
          any = 1;
        }
      }
    }
    if (!__syncthreads_or(any)) break;
#pragma unroll
    for (int t = 0; t < ON_PER_THREAD; ++t)
      if (hook[t] != ON_NO_HOOK) P[tid + t * ON_THREADS] = hook[t];
    for (int v = tid; v < n; v += ON_THREADS) best[v] = OM_NO_ENTRY;
    __syncthreads();

    for (int pass = 0; pass < ON_MAX_JUMPS; ++pass) {
      int changed = 0;
      for (int v = tid; v < n; v += ON_THREADS) {
        const uint32_t w = P[v], p = w & ~OM_PARITY;
        const uint32_t wp = P[p], q = wp & ~OM_PARITY;
        if (q != p) {
          P[v] = q | ((w ^ wp) & OM_PARITY);
          changed = 1;
        }
      }
      if (!__syncthreads_or(changed)) break;
    }
  }

  // the seed of every component
  __syncthreads();
  for (int v = tid; v < n; v += ON_THREADS) best[v] = 0ull;
  __syncthreads();
  for (int v = tid; v < n; v += ON_THREADS) {
    const uint32_t r = P[v] & ~OM_PARITY;
    const unsigned long long zk = om_zkey(pts[3 * ((size_t)o0 + v) + 2], (uint32_t)v);
    if (zk > best[r]) atomicMax(&best[r], zk);
  }
  __syncthreads();
  for (int v = tid; v < n; v += ON_THREADS) {
    const uint32_t w = P[v];
    uint32_t sd = om_zkey_vertex(best[w & ~OM_PARITY]);                // a vertex of this component: below n
    if (sd >= (uint32_t)n) sd = (uint32_t)v;                           // (only if a cap above ended the rounds early)
    const int f = (int)((w ^ P[sd]) >> 31) ^ om_seed_flip(N[3 * sd + 2]);
    const size_t g = (size_t)o0 + v;
    nout[3 * g] = om_apply(N[3 * v], f);
    nout[3 * g + 1] = om_apply(N[3 * v + 1], f);
    nout[3 * g + 2] = om_apply(N[3 * v + 2], f);
    if (flip) flip[g] = f;
    if (seed) seed[g] = (int)sd;
  }
}

extern "C" int pn_orient_normals_max_points(void) { return ON_MAX_POINTS; }

extern "C" int pn_orient_normals_f32(const float* pts, const int* off, int S, int total, const int32_t* idx, int k,
                                     const float* normals_in, float* normals_out, int32_t* flip, int32_t* seed,
                                     void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PN_CHECK_ARG(k >= OM_MIN_K && k <= OM_MAX_K, "pn_orient_normals_f32: k=%d (%d <= k <= %d)", k, OM_MIN_K, OM_MAX_K);
  PN_CHECK_ARG(S >= 0 && total >= 0, "pn_orient_normals_f32: S=%d total=%d", S, total);
  if (total == 0 || S == 0) return PN_OK;
  PN_CHECK_ARG(pts && off && idx && normals_in && normals_out, "pn_orient_normals_f32: null pointer");
  PN_CHECK_ARG(normals_in != normals_out, "pn_orient_normals_f32: normals_out must not be normals_in");
  const int cap = total < ON_MAX_POINTS ? total : ON_MAX_POINTS;
  static unsigned attr_devs = 0;
  if (pn_first_on_device(&attr_devs)) {
    PN_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pn_orient_normals_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, ON_MAX_POINTS * ON_LDS_PER_POINT));
  }
  PN_PROF("orient_normals", stream);
  hipLaunchKernelGGL(pn_orient_normals_kernel, dim3(S), dim3(ON_THREADS), (size_t)cap * ON_LDS_PER_POINT, stream, pts,
                     off, total, idx, k, normals_in, cap, normals_out, flip, seed);
  PN_CHECK_LAUNCH();
  return PN_OK;
}
