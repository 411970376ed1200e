// Linear sum assignment on the device: a batched forward auction with eps-scaling (Bertsekas), minimising cost,
// fp64 costs and fp64 prices.  It serves the evaluation-mode LS refit (src/primitive_forward.py:197-198, 272-273:
// lapsolver.solve_dense on a 1 600 x 1 600 ... 2 100 distance matrix per spline segment); the reference has no
// counterpart on the GPU.  The result is eps-optimal, not optimal: the caller finishes it exactly on the host from
// the prices (parsenet_codebase_amd/assignment.py).
//
//   pn_lsa_auction_f64   S independent problems in ONE launch, sizes may differ
//
// One workgroup of 16 waves per problem: no grid-wide synchronisation, no global atomics.  Problem s has n rows and
// m >= n columns and is solved as the square m x m problem with m - n zero-cost rows, which are never materialised
// (a dummy row's bid reads the prices alone).  Row i values column j at c_ij + p_j (smaller is better).
//
// A round (Jacobi): every unassigned row bids — one wave per row scans the cost row for the best and the second-best
// value (ties -> the smaller column) and offers its best column j1 the price p_j1 + (w2 - w1) + eps; every column
// takes its HIGHEST offer, a tie goes to the LOWEST row; the previous owner of a column that changed hands is
// unassigned again.  The offers of a round are resolved with LDS max / min operations, whose result does not depend
// on the order they arrive in, so prices, assignment and the round count are the same from run to run (the ORDER of
// the unassigned list is not, and nothing depends on it: a row's bid is a function of the prices alone).
// After a round every assigned row i satisfies c_i,col(i) + p_col(i) <= min_j (c_ij + p_j) + eps: the winner's
// column costs it exactly w2 + eps, and the other prices only rise.
//
// Phases: eps starts at max(eps_start, eps_final) x the cost range, is divided by theta until it reaches
// eps_final x the range; between phases all assignments are reset and the prices are kept.
//
// LDS holds prices, owners, the offers and both unassigned lists (44 bytes per column; 2 100 columns = 90 KiB, so
// one workgroup per CU, which is all a batch of 16 problems asks of 256 CUs).  The cost matrix stays in global
// memory: a row (up to 16.4 KiB) is read ONCE per bid with no reuse inside the bid, and the reuse between rounds is
// of the whole 20-27 MB matrix, which no tile of the 160 KiB LDS holds — it is served by L2 / the Infinity Cache.
#include "common.h"
#include <limits.h>

#define LSA_WAVES 16
#define LSA_THREADS (LSA_WAVES * 64)
#define LSA_MAX_BATCH 64           // problems per launch (the table travels as a kernel argument)
#define LSA_MAX_M 3584             // 44 bytes of LDS per column: 154 KiB
#define LSA_COL_BYTES 44

struct LsaBatch {
  const double* cost[LSA_MAX_BATCH];
  int n[LSA_MAX_BATCH], m[LSA_MAX_BATCH], ld[LSA_MAX_BATCH];
};

// (best value, its column, second-best value) of two disjoint column sets
__device__ static inline void lsa_merge(double& a1, int& k1, double& a2, double b1, int kb, double b2) {
  if (b1 < a1 || (b1 == a1 && kb < k1)) {
    a2 = fmin(a1, b2);
    a1 = b1;
    k1 = kb;
  } else {
    a2 = fmin(a2, b1);
  }
}

// One wave: best / second-best of c_j + p_j over the m columns; crow == nullptr: a zero-cost dummy row.
__device__ static inline void lsa_scan(const double* __restrict__ crow, const double* price, int m, int lane, double& w1,
                                       int& j1, double& w2) {
  const double inf = __builtin_inf();
  double a1 = inf, a2 = inf;
  int k1 = INT_MAX;
  if (crow) {
    for (int j0 = 0; j0 < m; j0 += 512) {
      double c[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {           // eight loads in flight per lane
        const int j = j0 + 64 * u + lane;
        c[u] = j < m ? crow[j] : inf;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = j0 + 64 * u + lane;
        const double v = c[u] + (j < m ? price[j] : 0.0);
        if (v < a1) {                         // j ascends: strict < keeps the smaller column
          a2 = a1;
          a1 = v;
          k1 = j;
        } else if (v < a2) {
          a2 = v;
        }
      }
    }
  } else {
    for (int j = lane; j < m; j += 64) {
      const double v = price[j];
      if (v < a1) {
        a2 = a1;
        a1 = v;
        k1 = j;
      } else if (v < a2) {
        a2 = v;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double b1 = __shfl_xor(a1, o, 64), b2 = __shfl_xor(a2, o, 64);
    const int kb = __shfl_xor(k1, o, 64);
    lsa_merge(a1, k1, a2, b1, kb, b2);
  }
  w1 = a1;
  j1 = k1;
  w2 = a2;
}

// grid (problems of the launch), LSA_THREADS threads, dynamic LDS = 44 bytes x (largest m, rounded up to even).
__global__ __launch_bounds__(LSA_THREADS) void pn_lsa_auction_kernel(LsaBatch bt, int s0, double eps_start, double theta,
                                                                     double eps_final, int max_rounds, int out_ld,
                                                                     int* __restrict__ col, double* __restrict__ price_out,
                                                                     double* __restrict__ eps_out, int* __restrict__ rounds_out,
                                                                     int* __restrict__ status_out) {
  extern __shared__ double lsa_lds[];
  __shared__ double red_lo[LSA_WAVES], red_hi[LSA_WAVES];
  __shared__ int s_new;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = bt.n[s], m = bt.m[s], ld = bt.ld[s];
  const double* __restrict__ C = bt.cost[s];
  const int mp = (m + 1) & ~1;
  double* price = lsa_lds;                                                       // [m] column prices
  unsigned long long* bidv = reinterpret_cast<unsigned long long*>(price + mp);  // [m] highest offer of the round (bits)
  double* rbv = reinterpret_cast<double*>(bidv + mp);                            // [m] offer of list entry t
  int* bidr = reinterpret_cast<int*>(rbv + mp);                                  // [m] lowest row among the highest offers
  int* owner = bidr + mp;                                                        // [m] row that holds the column, -1 none
  int* rbj = owner + mp;                                                         // [m] column list entry t bids for
  int* list = rbj + mp;                                                          // [m] unassigned rows
  int* next = list + mp;                                                         // [m] ... of the next round

  // the cost range (real rows): the scale of eps
  double lo = __builtin_inf(), hi = -__builtin_inf();
  for (int i = wave; i < n; i += LSA_WAVES) {
    const double* crow = C + (size_t)i * ld;
    for (int j = lane; j < m; j += 64) {
      const double v = crow[j];
      lo = fmin(lo, v);
      hi = fmax(hi, v);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o, 64));
    hi = fmax(hi, __shfl_xor(hi, o, 64));
  }
  if (lane == 0) {
    red_lo[wave] = lo;
    red_hi[wave] = hi;
  }
  for (int j = tid; j < m; j += LSA_THREADS) {
    price[j] = 0.0;
    bidv[j] = 0ull;
    bidr[j] = INT_MAX;
  }
  __syncthreads();
  lo = red_lo[0];
  hi = red_hi[0];
  for (int w = 1; w < LSA_WAVES; ++w) {
    lo = fmin(lo, red_lo[w]);
    hi = fmax(hi, red_hi[w]);
  }
  double range = hi - lo;
  if (!(range > 0.0) || range == __builtin_inf()) range = 1.0;

  const double eps_last = eps_final * range;
  double eps = fmax(eps_start, eps_final) * range;
  int rounds = 0, status = 0;
  for (;;) {
    // a phase starts from no assignment and the prices of the last one
    for (int j = tid; j < m; j += LSA_THREADS) {
      owner[j] = -1;
      list[j] = j;
    }
    int cnt = m;
    __syncthreads();
    while (cnt > 0) {
      if (rounds >= max_rounds) {
        status = 1;
        break;
      }
      ++rounds;
      // offers: one wave per unassigned row
      for (int t = wave; t < cnt; t += LSA_WAVES) {
        const int row = list[t];
        double w1, w2;
        int j1;
        lsa_scan(row < n ? C + (size_t)row * ld : nullptr, price, m, lane, w1, j1, w2);
        if (lane == 0) {
          if (w2 == __builtin_inf()) w2 = w1;          // a single column
          const double b = price[j1] + ((w2 - w1) + eps);
          rbj[t] = j1;
          rbv[t] = b;
          // prices start at 0 and only rise: an offer is positive, its bit pattern orders like its value
          atomicMax(&bidv[j1], (unsigned long long)__double_as_longlong(b));
        }
      }
      __syncthreads();
      for (int t = tid; t < cnt; t += LSA_THREADS) {
        const int j = rbj[t];
        if ((unsigned long long)__double_as_longlong(rbv[t]) == bidv[j]) atomicMin(&bidr[j], list[t]);
      }
      if (tid == 0) s_new = 0;
      __syncthreads();
      // winners take their column (one per column: nobody else writes owner / price of it); losers and the rows
      // they displace bid again
      for (int t = tid; t < cnt; t += LSA_THREADS) {
        const int row = list[t], j = rbj[t];
        if (bidr[j] == row) {
          const int prev = owner[j];
          owner[j] = row;
          price[j] = rbv[t];
          if (prev >= 0) next[atomicAdd(&s_new, 1)] = prev;
        } else {
          next[atomicAdd(&s_new, 1)] = row;
        }
      }
      __syncthreads();
      for (int t = tid; t < cnt; t += LSA_THREADS) {
        const int j = rbj[t];
        bidv[j] = 0ull;
        bidr[j] = INT_MAX;
      }
      cnt = s_new;
      int* sw = list;
      list = next;
      next = sw;
      __syncthreads();
    }
    if (status || eps <= eps_last) break;
    eps = fmax(eps / theta, eps_last);
  }

  // (status and cnt are uniform: every thread took the same branches)
  int* oc = col + (size_t)(s0 + s) * out_ld;
  double* op = price_out + (size_t)(s0 + s) * out_ld;
  for (int j = tid; j < out_ld; j += LSA_THREADS) {
    oc[j] = -1;
    op[j] = j < m ? price[j] : 0.0;
  }
  __syncthreads();
  for (int j = tid; j < m; j += LSA_THREADS) {
    const int r = owner[j];
    if (r >= 0) oc[r] = j;
  }
  if (tid == 0) {
    eps_out[s0 + s] = eps;
    rounds_out[s0 + s] = rounds;
    status_out[s0 + s] = status;
  }
}

extern "C" int pn_lsa_auction_f64(const double* const* h_cost, const int* h_n, const int* h_m, const int* h_ld, int S,
                                  double eps_start, double theta, double eps_final, int max_rounds, int out_ld, int* col,
                                  double* price, double* eps, int* rounds, int* status, void* stream) {
  PN_CHECK_ARG(h_cost && h_n && h_m && h_ld && col && price && eps && rounds && status && S > 0,
               "pn_lsa_auction_f64: bad arguments");
  PN_CHECK_ARG(eps_start > 0.0 && eps_final > 0.0 && theta > 1.0 && max_rounds >= 1,
               "pn_lsa_auction_f64: schedule needs eps_start > 0, eps_final > 0, theta > 1 and max_rounds >= 1");
  int mmax = 0;
  for (int s = 0; s < S; ++s) {
    PN_CHECK_ARG(h_cost[s], "pn_lsa_auction_f64: problem %d has no cost matrix", s);
    PN_CHECK_ARG(h_n[s] >= 1 && h_n[s] <= h_m[s], "pn_lsa_auction_f64: problem %d has %d rows and %d columns (1 <= n <= m)",
                 s, h_n[s], h_m[s]);
    PN_CHECK_ARG(h_m[s] <= LSA_MAX_M, "pn_lsa_auction_f64: problem %d has %d columns (at most %d)", s, h_m[s], LSA_MAX_M);
    PN_CHECK_ARG(h_ld[s] >= h_m[s], "pn_lsa_auction_f64: problem %d has leading dimension %d < %d columns", s, h_ld[s],
                 h_m[s]);
    mmax = h_m[s] > mmax ? h_m[s] : mmax;
  }
  PN_CHECK_ARG(out_ld >= mmax, "pn_lsa_auction_f64: out_ld %d < %d columns", out_ld, mmax);
  static unsigned attr_devs = 0;
  if (pn_first_on_device(&attr_devs)) {
    PN_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pn_lsa_auction_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, LSA_MAX_M * LSA_COL_BYTES));
  }
  PN_PROF("lsa_auction", (hipStream_t)stream);
  for (int s0 = 0; s0 < S; s0 += LSA_MAX_BATCH) {
    const int ns = S - s0 < LSA_MAX_BATCH ? S - s0 : LSA_MAX_BATCH;
    LsaBatch bt;
    memset(&bt, 0, sizeof(bt));
    int mc = 0;
    for (int s = 0; s < ns; ++s) {
      bt.cost[s] = h_cost[s0 + s];
      bt.n[s] = h_n[s0 + s];
      bt.m[s] = h_m[s0 + s];
      bt.ld[s] = h_ld[s0 + s];
      mc = bt.m[s] > mc ? bt.m[s] : mc;
    }
    const size_t lds = (size_t)((mc + 1) & ~1) * LSA_COL_BYTES;
    hipLaunchKernelGGL(pn_lsa_auction_kernel, dim3(ns), dim3(LSA_THREADS), lds, (hipStream_t)stream, bt, s0, eps_start, theta,
                       eps_final, max_rounds, out_ld, col, price, eps, rounds, status);
    PN_CHECK_LAUNCH();
  }
  return PN_OK;
}
