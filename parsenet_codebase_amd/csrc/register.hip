// Rigid registration of a ragged batch of (source, target) cloud pairs of ANY size, for gfx950: the definition of
// register_math.h, the same source the test suite compiles for the host.  Iterative closest point on the exact grid
// search of knn3_query.hip — the kernels of knn3_query_kernels.h, compiled here a second time from the one source —:
// the target's grid is built ONCE per call (the four build launches of knn3_grid_build.h), every iteration only moves
// the source, bins the moved points into the target's cells and searches them.
//
// pn_register_launches(max_iter) = 12 + 9 max_iter stream-ordered launches (memsets come on top), a FIXED schedule: no
// host synchronisation, no cooperative launch, no workgroup waits for another.
//   1 - 4       bbox, cells, scan, scatter of the target
//   5 init      the tile table of the source (tile -> segment, first point), the state of every segment from init or the
//               identity, stop = 0, iterations = 0, status = MAX_ITER
//   per iteration, nine launches; every workgroup of a segment whose stop flag is set exits in its first instructions:
//     move      p' of every source point into the workspace (rr_move)
//     cells, scan, scatter, search   pn_knn3_query's launches 5 - 8 on p' with k = 1 and the stop flags: a stopped row
//               takes no position in the cell order, so no wave searches it
//     sums<0>   per tile of 1 024 source points (one workgroup of 256 lanes, four points per lane, lane-interleaved): the
//               paired target point is gathered, the six mean terms formed in fp64, added over the lane's four points in
//               point order (ol_lane_sum), over the wave by the xor butterfly of shuffles, over the four waves through
//               LDS (ol_wave_sum); one partial per tile and quantity, no floating atomic; the accepted pairs by ballots
//     means     per segment: the tile partials added in ascending order, the tiles' counts, pbar and qbar
//     sums<1>   per tile: the 9 (RR_POINT) or 27 (RR_PLANE, with the normal gathered too) centred terms, the same tree
//     solve     per segment: the partials in ascending order, then one lane runs rr_step — Horn's 4 x 4 Jacobi or the
//               6 x 6 LDL^T, the composition, the stopping rule — and writes state, iterations, status and the stop flag
//   final       move, cells, scan, scatter, search without stop flags into idx / dist (the caller's, or the workspace's),
//               sums<2> (dist^2 per tile and the accepted pairs), outputs (per segment: transform, count, rmse)
// With no source point the row launches are left out, with no target point the build, scan, scatter and search are.
// Visibility: a launch reads what earlier launches wrote (stream order); nothing is handed over inside a launch.
//
// Workspace (pn_register_workspace_bytes), tiles = totalS / 1024 + S: part 8 x 28 tiles | state 8 x 8 S | mean 8 x 6 S |
// the query's workspace over (target, source) (knn3_query_kernels.h) | moved 12 totalS | idx 4 totalS | dist 4 totalS |
// tcount, tile_seg, tile_first 4 tiles each | m, stop 4 S each.
//
// Resource report of hipcc --offload-arch=gfx950 -O3 (-Rpass-analysis=kernel-resource-usage), VGPRs / waves per SIMD, no
// kernel with scratch:
//   sums<0, POINT> 55 / 8   sums<0, PLANE> 57 / 8   sums<1, POINT> 80 / 6   sums<1, PLANE> 228 / 2 (27 fp64 accumulators
//   and the terms of a point)   sums<2> 14 / 8   move 38 / 8   init 42 / 8   means 30 / 8 (3 KiB LDS)   outputs 32 / 8
//   solve<POINT> 72 / 7 (the 4 x 4 Jacobi unrolled over its six pairs: the matrix in registers), 4.6 KiB LDS
//   solve<PLANE> 62 / 8, 13.7 KiB LDS (27 sums x RR_STAGE staged tiles)
//   the query's kernels here: cells<true> 29 VGPRs / 44 SGPRs, scatter 14 / 20, search 67 / 91, 7 waves: as in
//   knn3_query.hip but for the two scalar registers of the stop pointer in cells
#include "knn3_query_kernels.h"
#include "register_math.h"

struct RrWs {
  double* part;         // (28, tiles) sum q of tile b; 27 in use
  double* state;        // (S, 8) q (4), t (3), one spare
  double* mean;         // (S, 6) pbar, qbar
  KqWs q;
  float* moved;         // (totalS, 3)
  int32_t* idx;         // (totalS)
  float* dist;          // (totalS)
  int* tcount;          // (tiles) accepted pairs of the tile
  int* tile_seg;        // (tiles) -1: the tile number holds nothing
  int* tile_first;      // (tiles)
  int* m;               // (S) accepted pairs
  uint32_t* stop;       // (S)
  long long tiles;
};

#define RR_PART_ROWS 28
#define RR_STATE 8
#define RR_STAGE 64      // tile partials staged in LDS per round of a per-segment launch

static long long rr_carve(void* base, long long totalS, long long totalT, int S, RrWs* w) {
  RgCarver c = {(uintptr_t)base, 0};
  const long long tiles = ol_tiles(totalS, S);
  w->tiles = tiles;
  w->part = c.take<double>(RR_PART_ROWS * tiles);
  w->state = c.take<double>((long long)RR_STATE * S);
  w->mean = c.take<double>(6ll * S);
  kg_take(c, totalT, S, &w->q.g);
  w->q.qord = c.take<int>(totalS);
  w->q.qcell = c.take<int>(totalS);
  w->q.qrank = c.take<int>(totalS);
  w->q.qstart = c.take<int>(totalT + 2ll * S);
  w->moved = c.take<float>(3 * totalS);
  w->idx = c.take<int32_t>(totalS);
  w->dist = c.take<float>(totalS);
  w->tcount = c.take<int>(tiles);
  w->tile_seg = c.take<int>(tiles);
  w->tile_first = c.take<int>(tiles);
  w->m = c.take<int>(S);
  w->stop = c.take<uint32_t>(S);
  return c.bytes;
}

struct RrArgs {
  int mode;
  float max_dist;
  double tol_rot, tol_trans;
};

__device__ static inline RrState rr_load_state(const double* p) {
  RrState s;
  s.q[0] = p[0], s.q[1] = p[1], s.q[2] = p[2], s.q[3] = p[3];
  s.t[0] = p[4], s.t[1] = p[5], s.t[2] = p[6];
  return s;
}

// ---- 5: the tile table, the states, the flags ------------------------------------------------------------------------------
__global__ __launch_bounds__(RR_LANES) void pn_register_init_kernel(const int* __restrict__ off_s, int S, int totalS,
                                                                    const double* __restrict__ init, RrWs w,
                                                                    int32_t* __restrict__ iterations,
                                                                    int32_t* __restrict__ status) {
  const long long b = blockIdx.x;
  for (long long g = b * RR_LANES + threadIdx.x; g < S; g += (long long)gridDim.x * RR_LANES) {
    const RrState st = init ? rr_from_matrix(init + 16 * (size_t)g) : rr_identity();
    double* out = w.state + RR_STATE * (size_t)g;
    out[0] = st.q[0], out[1] = st.q[1], out[2] = st.q[2], out[3] = st.q[3];
    out[4] = st.t[0], out[5] = st.t[1], out[6] = st.t[2], out[7] = 0.0;
    w.stop[g] = 0u;
    w.m[g] = 0;
    iterations[g] = 0;
    status[g] = RR_MAX_ITER;
  }
  if (threadIdx.x != 0) return;
  const int c = rg_segment(S, b, [off_s](int s) { return ol_tile_base(off_s[s], s); });
  const int o0 = off_s[c], o1 = off_s[c + 1];
  const long long first = (b - ol_tile_base(o0, c)) * RR_TILE;
  const bool live = rg_valid_segment(o0, o1, totalS) && first >= 0 && first < o1 - o0;
  w.tile_seg[b] = live ? c : -1;
  w.tile_first[b] = live ? (int)first : 0;
  w.tcount[b] = 0;
}

// ---- move: p' of every source point ----------------------------------------------------------------------------------------
// state: (S, stride) doubles — the workspace's states (stride RR_STATE), or 4 x 4 matrices (stride 16, MATRIX).
template <bool MATRIX>
__global__ __launch_bounds__(256) void pn_register_move_kernel(const float* __restrict__ src,
                                                               const int* __restrict__ off_s, int S, int totalS,
                                                               const double* __restrict__ state,
                                                               const uint32_t* __restrict__ stop,
                                                               float* __restrict__ out) {
  const long long row64 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row64 >= totalS) return;
  const int row = (int)row64;
  const int s = kg_segment(off_s, S, row);
  if (stop && stop[s]) return;
  const float p[3] = {src[(size_t)row * 3], src[(size_t)row * 3 + 1], src[(size_t)row * 3 + 2]};
  float o[3] = {p[0], p[1], p[2]};                        // a row that no valid segment holds stays where it is
  if (rg_segment_holds(off_s[s], off_s[s + 1], totalS, row)) {
    const RrState st = MATRIX ? rr_from_matrix(state + 16 * (size_t)s) : rr_load_state(state + RR_STATE * (size_t)s);
    double R[9];
    rr_rotation(st.q, R);
    rr_move(R, st.t, p, o);
  }
  out[(size_t)row * 3] = o[0], out[(size_t)row * 3 + 1] = o[1], out[(size_t)row * 3 + 2] = o[2];
}

// ---- the sums of a tile ----------------------------------------------------------------------------------------------------
// STAGE 0: the six mean terms; 1: the centred terms of MODE; 2: dist^2 (the final evaluation: no stop flag is read).
template <int STAGE, int MODE>
__global__ __launch_bounds__(RR_LANES) void pn_register_sums_kernel(const int* __restrict__ off_s,
                                                                    const float* __restrict__ tgt,
                                                                    const int* __restrict__ off_t, int totalT,
                                                                    const float* __restrict__ normals, float max_dist,
                                                                    RrWs w, const int32_t* __restrict__ idx,
                                                                    const float* __restrict__ dist) {
  constexpr int K = STAGE == 0 ? RR_SUMS_MEAN : STAGE == 2 ? 1 : (MODE == RR_PLANE ? RR_SUMS_PLANE : RR_SUMS_POINT);
  __shared__ double sh[K][OL_WAVES];
  __shared__ int shc[OL_WAVES];
  const int c = w.tile_seg[blockIdx.x];
  if (c < 0) return;
  if (STAGE < 2 && w.stop[c]) return;
  const int o0 = off_s[c], n = off_s[c + 1] - o0, first = w.tile_first[blockIdx.x];
  const int t0 = off_t[c], t1 = off_t[c + 1];
  const int nt = rg_valid_segment(t0, t1, totalT) ? t1 - t0 : 0;
  double mean[RR_SUMS_MEAN] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (STAGE == 1) {
#pragma unroll
    for (int k = 0; k < RR_SUMS_MEAN; ++k) mean[k] = w.mean[RR_SUMS_MEAN * (size_t)c + k];
  }
  double acc[K];
  int cnt = 0;                                            // of this wave: the same in all its lanes
#pragma unroll
  for (int p = 0; p < RR_PER_LANE; ++p) {
    const int i = first + p * RR_LANES + (int)threadIdx.x;
    int j = -1;
    float d = 0.0f;
    if (i < n) j = idx[(size_t)o0 + i], d = dist[(size_t)o0 + i];
    if (j >= nt) j = -1;                                  // (cannot happen; never read outside the target segment)
    const float* nrm = MODE == RR_PLANE && j >= 0 ? normals + 3 * ((size_t)t0 + j) : nullptr;
    const int ok = rr_accept(j, d, max_dist, nrm);
    cnt += __popcll(__ballot(ok));
    double term[K];
#pragma unroll
    for (int k = 0; k < K; ++k) term[k] = 0.0;
    if (ok) {
      const float* q = tgt + 3 * ((size_t)t0 + j);
      const float* m = w.moved + 3 * ((size_t)o0 + i);
      if (STAGE == 0) rr_mean_terms(m, q, term);
      else if (STAGE == 2) term[0] = rr_residual_term(d);
      else if (MODE == RR_PLANE) rr_plane_terms(m, q, nrm, mean, term);
      else rr_point_terms(m, q, mean, term);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = p == 0 ? term[k] : ol_add(acc[k], term[k]);      // ol_lane_sum
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = acc[k];
#pragma unroll
    for (int h = OL_WAVE / 2; h > 0; h >>= 1) s = ol_add(s, __shfl_xor(s, h, OL_WAVE));
    if (pn_lane() == 0) sh[k][wave] = s;
  }
  if (pn_lane() == 0) shc[wave] = cnt;
  __syncthreads();
  if (threadIdx.x < K)
    w.part[(size_t)threadIdx.x * w.tiles + blockIdx.x] =
        ol_wave_sum(sh[threadIdx.x][0], sh[threadIdx.x][1], sh[threadIdx.x][2], sh[threadIdx.x][3]);
  if (STAGE != 1 && threadIdx.x == 0) w.tcount[blockIdx.x] = ((shc[0] + shc[1]) + shc[2]) + shc[3];
}

// The K sums of segment c: the tile partials in ascending order, lane k those of sum k, RR_STAGE tiles staged per round.
// Returns the sum in the lanes below K; every lane of the workgroup must call it.
template <int K>
__device__ static inline double rr_cloud_sum(const RrWs& w, int o0, int n, int c, double (*buf)[RR_STAGE]) {
  const int nt = ol_cloud_tiles(n);
  const long long tb = ol_tile_base(o0, c);
  double s = 0.0;
  for (int base = 0; base < nt; base += RR_STAGE) {
    if ((int)threadIdx.x < RR_STAGE && base + (int)threadIdx.x < nt) {
#pragma unroll
      for (int k = 0; k < K; ++k) buf[k][threadIdx.x] = w.part[(size_t)k * w.tiles + tb + base + threadIdx.x];
    }
    __syncthreads();
    if (threadIdx.x < K) {
      const int m = nt - base < RR_STAGE ? nt - base : RR_STAGE;
#pragma unroll 8
      for (int j = 0; j < m; ++j) s = ol_add(s, buf[threadIdx.x][j]);
    }
    __syncthreads();
  }
  return s;
}

// The accepted pairs of segment c: the tiles' counts, integers in any order.  Valid in thread 0.
__device__ static inline int rr_cloud_count(const RrWs& w, int o0, int n, int c, int* sh) {
  const int nt = ol_cloud_tiles(n);
  const int* tcount = w.tcount + ol_tile_base(o0, c);
  int s = 0;
  for (int t = threadIdx.x; t < nt; t += RR_LANES) s += tcount[t];
  s = pn_wave_sum_i(s);
  if (pn_lane() == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// ---- means: pbar, qbar and m of every running segment ---------------------------------------------------------------------
__global__ __launch_bounds__(RR_LANES) void pn_register_mean_kernel(const int* __restrict__ off_s, int totalS, RrWs w) {
  __shared__ double buf[RR_SUMS_MEAN][RR_STAGE];
  __shared__ int shc[OL_WAVES];
  const int c = blockIdx.x;
  if (w.stop[c]) return;
  const int o0 = off_s[c], o1 = off_s[c + 1];
  const int n = rg_valid_segment(o0, o1, totalS) ? o1 - o0 : 0;
  const int m = rr_cloud_count(w, o0, n, c, shc);
  const double s = rr_cloud_sum<RR_SUMS_MEAN>(w, o0, n, c, buf);
  if (threadIdx.x == 0) w.m[c] = m;
  if (threadIdx.x < RR_SUMS_MEAN) w.mean[RR_SUMS_MEAN * (size_t)c + threadIdx.x] = rr_mean(s, m);
}

// ---- solve: the step of every running segment and its stop flag -------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(RR_LANES) void pn_register_solve_kernel(const int* __restrict__ off_s, int totalS, RrArgs a,
                                                                     int it, RrWs w, int32_t* __restrict__ iterations,
                                                                     int32_t* __restrict__ status) {
  constexpr int K = MODE == RR_PLANE ? RR_SUMS_PLANE : RR_SUMS_POINT;
  __shared__ double buf[K][RR_STAGE];
  __shared__ double sums[K];
  const int c = blockIdx.x;
  if (w.stop[c]) return;
  const int o0 = off_s[c], o1 = off_s[c + 1];
  const int n = rg_valid_segment(o0, o1, totalS) ? o1 - o0 : 0;
  const double s = rr_cloud_sum<K>(w, o0, n, c, buf);
  if (threadIdx.x < K) sums[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* sp = w.state + RR_STATE * (size_t)c;
  RrState st = rr_load_state(sp);
  const int stop = rr_step(MODE, (int)w.q.g.flag[c], w.m[c], w.mean + RR_SUMS_MEAN * (size_t)c, sums, a.tol_rot,
                           a.tol_trans, RR_SWEEPS, &st);
  sp[0] = st.q[0], sp[1] = st.q[1], sp[2] = st.q[2], sp[3] = st.q[3];
  sp[4] = st.t[0], sp[5] = st.t[1], sp[6] = st.t[2];
  iterations[c] = it;
  if (stop != RR_RUNNING) {
    status[c] = stop;
    w.stop[c] = 1u;
  }
}

// ---- outputs: transform, count and rmse of every segment --------------------------------------------------------------------
__global__ __launch_bounds__(RR_LANES) void pn_register_out_kernel(const int* __restrict__ off_s, int totalS, RrWs w,
                                                                   double* __restrict__ transform,
                                                                   int32_t* __restrict__ count,
                                                                   double* __restrict__ rmse) {
  __shared__ double buf[1][RR_STAGE];
  __shared__ int shc[OL_WAVES];
  const int c = blockIdx.x;
  const int o0 = off_s[c], o1 = off_s[c + 1];
  const int n = rg_valid_segment(o0, o1, totalS) ? o1 - o0 : 0;
  const int m = rr_cloud_count(w, o0, n, c, shc);
  const double s = rr_cloud_sum<1>(w, o0, n, c, buf);
  if (threadIdx.x != 0) return;
  rr_matrix(rr_load_state(w.state + RR_STATE * (size_t)c), transform + 16 * (size_t)c);
  count[c] = m;
  rmse[c] = rr_rmse(s, m);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
extern "C" int pn_register_launches(int max_iter) { return rr_launches(max_iter); }

extern "C" long long pn_register_workspace_bytes(long long totalS, long long totalT, int S) {
  if (totalS < 0 || totalT < 0 || S < 0 || totalS >= (1ll << 31) || totalT >= (1ll << 31)) return 0;
  RrWs w;
  return rr_carve(nullptr, totalS, totalT, S, &w) + 16;
}

// Move, bin and search: the launches of one pairing.  stop: the flags, or null for the final evaluation.
static int rr_pair_launch(const float* src, const int* off_s, int totalS, const int* off_t, int totalT, int S, int ppc,
                          int bin, const RrWs& w, const uint32_t* stop, int32_t* idx, float* dist, hipStream_t stream) {
  if (totalS == 0) return PN_OK;
  const int row_blocks = pn_cdiv(totalS, 256);
  {
    PN_PROF("register_move", stream);
    hipLaunchKernelGGL(pn_register_move_kernel<false>, dim3(row_blocks), dim3(256), 0, stream, src, off_s, S, totalS,
                       (const double*)w.state, stop, w.moved);
  }
  PN_PROF("register_search", stream);      // the two memsets and the query's launches
  PN_CHECK_HIP(hipMemsetAsync(w.q.qord, 0xff, (size_t)4 * totalS, stream));
  PN_CHECK_HIP(hipMemsetAsync(w.q.qstart, 0, (size_t)4 * ((size_t)totalT + 2 * (size_t)S), stream));
  hipLaunchKernelGGL(pn_knn3_query_cells_kernel<true>, dim3(row_blocks), dim3(256), 0, stream, (const float*)w.moved,
                     off_t, off_s, S, totalT, totalS, 1, ppc, bin, w.q, idx, dist, stop);
  if (totalT == 0) return PN_OK;
  if (bin) {
    hipLaunchKernelGGL(pn_knn3_grid_scan_kernel, dim3(S), dim3(1024), 0, stream, off_t, off_s, totalT, ppc, w.q.g,
                       w.q.qstart);
    hipLaunchKernelGGL(pn_knn3_query_scatter_kernel, dim3(row_blocks), dim3(256), 0, stream, off_t, off_s, S, totalS,
                       w.q);
  }
  hipLaunchKernelGGL(pn_knn3_query_search_kernel, dim3(pn_cdiv(totalS, 4)), dim3(256), 0, stream, (const float*)w.moved,
                     off_t, off_s, S, totalT, totalS, 1, ppc, w.q, idx, dist, stop);
  return PN_OK;
}

extern "C" int pn_register_f32(const float* src, const int* off_s, int totalS, const float* tgt, const int* off_t,
                               int totalT, const float* normals, int S, int mode, float max_dist, int max_iter,
                               double tol_rot, double tol_trans, const double* init, double* transform,
                               int32_t* iterations, int32_t* status, int32_t* count, double* rmse, int32_t* idx,
                               float* dist, void* ws, long long ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "pn_register_f32";
  PN_CHECK_ARG(S >= 0 && totalS >= 0 && totalT >= 0, "%s: S=%d totalS=%d totalT=%d", who, S, totalS, totalT);
  PN_CHECK_ARG(mode == RR_POINT || mode == RR_PLANE, "%s: mode=%d (0: point to point, 1: point to plane)", who, mode);
  PN_CHECK_ARG(mode == RR_POINT || normals, "%s: mode=1 needs the target's normals", who);
  PN_CHECK_ARG(max_iter >= 1 && max_iter <= RR_MAX_ITERATIONS, "%s: max_iter=%d (1 .. %d)", who, max_iter,
               RR_MAX_ITERATIONS);
  PN_CHECK_ARG(max_dist >= 0.0f, "%s: max_dist=%g (>= 0, +inf accepts every pair)", who, (double)max_dist);
  PN_CHECK_ARG(tol_rot >= 0.0 && tol_trans >= 0.0, "%s: tol_rot=%g tol_trans=%g (>= 0)", who, tol_rot, tol_trans);
  if (S == 0) return PN_OK;
  PN_CHECK_ARG((src || totalS == 0) && off_s && (tgt || totalT == 0) && off_t && transform && iterations && status &&
                   count && rmse && ws,
               "%s: null pointer (src, off_s, tgt, off_t, transform, iterations, status, count, rmse and ws are required)",
               who);
  PN_CHECK_ARG(ws_bytes >= pn_register_workspace_bytes(totalS, totalT, S), "%s: workspace of %lld bytes (%lld)", who,
               ws_bytes, pn_register_workspace_bytes(totalS, totalT, S));
  RrWs w;
  rr_carve((void*)pn_align_up((size_t)ws, 16), totalS, totalT, S, &w);
  const int ppc = kg_ppc(), bin = kq_bin();
  const RrArgs a = {mode, max_dist, tol_rot, tol_trans};
  const dim3 block(RR_LANES), tiles((unsigned)w.tiles), clouds((unsigned)S);
  PN_PROF("register", stream);
  if (totalT > 0) {
    const int rc = kg_build_launch(tgt, off_t, S, totalT, ppc, w.q.g, stream);
    if (rc != PN_OK) return rc;
  } else {
    PN_CHECK_HIP(hipMemsetAsync(w.q.g.flag, 0, (size_t)4 * S, stream));
  }
  hipLaunchKernelGGL(pn_register_init_kernel, tiles, block, 0, stream, off_s, S, totalS, init, w, iterations, status);
  for (int it = 1; it <= max_iter; ++it) {
    const int rc = rr_pair_launch(src, off_s, totalS, off_t, totalT, S, ppc, bin, w, w.stop, w.idx, w.dist, stream);
    if (rc != PN_OK) return rc;
    {
      PN_PROF("register_sums", stream);
      if (mode == RR_PLANE)      // (the mode decides which pairs are accepted: a pair with a non-finite normal is not)
        hipLaunchKernelGGL((pn_register_sums_kernel<0, RR_PLANE>), tiles, block, 0, stream, off_s, tgt, off_t, totalT,
                           normals, max_dist, w, (const int32_t*)w.idx, (const float*)w.dist);
      else
        hipLaunchKernelGGL((pn_register_sums_kernel<0, RR_POINT>), tiles, block, 0, stream, off_s, tgt, off_t, totalT,
                           normals, max_dist, w, (const int32_t*)w.idx, (const float*)w.dist);
    }
    {
      PN_PROF("register_solve", stream);
      hipLaunchKernelGGL(pn_register_mean_kernel, clouds, block, 0, stream, off_s, totalS, w);
    }
    {
      PN_PROF("register_sums", stream);
      if (mode == RR_PLANE)
        hipLaunchKernelGGL((pn_register_sums_kernel<1, RR_PLANE>), tiles, block, 0, stream, off_s, tgt, off_t, totalT,
                           normals, max_dist, w, (const int32_t*)w.idx, (const float*)w.dist);
      else
        hipLaunchKernelGGL((pn_register_sums_kernel<1, RR_POINT>), tiles, block, 0, stream, off_s, tgt, off_t, totalT,
                           normals, max_dist, w, (const int32_t*)w.idx, (const float*)w.dist);
    }
    {
      PN_PROF("register_solve", stream);
      if (mode == RR_PLANE)
        hipLaunchKernelGGL(pn_register_solve_kernel<RR_PLANE>, clouds, block, 0, stream, off_s, totalS, a, it, w,
                           iterations, status);
      else
        hipLaunchKernelGGL(pn_register_solve_kernel<RR_POINT>, clouds, block, 0, stream, off_s, totalS, a, it, w,
                           iterations, status);
    }
  }
  int32_t* fidx = idx ? idx : w.idx;
  float* fdist = dist ? dist : w.dist;
  const int rc = rr_pair_launch(src, off_s, totalS, off_t, totalT, S, ppc, bin, w, nullptr, fidx, fdist, stream);
  if (rc != PN_OK) return rc;
  if (mode == RR_PLANE)
    hipLaunchKernelGGL((pn_register_sums_kernel<2, RR_PLANE>), tiles, block, 0, stream, off_s, tgt, off_t, totalT, normals,
                       max_dist, w, (const int32_t*)fidx, (const float*)fdist);
  else
    hipLaunchKernelGGL((pn_register_sums_kernel<2, RR_POINT>), tiles, block, 0, stream, off_s, tgt, off_t, totalT, normals,
                       max_dist, w, (const int32_t*)fidx, (const float*)fdist);
  hipLaunchKernelGGL(pn_register_out_kernel, clouds, block, 0, stream, off_s, totalS, w, transform, count, rmse);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

extern "C" int pn_rigid_apply_f32(const float* src, const int* off_s, int S, int totalS, const double* transform,
                                  float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "pn_rigid_apply_f32";
  PN_CHECK_ARG(S >= 0 && totalS >= 0, "%s: S=%d totalS=%d", who, S, totalS);
  if (S == 0 || totalS == 0) return PN_OK;
  PN_CHECK_ARG(src && off_s && transform && out, "%s: null pointer", who);
  PN_PROF("rigid_apply", stream);
  hipLaunchKernelGGL(pn_register_move_kernel<true>, dim3(pn_cdiv(totalS, 256)), dim3(256), 0, stream, src, off_s, S,
                     totalS, transform, (const uint32_t*)nullptr, out);
  PN_CHECK_LAUNCH();
  return PN_OK;
}
