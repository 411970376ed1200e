// Mean-shift iterations at embedding widths W = 32 and 64 (bf16 x 3 arithmetic, dense launches).
//
// Same mathematics, outputs and pass structure as the 128-wide kernels of meanshift_x3.h:
//   forward      s_ij = clamp((q_i . x_j - 1) / b^2, -75, 75), K_ij = exp(s_ij), r_i = sum_j K_ij,
//                u_i = (sum_j K_ij x_j) / r_i, n_i = ||u_i||, y_i = u_i / n_i
//   backward     gu_i = (gy_i - y_i (y_i . gy_i)) / n_i, c_i = gu_i . u_i, alpha_i = 1 / (r_i b^2),
//                gs_ij = K_ij (gu_i . x_j - c_i) alpha_i (0 where the clamp is active),
//                row pass     gq_i  = sum_j gs_ij x_j
//                column pass  gX_j += sum_i (gs_ij q_i + K_ij gu_i / r_i)
// with every product formed from the six significant piece products of the error-free three-way
// bf16 split (split_common.h) on v_mfma_f32_32x32x16_bf16: fp32 dot products in another summation
// order.  The N x N matrix never exists: 32-point tiles of the streamed operand go through LDS, and
// both GEMMs of a (resident 32 rows, streamed tile) pair run on the matrix cores.
//
// What differs from the 128-wide code is sized for the narrower rows:
//  * A tile image holds the streamed rows TWICE, row-major for the first GEMM (contraction over the
//    channels) and transposed for the second (contraction over the streamed points), both pre-split:
//      row part  [piece 3][row j 32][W/8 chunks of 8 channels], chunk c of row j at c ^ swz(j)
//      transposed part [piece 3][k-step t 2][half h 2][channel f W] x 8 points: element e is point
//        (e & 3) + 8 (2 t + (e >> 2)) + 4 h — the order in which the D layout of the first GEMM hands
//        the kernel values to the second one as its B operand.
//    Both operands of both GEMMs are then plain 16-byte LDS reads of consecutive lanes; the image is
//    24 W 16-byte units (24 KiB at W = 64, 12 KiB at W = 32), as much as ONE 128-wide image or half.
//  * Eight waves (two per SIMD) in every pass: the resident operands of a 32-row wave are 12 W / 16
//    registers, so even the row pass with its two resident operands stays below 256 registers.
//  * Images are fetched with ordinary vector loads one tile ahead (into registers during the GEMMs of
//    the current tile, into the other LDS buffer behind them): one barrier per tile.
// Partial results of the column slices are combined in slice order by separate launches: no
// floating-point atomics, bit-identical results from run to run.  Rows >= N of a tail tile are zero
// image rows (they add nothing in the second GEMM) and their K is masked out of the row sums.
//
// KIND (compile time) selects the kernel profile of the elementwise stage between the two GEMMs:
//   MSW_GAUSS  the above;
//   MSW_EPA    Epanechnikov: with dist_ij = 2 - 2 q_i . x_j, K_ij = max(0, 0.75 (1 - dist_ij / b^2)), no clamp,
//              and, dK/d(q.x) being 1.5 / b^2 on the support and 0 off it,
//              gs_ij = K_ij > 0 ? 1.5 (gu_i . x_j - c_i) alpha_i : 0.
// Everything else (r, u, n, y, gu, c, alpha, the K / r_i weight of the GU term, images, slices, combines)
// is shared.  A row without support has r_i = 0 and comes out non-finite, as in the reference.
#include "split_common.h"

#define MSW_LOG2E 1.4426950408889634f
#define MSW_LIM2 (75.0f * MSW_LOG2E)
#define MSW_WAVES 8
#define MSW_THREADS (64 * MSW_WAVES)
#define MSW_ROWS (32 * MSW_WAVES)       // resident rows of a workgroup
#define MSW_MAX_SLICES 8
#define MSW_GAUSS 0
#define MSW_EPA 1

typedef float mswf16 __attribute__((ext_vector_type(16)));

#define MSW_MFMA(ACC, A, B) ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, ACC, 0, 0, 0)

template <int W>
struct MswImg {
  static constexpr int NCH = W / 8;            // 16-byte chunks per row and piece
  static constexpr int ROW_U4 = 32 * NCH;      // one piece of the row part
  static constexpr int TR_U4 = 4 * W;          // one piece of the transposed part
  static constexpr int TR_OFF = 3 * ROW_U4;
  static constexpr int IMG_U4 = 3 * ROW_U4 + 3 * TR_U4;   // = 24 W
  // eight consecutive rows read the same chunk number in one ds_read_b128 service group: spread
  // them over the eight 16-byte columns of 128 bytes (one row at W = 64, two rows at W = 32)
  __host__ __device__ static inline int swz(int j) { return (j / (8 / NCH)) & (NCH - 1); }
};

// 32 rows of W floats in LDS (rows >= N zero) -> the tile image at P
template <int W>
__device__ static inline void msw_write_image(const float* tl, u32x4* __restrict__ P, int tid, int nthreads) {
  using I = MswImg<W>;
  for (int it = tid; it < 32 * I::NCH; it += nthreads) {
    const int j = it / I::NCH, c = it % I::NCH;
    const float4 v0 = *reinterpret_cast<const float4*>(tl + j * W + 8 * c);
    const float4 v1 = *reinterpret_cast<const float4*>(tl + j * W + 8 * c + 4);
    u32x4 h, m, l;
    X3_SPLIT_TO(v0.x, v0.y, h, m, l, 0);
    X3_SPLIT_TO(v0.z, v0.w, h, m, l, 1);
    X3_SPLIT_TO(v1.x, v1.y, h, m, l, 2);
    X3_SPLIT_TO(v1.z, v1.w, h, m, l, 3);
    const int slot = j * I::NCH + (c ^ I::swz(j));
    P[slot] = h;
    P[I::ROW_U4 + slot] = m;
    P[2 * I::ROW_U4 + slot] = l;
  }
  for (int it = tid; it < 4 * W; it += nthreads) {
    const int f = it % W, th = it / W;   // th = 2 t + h
    const int t = th >> 1, hh = th & 1;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = tl[((e & 3) + 8 * (2 * t + (e >> 2)) + 4 * hh) * W + f];
    u32x4 h, m, l;
    X3_SPLIT_TO(v[0], v[1], h, m, l, 0);
    X3_SPLIT_TO(v[2], v[3], h, m, l, 1);
    X3_SPLIT_TO(v[4], v[5], h, m, l, 2);
    X3_SPLIT_TO(v[6], v[7], h, m, l, 3);
    P[I::TR_OFF + it] = h;
    P[I::TR_OFF + I::TR_U4 + it] = m;
    P[I::TR_OFF + 2 * I::TR_U4 + it] = l;
  }
}

// x (B,N,W) -> the image of every 32-point tile.  One workgroup per tile.
template <int W>
__global__ __launch_bounds__(256) void pn_msw_split_kernel(const float* __restrict__ x, int N, int ntiles,
                                                           u32x4* __restrict__ pimg) {
  __shared__ __attribute__((aligned(16))) float tl[32 * W];
  const int b = blockIdx.y, tile = blockIdx.x, j0 = tile * 32;
  const float* __restrict__ xb = x + (size_t)b * N * W;
  for (int it = threadIdx.x; it < 32 * W / 4; it += 256) {
    const int j = it / (W / 4), c = it % (W / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j0 + j < N) v = *reinterpret_cast<const float4*>(xb + (size_t)(j0 + j) * W + 4 * c);
    *reinterpret_cast<float4*>(tl + j * W + 4 * c) = v;
  }
  __syncthreads();
  msw_write_image<W>(tl, pimg + ((size_t)b * ntiles + tile) * MswImg<W>::IMG_U4, threadIdx.x, 256);
}

// backward prologue, one workgroup per tile, one wave per row: gu, c, alpha of the tile's rows and
// the tile images of q and of gu
template <int W>
__global__ __launch_bounds__(256) void pn_msw_prologue_bwd_kernel(
    const float* __restrict__ gy, const float* __restrict__ y, const float* __restrict__ q,
    const float* __restrict__ rsum, const float* __restrict__ unorm, const float* __restrict__ bsq, int N, int ntiles,
    float* __restrict__ gu, float* __restrict__ cs, float* __restrict__ alpha, u32x4* __restrict__ img_q,
    u32x4* __restrict__ img_gu) {
  __shared__ __attribute__((aligned(16))) float tq[32 * W];
  __shared__ __attribute__((aligned(16))) float tg[32 * W];
  const int b = blockIdx.y, tile = blockIdx.x, j0 = tile * 32;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool on = lane < W;
  for (int r = wave; r < 32; r += 4) {
    const int i = j0 + r;
    float u0 = 0.f, q0 = 0.f;
    if (i < N) {   // (wave-uniform)
      const size_t base = ((size_t)b * N + i) * W;
      const float y0 = on ? y[base + lane] : 0.f;
      const float g0 = on ? gy[base + lane] : 0.f;
      q0 = on ? q[base + lane] : 0.f;
      const float nn = unorm[(size_t)b * N + i], rr = rsum[(size_t)b * N + i];
      const float yg = pn_wave_sum(y0 * g0);
      u0 = (g0 - y0 * yg) / nn;
      const float c = pn_wave_sum(u0 * (y0 * nn));
      if (on) gu[base + lane] = u0;
      if (lane == 0) {
        cs[(size_t)b * N + i] = c;
        alpha[(size_t)b * N + i] = 1.0f / (rr * bsq[b]);
      }
    }
    if (on) {
      tq[r * W + lane] = q0;
      tg[r * W + lane] = u0;
    }
  }
  __syncthreads();
  const size_t off = ((size_t)b * ntiles + tile) * MswImg<W>::IMG_U4;
  msw_write_image<W>(tq, img_q + off, threadIdx.x, 256);
  msw_write_image<W>(tg, img_gu + off, threadIdx.x, 256);
}

// PASS 0 forward       resident rows Q;      streamed X:      out[f][i] += X[j][f] K
// PASS 1 backward/rows resident rows Q, GU;  streamed X:      out[f][i] += X[j][f] gs
// PASS 2 backward/cols resident cols X;      streamed Q, GU:  out[f][j] += Q[i][f] gs + GU[i][f] K / r_i
// R, R1   (B,N,W) fp32 resident operands (split in registers once per workgroup)
// PA, PB  tile images of the streamed operand(s) (PB: GU, PASS 2 only)
// cs, rs  per-row c_i and alpha_i: of the resident row (PASS 1) / of the streamed rows (PASS 2)
// grid (slices, blocks of 256 resident indices, B), 512 threads: wave w owns rows 32 w .. 32 w + 31.
template <int W, int PASS, int KIND>
__global__ __launch_bounds__(MSW_THREADS) void pn_msw_kernel(
    const float* __restrict__ R, const float* __restrict__ R1, const u32x4* __restrict__ PA,
    const u32x4* __restrict__ PB, const float* __restrict__ cs, const float* __restrict__ rs,
    const float* __restrict__ bsq_, int N, int ntiles, int tiles_per_slice, float* __restrict__ opart,
    float* __restrict__ rpart) {
  using I = MswImg<W>;
  constexpr int KS = W / 16, FB = W / 32, NIMG = PASS == 2 ? 2 : 1, IMG = I::IMG_U4;
  constexpr int PER = (IMG + MSW_THREADS - 1) / MSW_THREADS;
  constexpr int NR1 = PASS == 1 ? KS : 1;
  __shared__ __attribute__((aligned(16))) u32x4 ldsP[2][NIMG][IMG];
  __shared__ float lds_sc[2][64];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, col = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, rblk = blockIdx.y, slice = blockIdx.x, S = gridDim.x;
  const int t_begin = slice * tiles_per_slice;
  const int t_end = min(ntiles, t_begin + tiles_per_slice);
  const int i0 = (rblk * MSW_WAVES + wave) * 32;
  const bool wave_on = i0 < N;
  const float bsqv = bsq_[b];
  const float hl = (0.5f / bsqv) * MSW_LOG2E;
  const float ib = 1.0f / bsqv;   // (MSW_EPA)
  const size_t bN = (size_t)b * N;
  const u32x4* __restrict__ PAb = PA + (size_t)b * ntiles * IMG;
  const u32x4* __restrict__ PBb = PASS == 2 ? PB + (size_t)b * ntiles * IMG : nullptr;

  // the image(s) of a tile: global -> registers (MSW_FETCH), registers -> LDS buffer (MSW_PUT)
  u32x4 pre[NIMG][PER];
  float pre_sc = 0.f;
#define MSW_FETCH(MT)                                                                   \
  {                                                                                     \
    _Pragma("unroll") for (int u = 0; u < PER; ++u) {                                   \
      const int idx = tid + MSW_THREADS * u;                                            \
      if (IMG % MSW_THREADS == 0 || idx < IMG) {                                        \
        pre[0][u] = PAb[(size_t)(MT) * IMG + idx];                                      \
        if (PASS == 2) pre[NIMG - 1][u] = PBb[(size_t)(MT) * IMG + idx];                \
      }                                                                                 \
    }                                                                                   \
    if (PASS == 2 && tid < 64) { /* c_i | alpha_i of the 32 streamed rows */            \
      const int jc = min((MT) * 32 + (tid & 31), N - 1);                                \
      pre_sc = (tid < 32 ? cs : rs)[bN + jc];                                           \
    }                                                                                   \
  }
#define MSW_PUT(BUF)                                                                    \
  {                                                                                     \
    _Pragma("unroll") for (int u = 0; u < PER; ++u) {                                   \
      const int idx = tid + MSW_THREADS * u;                                            \
      if (IMG % MSW_THREADS == 0 || idx < IMG) {                                        \
        ldsP[BUF][0][idx] = pre[0][u];                                                  \
        if (PASS == 2) ldsP[BUF][NIMG - 1][idx] = pre[NIMG - 1][u];                     \
      }                                                                                 \
    }                                                                                   \
    if (PASS == 2 && tid < 64) lds_sc[BUF][tid] = pre_sc;                               \
  }
  if (t_begin < t_end) MSW_FETCH(t_begin);

  // resident operand(s) as B operands of the first GEMM: k-step s = channels 16 s + 8 h + e
  const int ires = min(i0 + col, N - 1);
  bf16x8 qh[KS], qm[KS], ql[KS];
  bf16x8 uh[NR1], um[NR1], ul[NR1];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    {
      const float* src = R + (bN + ires) * W + 16 * s + 8 * h;
      const float4 a = *reinterpret_cast<const float4*>(src);
      const float4 c = *reinterpret_cast<const float4*>(src + 4);
      u32x4 vh, vm, vl;
      X3_SPLIT_TO(a.x, a.y, vh, vm, vl, 0);
      X3_SPLIT_TO(a.z, a.w, vh, vm, vl, 1);
      X3_SPLIT_TO(c.x, c.y, vh, vm, vl, 2);
      X3_SPLIT_TO(c.z, c.w, vh, vm, vl, 3);
      qh[s] = x3_as_bf16(vh);
      qm[s] = x3_as_bf16(vm);
      ql[s] = x3_as_bf16(vl);
    }
    if (PASS == 1) {
      const float* src = R1 + (bN + ires) * W + 16 * s + 8 * h;
      const float4 a = *reinterpret_cast<const float4*>(src);
      const float4 c = *reinterpret_cast<const float4*>(src + 4);
      u32x4 vh, vm, vl;
      X3_SPLIT_TO(a.x, a.y, vh, vm, vl, 0);
      X3_SPLIT_TO(a.z, a.w, vh, vm, vl, 1);
      X3_SPLIT_TO(c.x, c.y, vh, vm, vl, 2);
      X3_SPLIT_TO(c.z, c.w, vh, vm, vl, 3);
      uh[PASS == 1 ? s : 0] = x3_as_bf16(vh);
      um[PASS == 1 ? s : 0] = x3_as_bf16(vm);
      ul[PASS == 1 ? s : 0] = x3_as_bf16(vl);
    }
  }
  float c_res = 0.f, a_res = 0.f;
  if (PASS == 1) {
    c_res = cs[bN + ires];
    a_res = rs[bN + ires];
  }
  mswf16 acc_o[FB];
#pragma unroll
  for (int fb = 0; fb < FB; ++fb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_o[fb][r] = 0.f;
  float rsum = 0.f;

  if (t_begin < t_end) MSW_PUT(0);
  int cur = 0;
  for (int mt = t_begin; mt < t_end; ++mt) {
    const int j0 = mt * 32;
    __syncthreads();   // the image(s) of tile mt are in ldsP[cur]; every wave is done with tile mt - 1
    const bool more = mt + 1 < t_end;
    if (more) MSW_FETCH(mt + 1);
    if (wave_on) {
      // ---- first GEMM: S[streamed][resident] (and T with the second operand) ----
      mswf16 sa, ta;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sa[r] = 0.f;
        ta[r] = 0.f;
      }
      const u32x4* __restrict__ lp = ldsP[cur][0];
      const u32x4* __restrict__ lp1 = ldsP[cur][NIMG - 1];
      const int rowoff = col * I::NCH, sw = I::swz(col);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int slot = rowoff + ((2 * s + h) ^ sw);
        const bf16x8 ah = x3_as_bf16(lp[slot]);
        const bf16x8 am = x3_as_bf16(lp[I::ROW_U4 + slot]);
        const bf16x8 al = x3_as_bf16(lp[2 * I::ROW_U4 + slot]);
        // small terms first
        MSW_MFMA(sa, al, qh[s]);
        MSW_MFMA(sa, ah, ql[s]);
        MSW_MFMA(sa, am, qm[s]);
        MSW_MFMA(sa, am, qh[s]);
        MSW_MFMA(sa, ah, qm[s]);
        MSW_MFMA(sa, ah, qh[s]);
        if (PASS == 1) {  // T = X . GU: same streamed operand, second resident one
          const int z = PASS == 1 ? s : 0;
          MSW_MFMA(ta, al, uh[z]);
          MSW_MFMA(ta, ah, ul[z]);
          MSW_MFMA(ta, am, um[z]);
          MSW_MFMA(ta, am, uh[z]);
          MSW_MFMA(ta, ah, um[z]);
          MSW_MFMA(ta, ah, uh[z]);
        }
        if (PASS == 2) {  // T = GU . X: second streamed operand, same resident one
          const bf16x8 gh = x3_as_bf16(lp1[slot]);
          const bf16x8 gm = x3_as_bf16(lp1[I::ROW_U4 + slot]);
          const bf16x8 gl = x3_as_bf16(lp1[2 * I::ROW_U4 + slot]);
          MSW_MFMA(ta, gl, qh[s]);
          MSW_MFMA(ta, gh, ql[s]);
          MSW_MFMA(ta, gm, qm[s]);
          MSW_MFMA(ta, gm, qh[s]);
          MSW_MFMA(ta, gh, qm[s]);
          MSW_MFMA(ta, gh, qh[s]);
        }
      }
      // ---- elementwise stage on D[streamed = (r&3) + 8 (r>>2) + 4 h][resident = col] ----
      float kv[16], gs[PASS == 0 ? 1 : 16];
      const bool tail = j0 + 32 > N;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float dist = __builtin_fmaf(-2.0f, sa[r], 2.0f);
        float k, a2 = 0.f, a2c = 0.f;
        if constexpr (KIND == MSW_EPA) {
          k = fmaxf(0.0f, 0.75f * __builtin_fmaf(-dist, ib, 1.0f));
        } else {
          a2 = -dist * hl;
          a2c = __builtin_amdgcn_fmed3f(a2, -MSW_LIM2, MSW_LIM2);
          k = __builtin_amdgcn_exp2f(a2c);
        }
        if (PASS == 0) {
          // padded points have all-zero image rows: they add nothing in the second GEMM whatever
          // their weight, so only the row sums need the mask
          if (tail && j0 + row >= N) k = 0.f;
          kv[r] = k;
          rsum += k;
        } else {
          const float cc = PASS == 1 ? c_res : lds_sc[cur][row];
          const float aa = PASS == 1 ? a_res : lds_sc[cur][32 + row];
          if constexpr (KIND == MSW_EPA) {   // dK/d(q.x) = 1.5 / b^2 on the support, 0 off it
            const float g = 1.5f * ((ta[r] - cc) * aa);
            gs[PASS == 0 ? 0 : r] = k > 0.0f ? g : 0.f;
          } else {
            const float g = k * ((ta[r] - cc) * aa);
            gs[PASS == 0 ? 0 : r] = a2c == a2 ? g : 0.f;
          }
          kv[r] = PASS == 2 ? k * (aa * bsqv) : k;   // weight of the GU term: K / r_i
        }
      }
      // ---- second GEMM: out[f][resident] += sum_streamed C[f][streamed] w[streamed][resident];
      //      k-step t = D registers 8 t .. 8 t + 7 of the first GEMM ----
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        u32x4 wh, wm, wl, vh, vm, vl;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = 8 * t + 2 * q;
          if (PASS == 0) {
            X3_SPLIT_TO(kv[e], kv[e + 1], wh, wm, wl, q);
          } else {
            X3_SPLIT_TO(gs[PASS == 0 ? 0 : e], gs[PASS == 0 ? 0 : e + 1], wh, wm, wl, q);
            if (PASS == 2) X3_SPLIT_TO(kv[e], kv[e + 1], vh, vm, vl, q);
          }
        }
        const bf16x8 bh = x3_as_bf16(wh), bm = x3_as_bf16(wm), bl = x3_as_bf16(wl);
#pragma unroll
        for (int fb = 0; fb < FB; ++fb) {
          const int tslot = I::TR_OFF + (2 * t + h) * W + fb * 32 + col;
          const bf16x8 xh = x3_as_bf16(lp[tslot]);
          const bf16x8 xm = x3_as_bf16(lp[I::TR_U4 + tslot]);
          const bf16x8 xl = x3_as_bf16(lp[2 * I::TR_U4 + tslot]);
          MSW_MFMA(acc_o[fb], xl, bh);
          MSW_MFMA(acc_o[fb], xh, bl);
          MSW_MFMA(acc_o[fb], xm, bm);
          MSW_MFMA(acc_o[fb], xm, bh);
          MSW_MFMA(acc_o[fb], xh, bm);
          MSW_MFMA(acc_o[fb], xh, bh);
          if (PASS == 2) {
            const bf16x8 kh = x3_as_bf16(vh), km = x3_as_bf16(vm), kl = x3_as_bf16(vl);
            const bf16x8 oh = x3_as_bf16(lp1[tslot]);
            const bf16x8 om = x3_as_bf16(lp1[I::TR_U4 + tslot]);
            const bf16x8 ol = x3_as_bf16(lp1[2 * I::TR_U4 + tslot]);
            MSW_MFMA(acc_o[fb], ol, kh);
            MSW_MFMA(acc_o[fb], oh, kl);
            MSW_MFMA(acc_o[fb], om, km);
            MSW_MFMA(acc_o[fb], om, kh);
            MSW_MFMA(acc_o[fb], oh, km);
            MSW_MFMA(acc_o[fb], oh, kh);
          }
        }
      }
    }
    if (more) MSW_PUT(cur ^ 1);   // (its last readers passed this tile's barrier)
    cur ^= 1;
  }
#undef MSW_FETCH
#undef MSW_PUT
  const int ir = i0 + col;
  if (wave_on && ir < N) {
    float* o = opart + (((size_t)b * S + slice) * N + ir) * W;
#pragma unroll
    for (int fb = 0; fb < FB; ++fb)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(o + fb * 32 + 8 * g + 4 * h) =
            make_float4(acc_o[fb][4 * g], acc_o[fb][4 * g + 1], acc_o[fb][4 * g + 2], acc_o[fb][4 * g + 3]);
  }
  if (PASS == 0) {
    rsum += __shfl_xor(rsum, 32, 64);
    if (wave_on && h == 0 && ir < N) rpart[((size_t)b * S + slice) * N + ir] = rsum;
  }
}

// partial results of the slices, in slice order -> y, rsum, unorm.  One wave per row.
template <int W>
__global__ __launch_bounds__(256) void pn_msw_combine_fwd_kernel(
    const float* __restrict__ opart, const float* __restrict__ rpart, const float* __restrict__ q, int N, int S,
    float* __restrict__ y, float* __restrict__ rsum, float* __restrict__ unorm) {
  const int b = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + wave;
  if (i >= N) return;
  const bool on = lane < W;
  float o0 = 0.f, r = 0.f;
  for (int s = 0; s < S; ++s) {
    if (on) o0 += opart[(((size_t)b * S + s) * N + i) * W + lane];
    r += rpart[((size_t)b * S + s) * N + i];
  }
  const float D = 1.0f / r;
  const size_t base = ((size_t)b * N + i) * W;
  const float q0 = on ? q[base + lane] : 0.f;
  const float n0 = q0 + (o0 * D - q0);     // the reference's update, term by term
  const float nn = sqrtf(pn_wave_sum(n0 * n0));
  if (on) y[base + lane] = n0 / nn;
  if (lane == 0) {
    rsum[(size_t)b * N + i] = r;
    unorm[(size_t)b * N + i] = nn;
  }
}

// gq = sum of the row pass's slices; gx += sum of the column pass's slices (slice order)
__global__ __launch_bounds__(256) void pn_msw_combine_bwd_kernel(const float* __restrict__ opart_q,
                                                                 const float* __restrict__ opart_x, long long NW4,
                                                                 int S, float* __restrict__ gq,
                                                                 float* __restrict__ gx) {
  const int b = blockIdx.y;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= NW4) return;
  const float4* pq = reinterpret_cast<const float4*>(opart_q) + (size_t)b * S * NW4 + e;
  const float4* px = reinterpret_cast<const float4*>(opart_x) + (size_t)b * S * NW4 + e;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
  for (int s = 0; s < S; ++s) {
    const float4 u = pq[(size_t)s * NW4];
    a.x += u.x, a.y += u.y, a.z += u.z, a.w += u.w;
    const float4 v = px[(size_t)s * NW4];
    c.x += v.x, c.y += v.y, c.z += v.z, c.w += v.w;
  }
  reinterpret_cast<float4*>(gq)[(size_t)b * NW4 + e] = a;
  float4* g = reinterpret_cast<float4*>(gx) + (size_t)b * NW4 + e;
  float4 o = *g;
  o.x += c.x, o.y += c.y, o.z += c.z, o.w += c.w;
  *g = o;
}

// ---- host side ------------------------------------------------------------------------------
// Column slices of a launch: a function of (B, N) alone (256 compute units assumed whatever the
// device: the summation order, and with it the bits of the result, must not depend on the machine).
static int msw_slices(int B, int N, int* tps) {
  const int ntiles = pn_cdiv(N, 32);
  const long long rowblocks = (long long)B * pn_cdiv(N, MSW_ROWS);
  int best = 1;
  double best_score = -1.0;
  const int smax = ntiles / 8 < MSW_MAX_SLICES ? ntiles / 8 : MSW_MAX_SLICES;
  for (int S = 1; S <= smax; ++S) {
    const int t = pn_cdiv(ntiles, S);
    if (pn_cdiv(ntiles, t) != S) continue;   // every slice has tiles
    const double rounds = (double)(rowblocks * S) / 256.0;
    const double eff = rounds / (double)(long long)(rounds + 0.999999);
    // (a slice costs N x 4 W bytes of partial sums written and read back: the same trade as x3_slices)
    const double score = eff * (double)t / ((double)t + 1.5) - 0.01 * S;
    if (score > best_score) {
      best_score = score;
      best = S;
    }
  }
  *tps = pn_cdiv(ntiles, best);
  return best;
}

// workspace: [image of x | partial sums | forward: row-sum parts
//                                       | backward: column-pass parts, images of q and gu, gu, c, alpha]
struct MswLayout {
  int ntiles, S, tps;
  size_t img_x, opart, rpart, opart_x, img_q, img_gu, gu, cs, total;
};
static MswLayout msw_layout(int B, int N, int W, int backward) {
  MswLayout L;
  L.ntiles = pn_cdiv(N, 32);
  L.S = msw_slices(B, N, &L.tps);
  const size_t img = pn_align_up((size_t)B * L.ntiles * 24 * W * 16, 256);
  const size_t part = pn_align_up((size_t)B * L.S * N * W * sizeof(float), 256);
  size_t o = 0;
  L.img_x = o, o += img;
  L.opart = o, o += part;
  L.rpart = L.opart_x = L.img_q = L.img_gu = L.gu = L.cs = 0;
  if (!backward) {
    L.rpart = o, o += pn_align_up((size_t)B * L.S * N * sizeof(float), 256);
  } else {
    L.opart_x = o, o += part;
    L.img_q = o, o += img;
    L.img_gu = o, o += img;
    L.gu = o, o += pn_align_up((size_t)B * N * W * sizeof(float), 256);
    L.cs = o, o += pn_align_up((size_t)2 * B * N * sizeof(float), 256);
  }
  L.total = o;
  return L;
}

static bool msw_width_ok(int D) { return D == 32 || D == 64; }

extern "C" size_t pn_meanshift_w_workspace(int B, int N, int D, int backward) {
  if (B <= 0 || N <= 0 || !msw_width_ok(D)) return 0;
  return msw_layout(B, N, D, backward).total;
}

template <int W, int KIND>
static int msw_fwd(const float* q, const float* x, const float* bsq, int B, int N, float* y, float* rsum,
                   float* unorm, char* ws, int reuse_image, hipStream_t stream) {
  const MswLayout L = msw_layout(B, N, W, 0);
  u32x4* img_x = (u32x4*)(ws + L.img_x);
  float* opart = (float*)(ws + L.opart);
  float* rpart = (float*)(ws + L.rpart);
  if (!reuse_image) {
    hipLaunchKernelGGL((pn_msw_split_kernel<W>), dim3(L.ntiles, B), dim3(256), 0, stream, x, N, L.ntiles, img_x);
    PN_CHECK_LAUNCH();
  }
  {
    PN_PROF("meanshift_w_fwd", stream);
    hipLaunchKernelGGL((pn_msw_kernel<W, 0, KIND>), dim3(L.S, pn_cdiv(N, MSW_ROWS), B), dim3(MSW_THREADS), 0, stream, q,
                       (const float*)nullptr, (const u32x4*)img_x, (const u32x4*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, bsq, N, L.ntiles, L.tps, opart, rpart);
  }
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL((pn_msw_combine_fwd_kernel<W>), dim3(pn_cdiv(N, 4), B), dim3(256), 0, stream,
                     (const float*)opart, (const float*)rpart, q, N, L.S, y, rsum, unorm);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

template <int W, int KIND>
static int msw_bwd(const float* gy, const float* y, const float* q, const float* x, const float* rsum,
                   const float* unorm, const float* bsq, int B, int N, float* gq, float* gx, char* ws,
                   int reuse_image, hipStream_t stream) {
  const MswLayout L = msw_layout(B, N, W, 1);
  u32x4* img_x = (u32x4*)(ws + L.img_x);
  u32x4* img_q = (u32x4*)(ws + L.img_q);
  u32x4* img_gu = (u32x4*)(ws + L.img_gu);
  float* opart_q = (float*)(ws + L.opart);
  float* opart_x = (float*)(ws + L.opart_x);
  float* gu = (float*)(ws + L.gu);
  float* cs = (float*)(ws + L.cs);
  float* alpha = cs + (size_t)B * N;
  if (!reuse_image) {
    hipLaunchKernelGGL((pn_msw_split_kernel<W>), dim3(L.ntiles, B), dim3(256), 0, stream, x, N, L.ntiles, img_x);
    PN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL((pn_msw_prologue_bwd_kernel<W>), dim3(L.ntiles, B), dim3(256), 0, stream, gy, y, q, rsum, unorm,
                     bsq, N, L.ntiles, gu, cs, alpha, img_q, img_gu);
  PN_CHECK_LAUNCH();
  const dim3 grid(L.S, pn_cdiv(N, MSW_ROWS), B);
  {
    PN_PROF("meanshift_w_bwd_rows", stream);
    hipLaunchKernelGGL((pn_msw_kernel<W, 1, KIND>), grid, dim3(MSW_THREADS), 0, stream, q, (const float*)gu,
                       (const u32x4*)img_x, (const u32x4*)nullptr, (const float*)cs, (const float*)alpha, bsq, N,
                       L.ntiles, L.tps, opart_q, (float*)nullptr);
  }
  PN_CHECK_LAUNCH();
  {
    PN_PROF("meanshift_w_bwd_cols", stream);
    hipLaunchKernelGGL((pn_msw_kernel<W, 2, KIND>), grid, dim3(MSW_THREADS), 0, stream, x, (const float*)nullptr,
                       (const u32x4*)img_q, (const u32x4*)img_gu, (const float*)cs, (const float*)alpha, bsq, N,
                       L.ntiles, L.tps, opart_x, (float*)nullptr);
  }
  PN_CHECK_LAUNCH();
  const long long NW4 = (long long)N * W / 4;
  hipLaunchKernelGGL(pn_msw_combine_bwd_kernel, dim3(pn_cdiv(NW4, 256), B), dim3(256), 0, stream,
                     (const float*)opart_q, (const float*)opart_x, NW4, L.S, gq, gx);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

static bool msw_kind_ok(int kind) { return kind == MSW_GAUSS || kind == MSW_EPA; }

// One forward iteration at D = 32 or 64.  q, x (B,N,D) (q: the current iterate, x: the data), bsq (B);
// writes y (B,N,D), rsum, unorm (B,N).  workspace: pn_meanshift_w_workspace(B, N, D, 0) bytes;
// reuse_image != 0: it already holds the tile images of this x (an earlier call with the same
// workspace, i.e. the previous iteration of the same clustering call).  kind: the kernel profile,
// 0 Gaussian / 1 Epanechnikov (the images and the workspace do not depend on it).
extern "C" int pn_meanshift_w_iter_fwd_kind_f32(const float* q, const float* x, const float* bsq, int B, int N,
                                                int D, float* y, float* rsum, float* unorm, void* workspace,
                                                size_t workspace_bytes, int reuse_image, int kind, void* stream) {
  PN_CHECK_ARG(q && x && bsq && y && rsum && unorm && workspace, "pn_meanshift_w_iter_fwd: null pointer");
  PN_CHECK_ARG(B > 0 && N > 0, "pn_meanshift_w_iter_fwd: empty input");
  PN_CHECK_ARG(msw_width_ok(D), "pn_meanshift_w: embedding size %d unsupported (32 or 64; pad narrower rows with zeros)", D);
  PN_CHECK_ARG(msw_kind_ok(kind), "pn_meanshift_w: kernel kind %d unknown (0 Gaussian, 1 Epanechnikov)", kind);
  if (workspace_bytes < pn_meanshift_w_workspace(B, N, D, 0)) {
    pn_set_error("pn_meanshift_w_iter_fwd: workspace of %zu bytes, %zu needed", workspace_bytes,
                 pn_meanshift_w_workspace(B, N, D, 0));
    return PN_ERR_WORKSPACE;
  }
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (kind == MSW_EPA)
    return D == 32 ? msw_fwd<32, MSW_EPA>(q, x, bsq, B, N, y, rsum, unorm, ws, reuse_image, st)
                   : msw_fwd<64, MSW_EPA>(q, x, bsq, B, N, y, rsum, unorm, ws, reuse_image, st);
  return D == 32 ? msw_fwd<32, MSW_GAUSS>(q, x, bsq, B, N, y, rsum, unorm, ws, reuse_image, st)
                 : msw_fwd<64, MSW_GAUSS>(q, x, bsq, B, N, y, rsum, unorm, ws, reuse_image, st);
}

// ... with the Gaussian kernel
extern "C" int pn_meanshift_w_iter_fwd_f32(const float* q, const float* x, const float* bsq, int B, int N, int D,
                                           float* y, float* rsum, float* unorm, void* workspace,
                                           size_t workspace_bytes, int reuse_image, void* stream) {
  return pn_meanshift_w_iter_fwd_kind_f32(q, x, bsq, B, N, D, y, rsum, unorm, workspace, workspace_bytes,
                                          reuse_image, MSW_GAUSS, stream);
}

// Backward of that iteration (recomputes K): gy = dL/dy, (y, rsum, unorm) the iteration's saved
// outputs, q its input iterate.  Writes gq = dL/dq (B,N,D) and ADDS the iteration's contribution to
// dL/dx into gx.  workspace: pn_meanshift_w_workspace(B, N, D, 1) bytes; reuse_image, kind as above.
extern "C" int pn_meanshift_w_iter_bwd_kind_f32(const float* gy, const float* y, const float* q, const float* x,
                                                const float* rsum, const float* unorm, const float* bsq, int B,
                                                int N, int D, float* gq, float* gx, void* workspace,
                                                size_t workspace_bytes, int reuse_image, int kind, void* stream) {
  PN_CHECK_ARG(gy && y && q && x && rsum && unorm && bsq && gq && gx && workspace,
               "pn_meanshift_w_iter_bwd: null pointer");
  PN_CHECK_ARG(B > 0 && N > 0, "pn_meanshift_w_iter_bwd: empty input");
  PN_CHECK_ARG(msw_width_ok(D), "pn_meanshift_w: embedding size %d unsupported (32 or 64; pad narrower rows with zeros)", D);
  PN_CHECK_ARG(msw_kind_ok(kind), "pn_meanshift_w: kernel kind %d unknown (0 Gaussian, 1 Epanechnikov)", kind);
  if (workspace_bytes < pn_meanshift_w_workspace(B, N, D, 1)) {
    pn_set_error("pn_meanshift_w_iter_bwd: workspace of %zu bytes, %zu needed", workspace_bytes,
                 pn_meanshift_w_workspace(B, N, D, 1));
    return PN_ERR_WORKSPACE;
  }
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (kind == MSW_EPA)
    return D == 32 ? msw_bwd<32, MSW_EPA>(gy, y, q, x, rsum, unorm, bsq, B, N, gq, gx, ws, reuse_image, st)
                   : msw_bwd<64, MSW_EPA>(gy, y, q, x, rsum, unorm, bsq, B, N, gq, gx, ws, reuse_image, st);
  return D == 32 ? msw_bwd<32, MSW_GAUSS>(gy, y, q, x, rsum, unorm, bsq, B, N, gq, gx, ws, reuse_image, st)
                 : msw_bwd<64, MSW_GAUSS>(gy, y, q, x, rsum, unorm, bsq, B, N, gq, gx, ws, reuse_image, st);
}

extern "C" int pn_meanshift_w_iter_bwd_f32(const float* gy, const float* y, const float* q, const float* x,
                                           const float* rsum, const float* unorm, const float* bsq, int B, int N,
                                           int D, float* gq, float* gx, void* workspace, size_t workspace_bytes,
                                           int reuse_image, void* stream) {
  return pn_meanshift_w_iter_bwd_kind_f32(gy, y, q, x, rsum, unorm, bsq, B, N, D, gq, gx, workspace,
                                          workspace_bytes, reuse_image, MSW_GAUSS, stream);
}
