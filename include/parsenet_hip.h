/* parsenet_hip.h — C ABI of the MI355X (gfx950) ParSeNet hot-path library.
 *
 * The reference (Hippogriff/parsenet-codebase) is pure Python on PyTorch: it has no FFI
 * of its own, so every entry point below replaces a *composition of stock torch ops*
 * inside one reference function (cited as file:line, paths relative to the upstream
 * repository).  The binding a maintainer adds is a ctypes stub — see INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers + sizes only; all pointers are DEVICE pointers unless named h_*;
 *   - every tensor is dense row-major ("contiguous") in the stated shape;
 *   - floating data is fp32, index data is int64 (torch defaults), unless stated;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on it;
 *   - buffers are caller-owned; scratch space is passed in, its size queried with the
 *     matching pn_*_workspace();
 *   - return value 0 = success, negative = error (PN_ERR_*); pn_last_error() returns a
 *     thread-local description.  Functions are re-entrant and keep no global state.
 */
#ifndef PARSENET_HIP_H
#define PARSENET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* pn_abi_version() of the library this header describes; it changes with every change of a declaration below */
#define PN_ABI_VERSION 23

#define PN_OK 0
#define PN_ERR_ARG (-1)
#define PN_ERR_HIP (-2)
#define PN_ERR_WORKSPACE (-3)
#define PN_ERR_UNSUPPORTED (-4)

const char* pn_last_error(void);
int pn_abi_version(void);

/* ---- per-kernel timing (HIP events on the launch stream; off by default) -----------
 * enable(1) brackets every kernel family launched through this library with an event pair;
 * count() resolves outstanding events and returns the number of families seen; get(i, ...)
 * returns name, accumulated milliseconds and number of launches; reset() clears. */
void pn_prof_enable(int on);
void pn_prof_reset(void);
int pn_prof_count(void);
int pn_prof_get(int i, char* name, int name_len, double* total_ms, long long* calls);

/* ---- kNN graph ------------------------------------------------------------------
 * pn_knn_f32 replaces src/model.py:9-22 knn(x,k) and src/PointNet.py:9-26 knn(x,k1,k2)
 * (k1 == k2; a dilation k2 > k1 is a strided slice of the k2 result done by the caller);
 * pn_knn_pn_f32 replaces src/PointNet.py:29-69 knn_points_normals (rows 0:3 xyz, 3:6 unit
 * normals, metric |dp|^2 * (1 + (2 - 2 ni.nj))).
 * x (B,C,N) channel-first.  idx (B,N,k): for every point the k candidates with the LARGEST
 * negated distance, best first, the point itself included; equal values -> smaller index.
 * Arithmetic: dot products / squared norms are channel-ordered fp32 fma chains, combined as
 * (-xx[j] - (-2*dot)) - xx[i] like the reference, every step rounded to fp32.
 * Limits: 1 <= k <= 128, k <= N. */
size_t pn_knn_workspace(int B, int C, int N, int k);
int pn_knn_f32(const float* x, int B, int C, int N, int k, int64_t* idx, void* workspace,
               size_t workspace_bytes, void* stream);
int pn_knn_pn_f32(const float* x6, int B, int N, int k, int64_t* idx, void* workspace,
                  size_t workspace_bytes, void* stream);
/* The same graph with int32 indices — the form the library's own edge-conv kernels consume
 * (pn_edgeconv_reduce_fwd_i32, pn_edgeconv_bwd_i32: half the index bytes of the torch dtype the
 * reference's topk returns, src/model.py:19).  metric 0: feature space (pn_knn_f32), 1: points +
 * normals (pn_knn_pn_f32, C = 6).  k <= 16 (the SplineNets' graphs, src/model.py:9-22 with k = 10)
 * takes ONE distance pass with the k best candidates of a lane in registers (csrc/knn_smallk.h);
 * same workspace query. */
int pn_knn_graph_i32(const float* x, int B, int C, int N, int k, int metric, int32_t* idx,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- neighbours of 3-D points from coordinate differences (evaluation-mode fitting) ----------
 * Replaces the broadcast difference + topk of src/fitting_utils.py:150-164, 202-237
 * (up_sample_points_torch(_in_range): k = 5) and the KD-tree search behind open3d's
 * remove_statistical_outlier (src/fitting_utils.py:704-710: k = 20, float64) for a RAGGED batch of
 * segments: pts (total,3) fp32, off (S+1) int32 row offsets, max_n >= the largest segment.
 * d = ((dx^2 + dy^2) + dz^2), each operation rounded once (f64 = 1: in float64 on the fp32 points).
 * idx (total,k) int32 indices LOCAL to the segment, nearest first, the point itself first, equal
 * distances -> smaller index; a segment with fewer than k points is padded with the point itself.
 * dist (total,k) float / double (per f64) or NULL: the Euclidean distances of those neighbours.
 * Limits: k <= 64; segments up to 10 240 points (float64: 5 120). */
int pn_knn3_ragged(const float* pts, const int* off, int S, int max_n, int k, int f64, int32_t* idx,
                   void* dist, void* stream);

/* ---- dot-product selection between two point sets ------------------------------------
 * Replaces src/mean_shift.py:125-137 (compute_bandwidth: 2 - 2 X X^T, topk(K, largest=False),
 * the K-th smallest distance per row) and :146-149 (nms: argmin over centres of 2 - 2 C X^T).
 * 2 - 2*dot is an exact decreasing map of dot for unit vectors, so both are selections on the
 * dot products.  q (B,Nq,C), c (B,Nc,C) point-major.  Exactly one of out_idx (B,Nq,k) int64
 * (indices of the k largest dots, best first, ties -> smaller index, k <= 128) and out_val
 * (B,Nq) fp32 (the k-th largest dot, k <= 512) is non-NULL.  flags (B,Nq) int32 is set to 1
 * for queries whose result is invalid (survivor overflow on massively tied data): the caller
 * recomputes those rows.  PN_ERR_UNSUPPORTED if the shape is outside the fast path
 * (needs Nc/16 >= 2k and C <= 256); pn_dot_select_workspace then returns 0. */
size_t pn_dot_select_workspace(int B, int C, int Nq, int Nc, int k, int want_value);
int pn_dot_select_f32(const float* q, int Nq, const float* c, int Nc, int B, int C, int k,
                      int64_t* out_idx, float* out_val, int* flags, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- mean-shift iterations ----------------------------------------------------------
 * Replaces src/mean_shift.py:45-79 (mean_shift_, gaussian kernel) and the autograd graph the
 * reference keeps through it.  All tensors point-major (B,N,D) with D = 128; bsq (B) = b^2.
 *   slices   : upper bound S of the column slices the launches use for (B,N) (sizes the scratch).
 *   pack     : x (B,N,D) -> xt (B,D,Np), Np = N rounded up to 64, zero padded.
 *   iter_fwd : y = normalise(q + ((K X) / rowsum(K) - q)), K = exp(clamp(-(2 - 2 q x^T)/b^2/2)).
 *              Scratch opart (B,S,N,D), rpart (B,S,N).  Saves rsum, unorm (B,N).
 *   iter_bwd : given gy = dL/dy: gq = dL/dq (overwritten), gx += this iteration's contribution
 *              to dL/dx (recomputes K; nothing of size N x N is stored).
 *              Scratch gu, go (B,N,D), cs (B,2,N), qt, gut (B,D,Np), opart_q, opart_x (B,S,N,D). */
int pn_meanshift_slices(int B, int N);
int pn_meanshift_pack_f32(const float* x, int B, int N, int D, float* xt, void* stream);
int pn_meanshift_iter_fwd_f32(const float* q, const float* x, const float* xt, const float* bsq,
                              int B, int N, int D, float* opart, float* rpart, float* y,
                              float* rsum, float* unorm, void* stream);
int pn_meanshift_iter_bwd_f32(const float* gy, const float* y, const float* q, const float* x,
                              const float* xt, const float* rsum, const float* unorm,
                              const float* bsq, int B, int N, int D, float* gu, float* go,
                              float* cs, float* qt, float* gut, float* opart_q, float* opart_x,
                              float* gq, float* gx, void* stream);

/* ---- mean-shift, fp32-grade products on the bf16 matrix cores ("bf16 x 3") ---------------
 * Same contract and outputs as the entry points above; every fp32 operand is split without
 * error into three bf16 pieces and each product is formed from the six significant piece
 * products with fp32 accumulation (an fp32 dot product in a different summation order).
 *   image_bytes : size of one tile-image array for (B,N).
 *   split       : x (B,N,D) -> img (pre-split, LDS-ready image of every 32-point tile; both
 *                 GEMMs read it, the second one through the hardware transpose read).
 *   iter_fwd    : as pn_meanshift_iter_fwd_f32 with img_x in place of (x, xt).
 *   iter_bwd    : as pn_meanshift_iter_bwd_f32 with img_x in place of xt and two scratch image
 *                 arrays (images of q and gu) in place of (go, qt, gut). */
size_t pn_meanshift_x3_image_bytes(int B, int N);
int pn_meanshift_x3_split_f32(const float* x, int B, int N, int D, void* img, void* stream);
int pn_meanshift_x3_iter_fwd_f32(const float* q, const void* img_x, const float* bsq, int B, int N,
                                 int D, float* opart, float* rpart, float* y, float* rsum,
                                 float* unorm, void* stream);
int pn_meanshift_x3_iter_bwd_f32(const float* gy, const float* y, const float* q, const float* x,
                                 const void* img_x, const float* rsum, const float* unorm,
                                 const float* bsq, int B, int N, int D, float* gu, float* cs,
                                 void* img_q, void* img_gu, float* opart_q, float* opart_x, float* gq,
                                 float* gx, void* stream);

/* ---- mean-shift at embedding widths D = 32 and 64 (csrc/meanshift_w.hip) -------------------
 * The same iteration and its recompute backward in bf16 x 3 arithmetic, dense launches only, for
 * narrower embeddings (rows narrower than 32 / 64 are zero-padded by the caller: zero columns are
 * exact in every product and stay zero through the renormalisation).  All scratch lives in ONE
 * caller-allocated workspace.
 *   workspace : bytes needed for (B,N,D); backward != 0: for iter_bwd.  0 for an unsupported shape.
 *   iter_fwd  : q (B,N,D) the current iterate, x (B,N,D) the data, bsq (B) -> y (B,N,D), rsum,
 *               unorm (B,N), as pn_meanshift_iter_fwd_f32.
 *   iter_bwd  : gy = dL/dy -> gq = dL/dq (overwritten), gx += the iteration's contribution to dL/dx.
 *   reuse_image != 0: the workspace still holds the tile images of this x from an earlier call
 *               (the iterations of one clustering call share x); 0: they are rebuilt first.
 * No atomics: partial sums are combined in a fixed order, results are bit-reproducible. */
size_t pn_meanshift_w_workspace(int B, int N, int D, int backward);
int pn_meanshift_w_iter_fwd_f32(const float* q, const float* x, const float* bsq, int B, int N, int D,
                                float* y, float* rsum, float* unorm, void* workspace,
                                size_t workspace_bytes, int reuse_image, void* stream);
int pn_meanshift_w_iter_bwd_f32(const float* gy, const float* y, const float* q, const float* x,
                                const float* rsum, const float* unorm, const float* bsq, int B, int N,
                                int D, float* gq, float* gx, void* workspace, size_t workspace_bytes,
                                int reuse_image, void* stream);

/* ---- mean-shift with the kernel profile as an argument ---------------------------------------
 * The entry points above with one more argument, `kind` (before `stream`): the kernel_type of
 * src/mean_shift.py:45-79.  The two profiles differ in the elementwise stage between the two GEMMs
 * of a tile pair only; images, workspaces, scratch sizes, slices and outputs are the same.
 *   PN_MS_KERNEL_GAUSSIAN      K = exp(clamp(-(2 - 2 q x^T) / b^2 / 2, -75, 75)): exactly the calls above.
 *   PN_MS_KERNEL_EPANECHNIKOV  K = max(0, 3/4 (1 - (2 - 2 q x^T) / b^2)) (src/mean_shift.py:64-68); in the
 *                              backward dK is 3/2 / b^2 on the support and 0 off it.  A row without
 *                              support has row sum 0 and comes out non-finite, as in the reference.
 * The 128-wide calls take the `plan` of the _plan_ variants; block-sparse plans bound the tail of the
 * exponential, so a call with kind != PN_MS_KERNEL_GAUSSIAN and plan != NULL is refused
 * (PN_ERR_UNSUPPORTED, nothing is launched).  Any other kind: PN_ERR_ARG. */
#define PN_MS_KERNEL_GAUSSIAN 0
#define PN_MS_KERNEL_EPANECHNIKOV 1
int pn_meanshift_w_iter_fwd_kind_f32(const float* q, const float* x, const float* bsq, int B, int N, int D,
                                     float* y, float* rsum, float* unorm, void* workspace,
                                     size_t workspace_bytes, int reuse_image, int kind, void* stream);
int pn_meanshift_w_iter_bwd_kind_f32(const float* gy, const float* y, const float* q, const float* x,
                                     const float* rsum, const float* unorm, const float* bsq, int B, int N,
                                     int D, float* gq, float* gx, void* workspace, size_t workspace_bytes,
                                     int reuse_image, int kind, void* stream);
int pn_meanshift_x3_iter_fwd_kind_f32(const float* q, const void* img_x, const float* bsq, int B, int N,
                                      int D, float* opart, float* rpart, float* y, float* rsum,
                                      float* unorm, const void* plan, int kind, void* stream);
int pn_meanshift_x3_iter_bwd_kind_f32(const float* gy, const float* y, const float* q, const float* x,
                                      const void* img_x, const float* rsum, const float* unorm,
                                      const float* bsq, int B, int N, int D, float* gu, float* cs,
                                      void* img_q, void* img_gu, float* opart_q, float* opart_x, float* gq,
                                      float* gx, const void* plan, int kind, void* stream);

/* Block-sparse variant.  K_ij = exp((q_i . x_j - 1) / b^2) of src/mean_shift.py:58-64 decays fast
 * on a clustered embedding; the (32-row tile of q) x (32-row tile of x) pairs a plan skips are
 * chosen, from rigorous bounds on the tiles' bounding caps on the unit sphere, such that for EVERY
 * row of q all skipped terms together stay below rel_eps of that row's sum (the caller's choice;
 * the host side uses 1e-6, below the rounding of an fp32 sum of N terms) — the result is the dense
 * one to fp32 noise.  Per q cap A: L_A = lower bound of its rows' best dot product, R_A = sum over
 * the data caps B of n_B exp((Lo_AB - L_A) / b^2) (n_B rows, Lo_AB <= every dot product of the
 * pair) bounds every row sum from below by exp((L_A - 1) / b^2) R_A, and the data caps with the
 * smallest upper bounds U_AB are dropped as long as sum n_B exp((U_AB - L_A) / b^2) <= rel_eps R_A.
 * The caller orders the points so that tiles are local (any order is valid; mean-shift is
 * permutation-equivariant).
 *   tileinfo : z (B,N,D) unit rows -> two bounding caps per tile (its rows dealt to two far-apart
 *              seeds): cen (B,T,2,D) normalised means, rho (B,T,2) angular radii (+1e-3 slack;
 *              < 0: empty cap), cnt (B,T,2) rows per cap (may be NULL), T = align_up(N,64)/32.
 *   plan     : caps of the iterate q and of the data x (cntX: the data caps' row counts; NULL: one
 *              row per non-empty cap in R, 32 in the dropped mass — rigorous, keeps more pairs)
 *              -> plan (pn_meanshift_x3_plan_bytes), N <= 32768:
 *              the pair predicate (T x T bytes), per resident block of each pass the compact
 *              list of streamed tiles with at least one pair set, and the prefix sums of the list
 *              lengths (the launches cut the concatenated lists into one equal range per CU).
 *   iter_fwd_plan / iter_bwd_plan : as iter_fwd / iter_bwd, skipping what the plan of THIS
 *              iteration excludes (plan == NULL: dense; the backward must get the forward's plan).
 *   chain_order : sim (B,P,P) similarities of P = 128 cell centres -> rank (B,P) int32, the position
 *              of every cell in the greedy nearest-neighbour chain from cell 0 (the order the
 *              caller lays the cells, hence the points, out in: neighbours in the sequence are
 *              neighbours on the sphere).  Only a heuristic for locality; never affects results.
 */
int pn_meanshift_chain_order_f32(const float* sim, int B, int P, int* rank, void* stream);
/* Executed work of the bf16 x 3 mean-shift launches, counted by the launches themselves: every wave
 * counts the (resident 32-row tile, streamed 32-row tile) pairs whose GEMMs it runs (all pairs in a
 * dense launch, the pairs the plan keeps in a planned one).  out3[0..2] = pairs executed by the
 * forward / row-pass / column-pass launches since the previous call; reading clears the counters
 * and synchronises with the device.  One pair is 2 * 32 * 32 * 128 FLOP per GEMM unit (2 / 3 / 4
 * units) x 6 piece products on the bf16 matrix cores. */
int pn_meanshift_x3_exec_tiles(unsigned long long* out3);
/* Nearest candidate of every query — arg-max_j xq_i . xc_j, the first step of MeanShift.nms
 * (src/mean_shift.py:146-149) — by EXACT pruning: xq, xc (B,N,D) unit rows in one common order that
 * keeps neighbours together (the locality order of the iterations), their tile caps from
 * pn_meanshift_x3_tileinfo_f32.  A candidate tile whose upper bound lies below the query tile's
 * guaranteed best cannot hold a maximum; only the remaining tile pairs are evaluated, as fp32 fma
 * chains over the channels in order (the arithmetic of pn_dot_select_f32, bit for bit).  perm (B,N)
 * position -> original index (NULL: identity): nearest (B,N) is indexed by the query's ORIGINAL
 * index and holds the candidate's ORIGINAL index, ties to the smaller one.  workspace:
 * pn_meanshift_x3_plan_bytes(B, N). */
int pn_meanshift_x3_nearest_f32(const float* xq, const float* xc, const float* cenQ, const float* rhoQ,
                                const float* cenC, const float* rhoC, const int64_t* perm, int B, int N, int D,
                                int64_t* nearest, void* workspace, size_t workspace_bytes, void* stream);
/* fp32-grade GEMM of the per-point layers (nn.Conv1d(kernel_size=1): src/model.py:56-180,
 * src/PointNet.py:143-289) on the bf16 matrix cores (csrc/gemm_x3.hip): operands split error-free into
 * three bf16 pieces, six piece products per fp32 product, fp32 accumulation.
 * pn_gemm_x3_weight_image_f32: the pre-split image of a weight W (M,K) row-major for y = W x
 * (transposed = 0) or of W^T for gx = W^T gy (transposed = 1; the image then belongs to a (K,M) operand);
 * img: pn_gemm_x3_weight_image_bytes(M, K) resp. (K, M) bytes.
 * pn_gemm_x3_f32: out (B,M,N) = A x (+ bias (M) or NULL), img_a the image of the (M,K) operand A,
 * x (B,K,N) channel-first; workspace: pn_gemm_x3_points_image_bytes(B, K, N) bytes. */
size_t pn_gemm_x3_weight_image_bytes(int M, int K);
size_t pn_gemm_x3_points_image_bytes(int B, int C, int N);
int pn_gemm_x3_weight_image_f32(const float* w, int M, int K, int transposed, void* img, void* stream);
int pn_gemm_x3_f32(const void* img_a, const float* x, const float* bias, int B, int M, int K, int N, float* out,
                   void* workspace, size_t workspace_bytes, void* stream);
/* pn_gemm_x3_cat_f32: the same product with the K input channels spread over nsrc <= 4 tensors xs[s] (B, cs[s], N)
 * (every cs[s] a multiple of 8, K = sum cs): W applied to the concatenation torch.cat builds in src/model.py:150
 * without writing it.  xs, cs: HOST arrays of nsrc device pointers / channel counts. */
int pn_gemm_x3_cat_f32(const void* img_a, const float* const* xs, const int* cs, int nsrc, const float* bias, int B,
                       int M, int N, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* The weight gradient of such a layer (what autograd's conv1d backward forms over the B N points:
 * src/model.py:157-176, src/PointNet.py:196-284 under loss.backward()): gw (M,K) = sum_b gy[b] (M,N) x[b]^T (N,K)
 * in the same arithmetic, split over the points with a FIXED-ORDER sum of the partial results (bit-reproducible,
 * no atomics); gb (M) or NULL: the bias gradient sum_b sum_n gy[b][m][n].  gy (B,M,N), x (B,K,N) channel-first;
 * workspace: pn_gemm_x3_wgrad_workspace(B, M, K, N) bytes. */
size_t pn_gemm_x3_wgrad_workspace(int B, int M, int K, int N);
int pn_gemm_x3_wgrad_f32(const float* gy, const float* x, int B, int M, int K, int N, float* gw, float* gb,
                         void* workspace, size_t workspace_bytes, void* stream);
/* Mean-shift backward restricted to R <= 64 rows per batch item (csrc/meanshift_rows.hip).  A step of
 * src/mean_shift.py:45-79 maps row i of the iterate to a function of that row and of the data alone, and
 * the training path reads the final iterate only at the cluster centres (src/mean_shift.py:36-43): the
 * gradient is zero outside those rows in every step on the way back.  One call = one step: gy, y, q
 * (B,R,D) are the R rows of the incoming gradient, of the step's result and of its input iterate, rsum,
 * unorm (B,R) the saved row sums and pre-normalisation norms of those rows, x (B,N,D) the data, bsq (B)
 * the squared bandwidths.  Writes gq (B,R,D), the gradient w.r.t. the input rows, and ADDS the step's
 * gradient w.r.t. the data into gx (B,N,D).  D in {32, 64, 128}.  No atomics.  workspace:
 * pn_meanshift_rows_bwd_workspace(B, N) bytes.
 * _kind_: the same with the kernel profile of the forward pass as an argument (before `stream`), as in the
 * _kind_ entry points above: PN_MS_KERNEL_GAUSSIAN is exactly pn_meanshift_rows_bwd_f32;
 * PN_MS_KERNEL_EPANECHNIKOV recomputes K = max(0, 3/4 (1 - (2 - 2 q x^T) / b^2)) with dK = 3/2 / b^2 on the
 * support and exactly 0 off it.  Same workspace, same launches.  Any other kind: PN_ERR_ARG. */
size_t pn_meanshift_rows_bwd_workspace(int B, int N);
int pn_meanshift_rows_bwd_f32(const float* gy, const float* y, const float* q, const float* rsum, const float* unorm,
                              const float* x, const float* bsq, int B, int N, int D, int R, float* gq, float* gx,
                              void* workspace, size_t workspace_bytes, void* stream);
int pn_meanshift_rows_bwd_kind_f32(const float* gy, const float* y, const float* q, const float* rsum,
                                   const float* unorm, const float* x, const float* bsq, int B, int N, int D, int R,
                                   float* gq, float* gx, void* workspace, size_t workspace_bytes, int kind,
                                   void* stream);
/* gx[b, rows[b,r], :] += g[b, r, :], r ascending (rows (B,R) int64 may repeat; entries outside [0, N)
 * are skipped): the first iterate of the mean-shift iterations IS the data. */
int pn_meanshift_rows_scatter_add_f32(const float* g, const int64_t* rows, int B, int N, int D, int R, float* gx,
                                      void* stream);
size_t pn_meanshift_x3_plan_bytes(int B, int N);
/* the part of a plan its consumers read (the rest is scratch of the plan call: plans of T iterations may be placed
 * core_bytes apart in one buffer of T * core + (plan_bytes - core) bytes) */
size_t pn_meanshift_x3_plan_core_bytes(int B, int N);
/* Spherical k-means steps of the locality order the block-sparse iterations run on (no counterpart in the
 * reference: mean-shift, src/mean_shift.py:45-79, is permutation-equivariant and the order is free).
 * x (B,N,128) unit rows, cen / old (B,K,128); lab (B,N) int32 = arg-max over the centres of the dot product
 * (ties -> the smaller centre); new centre = normalised sum of the cell's points in index order, the old
 * centre when the cell is empty.  Deterministic. */
int pn_kmeans_assign_f32(const float* x, const float* cen, int B, int N, int D, int K, int* lab, void* stream);
int pn_kmeans_centres_f32(const float* x, const int* lab, const float* old, int B, int N, int D, int K,
                          float* cen, void* stream);
/* The locality order itself (mean_shift.locality_order; no counterpart in the reference): perm (B,N) int64 = the
 * STABLE argsort of key[n] = rank[home[fine[n]]] * F + fine[n] — rank (B,P) int32 position of a coarse cell in the
 * chain, home (B,F) int32 coarse cell of a fine cell, fine (B,N) int32 fine cell of a point — as a counting sort
 * over the F <= 768 cells, one launch.  Identical to the tensor library's argsort(stable=True) of the keys. */
int pn_cell_order_i32(const int* rank, const int* home, const int* fine, int B, int N, int P, int F,
                      long long* perm, void* stream);
int pn_meanshift_x3_tileinfo_f32(const float* z, int B, int N, int D, float* cen, float* rho, float* cnt,
                                 void* stream);
int pn_meanshift_x3_plan_f32(const float* cenQ, const float* rhoQ, const float* cenX, const float* rhoX,
                             const float* cntX, const float* bsq, int B, int N, float rel_eps, void* plan,
                             void* stream);
int pn_meanshift_x3_iter_fwd_plan_f32(const float* q, const void* img_x, const float* bsq, int B, int N,
                                      int D, float* opart, float* rpart, float* y, float* rsum,
                                      float* unorm, const void* plan, void* stream);
/* the same, and the bounding caps of the result's tiles (what pn_meanshift_x3_tileinfo_f32 of y returns:
 * the q caps of the NEXT iteration's plan) out of the launch that combines the partial results; cen / rho
 * NULL: exactly pn_meanshift_x3_iter_fwd_plan_f32.  src/mean_shift.py:58-64, one iteration. */
int pn_meanshift_x3_iter_fwd_info_f32(const float* q, const void* img_x, const float* bsq, int B, int N,
                                      int D, float* opart, float* rpart, float* y, float* rsum,
                                      float* unorm, const void* plan, float* cen, float* rho, float* cnt,
                                      void* stream);
int pn_meanshift_x3_iter_bwd_plan_f32(const float* gy, const float* y, const float* q, const float* x,
                                      const void* img_x, const float* rsum, const float* unorm,
                                      const float* bsq, int B, int N, int D, float* gu, float* cs,
                                      void* img_q, void* img_gu, float* opart_q, float* opart_x,
                                      float* gq, float* gx, const void* plan, void* stream);

/* K-th largest dot product of every query row with both distance passes in bf16 x 3 arithmetic
 * (error-free operand split on the bf16 matrix cores, fp32 accumulate: fp32-grade values, not the
 * fma chain of pn_dot_select_f32) — the bandwidth statistic of src/mean_shift.py:125-137 under the
 * default mean-shift arithmetic.  q (B,Nq,C), c (B,Nc,C) point-major; workspace and flags as
 * pn_dot_select_f32 with want_value; PN_ERR_UNSUPPORTED outside C <= 128, Nc >= 2048. */
int pn_dot_kth_x3_f32(const float* q, int Nq, const float* c, int Nc, int B, int C, int k, float* out_val,
                      int* flags, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K-th largest dot product between unit vectors, fp16 x 2 matrix-core passes -----------
 * The bandwidth statistic of src/mean_shift.py:125-137 only needs the VALUE of the K-th nearest
 * neighbour (to 1e-5 after averaging): same engine as pn_dot_select_f32(out_val), with both
 * distance passes on the fp16 matrix cores (scaled fp16 x 2 split, |error| ~1e-7 on the dot
 * products).  q (B,Nq,128) unit rows; img_c = pn_meanshift_h2_split_f32 of the candidates
 * (B,Nc,128); workspace as pn_dot_select_workspace(B,128,Nq,Nc,k,1); flags as pn_dot_select_f32. */
int pn_dot_kth_unit_h2_f32(const float* q, int Nq, const void* img_c, int Nc, int B, int D, int k,
                           float* out_val, int* flags, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- mean-shift, fp32-grade products on the fp16 matrix cores ("fp16 x 2") ---------------
 * Same contract and outputs again; every operand is scaled by a power of two into the fp16
 * range and split into two fp16 pieces, each product is formed from the three significant
 * piece products with fp32 accumulation (error below that of an fp32 fma chain; see
 * csrc/meanshift_h2.h for the scaling rules).  Rows of x and of the iterates must be unit
 * vectors.  Entry points as the x3 ones; the backward takes ``rowsc`` (3 B N + B ntiles floats of
 * scratch, ntiles = 2 ceil(N / 64): per-row scalars and per-tile maxima) in place of ``cs``. */
size_t pn_meanshift_h2_image_bytes(int B, int N);
int pn_meanshift_h2_split_f32(const float* x, int B, int N, int D, void* img, void* stream);
int pn_meanshift_h2_iter_fwd_f32(const float* q, const void* img_x, const float* bsq, int B, int N,
                                 int D, float* opart, float* rpart, float* y, float* rsum,
                                 float* unorm, void* stream);
int pn_meanshift_h2_iter_bwd_f32(const float* gy, const float* y, const float* q, const float* x,
                                 const void* img_x, const float* rsum, const float* unorm,
                                 const float* bsq, int B, int N, int D, float* gu, float* rowsc,
                                 void* img_q, void* img_gu, float* opart_q, float* opart_x, float* gq,
                                 float* gx, void* stream);

/* ---- GroupNorm (+ReLU) (+max over points) of the per-point heads -------------------------
 * Replaces torch GroupNorm -> ReLU (-> max over N) of src/PointNet.py:216-218, 274-283 on
 * channel-first (B,C,N) tensors.  One block per (b,c) row.
 *   rows_fwd      : per-row sum and sum of squares (B,C); with rmax != NULL also the row maximum /
 *                   minimum and their positions (int32) for the max-over-N variant.
 *   group_moments : (B,groups) mean and rstd = 1/sqrt(var+eps) from the row sums (fp64 inside).
 *   apply_fwd     : out = [relu](gamma*(y-mean)*rstd + beta).
 *   rows_bwd      : ra = sum_n gz, rb = sum_n gz*yhat per row, gz = gout*[z>0] (or gout if !relu).
 *   group_bwd     : c1c2 (B,groups,2) = group means of gamma*gz and gamma*gz*yhat.
 *   apply_bwd     : dy = rstd*(gamma*gz - c1 - yhat*c2); with gsp/arg non-NULL gz is the sparse
 *                   gradient gsp (B,C) placed at position arg (B,C) of every row (gout ignored).
 * rowbias (NULL, or C floats with rb_bstride = 0: one value per channel, or B * C floats with rb_bstride = C: one per
 * (item, channel)): the four row kernels read y + rowbias[b * rb_bstride + c] — the preceding convolution's bias
 * (src/PointNet.py:196, 268-284) added at load instead of by a pass of its own; the same fp32 addition. */
int pn_gn_rows_fwd_f32(const float* y, int B, int C, int N, float* rsum, float* rsq, float* rmax,
                       int* amax, float* rmin, int* amin, const float* rowbias, int rb_bstride, void* stream);
int pn_gn_group_moments_f32(const float* rsum, const float* rsq, int B, int C, int groups, int N,
                            float eps, float* mean, float* rstd, void* stream);
int pn_gn_apply_fwd_f32(const float* y, const float* mean, const float* rstd, const float* gamma,
                        const float* beta, int B, int C, int groups, int N, int relu, float* out,
                        const float* rowbias, int rb_bstride, void* stream);
int pn_gn_rows_bwd_f32(const float* gout, const float* y, const float* mean, const float* rstd,
                       const float* gamma, const float* beta, int B, int C, int groups, int N,
                       int relu, float* ra, float* rb, const float* rowbias, int rb_bstride, void* stream);
/* The (B,C) tail of max_n relu(GroupNorm(y)) (src/PointNet.py:199-201: bnmlp1 + relu + max over the points, taken
 * on the row extrema): extremum by the sign of gamma, (ext - mean) * rstd, gamma * yhat + beta, relu — and of its
 * backward pass: gz = g * (z > 0), rb = gz * yhat.  The tensor-library operations they replace, separately rounded. */
int pn_gn_max_finish_f32(const float* rmax, const int* amax, const float* rmin, const int* amin,
                         const float* mean, const float* rstd, const float* gamma, const float* beta,
                         int B, int C, int groups, float* yhat, float* z, int* arg, float* out, void* stream);
int pn_gn_max_bwd_prep_f32(const float* g, const float* z, const float* yhat, int B, int C, float* gz, float* rb,
                           void* stream);
int pn_gn_group_bwd_f32(const float* ra, const float* rb, const float* gamma, int B, int C,
                        int groups, int N, float* c1c2, void* stream);
int pn_gn_apply_bwd_f32(const float* gout, const float* y, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, const float* c1c2, int B, int C,
                        int groups, int N, int relu, const float* gsp, const int* arg, float* dy,
                        const float* rowbias, int rb_bstride, void* stream);

/* ---- batched symmetric 3x3 eigen-decomposition (fp64) ---------------------------------
 * Serves the right singular vectors the primitive fits need (torch.svd of a tall n x 3 matrix in
 * src/fitting_utils.py:440 used by src/primitive_forward.py:725,794): they are the eigenvectors
 * of the 3x3 Gram matrix.  G (M,3,3) row-major -> evals (M,3) descending, evecs (M,3,3) with
 * eigenvectors in COLUMNS, each signed so that its largest-magnitude component is positive. */
int pn_sym3_eig_f64(const double* G, int M, double* evals, double* evecs, void* stream);

/* ---- layout helper: (B,R,C) -> (B,C,R) --------------------------------------------- */
int pn_transpose_f32(const float* in, float* out, int B, int R, int C, void* stream);

/* ---- edge features, API form ------------------------------------------------------
 * Replaces the gather + repeat + cat of src/model.py:25-53 (get_graph_feature) and
 * src/PointNet.py:72-103, :106-140.  xt (B,N,C) is the point-major copy of x (the
 * reference builds it with x.transpose(2,1).contiguous(), model.py:42); idx (B,N,k) are
 * per-item indices (the reference's idx_base offset is applied internally).
 * feat (B,N,k,2C): [x_j - x_i | x_i] — the memory behind the (B,2C,N,k) permuted view the
 * reference returns.  The backward reduces a gradient of that shape into gxt (B,N,C): it
 * transposes the kNN graph (sorted CSR by target point, built in `workspace` of
 * pn_edgeconv_bwd_workspace(B, N, k) bytes) and every row of gxt is summed by one wave in list
 * order — no floating-point atomics, bit-reproducible. */
int pn_edge_feature_fwd_f32(const float* xt, const int64_t* idx, int B, int N, int k, int C,
                            float* feat, void* stream);
int pn_edge_feature_bwd_f32(const float* gfeat, const int64_t* idx, int B, int N, int k, int C,
                            float* gxt, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused edge convolution ---------------------------------------------------------
 * Replaces get_graph_feature -> Conv2d 1x1 (no bias) -> GroupNorm / BatchNorm2d ->
 * LeakyReLU -> max over k of src/PointNet.py:157-165,180-191,203-214 and
 * src/model.py:75-86,146-159, without the (B,2C,N,k) tensor: the convolution is applied to
 * points (PQ = xt @ [Wa ; Wb-Wa]^T, a plain GEMM done by the caller), the edge stage reduces
 * y = P[idx] + Q over the k neighbours.
 *   reduce_fwd : PQ (B,N,2*Cout), idx (B,N,k), gamma (Cout; only its sign is used: max where
 *                gamma >= 0, min otherwise) -> yext, s1 = sum_k y (B,N,Cout) fp32, argk uint8
 *                (B,N,Cout), stats fp64 [(per_sample ? B : 1)][groups][2] = sum y, sum y^2
 *                (per-workgroup partials in `workspace`, combined in index order: no atomics).
 *                per_sample = 1: GroupNorm statistics; 0: BatchNorm statistics (groups = Cout).
 *   moments    : stats -> mean, rstd = 1/sqrt(var + eps) (fp32), n = number of groups in total.
 *   finalize   : out (B,Cout,N) = LeakyReLU(gamma*(yext-mean)*rstd + beta).
 *   bwd_prep   : gout (B,Cout,N) -> gz = gout * LeakyReLU'(z), yhat, both (B,N,Cout).
 *   bwd        : exact Group/BatchNorm gradient on every edge -> dPQ (B,N,2*Cout);
 *                t = gamma*gz, c1c2 fp32 [(per_sample?B:1)][groups][2] = group means of t and
 *                t*yhat over the edge activations; dense = 0 when the statistics were constants
 *                (eval-mode BatchNorm).  Both edge terms are evaluated by transposing the kNN
 *                graph (CSR by target point, lists sorted by (source, slot), built inside the
 *                call in `workspace`) and gathering rows of Q, t and argk: every dP row is summed
 *                by one wave in list order.  No floating-point atomics: two calls on the same
 *                inputs return the same bits (the reference on one device is deterministic). */
size_t pn_edgeconv_reduce_workspace(int B, int N, int Cout, int groups);
int pn_edgeconv_reduce_fwd_f32(const float* PQ, const int64_t* idx, const float* gamma, int B,
                               int N, int k, int Cout, int groups, int per_sample, float* yext,
                               uint8_t* argk, float* s1, double* stats, void* workspace,
                               size_t workspace_bytes, void* stream);
int pn_edgeconv_reduce_fwd_i32(const float* PQ, const int32_t* idx, const float* gamma, int B,
                               int N, int k, int Cout, int groups, int per_sample, float* yext,
                               uint8_t* argk, float* s1, double* stats, void* workspace,
                               size_t workspace_bytes, void* stream);
int pn_moments_f32(const double* stats, int n, double count, float eps, float* mean, float* rstd,
                   void* stream);
int pn_edgeconv_finalize_fwd_f32(const float* yext, const float* mean, const float* rstd,
                                 const float* gamma, const float* beta, int B, int N, int Cout,
                                 int groups, int per_sample, float slope, float* out,
                                 void* stream);
int pn_edgeconv_bwd_prep_f32(const float* gout, const float* yext, const float* mean,
                             const float* rstd, const float* gamma, const float* beta, int B,
                             int N, int Cout, int groups, int per_sample, float slope, float* gz,
                             float* yhat, void* stream);
size_t pn_edgeconv_bwd_workspace(int B, int N, int k);
int pn_edgeconv_bwd_f32(const float* PQ, const int64_t* idx, const float* t, const float* s1,
                        const uint8_t* argk, const float* mean, const float* rstd,
                        const float* c1c2, int B, int N, int k, int Cout, int groups,
                        int per_sample, int dense, float* dPQ, void* workspace,
                        size_t workspace_bytes, void* stream);
int pn_edgeconv_bwd_i32(const float* PQ, const int32_t* idx, const float* t, const float* s1,
                        const uint8_t* argk, const float* mean, const float* rstd,
                        const float* c1c2, int B, int N, int k, int Cout, int groups,
                        int per_sample, int dense, float* dPQ, void* workspace,
                        size_t workspace_bytes, void* stream);
/* The transposed graph is a function of idx alone: pn_edgeconv_csr_build writes it into a workspace of
 * pn_edgeconv_bwd_workspace(B, N, k) bytes (idx_is_i32: int32 / int64 indices) — e.g. during the forward pass, on a
 * side stream — and pn_edgeconv_bwd_prebuilt runs the backward on it (same kernels, same result). */
int pn_edgeconv_csr_build(const void* idx, int idx_is_i32, int B, int N, int k, void* workspace, size_t workspace_bytes,
                          void* stream);
int pn_edgeconv_bwd_prebuilt(const float* PQ, const void* idx, int idx_is_i32, const float* t, const float* s1,
                             const uint8_t* argk, const float* mean, const float* rstd, const float* c1c2, int B, int N,
                             int k, int Cout, int groups, int per_sample, int dense, float* dPQ, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- Chamfer nearest neighbour ---------------------------------------------------
 * Replaces the (M,N,3) broadcast + torch.min of src/utils.py:286-296 (chamfer_distance),
 * :313-323 (chamfer_distance_one_side), :338-358 (chamfer_distance_single_shape).
 * a (B,Na,3), b (B,Nb,3).  minA/argA (B,Na): squared distance to / index of the nearest
 * point of b for every point of a; minB/argB (B,Nb) the other way.  Any output pointer
 * may be NULL (a side whose two outputs are NULL is skipped).  Ties -> smallest index.
 * d = ((dx*dx + dy*dy) + dz*dz), each operation rounded to fp32. */
size_t pn_chamfer_nn_workspace(int B, int Na, int Nb);
int pn_chamfer_nn_f32(const float* a, const float* b, int B, int Na, int Nb, float* minA,
                      int64_t* argA, float* minB, int64_t* argB, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Ragged batch: item i is a[offA[i] .. offA[i+1]) against b[offB[i] .. offB[i+1]) of two
 * concatenated clouds (totalA / totalB rows; offsets: B+1 device ints; maxA / maxB = largest item,
 * used to size the grid).  Outputs are concatenated like the inputs, indices are local to the
 * item.  Used for the spline segments of a step (src/primitives.py:204-206: 900 | 930 samples
 * against a different number of ground-truth points per segment) in ONE launch per direction. */
size_t pn_chamfer_nn_ragged_workspace(int totalA, int totalB);
int pn_chamfer_nn_ragged_f32(const float* a, const int* offA, int totalA, int maxA, const float* b,
                             const int* offB, int totalB, int maxB, int B, float* minA,
                             int64_t* argA, float* minB, int64_t* argB, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Reduced two-sided distance of every item of the ragged batch and its backward (round 4):
 *   out[s] = (mean_i minA_i + mean_j minB_j) / 2      (src/utils.py:326-358, reduce=True)
 *   gpred[i] = (pred_i - gt[argA_i]) g_s / nA + sum_{j: argB_j = i} (pred_i - gt_j) g_s / nB
 * pred / minA / argA are concatenated over the items like the clouds (offA, offB: S+1 ints),
 * indices local to the item.  Fixed summation order, no atomics. */
int pn_chamfer_ragged_reduce_f32(const float* minA, const int* offA, const float* minB, const int* offB, int S,
                                 float* out, void* stream);
int pn_chamfer_ragged_bwd_f32(const float* pred, const int* offA, int maxA, const float* gt, const int* offB,
                              const int64_t* argA, const int64_t* argB, const float* g, int S, float* gpred,
                              void* stream);

/* Coverage figures of test.py:157-180 for S shapes at once: the squared nearest-neighbour minima of both sides
 * concatenated over the shapes (offA, offB: S+1 ints) -> out (S,6) float64, per side
 *   sum_i sqrtf(fmaxf(x_i, 1e-5f))   (guard_sqrt, the square root in fp32, the sum in fp64),
 *   #{i : that root < 0.01f},  #{i : that root < 0.02f}                  (fp32 comparisons);
 * columns 0-2 side A, 3-5 side B.  One workgroup per (shape, side); every thread adds a strided range in ascending
 * order, a fixed tree combines the 256 partial sums: no atomics, a shape's row depends on its own values only.  The
 * means, and cd, are the host's to form (float64). */
int pn_coverage_reduce_f32(const float* minA, const int* offA, const float* minB, const int* offB, int S, double* out,
                           void* stream);

/* Gradient of out[b,m,:] = src[b,idx[b,m],:] for rows of 3 floats (the nearest-neighbour gather of
 * src/utils.py:273-358's min over the broadcast): gsrc[b,i,:] = sum_{m: idx[b,m] = i} g[b,m,:] in
 * ascending m, gathered per row — no atomics.  g (B,M,3), idx (B,M), gsrc (B,N,3) fully written. */
int pn_gather_rows3_bwd_f32(const float* g, const int64_t* idx, int B, int M, int N, float* gsrc, void* stream);

/* ---- batched per-segment fitting (pn_weighted_moments, pn_small_lstsq,
 *      pn_bspline_eval) ------------------------------------------------------------------
 * Replace the serial per-segment Python loop of src/primitive_forward.py:925-1047
 * (fit_one_shape_torch), the four fits :708-843 (Fit.fit_{plane,sphere,cylinder,cone}_torch),
 * src/fitting_utils.py:32-85 (LeastSquares.lstsq, best_lambda), :385-455 (CustomSVD and its
 * custom backward), src/primitives.py:58-206 (ComputePrimitiveDistance) and the per-segment
 * loop of src/residual_utils.py:154-208 — for ALL analytic segments of ALL shapes of a step.
 *
 * Segment table (device int32 arrays of S entries): seg_shape = shape index b, seg_row = row of
 * the membership matrix W (B,Cp,N) holding the segment's soft weights, seg_type = 0 plane,
 * 1 sphere, 2 cylinder, 3 cone, seg_rows = number of fitted points (rank tolerance).  The fit
 * uses the points stride*j of the shape (fit_one_shape_torch keeps every 4th point for
 * analytic primitives) with weight W[b,row,stride*j] + eps.
 *
 *   pn_weighted_moments_f64   partial (S, pn_weighted_moments_chunks(), pn_weighted_moments_count())
 *                             fp64: sums of w^e * monomial(p, n), e <= 3, degree <= 3 (table in
 *                             csrc/fit_math.h) — everything the four fits need, one pass.
 *   pn_primitive_fit_f64      (the "pn_small_lstsq" of the survey, fused with the 3x3
 *                             eigen-decomposition) moments -> params (S,16) fp64 and the Jacobian
 *                             jac (S,16,64) = d params / d moments; 3x3 Jacobi, normal equations,
 *                             torch.matrix_rank-style rank test and the 1e-6*10^i ridge search on the
 *                             device.  params: plane a(3),d | sphere c(3),r | cylinder axis(3),c(3),r |
 *                             cone apex(3),axis(3),theta; slot 15 = ridge lambda used.  status bits:
 *                             1 = non-finite / no full-rank system (the reference raises),
 *                             2 = null cone (cond > 1e5: zero cone, no gradient), 4 = NaN residual.
 *   pn_cone_angle_f64         second pass of fit_cone_torch: theta (params slot 6), its Jacobian
 *                             row, and cone_direct (S) = factor of the direct path d theta / d w_i.
 *   pn_primitive_residual_f32 mean (squared, or guard_sqrt'ed if sqrt_flag) distance of the
 *                             ground-truth points gt_idx[gt_off[s] .. gt_off[s+1]) (indices into
 *                             the shape's points) to the primitive: dist (S) fp32, and
 *                             dparam (S,16) fp64 = d dist / d params.
 *   pn_weighted_moments_bwd_f32  gW (B,Cp,N) fp32 (zero-initialised by the caller) receives
 *                             d loss / d W at the fitted points given g_dist (S) = d loss / d dist. */
int pn_weighted_moments_chunks(void);
int pn_weighted_moments_count(void);
int pn_weighted_moments_f64(const float* P, const float* Nrm, const float* W, int B, int N, int Cp,
                            int stride, float eps, const int* seg_shape, const int* seg_row, int S,
                            double* partial, void* stream);
int pn_primitive_fit_f64(const double* partial, const int* seg_type, const int* seg_rows, int S,
                         double* params, double* jac, int* status, void* stream);
int pn_cone_angle_f64(const float* P, const float* W, int B, int N, int Cp, int stride, float eps,
                      const int* seg_shape, const int* seg_row, const int* seg_type,
                      const int* status, int S, double* params, double* jac, double* cone_direct,
                      void* stream);
int pn_primitive_residual_f32(const float* P, int B, int N, const int* seg_shape, const int* seg_type,
                              const int* gt_off, const int* gt_idx, int S, const double* params,
                              int sqrt_flag, float* dist, double* dparam, int* status, void* stream);
int pn_weighted_moments_bwd_f32(const float* P, const float* Nrm, const float* W, int B, int N, int Cp,
                                int stride, float eps, const int* seg_shape, const int* seg_row,
                                const int* seg_type, int S, const float* g_dist, const double* dparam,
                                const double* jac, const double* params, const double* cone_direct,
                                float* gW, void* stream);

/* B-spline surface evaluation, src/fitting_utils.py:609-622 sample_points_from_control_points_:
 * out[s,u,v,:] = A_s (sum_ij nu[u,i] nv[v,j] ctrl[s,i,j,:]) + t_s with nu (gu,cu), nv (gv,cv),
 * ctrl (S,cu,cv,3); affine (S,3,4) = [A_s | t_s] or NULL (the de-standardisation of
 * src/primitive_forward.py:60-72 folded in); wrap = 1 appends the first u-row again (closed
 * splines, :377-385): out (S,(gu+wrap)*gv,3).  _bwd: gctrl (S,cu,cv,3) from gout. */
int pn_bspline_eval_f32(const float* nu, const float* nv, const float* ctrl, const float* affine, int S,
                        int gu, int gv, int cu, int cv, int wrap, float* out, void* stream);
int pn_bspline_eval_bwd_f32(const float* nu, const float* nv, const float* gout, const float* affine,
                            int S, int gu, int gv, int cu, int cv, int wrap, float* gctrl, void* stream);

/* ---- round-3 fusions (csrc/fused.hip) ------------------------------------------------------
 * pn_edgeconv_bwd_stats_f32: step A of the fused edge-conv backward WITH its reductions (what
 * src/model.py:127-156 / src/PointNet.py:186-205 leave to autograd through Conv2d -> Norm ->
 * LeakyReLU -> max): from gout (B,Cout,N) and the forward's yext (B,N,Cout), mean / rstd writes
 *   t (B,N,Cout) = gamma * gout * LeakyReLU'(z),  dgamma (Cout), dbeta (Cout) and the group means
 *   c1c2 ((per_sample ? B : 1), groups, 2) that pn_edgeconv_bwd_f32 consumes (zeros when !dense:
 *   evaluation-mode BatchNorm).  Fixed-order partial sums, fp64 combination. */
size_t pn_edgeconv_bwd_stats_workspace(int B, int N, int Cout);
int pn_edgeconv_bwd_stats_f32(const float* gout, const float* yext, const float* mean, const float* rstd,
                              const float* gamma, const float* beta, int B, int N, int k, int Cout,
                              int groups, int per_sample, int dense, float slope, float* t, float* dgamma,
                              float* dbeta, float* c1c2, void* workspace, size_t workspace_bytes,
                              void* stream);

/* Triplet embedding loss, src/segment_loss.py:85-123 (EmbeddingLoss.triplet_loss, the arithmetic
 * after the numpy sampling): E (rows,D) unit-row embedding (D in {32, 64, 128}); item p of P has num <= 32
 * anchor/positive rows ia[p][:] and negative rows ib[p][:] (row indices into E) and a weight w[p]
 * (1 / (pairs of its shape + 1e-8));  c_ij = relu(|a_i - p_j|^2 - |a_i - n_j|^2 + margin),
 * item_loss[p] = w[p] * (sum_ij c_ij - sum_i c_ii) / (#(c_ij > 0) + 1), loss[0] = sum_p item_loss[p];
 * item_scale[p] = w[p] / (# + 1) is kept for the backward.  _bwd STORES gout[0] * d loss / d E into
 * the rows of gE (rows,D) that some item names and leaves the others as they are (the caller
 * zeroes gE).  A point can be sampled more than once: the per-item gradient rows go to `workspace`
 * (pn_triplet_bwd_workspace bytes) and rows naming the same point are added in item order — no
 * atomics, bit-reproducible. */
int pn_triplet_fwd_f32(const float* E, int rows, int D, const int64_t* ia, const int64_t* ib, const float* w,
                       int P, int num, float margin, float* item_loss, float* item_scale, float* loss,
                       void* stream);
size_t pn_triplet_bwd_workspace(int P, int num, int D);
int pn_triplet_bwd_f32(const float* E, int rows, int D, const int64_t* ia, const int64_t* ib,
                       const float* item_scale, const float* gout, int P, int num, float margin, float* gE,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Memberships of the fitting stage in one pass: src/residual_utils.py:120 (weights = center @
 * embedding^T), src/fitting_utils.py:306-325 (weights_normalize) and the labels of
 * src/mean_shift.py:176-178 (arg-max over the centres, first index on ties).
 * cen (B,CP,D) centre rows padded to CP in {16,32,64} (rows >= ncl[b] ignored), emb (B,N,D), D in {32, 64, 128},
 * bw (B), ncl (B) int64.  Outputs Wraw, prob, Wn (B,CP,N) (padding rows of prob / Wn are zero),
 * rowstat (B,CP,4) = (min_n prob, max_n (prob - min) + eps, arg-min, arg-max as int bits), labels
 * (B,N) int64 or NULL.  _bwd: gWraw (B,CP,N) from gWn, the exact gradient of weights_normalize
 * (min / max route to their first arg-min / arg-max column; clamp passes inclusively); rowgrad
 * (B,CP,2) is scratch.  d cen and d emb are then two GEMMs on gWraw (the caller's). */
int pn_membership_fwd_f32(const float* cen, const float* emb, const float* bw, const int64_t* ncl, int B,
                          int CP, int N, int D, float eps, float* Wraw, float* prob, float* Wn,
                          float* rowstat, int64_t* labels, void* stream);
int pn_membership_bwd_f32(const float* gWn, const float* Wraw, const float* prob, const float* rowstat,
                          const float* bw, const int64_t* ncl, int B, int CP, int N, float* rowgrad,
                          float* gWraw, void* stream);

/* Non-maximum suppression of the shifted points, src/mean_shift.py:139-179, without leaving the
 * device.  pn_nms_occupied_f32: membership (B,N) int64 = nearest shifted point of every input point
 * (pn_dot_select_f32, k = 1) -> counts (B,N) int32 members per shifted point (np.unique's counts,
 * :150-153), uq (B,U) int64 the occupied ones in ascending order (zero-padded), nocc (B) their number
 * (may exceed U: the caller retries with a larger U).  pn_nms_vote_f32: G (B,U,U) = Cu Cu^T of the
 * occupied centres -> every occupied centre votes for the FIRST arg-max of [2 - 2 G < bw] * counts
 * (:160-168; distance < b, not b^2, like the reference; only occupied columns can win: an
 * unoccupied one scores 0 and the centre itself scores its own count) -> hits (B,N) int32 scratch,
 * cid (B,cmax) int64 the voted centres in ascending order (zero-padded), ncl (B) their number. */
int pn_nms_occupied_f32(const int64_t* membership, int B, int N, int U, int* counts, int64_t* uq, int64_t* nocc,
                        void* stream);
int pn_nms_vote_f32(const float* G, const int64_t* uq, const int64_t* nocc, const int* counts, const float* bw,
                    int B, int N, int U, int cmax, int* hits, int64_t* cid, int64_t* ncl, void* stream);

/* y = act(x * scale[c] + shift[c]) on (B,C,N): evaluation-mode BatchNorm1d folded with the
 * activation that follows it (src/model.py:160-176: conv5/bn5 LeakyReLU(0.2), conv6/bn6 and
 * conv7/bn7 ReLU of the frozen SplineNets).  act: 0 none, 1 ReLU, 2 LeakyReLU(slope).
 * _bwd: gx = gy * scale[c] * act'(y). */
int pn_affine_act_fwd_f32(const float* x, const float* scale, const float* shift, int B, int C, int N,
                          int act, float slope, float* y, void* stream);
int pn_affine_act_bwd_f32(const float* gy, const float* y, const float* scale, int B, int C, int N, int act,
                          float slope, float* gx, void* stream);

/* out[s][c] = max_n act(x[s][c][n] * scale[c] + shift[c]) * w[s][n]: the frozen SplineNet's
 * conv5 -> bn5 (evaluation mode) -> LeakyReLU, "x *= weights" and the max pool over the points
 * (src/model.py:160-170) in one pass; idx (S,C) int32 first arg-max, val (S,C) the activation there.
 * _bwd: gw (S,N) = d / d w from g (S,C) (no gradient to x: the network is frozen); N <= 13 600 (12 bytes of LDS per point). */
int pn_weighted_max_fwd_f32(const float* x, const float* scale, const float* shift, const float* w, int S, int C,
                            int N, int act, float slope, float* out, int* idx, float* val, void* stream);
int pn_weighted_max_bwd_f32(const float* g, const int* idx, const float* val, int S, int C, int N, float* gw,
                            void* stream);

/* Standardisation of S spline segments (src/fitting_utils.py:512-553, standardize_point_torch): the two steps that
 * are not arithmetic on the points (mean, covariance and rotation stay tensor expressions: csrc/fused.hip says why).
 *   select: sel (S,n) bytes = w > 0.8, or — fewer than 400 such points — the kf largest memberships (ties to the
 *           smaller index);
 *   scale : std (S,3) = | max - min | over the selected points of Pr * w per axis, pts (S,n,3) = Pr / (std + eps),
 *           Pr (S,n,3) the rotated centred points.
 * w (S,n) fp32; one 256-thread workgroup per segment; exact operations, bit-identical to the tensor-library form. */
int pn_standardize_select_f32(const float* w, int S, int n, int kf, unsigned char* sel, void* stream);
int pn_standardize_scale_f32(const float* Pr, const float* w, const unsigned char* sel, int S, int n, float eps,
                             float* pts, float* stdv, void* stream);
/* Adam (torch.optim.Adam's defaults and update rule: train_parsenet.py:96, train_parsenet_e2e.py:88,
 * train_open_splines.py:81) on ONE flat fp32 buffer of n parameters: p, the gradients g and both moments m, v are
 * contiguous arrays of n floats; step = the 1-based count of this update.  One launch for the whole model. */
int pn_adam_flat_f32(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                     float eps, int step, void* stream);

/* Gradient tensors into the flat data-parallel bucket (the buffer the ONE all-reduce of a step works on; the
 * reference's DataParallel reduces per parameter, train_parsenet.py:90-91): tensor e = ns[e] floats at srcs[e] goes
 * to flat + offs[e].  srcs / offs / ns are HOST arrays of count entries; 64 tensors per launch. */
int pn_gather_flat_f32(const float* const* srcs, const long long* offs, const long long* ns, int count, float* flat,
                       void* stream);

/* ---- linear sum assignment: batched forward auction with eps-scaling (evaluation-mode LS refit) ------
 * Replaces the solver behind lapsolver.solve_dense in src/primitive_forward.py:197-198, 272-273 up to eps: S
 * independent problems in one launch, one workgroup each.  Problem s: cost matrix h_cost[s] (a DEVICE pointer; the
 * four h_* tables are HOST arrays of S entries), h_n[s] rows, h_m[s] >= h_n[s] columns, row stride h_ld[s] >= h_m[s]
 * doubles, minimised; it is solved as the square h_m x h_m problem with h_m - h_n zero-cost rows (not materialised).
 * Schedule: eps = max(eps_start, eps_final) x (max - min of the costs), divided by theta > 1 per phase down to
 * eps_final x that range; assignments are reset between phases, prices kept.  At most max_rounds bidding rounds.
 * Outputs, out_ld >= every h_m:  col (S,out_ld) int32 — column of row i for i < h_m[s] (rows >= h_n[s] are the
 * zero-cost rows), -1 where unassigned or beyond h_m[s];  price (S,out_ld) column prices p >= 0;  eps (S) the eps
 * reached;  rounds (S);  status (S): 0 = complete, then c[i,col_i] + p[col_i] <= min_j (c[i,j] + p[j]) + eps for every
 * row of the square problem; 1 = stopped by max_rounds with the prices and the partial assignment it had.
 * Bit-reproducible from run to run.  Limits: h_m <= 3584 (44 bytes of LDS per column). */
int pn_lsa_auction_f64(const double* const* h_cost, const int* h_n, const int* h_m, const int* h_ld, int S,
                       double eps_start, double theta, double eps_final, int max_rounds, int out_ld, int* col,
                       double* price, double* eps, int* rounds, int* status, void* stream);

/* ---- trimmed surfaces of the evaluation mode (csrc/surface.hip) ------------------------------------------------
 * Grid occupancy: replaces the loop of src/fitting_utils.py:240-273 (create_grid) for the S fitted segments of a
 * shape in one launch.  Segment s: a regular size_u[s] x size_v[s] grid of vertices, rows voff[s] .. of grid
 * (sum U V, 3) fp32, row-major; its up-sampled cloud, rows coff[s] .. coff[s+1] of cloud (sum P, 3) fp32; a threshold.
 * mask (sum (U-1)(V-1)) bytes, the cells of segment s row-major from cell_off[s]:
 *   centre = (((v[i][j] + v[i][j+1]) + v[i+1][j]) + v[i+1][j+1]) * 0.25f   per coordinate,
 *   d      = ((dx*dx + dy*dy) + dz*dz)                                      every operation rounded to fp32 once,
 *   mask   = sqrtf(min over the cloud of d) < thres[s]                      (a NaN distance never hits),
 * the decision of the tensor expression bit for bit (the kernel stops at the first hit).  A workgroup owns
 * pn_grid_occupancy_tile() cells of one segment: tile_off (S+1) is the prefix sum of ceil(cells / tile) and
 * total_tiles its last entry.  All tables are DEVICE arrays of int32 (thres: fp32).
 * Limits: size_u, size_v >= 2; every cloud has at least one point; int32 offsets (sum U V, sum P < 2^31 / 3). */
int pn_grid_occupancy_tile(void);
int pn_grid_occupancy_ragged_f32(const float* grid, const int* size_u, const int* size_v, const int* voff,
                                 const float* cloud, const int* coff, const float* thres, const int* tile_off,
                                 const int* cell_off, int S, int total_tiles, unsigned char* mask, void* stream);
/* Triangles of the kept cells and area-weighted samples (src/fitting_utils.py:276-303 tessalate_points_fast,
 * src/utils.py:123-178 sample_mesh / triangle_area_multi), float64 on the widened fp32 vertices, M meshes in one
 * launch.  Mesh m: grid rows from voff[m], row length size_v[m]; its faces are face_off[m] .. face_off[m+1]
 * (face_off (M+1), two per kept cell); cells (total_faces / 2) int32: the kept cells of all meshes, row-major index
 * into the mesh's (U-1) x (V-1) cells, ascending.  Face 2c is (i,j),(i+1,j),(i+1,j+1), face 2c+1 is
 * (i,j),(i+1,j+1),(i,j+1).
 *   area: area[f] = 0.5 |(v2 - v1) x (v3 - v1)|.
 *   sample: sample k of mesh m (samp_off (M+1), every mesh at least one sample) takes the first face of the mesh
 *   whose cdf (total_faces, per mesh ascending, last entry 1) exceeds pick[k]; (u, v) -> (1-u, 1-v) when u + v > 1;
 *   out[k] = (float)(v1*u + v2*v + (1 - (u+v))*v3).  face (total_samples) int32, optional: the face taken, local
 *   to the mesh.  pick, u, v: caller-supplied uniforms in [0, 1), float64. */
int pn_trimesh_area_f64(const float* grid, const int* voff, const int* size_v, const int* face_off, const int* cells,
                        int M, int total_faces, double* area, void* stream);
int pn_trimesh_sample_f64(const float* grid, const int* voff, const int* size_v, const int* face_off,
                          const int* cells, const double* cdf, const int* samp_off, const double* pick,
                          const double* u, const double* v, int M, int total_samples, float* out, int* face,
                          void* stream);

/* ---- point coverage of the fitted primitives (csrc/cover.hip) --------------------------------------------------
 * Replaces src/eval_utils.py:103-127 (p_coverage: one residual call per primitive over the whole cloud, stack,
 * minimum) for the B shapes of a ragged batch in one launch.  Shape b: points pt_off[b] .. pt_off[b+1] of points
 * (T,3) fp32 and primitives prim_off[b] .. prim_off[b+1].  Primitive s: prim_type[s] and the row prim_par[s]
 * (16 fp32 slots, the layout of pn_primitive_residual_f32):
 *   0 plane a(3), d;  1 sphere centre(3), r;  2 cylinder axis(3), centre(3), r;  3 cone apex(3), axis(3), theta;
 *   >= 4 sampled (the two spline kinds): rows samp_off[s] .. samp_off[s+1] of samp (sum, 3) fp32, at least one; the
 *   parameter row is not read.  samp_off (S+1) is ascending with empty slices for the analytic primitives; samp
 *   may be NULL when no primitive is sampled.
 * Per point:  dmin (T) fp32 = the smallest distance over the shape's primitives, each with guard_sqrt
 * (sqrtf(max(d, 1e-5f))): analytic ones by the fp32 arithmetic of the batched fitting stage; for a sampled one the
 * nearest sample j is the first arg-min of ((dx*dx + dy*dy) + dz*dz) (the Chamfer kernel's chain, every operation
 * rounded once) and the distance is sqrtf(max(((dx*dx + dz*dz) + dy*dy) at j, 1e-5f)) — the order in which the
 * tensor library's GPU reduction was observed to add the three squares (tools/sum3_order_probe.py,
 * profiles/sum3_order.txt; pinned bit for bit by tests/test_pcover_gpu.py, not guaranteed by that library), so that
 * the value is chamfer_distance_single_shape's;
 * arg (T) int32 = the index of that primitive within the shape, the lowest on equal values.  A NaN distance is kept
 * (the first one; a point with a NaN coordinate gets NaN from sampled primitives too: they re-evaluate at sample 0
 * when no comparison held); a shape without primitives, or a point whose distances are all inf, gets (inf, -1).
 * A workgroup owns pn_point_primitive_min_tile() consecutive points of one shape: tile t starts at point
 * tile_first[t] (a row of points) of shape tile_shape[t]; total_tiles = sum_b ceil(N_b / tile).  All tables are
 * DEVICE arrays of int32.  The result of a point does not depend on the tiling.
 * Limits: int32 offsets (T, sum of samples < 2^31 / 3). */
int pn_point_primitive_min_tile(void);
int pn_point_primitive_min_f32(const float* points, const int* pt_off, const int* prim_off, const int* prim_type,
                               const float* prim_par, const float* samp, const int* samp_off, const int* tile_shape,
                               const int* tile_first, int B, int total_tiles, float* dmin, int* arg, void* stream);

/* ---- exact distance from points to the trimmed surfaces (csrc/tridist.hip, arithmetic: csrc/tri_math.h) --------
 * The distance from every point of a shape to the nearest triangle of the kept cells of the shape's surfaces: the
 * limit, for infinitely many samples, of the distance to the nearest sample that the coverage metrics use.
 * Two launches for a ragged batch of B shapes.  The mesh tables are those of pn_trimesh_area_f64 over the M meshes
 * of all shapes, a shape's meshes consecutive: shape b owns the faces shape_face[b] .. shape_face[b+1]
 * (shape_face (B+1) = face_off at the shape's first mesh) and the triangle SLOTS slot_off[b] .. slot_off[b+1]
 * (slot_off (B+1), slot_off[0] = 0, a shape's slot count = its face count rounded up to a multiple of
 * pn_trimesh_group(), at least one face per shape); total_slots = slot_off[B].
 *   records: rec (16 * total_slots) fp32, structure of arrays: rec[k * total_slots + slot] = value k of the slot's
 *   triangle (vertex opposite the longest edge, two edges, their cross product, four reciprocals; padding slots hold
 *   a record no finite point is nearest to); sph (total_slots / group, 4) fp32, 16-byte aligned: centre and radius
 *   of a ball that holds the group's triangles.
 *   distance: points (T,3) fp32, shape b rows pt_off[b] .. pt_off[b+1]; a workgroup of `waves` (4, 8 or 16) waves
 *   owns pn_trimesh_point_dist_tile() consecutive points of one shape: tile t starts at row tile_first[t] of shape
 *   tile_shape[t]; total_tiles = sum_b ceil(N_b / tile).  dist2 (T) fp32: the squared distance to the nearest
 *   triangle; face (T) int32: its index among the shape's faces, the lowest on equal distances.  prune != 0 skips
 *   groups whose certified lower bound exceeds the running minimum of all 64 points of a wave; the results are the
 *   same bits for prune 0 and 1, for every `waves`, and from run to run.  skipped (one 64-bit counter, optional):
 *   the number of groups skipped is ADDED to it.
 * All tables are DEVICE arrays of int32.  Limits: int32 offsets (3 T, 16 total_slots < 2^31); coordinates far
 * below 1e18 in magnitude. */
int pn_trimesh_group(void);
int pn_trimesh_point_dist_tile(void);
int pn_trimesh_records_f32(const float* grid, const int* voff, const int* size_v, const int* face_off,
                           const int* cells, int M, const int* shape_face, const int* slot_off, int B,
                           int total_slots, float* rec, float* sph, void* stream);
int pn_trimesh_point_dist_f32(const float* points, const int* pt_off, const int* slot_off, const float* rec,
                              int total_slots, const float* sph, const int* tile_shape, const int* tile_first, int B,
                              int total_tiles, int waves, int prune, float* dist2, int* face,
                              unsigned long long* skipped, void* stream);

/* ---- point normals from the cloud itself: k-NN PCA (csrc/normals.hip, arithmetic: csrc/normal_math.h) ----------
 * The reference reads normals from its data files (its own estimate_normals call is commented out, src/utils.py:61);
 * this produces them for a cloud that has none, for a RAGGED batch of S segments in one launch.
 * pts (total,3) fp32, off (S+1) int32 row offsets, idx (total,k) int32: the LOCAL indices pn_knn3_ragged wrote (the
 * point itself first; a segment with fewer than k points arrives padded with the point itself, and the padding
 * entries count as copies of the point).  3 <= k <= 64.
 * Per point, in fp64 on the fp32 coordinates, every sum in neighbour order: the mean of the k neighbours, the
 * covariance of the differences to it (divided by k), its eigenvalues l0 <= l1 <= l2 by cyclic Jacobi (a fixed number
 * of sweeps).  normals (total,3) fp32: the unit eigenvector of l0, rounded to fp32 once; viewpoints NULL: the
 * component of largest magnitude is positive (the lowest axis on a tie); viewpoints (S,3) fp32: that normal, flipped
 * iff n . (v_s - p) < 0 (fp64; a zero dot keeps it).  variation (total) fp32 or NULL: l0 / (l0 + l1 + l2);
 * gap (total) fp32 or NULL: (l1 - l0) / l2, small where the normal is ill-defined (edges, corners, lines).
 * l2 <= 1e-30 (coincident neighbours) or a segment of fewer than 3 points: normal (0,0,0), variation = gap = 0; no
 * NaN for finite input.
 * A workgroup owns pn_point_normals_tile() consecutive points of one segment: tile t starts at row tile_first[t] of
 * segment tile_seg[t]; total_tiles = sum_s ceil(n_s / tile).  off and the tile tables are DEVICE arrays of int32.
 * The result of a point depends on its neighbourhood alone: the same bits from run to run and for every batching.
 * PN_ERR_ARG (before any launch) for k out of range, S < 0, total < 0 or a NULL required pointer; total == 0 or
 * S == 0 returns 0 without a launch. */
int pn_point_normals_tile(void);
int pn_point_normals_f32(const float* pts, const int* off, int S, int total, const int32_t* idx, int k,
                         const float* viewpoints, const int* tile_seg, const int* tile_first, int total_tiles,
                         float* normals, float* variation, float* gap, void* stream);

/* ---- consistent normal orientation without a viewpoint (csrc/orient.hip, definition: csrc/orient_math.h) --------
 * Signs are propagated along the minimum spanning forest of the k-NN graph under the weight 1 - |n_i . n_j| (Hoppe
 * et al. 1992), for a RAGGED batch of S segments in one launch, one workgroup per segment, no workspace.
 * pts (total,3) fp32 (only z is read: the seed rule), off (S+1) DEVICE int32 row offsets, idx (total,k) int32: the
 * LOCAL indices pn_knn3_ragged wrote, 1 <= k <= 64; normals_in (total,3) fp32, from anywhere.
 * Entries: one per (point i, slot s), e = i k + s, j = idx[i][s]; an entry with j == i (self and padding) or j outside
 * the segment is dropped; an entry is incident to i and to j.  dot = (nx_i nx_j + ny_i ny_j) + nz_i nz_j in fp64,
 * w = (float) max(0, 1 - |dot|), neg = dot < 0 (a zero normal: w = 1, neg = false).  Entries are ordered by the key
 * (bits of w) << 32 | e, a strict order, so the minimum spanning forest is unique.  Along every forest edge
 * flip(j) = flip(i) XOR neg.  The seed of a connected component is its vertex of largest fp32 z (the lowest index on
 * equal z); the component's bit makes the seed's oriented n_z >= 0 (a seed with n_z == 0 keeps flip = 0).
 * normals_out (total,3): the input normal, bit-identical or with every sign bit inverted; it must not be normals_in.
 * flip (total) int32 0/1 or NULL; seed (total) int32 or NULL: the local index of the seed of the point's component.
 * All outputs are functions of the input alone: the same bits from run to run and for every batching.
 * A segment of more than pn_orient_normals_max_points() points is not truncated: its normals come out NaN, its flip
 * and seed -1.  PN_ERR_ARG (before any launch) for k out of range, S < 0, total < 0 or a NULL required pointer;
 * total == 0 or S == 0 returns 0 without a launch. */
int pn_orient_normals_max_points(void);
int pn_orient_normals_f32(const float* pts, const int* off, int S, int total, const int32_t* idx, int k,
                          const float* normals_in, float* normals_out, int32_t* flip, int32_t* seed, void* stream);

/* ---- exact neighbours of 3-D points on clouds of any size: uniform-grid search (csrc/knn3_grid.hip, definition:
 * csrc/knn3_grid_math.h) --------------------------------------------------------------------------------------------
 * The results of pn_knn3_ragged's fp32 mode, bit for bit, at cost O(n k) and without its limit on the segment size.
 * pts (total,3) fp32, off (S+1) DEVICE int32 row offsets, max_n >= the largest segment (kept for symmetry with
 * pn_knn3_ragged: nothing is sized by it).  idx (total,k) int32 LOCAL to the segment: the k smallest under
 * d(i,j) = ((x_i-x_j)^2 + (y_i-y_j)^2) + (z_i-z_j)^2, every operation rounded once in fp32, no fma, ordered by (d, j)
 * ascending — the point itself (or a coincident point of smaller index) first; a segment with fewer than k points is
 * padded with the point itself.  dist (total,k) fp32 or NULL: (float) sqrt((double) d).  1 <= k <= 64, any segment
 * size, total * k < 2^31.  A segment that holds a non-finite coordinate: every row the point itself k times, dist NaN.
 * Five stream-ordered launches (bounding boxes, cells and histogram, scan, scatter into cell order, search), no host
 * synchronisation; workspace of pn_knn3_grid_workspace_bytes(total, S) bytes, linear in total.  All outputs are
 * functions of the input alone: the same bits from run to run and for every batching.
 * PN_ERR_ARG (before any launch) for k out of range, S < 0, total < 0, a NULL required pointer or a workspace that is
 * too small; total == 0 or S == 0 returns 0 without a launch. */
long long pn_knn3_grid_workspace_bytes(long long total, int S);
int pn_knn3_grid_f32(const float* pts, const int* off, int S, int total, int max_n, int k, int32_t* idx, float* dist,
                     void* ws, long long ws_bytes, void* stream);

/* ---- consistent normal orientation on clouds of any size: the global-memory engine (csrc/orient_global.hip, steps
 * and schedule: csrc/orient_global_math.h, definition: csrc/orient_math.h) -------------------------------------------
 * The definition, the arguments and the outputs of pn_orient_normals_f32, bit for bit, with no limit on the points of
 * a segment: the Boruvka state (a packed parent word and a 64-bit slot per point, the pending hooks) lives in a
 * workspace of pn_orient_normals_global_workspace_bytes(total, S) bytes, linear in total, and every step runs over
 * many workgroups.  max_n >= the largest segment (a host integer): it alone fixes the schedule —
 * ceil(log2 max_n) + 1 rounds of one offer launch (64-bit integer atomic minima), one hook launch and
 * ceil(log_64 max_n) compress launches (every vertex walks up to 64 parents), between one init launch and two tail
 * launches; pn_orient_normals_global_launches(max_n) is that number of kernel launches (two memsets come on top) and
 * needs no GPU.  All of it is stream-ordered: no host synchronisation, no cooperative launch, no waiting between
 * workgroups; once no component finds an entry the remaining launches exit at a device flag.
 * A point that no valid segment of off holds gets NaN normals, flip and seed -1.  A max_n below the largest segment
 * can end the rounds early (a wrong forest, never an access outside the buffers).
 * PN_ERR_ARG (before any launch) for k out of range, S < 0, total < 0, max_n < 0, total * k >= 2^31, a NULL required
 * pointer (the workspace included), normals_out == normals_in or a workspace that is too small; total == 0 or S == 0
 * returns 0 without a launch. */
long long pn_orient_normals_global_workspace_bytes(long long total, int S);
int pn_orient_normals_global_launches(int max_n);
int pn_orient_normals_global_f32(const float* pts, const int* off, int S, int total, int max_n, const int32_t* idx,
                                 int k, const float* normals_in, float* normals_out, int32_t* flip, int32_t* seed,
                                 void* ws, long long ws_bytes, void* stream);

/* ---- farthest-point sampling of clouds of any size, with the nearest sample of every point (csrc/fps.hip,
 * definition: csrc/fps_math.h) ----------------------------------------------------------------------------------------
 * pts (total,3) fp32, off (S+1) DEVICE int32 row offsets from 0 to total, max_n >= the largest segment (kept for
 * symmetry with pn_knn3_grid_f32: nothing is sized by it), m >= 1 samples per segment, start (S) int32 LOCAL indices
 * or NULL (0); a start outside its segment is clamped into it.  Per segment of n points, m_c = min(m, n), under
 * d(i,j) = ((x_i-x_j)^2 + (y_i-y_j)^2) + (z_i-z_j)^2, every operation rounded once in fp32, no fma: every point starts
 * with D = +inf and owner -1; for t = 0 .. m_c-1: radius_t = D of s_t, s_t becomes chosen (D = 0, owner = t), every
 * unchosen i with d(i, s_t) < D_i (strict) takes that D and owner t, and s_{t+1} is the unchosen point of largest D, the
 * lowest index on equal D.  sample (S,m) int32 LOCAL indices in selection order, -1 from m_c on; radius (S,m) fp32 or
 * NULL, +inf at t = 0, NaN where sample is -1; owner (total) int32 or NULL: the rank of the nearest sample, ties to the
 * earliest rank; dist (total) fp32 or NULL: the final D.  A segment that holds a non-finite coordinate: sample -1,
 * radius NaN, owner -1, dist NaN throughout.  owner and dist of a point that no valid segment of off holds are not
 * written.  All outputs are functions of the input alone: the same bits from run to run and for every batching.
 * pn_fps_launches(m) = m + 2 stream-ordered kernel launches (one memset comes on top), one per sample between an init
 * and an output launch, each over all segments; it needs no GPU.  No host synchronisation, no cooperative launch, no
 * waiting between workgroups; the candidates of a step meet in one 64-bit integer atomicMax per workgroup.  Workspace
 * of pn_fps_workspace_bytes(total, S, m) bytes: 8 S (m + 2) of slots + 4 total + 8 (total / 1024 + S) + 16; S (m + 2)
 * must stay below 2^59 so that the slots' byte count fits a long long (pn_fps_workspace_bytes returns 0 beyond it).
 * PN_ERR_ARG (before any launch) for m < 1, S < 0, total < 0 (a total of 2^31 or more does not fit the int), max_n < 0,
 * S (m + 2) >= 2^59, a NULL pts, off, sample or ws, or a workspace that is too small; S == 0 returns 0 without a
 * launch. */
long long pn_fps_workspace_bytes(long long total, int S, int m);
int pn_fps_launches(int m);
int pn_fps_f32(const float* pts, const int* off, int S, int total, int max_n, int m, const int32_t* start,
               int32_t* sample, float* radius, int32_t* owner, float* dist, void* ws, long long ws_bytes, void* stream);

/* ---- statistical outlier removal on clouds of any size (csrc/outlier.hip, definition: csrc/outlier_math.h) ----------
 * dist (total,k) fp32: the neighbour distances pn_knn3_ragged (fp32 mode) or pn_knn3_grid_f32 wrote — nearest first, the
 * point itself first, padded with the point itself in a segment shorter than k; off (S+1) DEVICE int32 row offsets from
 * 0 to total; 1 <= k <= 64; std_ratio finite and >= 0.  Per segment of n points, k_c = min(k, n), under the definition
 * of csrc/outlier_math.h: avg (total) fp64, a_i = the sum of the k_c distances in ascending order / k_c; stats (S,3)
 * fp64: mean = SUM(a_i > 0 ? a_i : 0) / n, std = sqrt(SUM(a_i > 0 ? (a_i - mean)^2 : 0) / (n - 1)) (0 for n <= 1) and
 * thr = mean + std_ratio * std, SUM being one fixed tree over tiles of 1 024 points of the segment; keep (total) 0/1:
 * a_i > 0 && a_i < thr; kept (S) int32: the kept points of the segment; index (total) int32 or NULL: the LOCAL indices
 * of the kept points ascending in the first kept[s] entries of the segment's rows, -1 behind them.  A NaN a_i enters
 * the sums as NaN and then replaces every a_i of its segment: a segment that holds a non-finite coordinate (some or all
 * of its rows of dist NaN) ends with avg, mean, std and thr NaN, keep 0 and kept 0.  An empty segment: mean and thr NaN, std 0, kept 0.  A row that no valid segment of off holds gets
 * avg NaN, keep 0 and index -1; a segment that does not lie inside 0 .. total gets NaN stats and kept 0.  All outputs
 * are functions of dist, the offsets of the segment's own rows, k and std_ratio alone: the same bits from run to run
 * and for every batching.
 * pn_outlier_launches() = 6 stream-ordered kernel launches, each over all segments; it needs no GPU.  No host
 * synchronisation, no cooperative launch, no waiting between workgroups, no atomics.  Workspace of
 * pn_outlier_workspace_bytes(total, S) bytes: 20 (total / 1024 + S) + 16.
 * PN_ERR_ARG (before any launch) for k < 1 or k > 64, S < 0, total < 0, total * k >= 2^31, a negative or non-finite
 * std_ratio, a NULL dist, off, avg, stats, keep, kept or ws, or a workspace that is too small; total == 0 or S == 0
 * returns 0 without a launch and writes nothing. */
long long pn_outlier_workspace_bytes(long long total, int S);
int pn_outlier_launches(void);
int pn_outlier_stat_f32(const float* dist, const int* off, int S, int total, int k, double std_ratio, double* avg,
                        double* stats, uint8_t* keep, int32_t* kept, int32_t* index, void* ws, long long ws_bytes,
                        void* stream);

/* ---- voxel-grid downsampling of clouds of any size, with the voxel of every point (csrc/voxel.hip, definition:
 * csrc/voxel_math.h) ---------------------------------------------------------------------------------------------------
 * pts (total,3) fp32, off (S+1) DEVICE int32 row offsets from 0 to total, voxel (S) fp32 DEVICE: the edge h of the
 * cubic cells of every segment, origin (S,3) fp32 DEVICE or NULL (the per-axis minimum lo of the segment).  Per segment
 * of n points: the cell of a point is c_a = floor(((double) x_a - (double) o_a) / (double) h) in fp64, a point on a
 * face in the upper cell; a voxel is the set of points with the same cell triple, and voxels are numbered 0 .. V-1 by
 * the ascending lowest point index they hold.  owner (total) int32: the number of every point's voxel (owner of a
 * segment's first point is 0); nvox (S) int32: V.  centroid (total,3) fp32, count, first, rep (total) int32, any of them
 * NULL: the voxel arrays of a segment occupy the first nvox[s] entries of the segment's own rows, NaN (centroid) and -1
 * stand behind them — nothing is sized by a number that only the device knows.  centroid: with lo, hi the bounds of
 * the segment, 2^E > max extent (frexp of the fp64 difference), s = 32 - E (0 for a zero extent) and
 * u = llrint(((double) x - (double) lo) 2^s), (float) ((double) lo + ((double) SUM u / (double) count) 2^-s), the sum
 * in 64-bit integers: exact in any order, within extent 2^-33 plus one fp32 rounding of the true mean.  first: the
 * lowest LOCAL index of the voxel, ascending over the rows.  rep: the LOCAL index of the member with the smallest
 * d = ((dx^2 + dy^2) + dz^2) to the fp32 centroid, every operation rounded once in fp32, no fma, the lowest index on
 * equal d.  Status instead of V in nvox, with owner -1 throughout and no voxel rows (NaN / -1 in all of them): -1 for a
 * segment that holds a non-finite coordinate; -2 ("voxel too small for the extent") where some c_a lies outside
 * [-2^20, 2^20), where voxel[s] is not a positive finite number or an origin is not finite.  Rows that no valid segment
 * of off holds are not written; a segment that does not lie inside 0 .. total gets nvox 0.  All outputs are functions
 * of the segment's points, voxel[s] and origin[s] alone: the same bits from run to run and for every batching.
 * pn_voxel_launches() = 7 stream-ordered kernel launches (two memsets come on top; 6 when rep is NULL), each over all
 * segments; it needs no GPU.  No host synchronisation, no cooperative launch, no waiting between workgroups; the points
 * of a voxel meet in 64-bit integer atomics (compare-and-swap on the cell key, add, min) on an open-addressing table of
 * two slots per point.  Workspace of pn_voxel_workspace_bytes(total, S) bytes: 104 total + 12 (total / 1024 + S) +
 * 40 S + 16, known from its arguments alone; 0 for total < 0, total >= 2^31 or S < 0.
 * PN_ERR_ARG (before any launch) for S < 0, total < 0 (a total of 2^31 or more does not fit the int), a NULL pts, off,
 * voxel, owner, nvox or ws, or a workspace that is too small; S == 0 or total == 0 returns 0 without a launch and
 * writes nothing. */
long long pn_voxel_workspace_bytes(long long total, int S);
int pn_voxel_launches(void);
int pn_voxel_f32(const float* pts, const int* off, int S, int total, const float* voxel, const float* origin,
                 int32_t* owner, int32_t* nvox, float* centroid, int32_t* count, int32_t* first, int32_t* rep,
                 void* ws, long long ws_bytes, void* stream);

/* ---- Euclidean cluster extraction on clouds of any size (csrc/cluster.hip, definition: csrc/cluster_math.h) ----------
 * pts (total,3) fp32, off (S+1) DEVICE int32 row offsets from 0 to total, max_n >= the largest segment (a host integer:
 * it alone fixes the schedule), radius (S) fp32 DEVICE: the radius r of every segment, min_size >= 1.  Per segment of n
 * points, indices LOCAL to it, r2 = fl(r * r) in fp32: {i, j}, i != j, is an edge iff
 * d = ((x_i-x_j)^2 + (y_i-y_j)^2) + (z_i-z_j)^2 <= r2, every operation rounded once in fp32, no fma (equality is an
 * edge); a component is a connected component of that graph, kept iff it holds at least min_size points; the kept
 * components are numbered 0 .. C-1 by their ascending lowest point index.  label (total) int32: the number of every
 * point's component, -1 for a point of a dropped component; ncomp (S) int32: C.  count, first (total) int32 or NULL: the
 * size and the lowest LOCAL index of the kept components in the first ncomp[s] entries of the segment's own rows
 * (first ascends), -1 behind them — nothing is sized by a number that only the device knows.  ndrop (S) int32 or NULL:
 * the points of the segment with label -1.  Status instead of C in ncomp, with label, count and first -1 throughout and
 * ndrop n: -1 for a segment that holds a non-finite coordinate (flagged while the bounding box is taken, never
 * searched); -2 where r or r2 is not a positive finite number (r = 1e-30: r2 underflows).  Rows that no valid segment
 * of off holds are not written; a segment that does not lie inside 0 .. total gets ncomp 0 (and ndrop 0).  All outputs
 * are functions of the segment's points, radius[s] and min_size alone: the same bits from run to run and for every
 * batching.
 * The neighbours come from an exact uniform-grid search (the cells and the bound of csrc/knn3_grid_math.h, a cell edge
 * not below r where the cloud allows it); the components from ceil(log2 max_n) + 1 Boruvka rounds in global memory —
 * one offer launch (every point searches its ball; one 64-bit integer atomic minimum per point), one hook launch and
 * ceil(log_64 max_n) compress launches each — between four launches that build the grid and three that number the
 * components: pn_cluster_launches(max_n) = 4 + (ceil(log2 max_n) + 1) (2 + ceil(log_64 max_n)) + 3 kernel launches
 * (three memsets come on top); it needs no GPU.  All of it is stream-ordered: no host synchronisation, no cooperative
 * launch, no waiting between workgroups; once no component finds an edge the remaining rounds exit at a device flag.
 * A max_n below the largest segment can end the rounds early (components left apart, never an access outside the
 * buffers).  Workspace of pn_cluster_workspace_bytes(total, S) bytes: 56 total + 36 S + 1296, known from its arguments
 * alone; 0 for total < 0, total >= 2^31 or S < 0.  Its first 32 words (after alignment to 16 bytes) hold, after the
 * call, 1 for every round in which a component found an edge.
 * PN_ERR_ARG (before any launch) for S < 0, total < 0, max_n < 0, min_size < 1, a NULL pts, off, radius, label, ncomp
 * or ws, or a workspace that is too small; S == 0 or total == 0 returns 0 without a launch and writes nothing. */
long long pn_cluster_workspace_bytes(long long total, int S);
int pn_cluster_launches(int max_n);
int pn_cluster_f32(const float* pts, const int* off, int S, int total, int max_n, const float* radius, int min_size,
                   int32_t* label, int32_t* ncomp, int32_t* count, int32_t* first, int32_t* ndrop, void* ws,
                   long long ws_bytes, void* stream);

/* ---- Dominant-plane extraction on clouds of any size (csrc/plane.hip, definition: csrc/plane_math.h) -----------------
 * pts (total,3) fp32, off (S+1) DEVICE int32 row offsets from 0 to total, threshold (S) fp32 DEVICE: the threshold t of
 * every segment, H hypotheses (1 .. 4096), seed: 64 bits, passed as the bits of a long long, refine: 0 .. 4 rounds, axis:
 * NULL or three HOST doubles of unit length with min_cos in [0, 1].  Per segment of n points, indices LOCAL to it:
 * hypothesis h is the plane (n, d), |n| = 1 in fp64 with the component of largest magnitude positive, through the
 * points ((splitmix64(seed + 0x9E3779B97F4A7C15 (3 h + s + 1)) >> 32) n) >> 32, s = 0, 1, 2; it is invalid when two of
 * them are equal, when they are collinear and, with an axis, when |n . axis| < min_cos.  A point is an inlier iff
 * |((nx x + ny y) + nz z) + d| <= (double) t in fp64, every operation rounded once.  The valid hypothesis with the most
 * inliers wins, the lowest h on equal counts; every refinement round replaces the plane by the least-squares plane
 * through its inliers (fp64 moments summed by the fixed tree of csrc/outlier_math.h, the Jacobi solver of
 * csrc/normal_math.h) iff that plane is not degenerate, satisfies the axis constraint and has at least as many inliers.
 *   plane (S,4) fp64: nx, ny, nz, d; count (S) int32: its inliers; best (S) int32: the winning h, whatever the refinement
 *   did, -1 without a valid hypothesis (count 0, plane zeros); inlier (total) one byte per point; dist (total) fp32 or
 *   NULL: the signed distance of every point, formed in fp64 and rounded once, NaN in a segment without a plane.
 *   count -1: the segment holds a non-finite coordinate; -2: t is no positive finite number; both: best -1, plane zeros,
 *   no inlier.  A point that no valid segment of off holds gets inlier 0 and dist NaN.
 * All outputs are functions of the segment and the arguments alone: the same bits from run to run and for every
 * batching.  pn_plane_launches(refine) = 5 + 6 refine stream-ordered kernel launches (0 for refine outside 0 .. 4); it
 * needs no GPU.  No host synchronisation, no cooperative launch, no waiting between workgroups; the inlier counts of a
 * hypothesis meet in integer atomic additions.  Workspace of pn_plane_workspace_bytes(total, S, H) bytes:
 * 36 S H + 64 (total / 1024 + S) + 60 S + 16, known from its arguments alone; 0 for total < 0, total >= 2^31, S < 0 or H
 * outside 1 .. 4096.
 * PN_ERR_ARG (before any launch) for S < 0, total < 0, H outside 1 .. 4096, refine outside 0 .. 4, min_cos outside [0, 1]
 * with an axis, S * H >= 2^31, a NULL pts, off, threshold, plane, count, best, inlier or ws, or a workspace that is too
 * small; S == 0 or total == 0 returns 0 without a launch and writes nothing. */
long long pn_plane_workspace_bytes(long long total, int S, int H);
int pn_plane_launches(int refine);
int pn_plane_f32(const float* pts, const int* off, int S, int total, const float* threshold, int H, long long seed,
                 int refine, const double* axis, double min_cos, double* plane, int32_t* count, int32_t* best,
                 uint8_t* inlier, float* dist, void* ws, long long ws_bytes, void* stream);

/* ---- exact neighbours ACROSS two clouds of any size (csrc/knn3_query.hip; grid, cells and bound: csrc/knn3_grid_math.h,
 * build phases and ring loop shared with csrc/knn3_grid.hip through csrc/knn3_grid_build.h) -----------------------------
 * ref (totalR,3) and qry (totalQ,3) fp32, off_r and off_q (S+1) DEVICE int32 row offsets from 0 to totalR / totalQ:
 * segment s of the queries is searched in segment s of the reference.  For query i the result is the k smallest
 * reference points of its segment under the key (d, j) ascending, d = ((x_i-x_j)^2 + (y_i-y_j)^2) + (z_i-z_j)^2, every
 * operation rounded once in fp32, no fma (kg_dist, the expression of pn_knn3_grid_f32), j the index LOCAL to the
 * reference segment.  idx (totalQ,k) int32; dist (totalQ,k) fp32 or NULL: (float) sqrt((double) d).
 *   A reference segment of n_r < k points: idx -1, dist +inf from entry n_r on (an empty one: in every entry).
 *   A reference segment that holds a non-finite coordinate: idx -1, dist NaN in every row of its queries.
 *   A query with a non-finite coordinate: idx -1, dist NaN in that row alone (whatever its reference holds).
 *   A row of qry that no valid segment holds (or whose reference segment does not lie inside 0 .. totalR): -1, NaN.
 * 1 <= k <= 64, any sizes with totalQ * k < 2^31.  All outputs are functions of the inputs alone: the same bits from run
 * to run and for every batching.
 * pn_knn3_query_launches() = 8 stream-ordered kernel launches (four memsets come on top); it needs no GPU: bounding
 * boxes, cells, scan and scatter of the reference; the queries' cells in the reference's grid, scan and scatter of the
 * queries into that cell order; the search, one wave per query, the row written to the query's original position.  No
 * host synchronisation, no cooperative launch, no waiting between workgroups.  Workspace of
 * pn_knn3_query_workspace_bytes(totalR, totalQ, S) bytes, linear in both totals: 32 totalR + 12 totalQ + 44 S + 16
 * (0 for a negative argument).
 * PN_ERR_ARG (before any launch) for k out of range, S < 0, totalR < 0, totalQ < 0, totalQ * k >= 2^31, a NULL off_r,
 * qry, off_q, idx or ws, a NULL ref with totalR > 0, or a workspace that is too small; S == 0 or totalQ == 0 returns 0
 * without a launch; totalR == 0 with queries writes the empty-reference rows in one launch. */
long long pn_knn3_query_workspace_bytes(long long totalR, long long totalQ, int S);
int pn_knn3_query_launches(void);
int pn_knn3_query_f32(const float* ref, const int* off_r, int totalR, const float* qry, const int* off_q, int totalQ,
                      int S, int k, int32_t* idx, float* dist, void* ws, long long ws_bytes, void* stream);

/* ---- k-nearest-sample lifting: per-sample values carried to every point (csrc/knn_lift.hip, definition:
 * csrc/knn_lift_math.h) -------------------------------------------------------------------------------------------------
 * idx, dist (totalQ,k): what pn_knn3_query_f32 wrote for the same off_r, off_q, S and k; an entry is valid when
 * 0 <= idx < n_r of its segment.  One launch each, no workspace, no host synchronisation.
 * pn_knn_interpolate_f32: values (totalR,C) fp32, out (totalQ,C) fp32, C >= 1.  w_j = 1.0 / ((double) dist_j + 1e-8)
 * (PointNet++'s three_interpolate), out_c = (float) ((SUM_j w_j v_jc) / (SUM_j w_j)) over the valid entries in ascending
 * rank, both sums in fp64 from 0.0, every operation rounded once, no fma.  A row with no valid entry or with a NaN in
 * dist, and a row that no valid segment holds, is NaN in every channel.  totalQ * C < 2^39.
 * pn_knn_vote_i32: labels (totalR) int32, out (totalQ) int32: the label that occurs most often among the valid entries
 * with a label >= 0, on equal counts the one whose first occurrence has the lowest rank; none, or a row that no valid
 * segment holds: -1.  Integer arithmetic only.
 * PN_ERR_ARG (before any launch) for k < 1 or k > 64, S < 0, totalR < 0, totalQ < 0, totalQ * k >= 2^31, C < 1,
 * totalQ * C >= 2^39, a NULL off_r, idx, dist (interpolate), off_q or out, or a NULL values / labels with totalR > 0;
 * S == 0 or totalQ == 0 returns 0 without a launch. */
int pn_knn_interpolate_f32(const float* values, const int* off_r, int totalR, const int32_t* idx, const float* dist,
                           const int* off_q, int totalQ, int S, int k, int C, float* out, void* stream);
int pn_knn_vote_i32(const int32_t* labels, const int* off_r, int totalR, const int32_t* idx, const int* off_q,
                    int totalQ, int S, int k, int32_t* out, void* stream);

/* ---- rigid registration of two scans: ICP on the exact grid search (csrc/register.hip, definition:
 * csrc/register_math.h; the search: the kernels of pn_knn3_query_f32, csrc/knn3_query_kernels.h) --------------------------
 * src (totalS,3) the cloud that moves, tgt (totalT,3), normals (totalT,3) or NULL, all fp32; off_s, off_t (S+1) DEVICE
 * int32 row offsets: segment s of the source is registered onto segment s of the target.  mode 0: point to point (Horn's
 * quaternion by a 4 x 4 Jacobi), 1: point to plane, linearised (6 x 6 LDL^T; needs normals, their orientation does not
 * matter).  A pair (moved point, its nearest target point under pn_knn3_query_f32's key, k = 1) is accepted iff
 * dist <= max_dist in fp32 (+inf: every found pair) and, in mode 1, its normal is finite.  init (S,16) fp64 DEVICE
 * row-major 4 x 4 starts, or NULL for the identity.  Every sum is the fixed fp64 tree of csrc/outlier_math.h over tiles of
 * 1 024 source points: all outputs are functions of the segment pair and the arguments alone, the same bits alone, in any
 * batch and in any batch order.
 * Outputs per segment: transform (S,16) fp64 row-major 4 x 4 (its rotation derived from a unit quaternion), iterations
 * int32, status int32 (0 converged: 2 |vec(dq)| <= tol_rot and the step moves the centroid by <= tol_trans; 1 max_iter
 * reached; 2 fewer than 3 (mode 1: 6) accepted pairs; 3 degenerate solve; 4 non-finite target), count int32 and rmse fp64
 * (sqrt(SUM dist^2 / count), NaN for count 0) of one more pairing with the final transform; per source point, optional
 * (NULL): idx int32 LOCAL to the target segment and dist fp32 of that pairing, as pn_knn3_query_f32 defines them.
 * pn_register_launches(max_iter) = 12 + 9 max_iter stream-ordered kernel launches (0 for max_iter outside 1 .. 256; it
 * needs no GPU): the grid of the target is built once (4), one init launch, per iteration move, the query's four
 * launches, mean sums, means, centred sums, solve, and a final evaluation of 7.  The schedule is fixed: no host
 * synchronisation, no cooperative launch, no waiting between workgroups; the workgroups of a segment that has stopped
 * exit at its device flag.  Workspace of pn_register_workspace_bytes(totalS, totalT, S) bytes:
 * pn_knn3_query_workspace_bytes(totalT, totalS, S) + 20 totalS + 236 (totalS / 1024 + S) + 120 S (0 for a negative
 * argument or a total of 2^31 or more).
 * PN_ERR_ARG (before any launch) for S < 0, totalS < 0, totalT < 0, mode outside 0 .. 1, mode 1 without normals, max_iter
 * outside 1 .. 256, max_dist < 0 or NaN, tol_rot or tol_trans < 0 or NaN, a NULL off_s, off_t, transform, iterations,
 * status, count, rmse or ws, a NULL src with totalS > 0 or tgt with totalT > 0, or a workspace that is too small; S == 0
 * returns 0 without a launch.
 * pn_rigid_apply_f32: the move step alone, the same bits: out (totalS,3) fp32 = (float)(((R00 x + R01 y) + R02 z) + t0)
 * ... in fp64 with R derived from the unit quaternion of transform's (S,16 fp64, DEVICE) rotation block.  One launch;
 * PN_ERR_ARG for S < 0, totalS < 0 or a NULL pointer; S == 0 or totalS == 0 returns 0 without a launch. */
long long pn_register_workspace_bytes(long long totalS, long long totalT, int S);
int pn_register_launches(int max_iter);
int pn_register_f32(const float* src, const int* off_s, int totalS, const float* tgt, const int* off_t, int totalT,
                    const float* normals, int S, int mode, float max_dist, int max_iter, double tol_rot,
                    double tol_trans, const double* init, double* transform, int32_t* iterations, int32_t* status,
                    int32_t* count, double* rmse, int32_t* idx, float* dist, void* ws, long long ws_bytes, void* stream);
int pn_rigid_apply_f32(const float* src, const int* off_s, int S, int totalS, const double* transform, float* out,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PARSENET_HIP_H */
