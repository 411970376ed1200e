// Point coverage of the fitted primitives (p-coverage) for gfx950.
//
// Replaces src/eval_utils.py:103-127 (p_coverage): one ResidualLoss(one_side=True, reduce=False) call per primitive
// over the whole cloud, a stack of the S results of N floats and a minimum — S launches of small tensor expressions
// plus a Chamfer launch per spline — by ONE launch for all primitives of all shapes of a ragged batch.
//
// pn_point_primitive_min_f32 — a workgroup owns CV_THREADS consecutive points of one shape (flat tile table
// tile -> (shape, first point), built on the host), one point per lane, and walks the shape's primitives in index
// order with the running minimum and its index in registers.  The loop counter, the type id and the parameter row
// are workgroup-uniform, so they come through scalar loads and the type switch is a scalar branch.
//   analytic (plane, sphere, cylinder, cone): residual_point_value of fit_math.h with sqrt_flag = 1 — the value
//       part of the arithmetic the batched fitting stage uses, fp32.
//   sampled (the two spline kinds): the primitive's sample cloud goes through LDS in tiles of CV_TILE points
//       (structure of arrays, read back as ds_read_b128 broadcasts: three LDS reads per four samples).  The nearest
//       sample is DECIDED with the Chamfer kernel's chain d = ((dx*dx + dy*dy) + dz*dz), every operation rounded
//       once, strictly smaller wins (the first sample on equal values), and its squared distance is then
//       RE-EVALUATED as ((dx*dx + dz*dz) + dy*dy): chamfer_distance_single_shape reports the tensor expression
//       torch.sum((a - b) ** 2, 2) at the kernel's arg-min, and the tensor library's GPU reduction adds the three
//       terms in that order.  That order is an observation about the tensor library, not a contract of it:
//       tools/sum3_order_probe.py compares the expression on the GPU with the three association orders and their
//       contracted forms at 1 to 100 000 rows (profiles/sum3_order.txt: this order reproduces every row, no other
//       candidate does), and tests/test_pcover_gpu.py::test_spline_only_shape_is_the_chamfer_chain pins it bit for
//       bit.  If a later tensor library reduces in another order, that test fails and this line follows the probe.
//       guard_sqrt is applied once per spline, to that value: sqrtf and the clamp at 1e-5 are monotone
//       (non-decreasing) and correctly rounded, so guarding the smallest squared distance equals taking the
//       smallest guarded root bit for bit — the value
//       chamfer_distance_single_shape(one_side=True, sqrt=True, reduce=False) returns.
// A primitive replaces the running minimum only when strictly smaller: on equal values the lowest index wins.  A
// NaN distance is kept (first NaN wins), as torch.min over the stack propagates it.  For a point with a NaN
// coordinate the analytic arithmetic yields NaN by itself; a sampled primitive, whose comparisons all fail then,
// re-evaluates at its sample 0 and so yields NaN too, as the tensor expression does.
// No atomics, no scratch, vector stores only; a point's result depends on its own lane alone, so it does not depend
// on the launch geometry.
//
// Tile sizes.  The work of a lane is serial (every sample of every spline of its shape), so the kernel's time is one
// lane's time as long as no SIMD holds more than one wave: at the workload's 10 000 points, 64-point tiles give 157
// one-wave workgroups that spread over 157 of the 256 CUs (a batch of 4: 628, still about one wave per SIMD), where
// 256-point tiles would put the same waves on 40 CUs for no shorter a chain.  One wave per workgroup also makes the
// two barriers around the staging free.  A lone wave keeps its SIMD's VALU busy (a dependent wave64 instruction
// issues back to back), and per four samples it issues 3 ds_read_b128 against 36 VALU operations, far below the
// LDS rate a single wave reaches.  CV_TILE = 1024 samples (12 KB) holds the 900 / 930 samples of a spline in one
// tile, so a spline costs one staging pass; 12 KB per one-wave workgroup allows 13 workgroups per CU.
#include "common.h"
#include "fit_math.h"

#define CV_THREADS 64
#define CV_TILE 1024    // samples per LDS tile (12 KB), a multiple of 4
#define CV_SAMPLED 4    // type ids >= CV_SAMPLED: distance to a sample cloud (0..3: FB_PLANE .. FB_CONE)

__device__ static inline float cv_dist(float qx, float qy, float qz, float cx, float cy, float cz) {
  const float dx = __fsub_rn(qx, cx);
  const float dy = __fsub_rn(qy, cy);
  const float dz = __fsub_rn(qz, cz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

__global__ __launch_bounds__(CV_THREADS) void pn_point_primitive_min_kernel(
    const float* __restrict__ points, const int* __restrict__ pt_off, const int* __restrict__ prim_off,
    const int* __restrict__ prim_type, const float* __restrict__ prim_par, const float* __restrict__ samp,
    const int* __restrict__ samp_off, const int* __restrict__ tile_shape, const int* __restrict__ tile_first,
    float* __restrict__ dmin, int* __restrict__ arg) {
  __shared__ __attribute__((aligned(16))) float sx[CV_TILE];
  __shared__ __attribute__((aligned(16))) float sy[CV_TILE];
  __shared__ __attribute__((aligned(16))) float sz[CV_TILE];
  const int b = tile_shape[blockIdx.x];
  const int p = tile_first[blockIdx.x] + threadIdx.x;
  const bool valid = p < pt_off[b + 1];
  float qx = 0.f, qy = 0.f, qz = 0.f;   // a lane past the end of the shape helps with the staging and stores nothing
  if (valid) {
    const float* q = points + 3 * (size_t)p;
    qx = q[0], qy = q[1], qz = q[2];
  }
  const float inf = __builtin_inff();
  const int s0 = prim_off[b], s1 = prim_off[b + 1];
  float best = inf;
  int besti = -1;   // a shape without primitives: (inf, -1)
  for (int s = s0; s < s1; ++s) {
    const int type = prim_type[s];
    float d;
    if (type < CV_SAMPLED) {
      d = residual_point_value(type, qx, qy, qz, prim_par + (size_t)s * FB_NPAR, 1);
    } else {
      const int c0 = samp_off[s], nc = samp_off[s + 1] - c0;
      float m = inf;
      int j = -1;
      for (int base = 0; base < nc; base += CV_TILE) {
        const int n = min(CV_TILE, nc - base);
        const int n4 = (n + 3) & ~3;   // <= CV_TILE; the padding is staged as inf: d = inf, never the minimum
        __syncthreads();               // the reads of the previous tile are done
        for (int t = threadIdx.x; t < n4; t += CV_THREADS) {
          float x = inf, y = inf, z = inf;
          if (t < n) {
            const float* c = samp + 3 * ((size_t)c0 + base + t);
            x = c[0], y = c[1], z = c[2];
          }
          sx[t] = x, sy[t] = y, sz[t] = z;
        }
        __syncthreads();
        for (int t = 0; t < n4; t += 4) {
          const float4 X = *(const float4*)&sx[t];
          const float4 Y = *(const float4*)&sy[t];
          const float4 Z = *(const float4*)&sz[t];
          const float d0 = cv_dist(qx, qy, qz, X.x, Y.x, Z.x);
          const float d1 = cv_dist(qx, qy, qz, X.y, Y.y, Z.y);
          const float d2 = cv_dist(qx, qy, qz, X.z, Y.z, Z.z);
          const float d3 = cv_dist(qx, qy, qz, X.w, Y.w, Z.w);
          if (d0 < m) m = d0, j = base + t;
          if (d1 < m) m = d1, j = base + t + 1;
          if (d2 < m) m = d2, j = base + t + 2;
          if (d3 < m) m = d3, j = base + t + 3;
        }
      }
      if (nc > 0) {   // (j < nc: a padded sample has d = inf, never < m)
        // j < 0: no distance compared smaller than inf, i.e. every one was NaN or inf (a NaN or infinite coordinate).
        // Sample 0 then gives the NaN or inf the tensor expression reports, instead of a silent inf.
        const float* c = samp + 3 * ((size_t)c0 + max(j, 0));
        const float dx = __fsub_rn(qx, c[0]), dy = __fsub_rn(qy, c[1]), dz = __fsub_rn(qz, c[2]);
        m = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dz, dz)), __fmul_rn(dy, dy));   // the tensor sum's order
      }
      d = sqrtf(fclampv(m, 1e-5f, inf));   // guard_sqrt once per spline (see the head of the file)
    }
    if (d < best || (d != d && best == best)) {
      best = d;
      besti = s - s0;
    }
  }
  if (valid) {
    dmin[p] = best;
    arg[p] = besti;
  }
}

extern "C" int pn_point_primitive_min_tile(void) { return CV_THREADS; }

extern "C" int pn_point_primitive_min_f32(const float* points, const int* pt_off, const int* prim_off,
                                          const int* prim_type, const float* prim_par, const float* samp,
                                          const int* samp_off, const int* tile_shape, const int* tile_first, int B,
                                          int total_tiles, float* dmin, int* arg, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PN_CHECK_ARG(points && pt_off && prim_off && prim_type && prim_par && samp_off && tile_shape && tile_first &&
                   dmin && arg,
               "pn_point_primitive_min_f32: null pointer");
  PN_CHECK_ARG(B > 0 && total_tiles > 0, "pn_point_primitive_min_f32: empty batch (B=%d tiles=%d)", B, total_tiles);
  PN_PROF("point_primitive_min", stream);
  hipLaunchKernelGGL(pn_point_primitive_min_kernel, dim3(total_tiles), dim3(CV_THREADS), 0, stream, points, pt_off,
                     prim_off, prim_type, prim_par, samp, samp_off, tile_shape, tile_first, dmin, arg);
  PN_CHECK_LAUNCH();
  return PN_OK;
}
