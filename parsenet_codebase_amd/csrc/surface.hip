// Trimmed surfaces of the evaluation mode for gfx950.
//
// Replaces, for ALL fitted segments of a shape at once,
//   src/fitting_utils.py:240-273 (create_grid: the centre of every cell of a regular U x V grid on the fitted surface,
//       kept when some point of the segment's up-sampled cloud lies within `thres` of it — a Python loop over up to
//       14 161 cells of an (1, P) distance row each),
//   src/utils.py:123-178 (sample_mesh / triangle_area_multi on the two-triangle tessellation of the kept cells,
//       src/fitting_utils.py:276-303).
//
// pn_grid_occupancy_ragged_f32 — a THRESHOLD query, not a minimum.  A workgroup owns 256 cells of one segment (prefix
// table of cell tiles over the segments), one cell per lane, and walks the segment's cloud through LDS tiles of
// OC_TILE points (structure of arrays, read back as ds_read_b128 broadcasts: three LDS reads per four points).  The
// distance is the Chamfer kernel's chain d = ((dx*dx + dy*dy) + dz*dz), every operation rounded once, and the
// centre (((v00 + v01) + v10) + v11) * 0.25f, so the decision sqrtf(min d) < thres is the one the tensor
// expression takes, bit for bit:  sqrtf is monotone, so  sqrtf(min d) < thres  <=>  some d <= T  with T the largest
// float whose root is below thres (oc_limit, found once per workgroup).  A lane stops at its first hit, a wave skips the
// rest of the cloud once its 64 cells are decided (vote after every 16 points), and the workgroup leaves the loop when
// all four waves have.
//
// pn_trimesh_area_f64 / pn_trimesh_sample_f64 — float64 like numpy: the areas of the triangles of the kept cells,
// and area-weighted samples from caller-supplied uniforms (numpy's stream stays on the host so that a seeded run
// consumes the reference's draws).
#include "common.h"

#define OC_THREADS 256
#define OC_TILE 1024     // cloud points per LDS tile (12 KB)
#define OC_CHUNK 16      // points between two votes

__device__ static inline float oc_dist(float qx, float qy, float qz, float cx, float cy, float cz) {
  const float dx = __fsub_rn(qx, cx);
  const float dy = __fsub_rn(qy, cy);
  const float dz = __fsub_rn(qz, cz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// largest float t >= 0 with sqrtf(t) < th, or -1 when there is none (th <= 0 or NaN): d <= t <=> sqrtf(d) < th
__device__ static inline float oc_limit(float th) {
  if (!(th > 0.f)) return -1.f;
  const float fmax = __uint_as_float(0x7f7fffffu);
  float t = __fmul_rn(th, th);
  if (!(t <= fmax)) t = fmax;
  while (t > 0.f && !(sqrtf(t) < th)) t = __uint_as_float(__float_as_uint(t) - 1u);
  while (t < fmax) {
    const float up = __uint_as_float(__float_as_uint(t) + 1u);
    if (!(sqrtf(up) < th)) break;
    t = up;
  }
  return t;   // (t == 0: sqrtf(0) = 0 < th holds)
}

// the last s with off[s] <= x (off ascending, off[0] = 0 <= x)
__device__ static inline int sf_find(const int* __restrict__ off, int n, int x) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= x)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(OC_THREADS) void pn_grid_occupancy_kernel(
    const float* __restrict__ grid, const int* __restrict__ size_u, const int* __restrict__ size_v,
    const int* __restrict__ voff, const float* __restrict__ cloud, const int* __restrict__ coff,
    const float* __restrict__ thres, const int* __restrict__ tile_off, const int* __restrict__ cell_off, int S,
    unsigned char* __restrict__ mask) {
  __shared__ __attribute__((aligned(16))) float sx[OC_TILE];
  __shared__ __attribute__((aligned(16))) float sy[OC_TILE];
  __shared__ __attribute__((aligned(16))) float sz[OC_TILE];
  const int s = sf_find(tile_off, S, blockIdx.x);
  const int sv = size_v[s];
  const int ncell = (size_u[s] - 1) * (sv - 1);
  const int cell = (blockIdx.x - tile_off[s]) * OC_THREADS + threadIdx.x;
  const bool valid = cell < ncell;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (valid) {
    const int i = cell / (sv - 1), j = cell - i * (sv - 1);
    const float* g0 = grid + 3 * ((size_t)voff[s] + (size_t)i * sv + j);
    const float* g1 = g0 + 3 * (size_t)sv;
    qx = __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(g0[0], g0[3]), g1[0]), g1[3]), 0.25f);
    qy = __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(g0[1], g0[4]), g1[1]), g1[4]), 0.25f);
    qz = __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(g0[2], g0[5]), g1[2]), g1[5]), 0.25f);
  }
  const float limit = oc_limit(thres[s]);
  const int p0 = coff[s], np = coff[s + 1] - p0;
  const float inf = __builtin_inff();
  bool hit = false;
  bool open = valid;   // the lane's cell is still undecided
  for (int base = 0; base < np; base += OC_TILE) {
    for (int t = threadIdx.x; t < OC_TILE; t += OC_THREADS) {
      const int p = base + t;
      float x = inf, y = inf, z = inf;   // padding: d = inf, never <= limit
      if (p < np) {
        const float* c = cloud + 3 * ((size_t)p0 + p);
        x = c[0], y = c[1], z = c[2];
      }
      sx[t] = x, sy[t] = y, sz[t] = z;
    }
    __syncthreads();
    if (__ballot(open)) {   // wave-uniform: a wave whose cells are all decided only helps with the staging
      const int n = min(OC_TILE, np - base);
      for (int t = 0; t < n; t += OC_CHUNK) {   // OC_TILE is a multiple of OC_CHUNK: the reads stay inside the tile
        float m = inf;
#pragma unroll
        for (int k = 0; k < OC_CHUNK; k += 4) {
          const float4 X = *(const float4*)&sx[t + k];
          const float4 Y = *(const float4*)&sy[t + k];
          const float4 Z = *(const float4*)&sz[t + k];
          m = fminf(m, oc_dist(qx, qy, qz, X.x, Y.x, Z.x));
          m = fminf(m, oc_dist(qx, qy, qz, X.y, Y.y, Z.y));
          m = fminf(m, oc_dist(qx, qy, qz, X.z, Y.z, Z.z));
          m = fminf(m, oc_dist(qx, qy, qz, X.w, Y.w, Z.w));
        }
        if (open && m <= limit) {
          hit = true;
          open = false;
        }
        if (!__ballot(open)) break;
      }
    }
    // (also the barrier in front of the next tile's staging)
    if (!__syncthreads_or(open ? 1 : 0)) break;
  }
  if (valid) mask[(size_t)cell_off[s] + cell] = hit ? 1 : 0;
}

extern "C" int pn_grid_occupancy_ragged_f32(const float* grid, const int* size_u, const int* size_v, const int* voff,
                                            const float* cloud, const int* coff, const float* thres,
                                            const int* tile_off, const int* cell_off, int S, int total_tiles,
                                            unsigned char* mask, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PN_CHECK_ARG(grid && size_u && size_v && voff && cloud && coff && thres && tile_off && cell_off && mask,
               "pn_grid_occupancy_ragged_f32: null pointer");
  PN_CHECK_ARG(S > 0 && total_tiles > 0, "pn_grid_occupancy_ragged_f32: empty batch (S=%d tiles=%d)", S, total_tiles);
  PN_PROF("grid_occupancy", stream);
  hipLaunchKernelGGL(pn_grid_occupancy_kernel, dim3(total_tiles), dim3(OC_THREADS), 0, stream, grid, size_u, size_v,
                     voff, cloud, coff, thres, tile_off, cell_off, S, mask);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

extern "C" int pn_grid_occupancy_tile(void) { return OC_THREADS; }

// ---- triangles of the kept cells ------------------------------------------------------------------------------------
// face f of mesh m: kept cell cells[f >> 1] (row-major index into the (U-1) x (V-1) cells of the mesh's grid), triangle
// f & 1 of  (i,j),(i+1,j),(i+1,j+1)  then  (i,j),(i+1,j+1),(i,j+1)  (tessalate_points_fast's order).
__device__ static inline void sf_triangle(const float* __restrict__ grid, int voff, int sv, int cell, int second,
                                          double v1[3], double v2[3], double v3[3]) {
  const int i = cell / (sv - 1), j = cell - i * (sv - 1);
  const float* a = grid + 3 * ((size_t)voff + (size_t)i * sv + j);
  const float* b = a + 3 * (size_t)sv;   // (i+1, j)
  const float* p2 = second ? b + 3 : b;
  const float* p3 = second ? a + 3 : b + 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) v1[k] = (double)a[k], v2[k] = (double)p2[k], v3[k] = (double)p3[k];
}

__global__ __launch_bounds__(256) void pn_trimesh_area_kernel(const float* __restrict__ grid,
                                                              const int* __restrict__ voff,
                                                              const int* __restrict__ size_v,
                                                              const int* __restrict__ face_off,
                                                              const int* __restrict__ cells, int M, int total,
                                                              double* __restrict__ area) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= total) return;
  const int m = sf_find(face_off, M, f);
  double v1[3], v2[3], v3[3];
  sf_triangle(grid, voff[m], size_v[m], cells[f >> 1], f & 1, v1, v2, v3);
  const double ax = v2[0] - v1[0], ay = v2[1] - v1[1], az = v2[2] - v1[2];
  const double bx = v3[0] - v1[0], by = v3[1] - v1[1], bz = v3[2] - v1[2];
  const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  area[f] = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

extern "C" int pn_trimesh_area_f64(const float* grid, const int* voff, const int* size_v, const int* face_off,
                                   const int* cells, int M, int total_faces, double* area, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PN_CHECK_ARG(grid && voff && size_v && face_off && cells && area, "pn_trimesh_area_f64: null pointer");
  PN_CHECK_ARG(M > 0 && total_faces > 0, "pn_trimesh_area_f64: no faces");
  hipLaunchKernelGGL(pn_trimesh_area_kernel, dim3(pn_cdiv(total_faces, 256)), dim3(256), 0, stream, grid, voff,
                     size_v, face_off, cells, M, total_faces, area);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

__global__ __launch_bounds__(256) void pn_trimesh_sample_kernel(
    const float* __restrict__ grid, const int* __restrict__ voff, const int* __restrict__ size_v,
    const int* __restrict__ face_off, const int* __restrict__ cells, const double* __restrict__ cdf,
    const int* __restrict__ samp_off, const double* __restrict__ pick, const double* __restrict__ uu,
    const double* __restrict__ vv, int M, int total, float* __restrict__ out, int* __restrict__ face) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= total) return;
  const int m = sf_find(samp_off, M, k);
  const int f0 = face_off[m], nf = face_off[m + 1] - f0;
  // first face whose cdf exceeds the pick (numpy's searchsorted(side="right") inside random.choice)
  const double r = pick[k];
  int lo = 0, hi = nf;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[f0 + mid] <= r)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo > nf - 1) lo = nf - 1;
  const int f = f0 + lo;
  double v1[3], v2[3], v3[3];
  sf_triangle(grid, voff[m], size_v[m], cells[f >> 1], f & 1, v1, v2, v3);
  double u = uu[k], v = vv[k];
  if (u + v > 1.0) {
    u = 1.0 - u;
    v = 1.0 - v;
  }
  const double w = 1.0 - (u + v);
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * (size_t)k + c] = (float)((v1[c] * u + v2[c] * v) + w * v3[c]);
  if (face) face[k] = lo;
}

extern "C" int pn_trimesh_sample_f64(const float* grid, const int* voff, const int* size_v, const int* face_off,
                                     const int* cells, const double* cdf, const int* samp_off, const double* pick,
                                     const double* u, const double* v, int M, int total_samples, float* out,
                                     int* face, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PN_CHECK_ARG(grid && voff && size_v && face_off && cells && cdf && samp_off && pick && u && v && out,
               "pn_trimesh_sample_f64: null pointer");
  PN_CHECK_ARG(M > 0 && total_samples > 0, "pn_trimesh_sample_f64: nothing to sample");
  PN_PROF("trimesh_sample", stream);
  hipLaunchKernelGGL(pn_trimesh_sample_kernel, dim3(pn_cdiv(total_samples, 256)), dim3(256), 0, stream, grid, voff,
                     size_v, face_off, cells, cdf, samp_off, pick, u, v, M, total_samples, out, face);
  PN_CHECK_LAUNCH();
  return PN_OK;
}
