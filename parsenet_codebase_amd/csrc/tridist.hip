// Exact distance from points to the trimmed surfaces (the triangles of their kept cells) for gfx950.
//
// The evaluation mode measures a reconstruction by the distance from every input point to the nearest of 10 000
// SAMPLES of the surfaces; this is the limit of that figure for infinitely many samples: the distance to the nearest
// triangle itself.  Two launches for all surfaces of all shapes of a batch.
//
// pn_trimesh_records_f32 — one thread per triangle SLOT.  Shape b owns the slots slot_off[b] .. slot_off[b+1], its
// kept triangles in TrimmedSurface.triangles() order (the faces shape_face[b] .. shape_face[b+1] of the mesh tables
// pn_trimesh_area_f64 reads) padded to a multiple of TM_GROUP with records no finite point is nearest to.  A slot's
// record is the 16 floats of tm_make (tri_math.h), structure of arrays: rec[k * total_slots + slot].  The TM_GROUP
// lanes of a group (consecutive triangles of a grid are neighbours in space) reduce the bounding box of their
// vertices and the largest distance from its centre by shuffles and write one sphere (cx, cy, cz, r) per group.
//
// pn_trimesh_point_dist_f32 — a workgroup of W waves (W = blockDim / 64: 4, 8 or 16, chosen by the caller from the
// number of point tiles so that the grid fills the machine: 157 tiles of a 10 000-point cloud are 2 512 waves at
// W = 16 on 1 024 SIMDs) owns 64 consecutive points of one shape (flat tile table tile -> (shape, first point) as
// in cover.hip).  EVERY wave holds the same 64 points, one per lane.  The workgroup streams the shape's records
// through LDS in tiles of 64 W triangles (W x 4 KB, the 16 arrays side by side), and wave w takes the 64 triangles
// w of every tile — interleaved triangle tiles for the same points —, reading them back as ds_read_b64 broadcasts
// (sixteen reads per two triangles: four at a time would need more than the 128 registers a 16-wave workgroup has) and keeping its running minimum and the face in registers; the W waves merge
// their minima through LDS at the end, in wave order.  A triangle replaces the minimum only when strictly nearer and
// a wave meets its faces in ascending order, the merge prefers the lower face on equal values: the lowest face id
// wins, whatever W is.  No atomics on results, no floating-point atomics at all: a point's (distance, face) is the
// lexicographic minimum over the shape's triangles of values that depend on the point and the triangle alone, so
// it is the same bits from run to run and for every W.
// Pruning (prune != 0).  First every lane finds an upper bound of its result, the smallest tm_upper2 over the
// shape's spheres (the waves share the spheres and merge through LDS).  Then, in front of each group of TM_GROUP
// triangles, a wave evaluates tm_lower2 against the group's sphere and skips the group when the bound is strictly
// greater than min(running minimum, upper bound) in every lane (one ballot).  Both bounds are certified against the
// COMPUTED distances (tri_math.h), so a skipped triangle can neither be the minimum nor tie with it: values and faces
// are bit-identical with pruning on and off.  The vote needs all 64 points to be far from the group, so the caller
// orders the points along a space-filling curve first (surface.point_surface_distance).  `skipped`, optional, counts
// the skipped groups (one integer atomic add per wave).
// Lanes past the end of the shape take the shape's last point, so that they vote like a neighbour, and store nothing.
#include "common.h"
#include "tri_math.h"

#define TD_POINTS 64      // points per workgroup, one per lane
#define TD_WAVE_TRIS 64   // triangles of an LDS tile per wave (8 groups)
#define TD_MAX_WAVES 16

// the last s with off[s] <= x (off ascending, off[0] <= x)
__device__ static inline int td_find(const int* __restrict__ off, int n, int x) {
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

__global__ __launch_bounds__(256) void pn_trimesh_records_kernel(
    const float* __restrict__ grid, const int* __restrict__ voff, const int* __restrict__ size_v,
    const int* __restrict__ face_off, const int* __restrict__ cells, int M, const int* __restrict__ shape_face,
    const int* __restrict__ slot_off, int B, int total_slots, float* __restrict__ rec, float4* __restrict__ sph) {
  const int slot = blockIdx.x * 256 + threadIdx.x;   // (no early return: every lane takes part in the shuffles)
  const bool in = slot < total_slots;
  bool real = false;
  float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (in) {
    const int b = td_find(slot_off, B, slot);
    const int i = slot - slot_off[b];
    real = i < shape_face[b + 1] - shape_face[b];
    if (real) {
      // face f of mesh m: kept cell cells[f >> 1], triangle f & 1 of (i,j),(i+1,j),(i+1,j+1) then (i,j),(i+1,j+1),(i,j+1)
      const int f = shape_face[b] + i;
      const int m = td_find(face_off, M, f);
      const int sv = size_v[m], cell = cells[f >> 1];
      const int r = cell / (sv - 1), c = cell - r * (sv - 1);
      const float* a = grid + 3 * ((size_t)voff[m] + (size_t)r * sv + c);
      const float* d = a + 3 * (size_t)sv;   // (r+1, c)
      const float* p2 = (f & 1) ? d + 3 : d;
      const float* p3 = (f & 1) ? a + 3 : d + 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = a[k], v[3 + k] = p2[k], v[6 + k] = p3[k];
    }
  }
  const TmTri t = real ? tm_make(v, v + 3, v + 6) : tm_pad();
  if (in) {
    const float f[TM_NREC] = {t.ax, t.ay, t.az, t.ux, t.uy, t.uz, t.vx, t.vy, t.vz, t.nx, t.ny, t.nz,
                              t.iu, t.iv, t.iw, t.in};
#pragma unroll
    for (int k = 0; k < TM_NREC; ++k) rec[(size_t)k * total_slots + slot] = f[k];
  }
  // the group's sphere: bounding box of the vertices of its real triangles, then the farthest vertex from its centre
  const float inf = __builtin_inff();
  float lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = real ? fminf(fminf(v[k], v[3 + k]), v[6 + k]) : inf;
    hi[k] = real ? fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]) : -inf;
#pragma unroll
    for (int o = 1; o < TM_GROUP; o <<= 1) {
      lo[k] = fminf(lo[k], __shfl_xor(lo[k], o, 64));
      hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o, 64));
    }
  }
  const float cx = tm_centre(lo[0], hi[0]), cy = tm_centre(lo[1], hi[1]), cz = tm_centre(lo[2], hi[2]);
  float r2 = 0.f;
  if (real) {
#pragma unroll
    for (int k = 0; k < 9; k += 3) r2 = fmaxf(r2, tm_sq(v[k], v[k + 1], v[k + 2], cx, cy, cz));
  }
#pragma unroll
  for (int o = 1; o < TM_GROUP; o <<= 1) r2 = fmaxf(r2, __shfl_xor(r2, o, 64));
  // (a group's first slot is always a real triangle: a shape is padded to the next multiple of TM_GROUP only)
  if (in && (slot & (TM_GROUP - 1)) == 0) sph[slot / TM_GROUP] = make_float4(cx, cy, cz, tm_radius(r2));
}

extern "C" int pn_trimesh_group(void) { return TM_GROUP; }

extern "C" int pn_trimesh_records_f32(const float* grid, const int* voff, const int* size_v, const int* face_off,
                                      const int* cells, int M, const int* shape_face, const int* slot_off, int B,
                                      int total_slots, float* rec, float* sph, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PN_CHECK_ARG(grid && voff && size_v && face_off && cells && shape_face && slot_off && rec && sph,
               "pn_trimesh_records_f32: null pointer");
  PN_CHECK_ARG(M > 0 && B > 0 && total_slots > 0 && total_slots % TM_GROUP == 0,
               "pn_trimesh_records_f32: M=%d B=%d total_slots=%d (a positive multiple of %d)", M, B, total_slots,
               TM_GROUP);
  PN_CHECK_ARG(((uintptr_t)sph & 15) == 0, "pn_trimesh_records_f32: sph must be 16-byte aligned");
  PN_PROF("trimesh_records", stream);
  hipLaunchKernelGGL(pn_trimesh_records_kernel, dim3(pn_cdiv(total_slots, 256)), dim3(256), 0, stream, grid, voff,
                     size_v, face_off, cells, M, shape_face, slot_off, B, total_slots, rec, (float4*)sph);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

__device__ static inline TmTri td_tri(const float2* r, int k) {
  TmTri t;
#define TD_PICK(q) (k == 0 ? (q).x : (q).y)
  t.ax = TD_PICK(r[0]), t.ay = TD_PICK(r[1]), t.az = TD_PICK(r[2]);
  t.ux = TD_PICK(r[3]), t.uy = TD_PICK(r[4]), t.uz = TD_PICK(r[5]);
  t.vx = TD_PICK(r[6]), t.vy = TD_PICK(r[7]), t.vz = TD_PICK(r[8]);
  t.nx = TD_PICK(r[9]), t.ny = TD_PICK(r[10]), t.nz = TD_PICK(r[11]);
  t.iu = TD_PICK(r[12]), t.iv = TD_PICK(r[13]), t.iw = TD_PICK(r[14]), t.in = TD_PICK(r[15]);
#undef TD_PICK
  return t;
}

__global__ __launch_bounds__(TD_MAX_WAVES * 64) void pn_trimesh_point_dist_kernel(
    const float* __restrict__ points, const int* __restrict__ pt_off, const int* __restrict__ slot_off,
    const float* __restrict__ rec, int total_slots, const float4* __restrict__ sph,
    const int* __restrict__ tile_shape, const int* __restrict__ tile_first, int prune, float* __restrict__ dist2,
    int* __restrict__ face, unsigned long long* __restrict__ skipped) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [TM_NREC][W * 64]; afterwards the merge area
  const int W = blockDim.x >> 6;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int stride = W * TD_WAVE_TRIS;
  const int b = tile_shape[blockIdx.x];
  const int pend = pt_off[b + 1];
  const int p = tile_first[blockIdx.x] + lane;
  const bool valid = p < pend;
  const float* q = points + 3 * (size_t)(valid ? p : pend - 1);
  const float qx = q[0], qy = q[1], qz = q[2];
  const int s0 = slot_off[b], n = slot_off[b + 1] - s0;   // multiples of TM_GROUP
  const float inf = __builtin_inff();
  float ub2 = inf;
  if (prune) {
    const float4* sp = sph + s0 / TM_GROUP;
    for (int g = w; g < n / TM_GROUP; g += W) {
      const float4 s = sp[g];
      ub2 = fminf(ub2, tm_upper2(qx, qy, qz, s.x, s.y, s.z, s.w));
    }
    lds[threadIdx.x] = ub2;
    __syncthreads();
    for (int k = 0; k < W; ++k) ub2 = fminf(ub2, lds[k * 64 + lane]);
    __syncthreads();
  }
  float best = inf;
  int besti = 0x7fffffff;
  unsigned nskip = 0;
  for (int base = 0; base < n; base += stride) {
    const int t = base + (int)threadIdx.x;
    if (t < n) {   // (slots past the shape's end are never read: the loops below stop at n)
#pragma unroll
      for (int k = 0; k < TM_NREC; ++k) lds[k * stride + threadIdx.x] = rec[(size_t)k * total_slots + s0 + t];
    }
    __syncthreads();
    const int wb = base + w * TD_WAVE_TRIS;
    for (int g = 0; g < TD_WAVE_TRIS; g += TM_GROUP) {
      if (wb + g >= n) break;   // wave-uniform
      if (prune) {
        const float4 s = sph[(s0 + wb + g) / TM_GROUP];
        const float lb2 = tm_lower2(qx, qy, qz, s.x, s.y, s.z, s.w);
        if (!__ballot(lb2 <= fminf(best, ub2))) {
          ++nskip;
          continue;
        }
      }
#pragma unroll 1
      for (int h = 0; h < TM_GROUP; h += 2) {   // (unrolled, the compiler loads the whole group first and spills)
        float2 r[TM_NREC];
#pragma unroll
        for (int k = 0; k < TM_NREC; ++k) r[k] = *(const float2*)&lds[k * stride + w * TD_WAVE_TRIS + g + h];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const float d = tm_dist2(qx, qy, qz, td_tri(r, k));
          if (d < best) best = d, besti = wb + g + h + k;
        }
      }
    }
    __syncthreads();
  }
  // merge the waves' minima in wave order: strictly smaller, or equal with the lower face
  float* md = lds;
  int* mi = (int*)(lds + blockDim.x);
  md[threadIdx.x] = best;
  mi[threadIdx.x] = besti;
  __syncthreads();
  if (w == 0 && valid) {
    for (int k = 1; k < W; ++k) {
      const float d = md[k * 64 + lane];
      const int i = mi[k * 64 + lane];
      if (d < best || (d == best && i < besti)) best = d, besti = i;
    }
    dist2[p] = best;
    face[p] = besti;
  }
  if (skipped && lane == 0 && nskip) atomicAdd(skipped, (unsigned long long)nskip);
}

extern "C" int pn_trimesh_point_dist_tile(void) { return TD_POINTS; }

extern "C" int pn_trimesh_point_dist_f32(const float* points, const int* pt_off, const int* slot_off,
                                         const float* rec, int total_slots, const float* sph, const int* tile_shape,
                                         const int* tile_first, int B, int total_tiles, int waves, int prune,
                                         float* dist2, int* face, unsigned long long* skipped, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PN_CHECK_ARG(points && pt_off && slot_off && rec && sph && tile_shape && tile_first && dist2 && face,
               "pn_trimesh_point_dist_f32: null pointer");
  PN_CHECK_ARG(B > 0 && total_tiles > 0 && total_slots > 0 && total_slots % TM_GROUP == 0,
               "pn_trimesh_point_dist_f32: empty batch (B=%d tiles=%d slots=%d)", B, total_tiles, total_slots);
  PN_CHECK_ARG(waves == 4 || waves == 8 || waves == 16, "pn_trimesh_point_dist_f32: waves must be 4, 8 or 16, got %d",
               waves);
  PN_CHECK_ARG(((uintptr_t)sph & 15) == 0, "pn_trimesh_point_dist_f32: sph must be 16-byte aligned");
  PN_PROF("trimesh_point_dist", stream);
  const size_t lds_bytes = (size_t)waves * TD_WAVE_TRIS * TM_NREC * sizeof(float);   // 16 / 32 / 64 KB
  hipLaunchKernelGGL(pn_trimesh_point_dist_kernel, dim3(total_tiles), dim3(waves * 64), lds_bytes, stream, points,
                     pt_off, slot_off, rec, total_slots, (const float4*)sph, tile_shape, tile_first, prune, dist2,
                     face, skipped);
  PN_CHECK_LAUNCH();
  return PN_OK;
}
