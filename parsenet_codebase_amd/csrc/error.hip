// Thread-local error string behind the C ABI (include/parsenet_hip.h).
#include "common.h"
#include <stdarg.h>

static thread_local char g_err[512] = "";

void pn_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* pn_last_error(void) { return g_err; }

// 2: edge-conv backward takes a workspace, mean-shift backward reduces its partial sums itself,
//    bf16 x 3 mean-shift entry points
// 19: mean-shift at embedding widths 32 and 64 (pn_meanshift_w_*)
// 20: the kernel profile as an argument (pn_meanshift_*_iter_*_kind_f32: Gaussian / Epanechnikov)
// 21: linear sum assignment on the device (pn_lsa_auction_f64)
// 22: trimmed surfaces (pn_grid_occupancy_ragged_f32, pn_trimesh_area_f64, pn_trimesh_sample_f64)
// 23: point coverage of the fitted primitives (pn_point_primitive_min_f32)
//     (added symbols, no declaration changed: pn_trimesh_*, pn_point_normals_f32, pn_orient_normals_f32,
//      pn_knn3_grid_f32, pn_knn3_grid_workspace_bytes, pn_orient_normals_global_*, pn_fps_*)
extern "C" int pn_abi_version(void) { return PN_ABI_VERSION; }
