// Test-only host harness around the value-only residual of parsenet_codebase_amd/csrc/fit_math.h (the arithmetic the
// analytic branch of cover.hip runs per point), next to the value of the dual-number function it restates, so that
// tests/test_pcover_abi.py can hold both against the reference's fixture without a GPU.  Not part of the product
// library.
#include "../../parsenet_codebase_amd/csrc/fit_math.h"

extern "C" void cvh_residuals(const float* P, int n, int type, const float* th, int sqrt_flag, float* value,
                              float* dual_value) {
  for (int i = 0; i < n; ++i) {
    value[i] = residual_point_value(type, P[3 * i], P[3 * i + 1], P[3 * i + 2], th, sqrt_flag);
    dual_value[i] = residual_point(type, P[3 * i], P[3 * i + 1], P[3 * i + 2], th, sqrt_flag).v;
  }
}
