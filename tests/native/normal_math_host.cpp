// Test-only host harness around parsenet_codebase_amd/csrc/normal_math.h (the arithmetic normals.hip runs per point),
// so that tests/test_point_normals_abi.py can hold it against numpy.linalg.eigh in float64 without a GPU, and
// tests/test_point_normals_gpu.py can hold the kernel against it.  Not part of the product library.
//
// As a shared object it exports the nmh_* functions below.  As a program (it has a main) it reads neighbourhoods as
// text from the file named by its first argument, or from stdin:
//     n k                 the number of points of the segment and the number of neighbours
//     n lines  x y z      the points
//     then any number of lines of k indices into them, one neighbourhood per line
// and prints one line  nx ny nz variation gap  (%.9g) per neighbourhood.
#include <stdio.h>
#include <stdlib.h>

#include "../../parsenet_codebase_amd/csrc/normal_math.h"

// Every point q of every segment s of a ragged batch: P (total,3), off (S+1), idx (total,k) local indices,
// view (S,3) or null; normals (total,3), variation (total), gap (total).
extern "C" void nmh_normals(const float* P, const int* off, int S, const int32_t* idx, int k, int sweeps,
                            const float* view, float* normals, float* variation, float* gap) {
  for (int s = 0; s < S; ++s) {
    const int o0 = off[s], n = off[s + 1] - o0;
    for (int q = 0; q < n; ++q) {
      const size_t p = (size_t)o0 + q;
      nm_point(P + 3 * (size_t)o0, n, idx + p * k, k, sweeps, normals + 3 * p, variation + p, gap + p);
      if (view) nm_orient(normals + 3 * p, P + 3 * p, view + 3 * s);
    }
  }
}

extern "C" void nmh_canonical(float* n) { nm_canonical(n); }
extern "C" void nmh_orient(float* n, const float* p, const float* v) { nm_orient(n, p, v); }
extern "C" int nmh_sweeps(void) { return NM_SWEEPS; }

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) {
    fprintf(stderr, "normal_math_host: cannot open %s\n", argv[1]);
    return 2;
  }
  int n = 0, k = 0;
  if (fscanf(f, "%d %d", &n, &k) != 2 || n < 0 || n > (1 << 24) || k < NM_MIN_K || k > NM_MAX_K) {
    fprintf(stderr, "normal_math_host: expected `n k` with %d <= k <= %d\n", NM_MIN_K, NM_MAX_K);
    return 2;
  }
  float* P = (float*)malloc(sizeof(float) * 3 * (size_t)(n > 0 ? n : 1));
  int32_t* idx = (int32_t*)malloc(sizeof(int32_t) * (size_t)k);
  int rc = 0;
  for (int i = 0; i < 3 * n; ++i)
    if (fscanf(f, "%f", &P[i]) != 1) {
      fprintf(stderr, "normal_math_host: %d points announced, coordinate %d is missing\n", n, i);
      rc = 2;
      break;
    }
  while (rc == 0) {
    int got = 0;
    while (got < k && fscanf(f, "%d", &idx[got]) == 1) ++got;
    if (got == 0) break;
    if (got < k) {
      fprintf(stderr, "normal_math_host: a neighbourhood of %d indices, expected %d\n", got, k);
      rc = 2;
      break;
    }
    float nrm[3], variation, gap;
    nm_point(P, n, idx, k, NM_SWEEPS, nrm, &variation, &gap);
    printf("%.9g %.9g %.9g %.9g %.9g\n", nrm[0], nrm[1], nrm[2], variation, gap);
  }
  free(idx);
  free(P);
  if (f != stdin) fclose(f);
  return rc;
}
