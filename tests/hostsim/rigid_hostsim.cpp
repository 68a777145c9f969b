// Host build of trase_amd/csrc/rigid_math.h behind a C shim (tests/test_rigid_reference.py): the loops of the polar3 kernels of
// neighbors.hip over n matrices, row by row.
#include <stddef.h>

#include "../../trase_amd/csrc/rigid_math.h"

using namespace trase;

// R (n, 3, 3), s23 (n) = sigma_2 + sigma_3 as the arithmetic finds it, degenerate (n) by the rule of a matrix on its own
extern "C" void hs_polar3(const float* S, int n, float* R, double* s23, int* degenerate) {
  for (int i = 0; i < n; ++i) {
    s23[i] = polar3(S + 9 * (size_t)i, R + 9 * (size_t)i);
    degenerate[i] = polar3_is_degenerate(s23[i], 1.0, polar3_frobenius(S + 9 * (size_t)i)) ? 1 : 0;
  }
}

extern "C" void hs_polar3_bwd(const float* S, const float* R, const float* G, int n, float* gS) {
  for (int i = 0; i < n; ++i) polar3_row_bwd(S + 9 * (size_t)i, R + 9 * (size_t)i, G + 9 * (size_t)i, gS + 9 * (size_t)i);
}

// the rule with the edge count and edge scale of a graph row
extern "C" int hs_polar3_is_degenerate(double s23, double k, double m) { return polar3_is_degenerate(s23, k, m) ? 1 : 0; }
