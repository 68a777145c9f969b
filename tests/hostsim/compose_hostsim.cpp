// Host build of trase_amd/csrc/compose_math.h behind a C shim (tests/test_compose_hostsim.py): the loop of compose.hip's
// kernel over the output rows of one part, row by row, with the same guard on the rows[] entries.
#include "../../trase_amd/csrc/compose_math.h"

using namespace trase;

extern "C" void hs_compose_part(int n, int m, int F, const float* xyz, const float* scaling, const float* rotation,
                                const float* opacity, const float* f_dc, const float* f_rest, const float* feat,
                                const int64_t* rows, const float* d_xyz, const float* d_rotation, const float* d_scaling,
                                int edit_mode, float s, const float* R, const float* q, const float* t, float* means,
                                float* scales, float* rots, float* opac, float* shs, float* objs) {
  ComposeEdit e;
  e.mode = edit_mode; e.s = s;
  for (int k = 0; k < 9; ++k) e.R[k] = R[k];
  for (int k = 0; k < 4; ++k) e.q[k] = q[k];
  for (int k = 0; k < 3; ++k) e.t[k] = t[k];
  for (int i = 0; i < m; ++i) {
    const int src = rows ? compose_source_row(rows[i], n) : i;
    ComposeSmall o;
    if (src >= 0) {
      compose_row(xyz + 3 * src, scaling + 3 * src, rotation + 4 * src, opacity[src], d_xyz ? d_xyz + 3 * src : nullptr,
                  d_scaling ? d_scaling + 3 * src : nullptr, d_rotation ? d_rotation + 4 * src : nullptr, e, o);
    } else {
      compose_zero(o);
    }
    for (int k = 0; k < 3; ++k) { means[3 * i + k] = o.mean[k]; scales[3 * i + k] = o.scale[k]; }
    for (int k = 0; k < 4; ++k) rots[4 * i + k] = o.rot[k];
    opac[i] = o.opacity;
    for (int k = 0; k < 48; ++k) shs[48 * i + k] = src >= 0 ? compose_sh_element(f_dc, f_rest, src, k) : 0.f;
    for (int k = 0; k < F; ++k) objs[F * i + k] = src >= 0 ? feat[(size_t)F * src + k] : 0.f;
  }
}
