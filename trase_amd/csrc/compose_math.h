// compose_math.h -- the per-row arithmetic of trase_compose_part (compose.hip): one Gaussian of one part of a composited
// scene, from raw parameters to rasterizer inputs, in fp32, statement by statement as the reference's render_composite and
// its rigid-edit helpers evaluate it (gaussian_renderer/__init__.py:158-331):
//     means = xyz + d_xyz          scales = exp(_scaling) + d_scaling       rot = normalize(_rotation) + d_rotation
//     opacity = sigmoid(_opacity)
//     rescale:    means *= s, scales *= s                                   (about the world origin)
//     rotate:     means = R means, rot = normalize(q_edit (x) rot)          (skipped when all three angles are exactly zero:
//                                                                            rot then stays the un-renormalised sum above)
//     translate:  means += offset
// Pure scalar functions for HIP device code (the product) and, compiled with g++, for tests/test_compose_hostsim.py.
//
// exp and the sigmoid's exp are the LIBRARY expf (<= 1 ulp), not the __expf of preprocess_raw.hip's activate(): __expf scales
// its argument by log2(e) in fp32 first, which costs |x| * 2^-24 relative -- 4 to 5 roundings at the log-scales of a trained
// scene -- and the composed tensors are checked against float64 with 2 roundings per transcendental.  The kernel is bound by
// memory, so the slower exp costs nothing.  normalize is activate()'s: x * (1 / max(|x|, 1e-12)).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TRASE_CMP_HD __host__ __device__ __forceinline__
#else
#define TRASE_CMP_HD inline
#endif

namespace trase {

constexpr int COMPOSE_EDIT_NONE = 0;      // no edit record: the three activations and the deformation only
constexpr int COMPOSE_EDIT_NO_ROTATION = 1;   // rescale and translate (all angles exactly zero: the reference returns early)
constexpr int COMPOSE_EDIT_FULL = 2;      // rescale, rotate, translate

struct ComposeEdit {
  int mode;
  float s;            // scale_factor
  float R[9];         // row-major rotation matrix
  float q[4];         // q_edit, (r, x, y, z), r >= 0
  float t[3];         // offset
};

struct ComposeSmall {   // the 11 small values of one output row
  float mean[3], scale[3], rot[4], opacity;
};

// rows[] entry -> source row, or -1 if it lies outside [0, n): such a row is never dereferenced
TRASE_CMP_HD int compose_source_row(int64_t r, int n) { return (r >= 0 && r < (int64_t)n) ? (int)r : -1; }

TRASE_CMP_HD void compose_zero(ComposeSmall& o) {
  for (int k = 0; k < 3; ++k) { o.mean[k] = 0.f; o.scale[k] = 0.f; }
  for (int k = 0; k < 4; ++k) o.rot[k] = 0.f;
  o.opacity = 0.f;
}

// xyz / scaling / d_xyz / d_scaling: 3 floats, rotation / d_rotation: 4 floats, of ONE source row; the d_* may be null
TRASE_CMP_HD void compose_row(const float* xyz, const float* scaling, const float* rotation, float opacity_logit,
                              const float* d_xyz, const float* d_scaling, const float* d_rotation, const ComposeEdit& e,
                              ComposeSmall& o) {
  float m[3], sc[3], q[4];
  for (int k = 0; k < 3; ++k) {
    m[k] = xyz[k] + (d_xyz ? d_xyz[k] : 0.f);
    sc[k] = expf(scaling[k]) + (d_scaling ? d_scaling[k] : 0.f);
  }
  const float n = sqrtf(rotation[0] * rotation[0] + rotation[1] * rotation[1] + rotation[2] * rotation[2] + rotation[3] * rotation[3]);
  const float inv_n = 1.0f / fmaxf(n, 1e-12f);               // torch.nn.functional.normalize eps
  for (int k = 0; k < 4; ++k) q[k] = rotation[k] * inv_n + (d_rotation ? d_rotation[k] : 0.f);
  o.opacity = 1.0f / (1.0f + expf(-opacity_logit));
  if (e.mode != COMPOSE_EDIT_NONE) {
    for (int k = 0; k < 3; ++k) { m[k] *= e.s; sc[k] *= e.s; }
    if (e.mode == COMPOSE_EDIT_FULL) {
      const float x = m[0], y = m[1], z = m[2];
      m[0] = e.R[0] * x + e.R[1] * y + e.R[2] * z;
      m[1] = e.R[3] * x + e.R[4] * y + e.R[5] * z;
      m[2] = e.R[6] * x + e.R[7] * y + e.R[8] * z;
      // the reference's quat_multiply(rotations, q_edit): the Hamilton product q_edit (x) rot, components (r, x, y, z)
      const float w0 = q[0], x0 = q[1], y0 = q[2], z0 = q[3];
      const float w1 = e.q[0], x1 = e.q[1], y1 = e.q[2], z1 = e.q[3];
      const float pw = -x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0;
      const float px = x1 * w0 + y1 * z0 - z1 * y0 + w1 * x0;
      const float py = -x1 * z0 + y1 * w0 + z1 * x0 + w1 * y0;
      const float pz = x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0;
      const float pn = sqrtf(pw * pw + px * px + py * py + pz * pz);     // a true division, as the reference's `/ norm`
      q[0] = pw / pn; q[1] = px / pn; q[2] = py / pn; q[3] = pz / pn;
    }
    for (int k = 0; k < 3; ++k) m[k] += e.t[k];
  }
  for (int k = 0; k < 3; ++k) { o.mean[k] = m[k]; o.scale[k] = sc[k]; }
  for (int k = 0; k < 4; ++k) o.rot[k] = q[k];
}

// element e (0..47) of the (16,3) SH row of source row `src`: cat(features_dc (.,1,3), features_rest (.,15,3))
TRASE_CMP_HD float compose_sh_element(const float* f_dc, const float* f_rest, int src, int e) {
  return e < 3 ? f_dc[3 * (size_t)src + e] : f_rest[45 * (size_t)src + (e - 3)];
}

}  // namespace trase
