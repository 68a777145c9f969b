// frame_quads.h -- what the one-pass frame kernels (evaluate.hip, layers.hip) share: the accesses of a thread that owns 4
// consecutive pixels of a row, and the two 8-bit quantisers.  One copy of each, so that every 8-bit frame of the library is
// quantised by the same function.
#pragma once
#include "common.h"

namespace trase {

// ---- 4-pixel accesses: one wide access, or up to n scalar ones --------------------------------------------------------------
__device__ __forceinline__ void ld4f(const float* p, bool vec, int n, float (&v)[4]) {
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = u < n ? p[u] : 0.f;
  }
}
__device__ __forceinline__ void st4f(float* p, bool vec, int n, const float (&v)[4]) {
  if (vec) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < n) p[u] = v[u];
  }
}
// k bytes (k <= 4) as the low bytes of a dword, little-endian
__device__ __forceinline__ uint32_t ld4b(const uint8_t* p, bool vec, int k) {
  if (vec) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t w = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (u < k) w |= (uint32_t)p[u] << (8 * u);
  return w;
}
__device__ __forceinline__ void st4b(uint8_t* p, bool vec, int k, uint32_t w) {
  if (vec) {
    *reinterpret_cast<uint32_t*>(p) = w;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < k) p[u] = (uint8_t)(w >> (8 * u));
  }
}
// the 3 n bytes of n HWC pixels as three dwords: byte 3 u + c = channel c of pixel u
__device__ __forceinline__ void ld12b(const uint8_t* p, bool vec, int n, uint32_t (&w)[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) w[j] = ld4b(p + 4 * j, vec, 3 * n - 4 * j);
}
__device__ __forceinline__ void st12b(uint8_t* p, bool vec, int n, const uint32_t (&w)[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) st4b(p + 4 * j, vec, 3 * n - 4 * j, w[j]);
}
__device__ __forceinline__ uint32_t hwc_byte(const uint32_t (&w)[3], int u, int c) {
  const int k = 3 * u + c;
  return (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
}

// to8b (render.py:106): truncation of 255 * clip(x, 0, 1), the product rounded to fp32; a NaN gives 0
__device__ __forceinline__ uint32_t to8b(float x) {
  const float c = x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;
  return (uint32_t)__fmul_rn(255.f, c);
}
// torchvision's save_image: x.mul(255).add_(0.5).clamp_(0, 255) truncated, every step rounded to fp32; a NaN gives 0
__device__ __forceinline__ uint32_t save8b(float x) {
  const float v = __fadd_rn(__fmul_rn(x, 255.f), 0.5f);
  return v > 0.f ? (v < 255.f ? (uint32_t)v : 255u) : 0u;
}

}  // namespace trase
