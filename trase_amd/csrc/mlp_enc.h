// mlp_enc.h -- what the deformation-MLP kernels of mlp.hip (bf16 operands) and mlp_split.hip (split-bf16 operands) share:
// the network's constants, the MFMA fragment types, the positional encoding and the LDS activation-tile addressing.
#pragma once
#include "common.h"

namespace trase {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MW = 256;          // hidden width
constexpr int MD = 8;            // hidden layers
constexpr int EMB_T = 84;        // default network: PE(x) 63 + PE(t) 21 (t_multires = 10)
constexpr int EMB_B = 93;        // is_blender (D-NeRF): PE(x) 63 + timenet output 30 (utils/time_utils.py:74-86)
constexpr int EMBP = 96;         // padded to a multiple of 16
constexpr int SKIP = 5;          // layer whose input is cat(PE, h)
constexpr int MROWS = 32;        // rows per wave
constexpr int MWAVES = 4;
constexpr int HEADP = 32;        // 10 head outputs padded to one 32-wide MFMA block

// ---- positional encoding, generated straight into an MFMA A fragment ---------------------------------
// column order of cat(PE(x), PE(t)) as built by Embedder.embed (utils/time_utils.py:26-57):
//   x(3), then per frequency 2^f: sin(x 2^f)(3), cos(x 2^f)(3);  t, then per frequency: sin(t 2^f), cos(t 2^f)
//   is_blender: the time block is the timenet output instead (30 columns, the same for every row)
// LDS activation tile of one wave: 32 rows x 256 bf16, 16-byte chunks XOR-swizzled by the row
__device__ __forceinline__ int act_off(int m, int k) {   // element offset of (row m, column k)
  const int chunk = (k >> 3) ^ (m & 15);
  return m * MW + (chunk << 3) + (k & 7);
}

// sin / cos of v 2^f with the argument reduced to (-1/2, 1/2] revolutions first.  __sinf(a) is v_sin_f32(a / 2pi): the
// rounding of that product costs 2^-24 |a| / 2pi revolutions, ~5e-5 at |a| = 2^9 and ~1e-3 rad at scene-sized |v| = 40 --
// up to a quarter of a bf16 ulp of the encoding.  Here v / 2pi is carried as hi + lo (the product's rounding error exactly,
// by fma), scaled by 2^f exactly, and the whole revolutions are removed exactly: ~3e-8 revolutions for any |v 2^f| < 2^24.
// sin and cos of one (v, f) share the reduction (the compiler merges the identical expressions of the two columns).
__device__ __forceinline__ float pe_rev(float v, int f) {
  constexpr float INV2PI_HI = 0x1.45f306p-3f, INV2PI_LO = 0x1.b93910p-28f;   // 1 / 2pi = HI + LO + O(2^-53)
  const float hi = v * INV2PI_HI;
  const float lo = fmaf(v, INV2PI_HI, -hi) + v * INV2PI_LO;
  const float s = (float)(1 << f), u = hi * s;
  return (u - rintf(u)) + lo * s;
}

__device__ __forceinline__ float pe_const(int c, float x0, float x1, float x2, float t, const float* __restrict__ temb) {   // c is a compile-time constant
  if (c < 3) return c == 0 ? x0 : (c == 1 ? x1 : x2);
  if (c < 63) {
    const int q = c - 3, f = q / 6, r = q % 6, d = r % 3;
    const float u = pe_rev(d == 0 ? x0 : (d == 1 ? x1 : x2), f);
    return r < 3 ? __builtin_amdgcn_sinf(u) : __builtin_amdgcn_cosf(u);
  }
  if (temb) return c < EMB_B ? temb[c - 63] : 0.f;       // wave-uniform pointer and address: scalar loads
  if (c == 63) return t;
  if (c < EMB_T) {
    const int q = c - 64, f = q >> 1;
    const float u = pe_rev(t, f);
    return (q & 1) ? __builtin_amdgcn_cosf(u) : __builtin_amdgcn_sinf(u);
  }
  return 0.f;
}

// workgroup barrier that orders LDS traffic only: __syncthreads() is a release/acquire fence and drains vmcnt too, which
// would force the slab loads that are deliberately in flight across the barrier to complete at every K-step
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_s_waitcnt(0xC07F);        // lgkmcnt(0); vmcnt and expcnt left at their maxima
  __builtin_amdgcn_s_barrier();
}

}  // namespace trase
