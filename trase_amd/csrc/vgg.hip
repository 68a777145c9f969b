// vgg.hip -- VGG16's 3x3 convolutions on the matrix cores, described ONCE and used by two families of entry points:
//   * the style-transfer feature extractor, forward and gradient to the image (trase_vgg_ws_bytes / _pack / _forward / _backward;
//     trase_amd/vgg.py), which cuts the network behind one of its first VG_CUT_MAX = 8 convolutions;
//   * the LPIPS metric, forward only (trase_lpips_ws_bytes / _pack / _forward / _head; trase_amd/lpips.py), which runs all thirteen
//     for two images and adds a distance head behind five of them (described where its kernels begin, further down).
//
// Network (the one table: vg_chan, vg_shift, vg_pooled, vg_pixels over layers 0 .. VG_LAYERS = 13):
//   conv1_1 conv1_2 | conv2_1 conv2_2 | conv3_1 conv3_2 conv3_3 | conv4_1 conv4_2 conv4_3 | conv5_1 conv5_2 conv5_3
// (| = MaxPool2d(2, 2), floor), 3x3, stride 1, zero padding 1, bias, ReLU; channels 3 -> 64 -> 64 -> 128 -> 128 -> 256 -> 256 -> 256
// -> 512 -> .. -> 512.  What the families add to the table: the extractor its cut (`layers` = k in 1..8 returns the k-th
// convolution's output BEFORE the ReLU as fp32 (C, h*w)), the backward weight streams and w1t in its pack, and the saved decisions;
// LPIPS its five taps (LP_TAP_LAYER) and their `lin` vectors.  One pack description (VgPackSpec: how many layers, backward streams
// or not, lin vectors or not), one pack launch list, one builder of a forward convolution's VgConv and one set of argument checks
// serve both; the two layer loops stay apart, because they move different buffers.
//
// Arithmetic (mlp_split.hip's): every matrix operand v -- activations, weights, cotangents -- is hi = bf16(v), lo = bf16(v - hi);
// a product is lo.hi + hi.lo + hi.hi, three v_mfma_f32_32x32x16_bf16 into one fp32 accumulator that starts at the bias.  The
// 3-channel ends (conv1_1 and its gradient to the image) are fp32 VALU kernels with the normalisation fused in.
//
// Organisation: implicit GEMM, no im2col.  Between layers an activation is two channel-last planes [pixel][C] (hi, lo), so a
// lane's operand fragment -- 8 consecutive channels of one pixel at one tap -- is one 16-byte load.  K = 9 Cin is tap-major: a
// K-step of 16 stays inside one tap (Cin is a multiple of 64), an out-of-image tap is a zero fragment.
//   * a WORKGROUP (4 waves) owns a VG_TILE x VG_TILE = 16 x 16 pixel tile and 64 output channels (blockIdx.y); wave w owns the
//     tile's rows 4 w .. 4 w + 3 as two MFMA column groups of 32 pixels (2 rows x 16) and both 32-channel blocks: 64 accumulators;
//   * weights are a stream of K-step slabs [ks][hi|lo][k/8][n][k%8] written once per weight set by the pack kernel, forward and
//     backward: the backward stream holds the spatially flipped weights with Cin and Cout exchanged, so the gradient to a
//     layer's input is this same kernel run on the cotangent;
//   * per K-step a wave loads 4 activation and 4 weight fragments (global, one K-step ahead of their use) for 12 MFMAs;
//   * the accumulator layout (lane (m, h), register 4 q + j <-> channel 8 q + 4 h + j of pixel m) puts the four pixels of a 2x2
//     pool window into lanes m, m^1, m^16, m^17: the pool is fused into the epilogue (ATen's rule: scan in (row, column) order,
//     update on strict >).
// Saved for the backward: 1 bit per convolution output (z > 0) as uint16 [pixel][C/16], or, where a pool follows, 4 bits per
// POOLED unit (window position, maximum > 0) as uint64 [pooled pixel][C/16]; bit / nibble vg_bit(c) of word vg_group(c).
// No atomics: two calls give the same bits.
#include "common.h"
#include "mlp_enc.h"

namespace trase {

constexpr int VG_LAYERS = 13;                                     // convolutions of the table
constexpr int VG_CUT_MAX = 8;                                     // the extractor cuts behind conv1_1 .. conv4_1
constexpr int VG_TILE = 16;                                       // pixels per side of a workgroup's tile
constexpr int VG_NB = 64;                                         // output channels per workgroup
__host__ __device__ constexpr int vg_chan(int l) { return l == 0 ? 3 : l <= 2 ? 64 : l <= 4 ? 128 : l <= 7 ? 256 : 512; }   // channels behind layer l
__host__ __device__ constexpr int vg_shift(int l) { return l <= 2 ? 0 : l <= 4 ? 1 : l <= 7 ? 2 : l <= 10 ? 3 : 4; }      // pools in front of layer l
__host__ __device__ constexpr bool vg_pooled(int l) { return l == 2 || l == 4 || l == 7 || l == 10; }                     // a pool follows layer l
__host__ __device__ __forceinline__ int vg_group(int c) { return (c >> 5) * 2 + ((c >> 2) & 1); }
__host__ __device__ __forceinline__ int vg_bit(int c) { return ((c >> 3) & 3) * 4 + (c & 3); }

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void vg_split(float v, __bf16& hi, __bf16& lo) {
  hi = (__bf16)v;
  lo = (__bf16)(v - (float)hi);
}

// ---- pack ------------------------------------------------------------------------------------------------------------------
// one thread per weight element of one stream of one layer: [ks][hi|lo][k/8][n][k%8], ks = tap * (K / 16) + channel step
__global__ __launch_bounds__(256) void vgg_pack_kernel(const float* __restrict__ w, int Cin, int Cout, int backward,
                                                       __bf16* __restrict__ stream) {
  const int K = backward ? Cout : Cin, N = backward ? Cin : Cout;       // the stream's contraction and output widths
  const int plane = 2 * N * 8;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)9 * (K / 16) * plane;
  if (idx >= total) return;
  const int ks = (int)(idx / plane), r = (int)(idx % plane), h = r / (N * 8), n = (r >> 3) % N, e = r & 7;
  const int tap = ks / (K / 16), c = (ks % (K / 16)) * 16 + 8 * h + e, ky = tap / 3, kx = tap % 3;
  const float v = backward ? w[(((size_t)c * Cin + n) * 3 + (2 - ky)) * 3 + (2 - kx)]
                           : w[(((size_t)n * Cin + c) * 3 + ky) * 3 + kx];
  __bf16 hi, lo;
  vg_split(v, hi, lo);
  __bf16* o = stream + (size_t)ks * 2 * plane + r;
  o[0] = hi; o[plane] = lo;
}

__global__ __launch_bounds__(256) void vgg_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// ---- conv1_1: fp32, normalisation fused into the load -------------------------------------------------------------------
struct VgNorm { float mean[3]; float inv_std[3]; };

template <bool FINAL>
__global__ __launch_bounds__(256) void vgg_conv1_kernel(const float* __restrict__ img, int H, int W, VgNorm nm,
                                                        const float* __restrict__ w1, const float* __restrict__ b1,
                                                        __bf16* __restrict__ out_hi, __bf16* __restrict__ out_lo,
                                                        float* __restrict__ out_f32, uint16_t* __restrict__ relu_bits) {
  __shared__ float s_w[64 * 27 + 64];
  for (int i = threadIdx.x; i < 64 * 27; i += 256) s_w[i] = w1[i];
  if (threadIdx.x < 64) s_w[64 * 27 + threadIdx.x] = b1[threadIdx.x];
  __syncthreads();
  const int HW = H * W;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int y = pix / W, x = pix - y * W;
  float v[27];
#pragma unroll
  for (int ci = 0; ci < 3; ++ci)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y + ky - 1, xx = x + kx - 1;
        float t = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) t = (img[(size_t)ci * HW + (size_t)yy * W + xx] - nm.mean[ci]) * nm.inv_std[ci];
        v[ci * 9 + ky * 3 + kx] = t;
      }
  uint32_t bits[4] = {0u, 0u, 0u, 0u};
  for (int c4 = 0; c4 < 64; c4 += 4) {
    bf16x4 vh, vl;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c4 + j;
      float z = s_w[64 * 27 + c];
#pragma unroll
      for (int i = 0; i < 27; ++i) z = fmaf(v[i], s_w[c * 27 + i], z);
      if (FINAL) {
        out_f32[(size_t)c * HW + pix] = z;
      } else {
        if (z > 0.f) bits[vg_group(c)] |= 1u << vg_bit(c);
        __bf16 a, b;
        vg_split(fmaxf(z, 0.f), a, b);
        vh[j] = a; vl[j] = b;
      }
    }
    if (!FINAL) {
      *reinterpret_cast<bf16x4*>(out_hi + (size_t)pix * 64 + c4) = vh;
      *reinterpret_cast<bf16x4*>(out_lo + (size_t)pix * 64 + c4) = vl;
    }
  }
  if (!FINAL && relu_bits) {
#pragma unroll
    for (int g = 0; g < 4; ++g) relu_bits[(size_t)pix * 4 + g] = (uint16_t)bits[g];
  }
}

// gradient to the image: the transposed conv1_1 on the (masked) cotangent of its output, times 1 / std.  A workgroup owns
// 16 x 16 pixels; EIGHT lanes share a pixel, lane c of them owning channels 8 c .. 8 c + 7, so a load instruction reads eight
// pixels' whole 128-byte rows (one pixel per lane reads 16 bytes of 64 different lines per instruction and thrashes L1: 4.9 ms
// at 1080p).  The eight partial sums meet in a fixed butterfly.  Weights: w1t[tap][co] = (w[co][0..2][tap], 0), from LDS.
__global__ __launch_bounds__(256) void vgg_image_grad_kernel(const __bf16* __restrict__ g_hi, const __bf16* __restrict__ g_lo, int H,
                                                             int W, VgNorm nm, const float4* __restrict__ w1t, float* __restrict__ d_img) {
  __shared__ float4 s_w[9 * 64];
  for (int i = threadIdx.x; i < 9 * 64; i += 256) s_w[i] = w1t[i];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, cg = lane & 7, sub = lane >> 3;
  const size_t HW = (size_t)H * W;
  for (int i = 0; i < 8; ++i) {                     // the wave's 4 rows x 16 columns, eight pixels at a time
    const int y = blockIdx.y * 16 + wave * 4 + (i >> 1), x = blockIdx.x * 16 + (i & 1) * 8 + sub;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      const int yy = y - ky + 1, xx = x - kx + 1;
      const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;           // outside: the nearest pixel is read and not used
      const size_t o = ((size_t)min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1)) * 64 + 8 * cg;
      const bf16x8 vh = *reinterpret_cast<const bf16x8*>(g_hi + o), vl = *reinterpret_cast<const bf16x8*>(g_lo + o);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float gv = ok ? (float)vh[e] + (float)vl[e] : 0.f;
        const float4 wv = s_w[tap * 64 + 8 * cg + e];
        d0 = fmaf(gv, wv.x, d0); d1 = fmaf(gv, wv.y, d1); d2 = fmaf(gv, wv.z, d2);
      }
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) { d0 += __shfl_xor(d0, off); d1 += __shfl_xor(d1, off); d2 += __shfl_xor(d2, off); }
    if (x < W && y < H && cg < 3) {
      const float d = cg == 0 ? d0 * nm.inv_std[0] : cg == 1 ? d1 * nm.inv_std[1] : d2 * nm.inv_std[2];
      d_img[cg * HW + (size_t)y * W + x] = d;
    }
  }
}

__global__ __launch_bounds__(64) void vgg_w1t_kernel(const float* __restrict__ w1, float4* __restrict__ w1t) {
  const int tap = blockIdx.x, co = threadIdx.x;
  w1t[tap * 64 + co] = make_float4(w1[co * 27 + tap], w1[co * 27 + 9 + tap], w1[co * 27 + 18 + tap], 0.f);
}

// the cotangent of the returned layer, fp32 planar (C, HW) -> split channel-last planes
__global__ __launch_bounds__(256) void vgg_cot_split_kernel(const float* __restrict__ g, int C, int HW, __bf16* __restrict__ o_hi,
                                                            __bf16* __restrict__ o_lo) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int c8 = blockIdx.y * 8;
  if (pix >= HW) return;
  bf16x8 vh, vl;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    __bf16 a, b;
    vg_split(g[(size_t)(c8 + e) * HW + pix], a, b);
    vh[e] = a; vl[e] = b;
  }
  *reinterpret_cast<bf16x8*>(o_hi + (size_t)pix * C + c8) = vh;
  *reinterpret_cast<bf16x8*>(o_lo + (size_t)pix * C + c8) = vl;
}

// ---- the MFMA convolution ---------------------------------------------------------------------------------------------------
enum { VG_FWD_RELU = 0, VG_FWD_POOL = 1, VG_FWD_OUT = 2, VG_BWD_MASK = 3, VG_BWD_UNPOOL = 4 };

struct VgConv {
  const __bf16* in_hi; const __bf16* in_lo;      // [H * W][Cin]
  const __bf16* stream;                          // [9 Cin / 16][hi|lo][2][Cout][8]
  const float* bias;                             // (Cout) or null (backward)
  int H, W, Cin, Cout, lg_steps;                 // lg_steps = log2(Cin / 16)
  __bf16* out_hi; __bf16* out_lo;                // channel-last [pixels][Cout]: (H, W); POOL: (H/2, W/2); UNPOOL: (out_H, out_W)
  float* out_f32;                                // FWD_OUT: (Cout, H * W)
  uint16_t* relu_bits;                           // FWD_RELU writes (null: nothing is kept), BWD_MASK reads: [H * W][Cout / 16]
  uint64_t* pool_codes;                          // FWD_POOL writes (or null), BWD_UNPOOL reads: [pooled pixels][Cout / 16]
  int out_H, out_W;                              // BWD_UNPOOL: the full-resolution plane the windows scatter into
};

template <int EPI>
__global__ __launch_bounds__(256) void vgg_conv_kernel(VgConv a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = lane & 31, h = lane >> 5;
  const int ntx = (a.W + VG_TILE - 1) / VG_TILE;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int cb = blockIdx.y;
  const int H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout;
  int py[2], px[2];
#pragma unroll
  for (int rg = 0; rg < 2; ++rg) {
    py[rg] = ty * VG_TILE + wave * 4 + rg * 2 + (m >> 4);
    px[rg] = tx * VG_TILE + (m & 15);
  }
  const int steps = 1 << a.lg_steps, KS = 9 * steps;
  const int plane = 2 * Cout * 8;
  const __bf16* const gw = a.stream + h * (Cout * 8) + (size_t)(cb * VG_NB + m) * 8;

  // fragments of K-step ks: activations f[rg * 2 + hl], weights f[4 + nb * 2 + hl]; a pixel outside the image reads the
  // nearest inside one (never stored), a tap outside the image is zeros
  auto fetch = [&](int ks, bf16x8 (&f)[8]) {
    ks = min(ks, KS - 1);
    const int tap = ks >> a.lg_steps, c0 = (ks & (steps - 1)) * 16;
    const int ky = (tap * 11) >> 5, dy = ky - 1, dx = tap - 3 * ky - 1;
#pragma unroll
    for (int rg = 0; rg < 2; ++rg) {
      const int yy = py[rg] + dy, xx = px[rg] + dx;
      const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
      const int cy = min(max(yy, 0), H - 1), cx = min(max(xx, 0), W - 1);
      const size_t o = ((size_t)cy * W + cx) * Cin + c0 + 8 * h;
      bf16x8 vh = *reinterpret_cast<const bf16x8*>(a.in_hi + o), vl = *reinterpret_cast<const bf16x8*>(a.in_lo + o);
      if (!ok) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { vh[e] = (__bf16)0.f; vl[e] = (__bf16)0.f; }
      }
      f[rg * 2] = vh; f[rg * 2 + 1] = vl;
    }
    const __bf16* p = gw + (size_t)ks * 2 * plane;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int hl = 0; hl < 2; ++hl) f[4 + nb * 2 + hl] = *reinterpret_cast<const bf16x8*>(p + hl * plane + nb * 256);
  };

  f32x16 acc[2][2];                                // [pixel group][channel block]
  // lane (m, h), register 4 q + j <-> channel 32 nb + 8 q + 4 h + j of pixel m
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float b = a.bias ? a.bias[cb * VG_NB + nb * 32 + 8 * q + 4 * h + j] : 0.f;
        acc[0][nb][4 * q + j] = b; acc[1][nb][4 * q + j] = b;
      }
  auto mma = [&](const bf16x8 (&f)[8]) {
#pragma unroll
    for (int term = 0; term < 3; ++term)           // lo.hi, hi.lo, hi.hi: consecutive MFMAs go to different accumulators
#pragma unroll
      for (int rg = 0; rg < 2; ++rg)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          acc[rg][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[4 + nb * 2 + (term == 0 ? 1 : 0)], f[rg * 2 + (term == 1 ? 1 : 0)],
                                                                acc[rg][nb], 0, 0, 0);
  };
  bf16x8 f0[8], f1[8];
  fetch(0, f0);
  for (int ks = 0; ks < KS; ks += 2) {             // KS is even: Cin / 16 is a multiple of 4
    fetch(ks + 1, f1);
    mma(f0);
    fetch(ks + 2, f0);
    mma(f1);
  }

  // ---- epilogue ------------------------------------------------------------------------------------------------------------
  const int G = Cout / 16;                          // words per pixel of the saved bits
#pragma unroll
  for (int rg = 0; rg < 2; ++rg) {
    const int y = py[rg], x = px[rg];
    const bool inside = y < H && x < W;
    const size_t pix = (size_t)y * W + x;
    if (EPI == VG_FWD_OUT) {
      if (inside) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int c = cb * VG_NB + nb * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
            a.out_f32[(size_t)c * ((size_t)H * W) + pix] = acc[rg][nb][r];
          }
      }
    } else if (EPI == VG_FWD_RELU || EPI == VG_BWD_MASK) {
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const int g = (cb * 2 + nb) * 2 + h;
        uint32_t bits = 0u;
        if (EPI == VG_BWD_MASK && inside) bits = a.relu_bits[pix * G + g];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bf16x4 vh, vl;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float v = acc[rg][nb][4 * q + j];
            if (EPI == VG_FWD_RELU) {
              if (v > 0.f) bits |= 1u << (4 * q + j);
              v = fmaxf(v, 0.f);
            } else {
              v = ((bits >> (4 * q + j)) & 1u) ? v : 0.f;
            }
            __bf16 hi, lo;
            vg_split(v, hi, lo);
            vh[j] = hi; vl[j] = lo;
          }
          if (inside) {
            const size_t o = pix * Cout + cb * VG_NB + nb * 32 + 8 * q + 4 * h;
            *reinterpret_cast<bf16x4*>(a.out_hi + o) = vh;
            *reinterpret_cast<bf16x4*>(a.out_lo + o) = vl;
          }
        }
        if (EPI == VG_FWD_RELU && inside && a.relu_bits) a.relu_bits[pix * G + g] = (uint16_t)bits;
      }
    } else if (EPI == VG_FWD_POOL) {
      // the window of lanes m, m ^ 1, m ^ 16, m ^ 17 (the tile's origin is even); its owner is the lane with both bits clear
      const int PH = H >> 1, PW = W >> 1, Y = y >> 1, X = x >> 1;
      const bool owner = (m & 17) == 0 && Y < PH && X < PW;
      const size_t ppix = (size_t)Y * PW + X;
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        uint64_t codes = 0ull;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bf16x4 vh, vl;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float v00 = fmaxf(acc[rg][nb][4 * q + j], 0.f);
            const float v01 = __shfl_xor(v00, 1), v10 = __shfl_xor(v00, 16), v11 = __shfl_xor(v00, 17);
            float best = v00; uint32_t idx = 0u;
            if (v01 > best) { best = v01; idx = 1u; }
            if (v10 > best) { best = v10; idx = 2u; }
            if (v11 > best) { best = v11; idx = 3u; }
            codes |= (uint64_t)(idx | (best > 0.f ? 4u : 0u)) << (4 * (4 * q + j));
            __bf16 hi, lo;
            vg_split(best, hi, lo);
            vh[j] = hi; vl[j] = lo;
          }
          if (owner) {
            const size_t o = ppix * Cout + cb * VG_NB + nb * 32 + 8 * q + 4 * h;
            *reinterpret_cast<bf16x4*>(a.out_hi + o) = vh;
            *reinterpret_cast<bf16x4*>(a.out_lo + o) = vl;
          }
        }
        if (owner && a.pool_codes) a.pool_codes[ppix * G + (cb * 2 + nb) * 2 + h] = codes;
      }
    } else {                                        // VG_BWD_UNPOOL: pixel (y, x) is a pooled unit of the (out_H, out_W) plane
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        uint64_t codes = 0ull;
        if (inside) codes = a.pool_codes[pix * G + (cb * 2 + nb) * 2 + h];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            bf16x4 vh, vl;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const uint32_t code = (uint32_t)(codes >> (4 * (4 * q + j))) & 15u;
              const float v = code == (4u | (uint32_t)p) ? acc[rg][nb][4 * q + j] : 0.f;
              __bf16 hi, lo;
              vg_split(v, hi, lo);
              vh[j] = hi; vl[j] = lo;
            }
            if (inside) {
              const size_t opix = (size_t)(2 * y + (p >> 1)) * a.out_W + (2 * x + (p & 1));
              const size_t o = opix * Cout + cb * VG_NB + nb * 32 + 8 * q + 4 * h;
              *reinterpret_cast<bf16x4*>(a.out_hi + o) = vh;
              *reinterpret_cast<bf16x4*>(a.out_lo + o) = vl;
            }
          }
        }
      }
    }
  }
}

// ---- LPIPS (VGG): the stack to relu5_3 and the distance head, forward only ---------------------------------------------------
// (trase_lpips_ws_bytes / _pack / _forward / _head; trase_amd/lpips.py).  Thirteen convolutions
//   conv1_1 conv1_2 | conv2_1 conv2_2 | conv3_1 conv3_2 conv3_3 | conv4_1 conv4_2 conv4_3 | conv5_1 conv5_2 conv5_3
// run layer by layer for both images with the kernels above: vgg_conv1_kernel<false>, then vgg_conv_kernel<VG_FWD_RELU> for EVERY
// later layer -- also where a pool follows, because the tap (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3) is the full-resolution
// activation.  Behind a tapped layer:
//   * lpips_head_kernel reads both images' channel-last hi / lo planes, a value being t = (float)hi + (float)lo, and forms per
//     pixel  d = sum_c lin_c (a_c / (sqrt(sum a^2) + 1e-10) - b_c / (sqrt(sum b^2) + 1e-10))^2  in float64, in two passes over the
//     channels (norms, then differences: the expanded one-pass form cancels when x is close to y), rounded to fp32 ONCE into the
//     layer's map.  Eight lanes share a pixel, lane g of them owning channels 64 i + 8 g .. + 7 (16-byte loads, a pixel's 128-byte
//     row per instruction); the eight partial sums meet in a fixed xor butterfly, which gives every lane the same bits and treats
//     the two images alike: d(x, y) and d(y, x) are the same bits, d(x, x) is exactly 0.
//   * lpips_pool_kernel writes the 2x2 floor pool of the split planes for the next layer.  It SELECTS the (hi, lo) pair of the
//     window's maximum, compared lexicographically (hi, then lo) in ATen's scan order with update on strict >.  vg_split is monotone
//     in both parts, so the pair selected is the pair vg_split gives the maximum of the four fp32 values: the bits the VG_FWD_POOL
//     epilogue writes.  (Splitting max(hi + lo) again would not do: v = hi + 0.4999 ulp has lo rounded up to half an ulp, and
//     bf16(hi + lo) then rounds the tie to even, to hi + 1 ulp when hi is odd -- the same sum as another pair of bits.)  It is a
//     launch of its own and not part of the head: a lane of the head owns one pixel's channels, a window spans two rows.
//   * lpips_partial_kernel and lpips_mean_kernel sum each map in float64 in a fixed order (256 chunks per map, a workgroup each;
//     then one workgroup per layer joins the partial sums) and divide by the pixel count.  No atomics anywhere.
constexpr int LP_TAPS = 5;
constexpr int LP_TAP_LAYER[LP_TAPS] = {2, 4, 7, 10, 13};

__global__ __launch_bounds__(256) void lpips_head_kernel(const __bf16* __restrict__ x_hi, const __bf16* __restrict__ x_lo,
                                                         const __bf16* __restrict__ y_hi, const __bf16* __restrict__ y_lo, int C, int hw,
                                                         const float* __restrict__ lin, float* __restrict__ map) {
  // no contraction: a * ra - b * rb as ONE fused multiply-add would round the two images' terms differently, and (x, y) would no
  // longer be the bits of (y, x), nor (x, x) exactly 0; the fused multiply-adds wanted are written out
#pragma clang fp contract(off)
  const int pix = blockIdx.x * 32 + (threadIdx.x >> 3), cg = threadIdx.x & 7;
  const size_t row = (size_t)min(pix, hw - 1) * C;          // a pixel past the end reads the last one and stores nothing
  double na = 0.0, nb = 0.0;
  for (int c0 = 8 * cg; c0 < C; c0 += 64) {
    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(x_hi + row + c0), al = *reinterpret_cast<const bf16x8*>(x_lo + row + c0);
    const bf16x8 bh = *reinterpret_cast<const bf16x8*>(y_hi + row + c0), bl = *reinterpret_cast<const bf16x8*>(y_lo + row + c0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const double a = (double)((float)ah[e] + (float)al[e]), b = (double)((float)bh[e] + (float)bl[e]);
      na = fma(a, a, na); nb = fma(b, b, nb);
    }
  }
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) { na += __shfl_xor(na, off); nb += __shfl_xor(nb, off); }
  const double ra = 1.0 / (sqrt(na) + 1e-10), rb = 1.0 / (sqrt(nb) + 1e-10);      // the epsilon outside the root: a zero pixel gives 0
  double d = 0.0;
  for (int c0 = 8 * cg; c0 < C; c0 += 64) {
    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(x_hi + row + c0), al = *reinterpret_cast<const bf16x8*>(x_lo + row + c0);
    const bf16x8 bh = *reinterpret_cast<const bf16x8*>(y_hi + row + c0), bl = *reinterpret_cast<const bf16x8*>(y_lo + row + c0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const double a = (double)((float)ah[e] + (float)al[e]), b = (double)((float)bh[e] + (float)bl[e]);
      const double t = a * ra - b * rb;
      d = fma((double)lin[c0 + e], t * t, d);
    }
  }
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) d += __shfl_xor(d, off);
  if (cg == 0 && pix < hw) map[pix] = (float)d;
}

// one thread per pooled pixel and 8 channels: (H, W) -> (H / 2, W / 2), an odd last row or column lies in no window
__global__ __launch_bounds__(256) void lpips_pool_kernel(const __bf16* __restrict__ in_hi, const __bf16* __restrict__ in_lo, int H, int W,
                                                         int C, __bf16* __restrict__ out_hi, __bf16* __restrict__ out_lo) {
  const int PH = H >> 1, PW = W >> 1, G = C >> 3;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)PH * PW * G) return;
  const int g = (int)(idx % G);
  const size_t pp = idx / G;
  const int Y = (int)(pp / PW), X = (int)(pp - (size_t)Y * PW);
  bf16x8 bh, bl;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const size_t o = ((size_t)(2 * Y + (i >> 1)) * W + (2 * X + (i & 1))) * C + 8 * g;
    const bf16x8 vh = *reinterpret_cast<const bf16x8*>(in_hi + o), vl = *reinterpret_cast<const bf16x8*>(in_lo + o);
    if (i == 0) { bh = vh; bl = vl; continue; }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float h1 = (float)vh[e], h0 = (float)bh[e];
      if (h1 > h0 || (h1 == h0 && (float)vl[e] > (float)bl[e])) { bh[e] = vh[e]; bl[e] = vl[e]; }
    }
  }
  *reinterpret_cast<bf16x8*>(out_hi + pp * C + 8 * g) = bh;
  *reinterpret_cast<bf16x8*>(out_lo + pp * C + 8 * g) = bl;
}

// channel-last split planes -> fp32 planar (C, hw) of hi + lo, the values the head reads; one thread per pixel and 8 channels
__global__ __launch_bounds__(256) void lpips_tap_kernel(const __bf16* __restrict__ in_hi, const __bf16* __restrict__ in_lo, int C, int hw,
                                                        float* __restrict__ out) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int c8 = blockIdx.y * 8;
  if (pix >= hw) return;
  const bf16x8 vh = *reinterpret_cast<const bf16x8*>(in_hi + (size_t)pix * C + c8), vl = *reinterpret_cast<const bf16x8*>(in_lo + (size_t)pix * C + c8);
#pragma unroll
  for (int e = 0; e < 8; ++e) out[(size_t)(c8 + e) * hw + pix] = (float)vh[e] + (float)vl[e];
}

// the mean of a map in two fixed-order steps: workgroup (b, t) sums chunk b of layer t's map (LP_PARTS chunks of 256 ceil(n / 65536)
// elements; thread i: elements i, i + 256, .. of the chunk, then a tree over the 256 threads) into parts[t][b]; one workgroup per
// layer then joins the LP_PARTS partial sums in a tree and divides by n
constexpr int LP_PARTS = 256;
struct LpMeans { const float* map[LP_TAPS]; int n[LP_TAPS]; };
__device__ __forceinline__ double lp_block_sum(double v, double* s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  return s[0];
}
__global__ __launch_bounds__(256) void lpips_partial_kernel(LpMeans m, double* __restrict__ parts) {
  __shared__ double s[256];
  const float* __restrict__ map = m.map[blockIdx.y];
  const int n = m.n[blockIdx.y];
  const int chunk = 256 * ((n + 256 * LP_PARTS - 1) / (256 * LP_PARTS));
  const int lo = min((int)blockIdx.x * chunk, n), hi = min(lo + chunk, n);     // chunk * LP_PARTS < 2^25 + 2^16
  double acc = 0.0;
  for (int i = lo + threadIdx.x; i < hi; i += 256) acc += (double)map[i];
  const double sum = lp_block_sum(acc, s);
  if (threadIdx.x == 0) parts[blockIdx.y * LP_PARTS + blockIdx.x] = sum;
}
__global__ __launch_bounds__(256) void lpips_mean_kernel(LpMeans m, const double* __restrict__ parts, double* __restrict__ out) {
  __shared__ double s[256];
  const double sum = lp_block_sum(parts[blockIdx.x * LP_PARTS + threadIdx.x], s);
  if (threadIdx.x == 0) out[blockIdx.x] = sum / (double)m.n[blockIdx.x];
}

// ---- host side: the packs ----------------------------------------------------------------------------------------------------
// what a pack holds: the first `layers` layers' w1, biases and forward streams; with `backward` also w1t and the backward streams;
// with `lin` also the five lin vectors of the taps
struct VgPackSpec { int layers; bool backward; bool lin; };
static VgPackSpec vg_pack_spec(int k) { return VgPackSpec{k, true, false}; }           // the extractor cut behind layer k
constexpr VgPackSpec LP_PACK_SPEC{VG_LAYERS, false, true};
struct VgPack {
  float* w1; float4* w1t; float* bias[VG_LAYERS + 1]; __bf16* fwd[VG_LAYERS + 1]; __bf16* bwd[VG_LAYERS + 1]; float* lin[LP_TAPS];
};
static size_t vg_stream_elems(int l) { return (size_t)9 * vg_chan(l - 1) * vg_chan(l) * 2; }      // hi and lo
static size_t vg_pack_layout(void* p, VgPackSpec d, VgPack& f) {
  WsCursor c(p);
  f.w1 = c.take<float>(64 * 27);
  if (d.backward) f.w1t = c.take<float4>(9 * 64);
  for (int l = 1; l <= d.layers; ++l) {             // layer by layer: a pack of more layers begins with the pack of fewer
    f.bias[l] = c.take<float>(vg_chan(l));
    if (l > 1) f.fwd[l] = c.take<__bf16>(vg_stream_elems(l));
    if (l > 1 && d.backward) f.bwd[l] = c.take<__bf16>(vg_stream_elems(l));
  }
  if (d.lin)
    for (int t = 0; t < LP_TAPS; ++t) f.lin[t] = c.take<float>(vg_chan(LP_TAP_LAYER[t]));
  return c.bytes();
}

// (the launch helpers of this file run inside their callers' profiler scopes: each launch gets the check alone, on the primitive)
static int vg_launch_copy(const float* src, float* dst, int n, hipStream_t stream) {
  hipLaunchKernelGGL(vgg_copy_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, src, dst, n);
  TRASE_POST_LAUNCH("vgg_copy", stream, 0);
  return TRASE_OK;
}
// fills a pack from fp32 weights (Cout, Cin, 3, 3), biases and (where the pack has them) lin vectors, all on the device
static int vg_launch_pack(VgPackSpec d, const float* const* weights, const float* const* biases, const float* const* lin, const VgPack& p,
                          hipStream_t stream) {
  if (int rc = vg_launch_copy(weights[0], p.w1, 64 * 27, stream)) return rc;
  if (d.backward) {
    hipLaunchKernelGGL(vgg_w1t_kernel, dim3(9), dim3(64), 0, stream, weights[0], p.w1t);
    TRASE_POST_LAUNCH("vgg_w1t", stream, 0);
  }
  for (int l = 1; l <= d.layers; ++l)
    if (int rc = vg_launch_copy(biases[l - 1], p.bias[l], vg_chan(l), stream)) return rc;
  for (int l = 2; l <= d.layers; ++l) {
    const unsigned nb = (unsigned)((vg_stream_elems(l) / 2 + 255) / 256);
    hipLaunchKernelGGL(vgg_pack_kernel, dim3(nb), dim3(256), 0, stream, weights[l - 1], vg_chan(l - 1), vg_chan(l), 0, p.fwd[l]);
    if (d.backward) hipLaunchKernelGGL(vgg_pack_kernel, dim3(nb), dim3(256), 0, stream, weights[l - 1], vg_chan(l - 1), vg_chan(l), 1, p.bwd[l]);
    TRASE_POST_LAUNCH("vgg_pack_weights", stream, 0);
  }
  if (d.lin)
    for (int t = 0; t < LP_TAPS; ++t)
      if (int rc = vg_launch_copy(lin[t], p.lin[t], vg_chan(LP_TAP_LAYER[t]), stream)) return rc;
  return TRASE_OK;
}

// ---- host side: the workspaces -----------------------------------------------------------------------------------------------
static inline size_t vg_pixels(int l, int H, int W) { return (size_t)(H >> vg_shift(l)) * (size_t)(W >> vg_shift(l)); }

// the extractor's saved decisions of layers 1 .. k - 1
struct VgSaved { uint16_t* relu[VG_CUT_MAX + 1]; uint64_t* pool[VG_CUT_MAX + 1]; };
static size_t vg_saved_layout(void* p, int k, int H, int W, VgSaved& s) {
  WsCursor c(p);
  for (int l = 1; l < k; ++l) {
    s.relu[l] = nullptr; s.pool[l] = nullptr;
    if (vg_pooled(l)) s.pool[l] = c.take<uint64_t>(vg_pixels(l + 1, H, W) * (vg_chan(l) / 16));
    else s.relu[l] = c.take<uint16_t>(vg_pixels(l, H, W) * (vg_chan(l) / 16));
  }
  return c.bytes();
}

// the extractor's workspace: two ping-pong activation buffers (hi and lo planes each); layer l's output -- forward: the activation
// the next layer reads (pooled where a pool follows); backward: the cotangent of its convolution output -- lives in buffer l & 1
struct VgWs { __bf16* hi[2]; __bf16* lo[2]; };
static size_t vg_ws_layout(void* p, int k, int H, int W, bool backward, VgWs& w) {
  size_t units[2] = {0, 0};
  for (int l = 1; l <= k; ++l) {
    size_t n = 0;
    if (backward) n = vg_pixels(l, H, W) * vg_chan(l);
    else if (l < k) n = vg_pixels(vg_pooled(l) ? l + 1 : l, H, W) * vg_chan(l);
    if (n > units[l & 1]) units[l & 1] = n;
  }
  WsCursor c(p);
  for (int i = 0; i < 2; ++i) { w.hi[i] = c.take<__bf16>(units[i]); w.lo[i] = c.take<__bf16>(units[i]); }
  return c.bytes();
}

static size_t lp_map_floats(int H, int W) {
  size_t n = 0;
  for (int t = 0; t < LP_TAPS; ++t) n += vg_pixels(LP_TAP_LAYER[t], H, W);
  return n;
}

// the workspace of trase_lpips_forward: THREE buffers of H * W * 64 split values (hi and lo planes each), the five maps and the
// partial sums of their means.  The largest activation is a full-resolution 64-channel one and every activation behind the
// first pool is at most half of it, so: conv1_1 of image im -> buffer im; conv1_2 of x: 0 -> 2, of y: 1 -> 0 (x's conv1_1 output
// is spent by then); from the first pool on, image im ping-pongs between the im-th halves of buffers 1 and 2.
struct LpWs { __bf16* hi[3]; __bf16* lo[3]; float* maps; double* parts; };
static size_t lp_ws_layout(void* p, int H, int W, LpWs& w) {
  const size_t units = (size_t)H * W * 64;
  WsCursor c(p);
  for (int i = 0; i < 3; ++i) { w.hi[i] = c.take<__bf16>(units); w.lo[i] = c.take<__bf16>(units); }
  w.maps = c.take<float>(lp_map_floats(H, W));
  w.parts = c.take<double>(LP_TAPS * LP_PARTS);
  return c.bytes();
}

// the workspace of trase_lpips_head: both inputs' split planes, the map and the partial sums of its mean
struct LpHeadWs { __bf16* hi[2]; __bf16* lo[2]; float* map; double* parts; };
static size_t lp_head_layout(void* p, int C, int hw, LpHeadWs& w) {
  WsCursor c(p);
  for (int im = 0; im < 2; ++im) { w.hi[im] = c.take<__bf16>((size_t)C * hw); w.lo[im] = c.take<__bf16>((size_t)C * hw); }
  w.map = c.take<float>((size_t)hw);
  w.parts = c.take<double>(LP_PARTS);
  return c.bytes();
}

// ---- host side: the argument checks, each refusal once; they set the message and return the status ------------------------------
static int vg_check_cut(const char* who, int k) {
  if (k >= 1 && k <= VG_CUT_MAX) return TRASE_OK;
  set_error("%s: layers must be 1 .. 8 (conv1_1 .. conv4_1), got %d", who, k); return TRASE_ERR_INVALID;
}
// an image that every pool in front of the last layer run leaves at least one pixel of: sides of at least `need`
static int vg_check_image(const char* who, int need, int H, int W) {
  if (H >= need && W >= need && (int64_t)H * W < ((int64_t)1 << 25)) return TRASE_OK;
  set_error("%s: need H, W >= %d and H * W < 2^25 (got %d x %d)", who, need, H, W); return TRASE_ERR_INVALID;
}
static int vg_check_cut_image(const char* who, int k, int H, int W) {
  const int rc = vg_check_cut(who, k);
  return rc ? rc : vg_check_image(who, 1 << vg_shift(k), H, W);
}
static int lp_check_image(const char* who, int H, int W) { return vg_check_image(who, 1 << vg_shift(VG_LAYERS), H, W); }
static int vg_check_arrays(const char* who, int n, const float* const* weights, const float* const* biases) {
  for (int l = 0; l < n; ++l)
    if (!weights[l] || !biases[l]) { set_error("%s: null layer %d", who, l); return TRASE_ERR_INVALID; }
  return TRASE_OK;
}
static int vg_check_norm(const char* who, const float* mean, const float* inv_std) {
  if ((mean == nullptr) == (inv_std == nullptr)) return TRASE_OK;
  set_error("%s: mean and inv_std come together (both null: no normalisation)", who); return TRASE_ERR_INVALID;
}
// `what` names the buffers whose addresses were or-ed into `addresses`
static int vg_check_align16(const char* who, const char* what, size_t addresses) {
  if ((addresses & 15) == 0) return TRASE_OK;
  set_error("%s: %s must be 16-byte aligned", who, what); return TRASE_ERR_INVALID;
}
static int lp_check_align(const char* who, const char* out_name, const double* out, size_t fp32_addresses) {
  if (((size_t)out & 7) == 0 && (fp32_addresses & 3) == 0) return TRASE_OK;
  set_error("%s: %s must be 8-byte aligned, the fp32 buffers 4-byte aligned", who, out_name); return TRASE_ERR_INVALID;
}
// a buffer (`what`) of `have` bytes where `need` are wanted; `missing`: it is wanted and null
static int vg_check_room(const char* who, const char* what, size_t have, size_t need, bool missing = false) {
  if (!missing && have >= need) return TRASE_OK;
  set_error("%s: %s too small (%zu bytes, need %zu)", who, what, have, need); return TRASE_ERR_WORKSPACE;
}
// carves a filled pack for the forward and backward entries; the message says which cut when the pack is of a cut network
static int vg_check_pack(const char* who, VgPackSpec d, const void* pack, size_t pack_bytes, VgPack& p) {
  if (pack_bytes >= vg_pack_layout(const_cast<void*>(pack), d, p)) return TRASE_OK;
  if (d.layers < VG_LAYERS) set_error("%s: pack buffer too small for %d layers", who, d.layers);
  else set_error("%s: pack buffer too small", who);
  return TRASE_ERR_WORKSPACE;
}

// ---- host side: launches --------------------------------------------------------------------------------------------------------
static int vg_lg(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// forward layer l (>= 2) of an H x W image: geometry from the table, stream and bias from the pack; the caller sets the planes
// read and written and the epilogue's outputs
static VgConv vg_forward_conv(int l, int H, int W, const VgPack& p) {
  VgConv a{};
  a.stream = p.fwd[l]; a.bias = p.bias[l];
  a.H = H >> vg_shift(l); a.W = W >> vg_shift(l); a.Cin = vg_chan(l - 1); a.Cout = vg_chan(l); a.lg_steps = vg_lg(a.Cin / 16);
  return a;
}

template <int EPI>
static int vg_launch_conv(const VgConv& a, hipStream_t stream) {
  const dim3 grid(((a.W + VG_TILE - 1) / VG_TILE) * ((a.H + VG_TILE - 1) / VG_TILE), a.Cout / VG_NB);
  hipLaunchKernelGGL(vgg_conv_kernel<EPI>, grid, dim3(256), 0, stream, a);
  TRASE_POST_LAUNCH("vgg_conv", stream, 0);
  return TRASE_OK;
}

// the means of the first n maps of `m`, in two steps
static int lp_launch_means(const LpMeans& m, int n, double* parts, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(lpips_partial_kernel, dim3(LP_PARTS, n), dim3(256), 0, stream, m, parts);
  hipLaunchKernelGGL(lpips_mean_kernel, dim3(n), dim3(256), 0, stream, m, (const double*)parts, out);
  TRASE_POST_LAUNCH("lpips_means", stream, 0);
  return TRASE_OK;
}

// the profiling scopes' names: string literals, ProfScope keeps the pointer
#define VG_LAYER_NAMES(prefix)                                                                                                             \
  {"", prefix "conv1_1", prefix "conv1_2", prefix "conv2_1", prefix "conv2_2", prefix "conv3_1", prefix "conv3_2", prefix "conv3_3",       \
   prefix "conv4_1", prefix "conv4_2", prefix "conv4_3", prefix "conv5_1", prefix "conv5_2", prefix "conv5_3"}
static const char* const VG_FWD_NAMES[VG_LAYERS + 1] = VG_LAYER_NAMES("vgg_fwd_");
static const char* const VG_BWD_NAMES[VG_LAYERS + 1] = VG_LAYER_NAMES("vgg_bwd_");
static const char* const LP_CONV_NAMES[VG_LAYERS + 1] = VG_LAYER_NAMES("lpips_");
static const char* const LP_HEAD_NAMES[LP_TAPS] = {"lpips_head_relu1_2", "lpips_head_relu2_2", "lpips_head_relu3_3", "lpips_head_relu4_3",
                                                   "lpips_head_relu5_3"};

static VgNorm vg_norm(const float* mean, const float* inv_std) {
  VgNorm nm;
  for (int i = 0; i < 3; ++i) { nm.mean[i] = mean ? mean[i] : 0.f; nm.inv_std[i] = inv_std ? inv_std[i] : 1.f; }
  return nm;
}

}  // namespace trase

using namespace trase;

extern "C" {

int trase_vgg_ws_bytes(int32_t layers, int32_t H, int32_t W, size_t* pack_bytes, size_t* ws_forward_bytes, size_t* ws_backward_bytes,
                    size_t* saved_bytes, int32_t* C, int32_t* h, int32_t* w) {
  const char* who = "trase_vgg_ws_bytes";
  int rc = vg_check_cut_image(who, layers, H, W);
  if (rc) return rc;
  if (!pack_bytes || !ws_forward_bytes || !ws_backward_bytes || !saved_bytes || !C || !h || !w) {
    set_error("%s: null pointer", who); return TRASE_ERR_INVALID;
  }
  VgPack p; VgWs ws; VgSaved s;
  *pack_bytes = vg_pack_layout(nullptr, vg_pack_spec(layers), p);
  *ws_forward_bytes = vg_ws_layout(nullptr, layers, H, W, false, ws);
  *ws_backward_bytes = vg_ws_layout(nullptr, layers, H, W, true, ws);
  *saved_bytes = vg_saved_layout(nullptr, layers, H, W, s);
  *C = vg_chan(layers); *h = H >> vg_shift(layers); *w = W >> vg_shift(layers);
  return TRASE_OK;
}

int trase_vgg_pack(int32_t layers, const float* const* weights, const float* const* biases, void* pack, size_t pack_bytes,
                   int32_t device, trase_stream_t stream_) {
  const char* who = "trase_vgg_pack";
  int rc = vg_check_cut(who, layers);
  if (rc) return rc;
  if (!weights || !biases || !pack) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  if ((rc = vg_check_arrays(who, layers, weights, biases))) return rc;
  if ((rc = vg_check_align16(who, "the pack buffer", (size_t)pack))) return rc;
  VgPack p;
  if ((rc = vg_check_room(who, "pack buffer", pack_bytes, vg_pack_layout(pack, vg_pack_spec(layers), p)))) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCHES("vgg_pack", stream, 0, if ((rc = vg_launch_pack(vg_pack_spec(layers), weights, biases, nullptr, p, stream))) return rc);
  return TRASE_OK;
}

int trase_vgg_forward(int32_t layers, const void* pack, size_t pack_bytes, const float* image, int32_t H, int32_t W,
                      const float* mean, const float* inv_std, float* out, void* saved, size_t saved_bytes, void* ws,
                      size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  const char* who = "trase_vgg_forward";
  int rc = vg_check_cut_image(who, layers, H, W);
  if (rc) return rc;
  const int k = layers;
  if (!pack || !image || !out) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  if ((rc = vg_check_norm(who, mean, inv_std))) return rc;
  if ((rc = vg_check_align16(who, "pack, saved and ws", (size_t)pack | (size_t)ws | (size_t)saved))) return rc;
  VgPack p; VgWs b; VgSaved s;
  if ((rc = vg_check_pack(who, vg_pack_spec(k), pack, pack_bytes, p))) return rc;
  const size_t ws_need = vg_ws_layout(ws, k, H, W, false, b);
  if ((rc = vg_check_room(who, "workspace", ws_bytes, ws_need, ws_need > 0 && !ws))) return rc;
  if (saved && (rc = vg_check_room(who, "saved buffer", saved_bytes, vg_saved_layout(saved, k, H, W, s)))) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const VgNorm nm = vg_norm(mean, inv_std);
  const dim3 grid((unsigned)(((size_t)H * W + 255) / 256));
  TRASE_LAUNCHES_AS(VG_FWD_NAMES[1], "vgg_fwd_conv1_1", stream, 0,
    if (k == 1)
      hipLaunchKernelGGL(vgg_conv1_kernel<true>, grid, dim3(256), 0, stream, image, H, W, nm, p.w1, p.bias[1], (__bf16*)nullptr,
                         (__bf16*)nullptr, out, (uint16_t*)nullptr);
    else
      hipLaunchKernelGGL(vgg_conv1_kernel<false>, grid, dim3(256), 0, stream, image, H, W, nm, p.w1, p.bias[1], b.hi[1], b.lo[1],
                         (float*)nullptr, saved ? s.relu[1] : nullptr));
  for (int l = 2; l <= k; ++l) {
    VgConv a = vg_forward_conv(l, H, W, p);
    a.in_hi = b.hi[(l - 1) & 1]; a.in_lo = b.lo[(l - 1) & 1];
    a.out_hi = b.hi[l & 1]; a.out_lo = b.lo[l & 1];
    TRASE_LAUNCHES_AS(VG_FWD_NAMES[l], "vgg_fwd_conv", stream, 0,
      if (l == k) { a.out_f32 = out; rc = vg_launch_conv<VG_FWD_OUT>(a, stream); }
      else if (vg_pooled(l)) { a.pool_codes = saved ? s.pool[l] : nullptr; rc = vg_launch_conv<VG_FWD_POOL>(a, stream); }
      else { a.relu_bits = saved ? s.relu[l] : nullptr; rc = vg_launch_conv<VG_FWD_RELU>(a, stream); }
      if (rc) return rc);
  }
  return TRASE_OK;
}

int trase_vgg_backward(int32_t layers, const void* pack, size_t pack_bytes, const float* d_out, int32_t H, int32_t W,
                       const float* inv_std, const void* saved, size_t saved_bytes, float* d_image, void* ws, size_t ws_bytes,
                       int32_t device, trase_stream_t stream_) {
  const char* who = "trase_vgg_backward";
  int rc = vg_check_cut_image(who, layers, H, W);
  if (rc) return rc;
  const int k = layers;
  if (!pack || !d_out || !d_image || !ws || (k > 1 && !saved)) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  if ((rc = vg_check_align16(who, "pack, saved and ws", (size_t)pack | (size_t)ws | (size_t)saved))) return rc;
  VgPack p; VgWs b; VgSaved s;
  if ((rc = vg_check_pack(who, vg_pack_spec(k), pack, pack_bytes, p))) return rc;
  if ((rc = vg_check_room(who, "workspace", ws_bytes, vg_ws_layout(ws, k, H, W, true, b)))) return rc;
  if ((rc = vg_check_room(who, "saved buffer", saved_bytes, vg_saved_layout(const_cast<void*>(saved), k, H, W, s)))) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const int hw = (int)vg_pixels(k, H, W);
  TRASE_LAUNCH("vgg_bwd_split", stream, 0, vgg_cot_split_kernel, dim3((hw + 255) / 256, vg_chan(k) / 8), dim3(256), 0, d_out, vg_chan(k), hw,
               b.hi[k & 1], b.lo[k & 1]);
  for (int l = k; l >= 2; --l) {                   // the cotangent of layer l's output -> that of layer l - 1's
    VgConv a{};                                    // not vg_forward_conv: Cin and Cout are exchanged and there is no bias
    a.in_hi = b.hi[l & 1]; a.in_lo = b.lo[l & 1];
    a.stream = p.bwd[l]; a.bias = nullptr;
    a.H = H >> vg_shift(l); a.W = W >> vg_shift(l); a.Cin = vg_chan(l); a.Cout = vg_chan(l - 1); a.lg_steps = vg_lg(a.Cin / 16);
    a.out_hi = b.hi[(l - 1) & 1]; a.out_lo = b.lo[(l - 1) & 1];
    TRASE_LAUNCHES_AS(VG_BWD_NAMES[l], "vgg_bwd_conv", stream, 0,
      if (vg_pooled(l - 1)) {
        a.out_H = H >> vg_shift(l - 1); a.out_W = W >> vg_shift(l - 1);
        if ((a.out_H | a.out_W) & 1) {               // an odd last row / column lies in no window
          const size_t bytes = vg_pixels(l - 1, H, W) * vg_chan(l - 1) * sizeof(__bf16);
          rc = launch_zero_bytes(a.out_hi, bytes, stream); if (rc) return rc;
          rc = launch_zero_bytes(a.out_lo, bytes, stream); if (rc) return rc;
        }
        a.pool_codes = const_cast<uint64_t*>(s.pool[l - 1]);
        rc = vg_launch_conv<VG_BWD_UNPOOL>(a, stream);
      } else {
        a.relu_bits = const_cast<uint16_t*>(s.relu[l - 1]);
        rc = vg_launch_conv<VG_BWD_MASK>(a, stream);
      }
      if (rc) return rc);
  }
  const VgNorm nm = vg_norm(nullptr, inv_std);
  TRASE_LAUNCHES_AS(VG_BWD_NAMES[1], "vgg_bwd_conv1_1", stream, 0,
    hipLaunchKernelGGL(vgg_image_grad_kernel, dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, stream, b.hi[1], b.lo[1], H, W, nm,
                       (const float4*)p.w1t, d_image));
  return TRASE_OK;
}

int trase_lpips_ws_bytes(int32_t H, int32_t W, size_t* pack_bytes, size_t* ws_bytes, size_t* map_floats) {
  const char* who = "trase_lpips_ws_bytes";
  int rc = lp_check_image(who, H, W);
  if (rc) return rc;
  if (!pack_bytes || !ws_bytes || !map_floats) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  VgPack p; LpWs ws;
  *pack_bytes = vg_pack_layout(nullptr, LP_PACK_SPEC, p);
  *ws_bytes = lp_ws_layout(nullptr, H, W, ws);
  *map_floats = lp_map_floats(H, W);
  return TRASE_OK;
}

int trase_lpips_pack(const float* const* weights, const float* const* biases, const float* const* lin, void* pack, size_t pack_bytes,
                     int32_t device, trase_stream_t stream_) {
  const char* who = "trase_lpips_pack";
  if (!weights || !biases || !lin || !pack) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  int rc = vg_check_arrays(who, VG_LAYERS, weights, biases);
  if (rc) return rc;
  for (int t = 0; t < LP_TAPS; ++t)
    if (!lin[t]) { set_error("%s: null lin %d", who, t); return TRASE_ERR_INVALID; }
  if ((rc = vg_check_align16(who, "the pack buffer", (size_t)pack))) return rc;
  VgPack p;
  if ((rc = vg_check_room(who, "pack buffer", pack_bytes, vg_pack_layout(pack, LP_PACK_SPEC, p)))) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCHES("lpips_pack", stream, 0, if ((rc = vg_launch_pack(LP_PACK_SPEC, weights, biases, lin, p, stream))) return rc);
  return TRASE_OK;
}

int trase_lpips_forward(const void* pack, size_t pack_bytes, const float* x, const float* y, int32_t H, int32_t W, const float* mean,
                        const float* inv_std, double* out_layers, float* maps, float* taps_x, float* taps_y, void* ws, size_t ws_bytes,
                        int32_t device, trase_stream_t stream_) {
  const char* who = "trase_lpips_forward";
  int rc = lp_check_image(who, H, W);
  if (rc) return rc;
  if (!pack || !x || !y || !out_layers || !ws) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  if ((rc = vg_check_norm(who, mean, inv_std))) return rc;
  if ((taps_x == nullptr) != (taps_y == nullptr)) { set_error("%s: taps_x and taps_y come together", who); return TRASE_ERR_INVALID; }
  if ((rc = vg_check_align16(who, "pack and ws", (size_t)pack | (size_t)ws))) return rc;
  if ((rc = lp_check_align(who, "out_layers", out_layers, (size_t)x | (size_t)y | (size_t)maps | (size_t)taps_x | (size_t)taps_y))) return rc;
  VgPack p; LpWs b;
  if ((rc = vg_check_pack(who, LP_PACK_SPEC, pack, pack_bytes, p))) return rc;
  if ((rc = vg_check_room(who, "workspace", ws_bytes, lp_ws_layout(ws, H, W, b)))) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const VgNorm nm = vg_norm(mean, inv_std);
  const float* img[2] = {x, y};
  float* taps[2] = {taps_x, taps_y};
  float* const map_base = maps ? maps : b.maps;
  LpMeans means{};
  struct Planes { __bf16* hi; __bf16* lo; };
  const size_t half = (size_t)H * W * 32;          // elements of half a buffer
  auto halves = [&](int buf, int im) { return Planes{b.hi[buf] + im * half, b.lo[buf] + im * half}; };
  Planes cur[2] = {};                               // where each image's newest activation lives
  int deep = 0, tap = 0;                            // behind the first pool: the buffer (1 or 2) whose halves hold `cur`
  size_t map_off = 0, tap_off = 0;
  for (int l = 1; l <= VG_LAYERS; ++l) {
    const int h = H >> vg_shift(l), w = W >> vg_shift(l), hw = h * w, c = vg_chan(l);
    TRASE_LAUNCHES_AS(LP_CONV_NAMES[l], "lpips_conv", stream, 0,
      for (int im = 0; im < 2; ++im) {
        if (l == 1) {
          cur[im] = Planes{b.hi[im], b.lo[im]};
          hipLaunchKernelGGL(vgg_conv1_kernel<false>, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, stream, img[im], H, W, nm, p.w1,
                             p.bias[1], cur[im].hi, cur[im].lo, (float*)nullptr, (uint16_t*)nullptr);
        } else {
          const Planes dst = l == 2 ? (im == 0 ? Planes{b.hi[2], b.lo[2]} : Planes{b.hi[0], b.lo[0]}) : halves(3 - deep, im);
          VgConv a = vg_forward_conv(l, H, W, p);
          a.in_hi = cur[im].hi; a.in_lo = cur[im].lo;
          a.out_hi = dst.hi; a.out_lo = dst.lo;
          if ((rc = vg_launch_conv<VG_FWD_RELU>(a, stream))) return rc;
          cur[im] = dst;
        }
      });
    if (l > 2) deep = 3 - deep;
    if (l != LP_TAP_LAYER[tap]) continue;
    TRASE_LAUNCHES_AS(LP_HEAD_NAMES[tap], "lpips_head", stream, 0,
      hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)((hw + 31) / 32)), dim3(256), 0, stream, cur[0].hi, cur[0].lo, cur[1].hi, cur[1].lo, c,
                         hw, p.lin[tap], map_base + map_off);
      for (int im = 0; im < 2; ++im) {
        if (taps[im])
          hipLaunchKernelGGL(lpips_tap_kernel, dim3((unsigned)((hw + 255) / 256), c / 8), dim3(256), 0, stream, cur[im].hi, cur[im].lo, c, hw,
                             taps[im] + tap_off);
        if (vg_pooled(l)) {                         // the first pool goes to buffer 1, whose conv1_1 output of y is spent
          const Planes dst = halves(l == 2 ? 1 : 3 - deep, im);
          const size_t n = (size_t)(h >> 1) * (w >> 1) * (c / 8);
          hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, cur[im].hi, cur[im].lo, h, w, c, dst.hi,
                             dst.lo);
          cur[im] = dst;
        }
      });
    means.map[tap] = map_base + map_off; means.n[tap] = hw;
    map_off += (size_t)hw; tap_off += (size_t)hw * c;
    if (vg_pooled(l)) deep = l == 2 ? 1 : 3 - deep;
    ++tap;
  }
  TRASE_LAUNCHES("lpips_mean", stream, 0, if ((rc = lp_launch_means(means, LP_TAPS, b.parts, out_layers, stream))) return rc);
  return TRASE_OK;
}

int trase_lpips_head(const float* a, const float* b, const float* lin, int32_t C, int32_t hw, double* out_layer, float* map, void* ws,
                     size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  const char* who = "trase_lpips_head";
  if ((C != 64 && C != 128 && C != 256 && C != 512) || hw < 1 || (int64_t)C * hw >= ((int64_t)1 << 31)) {
    set_error("%s: need C in {64, 128, 256, 512}, hw >= 1 and C * hw < 2^31 (got C %d, hw %d)", who, C, hw); return TRASE_ERR_INVALID;
  }
  if (!a || !b || !lin || !out_layer || !ws) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  int rc = vg_check_align16(who, "ws", (size_t)ws);
  if (rc) return rc;
  if ((rc = lp_check_align(who, "out_layer", out_layer, (size_t)a | (size_t)b | (size_t)lin | (size_t)map))) return rc;
  LpHeadWs w;
  if ((rc = vg_check_room(who, "workspace", ws_bytes, lp_head_layout(ws, C, hw, w)))) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const float* in[2] = {a, b};
  float* const m = map ? map : w.map;
  LpMeans means{};
  means.map[0] = m; means.n[0] = hw;
  TRASE_LAUNCHES("lpips_head", stream, 0,
    for (int im = 0; im < 2; ++im)
      hipLaunchKernelGGL(vgg_cot_split_kernel, dim3((hw + 255) / 256, C / 8), dim3(256), 0, stream, in[im], C, hw, w.hi[im], w.lo[im]);
    hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)((hw + 31) / 32)), dim3(256), 0, stream, w.hi[0], w.lo[0], w.hi[1], w.lo[1], C, hw, lin, m);
    if ((rc = lp_launch_means(means, 1, w.parts, out_layer, stream))) return rc);
  return TRASE_OK;
}

}  // extern "C"
