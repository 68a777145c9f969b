// layers.hip -- the two launches around the one rasterizer pass of trase_amd.layers.render_layers: up to ten per-Gaussian colour
// tables ride through the compositing kernels as feature channels 3l .. 3l+2 (DESIGN.md "Colour layers in the feature
// channels") and come out as ten more images of the same view.
//
// layers_pack_kernel, one launch: L tables of (P,3) fp32 -> the (P,32) fp32 feature block, row i = [c0[i].rgb, c1[i].rgb, ...,
// 0 ... 0].  A workgroup owns LAYERS_ROWS rows.  A table's 3 * LAYERS_ROWS floats of those rows are one contiguous run: the
// workgroup reads it as consecutive dwords (a table base is only 4-byte aligned: a view one float off its storage is a valid
// table) into its own LDS plane; then eight lanes write each 128-byte row with one 16-byte store per lane, a wave 8 whole
// rows = 1 KB per store instruction.  Columns 3L .. 31 are +0.0f.  Rows at or past P are neither read nor written.
//
// layers_finish_kernel, one launch over the frame, evaluate.hip's quad walk: a thread owns 4 consecutive pixels of a row, 16-byte
// accesses where the quad is whole and every plane offset a multiple of 4 pixels, scalar ones for row tails and W % 4 != 0.
// It reads final_T once and writes plane[3l + c] = fmaf(T, bg[c], plane[3l + c]) in place for l < L -- the colour epilogue
// of the compositing kernel (render_fwd_mf.hip), which the feature channels do not get there.  With the 8-bit outputs the
// same pass writes to8b of the image and of every finished layer as (H,W,3) bytes.  No atomics: bitwise reproducible.
#include "common.h"
#include "frame_quads.h"

namespace trase {

constexpr int LAYERS_THREADS = 256;
constexpr int LAYERS_ROWS = 256;                       // rows of the feature block per workgroup
constexpr int LAYERS_MAX_BLOCKS = 2048;                // finish: grid-stride above this many workgroups
static_assert(3 * TRASE_LAYERS_MAX <= LAYERS_F, "every layer needs three feature channels");

struct LayersPackArgs {
  const float* tab[TRASE_LAYERS_MAX];
  float* out;                // (P, 32), 16-byte aligned
  int P, L;
};

__global__ __launch_bounds__(LAYERS_THREADS) void layers_pack_kernel(LayersPackArgs a) {
  __shared__ float stage[TRASE_LAYERS_MAX][3 * LAYERS_ROWS];
  const int r0 = blockIdx.x * LAYERS_ROWS;
  const int n = min(LAYERS_ROWS, a.P - r0);            // >= 1: the grid is ceil(P / LAYERS_ROWS)
  for (int l = 0; l < a.L; ++l) {
    const float* src = a.tab[l] + 3 * (size_t)r0;
    for (int k = threadIdx.x; k < 3 * n; k += LAYERS_THREADS) stage[l][k] = src[k];
  }
  __syncthreads();
  const int part = threadIdx.x & 7;                    // which 16 bytes of the row
  const int c0 = 4 * part;
  for (int r = threadIdx.x >> 3; r < n; r += LAYERS_THREADS / 8) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + u, l = c / 3;
      v[u] = l < a.L ? stage[l][3 * r + (c - 3 * l)] : 0.0f;
    }
    *reinterpret_cast<float4*>(a.out + (size_t)(r0 + r) * LAYERS_F + c0) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

int launch_layers_pack(const float* const* tables, int L, int P, float* out, hipStream_t stream) {
  if (P == 0) return TRASE_OK;
  LayersPackArgs a;
  for (int l = 0; l < TRASE_LAYERS_MAX; ++l) a.tab[l] = l < L ? tables[l] : nullptr;
  a.out = out; a.P = P; a.L = L;
  const int blocks = (P + LAYERS_ROWS - 1) / LAYERS_ROWS;
  TRASE_LAUNCH("layers_pack", stream, 0, layers_pack_kernel, dim3(blocks), dim3(LAYERS_THREADS), 0, a);
  return TRASE_OK;
}

struct LayersFinishArgs {
  float* planes;             // (32, H, W); planes 0 .. 3L-1 are finished in place
  const float* final_T;      // (H, W), or nullptr: the planes are final already (8-bit frames only)
  const float* bg;           // 3 floats on the device
  const float* image;        // (3, H, W) or nullptr
  uint8_t* image_u8;         // (H, W, 3) or nullptr
  uint8_t* layers_u8;        // (L, H, W, 3) or nullptr
  int W, H, L;
  int vec_ok;                // every pointer is aligned for the 16-byte / dword accesses and W * H is a multiple of 4
};

__device__ __forceinline__ void st_hwc(uint8_t* p, bool vec, int n, const float (&px)[3][4]) {
  uint32_t w[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 12; ++k) w[k >> 2] |= to8b(px[k % 3][k / 3]) << (8 * (k & 3));
  st12b(p, vec, n, w);
}

__global__ __launch_bounds__(LAYERS_THREADS) void layers_finish_kernel(LayersFinishArgs a) {
  const int W = a.W, Q = (W + 3) >> 2, items = Q * a.H;
  const size_t hw = (size_t)W * a.H;
  float bg[3] = {0.f, 0.f, 0.f};
  if (a.final_T) { bg[0] = a.bg[0]; bg[1] = a.bg[1]; bg[2] = a.bg[2]; }

  for (int it = blockIdx.x * LAYERS_THREADS + threadIdx.x; it < items; it += gridDim.x * LAYERS_THREADS) {
    const int row = it / Q, q = it - row * Q;
    const int n = min(4, W - 4 * q);
    const size_t p0 = (size_t)row * W + 4 * q;
    const bool vec = a.vec_ok && n == 4 && (p0 & 3) == 0;

    float T[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.final_T) ld4f(a.final_T + p0, vec, n, T);
    float px[3][4];
    if (a.image_u8) {
#pragma unroll
      for (int c = 0; c < 3; ++c) ld4f(a.image + c * hw + p0, vec, n, px[c]);
      st_hwc(a.image_u8 + 3 * p0, vec, n, px);
    }
    for (int l = 0; l < a.L; ++l) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float* const plane = a.planes + (size_t)(3 * l + c) * hw + p0;
        ld4f(plane, vec, n, px[c]);
        if (a.final_T) {
#pragma unroll
          for (int u = 0; u < 4; ++u) px[c][u] = fmaf(T[u], bg[c], px[c][u]);
          st4f(plane, vec, n, px[c]);
        }
      }
      if (a.layers_u8) st_hwc(a.layers_u8 + 3 * ((size_t)l * hw + p0), vec, n, px);
    }
  }
}

static inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int launch_layers_finish(float* planes, const float* final_T, const float* bg, int L, int W, int H, const float* image,
                         uint8_t* image_u8, uint8_t* layers_u8, hipStream_t stream) {
  if (W == 0 || H == 0) return TRASE_OK;
  LayersFinishArgs a;
  a.planes = planes; a.final_T = final_T; a.bg = bg; a.image = image; a.image_u8 = image_u8; a.layers_u8 = layers_u8;
  a.W = W; a.H = H; a.L = L;
  const size_t hw = (size_t)W * H;
  a.vec_ok = (hw & 3) == 0 && aligned(planes, 16) && aligned(final_T, 16) && aligned(image, 16) && aligned(image_u8, 4) &&
             aligned(layers_u8, 4);
  const int items = ((W + 3) / 4) * H;
  int blocks = (items + LAYERS_THREADS - 1) / LAYERS_THREADS;
  if (blocks > LAYERS_MAX_BLOCKS) blocks = LAYERS_MAX_BLOCKS;
  TRASE_LAUNCH("layers_finish", stream, 0, layers_finish_kernel, dim3(blocks), dim3(LAYERS_THREADS), 0, a);
  return TRASE_OK;
}

}  // namespace trase
