// frames.hip -- a view's ground truth kept as bytes on the device (trase_amd/frames.py, ByteFrame).
// The reference builds every ground-truth frame from a byte array (PILtoTorch, utils/general_utils.py:22-28) and keeps it as
// fp32, 24.9 MB per 1080p frame; the planar 8-bit frame is 6.2 MB and the loss kernels (loss.hip, GtBytes) read it in place.
//   frame_pack_kernel      : (H, W, 3 | 4) bytes -> three planes, rows `pitch` bytes apart; optionally the RGBA-over-background
//                            composite of train.py:221-228, in float64 with every operation rounded on its own (this file is
//                            compiled with -ffp-contract=off: the default would fuse nv * na + bg * (1 - na) into an fma)
//   frame_unpack_kernel    : the planes -> (3, H, W) fp32, the true quotient b / 255
//   frame_black_mask_kernel: r | g | b == 0 per pixel, or per destination pixel of the bilinear resize of train.py:267-268
#include "common.h"

namespace trase {

struct FrameBg { double c[3]; };

// np.array(arr * 255.0, dtype=np.byte) of train.py:226: the C conversion (toward zero), its low eight bits
__device__ __forceinline__ uint32_t composite_byte(uint32_t v, uint32_t a, double bg) {
  const double nv = (double)v / 255.0, na = (double)a / 255.0;
  const double p = nv * na;
  const double q = bg * (1.0 - na);
  const double arr = p + q;
  return (uint32_t)(int32_t)(arr * 255.0) & 0xffu;
}

// one thread per four pixels of a row (pitch / 4 groups per row): three dword stores, the row padding written as 0
template <int CH, bool COMPOSITE>
__global__ __launch_bounds__(256) void frame_pack_kernel(const uint8_t* __restrict__ hwc, int H, int W, int pitch, FrameBg bg,
                                                         uint8_t* __restrict__ planes) {
  const int groups = pitch >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)H * groups) return;
  const int y = (int)(i / groups), xg = (int)(i - (long long)y * groups) * 4;
  uint32_t out[3] = {0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = xg + j;
    if (x >= W) break;
    const uint8_t* px = hwc + ((size_t)y * W + x) * CH;
    uint32_t v[3] = {px[0], px[1], px[2]};
    if (COMPOSITE) {
      const uint32_t a = px[CH - 1];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = composite_byte(v[c], a, bg.c[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] |= v[c] << (8 * j);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(planes + ((size_t)c * H + y) * pitch + xg) = out[c];
}

// one thread per four pixels of a plane row: one dword load (it may take in row padding, never a byte past the row)
__global__ __launch_bounds__(256) void frame_unpack_kernel(const uint8_t* __restrict__ planes, int H, int W, int pitch,
                                                           float* __restrict__ chw) {
  const int groups = (W + 3) >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= 3ll * H * groups) return;
  const long long row = i / groups;                        // c * H + y
  const int xg = (int)(i - row * groups) * 4;
  const uint32_t v = *reinterpret_cast<const uint32_t*>(planes + (size_t)row * pitch + xg);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (xg + j < W) chw[(size_t)row * W + xg + j] = (float)((v >> (8 * j)) & 0xffu) / 255.0f;
}

// one thread per destination pixel.  The taps are ATen's (bilinear_source, common.h); a tap counts when both of its weights are
// non-zero, and the pixel is black when every such tap is 0 in all three planes: the interpolation's terms are non-negative and
// none of them can underflow (a weight is at least 2^-36 and a value at least 1 / 255), so their sum is 0 only if each is.
// At equal sizes the source coordinate is the destination's own, the second weights are 0 and one tap remains.
__global__ __launch_bounds__(256) void frame_black_mask_kernel(const uint8_t* __restrict__ planes, int H, int W, int pitch, int h, int w,
                                                               float scale_h, float scale_w, uint8_t* __restrict__ mask) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)h * w) return;
  const int oy = (int)(i / w), ox = (int)(i - (long long)oy * w);
  int y0, y1, x0, x1;
  float hl0, hl1, wl0, wl1;
  bilinear_source(scale_h, oy, H, y0, y1, hl0, hl1);
  bilinear_source(scale_w, ox, W, x0, x1, wl0, wl1);
  const size_t pl = (size_t)H * pitch;
  const int ys[2] = {y0, y1}, xs[2] = {x0, x1};
  const bool uy[2] = {hl0 != 0.f, hl1 != 0.f}, ux[2] = {wl0 != 0.f, wl1 != 0.f};
  uint32_t any = 0u;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
      if (uy[a] && ux[b]) {
        const size_t o = (size_t)ys[a] * pitch + xs[b];
        any |= (uint32_t)planes[o] | planes[pl + o] | planes[2 * pl + o];
      }
  mask[i] = any == 0u ? 1 : 0;
}

static int frame_ok(const char* who, const uint8_t* planes, int32_t H, int32_t W, int32_t pitch) {
  if (H < 1 || W < 1) { set_error("%s: need H, W >= 1 (got %d x %d)", who, H, W); return TRASE_ERR_INVALID; }
  if (pitch < W || (pitch & 15) != 0) {
    set_error("%s: pitch must be a multiple of 16 and at least W (got pitch %d, W %d)", who, pitch, W); return TRASE_ERR_INVALID;
  }
  if (((size_t)planes & 15) != 0) { set_error("%s: the planes must be 16-byte aligned", who); return TRASE_ERR_INVALID; }
  if ((long long)H * pitch > 0x7fffffffll / 3) { set_error("%s: a frame of %d x %d is more than one launch covers", who, H, W); return TRASE_ERR_INVALID; }
  return TRASE_OK;
}

}  // namespace trase

using namespace trase;

extern "C" {

int trase_frame_pack(const uint8_t* hwc, int32_t H, int32_t W, int32_t channels, const float* background, uint8_t* planes, int32_t pitch,
                     int32_t device, trase_stream_t stream_) {
  const char* who = "trase_frame_pack";
  if (!hwc || !planes) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  if (channels != 3 && channels != 4) { set_error("%s: channels must be 3 or 4 (got %d)", who, channels); return TRASE_ERR_INVALID; }
  if (background && channels != 4) { set_error("%s: a background needs the alpha of a 4-channel image", who); return TRASE_ERR_INVALID; }
  if (int rc = frame_ok(who, planes, H, W, pitch)) return rc;
  FrameBg bg = {{0.0, 0.0, 0.0}};
  if (background)
    for (int c = 0; c < 3; ++c) bg.c[c] = (double)background[c];
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const dim3 grid((unsigned)(((long long)H * (pitch / 4) + 255) / 256));
  {
    ProfScope ps("frame_pack", stream);
    if (channels == 3) hipLaunchKernelGGL((frame_pack_kernel<3, false>), grid, dim3(256), 0, stream, hwc, H, W, pitch, bg, planes);
    else if (!background) hipLaunchKernelGGL((frame_pack_kernel<4, false>), grid, dim3(256), 0, stream, hwc, H, W, pitch, bg, planes);
    else hipLaunchKernelGGL((frame_pack_kernel<4, true>), grid, dim3(256), 0, stream, hwc, H, W, pitch, bg, planes);
  }
  TRASE_POST_LAUNCH("frame_pack", stream, 0);
  return TRASE_OK;
}

int trase_frame_unpack(const uint8_t* planes, int32_t H, int32_t W, int32_t pitch, float* chw, int32_t device, trase_stream_t stream_) {
  const char* who = "trase_frame_unpack";
  if (!planes || !chw) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  if (int rc = frame_ok(who, planes, H, W, pitch)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  {
    ProfScope ps("frame_unpack", stream);
    hipLaunchKernelGGL(frame_unpack_kernel, dim3((unsigned)((3ll * H * ((W + 3) / 4) + 255) / 256)), dim3(256), 0, stream, planes, H, W, pitch,
                       chw);
  }
  TRASE_POST_LAUNCH("frame_unpack", stream, 0);
  return TRASE_OK;
}

int trase_frame_black_mask(const uint8_t* planes, int32_t H, int32_t W, int32_t pitch, int32_t h, int32_t w, uint8_t* mask, int32_t device,
                           trase_stream_t stream_) {
  const char* who = "trase_frame_black_mask";
  if (!planes || !mask) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  if (int rc = frame_ok(who, planes, H, W, pitch)) return rc;
  if (h < 1 || w < 1 || (long long)h * w > 0x7fffffffll) { set_error("%s: need h, w >= 1 and h * w < 2^31 (got %d x %d)", who, h, w); return TRASE_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  {
    ProfScope ps("frame_black_mask", stream);
    hipLaunchKernelGGL(frame_black_mask_kernel, dim3((unsigned)(((long long)h * w + 255) / 256)), dim3(256), 0, stream, planes, H, W, pitch, h, w,
                       (float)H / (float)h, (float)W / (float)w, mask);
  }
  TRASE_POST_LAUNCH("frame_black_mask", stream, 0);
  return TRASE_OK;
}

}  // extern "C"
