// frames.hip -- a view's ground truth kept as bytes on the device (trase_amd/frames.py, ByteFrame).
// The reference builds every ground-truth frame from a byte array (PILtoTorch, utils/general_utils.py:22-28) and keeps it as
// fp32, 24.9 MB per 1080p frame; the planar 8-bit frame is 6.2 MB and the loss kernels (loss.hip, GtBytes) read it in place.
//   frame_pack_kernel      : (H, W, 3 | 4) bytes -> three planes, rows `pitch` bytes apart; optionally the RGBA-over-background
//                            composite of train.py:221-228, in float64 with every operation rounded on its own (this file is
//                            compiled with -ffp-contract=off: the default would fuse nv * na + bg * (1 - na) into an fma)
//   frame_unpack_kernel    : the planes -> (3, H, W) fp32, the true quotient b / 255
//   frame_black_mask_kernel: r | g | b == 0 per pixel, or per destination pixel of the bilinear resize of train.py:267-268
//   frame_resize_kernel    : Pillow's 8-bit bicubic resize (PILtoTorch's pil_image.resize(resolution)) from any of the four sources
//                            to the planes, both passes in one launch: coefficient tables, source strip and the horizontally
//                            resampled bytes live in LDS
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

// ---- Pillow's resize (mode "RGB", BICUBIC): ImagingResample's coefficient rows and its two 8-bit passes ------------------------------
// Per axis: scale = in / out, filterscale = max(scale, 1), support = 2 * filterscale, ksize = (int)ceil(support) * 2 + 1; per output
// index the taps xmin .. xmin + n - 1 and their weights, normalised by their sum taken in tap order and rounded to 22 fractional
// bits.  Every double operation below is Pillow's, in its order (this file is compiled with -ffp-contract=off).
constexpr int RS_TW = 64;              // output columns of a tile: 16 dwords of a plane row
constexpr int RS_INTER_ROWS = 128;     // most source rows a tile's vertical taps may span (the host picks the tile height by it)
constexpr int RS_STAGE = 3072;         // source pixels staged per batch of rows, one dword each
constexpr int RS_MAX_SHRINK = 16;      // in <= 16 * out per axis: ksize <= 65

struct ResizeAxis { double scale, support, ss; int in, ksize; };

__host__ __device__ inline ResizeAxis resize_axis(int in, int out) {
  ResizeAxis a;
  a.in = in;
  a.scale = (double)in / (double)out;
  const double filterscale = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = 2.0 * filterscale;
  a.ksize = (int)ceil(a.support) * 2 + 1;
  a.ss = 1.0 / filterscale;
  return a;
}

__host__ __device__ inline double resize_bounds(const ResizeAxis& a, int xx, int& xmin, int& n) {
  const double center = ((double)xx + 0.5) * a.scale;
  xmin = (int)(center - a.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + a.support + 0.5);
  if (xmax > a.in) xmax = a.in;
  n = xmax - xmin;
  return center;
}

__device__ __forceinline__ double bicubic_weight(double t) {
  const double a = -0.5;
  if (t < 0.0) t = -t;
  if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1;
  if (t < 2.0) return (((t - 5) * t + 8) * t - 4) * a;
  return 0.0;
}

// the coefficient row of output index xx: ksize ints at coef (LDS or global), zero beyond n.  The weights are evaluated twice, for
// the sum and for the quotient: the same operations on the same values, so no per-thread array is needed.
__device__ inline void resize_coeffs(const ResizeAxis& a, int xx, int* coef, int& xmin, int& n) {
  const double center = resize_bounds(a, xx, xmin, n);
  double ww = 0.0;
  for (int x = 0; x < n; ++x) ww += bicubic_weight(((double)(x + xmin) - center + 0.5) * a.ss);
  for (int x = 0; x < a.ksize; ++x) {
    int q = 0;
    if (x < n) {
      double k = bicubic_weight(((double)(x + xmin) - center + 0.5) * a.ss);
      if (ww != 0.0) k /= ww;
      q = k < 0 ? (int)(k * 4194304.0 - 0.5) : (int)(k * 4194304.0 + 0.5);
    }
    coef[x] = q;
  }
}

// clamp(s >> 22, 0, 255), written as the clamp of s followed by the shift (the same value: the shift is monotone).  The direct
// form compiles to v_ashr_pk_u8_i32 for two neighbouring bytes, and the compiler then ORs the other two bytes into that
// register as if its upper half were zero; on the MI355X the upper half kept what the register held before (bytes 2 and 3 of
// the vertical pass came out with stray bits set, only ever added ones).
__device__ __forceinline__ uint32_t resize_clip8(int s) {
  s = s < 0 ? 0 : (s > 0x3fffffff ? 0x3fffffff : s);
  return (uint32_t)s >> 22;
}

struct ResizeArgs {
  const uint8_t* src; int sH, sW, sP;      // sP: bytes from row to row of a planar source
  uint8_t* planes; int H, W, pitch;
  int TH, tiles_x, rb, inter_rows;         // tile height, tiles per row of tiles, source rows per staged batch, rows of `inter`
  FrameBg bg;
};

// source loaders: one pixel as r | g << 8 | b << 16.  None reads a byte outside its pixel.
struct SrcRgb {
  static __device__ __forceinline__ uint32_t load(const ResizeArgs& a, int y, int x) {
    const uint8_t* p = a.src + ((size_t)y * a.sW + x) * 3;
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
  }
};
template <bool COMPOSITE>
struct SrcRgba {
  static __device__ __forceinline__ uint32_t load(const ResizeArgs& a, int y, int x) {
    const uint8_t* p = a.src + ((size_t)y * a.sW + x) * 4;
    uint32_t v;
    if (((size_t)a.src & 3) == 0) v = *reinterpret_cast<const uint32_t*>(p);       // (uniform) the pixel's own dword
    else v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    if (COMPOSITE) {
      const uint32_t al = v >> 24;
      v = composite_byte(v & 0xffu, al, a.bg.c[0]) | composite_byte((v >> 8) & 0xffu, al, a.bg.c[1]) << 8 |
          composite_byte((v >> 16) & 0xffu, al, a.bg.c[2]) << 16;
    }
    return v & 0xffffffu;
  }
};
struct SrcPlanes {
  static __device__ __forceinline__ uint32_t load(const ResizeArgs& a, int y, int x) {
    const size_t pl = (size_t)a.sH * a.sP;
    const uint8_t* p = a.src + (size_t)y * a.sP + x;
    return (uint32_t)p[0] | (uint32_t)p[pl] << 8 | (uint32_t)p[2 * pl] << 16;
  }
};

// One workgroup per tile of RS_TW x TH output pixels.  LDS: the coefficient rows and (xmin, n) of the tile's columns and rows; a
// batch of source rows over the columns the tile's horizontal taps span, one dword per pixel (composited once); `inter`, the
// horizontally resampled BYTES of every source row the tile's vertical taps span (three planes of inter_rows x RS_TW).  An axis
// whose size does not change is not resampled: its bytes pass through.
template <class SRC>
__global__ __launch_bounds__(256) void frame_resize_kernel(ResizeArgs a) {
  extern __shared__ uint32_t rs_lds[];
  const int tid = threadIdx.x, TH = a.TH;
  const bool skipx = a.sW == a.W, skipy = a.sH == a.H;
  const ResizeAxis ax = resize_axis(a.sW, a.W), ay = resize_axis(a.sH, a.H);
  const int kx = skipx ? 0 : ax.ksize, ky = skipy ? 0 : ay.ksize;
  int* cx = reinterpret_cast<int*>(rs_lds);
  int* cy = cx + RS_TW * kx;
  int* bx = cy + TH * ky;
  int* by = bx + 2 * RS_TW;
  uint32_t* stage = reinterpret_cast<uint32_t*>(by + 2 * TH);
  uint8_t* inter = reinterpret_cast<uint8_t*>(stage + RS_STAGE);
  const int tile_y = (int)blockIdx.x / a.tiles_x, tile_x = (int)blockIdx.x - tile_y * a.tiles_x;
  const int x0 = tile_x * RS_TW, y0 = tile_y * TH;
  const int tw = min(RS_TW, a.W - x0), th = min(TH, a.H - y0);

  if (tid < RS_TW) {
    int xmin = 0, n = 0;
    if (tid < tw) {
      if (skipx) { xmin = x0 + tid; n = 1; }
      else resize_coeffs(ax, x0 + tid, cx + tid * kx, xmin, n);
    }
    bx[2 * tid] = xmin; bx[2 * tid + 1] = n;
  } else if (tid < RS_TW + TH) {
    const int r = tid - RS_TW;
    int ymin = 0, n = 0;
    if (r < th) {
      if (skipy) { ymin = y0 + r; n = 1; }
      else resize_coeffs(ay, y0 + r, cy + r * ky, ymin, n);
    }
    by[2 * r] = ymin; by[2 * r + 1] = n;
  }
  __syncthreads();
  // (xmin and xmin + n do not decrease with the output index: the tile's span is from its first to its last column / row)
  const int col0 = bx[0], colspan = bx[2 * (tw - 1)] + bx[2 * (tw - 1) + 1] - col0;
  const int row0 = by[0], rows = by[2 * (th - 1)] + by[2 * (th - 1) + 1] - row0;
  if (rows > a.inter_rows || colspan * a.rb > RS_STAGE) return;      // never: the host sized both from the same bounds

  const int pl = a.inter_rows * RS_TW;
  for (int r0 = 0; r0 < rows; r0 += a.rb) {
    const int nr = min(a.rb, rows - r0);
    for (int i = tid; i < nr * colspan; i += 256) {
      const int r = i / colspan, c = i - r * colspan;
      stage[i] = SRC::load(a, row0 + r0 + r, col0 + c);
    }
    __syncthreads();
    for (int i = tid; i < nr * RS_TW; i += 256) {
      const int r = i >> 6, c = i & (RS_TW - 1);
      uint32_t px = 0u;
      if (skipx) {
        if (c < tw) px = stage[r * colspan + c];
      } else {
        const int n = bx[2 * c + 1];
        const uint32_t* sp = stage + r * colspan + (bx[2 * c] - col0);
        const int* k = cx + c * kx;
        int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
        for (int x = 0; x < n; ++x) {
          const uint32_t p = sp[x];
          const int q = k[x];
          s0 += q * (int)(p & 0xffu);
          s1 += q * (int)((p >> 8) & 0xffu);
          s2 += q * (int)((p >> 16) & 0xffu);
        }
        px = resize_clip8(s0) | resize_clip8(s1) << 8 | resize_clip8(s2) << 16;
      }
      uint8_t* ip = inter + (r0 + r) * RS_TW + c;
      ip[0] = (uint8_t)px; ip[pl] = (uint8_t)(px >> 8); ip[2 * pl] = (uint8_t)(px >> 16);
    }
    __syncthreads();
  }

  // one thread per dword of a plane row: four columns, the row padding (columns >= W hold 0 in `inter`) written as 0
  const int groups = min(RS_TW, a.pitch - x0) >> 2;
  for (int i = tid; i < 3 * th * (RS_TW / 4); i += 256) {
    const int g = i & (RS_TW / 4 - 1), t = i >> 4, ch = t / th, ty = t - ch * th;
    if (g >= groups) continue;
    const uint8_t* ip = inter + ch * pl + 4 * g;
    uint32_t out;
    if (skipy) {
      out = *reinterpret_cast<const uint32_t*>(ip + ty * RS_TW);
    } else {
      const int n = by[2 * ty + 1];
      ip += (by[2 * ty] - row0) * RS_TW;
      const int* k = cy + ty * ky;
      int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21, s3 = 1 << 21;
      for (int y = 0; y < n; ++y) {
        const uint32_t p = *reinterpret_cast<const uint32_t*>(ip + y * RS_TW);
        const int q = k[y];
        s0 += q * (int)(p & 0xffu);
        s1 += q * (int)((p >> 8) & 0xffu);
        s2 += q * (int)((p >> 16) & 0xffu);
        s3 += q * (int)(p >> 24);
      }
      out = resize_clip8(s0) | resize_clip8(s1) << 8 | resize_clip8(s2) << 16 | resize_clip8(s3) << 24;
    }
    *reinterpret_cast<uint32_t*>(a.planes + ((size_t)ch * a.H + y0 + ty) * a.pitch + x0 + 4 * g) = out;
  }
}

// one thread per output index: the rows of trase_selftest_resize_tables
__global__ __launch_bounds__(256) void resize_tables_kernel(int in, int out, int* __restrict__ coeffs, int* __restrict__ bounds) {
  const int xx = blockIdx.x * 256 + threadIdx.x;
  if (xx >= out) return;
  const ResizeAxis a = resize_axis(in, out);
  int xmin, n;
  resize_coeffs(a, xx, coeffs + (size_t)xx * a.ksize, xmin, n);
  bounds[2 * xx] = xmin; bounds[2 * xx + 1] = n;
}

// the most source indices the taps of one tile of `tile` outputs span: the bounds the kernel computes, evaluated on the host
static int resize_tile_span(int in, int out, int tile) {
  if (in == out) return tile < out ? tile : out;
  const ResizeAxis a = resize_axis(in, out);
  int best = 0;
  for (int t0 = 0; t0 < out; t0 += tile) {
    const int last = (t0 + tile < out ? t0 + tile : out) - 1;
    int lo, n0, hi, n1;
    resize_bounds(a, t0, lo, n0);
    resize_bounds(a, last, hi, n1);
    if (hi + n1 - lo > best) best = hi + n1 - lo;
  }
  return best;
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
  TRASE_LAUNCHES("frame_pack", stream, 0,
    if (channels == 3) hipLaunchKernelGGL((frame_pack_kernel<3, false>), grid, dim3(256), 0, stream, hwc, H, W, pitch, bg, planes);
    else if (!background) hipLaunchKernelGGL((frame_pack_kernel<4, false>), grid, dim3(256), 0, stream, hwc, H, W, pitch, bg, planes);
    else hipLaunchKernelGGL((frame_pack_kernel<4, true>), grid, dim3(256), 0, stream, hwc, H, W, pitch, bg, planes));
  return TRASE_OK;
}

int trase_frame_resize(const uint8_t* src, int32_t src_H, int32_t src_W, int32_t src_layout, int32_t src_pitch, const float* background,
                       uint8_t* planes, int32_t H, int32_t W, int32_t pitch, int32_t device, trase_stream_t stream_) {
  const char* who = "trase_frame_resize";
  if (!src || !planes) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  if (src_layout != 3 && src_layout != 4 && src_layout != TRASE_FRAME_PLANAR) {
    set_error("%s: src_layout must be 3, 4 or TRASE_FRAME_PLANAR (got %d)", who, src_layout); return TRASE_ERR_INVALID;
  }
  if (background && src_layout != 4) { set_error("%s: a background needs the alpha of a 4-channel image", who); return TRASE_ERR_INVALID; }
  if (src_H < 1 || src_W < 1) { set_error("%s: need src_H, src_W >= 1 (got %d x %d)", who, src_H, src_W); return TRASE_ERR_INVALID; }
  if (src_layout == TRASE_FRAME_PLANAR && src_pitch < src_W) {
    set_error("%s: the source pitch must be at least src_W (got pitch %d, src_W %d)", who, src_pitch, src_W); return TRASE_ERR_INVALID;
  }
  if (int rc = frame_ok(who, planes, H, W, pitch)) return rc;
  if ((long long)src_H > (long long)RS_MAX_SHRINK * H || (long long)src_W > (long long)RS_MAX_SHRINK * W) {
    set_error("%s: an axis may shrink by at most %d (got %d x %d -> %d x %d)", who, RS_MAX_SHRINK, src_H, src_W, H, W); return TRASE_ERR_INVALID;
  }
  if (src_layout != TRASE_FRAME_PLANAR && src_H == H && src_W == W)                       // a copy: the bits of trase_frame_pack
    return trase_frame_pack(src, H, W, src_layout, background, planes, pitch, device, stream_);

  ResizeArgs a;
  a.src = src; a.sH = src_H; a.sW = src_W; a.sP = src_pitch;
  a.planes = planes; a.H = H; a.W = W; a.pitch = pitch;
  a.bg = {{0.0, 0.0, 0.0}};
  if (background)
    for (int c = 0; c < 3; ++c) a.bg.c[c] = (double)background[c];
  // the tallest tile whose span of source rows fits `inter`; at a shrink of 16 four rows span at most 3 * 16 + 66 source rows
  a.TH = 0;
  for (int th : {32, 16, 8, 4}) {
    a.inter_rows = resize_tile_span(src_H, H, th);
    if (a.inter_rows <= RS_INTER_ROWS) { a.TH = th; break; }
  }
  const int colspan = resize_tile_span(src_W, W, RS_TW);
  if (a.TH == 0 || colspan > RS_STAGE) { set_error("%s: no tile fits %d x %d -> %d x %d", who, src_H, src_W, H, W); return TRASE_ERR_INVALID; }
  a.rb = RS_STAGE / colspan < a.inter_rows ? RS_STAGE / colspan : a.inter_rows;
  a.tiles_x = (W + RS_TW - 1) / RS_TW;
  const long long tiles = (long long)a.tiles_x * ((H + a.TH - 1) / a.TH);
  const int kx = src_W == W ? 0 : resize_axis(src_W, W).ksize, ky = src_H == H ? 0 : resize_axis(src_H, H).ksize;
  const size_t lds = sizeof(int) * ((size_t)RS_TW * kx + (size_t)a.TH * ky + 2 * RS_TW + 2 * a.TH + RS_STAGE) + 3 * (size_t)a.inter_rows * RS_TW;
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const dim3 grid((unsigned)tiles);
  TRASE_LAUNCHES("frame_resize", stream, 0,
    if (src_layout == 3) hipLaunchKernelGGL((frame_resize_kernel<SrcRgb>), grid, dim3(256), lds, stream, a);
    else if (src_layout == TRASE_FRAME_PLANAR) hipLaunchKernelGGL((frame_resize_kernel<SrcPlanes>), grid, dim3(256), lds, stream, a);
    else if (!background) hipLaunchKernelGGL((frame_resize_kernel<SrcRgba<false>>), grid, dim3(256), lds, stream, a);
    else hipLaunchKernelGGL((frame_resize_kernel<SrcRgba<true>>), grid, dim3(256), lds, stream, a));
  return TRASE_OK;
}

int trase_selftest_resize_tables(int32_t in, int32_t out, int32_t* coeffs, int32_t* bounds, int32_t device, trase_stream_t stream_) {
  const char* who = "trase_selftest_resize_tables";
  if (!coeffs || !bounds) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  if (in < 1 || out < 1) { set_error("%s: need in, out >= 1 (got %d -> %d)", who, in, out); return TRASE_ERR_INVALID; }
  if ((long long)in > (long long)RS_MAX_SHRINK * out) {
    set_error("%s: an axis may shrink by at most %d (got %d -> %d)", who, RS_MAX_SHRINK, in, out); return TRASE_ERR_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(resize_tables_kernel, dim3((unsigned)((out + 255) / 256)), dim3(256), 0, stream, in, out, coeffs, bounds);
  TRASE_POST_LAUNCH("resize_tables", stream, 0);         // the check alone: a test entry point, never a key of the profiler report
  return TRASE_OK;
}

int trase_frame_unpack(const uint8_t* planes, int32_t H, int32_t W, int32_t pitch, float* chw, int32_t device, trase_stream_t stream_) {
  const char* who = "trase_frame_unpack";
  if (!planes || !chw) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  if (int rc = frame_ok(who, planes, H, W, pitch)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCH("frame_unpack", stream, 0, frame_unpack_kernel, dim3((unsigned)((3ll * H * ((W + 3) / 4) + 255) / 256)), dim3(256), 0, planes, H, W, pitch,
               chw);
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
  TRASE_LAUNCH("frame_black_mask", stream, 0, frame_black_mask_kernel, dim3((unsigned)(((long long)h * w + 255) / 256)), dim3(256), 0, planes, H, W, pitch, h, w,
               (float)H / (float)h, (float)W / (float)w, mask);
  return TRASE_OK;
}

}  // extern "C"
