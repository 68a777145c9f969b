// display.hip -- the display stage of the reference's frame loop: point splats and PCA colours of the features.
//   render.py:247-294 (white dots, cluster colours, PCA colours; gui.py:984-1030, gui_standalone.py:1422-1470)
//   render.py:52-59 feature3d_to_rgb (gui.py:55-62, gui_standalone.py:490-497)
//
// Splat, three launches, all L images from ONE projection and ONE winner map:
//   1. splat_fill_kernel: the (H, W) int32 winner map = -1 (a kernel, not a memset node: common.h);
//   2. splat_project_kernel: one thread per point, p = [x, y, z, 1] @ full_proj_transform in float64 from the fp32 inputs,
//      px = (p.x / p.w + 1) / 2 * W, py likewise with H; the point lands if 0 < px < W and 0 < py < H (no near-plane or
//      w > 0 test, as in the reference; a non-finite coordinate fails the comparisons) at column trunc(px), row trunc(py):
//      atomicMax of the point index, so the winner of a pixel is the highest index landing there;
//   3. splat_resolve_kernel: four pixels per thread, every plane of every layer written with coalesced stores, colours
//      gathered for hit pixels only.
// Integer atomics only: bitwise reproducible.
//
// PCA colours: column means (block slabs, reduced in block order), the centred D x D Gram matrix Xc^T Xc (fp32 products and
// sums inside a block, block slabs reduced in block order in float64), the eigen-decomposition on the host, then one pass
// that projects every row on the three axes and takes the global min / max with integer atomics on the ordered-int image of
// the floats (min and max do not depend on the order), and one pass that normalises in place.  No float atomics.
#include "common.h"

namespace trase {

constexpr int SPLAT_MAX_L = 4;
constexpr int DISP_MAX_D = 64;
constexpr int DISP_MAX_BLOCKS = 256;          // about one block per CU
constexpr int DISP_ROWS = 64;                 // rows per LDS tile of the Gram kernel
constexpr int DISP_THREADS = 256;

struct SplatProj { double m[12]; };           // columns 0, 1 and 3 of full_proj_transform: m[4 * c + r]
struct SplatLayers {
  const float* colors[SPLAT_MAX_L];           // (N, 3) fp32 or null: the dot colour
  float* images[SPLAT_MAX_L];                 // (3, H, W) fp32
};

__global__ __launch_bounds__(256) void splat_fill_kernel(int32_t* __restrict__ winner, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) winner[i] = -1;
}

__global__ __launch_bounds__(256) void splat_project_kernel(const float* __restrict__ points, int N,
                                                            const uint8_t* __restrict__ mask, SplatProj P, int W, int H,
                                                            int32_t* __restrict__ winner) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (mask && !mask[i]) return;
  const double x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  const double px_h = x * P.m[0] + y * P.m[1] + z * P.m[2] + P.m[3];
  const double py_h = x * P.m[4] + y * P.m[5] + z * P.m[6] + P.m[7];
  const double w = x * P.m[8] + y * P.m[9] + z * P.m[10] + P.m[11];
  const double px = (px_h / w + 1.0) / 2.0 * (double)W;
  const double py = (py_h / w + 1.0) / 2.0 * (double)H;
  if (!(px > 0.0 && px < (double)W && py > 0.0 && py < (double)H)) return;     // NaN and inf land nowhere
  const int col = (int)px, row = (int)py;                                      // in [0, W - 1], [0, H - 1] by the test above
  atomicMax(&winner[(size_t)row * W + col], i);
}

__global__ __launch_bounds__(256) void splat_resolve_kernel(const int32_t* __restrict__ winner, int HW, int L, SplatLayers S,
                                                            float dot, float bg, int64_t* __restrict__ index_out) {
  const int p0 = 4 * (blockIdx.x * blockDim.x + threadIdx.x);
  if (p0 >= HW) return;
  const int n = min(4, HW - p0);
  int w[4];
  for (int u = 0; u < 4; ++u) w[u] = u < n ? winner[p0 + u] : -1;
  if (index_out)
    for (int u = 0; u < n; ++u) index_out[p0 + u] = w[u];
  for (int l = 0; l < L; ++l) {
    const float* col = S.colors[l];
    float v[3][4];
    for (int u = 0; u < 4; ++u)
      for (int c = 0; c < 3; ++c) v[c][u] = w[u] < 0 ? bg : col ? col[3 * (size_t)w[u] + c] : dot;
    for (int c = 0; c < 3; ++c) {
      float* out = S.images[l] + (size_t)c * HW + p0;
      if (n == 4 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
        *reinterpret_cast<float4*>(out) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
      } else {
        for (int u = 0; u < n; ++u) out[u] = v[c][u];
      }
    }
  }
}

// ---- PCA colours ------------------------------------------------------------------------------------------------------------

static inline int disp_dpad(int D) { return D <= 16 ? 16 : D <= 32 ? 32 : 64; }
static inline int disp_blocks(int N) {
  const int g = (N + DISP_ROWS - 1) / DISP_ROWS;
  return g < 1 ? 1 : g > DISP_MAX_BLOCKS ? DISP_MAX_BLOCKS : g;
}

// slab[b][d] = sum of column d over the rows [b * chunk, (b + 1) * chunk): thread (r, d) adds rows r, r + R, ... in order,
// then the R partial sums are added in r order
template <int DP>
__global__ __launch_bounds__(DISP_THREADS) void disp_colsum_kernel(const float* __restrict__ X, int N, int D, int chunk,
                                                                   float* __restrict__ slabs) {
  constexpr int R = DISP_THREADS / DP;
  __shared__ float part[DISP_THREADS];
  const int d = threadIdx.x % DP, r = threadIdx.x / DP;
  const int lo = blockIdx.x * chunk, hi = min(N, lo + chunk);
  float s = 0.f;
  if (d < D)
    for (int i = lo + r; i < hi; i += R) s += X[(size_t)i * D + d];
  part[threadIdx.x] = s;
  __syncthreads();
  if (r == 0 && d < D) {
    float t = 0.f;
    for (int q = 0; q < R; ++q) t += part[q * DP + d];
    slabs[(size_t)blockIdx.x * D + d] = t;
  }
}

// out[e] = scale * (sum over the G block slabs of element e, in block order, in float64)
__global__ __launch_bounds__(256) void disp_reduce_kernel(const float* __restrict__ slabs, int G, int E, double scale,
                                                          float* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  double t = 0.0;
  for (int g = 0; g < G; ++g) t += (double)slabs[(size_t)g * E + e];
  out[e] = (float)(t * scale);
}

// slab[b] = Xc^T Xc over the block's rows, Xc = X - mean.  Rows go through LDS in tiles of DISP_ROWS, centred and zero
// padded to DP columns; thread (ti, tj) of the 16 x 16 grid owns the T x T outputs (ti * T + u, tj * T + v), T = DP / 16,
// and adds the rows in order.
template <int DP>
__global__ __launch_bounds__(DISP_THREADS) void disp_gram_kernel(const float* __restrict__ X, int N, int D, int chunk,
                                                                 const float* __restrict__ mean, float* __restrict__ slabs) {
  constexpr int T = DP / 16;
  __shared__ float xs[DISP_ROWS * DP];
  __shared__ float mu[DP];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  if (tid < DP) mu[tid] = tid < D ? mean[tid] : 0.f;
  float acc[T][T];
#pragma unroll
  for (int u = 0; u < T; ++u)
#pragma unroll
    for (int v = 0; v < T; ++v) acc[u][v] = 0.f;
  const int lo = blockIdx.x * chunk, hi = min(N, lo + chunk);
  __syncthreads();
  for (int r0 = lo; r0 < hi; r0 += DISP_ROWS) {
    for (int e = tid; e < DISP_ROWS * DP; e += DISP_THREADS) {
      const int r = e / DP, d = e - r * DP;
      xs[e] = (d < D && r0 + r < hi) ? X[(size_t)(r0 + r) * D + d] - mu[d] : 0.f;
    }
    __syncthreads();
    for (int r = 0; r < DISP_ROWS; ++r) {
      float a[T], b[T];
#pragma unroll
      for (int u = 0; u < T; ++u) { a[u] = xs[r * DP + ti * T + u]; b[u] = xs[r * DP + tj * T + u]; }
#pragma unroll
      for (int u = 0; u < T; ++u)
#pragma unroll
        for (int v = 0; v < T; ++v) acc[u][v] = fmaf(a[u], b[v], acc[u][v]);
    }
    __syncthreads();
  }
  float* out = slabs + (size_t)blockIdx.x * D * D;
#pragma unroll
  for (int u = 0; u < T; ++u)
#pragma unroll
    for (int v = 0; v < T; ++v) {
      const int i = ti * T + u, j = tj * T + v;
      if (i < D && j < D) out[i * D + j] = acc[u][v];
    }
}

// the order of the floats as signed integers
__device__ __forceinline__ int32_t float_to_ordered(float f) {
  const int32_t i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float ordered_to_float(int32_t i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

__global__ void disp_minmax_init_kernel(int32_t* __restrict__ minmax) {
  minmax[0] = 0x7fffffff;
  minmax[1] = (int32_t)0x80000000;
}

// out[i][c] = (X[i] - mean) . axes[c], one row per thread; the block's min and max go to minmax with one atomic each
__global__ __launch_bounds__(DISP_THREADS) void disp_project_kernel(const float* __restrict__ X, int N, int D,
                                                                    const float* __restrict__ axes, const float* __restrict__ mean,
                                                                    float* __restrict__ out, int32_t* __restrict__ minmax) {
  __shared__ float ax[3 * DISP_MAX_D];
  __shared__ float mu[DISP_MAX_D];
  __shared__ int32_t lo_s, hi_s;
  const int tid = threadIdx.x;
  for (int e = tid; e < 3 * D; e += DISP_THREADS) ax[e] = axes[e];
  if (tid < D) mu[tid] = mean[tid];
  if (tid == 0) { lo_s = 0x7fffffff; hi_s = (int32_t)0x80000000; }
  __syncthreads();
  const int i = blockIdx.x * DISP_THREADS + tid;
  if (i < N) {
    const float* x = X + (size_t)i * D;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f;
    for (int d = 0; d < D; ++d) {
      const float c = x[d] - mu[d];
      p0 = fmaf(c, ax[d], p0);
      p1 = fmaf(c, ax[D + d], p1);
      p2 = fmaf(c, ax[2 * D + d], p2);
    }
    out[3 * (size_t)i] = p0;
    out[3 * (size_t)i + 1] = p1;
    out[3 * (size_t)i + 2] = p2;
    atomicMin(&lo_s, float_to_ordered(fminf(p0, fminf(p1, p2))));
    atomicMax(&hi_s, float_to_ordered(fmaxf(p0, fmaxf(p1, p2))));
  }
  __syncthreads();
  if (tid == 0) {
    atomicMin(&minmax[0], lo_s);
    atomicMax(&minmax[1], hi_s);
  }
}

// render.py:58: (v - min) / (max - min) with the single global min and max; max == min gives 0 / 0
__global__ __launch_bounds__(256) void disp_normalise_kernel(float* __restrict__ out, int n, const int32_t* __restrict__ minmax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float mn = ordered_to_float(minmax[0]), mx = ordered_to_float(minmax[1]);
  out[i] = (out[i] - mn) / (mx - mn);
}

}  // namespace trase

using namespace trase;

// one-array workspaces: the per-pixel winner of the splat, the per-block Gram slabs
static size_t splat_layout(void* ws, int32_t W, int32_t H, int32_t*& winner) { return array_layout(ws, (size_t)W * H, winner); }
static size_t gram_layout(void* ws, int32_t N, int32_t D, float*& slabs) { return array_layout(ws, (size_t)D * D * disp_blocks(N), slabs); }

extern "C" {

int trase_splat_sizes(int32_t N, int32_t W, int32_t H, size_t* ws_bytes) {
  if (!ws_bytes || N < 0 || W < 1 || H < 1 || (int64_t)W * H >= ((int64_t)1 << 31)) {
    set_error("trase_splat_sizes: need N >= 0, W, H >= 1, W * H < 2^31 (got N %d, W %d, H %d)", N, W, H);
    return TRASE_ERR_INVALID;
  }
  int32_t* winner;
  *ws_bytes = splat_layout(nullptr, W, H, winner);
  return TRASE_OK;
}

int trase_splat_points(const float* points, int32_t N, const uint8_t* mask, const double* full_proj, int32_t W, int32_t H,
                       const float* const* colors, int32_t L, int32_t white_background, float* const* images_out,
                       int64_t* index_out, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  if (N < 0 || W < 1 || H < 1 || (int64_t)W * H >= ((int64_t)1 << 31) || L < 0 || L > SPLAT_MAX_L) {
    set_error("trase_splat_points: need N >= 0, W, H >= 1, W * H < 2^31, 0 <= L <= %d (got N %d, W %d, H %d, L %d)", SPLAT_MAX_L,
              N, W, H, L);
    return TRASE_ERR_INVALID;
  }
  if (!full_proj || (N > 0 && !points) || (L > 0 && (!colors || !images_out))) { set_error("trase_splat_points: null pointer"); return TRASE_ERR_INVALID; }
  SplatLayers S{};
  for (int l = 0; l < L; ++l) {
    if (!images_out[l]) { set_error("trase_splat_points: null image"); return TRASE_ERR_INVALID; }
    S.colors[l] = colors[l];
    S.images[l] = images_out[l];
  }
  const int HW = W * H;
  int32_t* winner;
  if (!ws || ws_bytes < splat_layout(ws, W, H, winner)) { set_error("trase_splat_points: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  SplatProj P;
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 4; ++r) P.m[4 * c + r] = full_proj[4 * r + (c == 2 ? 3 : c)];
  TRASE_LAUNCH("splat_fill", stream, 0, splat_fill_kernel, dim3((HW + 255) / 256), dim3(256), 0, winner, HW);
  if (N > 0)
    TRASE_LAUNCH("splat_project", stream, 0, splat_project_kernel, dim3((N + 255) / 256), dim3(256), 0, points, N, mask, P, W, H, winner);
  if (L > 0 || index_out)
    TRASE_LAUNCH("splat_resolve", stream, 0, splat_resolve_kernel, dim3(((HW + 3) / 4 + 255) / 256), dim3(256), 0, winner, HW, L, S,
                 white_background ? 0.f : 1.f, white_background ? 1.f : 0.f, index_out);
  return TRASE_OK;
}

int trase_feature_gram_sizes(int32_t N, int32_t D, size_t* ws_bytes) {
  if (!ws_bytes || N < 2 || D < 1 || D > DISP_MAX_D) {
    set_error("trase_feature_gram_sizes: need N >= 2, 1 <= D <= %d (got N %d, D %d)", DISP_MAX_D, N, D);
    return TRASE_ERR_INVALID;
  }
  float* slabs;
  *ws_bytes = gram_layout(nullptr, N, D, slabs);
  return TRASE_OK;
}

int trase_feature_gram(const float* X, int32_t N, int32_t D, float* gram_mean_out, void* ws, size_t ws_bytes, int32_t device,
                       trase_stream_t stream_) {
  if (N < 2 || D < 1 || D > DISP_MAX_D) {
    set_error("trase_feature_gram: need N >= 2, 1 <= D <= %d (got N %d, D %d)", DISP_MAX_D, N, D);
    return TRASE_ERR_INVALID;
  }
  if (!X || !gram_mean_out) { set_error("trase_feature_gram: null pointer"); return TRASE_ERR_INVALID; }
  float* slabs;
  if (!ws || ws_bytes < gram_layout(ws, N, D, slabs)) { set_error("trase_feature_gram: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const int G = disp_blocks(N), chunk = (N + G - 1) / G, dp = disp_dpad(D);
  float* gram = gram_mean_out;
  float* mean = gram_mean_out + (size_t)D * D;
#define TRASE_DISP_DP(KERNEL, ...)                                                                                  \
  do {                                                                                                              \
    if (dp == 16) hipLaunchKernelGGL((KERNEL<16>), dim3(G), dim3(DISP_THREADS), 0, stream, __VA_ARGS__);            \
    else if (dp == 32) hipLaunchKernelGGL((KERNEL<32>), dim3(G), dim3(DISP_THREADS), 0, stream, __VA_ARGS__);       \
    else hipLaunchKernelGGL((KERNEL<64>), dim3(G), dim3(DISP_THREADS), 0, stream, __VA_ARGS__);                     \
  } while (0)
  TRASE_LAUNCHES("feature_colsum", stream, 0, TRASE_DISP_DP(disp_colsum_kernel, X, N, D, chunk, slabs));
  TRASE_LAUNCH("feature_mean", stream, 0, disp_reduce_kernel, dim3((D + 255) / 256), dim3(256), 0, slabs, G, D, 1.0 / (double)N, mean);
  TRASE_LAUNCHES("feature_gram", stream, 0, TRASE_DISP_DP(disp_gram_kernel, X, N, D, chunk, mean, slabs));
#undef TRASE_DISP_DP
  TRASE_LAUNCH("feature_gram_reduce", stream, 0, disp_reduce_kernel, dim3((D * D + 255) / 256), dim3(256), 0, slabs, G, D * D, 1.0, gram);
  return TRASE_OK;
}

int trase_feature_project(const float* X, int32_t N, int32_t D, const float* axes, const float* mean, float* colors_out,
                          int32_t* minmax, int32_t device, trase_stream_t stream_) {
  if (N < 1 || D < 1 || D > DISP_MAX_D || (int64_t)N * 3 >= ((int64_t)1 << 31)) {
    set_error("trase_feature_project: need 1 <= N < 2^31 / 3, 1 <= D <= %d (got N %d, D %d)", DISP_MAX_D, N, D);
    return TRASE_ERR_INVALID;
  }
  if (!X || !axes || !mean || !colors_out || !minmax) { set_error("trase_feature_project: null pointer"); return TRASE_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCH("feature_minmax_init", stream, 0, disp_minmax_init_kernel, dim3(1), dim3(1), 0, minmax);
  TRASE_LAUNCH("feature_project", stream, 0, disp_project_kernel, dim3((N + DISP_THREADS - 1) / DISP_THREADS), dim3(DISP_THREADS), 0, X, N, D,
               axes, mean, colors_out, minmax);
  TRASE_LAUNCH("feature_normalise", stream, 0, disp_normalise_kernel, dim3((3 * N + 255) / 256), dim3(256), 0, colors_out, 3 * N, minmax);
  return TRASE_OK;
}

}  // extern "C"
