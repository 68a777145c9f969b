// trajectory.hip -- the viewer's trajectory view and the end of its frame loop.
//   utils/time_utils.py:375-396 farthest_point_sample (gui.py:1158-1166, gui_standalone.py:1596-1604)
//   gui.py:1169-1191 update_trajectory_overlay: the projected polylines of the tracked Gaussians (gui_standalone.py:1605-1629)
//   gui.py:1080-1122: depth normalisation, bilinear resize, HWC / clamp, the three host blends
//
// Sampler: npoint ordinary launches back to back on the caller's stream, no cooperative launch, no grid-wide barrier and no
// host read between the steps -- the order of the launches on the stream is the only synchronisation.  Launch i has G <=
// TRASE_FPS_MAX_BLOCKS workgroups, each owning a contiguous slice of the rows:
//   1. every workgroup reduces the G keys the previous launch left (launch 0: takes the start row) to the winner, sample i,
//      and workgroup 0 stores it to out[i];
//   2. it lowers its slice of the running minimum distances against that point, d = (dx*dx + dy*dy) + dz*dz with every
//      product and sum rounded to fp32 (no FMA contraction: bit for bit what numpy float32 gives), update on strict <;
//   3. it writes the largest key of its slice, (distance bits << 32) | ~row, with a plain 64-bit store into the other half of
//      the two-half `partial` buffer.  Distances are non-negative floats, so their bits order as integers; among equal
//      distances the larger ~row, the LOWEST row, wins.  A masked row has key 0, below every candidate's.
// The last launch is one workgroup that only reduces and stores out[npoint - 1].
//
// Overlay, three launches like the splat of display.hip: fill the int32 winner map with -1; one WAVE per segment projects
// both end points in float64, truncates to integer pixels and lets its lanes stride over the in-image part of the major axis
// with atomicMax(winner, trajectory index); resolve the winner map to the (H, W, 4) overlay.  Integer atomics only.
//
// Present: one thread per output pixel does the resize (ATen's align_corners = False arithmetic), the clamp and the blends,
// every blend product and sum rounded on its own as the separate torch / numpy operations of the reference round them.
//
// This file is compiled with -ffp-contract=off (Makefile): HIP defines __fmul_rn / __fadd_rn / __fsub_rn as the plain
// operators, so they alone would not keep the compiler from fusing a product into the following sum.
#include "common.h"

namespace trase {

constexpr int FPS_THREADS = 256;
constexpr int FPS_WAVES = FPS_THREADS / WAVE;
constexpr int FPS_MAX_BLOCKS = TRASE_FPS_MAX_BLOCKS;
static_assert(FPS_MAX_BLOCKS <= FPS_THREADS, "one thread per key of the previous launch");
constexpr int TRAJ_THREADS = 256;
constexpr int TRAJ_WAVES = TRAJ_THREADS / WAVE;
constexpr double TRAJ_COORD_LIMIT = 1048576.0;       // 2^20: a sample at or beyond it breaks its polyline

static inline int fps_blocks(int N) {
  const int g = (N + FPS_THREADS - 1) / FPS_THREADS;
  return g < 1 ? 1 : g > FPS_MAX_BLOCKS ? FPS_MAX_BLOCKS : g;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d, WAVE);
    v = o > v ? o : v;
  }
  return v;                                            // every lane holds the maximum
}
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* slots) {
  v = wave_max_u64(v);
  if ((threadIdx.x & (WAVE - 1)) == 0) slots[threadIdx.x / WAVE] = v;
  __syncthreads();
  unsigned long long m = slots[0];
#pragma unroll
  for (int w = 1; w < FPS_WAVES; ++w) m = slots[w] > m ? slots[w] : m;
  __syncthreads();                                     // the slots are used again
  return m;
}

// prev: the n_prev keys of the previous launch, or null in launch 0 (the winner is then *start_dev, or start).
// next: this launch's keys, one per workgroup, or null in the last launch (nothing is updated then).
__global__ __launch_bounds__(FPS_THREADS) void fps_step_kernel(const float* __restrict__ points, int N, const uint8_t* __restrict__ mask,
                                                               float* __restrict__ dist, const unsigned long long* __restrict__ prev,
                                                               int n_prev, unsigned long long* __restrict__ next, int chunk,
                                                               int start, const int64_t* __restrict__ start_dev,
                                                               int64_t* __restrict__ out_i) {
  __shared__ unsigned long long slots[FPS_WAVES];
  const int tid = threadIdx.x;
  uint32_t win;
  if (prev) {
    const unsigned long long k = block_max_u64(tid < n_prev ? prev[tid] : 0ull, slots);
    win = ~(uint32_t)k;
  } else {
    win = start_dev ? (uint32_t)*start_dev : (uint32_t)start;
  }
  if (win >= (uint32_t)N) win = 0;                     // never taken with a candidate in the cloud: no read outside `points`
  if (blockIdx.x == 0 && tid == 0) *out_i = (int64_t)win;
  if (!next) return;

  const float cx = points[3 * (size_t)win], cy = points[3 * (size_t)win + 1], cz = points[3 * (size_t)win + 2];
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < (int64_t)N ? lo + chunk : (int64_t)N;
  unsigned long long best = 0ull;
  for (int64_t r = lo + tid; r < hi; r += FPS_THREADS) {
    if (mask && !mask[r]) continue;
    const float dx = __fsub_rn(points[3 * r], cx), dy = __fsub_rn(points[3 * r + 1], cy), dz = __fsub_rn(points[3 * r + 2], cz);
    const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    float m = prev ? dist[r] : 1e10f;
    if (d < m) m = d;                                  // a NaN distance leaves the minimum as it is
    dist[r] = m;
    const unsigned long long key = ((unsigned long long)__float_as_uint(m) << 32) | (uint32_t)~(uint32_t)r;
    best = key > best ? key : best;
  }
  best = block_max_u64(best, slots);
  if (tid == 0) next[blockIdx.x] = best;
}

// ---- trajectory ring and overlay ---------------------------------------------------------------------------------------------

// slot[g] = points[rows[g]]; a row outside [0, N) gives NaN, which breaks the polyline there
__global__ __launch_bounds__(256) void traj_append_kernel(const float* __restrict__ points, int N, const int64_t* __restrict__ rows,
                                                          int G, float* __restrict__ slot) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int64_t r = rows[g];
  const bool ok = r >= 0 && r < (int64_t)N;
#pragma unroll
  for (int c = 0; c < 3; ++c) slot[3 * (size_t)g + c] = ok ? points[3 * (size_t)r + c] : __uint_as_float(0x7fc00000u);
}

struct TrajProj { double m[12]; };            // columns 0, 1 and 3 of full_proj_transform: m[4 * c + r]

// integer pixel of a sample, truncated toward zero as astype(int32) does; false if a coordinate is non-finite or >= 2^20
__device__ __forceinline__ bool traj_pixel(const float* __restrict__ p, const TrajProj& P, int W, int H, long long& ix, long long& iy) {
  const double x = p[0], y = p[1], z = p[2];
  const double px_h = x * P.m[0] + y * P.m[1] + z * P.m[2] + P.m[3];
  const double py_h = x * P.m[4] + y * P.m[5] + z * P.m[6] + P.m[7];
  const double w = x * P.m[8] + y * P.m[9] + z * P.m[10] + P.m[11];
  const double px = (px_h / w + 1.0) / 2.0 * (double)W;
  const double py = (py_h / w + 1.0) / 2.0 * (double)H;
  if (!(fabs(px) < TRAJ_COORD_LIMIT && fabs(py) < TRAJ_COORD_LIMIT)) return false;      // a NaN fails the comparison
  ix = (long long)px;
  iy = (long long)py;
  return true;
}

// One wave per segment (trajectory g, samples s and s + 1); with S == 1 the one sample is a segment of its own.  Sample s is
// row (first + s) % cap of `coords`.
__global__ __launch_bounds__(TRAJ_THREADS) void traj_draw_kernel(const float* __restrict__ coords, int S, int G, int first, int cap,
                                                                 TrajProj P, int W, int H, int32_t* __restrict__ winner) {
  const int segs = S > 1 ? S - 1 : 1;
  const int seg = blockIdx.x * TRAJ_WAVES + threadIdx.x / WAVE;
  if (seg >= G * segs) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const int g = seg / segs, s = seg - g * segs;
  const int sa = (first + s) % cap, sb = S > 1 ? (first + s + 1) % cap : sa;
  long long ax, ay, bx, by;
  if (!traj_pixel(coords + 3 * ((size_t)sa * G + g), P, W, H, ax, ay)) return;
  if (!traj_pixel(coords + 3 * ((size_t)sb * G + g), P, W, H, bx, by)) return;
  const long long dx = bx > ax ? bx - ax : ax - bx, dy = by > ay ? by - ay : ay - by;
  // (u, v) = (major, minor) axis
  const bool xmaj = dx >= dy;
  const long long au = xmaj ? ax : ay, av = xmaj ? ay : ax, bu = xmaj ? bx : by, bv = xmaj ? by : bx;
  const long long du = xmaj ? dx : dy, dv = xmaj ? dy : dx;
  const long long nu = xmaj ? W : H, nv = xmaj ? H : W;
  const long long sv = bv > av ? 1 : -1;
  long long u0 = au < bu ? au : bu, u1 = au < bu ? bu : au;
  if (u0 < 0) u0 = 0;
  if (u1 > nu - 1) u1 = nu - 1;
  for (long long u = u0 + lane; u <= u1; u += WAVE) {
    const long long t = u > au ? u - au : au - u;
    const long long v = du == 0 ? av : av + sv * ((2 * t * dv + du) / (2 * du));        // operands >= 0: the division floors
    if (v < 0 || v >= nv) continue;
    const long long x = xmaj ? u : v, y = xmaj ? v : u;
    atomicMax(&winner[(size_t)y * W + x], g);
  }
}

__global__ __launch_bounds__(256) void traj_fill_kernel(int32_t* __restrict__ winner, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) winner[i] = -1;
}

// overlay[p] = (colour of the winner, 1), or zeros where no line passes
__global__ __launch_bounds__(256) void traj_resolve_kernel(const int32_t* __restrict__ winner, int HW, const float* __restrict__ colors,
                                                           float* __restrict__ overlay, int vec_ok) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= HW) return;
  const int w = winner[p];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (w >= 0) v = make_float4(colors[3 * (size_t)w], colors[3 * (size_t)w + 1], colors[3 * (size_t)w + 2], 1.f);
  float* o = overlay + 4 * (size_t)p;
  if (vec_ok) {
    *reinterpret_cast<float4*>(o) = v;
  } else {
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
}

// ---- present -----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int32_t present_ordered(float f) {
  const int32_t i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float present_unordered(int32_t i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

__global__ void present_minmax_init_kernel(int32_t* __restrict__ minmax) {
  minmax[0] = 0x7fffffff;
  minmax[1] = (int32_t)0x80000000;
}

// global min and max of n floats: registers, then LDS, then one atomic pair per workgroup (a NaN takes no part)
__global__ __launch_bounds__(256) void present_minmax_kernel(const float* __restrict__ v, int n, int32_t* __restrict__ minmax) {
  __shared__ int32_t lo_s, hi_s;
  if (threadIdx.x == 0) { lo_s = 0x7fffffff; hi_s = (int32_t)0x80000000; }
  __syncthreads();
  float lo = __int_as_float(0x7f800000), hi = __int_as_float(0xff800000);
  bool any = false;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float x = v[i];
    if (x == x) { lo = fminf(lo, x); hi = fmaxf(hi, x); any = true; }
  }
  if (any) {
    atomicMin(&lo_s, present_ordered(lo));
    atomicMax(&hi_s, present_ordered(hi));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicMin(&minmax[0], lo_s);
    atomicMax(&minmax[1], hi_s);
  }
}

struct PresentArgs {
  const float* image;            // (C, h, w), C = 3, or 1 in depth mode
  int h, w, H, W;
  int depth;
  const int32_t* minmax;
  const float* control;          // (H, W, 3) or null
  const float* overlay;          // (H, W, 4) or null
  const float* tint;             // (H, W, 3) or null
  float tint_weight;
  float scale_h, scale_w;        // float(in) / out
  float* out;                    // (H, W, 3)
};

__global__ __launch_bounds__(256) void present_kernel(PresentArgs a) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.H * a.W) return;
  const int y = p / a.W, x = p - y * a.W;
  const bool same = a.H == a.h && a.W == a.w;          // ATen copies in this case
  int y0 = y, y1 = y, x0 = x, x1 = x;
  float hl0 = 1.f, hl1 = 0.f, wl0 = 1.f, wl1 = 0.f;
  if (!same) {
    bilinear_source(a.scale_h, y, a.h, y0, y1, hl0, hl1);
    bilinear_source(a.scale_w, x, a.w, x0, x1, wl0, wl1);
  }
  float mn = 0.f, den = 1.f;
  if (a.depth) {
    mn = present_unordered(a.minmax[0]);
    den = __fadd_rn(__fsub_rn(present_unordered(a.minmax[1]), mn), 1e-20f);
  }
  const size_t hw = (size_t)a.h * a.w;
  float b[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (a.depth && c > 0) { b[c] = b[0]; continue; }
    const float* pl = a.image + (a.depth ? 0 : c * hw);
    float v00 = pl[(size_t)y0 * a.w + x0];
    if (a.depth) v00 = __fsub_rn(v00, mn) / den;
    float v = v00;
    if (!same) {
      float v01 = pl[(size_t)y0 * a.w + x1], v10 = pl[(size_t)y1 * a.w + x0], v11 = pl[(size_t)y1 * a.w + x1];
      if (a.depth) { v01 = __fsub_rn(v01, mn) / den; v10 = __fsub_rn(v10, mn) / den; v11 = __fsub_rn(v11, mn) / den; }
      {
#pragma clang fp contract(fast)                        // as ATen's kernel is compiled; the rest of the file is contract(off)
        v = hl0 * (wl0 * v00 + wl1 * v01) + hl1 * (wl0 * v10 + wl1 * v11);
      }
    }
    b[c] = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);        // clamp(0, 1); a NaN stays a NaN as in torch
  }
  if (a.control) {
    const float* o = a.control + 3 * (size_t)p;
    const float o0 = o[0], o1 = o[1], o2 = o[2];
    const float m = __fadd_rn(__fadd_rn(o0, o1), o2) == 0.f ? 1.f : 0.f;
    b[0] = __fadd_rn(__fmul_rn(b[0], m), o0);
    b[1] = __fadd_rn(__fmul_rn(b[1], m), o1);
    b[2] = __fadd_rn(__fmul_rn(b[2], m), o2);
  }
  if (a.overlay) {
    const float* o = a.overlay + 4 * (size_t)p;
    const float al = o[3], ia = __fsub_rn(1.f, al);
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = __fadd_rn(__fmul_rn(b[c], ia), __fmul_rn(o[c], al));
  }
  if (a.tint) {
    const float* t = a.tint + 3 * (size_t)p;
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = __fadd_rn(b[c], __fmul_rn(a.tint_weight, t[c]));
  }
  float* out = a.out + 3 * (size_t)p;
  out[0] = b[0]; out[1] = b[1]; out[2] = b[2];
}

static void load_proj(const double* full_proj, TrajProj& P) {
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 4; ++r) P.m[4 * c + r] = full_proj[4 * r + (c == 2 ? 3 : c)];
}

}  // namespace trase

using namespace trase;

extern "C" {

int trase_fps_sample(const float* points, int32_t N, const uint8_t* mask, int32_t start, const int64_t* start_dev, int32_t npoint,
                     int64_t* out, float* dist, uint64_t* partial, int32_t device, trase_stream_t stream_) {
  if (N < 1 || npoint < 1 || npoint > TRASE_FPS_MAX_SAMPLES || (!start_dev && (start < 0 || start >= N))) {
    set_error("trase_fps_sample: need 1 <= N < 2^31, 1 <= npoint <= %d, 0 <= start < N (got N %d, npoint %d, start %d)",
              TRASE_FPS_MAX_SAMPLES, N, npoint, start);
    return TRASE_ERR_INVALID;
  }
  if (!points || !out || !dist || !partial) { set_error("trase_fps_sample: null pointer"); return TRASE_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const int G = fps_blocks(N), chunk = (int)(((int64_t)N + G - 1) / G);
  unsigned long long* half[2] = {(unsigned long long*)partial, (unsigned long long*)partial + FPS_MAX_BLOCKS};
  TRASE_LAUNCHES("fps_sample", stream, 0,
    for (int i = 0; i < npoint; ++i) {
      const bool last = i == npoint - 1;
      hipLaunchKernelGGL(fps_step_kernel, dim3(last ? 1 : G), dim3(FPS_THREADS), 0, stream, points, N, mask, dist,
                         i ? half[(i - 1) & 1] : nullptr, G, last ? nullptr : half[i & 1], chunk, start, i ? nullptr : start_dev,
                         out + i);
    });
  return TRASE_OK;
}

int trase_trajectory_append(const float* points, int32_t N, const int64_t* rows, int32_t G, float* slot_out, int32_t device,
                            trase_stream_t stream_) {
  if (N < 0 || G < 1 || G > TRASE_TRAJ_MAX_TRACKS) {
    set_error("trase_trajectory_append: need N >= 0, 1 <= G <= %d (got N %d, G %d)", TRASE_TRAJ_MAX_TRACKS, N, G);
    return TRASE_ERR_INVALID;
  }
  if ((N > 0 && !points) || !rows || !slot_out) { set_error("trase_trajectory_append: null pointer"); return TRASE_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCH("trajectory_append", stream, 0, traj_append_kernel, dim3((G + 255) / 256), dim3(256), 0, points, N, rows, G, slot_out);
  return TRASE_OK;
}

int trase_trajectory_draw(const float* coords, int32_t S, int32_t G, int32_t first, int32_t cap, const double* full_proj, int32_t W,
                          int32_t H, const float* colors, float* overlay_out, int32_t* winner, int32_t device,
                          trase_stream_t stream_) {
  if (S < 0 || S > TRASE_TRAJ_MAX_SAMPLES || G < 1 || G > TRASE_TRAJ_MAX_TRACKS || cap < 1 || cap > TRASE_TRAJ_MAX_SAMPLES || S > cap ||
      first < 0 || first >= cap || W < 1 || H < 1 || (int64_t)W * H >= ((int64_t)1 << 31)) {
    set_error("trase_trajectory_draw: need 0 <= S <= cap <= %d, 1 <= G <= %d, 0 <= first < cap, W, H >= 1, W * H < 2^31 "
              "(got S %d, G %d, first %d, cap %d, W %d, H %d)", TRASE_TRAJ_MAX_SAMPLES, TRASE_TRAJ_MAX_TRACKS, S, G, first, cap, W, H);
    return TRASE_ERR_INVALID;
  }
  if (!full_proj || !winner || (S > 0 && !coords) || (overlay_out && !colors)) {
    set_error("trase_trajectory_draw: null pointer");
    return TRASE_ERR_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TrajProj P;
  load_proj(full_proj, P);
  const int HW = W * H;
  TRASE_LAUNCH("trajectory_fill", stream, 0, traj_fill_kernel, dim3((HW + 255) / 256), dim3(256), 0, winner, HW);
  if (S > 0) {
    const int segs = G * (S > 1 ? S - 1 : 1);          // <= 2^16 * 2^10
    TRASE_LAUNCH("trajectory_draw", stream, 0, traj_draw_kernel, dim3((segs + TRAJ_WAVES - 1) / TRAJ_WAVES), dim3(TRAJ_THREADS), 0, coords, S, G,
                 first, cap, P, W, H, winner);
  }
  if (overlay_out)
    TRASE_LAUNCH("trajectory_resolve", stream, 0, traj_resolve_kernel, dim3((HW + 255) / 256), dim3(256), 0, winner, HW, colors, overlay_out,
                 (int)((reinterpret_cast<uintptr_t>(overlay_out) & 15) == 0));
  return TRASE_OK;
}

int trase_present_frame(const float* image, int32_t h, int32_t w, int32_t depth, int32_t H, int32_t W, const float* control_overlay,
                        const float* overlay, const float* tint, float tint_weight, float* out, int32_t* minmax, int32_t device,
                        trase_stream_t stream_) {
  if (h < 1 || w < 1 || H < 1 || W < 1 || (int64_t)h * w >= ((int64_t)1 << 31) || (int64_t)H * W >= ((int64_t)1 << 31)) {
    set_error("trase_present_frame: need h, w, H, W >= 1, h * w < 2^31, H * W < 2^31 (got %d x %d -> %d x %d)", h, w, H, W);
    return TRASE_ERR_INVALID;
  }
  if (!image || !out || (depth && !minmax)) { set_error("trase_present_frame: null pointer"); return TRASE_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  if (depth) {
    const int n = h * w;
    int blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    TRASE_LAUNCHES("present_minmax", stream, 0,
      hipLaunchKernelGGL(present_minmax_init_kernel, dim3(1), dim3(1), 0, stream, minmax);
      hipLaunchKernelGGL(present_minmax_kernel, dim3(blocks), dim3(256), 0, stream, image, n, minmax));
  }
  PresentArgs a;
  a.image = image; a.h = h; a.w = w; a.H = H; a.W = W; a.depth = depth ? 1 : 0; a.minmax = minmax;
  a.control = control_overlay; a.overlay = overlay; a.tint = tint; a.tint_weight = tint_weight;
  a.scale_h = (float)h / (float)H; a.scale_w = (float)w / (float)W;
  a.out = out;
  TRASE_LAUNCH("present_frame", stream, 0, present_kernel, dim3((H * W + 255) / 256), dim3(256), 0, a);
  return TRASE_OK;
}

}  // extern "C"
