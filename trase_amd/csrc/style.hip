// style.hip -- the rest of utils/loss_utils.py (trase_amd/losses.py): the image-space losses masked_l1_loss, weighted_l1_loss and
// l2_loss (:33-44) and the feature statistics of the style-transfer path: calc_mean_std (:230-238), gram_matrix (:240-249),
// cal_adain_style_loss (:251-262), cal_style_loss (:264-269), cal_mse_content_loss (:271-272).
// No float atomics anywhere: every sum has one fixed order, two calls give the same bits.  This unit is compiled with
// -ffp-contract=off: every fp32 operation below is rounded on its own; a fused product is written fmaf.
//   pixel_fwd_kernel / pixel_finish_kernel : terms in fp32 (subtract, abs, multiply), summed in float64 per workgroup (at most
//                            PX_WG_MAX workgroups over contiguous ranges), the workgroup sums added in workgroup order by one
//                            thread and rounded once
//   pixel_bwd_kernel       : one elementwise pass; s = g * float(1 / denominator), masked / weighted: sign(x - gt) * (m * s) with
//                            sign(0) = 0, l2: (2 s) * (x - gt)
//   stats_sum / stats_m2 / stats_finish : per-channel mean and unbiased std in TWO PASSES in float64 (the sum, then the squared
//                            deviations from the float64 mean), each pass split into at most ST_SLICES slices per channel
//   gram_kernel            : G = X X^T on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation in k order).  A workgroup of
//                            four waves owns a 128 x 128 tile of G on or above the diagonal and one slice of n; tiles of X go
//                            through LDS GR_KT columns at a time; the operand of lane l is X[c0 + (l & 31)][k0 + (l >> 5)] on both
//                            sides.  n is cut into chains of GR_CHAIN columns: a chain is accumulated in fp32 by the MFMA, chain
//                            results are added in float64 in chain order (in registers inside a slice, by gram_combine_kernel
//                            across slices) and rounded once.  Only 32 x 32 blocks on or above the diagonal are computed; the
//                            combine writes G[i][j] and G[j][i] from the same value.
//   style_gram_diff_kernel : D = coef * (G - S) for the backward and the float64 sum of (G - S)^2 per workgroup
//   style_reduce_kernel    : the three weighted terms and their sum in float64 on the device (workgroup sums in workgroup order),
//                            and the AdaIN coefficients a[i], b[i] for the backward
//   style_grad_kernel      : d x[i][k] = g * (2 * sum_j D[i][j] x[j][k] + a[i] + b[i] x[i][k] + c (x[i][k] - y[i][k])) in one
//                            GEMM-shaped launch on the same MFMA (K = C); a term that is switched off is skipped
#include "common.h"

namespace trase {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- image-space losses -----------------------------------------------------------------------------------------------------
constexpr int PX_WG_MAX = 512;            // workgroups of the forward: the length of the serial float64 combination
constexpr int PX_WG_MIN_ELEMS = 1024;     // below this many elements a workgroup is not worth starting

static inline int px_blocks(int64_t n) { return (int)((n + PX_WG_MIN_ELEMS - 1) / PX_WG_MIN_ELEMS < PX_WG_MAX ? (n + PX_WG_MIN_ELEMS - 1) / PX_WG_MIN_ELEMS : PX_WG_MAX); }
static inline int64_t px_per_block(int64_t n, int nb) { return ((n + nb - 1) / nb + 255) / 256 * 256; }

struct PxArgs {
  const float* x;
  const void* gt;        // fp32 (C,H,W), or the planes of a ByteFrame when pitch > 0
  const void* aux;       // mask / weight
  int pitch, aux_kind, kind;
  uint32_t n, HW, W, H;
};

template <bool BYTES>
__device__ __forceinline__ float px_gt(const PxArgs& a, uint32_t i) {
  if (!BYTES) return ((const float*)a.gt)[i];
  const uint32_t c = i / a.HW, p = i - c * a.HW, y = p / a.W, xx = p - y * a.W;
  return (float)((const uint8_t*)a.gt)[((size_t)c * a.H + y) * a.pitch + xx] / 255.0f;     // the exact division, as GtBytes
}
__device__ __forceinline__ float px_aux(const PxArgs& a, uint32_t i) {
  if (a.aux_kind == TRASE_PIXEL_AUX_F32_FULL) return ((const float*)a.aux)[i];
  const uint32_t p = i % a.HW;
  return a.aux_kind == TRASE_PIXEL_AUX_U8 ? (float)((const uint8_t*)a.aux)[p] : ((const float*)a.aux)[p];
}

__device__ __forceinline__ double block_sum_f64(double v, double* s_red) {      // 256 threads; the total in every thread
  s_red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o];
    __syncthreads();
  }
  const double r = s_red[0];
  __syncthreads();
  return r;
}

template <bool BYTES>
__global__ __launch_bounds__(256) void pixel_fwd_kernel(PxArgs a, uint32_t per, double* __restrict__ part) {
  __shared__ double s_red[256];
  const uint32_t lo = blockIdx.x * per, hi = min(a.n, lo + per);
  double acc = 0.0, accm = 0.0;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) {
    const float d = a.x[i] - px_gt<BYTES>(a, i);
    float term;
    if (a.kind == TRASE_PIXEL_L2) term = d * d;
    else {
      const float m = px_aux(a, i);
      term = fabsf(d) * m;
      accm += (double)m;
    }
    acc += (double)term;
  }
  acc = block_sum_f64(acc, s_red);
  accm = block_sum_f64(accm, s_red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = acc; part[2 * blockIdx.x + 1] = accm; }
}

// tot[0] = the sum of the terms, tot[1] = the denominator; out = their quotient (0 when the denominator is 0)
__global__ void pixel_finish_kernel(const double* __restrict__ part, int nb, int kind, int aux_kind, double n, double C,
                                    double* __restrict__ tot, float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double s = 0.0, m = 0.0;
  for (int k = 0; k < nb; ++k) { s += part[2 * k]; m += part[2 * k + 1]; }
  // masked: the mask is (H, W) and every pixel was visited once per channel: m = C * sum(mask) already
  const double den = kind == TRASE_PIXEL_MASKED_L1 ? m : n;
  (void)aux_kind; (void)C;
  tot[0] = s; tot[1] = den;
  out[0] = den != 0.0 ? (float)(s / den) : 0.f;
}

template <bool BYTES>
__global__ __launch_bounds__(256) void pixel_bwd_kernel(PxArgs a, const double* __restrict__ tot, const float* __restrict__ g,
                                                        float* __restrict__ d_x) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const double den = tot[1];
  const float inv = den != 0.0 ? (float)(1.0 / den) : 0.f;
  const float s = g[0] * inv;
  const float d = a.x[i] - px_gt<BYTES>(a, i);
  float r;
  if (a.kind == TRASE_PIXEL_L2) r = (2.0f * s) * d;
  else {
    const float ms = px_aux(a, i) * s;
    r = d > 0.f ? ms : (d < 0.f ? -ms : 0.f);
  }
  d_x[i] = r;
}

// ---- per-channel statistics ---------------------------------------------------------------------------------------------------
constexpr int ST_SLICES = 64, ST_SLICE_MIN = 4096;
static inline int st_slices(int64_t n) { const int64_t s = (n + ST_SLICE_MIN - 1) / ST_SLICE_MIN; return (int)(s < ST_SLICES ? s : ST_SLICES); }

// grid (slices, C).  M2 == false: psum[c][s] = sum of the slice; true: pm2[c][s] = sum of (x - mean)^2, mean from psum in slice order
template <bool M2>
__global__ __launch_bounds__(256) void stats_pass_kernel(const float* __restrict__ x, uint32_t n, int SS, const double* __restrict__ psum,
                                                         double* __restrict__ outp) {
  __shared__ double s_red[256];
  const int c = blockIdx.y, s = blockIdx.x;
  const uint32_t per = (n + SS - 1) / SS, lo = s * per, hi = min(n, lo + per);
  double mean = 0.0;
  if (M2) {
    for (int k = 0; k < SS; ++k) mean += psum[c * SS + k];
    mean /= (double)n;
  }
  const float* row = x + (size_t)c * n;
  double acc = 0.0;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) {
    const double v = (double)row[i];
    if (M2) { const double d = v - mean; acc += d * d; }
    else acc += v;
  }
  acc = block_sum_f64(acc, s_red);
  if (threadIdx.x == 0) outp[c * SS + s] = acc;
}

__global__ void stats_finish_kernel(const double* __restrict__ psum, const double* __restrict__ pm2, int C, uint32_t n, int SS, float eps,
                                    float* __restrict__ mean, float* __restrict__ stdv, double* __restrict__ mean64, double* __restrict__ sd64) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, m2 = 0.0;
  for (int k = 0; k < SS; ++k) { s += psum[c * SS + k]; m2 += pm2[c * SS + k]; }
  const double mu = s / (double)n, sd = sqrt(m2 / (double)(n - 1));
  mean[c] = (float)mu;
  stdv[c] = (float)sd + eps;
  mean64[c] = mu; sd64[c] = sd;
}

// ---- Gram matrix on the fp32 MFMA -----------------------------------------------------------------------------------------------
constexpr int GR_TILE = 128;              // rows of X per side of a workgroup's tile of G (four waves, 64 x 64 each)
constexpr int GR_KT = 32;                 // columns of X staged per step
constexpr int GR_CHAIN = 1024;            // columns accumulated in fp32 before the chain result is added in float64
constexpr int GR_SLICE_BUDGET = 400;      // tiles * slices: bounds the workspace (16384 float64 per tile and slice)
constexpr int GR_LD = GR_KT + 1;          // LDS row pitch (floats)

static inline int gr_tiles(int C) { const int t = (C + GR_TILE - 1) / GR_TILE; return t * (t + 1) / 2; }
static inline int gr_slice_cap(int C) { const int c = GR_SLICE_BUDGET / gr_tiles(C); return c < 1 ? 1 : c; }
struct GrPlan { int ntile, nchain, cps, S; };
static inline GrPlan gr_plan(int C, int64_t n) {
  GrPlan p;
  p.ntile = gr_tiles(C);
  p.nchain = (int)((n + GR_CHAIN - 1) / GR_CHAIN);
  const int cap = gr_slice_cap(C);
  const int s0 = p.nchain < cap ? p.nchain : cap;
  p.cps = (p.nchain + s0 - 1) / s0;                 // chains per slice
  p.S = (p.nchain + p.cps - 1) / p.cps;
  return p;
}

__device__ __forceinline__ void gr_tile_of(int t, int nt, int& ti, int& tj) {      // t-th tile on or above the diagonal, row-major
  ti = 0;
  while (t >= nt - ti) { t -= nt - ti; ++ti; }
  tj = ti + t;
}
// 32 x 32 block (I, J) of G (block indices) is computed iff it lies on or above the diagonal and inside the matrix
__device__ __forceinline__ bool gr_block_on(int I, int J, int C) { return I <= J && J * 32 < C; }

// MULTI: a slice holds several chains and adds their results in float64 registers (128 more VGPRs: one wave per SIMD); with one
// chain per slice the fp32 accumulators are the slice's result
template <bool MULTI>
__global__ __launch_bounds__(256, MULTI ? 1 : 2) void gram_kernel(const float* __restrict__ X, int C, uint32_t n, int nt, int cps, int nchain,
                                                   double* __restrict__ part) {
  __shared__ float s_a[GR_TILE * GR_LD];
  __shared__ float s_b[GR_TILE * GR_LD];
  int ti, tj;
  gr_tile_of(blockIdx.x, nt, ti, tj);
  const bool diag = ti == tj;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 31, h = lane >> 5;
  const int wi = wave >> 1, wj = wave & 1;
  const int I0 = ti * 4 + wi * 2, J0 = tj * 4 + wj * 2;
  bool on[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) on[s] = gr_block_on(I0 + (s >> 1), J0 + (s & 1), C);
  const bool wave_on = on[0] || on[1] || on[2] || on[3];
  double acc64[MULTI ? 4 : 1][16];
  if (MULTI) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc64[MULTI ? s : 0][r] = 0.0;
  }
  // the accumulators as they lie in the registers: [slice][tile][wave][block][r][lane]
  double* out = part + ((((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave) * 4) * 1024 + lane;
  const float* sb = diag ? s_a : s_b;
  const int c_lo = blockIdx.y * cps, c_hi = min(nchain, c_lo + cps);
  for (int ch = c_lo; ch < c_hi; ++ch) {
    f32x16 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
    const uint32_t k_lo = (uint32_t)ch * GR_CHAIN, k_hi = min(n, k_lo + GR_CHAIN);
    for (uint32_t k0 = k_lo; k0 < k_hi; k0 += GR_KT) {
      // stage: rows of the two panels, GR_KT columns; beyond C or the chain's end: 0 (adds nothing to a sum)
#pragma unroll 4
      for (int e = 0; e < GR_TILE * GR_KT / 256; ++e) {
        const int idx = threadIdx.x + 256 * e, row = idx / GR_KT, kk = idx % GR_KT;
        const uint32_t k = k0 + kk;
        const int ra = ti * GR_TILE + row, rb = tj * GR_TILE + row;
        s_a[row * GR_LD + kk] = (ra < C && k < k_hi) ? X[(size_t)ra * n + k] : 0.f;
        if (!diag) s_b[row * GR_LD + kk] = (rb < C && k < k_hi) ? X[(size_t)rb * n + k] : 0.f;
      }
      __syncthreads();
      if (wave_on) {
        const float* pa = s_a + (wi * 64 + m) * GR_LD + h;
        const float* pb = sb + (wj * 64 + m) * GR_LD + h;
#pragma unroll
        for (int ks = 0; ks < GR_KT; ks += 2) {
          const float a0 = pa[ks], a1 = pa[32 * GR_LD + ks], b0 = pb[ks], b1 = pb[32 * GR_LD + ks];
          if (on[0]) acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0], 0, 0, 0);
          if (on[1]) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[1], 0, 0, 0);
          if (on[2]) acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[2], 0, 0, 0);
          if (on[3]) acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[3], 0, 0, 0);
        }
      }
      __syncthreads();
    }
    if (MULTI) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc64[MULTI ? s : 0][r] += (double)acc[s][r];
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (on[s])
#pragma unroll
          for (int r = 0; r < 16; ++r) out[s * 1024 + r * 64] = (double)acc[s][r];
    }
  }
  if (MULTI) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (on[s])
#pragma unroll
        for (int r = 0; r < 16; ++r) out[s * 1024 + r * 64] = acc64[MULTI ? s : 0][r];
  }
}

// one thread per accumulator element of every tile: the slices in order in float64, rounded once, written to both triangles
__global__ __launch_bounds__(256) void gram_combine_kernel(const double* __restrict__ part, int C, int nt, int ntile, int S, float* __restrict__ G) {
  const uint32_t gid = blockIdx.x * 256 + threadIdx.x;                   // < ntile * 16384
  const int lane = gid & 63, r = (gid >> 6) & 15, s = (gid >> 10) & 3, wave = (gid >> 12) & 3, t = gid >> 14;
  if (t >= ntile) return;
  int ti, tj;
  gr_tile_of(t, nt, ti, tj);
  const int I = ti * 4 + (wave >> 1) * 2 + (s >> 1), J = tj * 4 + (wave & 1) * 2 + (s & 1);
  if (!gr_block_on(I, J, C)) return;
  const int i = I * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3), j = J * 32 + (lane & 31);
  if (i >= C || j >= C || (I == J && i > j)) return;
  double v = 0.0;
  for (int sl = 0; sl < S; ++sl) v += part[(size_t)sl * ntile * 16384 + gid];
  const float gv = (float)v;
  G[(size_t)i * C + j] = gv;
  G[(size_t)j * C + i] = gv;
}

// ---- the node's reduction ---------------------------------------------------------------------------------------------------------
struct ReduceArgs {
  const float* G;                          // gram term (null: off)
  const double* gd_part;                   // the workgroup sums of style_gram_diff_kernel
  const float *mean, *stdv, *smean, *sstd; // AdaIN term (mean null: off)
  const double *mean64, *sd64;
  const double* px_part; int px_nb;        // content term: the workgroup sums of the l2 pass (null: off)
  double gram_w, adain_w, content_w;
  int C; double n;
  float *a, *b;                            // outputs for the backward
  float* out4;                             // total, gram, adain, content (each weighted)
};

// D = coef * (G - S) and the float64 sum of (G - S)^2 of each workgroup's 1024 elements
constexpr int GD_PER = 1024;
__global__ __launch_bounds__(256) void style_gram_diff_kernel(const float* __restrict__ G, const float* __restrict__ S, int CC, float coef,
                                                              float* __restrict__ D, double* __restrict__ part) {
  __shared__ double s_red[256];
  double acc = 0.0;
  for (int e = blockIdx.x * GD_PER + threadIdx.x; e < min(CC, (int)(blockIdx.x + 1) * GD_PER); e += 256) {
    const float g = G[e], s = S[e];
    const double d = (double)g - (double)s;
    acc += d * d;
    D[e] = coef * (g - s);
  }
  acc = block_sum_f64(acc, s_red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void style_reduce_kernel(ReduceArgs q) {
  __shared__ double s_red[256];
  const int C = q.C;
  double lg = 0.0, la = 0.0, lc = 0.0;
  if (q.G && threadIdx.x == 0) {
    double acc = 0.0;
    for (int k = 0; k < (C * C + GD_PER - 1) / GD_PER; ++k) acc += q.gd_part[k];       // workgroup order
    lg = acc * (q.gram_w / ((double)C * (double)C) / ((double)C * q.n));
  }
  if (q.mean) {
    double acc = 0.0;
    const double k = q.adain_w * 2.0 / (double)C;
    for (int c = threadIdx.x; c < C; c += 256) {
      const double dm = (double)q.mean[c] - (double)q.smean[c], ds = (double)q.stdv[c] - (double)q.sstd[c];
      acc += dm * dm + ds * ds;
      const double sd = q.sd64[c];
      const double bb = sd > 0.0 ? k * ds / ((q.n - 1.0) * sd) : 0.0;       // a channel of zero variance: no gradient from the std term
      q.b[c] = (float)bb;
      q.a[c] = (float)(k * dm / q.n - bb * q.mean64[c]);
    }
    la = block_sum_f64(acc, s_red) * q.adain_w / (double)C;
  }
  if (threadIdx.x == 0) {
    if (q.px_part) {
      double s = 0.0;
      for (int k = 0; k < q.px_nb; ++k) s += q.px_part[2 * k];
      lc = q.content_w * (s / ((double)C * q.n));
    }
    q.out4[0] = (float)(lg + la + lc);
    q.out4[1] = (float)lg; q.out4[2] = (float)la; q.out4[3] = (float)lc;
  }
}

// ---- the gradient: one GEMM-shaped launch ---------------------------------------------------------------------------------------------
constexpr int SG_KT = 32, SG_LDD = SG_KT + 1, SG_LDX = 160;

template <bool GEMM>
__global__ __launch_bounds__(256) void style_grad_kernel(const float* __restrict__ D, const float* __restrict__ a, const float* __restrict__ b, float c,
                                                         const float* __restrict__ x, const float* __restrict__ y, int C, uint32_t n,
                                                         const float* __restrict__ g, float* __restrict__ dx) {
  __shared__ float s_d[GEMM ? GR_TILE * SG_LDD : 1];
  __shared__ float s_x[GEMM ? SG_KT * SG_LDX : 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 31, h = lane >> 5;
  const int wi = wave >> 1, wj = wave & 1;
  const int i0 = blockIdx.y * GR_TILE;
  const uint32_t p0 = blockIdx.x * GR_TILE;
  bool on[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) on[s] = i0 + wi * 64 + (s >> 1) * 32 < C && p0 + wj * 64 + (s & 1) * 32 < n;
  f32x16 acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
  if (GEMM) {
    const bool wave_on = on[0] || on[1] || on[2] || on[3];
    for (int k0 = 0; k0 < C; k0 += SG_KT) {
#pragma unroll 4
      for (int e = 0; e < GR_TILE * SG_KT / 256; ++e) {
        const int idx = threadIdx.x + 256 * e;
        const int row = idx / SG_KT, kk = idx % SG_KT;               // D tile: [128 rows][32 k]
        s_d[row * SG_LDD + kk] = (i0 + row < C && k0 + kk < C) ? D[(size_t)(i0 + row) * C + k0 + kk] : 0.f;
        const int kr = idx / GR_TILE, col = idx % GR_TILE;           // x tile: [32 k][128 positions]
        s_x[kr * SG_LDX + col] = (k0 + kr < C && p0 + col < n) ? x[(size_t)(k0 + kr) * n + p0 + col] : 0.f;
      }
      __syncthreads();
      if (wave_on) {
        const float* pa = s_d + (wi * 64 + m) * SG_LDD + h;
        const float* pb = s_x + h * SG_LDX + wj * 64 + m;
#pragma unroll
        for (int ks = 0; ks < SG_KT; ks += 2) {
          const float a0 = pa[ks], a1 = pa[32 * SG_LDD + ks], b0 = pb[ks * SG_LDX], b1 = pb[ks * SG_LDX + 32];
          if (on[0]) acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0], 0, 0, 0);
          if (on[1]) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[1], 0, 0, 0);
          if (on[2]) acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[2], 0, 0, 0);
          if (on[3]) acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[3], 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }
  const float gs = g ? g[0] : 1.0f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (!on[s]) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + wi * 64 + (s >> 1) * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
      const uint32_t p = p0 + wj * 64 + (s & 1) * 32 + m;
      if (i >= C || p >= n) continue;
      const size_t o = (size_t)i * n + p;
      float v = GEMM ? 2.0f * acc[s][r] : 0.f;
      if (a) v = fmaf(b[i], x[o], v + a[i]);
      if (y) v = fmaf(c, x[o] - y[o], v);
      dx[o] = v * gs;
    }
  }
}

}  // namespace trase

using namespace trase;

namespace {

struct PxWs { double* part; double* tot; };
size_t px_layout(void* ws, PxWs& w) {
  WsCursor c(ws);
  w.part = c.take<double>(2 * PX_WG_MAX);
  w.tot = c.take<double>(2);
  return c.bytes();
}

struct StyleWs { double* gpart; double *psum, *pm2, *mean64, *sd64; float *G, *mean, *stdv; PxWs px; double* gd_part; };
size_t style_layout(void* ws, int C, int64_t n, StyleWs& w) {
  WsCursor c(ws);
  const GrPlan p = gr_plan(C, n);
  w.gpart = c.take<double>((size_t)p.ntile * p.S * 16384);
  const int SS = st_slices(n);
  w.psum = c.take<double>((size_t)C * SS);
  w.pm2 = c.take<double>((size_t)C * SS);
  w.mean64 = c.take<double>(C);
  w.sd64 = c.take<double>(C);
  w.G = c.take<float>((size_t)C * C);
  w.mean = c.take<float>(C);
  w.stdv = c.take<float>(C);
  w.px.part = c.take<double>(2 * PX_WG_MAX);
  w.px.tot = c.take<double>(2);
  w.gd_part = c.take<double>(((size_t)C * C + GD_PER - 1) / GD_PER);
  return c.bytes();
}

int px_check(const char* who, const void* x, const void* gt, int32_t pitch, int32_t C, int32_t H, int32_t W, int32_t kind, const void* aux,
             int32_t aux_kind) {
  if (!x || !gt) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  if (C < 1 || H < 1 || W < 1 || (int64_t)C * H * W >= ((int64_t)1 << 31)) { set_error("%s: need C, H, W >= 1 and C * H * W < 2^31 (got %d, %d, %d)", who, C, H, W); return TRASE_ERR_INVALID; }
  if (kind != TRASE_PIXEL_MASKED_L1 && kind != TRASE_PIXEL_WEIGHTED_L1 && kind != TRASE_PIXEL_L2) { set_error("%s: unknown kind %d", who, kind); return TRASE_ERR_INVALID; }
  if (pitch != 0 && (C != 3 || pitch < W || (pitch & 15) != 0 || ((size_t)gt & 15) != 0)) {
    set_error("%s: a byte frame needs C = 3, a pitch that is a multiple of 16 and at least W, and 16-byte aligned planes", who); return TRASE_ERR_INVALID;
  }
  if (kind == TRASE_PIXEL_L2) {
    if (aux || aux_kind != TRASE_PIXEL_AUX_NONE) { set_error("%s: l2 takes no mask or weight", who); return TRASE_ERR_INVALID; }
  } else {
    const bool ok = kind == TRASE_PIXEL_MASKED_L1 ? (aux_kind == TRASE_PIXEL_AUX_U8 || aux_kind == TRASE_PIXEL_AUX_F32)
                                                  : (aux_kind == TRASE_PIXEL_AUX_F32 || aux_kind == TRASE_PIXEL_AUX_F32_FULL);
    if (!aux || !ok) { set_error("%s: kind %d needs a mask / weight (aux_kind %d)", who, kind, aux_kind); return TRASE_ERR_INVALID; }
  }
  return TRASE_OK;
}

PxArgs px_args(const float* x, const void* gt, int32_t pitch, int32_t C, int32_t H, int32_t W, int32_t kind, const void* aux, int32_t aux_kind) {
  PxArgs a;
  a.x = x; a.gt = gt; a.aux = aux; a.pitch = pitch; a.aux_kind = aux_kind; a.kind = kind;
  a.n = (uint32_t)C * H * W; a.HW = (uint32_t)H * W; a.W = W; a.H = H;
  return a;
}

int px_forward_launch(const PxArgs& a, double* part, hipStream_t stream) {
  const int nb = px_blocks(a.n);
  const uint32_t per = (uint32_t)px_per_block(a.n, nb);
  TRASE_LAUNCHES("pixel_loss_fwd", stream, 0,
    if (a.pitch) hipLaunchKernelGGL(pixel_fwd_kernel<true>, dim3(nb), dim3(256), 0, stream, a, per, part);
    else hipLaunchKernelGGL(pixel_fwd_kernel<false>, dim3(nb), dim3(256), 0, stream, a, per, part));
  return TRASE_OK;
}

int style_check(const char* who, int32_t C, int64_t n, int64_t n_min) {
  if (C < 1 || C > 512 || n < n_min || n >= ((int64_t)1 << 31)) {
    set_error("%s: need 1 <= C <= 512 and %lld <= n < 2^31 (got C %d, n %lld)", who, (long long)n_min, C, (long long)n); return TRASE_ERR_INVALID;
  }
  return TRASE_OK;
}

int launch_gram(const float* x, int C, int64_t n, const StyleWs& w, float* G, hipStream_t stream) {
  const GrPlan p = gr_plan(C, n);
  const int nt = (C + GR_TILE - 1) / GR_TILE;
  TRASE_LAUNCHES("gram", stream, 0,
    if (p.cps > 1) hipLaunchKernelGGL(gram_kernel<true>, dim3(p.ntile, p.S), dim3(256), 0, stream, x, C, (uint32_t)n, nt, p.cps, p.nchain, w.gpart);
    else hipLaunchKernelGGL(gram_kernel<false>, dim3(p.ntile, p.S), dim3(256), 0, stream, x, C, (uint32_t)n, nt, p.cps, p.nchain, w.gpart));
  TRASE_LAUNCH("gram_combine", stream, 0, gram_combine_kernel, dim3(p.ntile * 64), dim3(256), 0, w.gpart, C, nt, p.ntile, p.S, G);
  return TRASE_OK;
}

int launch_stats(const float* x, int C, int64_t n, float eps, const StyleWs& w, float* mean, float* stdv, hipStream_t stream) {
  const int SS = st_slices(n);
  TRASE_LAUNCHES("mean_std", stream, 0,
    hipLaunchKernelGGL(stats_pass_kernel<false>, dim3(SS, C), dim3(256), 0, stream, x, (uint32_t)n, SS, (const double*)nullptr, w.psum);
    hipLaunchKernelGGL(stats_pass_kernel<true>, dim3(SS, C), dim3(256), 0, stream, x, (uint32_t)n, SS, (const double*)w.psum, w.pm2);
    hipLaunchKernelGGL(stats_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, (const double*)w.psum, (const double*)w.pm2, C,
                       (uint32_t)n, SS, eps, mean, stdv, w.mean64, w.sd64));
  return TRASE_OK;
}

}  // namespace

extern "C" {

int trase_pixel_loss_ws_bytes(size_t* ws_bytes) {
  if (!ws_bytes) { set_error("pixel_loss_ws_bytes: null pointer"); return TRASE_ERR_INVALID; }
  PxWs w;
  *ws_bytes = px_layout(nullptr, w);
  return TRASE_OK;
}

int trase_pixel_loss_forward(const float* x, const void* gt, int32_t gt_pitch, int32_t C, int32_t H, int32_t W, int32_t kind,
                             const void* aux, int32_t aux_kind, float* out, void* ws, size_t ws_bytes, int32_t device,
                             trase_stream_t stream_) {
  if (int rc = px_check("pixel_loss_forward", x, gt, gt_pitch, C, H, W, kind, aux, aux_kind)) return rc;
  if (!out || !ws) { set_error("pixel_loss_forward: null pointer"); return TRASE_ERR_INVALID; }
  PxWs w;
  if (ws_bytes < px_layout(ws, w)) { set_error("pixel_loss_forward: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const PxArgs a = px_args(x, gt, gt_pitch, C, H, W, kind, aux, aux_kind);
  if (int rc = px_forward_launch(a, w.part, stream)) return rc;
  TRASE_LAUNCH("pixel_loss_finish", stream, 0, pixel_finish_kernel, dim3(1), dim3(64), 0, (const double*)w.part, px_blocks(a.n), kind, aux_kind,
               (double)a.n, (double)C, w.tot, out);
  return TRASE_OK;
}

int trase_pixel_loss_backward(const float* x, const void* gt, int32_t gt_pitch, int32_t C, int32_t H, int32_t W, int32_t kind,
                              const void* aux, int32_t aux_kind, const float* g, const void* ws, size_t ws_bytes, float* d_x,
                              int32_t device, trase_stream_t stream_) {
  if (int rc = px_check("pixel_loss_backward", x, gt, gt_pitch, C, H, W, kind, aux, aux_kind)) return rc;
  if (!g || !d_x || !ws) { set_error("pixel_loss_backward: null pointer"); return TRASE_ERR_INVALID; }
  PxWs w;
  if (ws_bytes < px_layout(const_cast<void*>(ws), w)) { set_error("pixel_loss_backward: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const PxArgs a = px_args(x, gt, gt_pitch, C, H, W, kind, aux, aux_kind);
  const dim3 grid((a.n + 255) / 256);
  TRASE_LAUNCHES("pixel_loss_bwd", stream, 0,
    if (gt_pitch) hipLaunchKernelGGL(pixel_bwd_kernel<true>, grid, dim3(256), 0, stream, a, (const double*)w.tot, g, d_x);
    else hipLaunchKernelGGL(pixel_bwd_kernel<false>, grid, dim3(256), 0, stream, a, (const double*)w.tot, g, d_x));
  return TRASE_OK;
}

int trase_style_ws_bytes(int32_t C, int64_t n, size_t* ws_bytes) {
  if (int rc = style_check("style_ws_bytes", C, n, 1)) return rc;
  if (!ws_bytes) { set_error("style_ws_bytes: null pointer"); return TRASE_ERR_INVALID; }
  StyleWs w;
  *ws_bytes = style_layout(nullptr, C, n, w);
  return TRASE_OK;
}

int trase_gram_matrix(const float* x, int32_t C, int64_t n, float* G, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  if (int rc = style_check("gram_matrix", C, n, 1)) return rc;
  if (!x || !G || !ws) { set_error("gram_matrix: null pointer"); return TRASE_ERR_INVALID; }
  StyleWs w;
  if (ws_bytes < style_layout(ws, C, n, w)) { set_error("gram_matrix: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  return launch_gram(x, C, n, w, G, stream);
}

int trase_mean_std(const float* x, int32_t C, int64_t n, float eps, float* mean, float* std_, void* ws, size_t ws_bytes, int32_t device,
                   trase_stream_t stream_) {
  if (int rc = style_check("mean_std", C, n, 2)) return rc;
  if (!x || !mean || !std_ || !ws) { set_error("mean_std: null pointer"); return TRASE_ERR_INVALID; }
  StyleWs w;
  if (ws_bytes < style_layout(ws, C, n, w)) { set_error("mean_std: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  return launch_stats(x, C, n, eps, w, mean, std_, stream);
}

int trase_style_node_forward(const float* x, int32_t C, int64_t n, const float* style_gram, const float* style_mean,
                             const float* style_std, const float* content, double gram_weight, double adain_weight,
                             double content_weight, float* out4, float* saved, void* ws, size_t ws_bytes, int32_t device,
                             trase_stream_t stream_) {
  const bool use_g = gram_weight != 0.0, use_a = adain_weight != 0.0, use_c = content_weight != 0.0;
  if (int rc = style_check("style_node_forward", C, n, use_a ? 2 : 1)) return rc;
  if (!x || !out4 || !saved || !ws || (use_g && !style_gram) || (use_a && (!style_mean || !style_std)) || (use_c && !content)) {
    set_error("style_node_forward: null pointer (every term with a weight needs its target)"); return TRASE_ERR_INVALID;
  }
  if (use_c && (int64_t)C * n >= ((int64_t)1 << 31)) { set_error("style_node_forward: the content term needs C * n < 2^31"); return TRASE_ERR_INVALID; }
  StyleWs w;
  if (ws_bytes < style_layout(ws, C, n, w)) { set_error("style_node_forward: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  ReduceArgs q = {};
  q.C = C; q.n = (double)n;
  q.gram_w = gram_weight; q.adain_w = adain_weight; q.content_w = content_weight;
  q.a = saved + (size_t)C * C; q.b = q.a + C; q.out4 = out4;
  if (use_a) {
    if (int rc = launch_stats(x, C, n, 1e-8f, w, w.mean, w.stdv, stream)) return rc;
    q.mean = w.mean; q.stdv = w.stdv; q.smean = style_mean; q.sstd = style_std; q.mean64 = w.mean64; q.sd64 = w.sd64;
  }
  if (use_g) {
    if (int rc = launch_gram(x, C, n, w, w.G, stream)) return rc;
    const float coef = (float)(2.0 * (gram_weight / ((double)C * (double)C) / ((double)C * (double)n)));
    TRASE_LAUNCH("style_gram_diff", stream, 0, style_gram_diff_kernel, dim3((C * C + GD_PER - 1) / GD_PER), dim3(256), 0, (const float*)w.G,
                 style_gram, C * C, coef, saved, w.gd_part);
    q.G = w.G; q.gd_part = w.gd_part;
  }
  if (use_c) {
    const PxArgs a = px_args(x, content, 0, 1, 1, (int32_t)((int64_t)C * n), TRASE_PIXEL_L2, nullptr, TRASE_PIXEL_AUX_NONE);
    if (int rc = px_forward_launch(a, w.px.part, stream)) return rc;
    q.px_part = w.px.part; q.px_nb = px_blocks(a.n);
  }
  TRASE_LAUNCH("style_reduce", stream, 0, style_reduce_kernel, dim3(1), dim3(256), 0, q);
  return TRASE_OK;
}

int trase_style_grad_gemm(const float* D, const float* a, const float* b, float c, const float* x, const float* y, int32_t C, int64_t n,
                          const float* g, float* dx, int32_t device, trase_stream_t stream_) {
  if (int rc = style_check("style_grad_gemm", C, n, 1)) return rc;
  if (!x || !dx || (a == nullptr) != (b == nullptr)) { set_error("style_grad_gemm: null pointer (a and b come together)"); return TRASE_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const dim3 grid((unsigned)((n + GR_TILE - 1) / GR_TILE), (C + GR_TILE - 1) / GR_TILE);
  TRASE_LAUNCHES("style_grad", stream, 0,
    if (D) hipLaunchKernelGGL(style_grad_kernel<true>, grid, dim3(256), 0, stream, D, a, b, c, x, y, C, (uint32_t)n, g, dx);
    else hipLaunchKernelGGL(style_grad_kernel<false>, grid, dim3(256), 0, stream, D, a, b, c, x, y, C, (uint32_t)n, g, dx));
  return TRASE_OK;
}

}  // extern "C"
