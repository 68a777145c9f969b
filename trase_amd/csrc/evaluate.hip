// evaluate.hip -- what the reference writes for a selection and what it scores from those files, in one pass over the frame.
//   render.py:344-366 (:380-395; gui.py render_set): the all-ones render binarised at 0.5 -> inlier mask, the selection's RGB
//     blanked outside it, both turned into 8-bit frames (to8b);
//   metrics_segmentation.py:33-48, :118-150: intersection / union / equal pixels of the predicted mask against the ground
//     truth, squared error of the cut-out against the benchmark's object image.
//
// An all-ones render on black is sum(alpha_i T_i) = 1 - T_final, and the compositing kernels already keep T_final per pixel,
// so the mask needs no second rasterizer pass: this kernel reads the three image planes and final_T once.
//
// evaluate_kernel, one launch: a thread owns 4 consecutive pixels of a row.  Where the quad is whole and every plane offset
// is a multiple of 4 pixels it moves 16 bytes per plane access (float4), the mask bytes as one packed dword and the 12 bytes
// of an HWC 8-bit quad as three dwords; row tails, rows that start off a 4-pixel boundary and images whose plane size is no
// multiple of 4 take the same arithmetic through scalar accesses.  Grid-stride over the quads, at most EVAL_MAX_BLOCKS
// workgroups.
// Scores: every thread counts in registers, the counts are reduced per wave (shuffles) and per workgroup (LDS, wave order),
// and lanes 0..4 of the first wave add the five totals to the frame's record with ONE 64-bit integer atomic instruction.
// The squared error of the quantised pair is a sum of squared 8-bit differences, an exact integer, so the record does not
// depend on the order of the adds: bitwise reproducible, no float atomics.  The unquantised squared error is summed in
// float64 per thread, per wave (a fixed shuffle tree) and per workgroup (wave order) and STORED to the workgroup's own
// slot; the slots are added in index order by the reader.
#include "common.h"
#include "frame_quads.h"

namespace trase {

constexpr int EVAL_THREADS = 256;
constexpr int EVAL_WAVES = EVAL_THREADS / WAVE;
constexpr int EVAL_MAX_BLOCKS = TRASE_EVAL_MAX_BLOCKS;

struct EvalArgs {
  TraseEvalFrame f;
  const float* final_T;      // the frame's, or the img workspace's
  int vec_ok;                // every pointer is aligned for the 16-byte / dword accesses and W * H is a multiple of 4
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d, WAVE);
  return v;                                            // lane 0 holds the total
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d, WAVE);
  return v;
}

__global__ __launch_bounds__(EVAL_THREADS) void evaluate_kernel(EvalArgs a) {
  const TraseEvalFrame& f = a.f;
  const int W = f.W, Q = (W + 3) >> 2, items = Q * f.H;
  const size_t hw = (size_t)W * f.H;
  const bool have_obj = f.image != nullptr;
  const bool score_px = f.gt_mask != nullptr, score_img = have_obj && f.gt_object != nullptr && f.gt_object_kind != 0;
  // per-thread tallies: intersection, union, equal pixels; squared error as an exact integer or in float64
  unsigned long long n_inter = 0, n_union = 0, n_equal = 0, sse = 0;
  double fse = 0.0;

  for (int it = blockIdx.x * EVAL_THREADS + threadIdx.x; it < items; it += gridDim.x * EVAL_THREADS) {
    const int row = it / Q, q = it - row * Q;
    const int n = min(4, W - 4 * q);
    const size_t p0 = (size_t)row * W + 4 * q;
    const bool vec = a.vec_ok && n == 4 && (p0 & 3) == 0;

    // the predicted mask
    bool in[4] = {true, true, true, true};
    if (a.final_T) {
      float T[4], al[4];
      ld4f(a.final_T + p0, vec, n, T);
#pragma unroll
      for (int u = 0; u < 4; ++u) { al[u] = 1.0f - T[u]; in[u] = al[u] >= f.threshold; }     // a NaN is outside
      if (f.alpha) st4f(f.alpha + p0, vec, n, al);
    } else if (f.pred_in) {
      const uint32_t w = ld4b(f.pred_in + p0, vec, n);
#pragma unroll
      for (int u = 0; u < 4; ++u) in[u] = ((w >> (8 * u)) & 0xffu) != 0;
    }
    if (f.pred_mask) {
      uint32_t w = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) w |= (in[u] ? 1u : 0u) << (8 * u);
      st4b(f.pred_mask + p0, vec, n, w);
    }
    if (f.pred_mask_u8) {                              // (H, W, 3): to8b of the binarised all-ones render
      uint32_t w[3] = {0, 0, 0};
#pragma unroll
      for (int k = 0; k < 12; ++k) w[k >> 2] |= (in[k / 3] ? 0xffu : 0u) << (8 * (k & 3));
      st12b(f.pred_mask_u8 + 3 * p0, vec, n, w);
    }
    if (score_px) {
      const uint32_t w = ld4b(f.gt_mask + p0, vec, n);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (u < n) {
          const bool g = ((w >> (8 * u)) & 0xffu) != 0;
          n_inter += (in[u] && g) ? 1 : 0;
          n_union += (in[u] || g) ? 1 : 0;
          n_equal += (in[u] == g) ? 1 : 0;
        }
      }
    }
    if (!have_obj) continue;

    // the cut-out
    float obj[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ld4f(f.image + c * hw + p0, vec, n, obj[c]);
#pragma unroll
      for (int u = 0; u < 4; ++u) obj[c][u] = in[u] ? obj[c][u] : f.outside;
      if (f.object) st4f(f.object + c * hw + p0, vec, n, obj[c]);
    }
    if (f.object_u8) {
      uint32_t w[3] = {0, 0, 0};
#pragma unroll
      for (int k = 0; k < 12; ++k) w[k >> 2] |= to8b(obj[k % 3][k / 3]) << (8 * (k & 3));
      st12b(f.object_u8 + 3 * p0, vec, n, w);
    }
    if (!score_img) continue;

    // the ground-truth object image: as floats, and (8-bit inputs) as the stored bytes
    float gt[3][4];
    uint32_t gq[3][4];
    if (f.gt_object_kind == TRASE_EVAL_GT_F32_CHW) {
      const float* g = (const float*)f.gt_object;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        ld4f(g + c * hw + p0, vec, n, gt[c]);
#pragma unroll
        for (int u = 0; u < 4; ++u) gq[c][u] = save8b(gt[c][u]);
      }
    } else {
      const uint8_t* g = (const uint8_t*)f.gt_object;
      if (f.gt_object_kind == TRASE_EVAL_GT_U8_CHW) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const uint32_t w = ld4b(g + c * hw + p0, vec, n);
#pragma unroll
          for (int u = 0; u < 4; ++u) gq[c][u] = (w >> (8 * u)) & 0xffu;
        }
      } else {
        uint32_t w[3];
        ld12b(g + 3 * p0, vec, n, w);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int u = 0; u < 4; ++u) gq[c][u] = hwc_byte(w, u, c);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int u = 0; u < 4; ++u) gt[c][u] = (float)gq[c][u] / 255.0f;       // to_tensor's division
    }
    // the compared pair: as the files hold it (quantised, read back as k / 255), or as it is
    float po[4], pg[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (f.quantize) {
          const uint32_t oq = save8b(obj[c][u]);
          const int d = (int)oq - (int)gq[c][u];
          if (u < n) sse += (unsigned long long)(d * d);
          po[u] = (float)oq / 255.0f;
          pg[u] = (float)gq[c][u] / 255.0f;
        } else {
          const double d = (double)obj[c][u] - (double)gt[c][u];
          if (u < n) fse += d * d;
          po[u] = obj[c][u];
          pg[u] = gt[c][u];
        }
      }
      if (f.pair_object) st4f(f.pair_object + c * hw + p0, vec, n, po);
      if (f.pair_gt) st4f(f.pair_gt + c * hw + p0, vec, n, pg);
    }
  }

  if (!f.record || (!score_px && !score_img)) return;   // (uniform: nothing below is reached by part of a workgroup)
  __shared__ unsigned long long part[EVAL_WAVES][4];
  __shared__ double fpart[EVAL_WAVES];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  n_inter = wave_sum_u64(n_inter); n_union = wave_sum_u64(n_union); n_equal = wave_sum_u64(n_equal); sse = wave_sum_u64(sse);
  fse = wave_sum_f64(fse);
  if (lane == 0) { part[wv][0] = n_inter; part[wv][1] = n_union; part[wv][2] = n_equal; part[wv][3] = sse; fpart[wv] = fse; }
  __syncthreads();
  if (threadIdx.x < 6) {
    // lanes 0..2: the three counts; 3: the pixel count; 4: the squared error; 5: the value count.  One atomic instruction.
    const int t = threadIdx.x;
    unsigned long long v = 0;
    if (t < 3 || t == 4) {
      const int k = t < 3 ? t : 3;
#pragma unroll
      for (int w = 0; w < EVAL_WAVES; ++w) v += part[w][k];
      if ((t < 3 && !score_px) || (t == 4 && !(score_img && f.quantize))) v = 0;
    } else if (blockIdx.x == 0) {
      v = t == 3 ? (score_px ? (unsigned long long)hw : 0ull) : (score_img ? 3ull * hw : 0ull);
    }
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(f.record) + t, v);
  }
  if (threadIdx.x == 0 && score_img && !f.quantize && f.partials) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < EVAL_WAVES; ++w) s += fpart[w];
    f.partials[blockIdx.x] = s;
  }
}

static inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int launch_evaluate(const TraseEvalFrame& f, const float* final_T, hipStream_t stream) {
  EvalArgs a;
  a.f = f;
  a.final_T = final_T;
  const size_t hw = (size_t)f.W * f.H;
  a.vec_ok = (hw & 3) == 0 && aligned(f.image, 16) && aligned(final_T, 16) && aligned(f.object, 16) && aligned(f.alpha, 16) &&
             aligned(f.pair_object, 16) && aligned(f.pair_gt, 16) && aligned(f.pred_in, 4) && aligned(f.pred_mask, 4) &&
             aligned(f.object_u8, 4) && aligned(f.pred_mask_u8, 4) && aligned(f.gt_mask, 4) &&
             aligned(f.gt_object, f.gt_object_kind == TRASE_EVAL_GT_F32_CHW ? 16 : 4);
  const int items = ((f.W + 3) / 4) * f.H;
  int blocks = (items + EVAL_THREADS - 1) / EVAL_THREADS;
  if (blocks > EVAL_MAX_BLOCKS) blocks = EVAL_MAX_BLOCKS;
  TRASE_LAUNCH("evaluate", stream, 0, evaluate_kernel, dim3(blocks), dim3(EVAL_THREADS), 0, a);
  return TRASE_OK;
}

}  // namespace trase
