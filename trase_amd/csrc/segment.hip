// segment.hip -- the segmentation stage after training: K-means over the per-Gaussian features and the per-frame query
// masks built from the clusters.
//   kmeans_pytorch.kmeans(X, K, distance='euclidean')            gui.py:248-270, gui_standalone.py:685-707
//   render.py:97-105 postprocessing + the loop at render.py:334-345 (also :370-380, gui.py:457-464, :598-607, :828)
//
// One Lloyd step is three launches, all of which return at once when the device state word says `done`, so the host can
// enqueue a batch of steps and look at the state once per batch:
//   1. seg_assign_accum_kernel<0>: G blocks (about one per CU), block b owns the contiguous point range
//      [b * chunk, (b + 1) * chunk).  The block walks its range in tiles of SEG_TILE points:
//        a. one thread per point: argmin_k (|c_k|^2 - 2 x.c_k) against the centres in LDS (ties to the lowest k);
//           writes ids and the tile's slots to LDS;
//        b. the first `wacc` waves of the block add the tile's rows into their own K x D slab in LDS (one lane per
//           dimension, lane 0 also counts): wave w takes the w-th contiguous sub-range of the tile, in point order.
//      At the end the block sums its wave slabs in wave order (0 + w0 + w1 + ...) into block slab b in global memory.
//   2. seg_reduce_kernel: every element of the G block slabs is summed in block order, as 16 contiguous runs of
//      ceil(G/16) blocks each (run p in block order), the 16 run sums then added in run order.
//   3. kmeans_finalize_kernel (one block): centres = sum / count, empty clusters re-seeded, center_shift, state word.
// No float atomics anywhere, and wacc, G and the run split depend only on (N, K, D): the summation order is fixed, so a
// step is bitwise reproducible from run to run.
//
// The query mask reuses launches 1 and 2 with the slots taken from the selected ids instead of the nearest centre
// (seg_assign_accum_kernel<1>), then scores every member point against its cluster's normalised mean in fp16
// (seg_mask_kernel).
//
// seg_assign_cosine_kernel (gui.py:276 + :288-290) is launch 1a alone with the cosine score in place of the distance and up
// to 4096 centres, chunked through LDS: the ids of clusters that did not come from K-means.
#include <hip/hip_fp16.h>

#include "common.h"

namespace trase {

constexpr int SEG_TILE = 512;                 // points per tile == threads per block of the assign/accumulate kernel
constexpr int SEG_WAVES = SEG_TILE / WAVE;    // 8
constexpr int SEG_MAX_K = 128, SEG_MAX_D = 64, SEG_MAX_S = 128;
constexpr int SEG_MAX_ASSIGN_K = 4096;         // assign_clusters: the bin limit of the prompt lift (knn.hip)
constexpr int SEG_MAX_BLOCKS = 256;           // about one block per CU
constexpr int SEG_LDS_FLOATS = 34816;         // 136 KiB: centres + tile slots + wave slabs (one block per CU)
constexpr int SEG_RUNS = 16;                  // seg_reduce_kernel: block runs per element

// kmeans state word (int32[4], device): {iterations, done, center_shift of the last step (float bits), 0}
enum { ST_ITER = 0, ST_DONE = 1, ST_SHIFT = 2 };

static inline int seg_dpad(int D) { return D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64; }
static inline int seg_blocks(int N) {
  const int g = (N + SEG_TILE - 1) / SEG_TILE;
  return g < 1 ? 1 : g > SEG_MAX_BLOCKS ? SEG_MAX_BLOCKS : g;
}
static inline int seg_head_floats(int K, int D) { return K * seg_dpad(D) + K + SEG_TILE; }
static inline int seg_slab_floats(int K, int D) { return K * (D + 1); }   // K x D sums, then K counts
static inline int seg_wacc(int K, int D) {
  const int w = (SEG_LDS_FLOATS - seg_head_floats(K, D)) / seg_slab_floats(K, D);
  return w > SEG_WAVES ? SEG_WAVES : w;                       // >= 1 for every K <= 128, D <= 64
}

// splitmix64 (Steele, Lea, Flood 2014): the output for state x, i.e. the increment added first
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// MODE 0 (kmeans): slot = nearest centre, written to `slot_out` as the cluster id.
// MODE 1 (segment mask): slot = position of the point's id in `sel` (-1: not selected), written to `slot_out`.
template <int MODE, int DP>
__global__ __launch_bounds__(SEG_TILE) void seg_assign_accum_kernel(const float* __restrict__ X, int N, int D, int K,
                                                                   const float* __restrict__ centres,
                                                                   const int32_t* __restrict__ ids,
                                                                   const int32_t* __restrict__ sel, int32_t* __restrict__ slot_out,
                                                                   float* __restrict__ slabs, int chunk, int wacc,
                                                                   const int32_t* __restrict__ state) {
  __shared__ __attribute__((aligned(16))) float lds[SEG_LDS_FLOATS];
  if (MODE == 0 && state[ST_DONE]) return;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  float* c_lds = lds;                                  // MODE 0: (K, DP) centres, zero padded;  MODE 1: K selected ids
  float* cc_lds = lds + K * DP;                        // MODE 0: |c_k|^2
  int* tile_slot = reinterpret_cast<int*>(lds + K * DP + K);
  float* wslab = lds + K * DP + K + SEG_TILE;          // wacc slabs of E floats
  const int E = K * (D + 1);

  if (MODE == 0) {
    for (int e = tid; e < K * DP; e += SEG_TILE) {
      const int k = e / DP, d = e - k * DP;
      c_lds[e] = d < D ? centres[k * D + d] : 0.f;
    }
  } else {
    for (int e = tid; e < K; e += SEG_TILE) reinterpret_cast<int*>(c_lds)[e] = sel[e];
  }
  for (int e = tid; e < wacc * E; e += SEG_TILE) wslab[e] = 0.f;
  __syncthreads();
  if (MODE == 0) {
    for (int k = tid; k < K; k += SEG_TILE) {
      float s = 0.f;
      for (int d = 0; d < D; ++d) s = fmaf(c_lds[k * DP + d], c_lds[k * DP + d], s);
      cc_lds[k] = s;
    }
    __syncthreads();
  }

  const int lo = blockIdx.x * chunk;
  const int hi = min(N, lo + chunk);
  const bool vec4 = (D & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  for (int t0 = lo; t0 < hi; t0 += SEG_TILE) {
    const int i = t0 + tid;
    int s = -1;
    if (i < hi) {
      if (MODE == 0) {
        float x[DP];
        if (vec4) {
#pragma unroll
          for (int d = 0; d < DP; d += 4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (d < D) v = *reinterpret_cast<const float4*>(X + (size_t)i * D + d);
            x[d] = v.x; x[d + 1] = v.y; x[d + 2] = v.z; x[d + 3] = v.w;
          }
        } else {
#pragma unroll
          for (int d = 0; d < DP; ++d) x[d] = d < D ? X[(size_t)i * D + d] : 0.f;
        }
        float best = __builtin_inff();
        int bk = 0;
        for (int k = 0; k < K; ++k) {
          const float4* c4 = reinterpret_cast<const float4*>(c_lds + k * DP);
          float dot = 0.f;
#pragma unroll
          for (int q = 0; q < DP / 4; ++q) {
            const float4 c = c4[q];
            dot = fmaf(x[4 * q], c.x, dot);
            dot = fmaf(x[4 * q + 1], c.y, dot);
            dot = fmaf(x[4 * q + 2], c.z, dot);
            dot = fmaf(x[4 * q + 3], c.w, dot);
          }
          const float dist = fmaf(-2.f, dot, cc_lds[k]);   // |x - c_k|^2 - |x|^2
          if (dist < best) { best = dist; bk = k; }         // strict: ties go to the lowest k, as torch.argmin
        }
        s = bk;
      } else {
        const int id = ids[i];
        if (id >= 0) {
          const int* sl = reinterpret_cast<const int*>(c_lds);
          for (int k = 0; k < K; ++k)
            if (sl[k] == id) { s = k; break; }
        }
      }
      slot_out[i] = s;
    }
    tile_slot[tid] = s;
    __syncthreads();
    if (wave < wacc) {
      const int n = min(SEG_TILE, hi - t0);
      const int per = (SEG_TILE + wacc - 1) / wacc;
      const int j0 = wave * per, j1 = min(n, j0 + per);
      float* slab = wslab + wave * E;
      float* cnt = slab + K * D;
      int j = j0;
      for (; j + 4 <= j1; j += 4) {                       // four rows in flight, added in point order
        int sj[4];
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          sj[u] = tile_slot[j + u];
          v[u] = (sj[u] >= 0 && lane < D) ? X[(size_t)(t0 + j + u) * D + lane] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (sj[u] >= 0) {
            if (lane < D) slab[sj[u] * D + lane] += v[u];
            if (lane == 0) cnt[sj[u]] += 1.f;
          }
        }
      }
      for (; j < j1; ++j) {
        const int sj = tile_slot[j];
        if (sj >= 0) {
          if (lane < D) slab[sj * D + lane] += X[(size_t)(t0 + j) * D + lane];
          if (lane == 0) cnt[sj] += 1.f;
        }
      }
    }
    __syncthreads();
  }
  float* out = slabs + (size_t)blockIdx.x * E;
  for (int e = tid; e < E; e += SEG_TILE) {
    float v = 0.f;
    for (int w = 0; w < wacc; ++w) v += wslab[w * E + e];
    out[e] = v;
  }
}

// total[e] = sum over the G block slabs of element e, in block order (16 runs of consecutive blocks, then the runs in order)
__global__ __launch_bounds__(256) void seg_reduce_kernel(const float* __restrict__ slabs, int G, int E, float* __restrict__ total,
                                                         const int32_t* __restrict__ state) {
  __shared__ float part[SEG_RUNS][16];
  if (state && state[ST_DONE]) return;
  const int el = threadIdx.x & 15, p = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el;
  const int run = (G + SEG_RUNS - 1) / SEG_RUNS;
  const int g0 = p * run, g1 = min(G, g0 + run);
  float v = 0.f;
  if (e < E)
    for (int g = g0; g < g1; ++g) v += slabs[(size_t)g * E + e];
  part[p][el] = v;
  __syncthreads();
  if (p == 0 && e < E) {
    float t = 0.f;
    for (int q = 0; q < SEG_RUNS; ++q) t += part[q][el];
    total[e] = t;
  }
}

// One block: new centres, re-seeding of empty clusters, center_shift, state word.
__global__ __launch_bounds__(1024) void kmeans_finalize_kernel(const float* __restrict__ X, int N, int D, int K,
                                                               const float* __restrict__ total, float* __restrict__ centres,
                                                               uint64_t key, float tol, int iter_limit, int32_t* __restrict__ state) {
  __shared__ float dsq[SEG_MAX_K * SEG_MAX_D];
  __shared__ float shift_k[SEG_MAX_K];
  if (state[ST_DONE]) return;
  const int it = state[ST_ITER];
  for (int e = threadIdx.x; e < K * D; e += blockDim.x) {
    const int k = e / D, d = e - k * D;
    const float cnt = total[K * D + k];
    float c;
    if (cnt > 0.f) {
      c = total[e] / cnt;
    } else {     // empty in iteration `it`: row splitmix64(key ^ (it << 32 | k)) mod N
      const uint64_t r = splitmix64(key ^ (((uint64_t)(uint32_t)it << 32) | (uint64_t)(uint32_t)k)) % (uint64_t)N;
      c = X[(size_t)r * D + d];
    }
    const float diff = c - centres[e];
    dsq[e] = diff * diff;
    centres[e] = c;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    float s = 0.f;
    for (int d = 0; d < D; ++d) s += dsq[k * D + d];
    shift_k[k] = sqrtf(s);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float shift = 0.f;
    for (int k = 0; k < K; ++k) shift += shift_k[k];
    const int n_it = it + 1;
    const bool done = shift * shift < tol || (iter_limit != 0 && n_it >= iter_limit);
    state[ST_SHIFT] = __float_as_int(shift);
    state[ST_ITER] = n_it;
    state[ST_DONE] = done ? 1 : 0;
  }
}

// render.py:97-105 for the points of the selected clusters: score = fp16( fp16(x / |x|) . fp16(q / |q|) ), fp32 sums,
// q = mean of the cluster's rows; mask = score >= fp16(threshold).  Unselected points, negative ids: 0.  A zero row or an
// empty cluster gives a NaN score, which fails the comparison as the reference's does.
__global__ __launch_bounds__(256) void seg_mask_kernel(const float* __restrict__ X, int N, int D, int S,
                                                       const float* __restrict__ total, const int32_t* __restrict__ slot,
                                                       float threshold, uint8_t* __restrict__ mask) {
  __shared__ float q[SEG_MAX_S * SEG_MAX_D];
  __shared__ float qn[SEG_MAX_S];
  for (int e = threadIdx.x; e < S * D; e += blockDim.x) {
    const int s = e / D;
    q[e] = total[e] / total[S * D + s];
  }
  __syncthreads();
  for (int s = threadIdx.x; s < S; s += blockDim.x) {
    float n2 = 0.f;
    for (int d = 0; d < D; ++d) n2 = fmaf(q[s * D + d], q[s * D + d], n2);
    qn[s] = sqrtf(n2);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < S * D; e += blockDim.x) q[e] = __half2float(__float2half(q[e] / qn[e / D]));
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int s = slot[i];
  uint8_t m = 0;
  if (s >= 0) {
    const float* x = X + (size_t)i * D;
    float n2 = 0.f;
    for (int d = 0; d < D; ++d) n2 = fmaf(x[d], x[d], n2);
    const float n = sqrtf(n2);
    float dot = 0.f;
    for (int d = 0; d < D; ++d) dot = fmaf(__half2float(__float2half(x[d] / n)), q[s * D + d], dot);
    const float thr = __half2float(__float2half(threshold));
    m = __half2float(__float2half(dot)) >= thr ? 1 : 0;
  }
  mask[i] = m;
}

// gui.py:276 + :288-290: id = argmax_k <x / |x|, c_k> for every row, the centres used as given.  One row per lane, held in
// registers; the centres go through LDS in chunks of ASSIGN_CHUNK_FLOATS / DP.  The dot product of a row with a centre is four
// fmaf chains over the dimensions d = 0, 1, 2, 3 (mod 4), added as (s0 + s1) + (s2 + s3); the division by |x| is common to
// all k, so the raw dot products are compared (strictly: ties go to the lowest k) and only the winner's is divided, by
// max(|x|, 1e-12) as F.normalize does: a zero row gets id 0 and score 0.
constexpr int ASSIGN_THREADS = 256;
constexpr int ASSIGN_CHUNK_FLOATS = 16384;    // 64 KiB of centres per chunk

template <int DP>
__global__ __launch_bounds__(ASSIGN_THREADS) void seg_assign_cosine_kernel(const float* __restrict__ X, int N, int D, int K,
                                                                           const float* __restrict__ centres,
                                                                           int64_t* __restrict__ ids_out, float* __restrict__ scores_out) {
  __shared__ __attribute__((aligned(16))) float c_lds[ASSIGN_CHUNK_FLOATS];
  constexpr int KC = ASSIGN_CHUNK_FLOATS / DP;
  const int tid = threadIdx.x;
  const int i = blockIdx.x * ASSIGN_THREADS + tid;
  const bool live = i < N;
  const bool vec4 = (D & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  float x[DP];
  if (live && vec4) {
#pragma unroll
    for (int d = 0; d < DP; d += 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (d < D) v = *reinterpret_cast<const float4*>(X + (size_t)i * D + d);
      x[d] = v.x; x[d + 1] = v.y; x[d + 2] = v.z; x[d + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int d = 0; d < DP; ++d) x[d] = (live && d < D) ? X[(size_t)i * D + d] : 0.f;
  }
  float n2 = 0.f;
#pragma unroll
  for (int d = 0; d < DP; ++d) n2 = fmaf(x[d], x[d], n2);
  float best = -__builtin_inff();
  int bk = 0;
  for (int k0 = 0; k0 < K; k0 += KC) {
    const int kc = min(KC, K - k0);
    __syncthreads();
    for (int e = tid; e < kc * DP; e += ASSIGN_THREADS) {
      const int k = e / DP, d = e - k * DP;
      c_lds[e] = d < D ? centres[(size_t)(k0 + k) * D + d] : 0.f;
    }
    __syncthreads();
    for (int k = 0; k < kc; ++k) {
      const float4* c4 = reinterpret_cast<const float4*>(c_lds + k * DP);
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
      for (int q = 0; q < DP / 4; ++q) {
        const float4 c = c4[q];
        s0 = fmaf(x[4 * q], c.x, s0);
        s1 = fmaf(x[4 * q + 1], c.y, s1);
        s2 = fmaf(x[4 * q + 2], c.z, s2);
        s3 = fmaf(x[4 * q + 3], c.w, s3);
      }
      const float dot = (s0 + s1) + (s2 + s3);
      if (dot > best) { best = dot; bk = k0 + k; }
    }
  }
  if (live) {
    ids_out[i] = bk;
    if (scores_out) scores_out[i] = best / fmaxf(sqrtf(n2), 1e-12f);
  }
}

}  // namespace trase

using namespace trase;

// per-block slabs | their sum | (the query mask and the label sums only) every sample's slot
static size_t seg_layout(void* ws, int32_t N, int32_t D, int32_t K, bool with_slots, LabelSumsWs& w) {
  const size_t E = (size_t)seg_slab_floats(K, D);
  WsCursor c(ws);
  w.slabs = c.take<float>(E * seg_blocks(N));
  w.total = c.take<float>(E);
  w.slot = with_slots ? c.take<int32_t>((size_t)N) : nullptr;
  return c.bytes();
}
static size_t seg_ws_bytes(int32_t N, int32_t D, int32_t K, bool with_slots) { LabelSumsWs w; return seg_layout(nullptr, N, D, K, with_slots, w); }

static int seg_launch_accum(int mode, const float* X, int32_t N, int32_t D, int32_t K, const float* centres, const int32_t* ids,
                            const int32_t* sel, int32_t* slot_out, float* slabs, const int32_t* state, hipStream_t stream) {
  const int G = seg_blocks(N), chunk = (N + G - 1) / G, wacc = seg_wacc(K, D), dp = seg_dpad(D);
#define TRASE_SEG_ACC(M, DPV) hipLaunchKernelGGL((seg_assign_accum_kernel<M, DPV>), dim3(G), dim3(SEG_TILE), 0, stream, X, N, D, K, \
                                                 centres, ids, sel, slot_out, slabs, chunk, wacc, state)
  if (mode == 1) TRASE_SEG_ACC(1, 8);
  else if (dp == 8) TRASE_SEG_ACC(0, 8);
  else if (dp == 16) TRASE_SEG_ACC(0, 16);
  else if (dp == 32) TRASE_SEG_ACC(0, 32);
  else TRASE_SEG_ACC(0, 64);
#undef TRASE_SEG_ACC
  return TRASE_OK;
}

// The per-label sums of the query mask for callers outside this file (hdbscan.hip: the centres of labelled samples): launches
// 1 and 2 with the slots taken from `sel` (S <= LABEL_SUMS_MAX labels on the device).  *total_out (inside ws) then holds the
// S x D sums followed by the S counts.  w: label_sums_layout(ws, N, D, S, w).
namespace trase {
size_t label_sums_layout(void* ws, int N, int D, int S, LabelSumsWs& w) { return seg_layout(ws, N, D, S, true, w); }
int launch_label_sums(const float* X, int N, int D, const int32_t* ids, const int32_t* sel, int S, const LabelSumsWs& w, hipStream_t stream) {
  static_assert(LABEL_SUMS_MAX == SEG_MAX_S, "label sums go through the query mask's accumulate kernel");
  const int G = seg_blocks(N), E = seg_slab_floats(S, D);
  // on the primitive: these two launches run inside the caller's profiler scope, not in one of their own
  seg_launch_accum(1, X, N, D, S, nullptr, ids, sel, w.slot, w.slabs, nullptr, stream);
  TRASE_POST_LAUNCH("label_sums_accum", stream, 0);
  hipLaunchKernelGGL(seg_reduce_kernel, dim3((E + 15) / 16), dim3(256), 0, stream, w.slabs, G, E, w.total, nullptr);
  TRASE_POST_LAUNCH("label_sums_reduce", stream, 0);
  return TRASE_OK;
}
}  // namespace trase

extern "C" {

int trase_kmeans_sizes(int32_t N, int32_t D, int32_t K, size_t* ws_bytes) {
  if (!ws_bytes || N < K || K < 1 || K > SEG_MAX_K || D < 1 || D > SEG_MAX_D) {
    set_error("trase_kmeans_sizes: need 1 <= K <= %d, 1 <= D <= %d, N >= K (got N %d, D %d, K %d)", SEG_MAX_K, SEG_MAX_D, N, D, K);
    return TRASE_ERR_INVALID;
  }
  *ws_bytes = seg_ws_bytes(N, D, K, false);
  return TRASE_OK;
}

int trase_kmeans_steps(const float* X, int32_t N, int32_t D, int32_t K, float* centres, int32_t* ids_out, uint64_t reseed_key,
                       float tol, int32_t iter_limit, int32_t n_steps, int32_t* state, void* ws, size_t ws_bytes, int32_t device,
                       trase_stream_t stream_) {
  if (N < K || K < 1 || K > SEG_MAX_K || D < 1 || D > SEG_MAX_D) {
    set_error("trase_kmeans_steps: need 1 <= K <= %d, 1 <= D <= %d, N >= K (got N %d, D %d, K %d)", SEG_MAX_K, SEG_MAX_D, N, D, K);
    return TRASE_ERR_INVALID;
  }
  if (n_steps < 0 || iter_limit < 0) { set_error("trase_kmeans_steps: bad arguments (n_steps %d, iter_limit %d)", n_steps, iter_limit); return TRASE_ERR_INVALID; }
  if (!X || !centres || !ids_out || !state) { set_error("trase_kmeans_steps: null pointer"); return TRASE_ERR_INVALID; }
  if (!ws || ws_bytes < seg_ws_bytes(N, D, K, false)) { set_error("trase_kmeans_steps: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const int G = seg_blocks(N), E = seg_slab_floats(K, D);
  LabelSumsWs w; seg_layout(ws, N, D, K, false, w);
  for (int step = 0; step < n_steps; ++step) {
    TRASE_LAUNCHES("kmeans_assign_accum", stream, 0,
                   seg_launch_accum(0, X, N, D, K, centres, nullptr, nullptr, ids_out, w.slabs, state, stream));
    TRASE_LAUNCH("kmeans_reduce", stream, 0, seg_reduce_kernel, dim3((E + 15) / 16), dim3(256), 0, w.slabs, G, E, w.total, state);
    TRASE_LAUNCH("kmeans_finalize", stream, 0, kmeans_finalize_kernel, dim3(1), dim3(1024), 0, X, N, D, K, w.total, centres, reseed_key, tol,
                 iter_limit, state);
  }
  return TRASE_OK;
}

int trase_segment_mask_sizes(int32_t N, int32_t D, int32_t S, size_t* ws_bytes) {
  if (!ws_bytes || N < 0 || S < 0 || S > SEG_MAX_S || D < 1 || D > SEG_MAX_D) {
    set_error("trase_segment_mask_sizes: need 0 <= S <= %d, 1 <= D <= %d (got N %d, D %d, S %d)", SEG_MAX_S, SEG_MAX_D, N, D, S);
    return TRASE_ERR_INVALID;
  }
  *ws_bytes = seg_ws_bytes(N, D, S > 0 ? S : 1, true);
  return TRASE_OK;
}

int trase_segment_mask(const float* X, int32_t N, int32_t D, const int32_t* ids, const int32_t* sel, int32_t S, float threshold,
                       uint8_t* mask_out, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  if (N < 0 || S < 0 || S > SEG_MAX_S || D < 1 || D > SEG_MAX_D) {
    set_error("trase_segment_mask: need 0 <= S <= %d, 1 <= D <= %d (got N %d, D %d, S %d)", SEG_MAX_S, SEG_MAX_D, N, D, S);
    return TRASE_ERR_INVALID;
  }
  if (N == 0) return TRASE_OK;
  if (!X || !ids || !mask_out || (S > 0 && !sel)) { set_error("trase_segment_mask: null pointer"); return TRASE_ERR_INVALID; }
  if (!ws || ws_bytes < seg_ws_bytes(N, D, S > 0 ? S : 1, true)) { set_error("trase_segment_mask: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  if (S == 0) return launch_zero_bytes(mask_out, (size_t)N, stream);
  const int G = seg_blocks(N), E = seg_slab_floats(S, D);
  LabelSumsWs w; seg_layout(ws, N, D, S, true, w);
  TRASE_LAUNCHES("segment_accum", stream, 0, seg_launch_accum(1, X, N, D, S, nullptr, ids, sel, w.slot, w.slabs, nullptr, stream));
  TRASE_LAUNCH("segment_reduce", stream, 0, seg_reduce_kernel, dim3((E + 15) / 16), dim3(256), 0, w.slabs, G, E, w.total, nullptr);
  TRASE_LAUNCH("segment_mask", stream, 0, seg_mask_kernel, dim3((N + 255) / 256), dim3(256), 0, X, N, D, S, w.total, w.slot, threshold, mask_out);
  return TRASE_OK;
}

int trase_assign_clusters_sizes(int32_t N, int32_t D, int32_t K, size_t* ws_bytes) {
  if (!ws_bytes || N < 0 || K < 1 || K > SEG_MAX_ASSIGN_K || D < 1 || D > SEG_MAX_D) {
    set_error("trase_assign_clusters_sizes: need 1 <= K <= %d, 1 <= D <= %d (got N %d, D %d, K %d)", SEG_MAX_ASSIGN_K, SEG_MAX_D, N, D, K);
    return TRASE_ERR_INVALID;
  }
  *ws_bytes = 0;        // the centres go from global memory to LDS directly: nothing to stage
  return TRASE_OK;
}

int trase_assign_clusters(const float* X, int32_t N, int32_t D, const float* centres, int32_t K, int64_t* ids_out,
                          float* scores_out, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  if (N < 0 || K < 1 || K > SEG_MAX_ASSIGN_K || D < 1 || D > SEG_MAX_D) {
    set_error("trase_assign_clusters: need 1 <= K <= %d, 1 <= D <= %d (got N %d, D %d, K %d)", SEG_MAX_ASSIGN_K, SEG_MAX_D, N, D, K);
    return TRASE_ERR_INVALID;
  }
  if (N == 0) return TRASE_OK;
  if (!X || !centres || !ids_out) { set_error("trase_assign_clusters: null pointer"); return TRASE_ERR_INVALID; }
  (void)ws; (void)ws_bytes;
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const int dp = seg_dpad(D);
  const dim3 grid((N + ASSIGN_THREADS - 1) / ASSIGN_THREADS), block(ASSIGN_THREADS);
  TRASE_LAUNCHES("assign_clusters", stream, 0,
    if (dp == 8) hipLaunchKernelGGL((seg_assign_cosine_kernel<8>), grid, block, 0, stream, X, N, D, K, centres, ids_out, scores_out);
    else if (dp == 16) hipLaunchKernelGGL((seg_assign_cosine_kernel<16>), grid, block, 0, stream, X, N, D, K, centres, ids_out, scores_out);
    else if (dp == 32) hipLaunchKernelGGL((seg_assign_cosine_kernel<32>), grid, block, 0, stream, X, N, D, K, centres, ids_out, scores_out);
    else hipLaunchKernelGGL((seg_assign_cosine_kernel<64>), grid, block, 0, stream, X, N, D, K, centres, ids_out, scores_out));
  return TRASE_OK;
}

}  // extern "C"
