// dense.hip -- exact all-pairs top-k at BOTH ends of the distance order, with indices, without ever holding the M x N matrix:
// the search of loss_feature3d (utils/loss_utils.py:154-175: the kp nearest and kn farthest rows of every row in xyz) and of
// loss_cls_3d (:89-130: the k nearest rows of 800 sampled rows in the 32-d feature space).
//
// The tiling is hdbscan.hip's: grid (ceil(M / rows), S), one query row per thread held in registers; block column y walks the
// contiguous range [y * chunk, (y + 1) * chunk) of `points` in tiles of 64 rows staged through LDS, which every lane then reads
// at the same address (a broadcast).  A squared distance is the chain  s = fmaf(q_d - p_d, q_d - p_d, s), d = 0 .. D-1  (never
// |q|^2 + |p|^2 - 2 q.p), so d(i, j) == d(j, i) bit for bit; a NaN becomes the canonical 0x7FC00000.
//
// Order: every comparison is on a 64-bit integer key.  Near end: ascending (bits(d2) << 32) | id -- smaller distance first, then
// lower id.  Far end: ascending (~bits(d2) << 32) | id -- larger distance first, then lower id.  A squared distance is never
// negative, so its bits order like the number; the NaN bits rank above +inf: last at the near end, first at the far end (torch's
// topk order).  Each thread keeps its two lists (k_near + k_far keys, each ascending) as one column of an LDS array and the
// current k-th key of either end in a register: a candidate that does not enter costs one compare per end.
//
// LDS per workgroup = 64 * DP * 4 (the tile) + (k_near + k_far) * rows * 8 (the lists), kept within DT_LDS_BUDGET = 64 KiB by
// halving the rows per workgroup: 256 rows to 24 keys, 128 to 48, 64 beyond.  The largest form, 64 keys at DP = 64, takes
// 16 384 + 64 * 64 * 8 = 49 152 bytes; 48 keys at DP = 64 take exactly 65 536.
//
// S = ceil(512 / row blocks), at most 64: loss_cls_3d's 800 rows are 4 row blocks x 64 column ranges = 256 workgroups, 300 000
// rows give S = 1.  With S > 1 every (row, range) writes its keys to the workspace and dt_merge_kernel, one wave per (row, end)
// with lane s at the head of list s, takes the k smallest heads in key order.  With S = 1 the sweep writes the outputs itself.
#include "common.h"

namespace trase {

constexpr int DT_TJ = 64;                      // points per LDS tile
constexpr int DT_MAX_D = 64, DT_MAX_K = 32;
constexpr int DT_MAX_SPLIT = 64;               // column ranges per row block == lanes of the merging wave
constexpr int DT_TARGET_BLOCKS = 512;
constexpr size_t DT_LDS_BUDGET = 64 * 1024;
constexpr unsigned long long DT_EMPTY = ~0ull;      // no key: bits 0xFFFFFFFF is no distance and id 0xFFFFFFFF no row
constexpr uint32_t DT_NAN = 0x7FC00000u;

struct DtPlan { int dp, rows, row_blocks, S, chunk; size_t lds; };
static inline int dt_dpad(int D) { return D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64; }
static inline size_t dt_lds_bytes(int rows, int kt, int dp) { return (size_t)DT_TJ * dp * 4 + (size_t)kt * rows * 8; }
static DtPlan dt_plan(int M, int N, int D, int kt) {
  DtPlan p;
  p.dp = dt_dpad(D);
  p.rows = 256;
  while (p.rows > 64 && dt_lds_bytes(p.rows, kt, p.dp) > DT_LDS_BUDGET) p.rows >>= 1;
  p.lds = dt_lds_bytes(p.rows, kt, p.dp);
  p.row_blocks = (int)(((int64_t)M + p.rows - 1) / p.rows);
  int s = p.row_blocks > 0 ? (DT_TARGET_BLOCKS + p.row_blocks - 1) / p.row_blocks : 1;
  s = s < 1 ? 1 : s > DT_MAX_SPLIT ? DT_MAX_SPLIT : s;
  const int64_t c = ((int64_t)N + s - 1) / s;
  p.chunk = (int)((c + DT_TJ - 1) / DT_TJ * DT_TJ);          // a multiple of the tile; the last range may be ragged
  p.S = (int)(((int64_t)N + p.chunk - 1) / p.chunk);         // no empty range
  return p;
}

struct DtWs { unsigned long long* part; };
static size_t dt_layout(void* ws, int M, int kt, const DtPlan& p, DtWs& w) {
  WsCursor c(ws);
  w.part = c.take<unsigned long long>(p.S > 1 ? (size_t)M * p.S * kt : 0);
  return c.bytes();
}

template <int DP>
__device__ __forceinline__ void dt_load_row(const float* __restrict__ X, int D, int i, bool live, float (&x)[DP]) {
  const bool vec4 = (D & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
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
}

// rows [j0, j0 + DT_TJ) of P into LDS, zero padded to DP columns and past row `hi`
template <int DP>
__device__ __forceinline__ void dt_load_tile(const float* __restrict__ P, int D, uint32_t j0, uint32_t hi, float* xs) {
  for (int e = threadIdx.x; e < DT_TJ * DP; e += blockDim.x) {
    const int r = e / DP, d = e - r * DP;
    xs[e] = (j0 + r < hi && d < D) ? P[(size_t)(j0 + r) * D + d] : 0.f;
  }
}

// U independent chains, each in dimension order (two at 64 dimensions, where four no longer fit beside the row)
template <int DP> struct DtCols { static constexpr int U = DP > 32 ? 2 : 4; };
template <int DP>
__device__ __forceinline__ void dt_dist(const float (&x)[DP], const float* xs, int jj, float (&d2)[DtCols<DP>::U]) {
  constexpr int U = DtCols<DP>::U;
#pragma unroll
  for (int u = 0; u < U; ++u) d2[u] = 0.f;
#pragma unroll
  for (int q = 0; q < DP / 4; ++q) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float4 c = reinterpret_cast<const float4*>(xs + (jj + u) * DP)[q];
      float t = x[4 * q] - c.x;
      d2[u] = fmaf(t, t, d2[u]);
      t = x[4 * q + 1] - c.y;
      d2[u] = fmaf(t, t, d2[u]);
      t = x[4 * q + 2] - c.z;
      d2[u] = fmaf(t, t, d2[u]);
      t = x[4 * q + 3] - c.w;
      d2[u] = fmaf(t, t, d2[u]);
    }
  }
}

// key into the thread's ascending list col[q * rows], q = 0 .. k-1 (the caller has found key < col[(k - 1) * rows]); -> the new k-th key
__device__ __forceinline__ unsigned long long dt_insert(unsigned long long* col, int rows, int k, unsigned long long key) {
  int p = k - 1;
  while (p > 0 && col[(p - 1) * rows] > key) {
    col[p * rows] = col[(p - 1) * rows];
    --p;
  }
  col[p * rows] = key;
  return col[(k - 1) * rows];
}

__device__ __forceinline__ void dt_store(unsigned long long key, bool far, float* __restrict__ d2, int64_t* __restrict__ idx, size_t at) {
  const uint32_t hi = (uint32_t)(key >> 32);
  d2[at] = __uint_as_float(far ? ~hi : hi);
  idx[at] = (int64_t)(uint32_t)key;
}

template <int DP>
__global__ __launch_bounds__(256) void dt_sweep_kernel(const float* __restrict__ Q, const float* __restrict__ P, int M, int N, int D,
                                                       int kn, int kf, int chunk, int S, unsigned long long* __restrict__ part,
                                                       float* __restrict__ near_d2, int64_t* __restrict__ near_idx,
                                                       float* __restrict__ far_d2, int64_t* __restrict__ far_idx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dt_lds[];
  float* xs = reinterpret_cast<float*>(dt_lds);                                                  // DT_TJ * DP floats
  unsigned long long* list = reinterpret_cast<unsigned long long*>(dt_lds + DT_TJ * DP * 4);    // list[q * rows + tid]
  constexpr int U = DtCols<DP>::U;
  const int rows = blockDim.x, tid = threadIdx.x, kt = kn + kf;
  const int64_t i64 = (int64_t)blockIdx.x * rows + tid;
  const bool live = i64 < M;
  const int i = live ? (int)i64 : 0;
  float x[DP];
  dt_load_row<DP>(Q, D, i, live, x);
  unsigned long long* near = list + tid;
  unsigned long long* far = list + (size_t)kn * rows + tid;
  for (int q = 0; q < kt; ++q) list[q * rows + tid] = DT_EMPTY;
  unsigned long long near_kth = kn ? DT_EMPTY : 0ull, far_kth = kf ? DT_EMPTY : 0ull;      // no key is below 0: an end with k = 0 takes nothing
  const uint32_t lo = (uint32_t)blockIdx.y * (uint32_t)chunk;
  const uint32_t hi = min((uint32_t)N, lo + (uint32_t)chunk);
  for (uint32_t j0 = lo; j0 < hi; j0 += DT_TJ) {
    __syncthreads();
    dt_load_tile<DP>(P, D, j0, hi, xs);
    __syncthreads();
    const int nj = (int)min((uint32_t)DT_TJ, hi - j0);
    for (int jj = 0; jj < nj; jj += U) {
      float d2[U];
      dt_dist<DP>(x, xs, jj, d2);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!live || jj + u >= nj) continue;
        uint32_t b = __float_as_uint(d2[u]);
        if (d2[u] != d2[u]) b = DT_NAN;
        const uint32_t j = j0 + (uint32_t)(jj + u);
        const unsigned long long nkey = ((unsigned long long)b << 32) | j, fkey = ((unsigned long long)(~b) << 32) | j;
        if (nkey < near_kth) near_kth = dt_insert(near, rows, kn, nkey);
        if (fkey < far_kth) far_kth = dt_insert(far, rows, kf, fkey);
      }
    }
  }
  if (!live) return;
  if (S > 1) {
    unsigned long long* out = part + ((size_t)i * S + blockIdx.y) * kt;
    for (int q = 0; q < kt; ++q) out[q] = list[q * rows + tid];
  } else {
    for (int q = 0; q < kn; ++q) dt_store(near[(size_t)q * rows], false, near_d2, near_idx, (size_t)i * kn + q);
    for (int q = 0; q < kf; ++q) dt_store(far[(size_t)q * rows], true, far_d2, far_idx, (size_t)i * kf + q);
  }
}

__device__ __forceinline__ unsigned long long dt_shfl_xor(unsigned long long v, int off) {
  const int lo = __shfl_xor((int)(uint32_t)v, off), hi = __shfl_xor((int)(uint32_t)(v >> 32), off);
  return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}

// one wave per (row, end): lane s stands at the head of the row's ascending list of column range s; k times the smallest head
// of the wave is the next key (keys are distinct: they carry the id) and its lane steps on
__global__ __launch_bounds__(256) void dt_merge_kernel(const unsigned long long* __restrict__ part, int M, int S, int kn, int kf,
                                                       float* __restrict__ near_d2, int64_t* __restrict__ near_idx,
                                                       float* __restrict__ far_d2, int64_t* __restrict__ far_idx) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool far = blockIdx.y == 1;
  const int k = far ? kf : kn, kt = kn + kf;
  if (i >= M || k == 0) return;                                   // the whole wave
  const unsigned long long* p = part + ((size_t)i * S + (lane < S ? lane : 0)) * kt + (far ? kn : 0);
  int pos = 0;
  unsigned long long head = lane < S ? p[0] : DT_EMPTY;
  float* d2 = far ? far_d2 : near_d2;
  int64_t* idx = far ? far_idx : near_idx;
  for (int t = 0; t < k; ++t) {
    unsigned long long m = head;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = dt_shfl_xor(m, off);
      m = o < m ? o : m;
    }
    if (lane == 0) dt_store(m, far, d2, idx, (size_t)i * k + t);
    if (head == m && m != DT_EMPTY) {
      ++pos;
      head = pos < k ? p[pos] : DT_EMPTY;
    }
  }
}

static int dt_dims_ok(const char* who, int32_t M, int32_t N, int32_t D, int32_t kn, int32_t kf) {
  if (M < 0 || N < 1 || D < 1 || D > DT_MAX_D || kn < 0 || kn > DT_MAX_K || kf < 0 || kf > DT_MAX_K || kn + kf < 1 || kn > N ||
      kf > N) {
    set_error("%s: need M >= 0, 1 <= D <= %d, 0 <= k_near, k_far <= %d, one of them positive, and both <= N (got M %d, N %d, D %d, "
              "k_near %d, k_far %d)", who, DT_MAX_D, DT_MAX_K, M, N, D, kn, kf);
    return TRASE_ERR_INVALID;
  }
  return TRASE_OK;
}

}  // namespace trase

using namespace trase;

extern "C" {

int trase_dense_topk_ws_bytes(int32_t M, int32_t N, int32_t D, int32_t k_near, int32_t k_far, size_t* ws_bytes, int32_t* splits) {
  if (!ws_bytes) { set_error("trase_dense_topk_ws_bytes: null pointer"); return TRASE_ERR_INVALID; }
  if (int rc = dt_dims_ok("trase_dense_topk_ws_bytes", M, N, D, k_near, k_far)) return rc;
  const DtPlan p = dt_plan(M, N, D, k_near + k_far);
  DtWs w;
  *ws_bytes = dt_layout(nullptr, M, k_near + k_far, p, w);
  if (splits) *splits = p.S;
  return TRASE_OK;
}

int trase_dense_topk(const float* queries, int32_t M, const float* points, int32_t N, int32_t D, int32_t k_near, int32_t k_far,
                     float* near_d2, int64_t* near_idx, float* far_d2, int64_t* far_idx, void* ws, size_t ws_bytes, int32_t device,
                     trase_stream_t stream_) {
  if (int rc = dt_dims_ok("trase_dense_topk", M, N, D, k_near, k_far)) return rc;
  if (M == 0) return TRASE_OK;
  if (!queries || !points || (k_near > 0 && (!near_d2 || !near_idx)) || (k_far > 0 && (!far_d2 || !far_idx))) {
    set_error("trase_dense_topk: null pointer"); return TRASE_ERR_INVALID;
  }
  const int kt = k_near + k_far;
  const DtPlan p = dt_plan(M, N, D, kt);
  DtWs w;
  const size_t need = dt_layout(nullptr, M, kt, p, w);
  if (need > 0 && (!ws || ws_bytes < need)) { set_error("trase_dense_topk: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  dt_layout(need > 0 ? ws : nullptr, M, kt, p, w);
  const dim3 grid(p.row_blocks, p.S), block(p.rows);
#define TRASE_DT_SWEEP(DPV) hipLaunchKernelGGL((dt_sweep_kernel<DPV>), grid, block, p.lds, stream, queries, points, M, N, D, k_near, \
                                               k_far, p.chunk, p.S, w.part, near_d2, near_idx, far_d2, far_idx)
  TRASE_LAUNCHES("dense_topk_sweep", stream, 0,
    if (p.dp == 8) TRASE_DT_SWEEP(8);
    else if (p.dp == 16) TRASE_DT_SWEEP(16);
    else if (p.dp == 32) TRASE_DT_SWEEP(32);
    else TRASE_DT_SWEEP(64));
#undef TRASE_DT_SWEEP
  if (p.S > 1)
    TRASE_LAUNCH("dense_topk_merge", stream, 0, dt_merge_kernel, dim3((unsigned)(((int64_t)M + 3) / 4), 2), dim3(256), 0, w.part, M, p.S, k_near, k_far,
                 near_d2, near_idx, far_d2, far_idx);
  return TRASE_OK;
}

}  // extern "C"
