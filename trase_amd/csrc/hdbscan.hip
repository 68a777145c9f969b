// hdbscan.hip -- the device side of HDBSCAN over the sampled per-Gaussian features: the viewer's default clustering mode
// (gui.py:271-301, gui_standalone.py:721-727; hdbscan.HDBSCAN(min_cluster_size=10, cluster_selection_epsilon=0.01)).
//
// The cost of HDBSCAN is two dense all-pairs passes over X (n, D): the core distances (each row's distance to its k-th
// nearest OTHER row) and the minimum spanning tree of the mutual-reachability graph w(i,j) = max(core_i, core_j, d(i,j)).
// Both walk the same tiling and never hold an n x n buffer:
//   grid (ceil(n / 256), S): one row per thread, held in registers; block column y walks the contiguous column range
//   [y * chunk, (y + 1) * chunk) in tiles of 64 rows staged through LDS, which every lane then reads at the same address
//   (a broadcast).  S = 1024 / row blocks (1..16) spreads a 6000-row problem over 384 workgroups.
// A squared distance is the fmaf chain  s = fmaf(a_d - b_d, a_d - b_d, s), d = 0 .. D-1  -- never |a|^2 + |b|^2 - 2ab, which
// for unit features 0.01 apart would lose every digit.  (a - b)^2 == (b - a)^2 exactly and the order is fixed, so
// d(i,j) == d(j,i) bit for bit and every pass that recomputes a distance gets the same value.  All weights stay SQUARED
// fp32 on the device (the square root is monotone; the host takes it in float64).
//
// Core distances: every thread keeps the k smallest squared distances of its column range in an LDS list (ascending, one
// column of the list per thread), hd_core_merge_kernel then merges the S lists of a row.
//
// Minimum spanning tree: Boruvka rounds, each three launches that all return at once when one component is left, so the
// ceil(log2 n) rounds are enqueued without the host looking at anything:
//   1. hd_min_edge_kernel: every thread finds the lightest edge from its row into another component and lowers its
//      component's word with a 64-bit integer atomicMin.  The key is (weight bits << 32 | min(i,j) << 16 | max(i,j)): a total
//      order on undirected edges, so equal weights never close a cycle, and n <= 65536.
//   2. hd_hook_kernel: every root hooks itself to the component at the other end of its edge and files the key under its own
//      index -- an index stops being a root exactly once, so the n - 1 edges land in fixed slots without a counter.  Two
//      components that chose the same edge: the lower index stays the root.  The surviving roots are counted.
//   3. hd_jump_kernel: every point follows the hooks to its new root; the component words are reset.
// Integer atomics only: the edge set, and with it everything downstream, is bitwise reproducible.
#include "common.h"

namespace trase {

constexpr int HD_ROWS = 256;          // rows per workgroup == threads
constexpr int HD_TJ = 64;             // columns per LDS tile
constexpr int HD_MAX_N = 65536, HD_MAX_D = 64, HD_MAX_K = 64;
constexpr int HD_MAX_SPLIT = 16;      // column ranges per row block
constexpr int HD_COUNTS = 18;         // components after round r, r = 0 .. 16 (counts[0] = n), and a spare
constexpr int HD_MAX_CENTRES = 4096;  // == the limit of trase_assign_clusters
constexpr unsigned long long HD_NO_EDGE = ~0ull;

static inline int hd_dpad(int D) { return D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64; }
static inline int hd_row_blocks(int n) { return (n + HD_ROWS - 1) / HD_ROWS; }
static inline int hd_splits(int n) {
  const int s = 1024 / hd_row_blocks(n);
  return s < 1 ? 1 : s > HD_MAX_SPLIT ? HD_MAX_SPLIT : s;
}
static inline int hd_chunk(int n) {                 // columns per range, a multiple of the tile
  const int s = hd_splits(n), c = (n + s - 1) / s;
  return (c + HD_TJ - 1) / HD_TJ * HD_TJ;
}
static inline int hd_rounds(int n) {                // ceil(log2 n): every round at least halves the components
  int r = 0;
  while ((1 << r) < n) ++r;
  return r;
}

template <int DP>
__device__ __forceinline__ void hd_load_row(const float* __restrict__ X, int D, int i, bool live, float (&x)[DP]) {
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

// rows [j0, j0 + HD_TJ) of X into LDS, zero padded to DP columns and past row `hi`
template <int DP>
__device__ __forceinline__ void hd_load_tile(const float* __restrict__ X, int D, int j0, int hi, float* xs) {
  for (int e = threadIdx.x; e < HD_TJ * DP; e += HD_ROWS) {
    const int r = e / DP, d = e - r * DP;
    xs[e] = (j0 + r < hi && d < D) ? X[(size_t)(j0 + r) * D + d] : 0.f;
  }
}

// squared distances of the row in registers to tile rows jj .. jj + U - 1: U independent chains, each in dimension order
// (two at 64 dimensions, where four no longer fit the register file beside the row)
template <int DP> struct HdCols { static constexpr int U = DP > 32 ? 2 : 4; };
template <int DP>
__device__ __forceinline__ void hd_dist(const float (&x)[DP], const float* xs, int jj, float (&d2)[HdCols<DP>::U]) {
  constexpr int U = HdCols<DP>::U;
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

// part[(i * S + y) * k + q]: the q-th smallest squared distance from row i to the OTHER rows of column range y (+inf where
// the range has fewer)
template <int DP, int KC>
__global__ __launch_bounds__(HD_ROWS) void hd_core_kernel(const float* __restrict__ X, int n, int D, int k, int chunk, int S,
                                                          float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float xs[HD_TJ * DP];
  __shared__ float list[KC * HD_ROWS];          // list[q * HD_ROWS + tid]: ascending in q
  constexpr int U = HdCols<DP>::U;
  const int tid = threadIdx.x, i = blockIdx.x * HD_ROWS + tid, y = blockIdx.y;
  const bool live = i < n;
  float x[DP];
  hd_load_row<DP>(X, D, i, live, x);
  for (int q = 0; q < k; ++q) list[q * HD_ROWS + tid] = __builtin_inff();
  float worst = __builtin_inff();
  const int lo = y * chunk, hi = min(n, lo + chunk);
  for (int j0 = lo; j0 < hi; j0 += HD_TJ) {
    __syncthreads();
    hd_load_tile<DP>(X, D, j0, hi, xs);
    __syncthreads();
    const int nj = min(HD_TJ, hi - j0);
    for (int jj = 0; jj < nj; jj += U) {
      float d2[U];
      hd_dist<DP>(x, xs, jj, d2);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = j0 + jj + u;
        if (live && jj + u < nj && j != i && d2[u] < worst) {
          int p = k - 1;
          while (p > 0 && list[(p - 1) * HD_ROWS + tid] > d2[u]) {
            list[p * HD_ROWS + tid] = list[(p - 1) * HD_ROWS + tid];
            --p;
          }
          list[p * HD_ROWS + tid] = d2[u];
          worst = list[(k - 1) * HD_ROWS + tid];
        }
      }
    }
  }
  if (live) {
    float* out = part + ((size_t)i * S + y) * k;
    for (int q = 0; q < k; ++q) out[q] = list[q * HD_ROWS + tid];
  }
}

// core2[i] = the k-th smallest of the union of row i's S ascending lists
__global__ __launch_bounds__(256) void hd_core_merge_kernel(const float* __restrict__ part, int n, int k, int S,
                                                            float* __restrict__ core2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = part + (size_t)i * S * k;
  int pos[HD_MAX_SPLIT];
  float head[HD_MAX_SPLIT];
#pragma unroll
  for (int s = 0; s < HD_MAX_SPLIT; ++s) {
    pos[s] = 0;
    head[s] = s < S ? p[s * k] : __builtin_inff();
  }
  float v = __builtin_inff();
  for (int t = 0; t < k; ++t) {
    int bs = 0;
    v = head[0];
#pragma unroll
    for (int s = 1; s < HD_MAX_SPLIT; ++s)
      if (head[s] < v) { v = head[s]; bs = s; }
#pragma unroll
    for (int s = 0; s < HD_MAX_SPLIT; ++s)
      if (s == bs) {
        ++pos[s];
        head[s] = (s < S && pos[s] < k) ? p[s * k + pos[s]] : __builtin_inff();
      }
  }
  core2[i] = v;
}

__global__ __launch_bounds__(256) void hd_mst_init_kernel(int n, int32_t* __restrict__ comp, unsigned long long* __restrict__ best,
                                                          unsigned long long* __restrict__ edge_key, int32_t* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < HD_COUNTS) counts[i] = i == 0 ? n : 0;
  if (i >= n) return;
  comp[i] = i;
  best[i] = HD_NO_EDGE;
  edge_key[i] = HD_NO_EDGE;
}

template <int DP>
__global__ __launch_bounds__(HD_ROWS) void hd_min_edge_kernel(const float* __restrict__ X, int n, int D,
                                                              const float* __restrict__ core2, const int32_t* __restrict__ comp,
                                                              int chunk, unsigned long long* __restrict__ best,
                                                              const int32_t* __restrict__ counts, int round) {
  __shared__ __attribute__((aligned(16))) float xs[HD_TJ * DP];
  __shared__ float cs[HD_TJ];
  __shared__ int ks[HD_TJ];
  if (counts[round] <= 1) return;
  constexpr int U = HdCols<DP>::U;
  const int tid = threadIdx.x, i = blockIdx.x * HD_ROWS + tid, y = blockIdx.y;
  const bool live = i < n;
  float x[DP];
  hd_load_row<DP>(X, D, i, live, x);
  const int ci = live ? comp[i] : -1;
  const float core_i = live ? core2[i] : 0.f;
  float bw = __builtin_inff();
  uint32_t bpair = 0xffffffffu;                 // (65535, 65535): no edge
  const int lo = y * chunk, hi = min(n, lo + chunk);
  for (int j0 = lo; j0 < hi; j0 += HD_TJ) {
    __syncthreads();
    hd_load_tile<DP>(X, D, j0, hi, xs);
    if (tid < HD_TJ) {
      const bool in = j0 + tid < hi;
      cs[tid] = in ? core2[j0 + tid] : 0.f;
      ks[tid] = in ? comp[j0 + tid] : -1;
    }
    __syncthreads();
    const int nj = min(HD_TJ, hi - j0);
    for (int jj = 0; jj < nj; jj += U) {
      float d2[U];
      hd_dist<DP>(x, xs, jj, d2);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = j0 + jj + u;
        const float w = fmaxf(fmaxf(core_i, cs[jj + u]), d2[u]);
        if (live && jj + u < nj && ks[jj + u] != ci && w <= bw) {
          const uint32_t pair = i < j ? ((uint32_t)i << 16 | (uint32_t)j) : ((uint32_t)j << 16 | (uint32_t)i);
          if (w < bw || pair < bpair) { bw = w; bpair = pair; }
        }
      }
    }
  }
  if (live && bpair != 0xffffffffu)
    atomicMin(&best[ci], ((unsigned long long)__float_as_uint(bw) << 32) | (unsigned long long)bpair);
}

__global__ __launch_bounds__(256) void hd_hook_kernel(int n, const int32_t* __restrict__ comp,
                                                      const unsigned long long* __restrict__ best, int32_t* __restrict__ next,
                                                      unsigned long long* __restrict__ edge_key, int32_t* __restrict__ counts,
                                                      int round) {
  if (counts[round] <= 1) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int r = comp[i];
  if (r != i) { next[i] = r; return; }
  const unsigned long long key = best[i];
  int to = i;
  if (key != HD_NO_EDGE) {
    const int a = (int)((key >> 16) & 0xffffu), b = (int)(key & 0xffffu);
    const int ca = comp[a], cb = comp[b];
    const int other = ca == i ? cb : ca;
    if (!(best[other] == key && i < other)) {      // both chose this edge: the lower index stays the root
      to = other;
      edge_key[i] = key;
    }
  }
  next[i] = to;
  if (to == i) atomicAdd(&counts[round + 1], 1);
}

__global__ __launch_bounds__(256) void hd_jump_kernel(int n, const int32_t* __restrict__ next, int32_t* __restrict__ comp,
                                                      unsigned long long* __restrict__ best, const int32_t* __restrict__ counts,
                                                      int round) {
  if (counts[round] <= 1) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int r = next[i];
  for (int p = next[r]; p != r; p = next[r]) r = p;
  comp[i] = r;
  best[i] = HD_NO_EDGE;
}

__global__ __launch_bounds__(256) void hd_iota_kernel(int32_t* __restrict__ sel, int S, int base) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < S) sel[s] = base + s;
}

// centres[base + s] = normalize(sum_s / count_s) as F.normalize does (the norm clamped at 1e-12); one thread per centre
// element, the norm summed in dimension order
__global__ __launch_bounds__(64) void hd_centre_kernel(const float* __restrict__ total, int S, int D, int base,
                                                       float* __restrict__ centres) {
  __shared__ float m[HD_MAX_D];
  const int s = blockIdx.x, d = threadIdx.x;
  const float cnt = total[S * D + s];
  if (d < D) m[d] = total[s * D + d] / cnt;
  __syncthreads();
  if (d >= D) return;
  float n2 = 0.f;
  for (int e = 0; e < D; ++e) n2 = fmaf(m[e], m[e], n2);
  centres[(size_t)(base + s) * D + d] = m[d] / fmaxf(sqrtf(n2), 1e-12f);
}

struct HdWs { float* part; int32_t* comp; int32_t* next; unsigned long long* best; };
static size_t hd_layout(void* ws, int n, int k, HdWs& w) {
  WsCursor c(ws);
  w.part = c.take<float>((size_t)n * hd_splits(n) * k);
  w.comp = c.take<int32_t>((size_t)n);
  w.next = c.take<int32_t>((size_t)n);
  w.best = c.take<unsigned long long>((size_t)n);
  return c.bytes();
}
static size_t hd_ws_bytes(int n, int k) { HdWs w; return hd_layout(nullptr, n, k, w); }
// label centres: the label sums of up to LABEL_SUMS_MAX labels at a time (sums: laid out for a full batch) | the batch's labels
struct CentresWs { LabelSumsWs sums; int32_t* sel; };
static size_t centres_layout(void* ws, int N, int D, int C, CentresWs& w) {
  const int S = C < LABEL_SUMS_MAX ? C : LABEL_SUMS_MAX;
  WsCursor c(ws);
  c.take<char>(label_sums_layout(ws, N, D, S, w.sums));      // the sums start at offset 0 and their size is a multiple of the alignment
  w.sel = c.take<int32_t>((size_t)S);
  return c.bytes();
}
static bool hd_limits_ok(int n, int D, int k) {
  return n >= 2 && n <= HD_MAX_N && D >= 1 && D <= HD_MAX_D && k >= 1 && k <= HD_MAX_K && k < n;
}
#define TRASE_HD_LIMITS(fn) \
  set_error(fn ": need 2 <= n <= %d, 1 <= D <= %d, 1 <= k <= %d, k < n (got n %d, D %d, k %d)", HD_MAX_N, HD_MAX_D, HD_MAX_K, n, D, k)

}  // namespace trase

using namespace trase;

extern "C" {

int trase_hdbscan_sizes(int32_t n, int32_t D, int32_t k, size_t* ws_bytes) {
  if (!ws_bytes || !hd_limits_ok(n, D, k)) { TRASE_HD_LIMITS("trase_hdbscan_sizes"); return TRASE_ERR_INVALID; }
  *ws_bytes = hd_ws_bytes(n, k);
  return TRASE_OK;
}

int trase_hdbscan_core(const float* X, int32_t n, int32_t D, int32_t k, float* core2_out, void* ws, size_t ws_bytes,
                       int32_t device, trase_stream_t stream_) {
  if (!hd_limits_ok(n, D, k)) { TRASE_HD_LIMITS("trase_hdbscan_core"); return TRASE_ERR_INVALID; }
  if (!X || !core2_out) { set_error("trase_hdbscan_core: null pointer"); return TRASE_ERR_INVALID; }
  if (!ws || ws_bytes < hd_ws_bytes(n, k)) { set_error("trase_hdbscan_core: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  HdWs w; hd_layout(ws, n, k, w);
  const int S = hd_splits(n), chunk = hd_chunk(n), dp = hd_dpad(D);
  const dim3 grid(hd_row_blocks(n), S), block(HD_ROWS);
#define TRASE_HD_CORE(DPV, KCV) hipLaunchKernelGGL((hd_core_kernel<DPV, KCV>), grid, block, 0, stream, X, n, D, k, chunk, S, w.part)
#define TRASE_HD_CORE_K(DPV) do { if (k <= 16) TRASE_HD_CORE(DPV, 16); else TRASE_HD_CORE(DPV, 64); } while (0)
  TRASE_LAUNCHES("hdbscan_core", stream, 0,
    if (dp == 8) TRASE_HD_CORE_K(8);
    else if (dp == 16) TRASE_HD_CORE_K(16);
    else if (dp == 32) TRASE_HD_CORE_K(32);
    else TRASE_HD_CORE_K(64));
#undef TRASE_HD_CORE_K
#undef TRASE_HD_CORE
  TRASE_LAUNCH("hdbscan_core_merge", stream, 0, hd_core_merge_kernel, dim3((n + 255) / 256), dim3(256), 0, w.part, n, k, S, core2_out);
  return TRASE_OK;
}

int trase_hdbscan_mst(const float* X, int32_t n, int32_t D, const float* core2, uint64_t* edge_keys_out, int32_t* counts_out,
                      void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  const int k = 1;
  if (!hd_limits_ok(n, D, k)) { TRASE_HD_LIMITS("trase_hdbscan_mst"); return TRASE_ERR_INVALID; }
  if (!X || !core2 || !edge_keys_out || !counts_out) { set_error("trase_hdbscan_mst: null pointer"); return TRASE_ERR_INVALID; }
  if (!ws || ws_bytes < hd_ws_bytes(n, k)) { set_error("trase_hdbscan_mst: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  HdWs w; hd_layout(ws, n, k, w);
  const int S = hd_splits(n), chunk = hd_chunk(n), dp = hd_dpad(D), rounds = hd_rounds(n);
  const dim3 grid(hd_row_blocks(n), S), block(HD_ROWS), grid1((n + 255) / 256), block1(256);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(edge_keys_out);
  hipLaunchKernelGGL(hd_mst_init_kernel, grid1, block1, 0, stream, n, w.comp, w.best, keys, counts_out);
  TRASE_POST_LAUNCH("hdbscan_mst_init", stream, 0);      // the check alone: this launch has never had a scope (a report key) of its own
#define TRASE_HD_EDGE(DPV) hipLaunchKernelGGL((hd_min_edge_kernel<DPV>), grid, block, 0, stream, X, n, D, core2, w.comp, chunk, w.best, counts_out, r)
  for (int r = 0; r < rounds; ++r) {
    TRASE_LAUNCHES("hdbscan_min_edge", stream, 0,
      if (dp == 8) TRASE_HD_EDGE(8);
      else if (dp == 16) TRASE_HD_EDGE(16);
      else if (dp == 32) TRASE_HD_EDGE(32);
      else TRASE_HD_EDGE(64));
    TRASE_LAUNCHES("hdbscan_hook", stream, 0,
      hipLaunchKernelGGL(hd_hook_kernel, grid1, block1, 0, stream, n, w.comp, w.best, w.next, keys, counts_out, r);
      hipLaunchKernelGGL(hd_jump_kernel, grid1, block1, 0, stream, n, w.next, w.comp, w.best, counts_out, r));
  }
#undef TRASE_HD_EDGE
  return TRASE_OK;
}

int trase_label_centres_sizes(int32_t N, int32_t D, int32_t C, size_t* ws_bytes) {
  if (!ws_bytes || N < 0 || C < 1 || C > HD_MAX_CENTRES || D < 1 || D > HD_MAX_D) {
    set_error("trase_label_centres_sizes: need 1 <= C <= %d, 1 <= D <= %d (got N %d, D %d, C %d)", HD_MAX_CENTRES, HD_MAX_D, N, D, C);
    return TRASE_ERR_INVALID;
  }
  CentresWs w;
  *ws_bytes = centres_layout(nullptr, N, D, C, w);
  return TRASE_OK;
}

int trase_label_centres(const float* X, int32_t N, int32_t D, const int32_t* labels, int32_t C, float* centres_out, void* ws,
                        size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  if (N < 0 || C < 1 || C > HD_MAX_CENTRES || D < 1 || D > HD_MAX_D) {
    set_error("trase_label_centres: need 1 <= C <= %d, 1 <= D <= %d (got N %d, D %d, C %d)", HD_MAX_CENTRES, HD_MAX_D, N, D, C);
    return TRASE_ERR_INVALID;
  }
  if (!X || !labels || !centres_out) { set_error("trase_label_centres: null pointer"); return TRASE_ERR_INVALID; }
  CentresWs w;
  if (!ws || ws_bytes < centres_layout(ws, N, D, C, w)) { set_error("trase_label_centres: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  for (int base = 0; base < C; base += LABEL_SUMS_MAX) {          // the per-cluster sums of K-means, 128 labels at a time
    const int S = C - base < LABEL_SUMS_MAX ? C - base : LABEL_SUMS_MAX;
    TRASE_LAUNCHES("label_centres", stream, 0,
      hipLaunchKernelGGL(hd_iota_kernel, dim3(1), dim3(256), 0, stream, w.sel, S, base);
      if (S < LABEL_SUMS_MAX) label_sums_layout(ws, N, D, S, w.sums);      // a last, shorter batch packs its slabs closer: inside the full batch's bytes
      const int rc = launch_label_sums(X, N, D, labels, w.sel, S, w.sums, stream);
      if (rc) return rc;
      hipLaunchKernelGGL(hd_centre_kernel, dim3(S), dim3(64), 0, stream, w.sums.total, S, D, base, centres_out));
  }
  return TRASE_OK;
}

}  // extern "C"
