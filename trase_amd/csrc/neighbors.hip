// neighbors.hip -- losses over a k-NN graph without N x k x ... edge tensors (utils/loss_utils.py:132-152 loss_reg_3d_feature,
// :179-221 loss_rigid_body_motion_reg_loss).
//
// A graph is idx (N, k) int32: edge number e = i * k + slot runs from row i (the "+" end) to row idx[e] (the "-" end).  A loss
// over the edges sends gradient to BOTH ends.  The "+" end is a loop over the row's own slots; the "-" end needs every edge
// that points AT a row.  Like every other backward of this library it is a gather, not a float atomic: the graph is transposed
// once (trase_graph_reverse: the stable radix sort of binning.hip over the targets with iota values, then launch_tile_ranges) and
// each row walks its incoming edges in ascending edge order, so every sum has one fixed order and is bitwise reproducible.
// An id outside [0, N) (a caller's own index tensor) is an edge to nowhere: it lands in no range and is never dereferenced.
#include "common.h"
#include "rigid_math.h"

namespace trase {

// ---- the transposed graph ---------------------------------------------------------------------------------------------
struct RevWs { uint32_t* n; SortBufs sort; uint2* ranges; };
static int rev_bits(int N) {
  int bits = 1;
  while ((1u << bits) < (uint32_t)N + 1u) ++bits;      // keys 0 .. N (N = "no such row")
  return bits;
}
// rows source rows of k edges each into `targets` target rows (the square graph: targets == rows)
static size_t rev_layout(void* ws, int rows, int k, int targets, RevWs& w) {
  WsCursor c(ws);
  const size_t M = (size_t)rows * (size_t)k;
  w.n = c.take<uint32_t>(1);
  sort_layout(c, w.sort, M > 0 ? M : 1, SORT_ALL, 8, 1);
  w.ranges = c.take<uint2>((size_t)targets + 1);
  return c.bytes();
}

__global__ __launch_bounds__(256) void rev_keys_kernel(const int32_t* __restrict__ idx, uint32_t M, uint32_t N,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ n_word) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e == 0) *n_word = M;
  if (e >= M) return;
  const uint32_t t = (uint32_t)idx[e];
  keys[e] = t < N ? t : N;
}

__global__ __launch_bounds__(256) void rev_finish_kernel(const uint32_t* __restrict__ vals, const uint2* __restrict__ ranges,
                                                         uint32_t M, uint32_t N, int32_t* __restrict__ rev_edges,
                                                         int32_t* __restrict__ rev_ranges) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e < M) rev_edges[e] = (int32_t)vals[e];
  if (e < N) { const uint2 r = ranges[e]; rev_ranges[2 * (size_t)e] = (int32_t)r.x; rev_ranges[2 * (size_t)e + 1] = (int32_t)r.y; }
}

// ---- loss_reg_3d_feature ------------------------------------------------------------------------------------------------
//   loss = mean over (i, slot, d) of s_i (log(s_i + eps) - log(s_j + eps)),  s = sigmoid(f),  j = idx[i, slot]
constexpr float F3_EPS = 1e-10f;
constexpr int F3_MAX_D = 64;

__global__ __launch_bounds__(256) void f3_table_kernel(const float* __restrict__ f, uint32_t n, float* __restrict__ s_tab,
                                                       float* __restrict__ l_tab) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const float s = 1.0f / (1.0f + expf(-f[t]));
  s_tab[t] = s;
  l_tab[t] = logf(s + F3_EPS);
}

// A[i, d] = sum over the row's slots, in slot order, of (l[i, d] - l[j, d]); an edge to nowhere adds nothing
__device__ __forceinline__ float f3_row_sum(const float* __restrict__ l_tab, const int32_t* __restrict__ idx, uint32_t i, uint32_t d,
                                            uint32_t N, uint32_t D, uint32_t k) {
  const float li = l_tab[(size_t)i * D + d];
  float a = 0.f;
  for (uint32_t slot = 0; slot < k; ++slot) {
    const uint32_t j = (uint32_t)idx[(size_t)i * k + slot];
    if (j < N) a += li - l_tab[(size_t)j * D + d];
  }
  return a;
}

// sum of the 256 values of a block in one fixed order (a tree over LDS); valid in thread 0
__device__ __forceinline__ double block_sum_256(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < (unsigned)s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

// one thread per (i, d), d fastest: the gathered rows of l are read D contiguous floats at a time
__global__ __launch_bounds__(256) void f3_forward_kernel(const float* __restrict__ s_tab, const float* __restrict__ l_tab,
                                                         const int32_t* __restrict__ idx, uint32_t N, uint32_t D, uint32_t k,
                                                         double* __restrict__ partial) {
  __shared__ double sh[256];
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  float v = 0.f;
  if (t < N * D) {
    const uint32_t i = t / D, d = t - i * D;
    v = s_tab[t] * f3_row_sum(l_tab, idx, i, d, N, D, k);
  }
  const double tot = block_sum_256((double)v, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// second stage: one block, every thread a strided share in ascending order, then the tree; out = sum * scale
__global__ __launch_bounds__(256) void f3_reduce_kernel(const double* __restrict__ partial, uint32_t n, double scale,
                                                        float* __restrict__ out) {
  __shared__ double sh[256];
  double v = 0.0;
  for (uint32_t b = threadIdx.x; b < n; b += 256u) v += partial[b];
  const double tot = block_sum_256(v, sh);
  if (threadIdx.x == 0) *out = (float)(tot * scale);
}

// d loss / d f[i, d] = g c [ A + (k s - R) / (s + eps) ] s (1 - s),  c = 1 / (N k D),
// R[i, d] = sum over the edges that point at i, in ascending edge order, of s[source row, d]
__global__ __launch_bounds__(256) void f3_backward_kernel(const float* __restrict__ s_tab, const float* __restrict__ l_tab,
                                                          const int32_t* __restrict__ idx, const int32_t* __restrict__ rev_ranges,
                                                          const int32_t* __restrict__ rev_edges, uint32_t N, uint32_t D, uint32_t k,
                                                          const float* __restrict__ g_loss, float c, float* __restrict__ g_f) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= N * D) return;
  const uint32_t i = t / D, d = t - i * D;
  const float s = s_tab[t];
  const float a = f3_row_sum(l_tab, idx, i, d, N, D, k);
  uint32_t valid = 0;
  for (uint32_t slot = 0; slot < k; ++slot) valid += ((uint32_t)idx[(size_t)i * k + slot] < N) ? 1u : 0u;
  float r = 0.f;
  const uint32_t e0 = (uint32_t)rev_ranges[2 * (size_t)i], e1 = (uint32_t)rev_ranges[2 * (size_t)i + 1];
  for (uint32_t q = e0; q < e1; ++q) {
    const uint32_t src = (uint32_t)rev_edges[q] / k;
    r += s_tab[(size_t)src * D + d];
  }
  const float dl = ((float)valid * s - r) / (s + F3_EPS);
  g_f[t] = (*g_loss * c) * ((a + dl) * (s * (1.0f - s)));
}

// ---- edge ops of the rigid-motion loss -----------------------------------------------------------------------------------
//   e1 = p1[i] - p1[j], e2 = p2[i] - p2[j], j = idx[i, slot]
//   edge_moments:  S[i] = sum_slot e1 e2^T (3 x 3, row index from e1)
//   edge_residual: r[i] = sum_slot |e1 - R[i] e2|^2
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 ld3(const float* __restrict__ p, uint32_t i) { return {p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]}; }
__device__ __forceinline__ V3 sub3(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
struct M3 { float m[9]; };
__device__ __forceinline__ M3 ldm(const float* __restrict__ p, uint32_t i) {
  M3 r;
#pragma unroll
  for (int q = 0; q < 9; ++q) r.m[q] = p[9 * (size_t)i + q];
  return r;
}
__device__ __forceinline__ V3 mul_mv(const M3& a, V3 v) {       // a v
  return {a.m[0] * v.x + a.m[1] * v.y + a.m[2] * v.z, a.m[3] * v.x + a.m[4] * v.y + a.m[5] * v.z,
          a.m[6] * v.x + a.m[7] * v.y + a.m[8] * v.z};
}
__device__ __forceinline__ V3 mul_tv(const M3& a, V3 v) {       // a^T v
  return {a.m[0] * v.x + a.m[3] * v.y + a.m[6] * v.z, a.m[1] * v.x + a.m[4] * v.y + a.m[7] * v.z,
          a.m[2] * v.x + a.m[5] * v.y + a.m[8] * v.z};
}

__global__ __launch_bounds__(256) void edge_moments_fwd_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                               const int32_t* __restrict__ idx, uint32_t N, uint32_t k,
                                                               float* __restrict__ S) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  const V3 a1 = ld3(p1, i), a2 = ld3(p2, i);
  float s[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (uint32_t slot = 0; slot < k; ++slot) {
    const uint32_t j = (uint32_t)idx[(size_t)i * k + slot];
    if (j >= N) continue;
    const V3 e1 = sub3(a1, ld3(p1, j)), e2 = sub3(a2, ld3(p2, j));
    s[0] += e1.x * e2.x; s[1] += e1.x * e2.y; s[2] += e1.x * e2.z;
    s[3] += e1.y * e2.x; s[4] += e1.y * e2.y; s[5] += e1.y * e2.z;
    s[6] += e1.z * e2.x; s[7] += e1.z * e2.y; s[8] += e1.z * e2.z;
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) S[9 * (size_t)i + q] = s[q];
}

// g1[i] = sum_slot G_i e2 - sum_{edges at i} G_src e2,   g2[i] = sum_slot G_i^T e1 - sum_{edges at i} G_src^T e1
__global__ __launch_bounds__(256) void edge_moments_bwd_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                               const int32_t* __restrict__ idx, const int32_t* __restrict__ rev_ranges,
                                                               const int32_t* __restrict__ rev_edges, uint32_t N, uint32_t k,
                                                               const float* __restrict__ gS, float* __restrict__ g1,
                                                               float* __restrict__ g2) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  const V3 a1 = ld3(p1, i), a2 = ld3(p2, i);
  V3 s1 = {0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f};     // the sums of e1, e2 over the row's own edges: G_i is common to them
  for (uint32_t slot = 0; slot < k; ++slot) {
    const uint32_t j = (uint32_t)idx[(size_t)i * k + slot];
    if (j >= N) continue;
    const V3 e1 = sub3(a1, ld3(p1, j)), e2 = sub3(a2, ld3(p2, j));
    s1.x += e1.x; s1.y += e1.y; s1.z += e1.z;
    s2.x += e2.x; s2.y += e2.y; s2.z += e2.z;
  }
  const M3 G = ldm(gS, i);
  V3 o1 = mul_mv(G, s2), o2 = mul_tv(G, s1);
  const uint32_t q0 = (uint32_t)rev_ranges[2 * (size_t)i], q1 = (uint32_t)rev_ranges[2 * (size_t)i + 1];
  for (uint32_t q = q0; q < q1; ++q) {
    const uint32_t src = (uint32_t)rev_edges[q] / k;
    const V3 e1 = sub3(ld3(p1, src), a1), e2 = sub3(ld3(p2, src), a2);
    const M3 Gs = ldm(gS, src);
    const V3 u = mul_mv(Gs, e2), v = mul_tv(Gs, e1);
    o1.x -= u.x; o1.y -= u.y; o1.z -= u.z;
    o2.x -= v.x; o2.y -= v.y; o2.z -= v.z;
  }
  g1[3 * (size_t)i] = o1.x; g1[3 * (size_t)i + 1] = o1.y; g1[3 * (size_t)i + 2] = o1.z;
  g2[3 * (size_t)i] = o2.x; g2[3 * (size_t)i + 1] = o2.y; g2[3 * (size_t)i + 2] = o2.z;
}

__global__ __launch_bounds__(256) void edge_residual_fwd_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                                const int32_t* __restrict__ idx, const float* __restrict__ R,
                                                                uint32_t N, uint32_t k, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  const V3 a1 = ld3(p1, i), a2 = ld3(p2, i);
  const M3 Ri = ldm(R, i);
  float acc = 0.f;
  for (uint32_t slot = 0; slot < k; ++slot) {
    const uint32_t j = (uint32_t)idx[(size_t)i * k + slot];
    if (j >= N) continue;
    const V3 e1 = sub3(a1, ld3(p1, j)), e2 = sub3(a2, ld3(p2, j));
    const V3 v = sub3(e1, mul_mv(Ri, e2));
    acc += v.x * v.x + v.y * v.y + v.z * v.z;
  }
  out[i] = acc;
}

// with v = e1 - R e2 and the cotangent g of r:  d/de1 = 2 g v,  d/de2 = -2 g R^T v,  d/dR = -2 g sum v e2^T
__global__ __launch_bounds__(256) void edge_residual_bwd_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                                const int32_t* __restrict__ idx, const int32_t* __restrict__ rev_ranges,
                                                                const int32_t* __restrict__ rev_edges, const float* __restrict__ R,
                                                                uint32_t N, uint32_t k, const float* __restrict__ g,
                                                                float* __restrict__ g1, float* __restrict__ g2, float* __restrict__ gR) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  const V3 a1 = ld3(p1, i), a2 = ld3(p2, i);
  const M3 Ri = ldm(R, i);
  V3 sv = {0.f, 0.f, 0.f};
  float m[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (uint32_t slot = 0; slot < k; ++slot) {
    const uint32_t j = (uint32_t)idx[(size_t)i * k + slot];
    if (j >= N) continue;
    const V3 e1 = sub3(a1, ld3(p1, j)), e2 = sub3(a2, ld3(p2, j));
    const V3 v = sub3(e1, mul_mv(Ri, e2));
    sv.x += v.x; sv.y += v.y; sv.z += v.z;
    m[0] += v.x * e2.x; m[1] += v.x * e2.y; m[2] += v.x * e2.z;
    m[3] += v.y * e2.x; m[4] += v.y * e2.y; m[5] += v.y * e2.z;
    m[6] += v.z * e2.x; m[7] += v.z * e2.y; m[8] += v.z * e2.z;
  }
  const float gi = 2.0f * g[i];
  const V3 rt = mul_tv(Ri, sv);
  V3 o1 = {gi * sv.x, gi * sv.y, gi * sv.z}, o2 = {-gi * rt.x, -gi * rt.y, -gi * rt.z};
#pragma unroll
  for (int q = 0; q < 9; ++q) gR[9 * (size_t)i + q] = -gi * m[q];
  const uint32_t q0 = (uint32_t)rev_ranges[2 * (size_t)i], q1 = (uint32_t)rev_ranges[2 * (size_t)i + 1];
  for (uint32_t q = q0; q < q1; ++q) {
    const uint32_t src = (uint32_t)rev_edges[q] / k;
    const V3 e1 = sub3(ld3(p1, src), a1), e2 = sub3(ld3(p2, src), a2);
    const M3 Rs = ldm(R, src);
    const V3 v = sub3(e1, mul_mv(Rs, e2));
    const V3 w = mul_tv(Rs, v);
    const float gs = 2.0f * g[src];
    o1.x -= gs * v.x; o1.y -= gs * v.y; o1.z -= gs * v.z;
    o2.x += gs * w.x; o2.y += gs * w.y; o2.z += gs * w.z;
  }
  g1[3 * (size_t)i] = o1.x; g1[3 * (size_t)i + 1] = o1.y; g1[3 * (size_t)i + 2] = o1.z;
  g2[3 * (size_t)i] = o2.x; g2[3 * (size_t)i + 1] = o2.y; g2[3 * (size_t)i + 2] = o2.z;
}

// ---- the rotation of a moment matrix and the fused rigid fit (rigid_math.h) -------------------------------------------------
//   polar3:     R[i] = V U^T of S[i] = U Sigma V^T, and gS for a cotangent of R, one matrix per thread
//   rigid_fit:  r[i] = sum_slot |e1 - R_i e2|^2 with R_i = polar3(S_i), S_i = sum_slot e1 e2^T, in one launch; the backward is one
//               launch too.  With v = e1 - R e2, T = sum_slot v e2^T and Z = polar3_bwd(S, R, -2 T) (so d r / d S = Z):
//                   d r / d e1 = 2 v + Z e2,      d r / d e2 = -2 R^T v + Z^T e1
//               The forward keeps, per row, Z and the two sums of these over the row's own edges (RIGID_STATE floats); the
//               backward scales them by g_i and gathers the incoming edges with R_src, Z_src and -g_src.
__global__ __launch_bounds__(256) void polar3_fwd_kernel(const float* __restrict__ S, uint32_t N, float* __restrict__ R) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  const M3 s = ldm(S, i);
  M3 r;
  polar3(s.m, r.m);
#pragma unroll
  for (int q = 0; q < 9; ++q) R[9 * (size_t)i + q] = r.m[q];
}

__global__ __launch_bounds__(256) void polar3_bwd_kernel(const float* __restrict__ S, const float* __restrict__ R,
                                                         const float* __restrict__ gR, uint32_t N, float* __restrict__ gS) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  const M3 s = ldm(S, i), r = ldm(R, i), g = ldm(gR, i);
  M3 o;
  polar3_row_bwd(s.m, r.m, g.m, o.m);
#pragma unroll
  for (int q = 0; q < 9; ++q) gS[9 * (size_t)i + q] = o.m[q];
}

constexpr int RIGID_STATE = TRASE_RIGID_STATE_FLOATS;      // Z (9), d r / d p1[i] and d r / d p2[i] over the own edges (3 + 3), 1 unused

__global__ __launch_bounds__(256) void rigid_fit_fwd_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                            const int32_t* __restrict__ idx, uint32_t N, uint32_t k,
                                                            float* __restrict__ out, float* __restrict__ R, float* __restrict__ state) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  const V3 a1 = ld3(p1, i), a2 = ld3(p2, i);
  // the first walk: edge_moments_fwd_kernel's statements in its order, and the edge scale of the degenerate rule beside them
  float s[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float scale = 0.f;
  for (uint32_t slot = 0; slot < k; ++slot) {
    const uint32_t j = (uint32_t)idx[(size_t)i * k + slot];
    if (j >= N) continue;
    const V3 e1 = sub3(a1, ld3(p1, j)), e2 = sub3(a2, ld3(p2, j));
    s[0] += e1.x * e2.x; s[1] += e1.x * e2.y; s[2] += e1.x * e2.z;
    s[3] += e1.y * e2.x; s[4] += e1.y * e2.y; s[5] += e1.y * e2.z;
    s[6] += e1.z * e2.x; s[7] += e1.z * e2.y; s[8] += e1.z * e2.z;
    scale += sqrtf(e1.x * e1.x + e1.y * e1.y + e1.z * e1.z) * sqrtf(e2.x * e2.x + e2.y * e2.y + e2.z * e2.z);
  }
  M3 Ri;
  const double s23 = polar3(s, Ri.m);
  const bool degenerate = polar3_is_degenerate(s23, (double)k, (double)scale);
  // the second walk (the edges are in L2 by now): edge_residual_fwd_kernel's statements, and the sums of the backward
  float acc = 0.f;
  V3 sv = {0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f};
  float t[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (uint32_t slot = 0; slot < k; ++slot) {
    const uint32_t j = (uint32_t)idx[(size_t)i * k + slot];
    if (j >= N) continue;
    const V3 e1 = sub3(a1, ld3(p1, j)), e2 = sub3(a2, ld3(p2, j));
    const V3 v = sub3(e1, mul_mv(Ri, e2));
    acc += v.x * v.x + v.y * v.y + v.z * v.z;
    sv.x += v.x; sv.y += v.y; sv.z += v.z;
    s1.x += e1.x; s1.y += e1.y; s1.z += e1.z;
    s2.x += e2.x; s2.y += e2.y; s2.z += e2.z;
    t[0] += v.x * e2.x; t[1] += v.x * e2.y; t[2] += v.x * e2.z;
    t[3] += v.y * e2.x; t[4] += v.y * e2.y; t[5] += v.y * e2.z;
    t[6] += v.z * e2.x; t[7] += v.z * e2.y; t[8] += v.z * e2.z;
  }
  M3 Z;
  if (degenerate) {
#pragma unroll
    for (int q = 0; q < 9; ++q) Z.m[q] = 0.f;
  } else {
    float G[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) G[q] = -2.0f * t[q];
    polar3_bwd(s, Ri.m, G, Z.m);
  }
  const V3 ze = mul_mv(Z, s2), zt = mul_tv(Z, s1), rt = mul_tv(Ri, sv);
  out[i] = acc;
  float* st = state + (size_t)RIGID_STATE * i;
#pragma unroll
  for (int q = 0; q < 9; ++q) { R[9 * (size_t)i + q] = Ri.m[q]; st[q] = Z.m[q]; }
  st[9] = 2.0f * sv.x + ze.x; st[10] = 2.0f * sv.y + ze.y; st[11] = 2.0f * sv.z + ze.z;
  st[12] = zt.x - 2.0f * rt.x; st[13] = zt.y - 2.0f * rt.y; st[14] = zt.z - 2.0f * rt.z;
  st[15] = 0.f;
}

__global__ __launch_bounds__(256) void rigid_fit_bwd_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                            const int32_t* __restrict__ rev_ranges, const int32_t* __restrict__ rev_edges,
                                                            const float* __restrict__ R, const float* __restrict__ state,
                                                            const float* __restrict__ g, uint32_t N, uint32_t k,
                                                            float* __restrict__ g1, float* __restrict__ g2) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  const V3 a1 = ld3(p1, i), a2 = ld3(p2, i);
  const float* st = state + (size_t)RIGID_STATE * i;
  const float gi = g[i];
  V3 o1 = {gi * st[9], gi * st[10], gi * st[11]}, o2 = {gi * st[12], gi * st[13], gi * st[14]};
  const uint32_t q0 = (uint32_t)rev_ranges[2 * (size_t)i], q1 = (uint32_t)rev_ranges[2 * (size_t)i + 1];
  for (uint32_t q = q0; q < q1; ++q) {
    const uint32_t src = (uint32_t)rev_edges[q] / k;
    const V3 e1 = sub3(ld3(p1, src), a1), e2 = sub3(ld3(p2, src), a2);
    const M3 Rs = ldm(R, src);
    M3 Zs;
#pragma unroll
    for (int c = 0; c < 9; ++c) Zs.m[c] = state[(size_t)RIGID_STATE * src + c];
    const V3 v = sub3(e1, mul_mv(Rs, e2));
    const V3 w = mul_tv(Rs, v), ze = mul_mv(Zs, e2), zt = mul_tv(Zs, e1);
    const float gs = g[src];
    o1.x -= gs * (2.0f * v.x + ze.x); o1.y -= gs * (2.0f * v.y + ze.y); o1.z -= gs * (2.0f * v.z + ze.z);
    o2.x -= gs * (zt.x - 2.0f * w.x); o2.y -= gs * (zt.y - 2.0f * w.y); o2.z -= gs * (zt.z - 2.0f * w.z);
  }
  g1[3 * (size_t)i] = o1.x; g1[3 * (size_t)i + 1] = o1.y; g1[3 * (size_t)i + 2] = o1.z;
  g2[3 * (size_t)i] = o2.x; g2[3 * (size_t)i + 1] = o2.y; g2[3 * (size_t)i + 2] = o2.z;
}

// ---- loss_feature3d (utils/loss_utils.py:154-175) ------------------------------------------------------------------------------
//   loss = lambda_p mean over (i, slot < kp) of sigmoid(1 - c) + lambda_n mean over (i, slot >= kp) of sigmoid(c),
//   c = u_i . u_j, u = f / max(|f|, 1e-8), j = idx[i, slot]: idx (rows, kp + kn) holds the kp nearest rows, then the kn farthest.
// The table pass writes u zero padded to DP = 8 / 16 / 32 / 64 columns (float4 reads, no tail) and the clamped norms; forward
// and backward are one thread per row with u_i in registers.  The backward accumulates g_u[i] = sum over the row's own slots of
// w_e u_j + sum over the edges that point at i, in ascending edge order, of w_e u_src with w_e = d loss / d c_e (the dot product
// is recomputed there), then applies the chain of the normalisation.
constexpr float FC_EPS = 1e-8f;
constexpr int FC_MAX_K = 32;
static inline int fc_dpad(int D) { return D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64; }
__device__ __forceinline__ float fc_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(256) void fc_table_kernel(const float* __restrict__ f, uint32_t rows, uint32_t D, uint32_t DP,
                                                       float* __restrict__ u_tab, float* __restrict__ nrm) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= rows) return;
  const float* fi = f + (size_t)i * D;
  float n2 = 0.f;
  for (uint32_t d = 0; d < D; ++d) n2 = fmaf(fi[d], fi[d], n2);
  const float n = fmaxf(sqrtf(n2), FC_EPS);
  nrm[i] = n;
  for (uint32_t d = 0; d < DP; ++d) u_tab[(size_t)i * DP + d] = d < D ? fi[d] / n : 0.f;
}

template <int DP>
__device__ __forceinline__ void fc_load(const float* __restrict__ u_tab, uint32_t i, float (&u)[DP]) {
  const float4* p = reinterpret_cast<const float4*>(u_tab + (size_t)i * DP);
#pragma unroll
  for (int q = 0; q < DP / 4; ++q) { const float4 v = p[q]; u[4 * q] = v.x; u[4 * q + 1] = v.y; u[4 * q + 2] = v.z; u[4 * q + 3] = v.w; }
}
template <int DP>
__device__ __forceinline__ float fc_dot(const float (&u)[DP], const float* __restrict__ u_tab, uint32_t j) {
  const float4* p = reinterpret_cast<const float4*>(u_tab + (size_t)j * DP);
  float c = 0.f;
#pragma unroll
  for (int q = 0; q < DP / 4; ++q) {
    const float4 v = p[q];
    c = fmaf(u[4 * q], v.x, c); c = fmaf(u[4 * q + 1], v.y, c); c = fmaf(u[4 * q + 2], v.z, c); c = fmaf(u[4 * q + 3], v.w, c);
  }
  return c;
}
template <int DP>
__device__ __forceinline__ void fc_axpy(float w, const float* __restrict__ u_tab, uint32_t j, float (&g)[DP]) {
  const float4* p = reinterpret_cast<const float4*>(u_tab + (size_t)j * DP);
#pragma unroll
  for (int q = 0; q < DP / 4; ++q) {
    const float4 v = p[q];
    g[4 * q] = fmaf(w, v.x, g[4 * q]); g[4 * q + 1] = fmaf(w, v.y, g[4 * q + 1]);
    g[4 * q + 2] = fmaf(w, v.z, g[4 * q + 2]); g[4 * q + 3] = fmaf(w, v.w, g[4 * q + 3]);
  }
}
// d loss / d c of one edge: a near edge is sigmoid(1 - c) * wp, a far edge sigmoid(c) * wn
__device__ __forceinline__ float fc_weight(float c, bool near_edge, float wp, float wn) {
  const float s = fc_sigmoid(near_edge ? 1.0f - c : c);
  return (near_edge ? -wp : wn) * (s * (1.0f - s));
}

template <int DP>
__global__ __launch_bounds__(256) void fc_forward_kernel(const float* __restrict__ u_tab, const int32_t* __restrict__ idx, uint32_t rows,
                                                         uint32_t kp, uint32_t kn, double wp, double wn, double* __restrict__ partial) {
  __shared__ double sh[256];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, kt = kp + kn;
  double v = 0.0;
  if (i < rows) {
    float u[DP];
    fc_load<DP>(u_tab, i, u);
    float a = 0.f, b = 0.f;
    for (uint32_t slot = 0; slot < kt; ++slot) {
      const uint32_t j = (uint32_t)idx[(size_t)i * kt + slot];
      if (j >= rows) continue;
      const float c = fc_dot<DP>(u, u_tab, j);
      if (slot < kp) a += fc_sigmoid(1.0f - c); else b += fc_sigmoid(c);
    }
    v = wp * (double)a + wn * (double)b;
  }
  const double tot = block_sum_256(v, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <int DP>
__global__ __launch_bounds__(256) void fc_backward_kernel(const float* __restrict__ u_tab, const float* __restrict__ nrm,
                                                          const int32_t* __restrict__ idx, const int32_t* __restrict__ rev_ranges,
                                                          const int32_t* __restrict__ rev_edges, uint32_t rows, uint32_t D, uint32_t kp,
                                                          uint32_t kn, float wp, float wn, const float* __restrict__ g_loss,
                                                          float* __restrict__ g_f) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, kt = kp + kn;
  if (i >= rows) return;
  float u[DP], g[DP];
  fc_load<DP>(u_tab, i, u);
#pragma unroll
  for (int d = 0; d < DP; ++d) g[d] = 0.f;
  for (uint32_t slot = 0; slot < kt; ++slot) {
    const uint32_t j = (uint32_t)idx[(size_t)i * kt + slot];
    if (j >= rows) continue;
    fc_axpy<DP>(fc_weight(fc_dot<DP>(u, u_tab, j), slot < kp, wp, wn), u_tab, j, g);
  }
  const uint32_t e0 = (uint32_t)rev_ranges[2 * (size_t)i], e1 = (uint32_t)rev_ranges[2 * (size_t)i + 1];
  for (uint32_t q = e0; q < e1; ++q) {
    const uint32_t e = (uint32_t)rev_edges[q], src = e / kt, slot = e - src * kt;
    fc_axpy<DP>(fc_weight(fc_dot<DP>(u, u_tab, src), slot < kp, wp, wn), u_tab, src, g);
  }
  float ug = 0.f;
#pragma unroll
  for (int d = 0; d < DP; ++d) ug = fmaf(u[d], g[d], ug);
  const float n = nrm[i], gl = *g_loss;
  const bool clamped = !(n > FC_EPS);
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if ((uint32_t)d < D) g_f[(size_t)i * D + d] = gl * (clamped ? g[d] / FC_EPS : (g[d] - u[d] * ug) / n);
}

// ---- loss_cls_3d (utils/loss_utils.py:89-130) -----------------------------------------------------------------------------------
//   loss = lambda / (S k C) sum over (s, slot, c) of p_s (log(p_s + 1e-10) - log(p_j + 1e-10)), p_s = pred[sample[s]],
//   j = idx[s, slot] the k nearest rows of sample[s] in feature space.  The gradient goes to pred (N, C): a sampled row gets its
//   direct term (found through the transpose of `sample` as an (S, 1) graph, so a row sampled twice sums in a fixed order),
//   every neighbour row -w p_s / (p_j + 1e-10) gathered over the transpose of idx.
constexpr int CL_MAX_C = 256;
__global__ __launch_bounds__(256) void cls_forward_kernel(const float* __restrict__ pred, const int32_t* __restrict__ sample,
                                                          const int32_t* __restrict__ idx, uint32_t S, uint32_t N, uint32_t C, uint32_t k,
                                                          double* __restrict__ partial) {
  __shared__ double sh[256];
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  float v = 0.f;
  if (t < S * C) {
    const uint32_t s = t / C, c = t - s * C, r = (uint32_t)sample[s];
    if (r < N) {
      const float p = pred[(size_t)r * C + c], lp = logf(p + F3_EPS);
      float a = 0.f;
      for (uint32_t slot = 0; slot < k; ++slot) {
        const uint32_t j = (uint32_t)idx[(size_t)s * k + slot];
        if (j < N) a += lp - logf(pred[(size_t)j * C + c] + F3_EPS);
      }
      v = p * a;
    }
  }
  const double tot = block_sum_256((double)v, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void cls_backward_kernel(const float* __restrict__ pred, const int32_t* __restrict__ sample,
                                                           const int32_t* __restrict__ idx, const int32_t* __restrict__ rev_ranges,
                                                           const int32_t* __restrict__ rev_edges, const int32_t* __restrict__ srev_ranges,
                                                           const int32_t* __restrict__ srev_edges, uint32_t N, uint32_t C, uint32_t k,
                                                           const float* __restrict__ g_loss, float w, float* __restrict__ g_pred) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= N * C) return;
  const uint32_t n = t / C, c = t - n * C;
  const float p = pred[t];
  float g = 0.f;
  const uint32_t s0 = (uint32_t)srev_ranges[2 * (size_t)n], s1 = (uint32_t)srev_ranges[2 * (size_t)n + 1];
  if (s0 < s1) {
    const float lp = logf(p + F3_EPS), self = p / (p + F3_EPS);
    for (uint32_t q = s0; q < s1; ++q) {
      const uint32_t s = (uint32_t)srev_edges[q];
      for (uint32_t slot = 0; slot < k; ++slot) {
        const uint32_t j = (uint32_t)idx[(size_t)s * k + slot];
        if (j < N) g += (lp - logf(pred[(size_t)j * C + c] + F3_EPS)) + self;
      }
    }
  }
  const uint32_t e0 = (uint32_t)rev_ranges[2 * (size_t)n], e1 = (uint32_t)rev_ranges[2 * (size_t)n + 1];
  for (uint32_t q = e0; q < e1; ++q) {
    const uint32_t r = (uint32_t)sample[(uint32_t)rev_edges[q] / k];
    if (r < N) g -= pred[(size_t)r * C + c] / (p + F3_EPS);
  }
  g_pred[t] = (*g_loss * w) * g;
}

// the size rules every entry point shares: N >= 0, 1 <= k, N * k < 2^31
static int graph_dims_ok(const char* who, int32_t N, int32_t k) {
  if (N < 0 || k < 1 || (int64_t)N * (int64_t)k >= ((int64_t)1 << 31)) {
    set_error("%s: need N >= 0, k >= 1 and N * k < 2^31 (got N %d, k %d)", who, N, k);
    return TRASE_ERR_INVALID;
  }
  return TRASE_OK;
}
static inline int blocks_of(uint32_t n) { return (int)((n + 255u) / 256u); }
static int graph_to_dims_ok(const char* who, int32_t rows, int32_t k, int32_t targets) {
  if (int rc = graph_dims_ok(who, rows, k)) return rc;
  if (rows < 1 || targets < 1 || targets == INT32_MAX) {
    set_error("%s: need rows >= 1 and 1 <= targets < 2^31 - 1 (got rows %d, targets %d)", who, rows, targets);
    return TRASE_ERR_INVALID;
  }
  return TRASE_OK;
}

// the transpose of idx (rows, k) over `targets` target rows (arguments checked by the caller): the stable radix sort of the
// edges by target, the ranges of every target, then rev_edges (rows * k) and rev_ranges (targets, 2)
static int graph_reverse(const char* who, const int32_t* idx, int32_t rows, int32_t k, int32_t targets, int32_t* rev_ranges,
                         int32_t* rev_edges, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  RevWs w;
  if (!ws || ws_bytes < rev_layout(nullptr, rows, k, targets, w)) { set_error("%s: workspace too small", who); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  rev_layout(ws, rows, k, targets, w);
  LaunchCtx c{stream, 0, 0};
  const uint32_t M = (uint32_t)rows * (uint32_t)k, T = (uint32_t)targets;
  TRASE_LAUNCH("graph_rev_keys", stream, 0, rev_keys_kernel, dim3(blocks_of(M)), dim3(256), 0, idx, M, T, w.sort.keys[0], w.n);
  int out = 0;
  int rc = radix_sort_pairs(c, w.sort, w.n, M, 0, rev_bits(targets), true, &out);
  if (rc) return rc;
  rc = launch_tile_ranges(c, w.sort.keys[out], w.n, M, w.ranges, targets + 1);
  if (rc) return rc;
  TRASE_LAUNCH("graph_rev_finish", stream, 0, rev_finish_kernel, dim3(blocks_of(M > T ? M : T)), dim3(256), 0, w.sort.vals[out], w.ranges, M,
               T, rev_edges, rev_ranges);
  return TRASE_OK;
}

}  // namespace trase

using namespace trase;

extern "C" {

int trase_graph_reverse_ws_bytes(int32_t N, int32_t k, size_t* ws_bytes) {
  if (!ws_bytes) { set_error("trase_graph_reverse_ws_bytes: null pointer"); return TRASE_ERR_INVALID; }
  if (int rc = graph_dims_ok("trase_graph_reverse_ws_bytes", N, k)) return rc;
  RevWs w;
  *ws_bytes = rev_layout(nullptr, N, k, N, w);
  return TRASE_OK;
}

int trase_graph_reverse(const int32_t* idx, int32_t N, int32_t k, int32_t* rev_ranges, int32_t* rev_edges, void* ws,
                        size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  if (int rc = graph_dims_ok("trase_graph_reverse", N, k)) return rc;
  if (N == 0) return TRASE_OK;
  if (!idx || !rev_ranges || !rev_edges) { set_error("trase_graph_reverse: null pointer"); return TRASE_ERR_INVALID; }
  return graph_reverse("trase_graph_reverse", idx, N, k, N, rev_ranges, rev_edges, ws, ws_bytes, device, stream_);
}

int trase_graph_reverse_to_ws_bytes(int32_t rows, int32_t k, int32_t targets, size_t* ws_bytes) {
  if (!ws_bytes) { set_error("trase_graph_reverse_to_ws_bytes: null pointer"); return TRASE_ERR_INVALID; }
  if (int rc = graph_to_dims_ok("trase_graph_reverse_to_ws_bytes", rows, k, targets)) return rc;
  RevWs w;
  *ws_bytes = rev_layout(nullptr, rows, k, targets, w);
  return TRASE_OK;
}

int trase_graph_reverse_to(const int32_t* idx, int32_t rows, int32_t k, int32_t targets, int32_t* rev_ranges, int32_t* rev_edges,
                           void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  if (int rc = graph_to_dims_ok("trase_graph_reverse_to", rows, k, targets)) return rc;
  if (!idx || !rev_ranges || !rev_edges) { set_error("trase_graph_reverse_to: null pointer"); return TRASE_ERR_INVALID; }
  return graph_reverse("trase_graph_reverse_to", idx, rows, k, targets, rev_ranges, rev_edges, ws, ws_bytes, device, stream_);
}

static int f3_dims_ok(const char* who, int32_t N, int32_t D, int32_t k) {
  if (int rc = graph_dims_ok(who, N, k)) return rc;
  if (D < 1 || D > F3_MAX_D || (int64_t)N * (int64_t)D >= ((int64_t)1 << 31)) {
    set_error("%s: need 1 <= D <= %d and N * D < 2^31 (got N %d, D %d)", who, F3_MAX_D, N, D);
    return TRASE_ERR_INVALID;
  }
  return TRASE_OK;
}

int trase_feat3d_ws_bytes(int32_t N, int32_t D, size_t* ws_bytes) {
  if (!ws_bytes) { set_error("trase_feat3d_ws_bytes: null pointer"); return TRASE_ERR_INVALID; }
  if (int rc = f3_dims_ok("trase_feat3d_ws_bytes", N, D, 1)) return rc;
  double* p;
  *ws_bytes = array_layout<double>(nullptr, (size_t)blocks_of((uint32_t)N * (uint32_t)D) + 1, p);
  return TRASE_OK;
}

int trase_feat3d_forward(const float* feats, const int32_t* idx, int32_t N, int32_t D, int32_t k, float* s_tab, float* l_tab,
                         float* loss, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  if (int rc = f3_dims_ok("trase_feat3d_forward", N, D, k)) return rc;
  if (N < 1) { set_error("trase_feat3d_forward: need N >= 1 (the mean of nothing)"); return TRASE_ERR_INVALID; }
  if (!feats || !idx || !s_tab || !l_tab || !loss) { set_error("trase_feat3d_forward: null pointer"); return TRASE_ERR_INVALID; }
  const uint32_t ND = (uint32_t)N * (uint32_t)D;
  double* partial;
  if (!ws || ws_bytes < array_layout<double>(nullptr, (size_t)blocks_of(ND) + 1, partial)) {
    set_error("trase_feat3d_forward: workspace too small"); return TRASE_ERR_WORKSPACE;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  array_layout<double>(ws, (size_t)blocks_of(ND) + 1, partial);
  TRASE_LAUNCHES("feat3d_forward", stream, 0,
    hipLaunchKernelGGL(f3_table_kernel, dim3(blocks_of(ND)), dim3(256), 0, stream, feats, ND, s_tab, l_tab);
    hipLaunchKernelGGL(f3_forward_kernel, dim3(blocks_of(ND)), dim3(256), 0, stream, s_tab, l_tab, idx, (uint32_t)N, (uint32_t)D,
                       (uint32_t)k, partial);
    hipLaunchKernelGGL(f3_reduce_kernel, dim3(1), dim3(256), 0, stream, partial, (uint32_t)blocks_of(ND),
                       1.0 / ((double)N * (double)k * (double)D), loss));
  return TRASE_OK;
}

int trase_feat3d_backward(const float* s_tab, const float* l_tab, const int32_t* idx, const int32_t* rev_ranges,
                          const int32_t* rev_edges, int32_t N, int32_t D, int32_t k, const float* g_loss, float* g_feats,
                          int32_t device, trase_stream_t stream_) {
  if (int rc = f3_dims_ok("trase_feat3d_backward", N, D, k)) return rc;
  if (N == 0) return TRASE_OK;
  if (!s_tab || !l_tab || !idx || !rev_ranges || !rev_edges || !g_loss || !g_feats) {
    set_error("trase_feat3d_backward: null pointer"); return TRASE_ERR_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const uint32_t ND = (uint32_t)N * (uint32_t)D;
  TRASE_LAUNCH("feat3d_backward", stream, 0, f3_backward_kernel, dim3(blocks_of(ND)), dim3(256), 0, s_tab, l_tab, idx, rev_ranges, rev_edges,
               (uint32_t)N, (uint32_t)D, (uint32_t)k, g_loss, (float)(1.0 / ((double)N * (double)k * (double)D)), g_feats);
  return TRASE_OK;
}

int trase_edge_moments_forward(const float* p1, const float* p2, const int32_t* idx, int32_t N, int32_t k, float* S,
                               int32_t device, trase_stream_t stream_) {
  if (int rc = graph_dims_ok("trase_edge_moments_forward", N, k)) return rc;
  if (N == 0) return TRASE_OK;
  if (!p1 || !p2 || !idx || !S) { set_error("trase_edge_moments_forward: null pointer"); return TRASE_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCH("edge_moments_fwd", stream, 0, edge_moments_fwd_kernel, dim3(blocks_of((uint32_t)N)), dim3(256), 0, p1, p2, idx, (uint32_t)N,
               (uint32_t)k, S);
  return TRASE_OK;
}

int trase_edge_moments_backward(const float* p1, const float* p2, const int32_t* idx, const int32_t* rev_ranges,
                                const int32_t* rev_edges, int32_t N, int32_t k, const float* gS, float* g1, float* g2,
                                int32_t device, trase_stream_t stream_) {
  if (int rc = graph_dims_ok("trase_edge_moments_backward", N, k)) return rc;
  if (N == 0) return TRASE_OK;
  if (!p1 || !p2 || !idx || !rev_ranges || !rev_edges || !gS || !g1 || !g2) {
    set_error("trase_edge_moments_backward: null pointer"); return TRASE_ERR_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCH("edge_moments_bwd", stream, 0, edge_moments_bwd_kernel, dim3(blocks_of((uint32_t)N)), dim3(256), 0, p1, p2, idx, rev_ranges,
               rev_edges, (uint32_t)N, (uint32_t)k, gS, g1, g2);
  return TRASE_OK;
}

int trase_edge_residual_forward(const float* p1, const float* p2, const int32_t* idx, const float* R, int32_t N, int32_t k,
                                float* out, int32_t device, trase_stream_t stream_) {
  if (int rc = graph_dims_ok("trase_edge_residual_forward", N, k)) return rc;
  if (N == 0) return TRASE_OK;
  if (!p1 || !p2 || !idx || !R || !out) { set_error("trase_edge_residual_forward: null pointer"); return TRASE_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCH("edge_residual_fwd", stream, 0, edge_residual_fwd_kernel, dim3(blocks_of((uint32_t)N)), dim3(256), 0, p1, p2, idx, R, (uint32_t)N,
               (uint32_t)k, out);
  return TRASE_OK;
}

int trase_edge_residual_backward(const float* p1, const float* p2, const int32_t* idx, const int32_t* rev_ranges,
                                 const int32_t* rev_edges, const float* R, int32_t N, int32_t k, const float* g, float* g1,
                                 float* g2, float* gR, int32_t device, trase_stream_t stream_) {
  if (int rc = graph_dims_ok("trase_edge_residual_backward", N, k)) return rc;
  if (N == 0) return TRASE_OK;
  if (!p1 || !p2 || !idx || !rev_ranges || !rev_edges || !R || !g || !g1 || !g2 || !gR) {
    set_error("trase_edge_residual_backward: null pointer"); return TRASE_ERR_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCH("edge_residual_bwd", stream, 0, edge_residual_bwd_kernel, dim3(blocks_of((uint32_t)N)), dim3(256), 0, p1, p2, idx, rev_ranges,
               rev_edges, R, (uint32_t)N, (uint32_t)k, g, g1, g2, gR);
  return TRASE_OK;
}

int trase_polar3_forward(const float* S, int32_t N, float* R, int32_t device, trase_stream_t stream_) {
  if (N < 0) { set_error("trase_polar3_forward: need N >= 0 (got %d)", N); return TRASE_ERR_INVALID; }
  if (N == 0) return TRASE_OK;
  if (!S || !R) { set_error("trase_polar3_forward: null pointer"); return TRASE_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCH("polar3_fwd", stream, 0, polar3_fwd_kernel, dim3(blocks_of((uint32_t)N)), dim3(256), 0, S, (uint32_t)N, R);
  return TRASE_OK;
}

int trase_polar3_backward(const float* S, const float* R, const float* gR, int32_t N, float* gS, int32_t device,
                          trase_stream_t stream_) {
  if (N < 0) { set_error("trase_polar3_backward: need N >= 0 (got %d)", N); return TRASE_ERR_INVALID; }
  if (N == 0) return TRASE_OK;
  if (!S || !R || !gR || !gS) { set_error("trase_polar3_backward: null pointer"); return TRASE_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCH("polar3_bwd", stream, 0, polar3_bwd_kernel, dim3(blocks_of((uint32_t)N)), dim3(256), 0, S, R, gR, (uint32_t)N, gS);
  return TRASE_OK;
}

int trase_rigid_fit_forward(const float* p1, const float* p2, const int32_t* idx, int32_t N, int32_t k, float* out, float* R,
                            float* state, int32_t device, trase_stream_t stream_) {
  if (int rc = graph_dims_ok("trase_rigid_fit_forward", N, k)) return rc;
  if (N == 0) return TRASE_OK;
  if (!p1 || !p2 || !idx || !out || !R || !state) { set_error("trase_rigid_fit_forward: null pointer"); return TRASE_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCH("rigid_fit_fwd", stream, 0, rigid_fit_fwd_kernel, dim3(blocks_of((uint32_t)N)), dim3(256), 0, p1, p2, idx, (uint32_t)N,
               (uint32_t)k, out, R, state);
  return TRASE_OK;
}

int trase_rigid_fit_backward(const float* p1, const float* p2, const int32_t* idx, const int32_t* rev_ranges,
                             const int32_t* rev_edges, const float* R, const float* state, const float* g, int32_t N, int32_t k,
                             float* g1, float* g2, int32_t device, trase_stream_t stream_) {
  if (int rc = graph_dims_ok("trase_rigid_fit_backward", N, k)) return rc;
  if (N == 0) return TRASE_OK;
  if (!p1 || !p2 || !idx || !rev_ranges || !rev_edges || !R || !state || !g || !g1 || !g2) {
    set_error("trase_rigid_fit_backward: null pointer"); return TRASE_ERR_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  // (the row's own edges come from the saved sums: idx is not walked)
  TRASE_LAUNCH("rigid_fit_bwd", stream, 0, rigid_fit_bwd_kernel, dim3(blocks_of((uint32_t)N)), dim3(256), 0, p1, p2, rev_ranges, rev_edges, R,
               state, g, (uint32_t)N, (uint32_t)k, g1, g2);
  return TRASE_OK;
}

static int fc_dims_ok(const char* who, int32_t rows, int32_t D, int32_t kp, int32_t kn) {
  if (rows < 1 || D < 1 || D > F3_MAX_D || kp < 1 || kp > FC_MAX_K || kn < 1 || kn > FC_MAX_K || rows > (INT32_MAX >> 6)) {
    set_error("%s: need 1 <= rows < 2^25, 1 <= D <= %d, 1 <= kp, kn <= %d (got rows %d, D %d, kp %d, kn %d)", who, F3_MAX_D, FC_MAX_K,
              rows, D, kp, kn);
    return TRASE_ERR_INVALID;
  }
  return TRASE_OK;
}

int trase_feature3d_ws_bytes(int32_t rows, size_t* ws_bytes) {
  if (!ws_bytes) { set_error("trase_feature3d_ws_bytes: null pointer"); return TRASE_ERR_INVALID; }
  if (int rc = fc_dims_ok("trase_feature3d_ws_bytes", rows, 1, 1, 1)) return rc;
  double* p;
  *ws_bytes = array_layout<double>(nullptr, (size_t)blocks_of((uint32_t)rows) + 1, p);
  return TRASE_OK;
}

int trase_feature3d_forward(const float* feats, const int32_t* idx, int32_t rows, int32_t D, int32_t kp, int32_t kn, float lambda_p,
                            float lambda_n, float* u_tab, float* nrm, float* loss, void* ws, size_t ws_bytes, int32_t device,
                            trase_stream_t stream_) {
  if (int rc = fc_dims_ok("trase_feature3d_forward", rows, D, kp, kn)) return rc;
  if (!feats || !idx || !u_tab || !nrm || !loss) { set_error("trase_feature3d_forward: null pointer"); return TRASE_ERR_INVALID; }
  const int nb = blocks_of((uint32_t)rows), dp = fc_dpad(D);
  double* partial;
  if (!ws || ws_bytes < array_layout<double>(nullptr, (size_t)nb + 1, partial)) {
    set_error("trase_feature3d_forward: workspace too small"); return TRASE_ERR_WORKSPACE;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  array_layout<double>(ws, (size_t)nb + 1, partial);
  const double wp = (double)lambda_p / ((double)rows * kp), wn = (double)lambda_n / ((double)rows * kn);
#define TRASE_FC_FWD(DPV) hipLaunchKernelGGL((fc_forward_kernel<DPV>), dim3(nb), dim3(256), 0, stream, u_tab, idx, (uint32_t)rows, \
                                             (uint32_t)kp, (uint32_t)kn, wp, wn, partial)
  TRASE_LAUNCHES("feature3d_forward", stream, 0,
    hipLaunchKernelGGL(fc_table_kernel, dim3(nb), dim3(256), 0, stream, feats, (uint32_t)rows, (uint32_t)D, (uint32_t)dp, u_tab, nrm);
    if (dp == 8) TRASE_FC_FWD(8);
    else if (dp == 16) TRASE_FC_FWD(16);
    else if (dp == 32) TRASE_FC_FWD(32);
    else TRASE_FC_FWD(64);
    hipLaunchKernelGGL(f3_reduce_kernel, dim3(1), dim3(256), 0, stream, partial, (uint32_t)nb, 1.0, loss));
#undef TRASE_FC_FWD
  return TRASE_OK;
}

int trase_feature3d_backward(const float* u_tab, const float* nrm, const int32_t* idx, const int32_t* rev_ranges,
                             const int32_t* rev_edges, int32_t rows, int32_t D, int32_t kp, int32_t kn, float lambda_p, float lambda_n,
                             const float* g_loss, float* g_feats, int32_t device, trase_stream_t stream_) {
  if (int rc = fc_dims_ok("trase_feature3d_backward", rows, D, kp, kn)) return rc;
  if (!u_tab || !nrm || !idx || !rev_ranges || !rev_edges || !g_loss || !g_feats) {
    set_error("trase_feature3d_backward: null pointer"); return TRASE_ERR_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const int nb = blocks_of((uint32_t)rows), dp = fc_dpad(D);
  const float wp = (float)((double)lambda_p / ((double)rows * kp)), wn = (float)((double)lambda_n / ((double)rows * kn));
#define TRASE_FC_BWD(DPV) hipLaunchKernelGGL((fc_backward_kernel<DPV>), dim3(nb), dim3(256), 0, stream, u_tab, nrm, idx, rev_ranges, \
                                             rev_edges, (uint32_t)rows, (uint32_t)D, (uint32_t)kp, (uint32_t)kn, wp, wn, g_loss, g_feats)
  TRASE_LAUNCHES("feature3d_backward", stream, 0,
    if (dp == 8) TRASE_FC_BWD(8);
    else if (dp == 16) TRASE_FC_BWD(16);
    else if (dp == 32) TRASE_FC_BWD(32);
    else TRASE_FC_BWD(64));
#undef TRASE_FC_BWD
  return TRASE_OK;
}

static int cls_dims_ok(const char* who, int32_t S, int32_t N, int32_t C, int32_t k) {
  if (int rc = graph_dims_ok(who, S, k)) return rc;
  if (S < 1 || N < 1 || N == INT32_MAX || C < 1 || C > CL_MAX_C || (int64_t)N * (int64_t)C >= ((int64_t)1 << 31) ||
      (int64_t)S * (int64_t)C >= ((int64_t)1 << 31)) {
    set_error("%s: need S >= 1, N >= 1, 1 <= C <= %d and S * C, N * C < 2^31 (got S %d, N %d, C %d)", who, CL_MAX_C, S, N, C);
    return TRASE_ERR_INVALID;
  }
  return TRASE_OK;
}

int trase_cls3d_ws_bytes(int32_t S, int32_t C, size_t* ws_bytes) {
  if (!ws_bytes) { set_error("trase_cls3d_ws_bytes: null pointer"); return TRASE_ERR_INVALID; }
  if (int rc = cls_dims_ok("trase_cls3d_ws_bytes", S, S > 0 ? S : 1, C, 1)) return rc;
  double* p;
  *ws_bytes = array_layout<double>(nullptr, (size_t)blocks_of((uint32_t)S * (uint32_t)C) + 1, p);
  return TRASE_OK;
}

int trase_cls3d_forward(const float* pred, const int32_t* sample, const int32_t* idx, int32_t S, int32_t N, int32_t C, int32_t k,
                        float lambda_val, float* loss, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  if (int rc = cls_dims_ok("trase_cls3d_forward", S, N, C, k)) return rc;
  if (S > N) { set_error("trase_cls3d_forward: need S <= N (got S %d, N %d)", S, N); return TRASE_ERR_INVALID; }
  if (!pred || !sample || !idx || !loss) { set_error("trase_cls3d_forward: null pointer"); return TRASE_ERR_INVALID; }
  const int nb = blocks_of((uint32_t)S * (uint32_t)C);
  double* partial;
  if (!ws || ws_bytes < array_layout<double>(nullptr, (size_t)nb + 1, partial)) {
    set_error("trase_cls3d_forward: workspace too small"); return TRASE_ERR_WORKSPACE;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  array_layout<double>(ws, (size_t)nb + 1, partial);
  TRASE_LAUNCHES("cls3d_forward", stream, 0,
    hipLaunchKernelGGL(cls_forward_kernel, dim3(nb), dim3(256), 0, stream, pred, sample, idx, (uint32_t)S, (uint32_t)N, (uint32_t)C,
                       (uint32_t)k, partial);
    hipLaunchKernelGGL(f3_reduce_kernel, dim3(1), dim3(256), 0, stream, partial, (uint32_t)nb,
                       (double)lambda_val / ((double)S * (double)k * (double)C), loss));
  return TRASE_OK;
}

int trase_cls3d_backward(const float* pred, const int32_t* sample, const int32_t* idx, const int32_t* rev_ranges, const int32_t* rev_edges,
                         const int32_t* srev_ranges, const int32_t* srev_edges, int32_t S, int32_t N, int32_t C, int32_t k,
                         float lambda_val, const float* g_loss, float* g_pred, int32_t device, trase_stream_t stream_) {
  if (int rc = cls_dims_ok("trase_cls3d_backward", S, N, C, k)) return rc;
  if (!pred || !sample || !idx || !rev_ranges || !rev_edges || !srev_ranges || !srev_edges || !g_loss || !g_pred) {
    set_error("trase_cls3d_backward: null pointer"); return TRASE_ERR_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCH("cls3d_backward", stream, 0, cls_backward_kernel, dim3(blocks_of((uint32_t)N * (uint32_t)C)), dim3(256), 0, pred, sample, idx,
               rev_ranges, rev_edges, srev_ranges, srev_edges, (uint32_t)N, (uint32_t)C, (uint32_t)k, g_loss,
               (float)((double)lambda_val / ((double)S * (double)k * (double)C)), g_pred);
  return TRASE_OK;
}

}  // extern "C"
