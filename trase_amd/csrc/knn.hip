// knn.hip -- simple_knn._C.distCUDA2 (call site scene/gaussian_model.py:237): for every point the
// mean of the squared distances to its 3 nearest neighbours (exact).
//
// MI355X design: a spatial hash instead of the lineage's Morton-sort + box pruning.  Points are
// bucketed by hash(cell) with the stable radix sort of binning.hip, a query walks cube shells of
// cells outwards until the 3rd-best distance is provably final.  Hash collisions only add
// candidates that are filtered by their true cell, so the result is exact for any cell size.
// The same hash serves pytorch3d.ops.knn_points (knn_points_kernel) and the prompt lift (lift_kernel: 2D prompt ->
// nearest Gaussian -> cluster votes; trase_lift_votes).
#include "common.h"

namespace trase {

// device-resident parameters (no host round trip after the bounding-box reduction)
struct KnnParams {
  uint32_t n;          // number of points (device copy for the sort)
  uint32_t bb[6];      // order-preserving uint encodings of min xyz / max xyz
  float origin[3];
  float h, inv_h;
  int dims[3];
};

__device__ __forceinline__ uint32_t f2ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) {
  const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}

__device__ __forceinline__ uint32_t cell_hash(int x, int y, int z, uint32_t mask) {
  uint32_t h = (uint32_t)x * 73856093u ^ (uint32_t)y * 19349663u ^ (uint32_t)z * 83492791u;
  h ^= h >> 15; h *= 0x2c1b3c6du; h ^= h >> 12;
  return h & mask;
}

__global__ void knn_init_kernel(KnnParams* p, uint32_t n) {
  p->n = n;
  p->bb[0] = p->bb[1] = p->bb[2] = 0xffffffffu;
  p->bb[3] = p->bb[4] = p->bb[5] = 0u;
}

__global__ __launch_bounds__(256) void knn_bbox_kernel(const float* __restrict__ pts, int n, KnnParams* p) {
  float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float v = pts[3 * i + k];
      mn[k] = fminf(mn[k], v);
      mx[k] = fmaxf(mx[k], v);
    }
  }
  __shared__ float smn[3][256], smx[3][256];
#pragma unroll
  for (int k = 0; k < 3; ++k) { smn[k][threadIdx.x] = mn[k]; smx[k][threadIdx.x] = mx[k]; }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < (unsigned)s) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        smn[k][threadIdx.x] = fminf(smn[k][threadIdx.x], smn[k][threadIdx.x + s]);
        smx[k][threadIdx.x] = fmaxf(smx[k][threadIdx.x], smx[k][threadIdx.x + s]);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) {
    atomicMin(&p->bb[threadIdx.x], f2ord(smn[threadIdx.x][0]));
    atomicMax(&p->bb[3 + threadIdx.x], f2ord(smx[threadIdx.x][0]));
  }
}

// occ: target points per cell (4 for the register-list kernels; the wide k-NN asks for cells that hold about K points)
__global__ void knn_params_kernel(KnnParams* p, float occ) {
  float e[3];
  for (int k = 0; k < 3; ++k) {
    p->origin[k] = ord2f(p->bb[k]);
    e[k] = fmaxf(ord2f(p->bb[3 + k]) - p->origin[k], 0.f);
  }
  // sort extents descending
  float a = e[0], b = e[1], c = e[2];
  if (a < b) { float t = a; a = b; b = t; }
  if (b < c) { float t = b; b = c; c = t; }
  if (a < b) { float t = a; a = b; b = t; }
  const float n = (float)(p->n > 0 ? p->n : 1);
  const float h1 = occ * a / n;
  const float h2 = sqrtf(occ * a * b / n);
  const float h3 = cbrtf(occ * a * b * c / n);
  // effective dimensionality of the cloud; <=, so that an extent of exactly 0 (h2 = 0 under a collinear cloud) leaves its
  // branch too: with < such a cloud got h3 = 0, the floor below, and queries that walk tens of thousands of empty shells
  float h = (c <= h2) ? ((b <= h1) ? h1 : h2) : h3;
  h = fmaxf(h, a * (1.0f / 1048576.0f));           // at most 2^20 cells per axis
  if (!(h > 0.f)) h = 1.0f;                         // all points coincide
  p->h = h;
  p->inv_h = 1.0f / h;
  for (int k = 0; k < 3; ++k) p->dims[k] = (int)(e[k] * p->inv_h) + 1;
}

__device__ __forceinline__ void cell_of(const KnnParams& p, float x, float y, float z, int& cx, int& cy, int& cz) {
  cx = min(p.dims[0] - 1, max(0, (int)((x - p.origin[0]) * p.inv_h)));
  cy = min(p.dims[1] - 1, max(0, (int)((y - p.origin[1]) * p.inv_h)));
  cz = min(p.dims[2] - 1, max(0, (int)((z - p.origin[2]) * p.inv_h)));
}

__global__ __launch_bounds__(256) void knn_keys_kernel(const float* __restrict__ pts, int n, const KnnParams* pp,
                                                       uint32_t mask, uint32_t* __restrict__ keys) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const KnnParams p = *pp;
  int cx, cy, cz;
  cell_of(p, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], cx, cy, cz);
  keys[i] = cell_hash(cx, cy, cz, mask);
}

__device__ __forceinline__ void best3_insert(float d, float& b0, float& b1, float& b2) {
  if (d < b2) {
    if (d < b1) {
      b2 = b1;
      if (d < b0) { b1 = b0; b0 = d; } else { b1 = d; }
    } else {
      b2 = d;
    }
  }
}

__global__ __launch_bounds__(256) void knn_query_kernel(const float* __restrict__ pts, int n, const KnnParams* pp,
                                                        uint32_t mask, const uint32_t* __restrict__ sorted_ids,
                                                        const uint2* __restrict__ buckets, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const KnnParams p = *pp;
  const uint32_t self = sorted_ids[i];
  const float x = pts[3 * self], y = pts[3 * self + 1], z = pts[3 * self + 2];
  int cx, cy, cz;
  cell_of(p, x, y, z, cx, cy, cz);
  float b0 = 3.0e38f, b1 = 3.0e38f, b2 = 3.0e38f;
  const int rmax = max(p.dims[0], max(p.dims[1], p.dims[2]));
  for (int r = 0; r <= rmax; ++r) {
    const int z0 = max(cz - r, 0), z1 = min(cz + r, p.dims[2] - 1);
    const int y0 = max(cy - r, 0), y1 = min(cy + r, p.dims[1] - 1);
    const int x0 = max(cx - r, 0), x1 = min(cx + r, p.dims[0] - 1);
    for (int zz = z0; zz <= z1; ++zz)
      for (int yy = y0; yy <= y1; ++yy) {
        const bool face = (abs(zz - cz) == r) || (abs(yy - cy) == r);
        // on a face row every x is part of the shell; otherwise only the two end cells
        const int step = face ? 1 : max(1, 2 * r);
        for (int xx = face ? x0 : cx - r; xx <= (face ? x1 : cx + r); xx += step) {
          if (xx < 0 || xx >= p.dims[0]) continue;
          const uint2 bk = buckets[cell_hash(xx, yy, zz, mask)];
          for (uint32_t k = bk.x; k < bk.y; ++k) {
            const uint32_t j = sorted_ids[k];
            if (j == self) continue;
            const float qx = pts[3 * j], qy = pts[3 * j + 1], qz = pts[3 * j + 2];
            int ox, oy, oz;
            cell_of(p, qx, qy, qz, ox, oy, oz);
            if (ox != xx || oy != yy || oz != zz) continue;   // hash collision: belongs to another cell
            const float dx = qx - x, dy = qy - y, dz = qz - z;
            best3_insert(dx * dx + dy * dy + dz * dz, b0, b1, b2);
          }
        }
      }
    // everything in shells > r is farther than r*h
    const float bound = (float)r * p.h;
    if (b2 <= bound * bound) break;
  }
  // fewer than 4 points: the lineage's behaviour is undefined; average what exists
  float sum = 0.f; int cnt = 0;
  if (b0 < 3.0e38f) { sum += b0; ++cnt; }
  if (b1 < 3.0e38f) { sum += b1; ++cnt; }
  if (b2 < 3.0e38f) { sum += b2; ++cnt; }
  out[self] = cnt ? sum / 3.0f : 0.f;
}

// The shell walk of one query (x, y, z) over the hashed cloud `pts`: on return bd / bi hold the KT nearest points,
// ascending, squared distances (3.0e38f where the cloud has fewer).  `out2` is a lower bound of the squared distance from
// the query to the cloud's bounding box (0 for a query inside it; 0 is always valid): a cell outside shell r is at least
// r*h away along one axis and the box at least its own distance along the others, so the walk of a query outside the box
// may end as soon as bd[KT - 1] <= (r*h)^2 + out2 instead of crossing the whole grid.
template <int KT>
__device__ __forceinline__ void knn_walk(const KnnParams& p, float x, float y, float z, float out2,
                                         const float* __restrict__ pts, uint32_t mask,
                                         const uint32_t* __restrict__ sorted_ids, const uint2* __restrict__ buckets,
                                         float (&bd)[KT], uint32_t (&bi)[KT]) {
  int cx, cy, cz;
  cell_of(p, x, y, z, cx, cy, cz);
#pragma unroll
  for (int k = 0; k < KT; ++k) { bd[k] = 3.0e38f; bi[k] = 0u; }
  const int rmax = max(p.dims[0], max(p.dims[1], p.dims[2]));
  for (int r = 0; r <= rmax; ++r) {
    const int z0 = max(cz - r, 0), z1 = min(cz + r, p.dims[2] - 1);
    const int y0 = max(cy - r, 0), y1 = min(cy + r, p.dims[1] - 1);
    const int x0 = max(cx - r, 0), x1 = min(cx + r, p.dims[0] - 1);
    for (int zz = z0; zz <= z1; ++zz)
      for (int yy = y0; yy <= y1; ++yy) {
        const bool face = (abs(zz - cz) == r) || (abs(yy - cy) == r);
        const int step = face ? 1 : max(1, 2 * r);
        for (int xx = face ? x0 : cx - r; xx <= (face ? x1 : cx + r); xx += step) {
          if (xx < 0 || xx >= p.dims[0]) continue;
          const uint2 bk = buckets[cell_hash(xx, yy, zz, mask)];
          for (uint32_t k = bk.x; k < bk.y; ++k) {
            const uint32_t j = sorted_ids[k];
            const float qx = pts[3 * j], qy = pts[3 * j + 1], qz = pts[3 * j + 2];
            int ox, oy, oz;
            cell_of(p, qx, qy, qz, ox, oy, oz);
            if (ox != xx || oy != yy || oz != zz) continue;   // hash collision: belongs to another cell
            // the wide kernel's expression: differences and squares exact in float64, the sum rounded ONCE to fp32 (within
            // 2^-24 relative; all in fp32 the three differences round as well, up to 5 * 2^-24)
            // (the query is converted here, per candidate: hoisted out of the walk its three doubles cost KT = 8 a wave of
            // occupancy, 64 -> 70 VGPRs and +9 % at K = 6; the empty statement keeps the compiler from hoisting them)
            float xs = x, ys = y, zs = z;
            asm volatile("" : "+v"(xs), "+v"(ys), "+v"(zs));
            const double dx = (double)qx - (double)xs, dy = (double)qy - (double)ys, dz = (double)qz - (double)zs;
            float d = (float)(dx * dx + dy * dy + dz * dz);
            uint32_t id = j;
            if (d < bd[KT - 1] || (d == bd[KT - 1] && id < bi[KT - 1])) {
              // sorted insertion (ties by index so the result does not depend on the bucket order)
#pragma unroll
              for (int t = 0; t < KT; ++t) {
                const bool lt = d < bd[t] || (d == bd[t] && id < bi[t]);
                const float td = lt ? bd[t] : d; const uint32_t ti = lt ? bi[t] : id;
                bd[t] = lt ? d : bd[t]; bi[t] = lt ? id : bi[t];
                d = td; id = ti;
              }
            }
          }
        }
      }
    const float bound = (float)r * p.h;
    if (bd[KT - 1] <= bound * bound + out2 && r > 0) break;
    if (KT == 1 && bd[0] == 0.0f) break;
  }
}

// top-KT nearest points of the hashed cloud `pts` for every query point; ascending, squared distance
template <int KT>
__global__ __launch_bounds__(256) void knn_points_kernel(const float* __restrict__ qpts, int nq,
                                                         const float* __restrict__ pts, int n, int K,
                                                         const KnnParams* pp, uint32_t mask,
                                                         const uint32_t* __restrict__ sorted_ids,
                                                         const uint2* __restrict__ buckets,
                                                         int64_t* __restrict__ idx_out, float* __restrict__ dist_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const KnnParams p = *pp;
  float bd[KT];
  uint32_t bi[KT];
  knn_walk<KT>(p, qpts[3 * i], qpts[3 * i + 1], qpts[3 * i + 2], 0.0f, pts, mask, sorted_ids, buckets, bd, bi);
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    if (k < K) {
      const bool have = bd[k] < 3.0e38f;     // fewer than K points in the cloud: pad like pytorch3d (idx 0, dist 0)
      idx_out[(size_t)i * K + k] = have ? (int64_t)bi[k] : 0;
      dist_out[(size_t)i * K + k] = have ? bd[k] : 0.0f;
    }
  }
}

// ---- wide k-NN: 17 <= K <= 256 ---------------------------------------------------------------------------------------
// knn_walk's sorted register list cannot hold that many entries, so here ONE WAVE serves a query and the list lives in LDS.
// The wave walks the cube shells in knn_walk's order; its lanes take the entries of a bucket, apply the same true-cell
// filter and evaluate dx*dx + dy*dy + dz*dz (in float64, rounded once to fp32).  A candidate is the 64-bit key (float bits of d) << 32 | id: d >= 0, so
// its bits order like its value and the key order IS knn_walk's total order (distance, then lower index).  Keys below the
// current K-th are appended behind the kept K through a ballot prefix; when that staging area cannot take another 64 the
// whole array (a power of two, at most 512 keys) is sorted in LDS by the wave and the threshold drops to the new K-th.
// The walk ends by the narrow kernel's rule.  No workgroup barrier anywhere: the four waves of a block are independent.
constexpr int KW_WAVES = 4;
constexpr int KW_KEYS = 512;                      // kept K (<= 256) + staging (>= 64)
constexpr int KW_MAX_K = 256;
constexpr uint64_t KW_NONE = ~0ull;               // above every key of a finite distance

// LDS written by some lanes of the wave is read by others: order the accesses (for the compiler and the counters)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// ascending bitonic sort of keys[0, n) by one wave; n a power of two, 128 <= n <= KW_KEYS
__device__ __forceinline__ void kw_sort(uint64_t* keys, int n, int lane) {
  for (int size = 2; size <= n; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = lane; t < (n >> 1); t += WAVE) {
        const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));     // t with a 0 inserted at the stride's bit
        const int hi = lo | stride;
        const bool up = (lo & size) == 0;
        const uint64_t a = keys[lo], b = keys[hi];
        if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
      }
      wave_lds_sync();
    }
}

// total: keys of LDS this K uses, a power of two with 128 <= total <= KW_KEYS and total - K >= 64
__global__ __launch_bounds__(WAVE * KW_WAVES) void knn_points_wide_kernel(const float* __restrict__ qpts, int nq,
                                                                          const float* __restrict__ pts, int n, int K, int total,
                                                                          const KnnParams* pp, uint32_t mask,
                                                                          const uint32_t* __restrict__ sorted_ids,
                                                                          const uint2* __restrict__ buckets,
                                                                          int64_t* __restrict__ idx_out, float* __restrict__ dist_out) {
  __shared__ uint64_t lds[KW_WAVES][KW_KEYS];
  const int lane = (int)(threadIdx.x & (WAVE - 1));
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int i = blockIdx.x * KW_WAVES + wv;
  if (i >= nq) return;
  uint64_t* keys = lds[wv];
  const KnnParams p = *pp;
  const float x = qpts[3 * (size_t)i], y = qpts[3 * (size_t)i + 1], z = qpts[3 * (size_t)i + 2];
  for (int t = lane; t < total; t += WAVE) keys[t] = KW_NONE;
  wave_lds_sync();
  const int cap = total - K;          // room behind the kept K
  int staged = 0;
  uint64_t thr = KW_NONE;             // the K-th key so far: a candidate must be below it
  // sort kept + staged, keep the K smallest
  auto merge = [&]() {
    const int used = K + staged;
    int ns = 128;
    while (ns < used) ns <<= 1;
    for (int t = used + lane; t < ns; t += WAVE) keys[t] = KW_NONE;
    wave_lds_sync();
    kw_sort(keys, ns, lane);
    thr = keys[K - 1];
    staged = 0;
  };
  if (fabsf(x) < 3.0e38f && fabsf(y) < 3.0e38f && fabsf(z) < 3.0e38f) {     // a NaN / inf query finds nothing
    int cx, cy, cz;
    cell_of(p, x, y, z, cx, cy, cz);
    const int rmax = max(p.dims[0], max(p.dims[1], p.dims[2]));
    for (int r = 0; r <= rmax; ++r) {
      const int z0 = max(cz - r, 0), z1 = min(cz + r, p.dims[2] - 1);
      const int y0 = max(cy - r, 0), y1 = min(cy + r, p.dims[1] - 1);
      const int x0 = max(cx - r, 0), x1 = min(cx + r, p.dims[0] - 1);
      for (int zz = z0; zz <= z1; ++zz)
        for (int yy = y0; yy <= y1; ++yy) {
          const bool face = (abs(zz - cz) == r) || (abs(yy - cy) == r);
          const int step = face ? 1 : max(1, 2 * r);
          for (int xx = face ? x0 : cx - r; xx <= (face ? x1 : cx + r); xx += step) {
            if (xx < 0 || xx >= p.dims[0]) continue;
            const uint2 bk = buckets[cell_hash(xx, yy, zz, mask)];
            for (uint32_t k0 = bk.x; k0 < bk.y; k0 += WAVE) {
              if (staged + WAVE > cap) merge();
              const uint32_t k = k0 + (uint32_t)lane;
              uint64_t key = KW_NONE;
              if (k < bk.y) {
                const uint32_t j = sorted_ids[k];
                const float qx = pts[3 * (size_t)j], qy = pts[3 * (size_t)j + 1], qz = pts[3 * (size_t)j + 2];
                int ox, oy, oz;
                cell_of(p, qx, qy, qz, ox, oy, oz);
                // differences and squares in float64 are exact, so d is the squared distance rounded ONCE (three roundings
                // of the sum, each far below an fp32 ulp, aside): within 2^-24 relative, the expression of knn_walk.
                const double dx = (double)qx - (double)x, dy = (double)qy - (double)y, dz = (double)qz - (double)z;
                const float d = (float)(dx * dx + dy * dy + dz * dz);
                // (a hash collision belongs to another cell; a NaN or overflowed distance is never a neighbour, as in knn_walk)
                if (ox == xx && oy == yy && oz == zz && d < 3.0e38f) key = ((uint64_t)__float_as_uint(d) << 32) | j;
              }
              const bool pass = key < thr;
              const unsigned long long m = __ballot(pass);
              if (pass) keys[K + staged + __popcll(m & lanemask_lt())] = key;
              staged += __popcll(m);
            }
          }
        }
      if (staged > 0) merge();
      const float kd = thr == KW_NONE ? 3.0e38f : __uint_as_float((uint32_t)(thr >> 32));
      const float bound = (float)r * p.h;
      if (kd <= bound * bound && r > 0) break;
    }
  }
  wave_lds_sync();
  for (int k = lane; k < K; k += WAVE) {
    const uint64_t key = keys[k];
    const bool have = key != KW_NONE;      // fewer than K points in the cloud: pad like pytorch3d (idx 0, dist 0)
    idx_out[(size_t)i * K + k] = have ? (int64_t)(uint32_t)key : 0;
    dist_out[(size_t)i * K + k] = have ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
  }
}

// ---- prompt lift: 2D prompts to cluster votes (render.py:208-229, gui.py:1039-1064; one clicked pixel: gui.py:786-800) ----
// One thread per pixel of a 16 x 16 tile (mask form) or per listed pixel (click form): read the mask and the depth,
// un-project, walk the hash for the nearest point (knn_walk<1>, everything in registers), read its cluster id, vote.
// Votes are integer atomics into a per-block LDS histogram, flushed once per block with integer atomics on the non-zero
// bins: integer sums do not depend on the order, so the result is bitwise reproducible.
constexpr int LIFT_MAX_BINS = 4096;     // the LDS histogram: 16 KiB of int32
constexpr int LIFT_TILE = 16;           // a block's unit of work is 16 x 16 pixels: a wave covers 16 x 4 neighbours
constexpr int LIFT_BLOCK = LIFT_TILE * LIFT_TILE;
constexpr int LIFT_MAX_BLOCKS = 2048;   // blocks stride over the tiles: one histogram flush per block, not per tile

// p = u * m[0] + v * m[1] + d * m[2] - m[3] with u = ((c - 0.5) * sx - 1) * d, v = ((r - 0.5) * sy - 1) * d, where the host folds
// z = za * d - zb into rows 2 and 3 of the float64 inverse I before rounding to fp32: m[2] = za * I[2] + I[3], m[3] = zb * I[2].
// (z * I[2] + d * I[3] cancels about (zfar - znear) / (zfar * znear) * d down to the size of the point: with the rows rounded
// to fp32 separately their rounding alone moves the point by 2e-4 at d = 6, half of what the reference's fp32 inverse does.)
struct LiftCam { float m[12]; double sx, sy; };

template <bool CLICK>
__global__ __launch_bounds__(LIFT_BLOCK) void lift_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ pmask,
                                                          const int32_t* __restrict__ pixels, int M, int W, int H, LiftCam cam,
                                                          const float* __restrict__ pts, int n, const KnnParams* pp,
                                                          uint32_t mask, const uint32_t* __restrict__ sorted_ids,
                                                          const uint2* __restrict__ buckets, const int32_t* __restrict__ ids,
                                                          int bins, int* __restrict__ votes, int32_t* __restrict__ idx_out,
                                                          float* __restrict__ pts_out) {
  __shared__ int hist[LIFT_MAX_BINS];
  const int tid = threadIdx.x;
  for (int b = tid; b < bins; b += LIFT_BLOCK) hist[b] = 0;
  __syncthreads();
  KnnParams p = {};
  float bbmax[3] = {0.f, 0.f, 0.f};
  if (n > 0) {
    p = *pp;
#pragma unroll
    for (int k = 0; k < 3; ++k) bbmax[k] = ord2f(p.bb[3 + k]);
  }
  const int tiles_x = (W + LIFT_TILE - 1) / LIFT_TILE, tiles_y = (H + LIFT_TILE - 1) / LIFT_TILE;
  const int units = CLICK ? (M + LIFT_BLOCK - 1) / LIFT_BLOCK : tiles_x * tiles_y;
  for (int unit = blockIdx.x; unit < units; unit += gridDim.x) {
    int col, row;
    size_t out;
    bool listed, on;     // listed: the thread has an output slot;  on: it has a prompted pixel inside the image
    if (CLICK) {
      const int q = unit * LIFT_BLOCK + tid;
      listed = q < M;
      col = listed ? pixels[2 * q] : 0;
      row = listed ? pixels[2 * q + 1] : 0;
      on = listed && col >= 0 && col < W && row >= 0 && row < H;
      out = (size_t)q;
    } else {
      const int ty = unit / tiles_x;
      col = (unit - ty * tiles_x) * LIFT_TILE + (tid & (LIFT_TILE - 1));
      row = ty * LIFT_TILE + tid / LIFT_TILE;
      listed = col < W && row < H;
      out = (size_t)row * W + col;
      on = listed && pmask[out] != 0;
    }
    int best = -1;
    float x = 0.f, y = 0.f, z = 0.f;
    if (on) {
      const double d = (double)depth[(size_t)row * W + col];
      const double u = (((double)col - 0.5) * cam.sx - 1.0) * d, v = (((double)row - 0.5) * cam.sy - 1.0) * d;
      x = (float)(u * cam.m[0] + v * cam.m[3] + d * cam.m[6] - cam.m[9]);
      y = (float)(u * cam.m[1] + v * cam.m[4] + d * cam.m[7] - cam.m[10]);
      z = (float)(u * cam.m[2] + v * cam.m[5] + d * cam.m[8] - cam.m[11]);
      if (n > 0 && fabsf(x) < 3.0e38f && fabsf(y) < 3.0e38f && fabsf(z) < 3.0e38f) {   // a NaN / inf depth finds nothing
        const float q3[3] = {x, y, z};
        float out2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float o = fmaxf(fmaxf(p.origin[k] - q3[k], q3[k] - bbmax[k]), 0.f);
          out2 = fmaf(o, o, out2);
        }
        out2 *= 0.9999f;                // the bound must not exceed the true distance to the box: keep it below its rounding
        float bd[1];
        uint32_t bi[1];
        knn_walk<1>(p, x, y, z, out2, pts, mask, sorted_ids, buckets, bd, bi);
        if (bd[0] < 3.0e38f) best = (int)bi[0];
      }
      if (best >= 0 && bins > 0) {
        const int id = ids[best];
        if (id >= 0 && id < bins) atomicAdd(&hist[id], 1);     // a negative id (HDBSCAN noise) casts no vote
      }
    }
    if (listed) {
      if (idx_out) idx_out[out] = best;
      if (pts_out) { pts_out[3 * out] = x; pts_out[3 * out + 1] = y; pts_out[3 * out + 2] = z; }
    }
  }
  __syncthreads();
  for (int b = tid; b < bins; b += LIFT_BLOCK) {
    const int v = hist[b];
    if (v) atomicAdd(&votes[b], v);
  }
}

static int knn_bits(int N) {
  int bits = 4;
  while ((1u << bits) < (uint32_t)N && bits < 26) ++bits;
  return bits;
}

struct KnnWs { KnnParams* prm; SortBufs sort; uint2* buckets; };

// hist_copies = 1: these sorts take the three-launch passes
static size_t knn_layout(void* ws, int N, KnnWs& w) {
  WsCursor c(ws);
  w.prm = c.take<KnnParams>(1);
  sort_layout(c, w.sort, (size_t)(N > 0 ? N : 1), SORT_ALL, 8, 1);
  w.buckets = c.take<uint2>((size_t)1 << knn_bits(N));
  return c.bytes();
}
static size_t knn_ws_bytes(int N) { KnnWs w; return knn_layout(nullptr, N, w); }

}  // namespace trase

using namespace trase;

extern "C" {

int trase_knn_sizes(int32_t N, size_t* ws_bytes) {
  if (!ws_bytes || N < 0) { set_error("trase_knn_sizes: bad arguments"); return TRASE_ERR_INVALID; }
  *ws_bytes = knn_ws_bytes(N);
  return TRASE_OK;
}

static int knn_build(const LaunchCtx& c, const float* points, int32_t N, KnnWs& w, uint32_t mask, int bits, int* idx_out,
                     float occ = 4.0f) {
  hipStream_t stream = c.stream;
  const int blocks = (N + 255) / 256;
  TRASE_LAUNCHES_AS("knn_bbox", "knn_keys", stream, 0,
    hipLaunchKernelGGL(knn_init_kernel, dim3(1), dim3(1), 0, stream, w.prm, (uint32_t)N);
    hipLaunchKernelGGL(knn_bbox_kernel, dim3(blocks < 1024 ? blocks : 1024), dim3(256), 0, stream, points, N, w.prm);
    hipLaunchKernelGGL(knn_params_kernel, dim3(1), dim3(1), 0, stream, w.prm, occ);
    hipLaunchKernelGGL(knn_keys_kernel, dim3(blocks), dim3(256), 0, stream, points, N, w.prm, mask, w.sort.keys[0]));
  int rc = radix_sort_pairs(c, w.sort, &w.prm->n, (uint32_t)N, 0, bits, true, idx_out);
  if (rc) return rc;
  return launch_tile_ranges(c, w.sort.keys[*idx_out], &w.prm->n, (uint32_t)N, w.buckets, 1 << bits);
}

int trase_knn_dist2(const float* points, int32_t N, float* out, void* ws, size_t ws_bytes, int32_t device,
                    trase_stream_t stream_) {
  if (N < 0 || (N > 0 && (!points || !out))) { set_error("trase_knn_dist2: bad arguments"); return TRASE_ERR_INVALID; }
  if (N == 0) return TRASE_OK;
  if (!ws || ws_bytes < knn_ws_bytes(N)) { set_error("trase_knn_dist2: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  LaunchCtx c{stream, 0, 0};
  KnnWs w; knn_layout(ws, N, w);
  const int bits = knn_bits(N);
  const uint32_t mask = (1u << bits) - 1u;
  int idx = 0;
  int rc = knn_build(c, points, N, w, mask, bits, &idx);
  if (rc) return rc;
  TRASE_LAUNCH("knn_query", stream, 0, knn_query_kernel, dim3((N + 255) / 256), dim3(256), 0, points, N, w.prm, mask, w.sort.vals[idx],
               w.buckets, out);
  return TRASE_OK;
}

// pytorch3d.ops.knn_points replacement (call sites scene/gaussian_model.py:88-92 K=16 self-KNN,
// render.py:222 / gui.py:1048 / utils/loss_utils.py:141,192 cross-KNN): the K nearest points of
// p2 for every point of p1, ascending, squared distances; a query that is itself in p2 finds itself.
// K <= 16: one thread per query (knn_points_kernel); 17 <= K <= 256: one wave per query (knn_points_wide_kernel).
int trase_knn_points(const float* p1, int32_t N1, const float* p2, int32_t N2, int32_t K, int64_t* idx_out,
                     float* dist_out, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  if (N1 < 0 || N2 < 0 || K < 1 || K > KW_MAX_K) {
    set_error("trase_knn_points: need N1, N2 >= 0 and 1 <= K <= %d (got N1 %d, N2 %d, K %d)", KW_MAX_K, N1, N2, K);
    return TRASE_ERR_INVALID;
  }
  if (N1 == 0) return TRASE_OK;
  if (!p1 || !idx_out || !dist_out || (N2 > 0 && !p2)) { set_error("trase_knn_points: null pointer"); return TRASE_ERR_INVALID; }
  if (!ws || ws_bytes < knn_ws_bytes(N2)) { set_error("trase_knn_points: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  LaunchCtx c{stream, 0, 0};
  const int blocks = (N1 + 255) / 256;
  if (N2 == 0) {   // nothing to find: pytorch3d pads with idx 0 / dist 0 -- keep that convention
    if (int rc = launch_zero_bytes(idx_out, sizeof(int64_t) * (size_t)N1 * K, stream)) return rc;
    return launch_zero_bytes(dist_out, sizeof(float) * (size_t)N1 * K, stream);
  }
  KnnWs w; knn_layout(ws, N2, w);
  const int bits = knn_bits(N2);
  const uint32_t mask = (1u << bits) - 1u;
  int idx = 0;
  const bool wide = K > 16;
  // wide: cells of about 3 K / 4 points, so that the ball the first shell guarantees usually holds the K nearest
  int rc = knn_build(c, p2, N2, w, mask, bits, &idx, wide ? 0.75f * (float)K : 4.0f);
  if (rc) return rc;
  if (wide) {
    int total = 128;
    while (total < 2 * K + WAVE && total < KW_KEYS) total <<= 1;
    TRASE_LAUNCH("knn_points_wide", stream, 0, knn_points_wide_kernel, dim3((N1 + KW_WAVES - 1) / KW_WAVES), dim3(WAVE * KW_WAVES), 0, p1, N1,
                 p2, N2, K, total, w.prm, mask, w.sort.vals[idx], w.buckets, idx_out, dist_out);
    return TRASE_OK;
  }
#define TRASE_KQ(KT) hipLaunchKernelGGL((knn_points_kernel<KT>), dim3(blocks), dim3(256), 0, stream, p1, N1, p2, N2, K, w.prm, mask, w.sort.vals[idx], w.buckets, idx_out, dist_out)
  TRASE_LAUNCHES("knn_points_query", stream, 0,
    if (K <= 1) TRASE_KQ(1); else if (K <= 4) TRASE_KQ(4); else if (K <= 8) TRASE_KQ(8); else TRASE_KQ(16));
#undef TRASE_KQ
  return TRASE_OK;
}

int trase_lift_sizes(int32_t N, int32_t bins, size_t* ws_bytes) {
  if (!ws_bytes || N < 0 || bins < 0 || bins > LIFT_MAX_BINS) {
    set_error("trase_lift_sizes: need N >= 0, 0 <= bins <= %d (got N %d, bins %d)", LIFT_MAX_BINS, N, bins);
    return TRASE_ERR_INVALID;
  }
  *ws_bytes = knn_ws_bytes(N);
  return TRASE_OK;
}

int trase_lift_votes(const float* depth, int32_t W, int32_t H, const double* inv_proj, double znear, double zfar,
                     const uint8_t* prompt_mask, const int32_t* pixels, int32_t M, const float* points, int32_t N,
                     const int32_t* cluster_ids, int32_t bins, int32_t* votes_out, int32_t* index_out, float* points_out,
                     void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream_) {
  if (N < 0 || bins < 0 || bins > LIFT_MAX_BINS) {
    set_error("trase_lift_votes: need N >= 0, 0 <= bins <= %d (got N %d, bins %d)", LIFT_MAX_BINS, N, bins);
    return TRASE_ERR_INVALID;
  }
  if (W < 1 || H < 1 || (int64_t)W * H > (int64_t)0x7fffffff || M < 0 || !(zfar != znear)) {
    set_error("trase_lift_votes: bad arguments (W %d, H %d, M %d, znear %g, zfar %g)", W, H, M, znear, zfar);
    return TRASE_ERR_INVALID;
  }
  const bool click = prompt_mask == nullptr;
  if (!depth || !inv_proj || (!click && pixels) || (click && M > 0 && !pixels) || (N > 0 && !points) ||
      (bins > 0 && (!votes_out || (N > 0 && !cluster_ids)))) {
    set_error("trase_lift_votes: null pointer (or both a mask and a pixel list)");
    return TRASE_ERR_INVALID;
  }
  if (N > 0 && (!ws || ws_bytes < knn_ws_bytes(N))) { set_error("trase_lift_votes: workspace too small"); return TRASE_ERR_WORKSPACE; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  if (int rc = launch_zero_bytes(votes_out, sizeof(int32_t) * (size_t)bins, stream)) return rc;   // (bins == 0: no launch)
  if (click && M == 0) return TRASE_OK;
  LiftCam cam;
  const double za = zfar / (zfar - znear), zb = zfar * znear / (zfar - znear);
  for (int k = 0; k < 3; ++k) {
    cam.m[k] = (float)inv_proj[k];
    cam.m[3 + k] = (float)inv_proj[4 + k];
    cam.m[6 + k] = (float)(za * inv_proj[8 + k] + inv_proj[12 + k]);
    cam.m[9 + k] = (float)(zb * inv_proj[8 + k]);
  }
  cam.sx = 2.0 / (double)W;
  cam.sy = 2.0 / (double)H;
  LaunchCtx c{stream, 0, 0};
  KnnWs w = {};
  uint32_t mask = 0u;
  int idx = 0;
  if (N > 0) {          // N == 0: nothing to find -- no hash, every index -1, no votes
    knn_layout(ws, N, w);
    const int bits = knn_bits(N);
    mask = (1u << bits) - 1u;
    int rc = knn_build(c, points, N, w, mask, bits, &idx);
    if (rc) return rc;
  }
  const int units = click ? (M + LIFT_BLOCK - 1) / LIFT_BLOCK
                          : ((W + LIFT_TILE - 1) / LIFT_TILE) * ((H + LIFT_TILE - 1) / LIFT_TILE);
  const int blocks = units < LIFT_MAX_BLOCKS ? units : LIFT_MAX_BLOCKS;
#define TRASE_LIFT(CLICK) hipLaunchKernelGGL((lift_kernel<CLICK>), dim3(blocks), dim3(LIFT_BLOCK), 0, stream, depth, prompt_mask, \
                                             pixels, M, W, H, cam, points, N, w.prm, mask, N > 0 ? w.sort.vals[idx] : nullptr, \
                                             w.buckets, cluster_ids, bins, votes_out, index_out, points_out)
  TRASE_LAUNCHES("lift_votes", stream, 0, if (click) TRASE_LIFT(true); else TRASE_LIFT(false));
#undef TRASE_LIFT
  return TRASE_OK;
}

}  // extern "C"
