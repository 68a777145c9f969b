// maskbits.hip -- a view's SAM masks as the bit stream the reference stores them in (extract_masks.py:91-99), read in place.
// The reference keeps the N x H x W bool masks of a view as ONE flat stream of N * H * W bits, big-endian inside a byte
// (numpy.packbits(masks.reshape(-1)) == bitarray(...).tobytes()): stream bit i is bit 7 - (i & 7) of byte i >> 3, mask n starts
// at stream bit n * HW -- in the middle of a byte wherever HW is no multiple of 8 -- and nothing is padded but the last byte.
// train.py:245-249 expands it to bool bytes on the host every FEATURE iteration; here the head's three needs are served from
// the stream itself, an eighth of the bytes:
//   mask_stats_bits   per-pixel cover counts + per-mask sizes in one pass (what mask_stats16_kernel does on bool bytes)
//   pack / unpack     bool bytes <-> stream on the device, flat over all N * HW elements
// (the third need, the membership bits of the sampled pixels, is ph_gather_kernel<.., BITS> in pairhead.hip).
// Every kernel takes the stream as aligned dwords of a buffer of bits_bytes (a multiple of 16) and reads no dword at or past
// it; bits at or past N * HW never reach a result.
#include "common.h"

namespace trase {

constexpr int MB_GROUP = 8;        // masks per carry-save group (and loads in flight per lane: two dwords each)
constexpr int MB_PLANES = 14;      // counter planes: cover counts up to 8192 = 2^13
constexpr int MB_PIX = 32;         // pixels per lane: one window

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {     // lanes with no source (or rows masked off) receive 0
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
// integer sum over the 64 lanes, valid in lane 63 only (wave_sum_lane63's steps)
__device__ __forceinline__ uint32_t wave_sum_u_lane63(uint32_t v) {
  v += dpp_u<0x111>(v);
  v += dpp_u<0x112>(v);
  v += dpp_u<0x114>(v);
  v += dpp_u<0x118>(v);
  v += dpp_u<0x142, 0xa>(v);
  v += dpp_u<0x143, 0xc>(v);
  return v;
}

// carry-save adder on 32 one-bit columns at once: a + b + c = sum + 2 carry
__device__ __forceinline__ void csa(uint32_t a, uint32_t b, uint32_t c, uint32_t& sum, uint32_t& carry) {
  const uint32_t u = a ^ b;
  carry = (a & b) | (u & c);
  sum = u ^ c;
}

// A lane owns the 32 pixels [p0, p0 + 32).  Its window of mask n is the 32 stream bits from n * HW + p0, first pixel in the MOST
// significant bit: two aligned dwords, each byte-swapped (the stream is big-endian inside a byte, so a swapped dword holds 32
// stream bits in descending significance), funnel-shifted by (n * HW + p0) & 31 = (n * HW) & 31 -- the same for every lane.
// Cover counts are bit-sliced: plane k holds bit k of the 32 pixels' counts; eight windows go through a Harley-Seal tree of
// seven carry-save adders into planes 0..2 and ONE carry word ripples into the planes above, so a mask costs ~6 logic
// operations per 32 pixels and no bit is extracted before the end.  Mask sizes: __popc of the window, two masks packed per
// word, wave total by DPP, LDS, one global integer atomic per workgroup and mask.
__global__ __launch_bounds__(256) void mask_stats_bits_kernel(const uint32_t* __restrict__ dw, unsigned long long ndw, int N,
                                                              long long HW, int nplanes, int32_t* __restrict__ cover,
                                                              uint32_t* __restrict__ size) {
  extern __shared__ uint32_t lsize[];
  for (int n = threadIdx.x; n < N; n += 256) lsize[n] = 0u;
  __syncthreads();
  const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * MB_PIX;
  const long long left = HW - p0;                             // pixels of this lane that exist
  const bool in = left > 0;
  const uint32_t vm = left >= MB_PIX ? 0xffffffffu : (in ? ~(0xffffffffu >> (int)left) : 0u);   // the window's bits below HW
  uint32_t c[MB_PLANES];
#pragma unroll
  for (int k = 0; k < MB_PLANES; ++k) c[k] = 0u;

  uint32_t hi[MB_GROUP], lo[MB_GROUP], nhi[MB_GROUP], nlo[MB_GROUP];
  auto fetch = [&](int n0, uint32_t* h, uint32_t* l) {
#pragma unroll
    for (int u = 0; u < MB_GROUP; ++u) {
      const int n = n0 + u;
      const unsigned long long b = (unsigned long long)n * (unsigned long long)HW + (unsigned long long)p0;
      const unsigned long long d = b >> 5;
      const bool on = in && n < N;                             // then d < ndw: stream bit b exists
      // no branch around a load (sixteen stay in flight): an index that is not wanted is clamped into the buffer, its value dropped
      const uint32_t vh = dw[min(d, ndw - 1)], vl = dw[min(d + 1, ndw - 1)];
      h[u] = on ? vh : 0u;
      l[u] = (on && d + 1 < ndw) ? vl : 0u;
    }
  };
  fetch(0, hi, lo);
  for (int n0 = 0; n0 < N; n0 += MB_GROUP) {
    if (n0 + MB_GROUP < N) fetch(n0 + MB_GROUP, nhi, nlo);     // the next group's loads are in flight under this group's adds
    uint32_t w[MB_GROUP];
#pragma unroll
    for (int u = 0; u < MB_GROUP; ++u) {
      const uint32_t sh = (uint32_t)(((unsigned long long)(n0 + u) * (unsigned long long)HW) & 31u);   // wave-uniform
      const unsigned long long both = ((unsigned long long)__builtin_bswap32(hi[u]) << 32) | __builtin_bswap32(lo[u]);
      w[u] = (uint32_t)(both >> (32u - sh)) & vm;
    }
    uint32_t t0, t1, f0, f1, e;
    csa(c[0], w[0], w[1], c[0], t0);
    csa(c[0], w[2], w[3], c[0], t1);
    csa(c[1], t0, t1, c[1], f0);
    csa(c[0], w[4], w[5], c[0], t0);
    csa(c[0], w[6], w[7], c[0], t1);
    csa(c[1], t0, t1, c[1], f1);
    csa(c[2], f0, f1, c[2], e);
#pragma unroll
    for (int k = 3; k < MB_PLANES; ++k) {
      if (k < nplanes) {                                       // (uniform) a count below 2^nplanes carries no further
        const uint32_t carry = c[k] & e;
        c[k] ^= e;
        e = carry;
      }
    }
#pragma unroll
    for (int u = 0; u < MB_GROUP; u += 2) {
      const uint32_t tot = wave_sum_u_lane63((uint32_t)__popc(w[u]) | ((uint32_t)__popc(w[u + 1]) << 16));   // each <= 2048
      if ((threadIdx.x & 63) == 63) {
        if (n0 + u < N && (tot & 0xffffu)) atomicAdd(&lsize[n0 + u], tot & 0xffffu);
        if (n0 + u + 1 < N && (tot >> 16)) atomicAdd(&lsize[n0 + u + 1], tot >> 16);
      }
    }
#pragma unroll
    for (int u = 0; u < MB_GROUP; ++u) { hi[u] = nhi[u]; lo[u] = nlo[u]; }
  }
  if (in) {
    uint32_t cnt[MB_PIX];
#pragma unroll
    for (int j = 0; j < MB_PIX; ++j) cnt[j] = 0u;
#pragma unroll
    for (int k = 0; k < MB_PLANES; ++k) {
      if (k < nplanes) {
#pragma unroll
        for (int j = 0; j < MB_PIX; ++j) cnt[j] |= ((c[k] >> (31 - j)) & 1u) << k;
      }
    }
    if (left >= MB_PIX && ((size_t)cover & 15) == 0) {
#pragma unroll
      for (int j = 0; j < MB_PIX; j += 4)
        *reinterpret_cast<int4*>(cover + p0 + j) = make_int4((int)cnt[j], (int)cnt[j + 1], (int)cnt[j + 2], (int)cnt[j + 3]);
    } else {
#pragma unroll
      for (int j = 0; j < MB_PIX; ++j) if (j < left) cover[p0 + j] = (int32_t)cnt[j];
    }
  }
  __syncthreads();
  for (int n = threadIdx.x; n < N; n += 256) if (lsize[n]) atomicAdd(&size[n], lsize[n]);
}

// ---- bool bytes <-> stream -------------------------------------------------------------------------------------------------
// four flag bytes (any non-zero byte is set) -> the nibble e0 e1 e2 e3, first element in the most significant bit
__device__ __forceinline__ uint32_t flags_nibble(uint32_t v) {
  const uint32_t x = ((((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u) >> 7;       // bits 0, 8, 16, 24 = e0 .. e3
  return ((x * 0x08040201u) >> 24) & 0xfu;                   // the ten partial products fall on distinct bits: no carries
}
// the nibble e0 e1 e2 e3 -> four bytes of exactly 0 / 1
__device__ __forceinline__ uint32_t nibble_flags(uint32_t n) { return (((n & 0xfu) * 0x08040201u) >> 3) & 0x01010101u; }

// one thread per dword of the output buffer (padding included: written as zero): 32 flags in, 16-byte loads where all 32 exist
__global__ __launch_bounds__(256) void pack_masks_kernel(const uint8_t* __restrict__ flags, unsigned long long total,
                                                         uint32_t* __restrict__ dw, unsigned long long ndw) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= ndw) return;
  const unsigned long long e0 = i * 32;
  uint32_t out = 0u;
  if (e0 + 32 <= total && ((size_t)flags & 15) == 0) {
    const uint4 a = *reinterpret_cast<const uint4*>(flags + e0), b = *reinterpret_cast<const uint4*>(flags + e0 + 16);
    const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) out |= ((flags_nibble(v[2 * q]) << 4) | flags_nibble(v[2 * q + 1])) << (8 * q);   // byte q of the dword
  } else {
#pragma unroll 4
    for (int j = 0; j < 32; ++j)
      if (e0 + j < total && flags[e0 + j]) out |= 1u << (8 * (j >> 3) + 7 - (j & 7));
  }
  dw[i] = out;
}

// one thread per dword of the stream that holds an element: 32 bytes out, as two 16-byte stores where all 32 exist
__global__ __launch_bounds__(256) void unpack_masks_kernel(const uint32_t* __restrict__ dw, unsigned long long total,
                                                           uint8_t* __restrict__ flags) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long e0 = i * 32;
  if (e0 >= total) return;
  const uint32_t v = dw[i];
  if (e0 + 32 <= total && ((size_t)flags & 15) == 0) {
    uint32_t o[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t byte = (v >> (8 * q)) & 0xffu;
      o[2 * q] = nibble_flags(byte >> 4);
      o[2 * q + 1] = nibble_flags(byte);
    }
    *reinterpret_cast<uint4*>(flags + e0) = make_uint4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<uint4*>(flags + e0 + 16) = make_uint4(o[4], o[5], o[6], o[7]);
  } else {
#pragma unroll 4
    for (int j = 0; j < 32; ++j)
      if (e0 + j < total) flags[e0 + j] = (uint8_t)((v >> (8 * (j >> 3) + 7 - (j & 7))) & 1u);
  }
}

}  // namespace trase

using namespace trase;

extern "C" {

int trase_mask_stats_bits(const uint8_t* bits, size_t bits_bytes, int32_t N, int64_t HW, int32_t* cover_count, uint32_t* mask_size,
                          int32_t device, trase_stream_t stream_) {
  if (!cover_count || !mask_size) { set_error("trase_mask_stats_bits: null pointer"); return TRASE_ERR_INVALID; }
  if (int rc = mask_bits_ok("trase_mask_stats_bits", bits, bits_bytes, N, HW)) return rc;
  int nplanes = 1;
  while ((1 << nplanes) <= N) ++nplanes;                     // floor(log2 N) + 1: every count <= N fits
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  if (int rc = launch_zero_bytes(mask_size, sizeof(uint32_t) * (size_t)N, stream)) return rc;
  const int64_t per_block = 256 * MB_PIX;
  TRASE_LAUNCH("mask_stats_bits", stream, 0, mask_stats_bits_kernel, dim3((unsigned)((HW + per_block - 1) / per_block)), dim3(256),
               sizeof(uint32_t) * (size_t)N, reinterpret_cast<const uint32_t*>(bits), (unsigned long long)(bits_bytes / 4), N, (long long)HW, nplanes,
               cover_count, mask_size);
  return TRASE_OK;
}

int trase_pack_masks(const uint8_t* sam_masks, int32_t N, int64_t HW, uint8_t* bits, size_t bits_bytes, int32_t device,
                     trase_stream_t stream_) {
  if (!sam_masks) { set_error("trase_pack_masks: null pointer"); return TRASE_ERR_INVALID; }
  if (int rc = mask_bits_ok("trase_pack_masks", bits, bits_bytes, N, HW)) return rc;
  const unsigned long long ndw = bits_bytes / 4, blocks = (ndw + 255) / 256;
  if (blocks > 0x7fffffffull) { set_error("trase_pack_masks: %zu stream bytes are more than one launch covers", bits_bytes); return TRASE_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCH("pack_masks", stream, 0, pack_masks_kernel, dim3((unsigned)blocks), dim3(256), 0, sam_masks,
               (unsigned long long)N * (unsigned long long)HW, reinterpret_cast<uint32_t*>(bits), ndw);
  return TRASE_OK;
}

int trase_unpack_masks(const uint8_t* bits, size_t bits_bytes, int32_t N, int64_t HW, uint8_t* sam_masks, int32_t device,
                       trase_stream_t stream_) {
  if (!sam_masks) { set_error("trase_unpack_masks: null pointer"); return TRASE_ERR_INVALID; }
  if (int rc = mask_bits_ok("trase_unpack_masks", bits, bits_bytes, N, HW)) return rc;
  const unsigned long long total = (unsigned long long)N * (unsigned long long)HW, blocks = ((total + 31) / 32 + 255) / 256;
  if (blocks > 0x7fffffffull) { set_error("trase_unpack_masks: %llu elements are more than one launch covers", total); return TRASE_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  TRASE_LAUNCH("unpack_masks", stream, 0, unpack_masks_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<const uint32_t*>(bits), total,
               sam_masks);
  return TRASE_OK;
}

}  // extern "C"
