// selftest.hip -- on-device checks of the wave64 primitives the kernels rely on.  Cheap insurance:
// DPP control codes, ballot widths and MFMA fragment layouts are easy to get subtly wrong and
// cannot be exercised in the GPU-less build container.
#include <string>

#include "common.h"

namespace trase {

// out[0]: wave_sum result from lane 63; out[1]: broadcast sum seen by lane 0; out[2..3]: ballot of
// odd lanes; out[4]: popcount(lanemask_lt) summed over lanes (= 2016); out[5]: lane_id sum
__global__ void selftest_wave_kernel(float* outf, unsigned long long* outu) {
  const unsigned lane = threadIdx.x;
  const float v = (float)(lane + 1);            // sum = 2080
  const float s63 = wave_sum_lane63(v);
  if (lane == 63) outf[0] = s63;
  const float all = wave_sum_all(v);
  if (lane == 0) outf[1] = all;
  const unsigned long long bal = __ballot(lane & 1u);
  if (lane == 0) outu[0] = bal;
  float pc = (float)__popcll(lanemask_lt());
  pc = wave_sum_all(pc);
  if (lane == 0) outf[2] = pc;
  float li = wave_sum_all((float)lane_id());
  if (lane == 0) outf[3] = li;
  // scans: inclusive add of 1..64 -> lane l holds (l+1)(l+2)/2; inclusive mul of 2 on even lanes (1 on odd)
  const float sa = wave_scan_add(v);
  float bad = (sa == 0.5f * (float)((lane + 1) * (lane + 2))) ? 0.f : 1.f;
  const float sm = wave_scan_mul((lane & 1u) ? 1.0f : 1.03125f);
  float want = 1.0f;
  for (unsigned k = 0; k <= lane; k += 2) want *= 1.03125f;
  bad += (fabsf(sm - want) <= 1e-5f * want) ? 0.f : 1.f;
  const float sa2 = wave_scan_add_asm(v);
  bad += (sa2 == sa) ? 0.f : 1.f;
  const float sm2 = wave_scan_mul_asm((lane & 1u) ? 1.0f : 1.03125f);
  bad += (sm2 == sm) ? 0.f : 1.f;
  const float sh = wave_shr1(v, -7.0f);
  bad += (sh == (lane == 0 ? -7.0f : (float)lane)) ? 0.f : 1.f;
  bad = wave_sum_all(bad);
  if (lane == 0) outf[4] = bad;
}

// MFMA f32 32x32x2 layout probe: A[i][k] = i + 100k, B[k][j] = (j+1) * (k ? 0.5 : 1)
//   D[i][j] = (i)*(j+1) + (i+100)*(j+1)*0.5
__global__ void selftest_mfma_kernel(float* out /* 32*32 */) {
  typedef float v16f __attribute__((ext_vector_type(16)));
  const unsigned lane = threadIdx.x;
  const int i = lane & 31, k = lane >> 5;
  const float a = (float)i + 100.f * (float)k;
  const float b = (float)(i + 1) * (k ? 0.5f : 1.0f);
  v16f acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  // documented layout: column = lane % 32, row = 8*(r/4) + 4*(lane/32) + r%4
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = 8 * (r / 4) + 4 * (int)(lane >> 5) + (r % 4);
    const int col = lane & 31;
    out[row * 32 + col] = acc[r];
  }
}

}  // namespace trase

using namespace trase;

extern "C" int trase_selftest(int32_t device, trase_stream_t stream_, char* msg, size_t msg_bytes) {
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  float* df = nullptr;
  unsigned long long* du = nullptr;
  float* dm = nullptr;
  TRASE_CHECK(hipMalloc((void**)&df, 16 * sizeof(float)));
  TRASE_CHECK(hipMalloc((void**)&du, 4 * sizeof(unsigned long long)));
  TRASE_CHECK(hipMalloc((void**)&dm, 1024 * sizeof(float)));
  // checked by hand, not through TRASE_POST_LAUNCH: an early return would leak the three buffers
  hipLaunchKernelGGL(selftest_wave_kernel, dim3(1), dim3(64), 0, stream, df, du);
  int rc = check_hip(hipGetLastError(), "selftest_wave");
  if (!rc) {
    hipLaunchKernelGGL(selftest_mfma_kernel, dim3(1), dim3(64), 0, stream, dm);
    rc = check_hip(hipGetLastError(), "selftest_mfma");
  }
  float hf[16];
  unsigned long long hu[4];
  static float hm[1024];
  if (!rc) rc = check_hip(hipMemcpyAsync(hf, df, sizeof(hf), hipMemcpyDeviceToHost, stream), "selftest copy");
  if (!rc) rc = check_hip(hipMemcpyAsync(hu, du, sizeof(hu), hipMemcpyDeviceToHost, stream), "selftest copy");
  if (!rc) rc = check_hip(hipMemcpyAsync(hm, dm, sizeof(hm), hipMemcpyDeviceToHost, stream), "selftest copy");
  if (!rc) rc = check_hip(hipStreamSynchronize(stream), "selftest sync");
  hipFree(df); hipFree(du); hipFree(dm);
  if (rc) return rc;
  std::string report;
  int bad = 0;
  auto expect = [&](const char* what, double got, double want) {
    char line[160];
    const bool ok = got == want;
    snprintf(line, sizeof(line), "%s: got %.6g want %.6g %s\n", what, got, want, ok ? "ok" : "FAIL");
    report += line;
    if (!ok) ++bad;
  };
  expect("wave_sum lane63", hf[0], 2080.0);
  expect("wave_sum broadcast", hf[1], 2080.0);
  expect("ballot odd lanes", (double)(hu[0] == 0xAAAAAAAAAAAAAAAAull), 1.0);
  expect("lanemask_lt popcount sum", hf[2], 2016.0);
  expect("lane_id sum", hf[3], 2016.0);
  expect("wave scans (builtin + asm add/mul, shr1) bad lanes", hf[4], 0.0);
  int mfma_bad = 0;
  for (int i = 0; i < 32; ++i)
    for (int j = 0; j < 32; ++j) {
      const float want = (float)i * (float)(j + 1) + ((float)i + 100.f) * ((float)(j + 1) * 0.5f);
      if (hm[i * 32 + j] != want) ++mfma_bad;
    }
  expect("mfma 32x32x2 f32 layout mismatches", mfma_bad, 0.0);
  if (msg && msg_bytes) {
    snprintf(msg, msg_bytes, "%s", report.c_str());
  }
  return bad;
}

// ---- test entry points of the radix sort, the tile ranges and the zero fill (binning.hip) ------------------------------------
namespace {
struct DevBlock {          // one allocation, freed on every way out
  void* p = nullptr;
  ~DevBlock() { if (p) hipFree(p); }
};
}  // namespace

extern "C" int trase_selftest_sort(const uint32_t* keys, const uint32_t* vals, uint32_t n, uint32_t cap, int32_t bit_lo,
                                   int32_t bit_hi, int32_t digit_bits, int32_t hist_copies, int32_t start, uint32_t flag_key,
                                   int32_t use_flag, uint32_t sentinel, uint32_t* keys_out, uint32_t* vals_out, uint32_t* result,
                                   int32_t device, trase_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!keys || !keys_out || !vals_out || !result || cap < 1 || (digit_bits != 8 && digit_bits != 9) || bit_lo < 0 ||
      bit_hi <= bit_lo || bit_hi > 32 || hist_copies < 0 || (start != 0 && start != 1)) {
    set_error("trase_selftest_sort: bad arguments");
    return TRASE_ERR_INVALID;
  }
  TRASE_CHECK(hipSetDevice(device));
  // the library's own layout of a sort of `cap` items, then the two device words of the call
  SortBufs s{};
  uint32_t *n_dev = nullptr, *flag_dev = nullptr;
  auto layout = [&](void* ws) {
    WsCursor w(ws);
    sort_layout(w, s, cap, SORT_ALL, digit_bits, hist_copies);
    n_dev = w.take<uint32_t>(1);
    flag_dev = w.take<uint32_t>(1);
    return w.bytes();
  };
  const size_t bytes = layout(nullptr);
  DevBlock blk;
  TRASE_CHECK(hipMalloc(&blk.p, bytes));
  layout(blk.p);
  // histograms and digit totals start as garbage: the sort must not rely on what an earlier call left there
  TRASE_CHECK(hipMemsetAsync(blk.p, 0xCD, bytes, stream));
  const size_t cb = sizeof(uint32_t) * (size_t)cap;
  TRASE_CHECK(hipMemsetD32Async((hipDeviceptr_t)s.keys[start ^ 1], (int)sentinel, cap, stream));
  TRASE_CHECK(hipMemsetD32Async((hipDeviceptr_t)s.vals[start ^ 1], (int)sentinel, cap, stream));
  TRASE_CHECK(hipMemcpyAsync(s.keys[start], keys, cb, hipMemcpyDeviceToDevice, stream));
  if (vals) TRASE_CHECK(hipMemcpyAsync(s.vals[start], vals, cb, hipMemcpyDeviceToDevice, stream));
  else TRASE_CHECK(hipMemsetD32Async((hipDeviceptr_t)s.vals[start], (int)sentinel, cap, stream));
  TRASE_CHECK(hipMemcpyAsync(n_dev, &n, sizeof(n), hipMemcpyHostToDevice, stream));
  TRASE_CHECK(hipMemsetAsync(flag_dev, 0, sizeof(uint32_t), stream));
  const LaunchCtx c{stream, 0, 0};
  int out_idx = -1;
  const int rc = radix_sort_pairs(c, s, n_dev, cap, bit_lo, bit_hi, vals == nullptr, &out_idx, digit_bits, start, flag_key,
                                  use_flag ? flag_dev : nullptr);
  if (rc != TRASE_OK) { hipStreamSynchronize(stream); return rc; }
  uint32_t flag = 0;
  TRASE_CHECK(hipMemcpyAsync(keys_out, s.keys[out_idx], cb, hipMemcpyDeviceToDevice, stream));
  TRASE_CHECK(hipMemcpyAsync(vals_out, s.vals[out_idx], cb, hipMemcpyDeviceToDevice, stream));
  TRASE_CHECK(hipMemcpyAsync(&flag, flag_dev, sizeof(flag), hipMemcpyDeviceToHost, stream));
  TRASE_CHECK(hipStreamSynchronize(stream));
  result[0] = (uint32_t)out_idx;
  result[1] = flag;
  result[2] = radix_sort_is_short(rs_blocks(cap), s.hist_copies, radix_passes(bit_lo, bit_hi, digit_bits)) ? 1u : 0u;
  return TRASE_OK;
}

extern "C" int trase_selftest_tile_ranges(const uint32_t* keys, uint32_t n, uint32_t cap, int32_t T, int32_t clear,
                                          uint32_t* ranges, uint32_t* dbg, int32_t device, trase_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!keys || !ranges || !dbg || T < 1) {
    set_error("trase_selftest_tile_ranges: bad arguments");
    return TRASE_ERR_INVALID;
  }
  TRASE_CHECK(hipSetDevice(device));
  DevBlock blk;                                   // {n, dbg[3]}
  TRASE_CHECK(hipMalloc(&blk.p, 4 * sizeof(uint32_t)));
  uint32_t* w = (uint32_t*)blk.p;
  const uint32_t init[4] = {n, 0u, 0u, 0u};
  TRASE_CHECK(hipMemcpyAsync(w, init, sizeof(init), hipMemcpyHostToDevice, stream));
  const LaunchCtx c{stream, 0, 0};
  const int rc = launch_tile_ranges(c, keys, w, cap, (uint2*)ranges, T, w + 1, clear != 0);
  if (rc != TRASE_OK) { hipStreamSynchronize(stream); return rc; }
  TRASE_CHECK(hipMemcpyAsync(dbg, w + 1, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  TRASE_CHECK(hipStreamSynchronize(stream));
  return TRASE_OK;
}

extern "C" int trase_selftest_zero_bytes(void* p, size_t bytes, int32_t device, trase_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  const int rc = launch_zero_bytes(p, bytes, stream);
  if (rc != TRASE_OK) return rc;
  TRASE_CHECK(hipGetLastError());
  TRASE_CHECK(hipStreamSynchronize(stream));
  return TRASE_OK;
}

// ---- test entry points of the live compaction and the tile scan (binning.hip) ---------------------------------------------------
namespace {
// the geom and the pre workspace of P Gaussians in one allocation, carved by the library's own walks
struct ScanWs {
  GeomBuf g{};
  PreBuf t{};
  size_t geom_b = 0, bytes = 0;
  void carve(void* base, int P) {
    geom_b = geom_layout(base, P, g);
    bytes = geom_b + pre_layout(base ? (void*)((uintptr_t)base + geom_b) : nullptr, P, t);
  }
};
int copy_header(const uint32_t* hdr, uint32_t* out5, hipStream_t stream) {
  uint32_t h[HDR_WORDS];
  TRASE_CHECK(hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, stream));
  TRASE_CHECK(hipStreamSynchronize(stream));
  out5[0] = h[HDR_R]; out5[1] = h[HDR_OVERFLOW]; out5[2] = h[HDR_R_EFF]; out5[3] = h[HDR_PACK]; out5[4] = h[HDR_WORDS - 1];
  return TRASE_OK;
}
}  // namespace

extern "C" int trase_selftest_compact_live(const uint32_t* tiles, const uint32_t* keys, int32_t P, uint32_t* keys_out,
                                           uint32_t* ids_out, uint32_t* live_ids_out, uint32_t* hdr_out, int32_t device,
                                           trase_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!tiles || !keys || !keys_out || !ids_out || !live_ids_out || !hdr_out || P < 1) {
    set_error("trase_selftest_compact_live: bad arguments");
    return TRASE_ERR_INVALID;
  }
  TRASE_CHECK(hipSetDevice(device));
  ScanWs w;
  w.carve(nullptr, P);
  DevBlock blk;
  TRASE_CHECK(hipMalloc(&blk.p, w.bytes));
  w.carve(blk.p, P);
  // everything starts as garbage: the block counts, the header, the three result arrays
  TRASE_CHECK(hipMemsetAsync(blk.p, 0xCD, w.bytes, stream));
  const size_t pb = sizeof(uint32_t) * (size_t)P;
  TRASE_CHECK(hipMemcpyAsync(w.g.tiles, tiles, pb, hipMemcpyDeviceToDevice, stream));
  TRASE_CHECK(hipMemcpyAsync(w.t.sort.keys[1], keys, pb, hipMemcpyDeviceToDevice, stream));
  const LaunchCtx c{stream, 0, 0};
  const int rc = launch_compact_live(c, w.g, P, w.t, w.t.sort.keys[1], w.t.sort.keys[0], w.t.sort.vals[0]);
  if (rc != TRASE_OK) { hipStreamSynchronize(stream); return rc; }
  TRASE_CHECK(hipMemcpyAsync(keys_out, w.t.sort.keys[0], pb, hipMemcpyDeviceToDevice, stream));
  TRASE_CHECK(hipMemcpyAsync(ids_out, w.t.sort.vals[0], pb, hipMemcpyDeviceToDevice, stream));
  TRASE_CHECK(hipMemcpyAsync(live_ids_out, w.t.live_ids, pb, hipMemcpyDeviceToDevice, stream));
  return copy_header(w.g.hdr, hdr_out, stream);
}

extern "C" int trase_selftest_scan_tiles(const uint32_t* tiles, const uint32_t* ids, const int32_t* radii, const float* xy,
                                         int32_t P, uint32_t n_live, uint32_t cap, int32_t pack_bits, int32_t gx, int32_t gy,
                                         uint32_t overflow_in, uint32_t* offsets_out, uint32_t* block_sums_out,
                                         uint32_t* hdr_out, int32_t device, trase_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!tiles || !ids || !radii || !xy || !offsets_out || !block_sums_out || !hdr_out || P < 1 || pack_bits < 0 || pack_bits > 31 ||
      gx < 1 || gy < 1) {
    set_error("trase_selftest_scan_tiles: bad arguments");
    return TRASE_ERR_INVALID;
  }
  TRASE_CHECK(hipSetDevice(device));
  ScanWs w;
  w.carve(nullptr, P);
  DevBlock blk;
  TRASE_CHECK(hipMalloc(&blk.p, w.bytes));
  w.carve(blk.p, P);
  TRASE_CHECK(hipMemsetAsync(blk.p, 0xCD, w.bytes, stream));
  const size_t pb = sizeof(uint32_t) * (size_t)P;
  TRASE_CHECK(hipMemcpyAsync(w.g.tiles, tiles, pb, hipMemcpyDeviceToDevice, stream));
  TRASE_CHECK(hipMemcpyAsync(w.t.sort.vals[0], ids, pb, hipMemcpyDeviceToDevice, stream));
  TRASE_CHECK(hipMemcpyAsync(w.g.xy, xy, 2 * sizeof(float) * (size_t)P, hipMemcpyDeviceToDevice, stream));
  // the two header words the scan reads: the length (depth ranks that exist) and the overflow word, whose bit 1 it must keep
  TRASE_CHECK(hipMemcpyAsync(w.g.hdr + (HDR_WORDS - 1), &n_live, sizeof(n_live), hipMemcpyHostToDevice, stream));
  TRASE_CHECK(hipMemcpyAsync(w.g.hdr + HDR_OVERFLOW, &overflow_in, sizeof(overflow_in), hipMemcpyHostToDevice, stream));
  const LaunchCtx c{stream, 0, 0};
  const int rc = launch_scan_tiles(c, w.g, w.t.sort.vals[0], P, w.t, cap, radii, gx, gy, pack_bits);
  if (rc != TRASE_OK) { hipStreamSynchronize(stream); return rc; }
  const int nblocks = (P + 1023) / 1024;
  TRASE_CHECK(hipMemcpyAsync(offsets_out, w.t.offsets, pb, hipMemcpyDeviceToDevice, stream));
  TRASE_CHECK(hipMemcpyAsync(block_sums_out, w.t.block_sums, sizeof(uint32_t) * (size_t)nblocks, hipMemcpyDeviceToDevice, stream));
  return copy_header(w.g.hdr, hdr_out, stream);
}
