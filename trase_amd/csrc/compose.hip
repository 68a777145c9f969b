// compose.hip -- the reference's render_composite without its ~40 torch launches (gaussian_renderer/__init__.py:251-331 and
// the rigid-edit helpers :158-249): the parts of a composited scene (a background model, a masked / deformed / rescaled /
// rotated / translated dynamic model, ...) are written straight from their RAW parameters into the six operator-level input
// tensors of the rasterizer, one launch per part at that part's row offset.
//
// A block of 256 threads owns 256 consecutive OUTPUT rows of the part:
//   1. thread t resolves the source row of output row t (rows[] or the identity) into LDS; an entry outside [0, n) becomes -1
//      and is never dereferenced -- its whole output row is zeros (zero opacity and scale: a null Gaussian);
//   2. thread t computes the 11 small values of its row (compose_math.h) and stores them;
//   3. the 192-byte SH row and the 4 F-byte feature row are moved by ALL lanes over consecutive 16-byte pieces of the block's
//      contiguous output range (a wave stores 1 KB runs); the sources are contiguous too when rows == NULL, row-sized runs
//      under a gather.  features_rest rows are 180 bytes, so their 16-byte alignment changes from row to row: the SH pieces
//      are read as four dwords (adjacent lanes, adjacent addresses) and stored as one float4.
// About 364 bytes read and 364 written per row; nothing else.  No atomics: bitwise reproducible.
#include "common.h"
#include "compose_math.h"

namespace trase {

constexpr int CMP_THREADS = 256;
constexpr int CMP_MAX_PARTS = 8;
constexpr int CMP_MAX_F = 64;

struct ComposeArgs {
  const float* xyz; const float* scaling; const float* rotation; const float* opacity;
  const float* f_dc; const float* f_rest; const float* feat;
  const int64_t* rows;
  const float* d_xyz; const float* d_rotation; const float* d_scaling;
  int n, m, F;
  float* means; float* scales; float* rots; float* opac; float* shs; float* objs;     // already advanced to the part's first row
  ComposeEdit edit;
};

__global__ __launch_bounds__(CMP_THREADS) void compose_part_kernel(ComposeArgs a) {
  __shared__ int src_s[CMP_THREADS];
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * CMP_THREADS;
  const int nrows = imin(CMP_THREADS, a.m - row0);
  const int row = row0 + t;
  int src = -1;
  if (t < nrows) src = a.rows ? compose_source_row(a.rows[row], a.n) : row;     // rows == NULL: m == n (checked by the host)
  src_s[t] = src;
  if (t < nrows) {
    ComposeSmall o;
    if (src >= 0) {
      const size_t s3 = 3 * (size_t)src;
      const float4 q = reinterpret_cast<const float4*>(a.rotation)[src];
      const float qv[4] = {q.x, q.y, q.z, q.w};
      float dq[4] = {0.f, 0.f, 0.f, 0.f};                     // (always passed: a pointer chosen at run time would live in scratch)
      if (a.d_rotation) {
        const float4 d = reinterpret_cast<const float4*>(a.d_rotation)[src];
        dq[0] = d.x; dq[1] = d.y; dq[2] = d.z; dq[3] = d.w;
      }
      compose_row(a.xyz + s3, a.scaling + s3, qv, a.opacity[src], a.d_xyz ? a.d_xyz + s3 : nullptr,
                  a.d_scaling ? a.d_scaling + s3 : nullptr, dq, a.edit, o);
    } else {
      compose_zero(o);
    }
    const size_t r3 = 3 * (size_t)row;
    a.means[r3] = o.mean[0]; a.means[r3 + 1] = o.mean[1]; a.means[r3 + 2] = o.mean[2];
    a.scales[r3] = o.scale[0]; a.scales[r3 + 1] = o.scale[1]; a.scales[r3 + 2] = o.scale[2];
    reinterpret_cast<float4*>(a.rots)[row] = make_float4(o.rot[0], o.rot[1], o.rot[2], o.rot[3]);
    a.opac[row] = o.opacity;
  }
  __syncthreads();
  // SH rows: 12 float4 per row
  {
    float4* out = reinterpret_cast<float4*>(a.shs) + 12 * (size_t)row0;
    const int total = 12 * nrows;
    for (int k = t; k < total; k += CMP_THREADS) {
      const int r = k / 12, e = 4 * (k - 12 * r);
      const int s = src_s[r];
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (s >= 0) {
        v.x = compose_sh_element(a.f_dc, a.f_rest, s, e);
        v.y = compose_sh_element(a.f_dc, a.f_rest, s, e + 1);
        v.z = compose_sh_element(a.f_dc, a.f_rest, s, e + 2);
        v.w = compose_sh_element(a.f_dc, a.f_rest, s, e + 3);
      }
      out[k] = v;
    }
  }
  // feature rows, copied as they are (render_composite does not normalise them)
  if (a.F > 0) {
    if ((a.F & 3) == 0) {
      const int per = a.F >> 2;
      float4* out = reinterpret_cast<float4*>(a.objs) + (size_t)per * row0;
      const float4* in = reinterpret_cast<const float4*>(a.feat);
      const int total = per * nrows;
      for (int k = t; k < total; k += CMP_THREADS) {
        const int r = k / per, j = k - per * r;
        const int s = src_s[r];
        out[k] = s >= 0 ? in[(size_t)per * s + j] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    } else {
      float* out = a.objs + (size_t)a.F * row0;
      const int total = a.F * nrows;
      for (int k = t; k < total; k += CMP_THREADS) {
        const int r = k / a.F, j = k - a.F * r;
        const int s = src_s[r];
        out[k] = s >= 0 ? a.feat[(size_t)a.F * s + j] : 0.f;
      }
    }
  }
}

}  // namespace trase

using namespace trase;

extern "C" {

int trase_compose_sizes(const int32_t* counts, int32_t n_parts, int32_t F, int64_t* offsets_out) {
  if (!counts || !offsets_out || n_parts < 1 || n_parts > CMP_MAX_PARTS || F < 0 || F > CMP_MAX_F) {
    set_error("trase_compose_sizes: need 1 <= parts <= %d, 0 <= F <= %d (got %d parts, F %d)", CMP_MAX_PARTS, CMP_MAX_F, n_parts, F);
    return TRASE_ERR_INVALID;
  }
  int64_t total = 0;
  for (int p = 0; p < n_parts; ++p) {
    if (counts[p] < 0) { set_error("trase_compose_sizes: part %d has %d rows", p, counts[p]); return TRASE_ERR_INVALID; }
    offsets_out[p] = total;
    total += counts[p];
  }
  offsets_out[n_parts] = total;
  if (total >= ((int64_t)1 << 31) / 64) {                 // 48 * P and F * P stay below 2^31 (the rasterizer's own limit is lower)
    set_error("trase_compose_sizes: %lld rows in all, the limit is 2^25 - 1", (long long)total);
    return TRASE_ERR_INVALID;
  }
  return TRASE_OK;
}

int trase_compose_part(const TraseComposePart* part, int64_t row_offset, int64_t P_total, float* means3D, float* scales,
                       float* rotations, float* opacities, float* shs, float* sh_objs, int32_t device, trase_stream_t stream_) {
  if (!part) { set_error("trase_compose_part: null part"); return TRASE_ERR_INVALID; }
  const TraseComposePart& p = *part;
  if (p.n < 0 || p.m < 0 || p.F < 0 || p.F > CMP_MAX_F || p.edit_mode < 0 || p.edit_mode > 2 || row_offset < 0 ||
      row_offset + p.m > P_total || P_total >= ((int64_t)1 << 31) / 64 || (!p.rows && p.m != p.n)) {
    set_error("trase_compose_part: bad arguments (n %d, m %d, F %d, edit_mode %d, row offset %lld of %lld; without rows m must be n)",
              p.n, p.m, p.F, p.edit_mode, (long long)row_offset, (long long)P_total);
    return TRASE_ERR_INVALID;
  }
  if (p.m == 0) return TRASE_OK;
  if (!means3D || !scales || !rotations || !opacities || !shs || (p.F > 0 && !sh_objs)) {
    set_error("trase_compose_part: null output");
    return TRASE_ERR_INVALID;
  }
  if (p.n > 0 && (!p.xyz || !p.scaling || !p.rotation || !p.opacity || !p.features_dc || !p.features_rest ||
                  (p.F > 0 && !p.gaussian_features))) {
    set_error("trase_compose_part: null parameter");
    return TRASE_ERR_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  ComposeArgs a;
  a.xyz = p.xyz; a.scaling = p.scaling; a.rotation = p.rotation; a.opacity = p.opacity;
  a.f_dc = p.features_dc; a.f_rest = p.features_rest; a.feat = p.gaussian_features;
  a.rows = p.rows; a.d_xyz = p.d_xyz; a.d_rotation = p.d_rotation; a.d_scaling = p.d_scaling;
  a.n = p.n; a.m = p.m; a.F = p.F;
  const size_t o = (size_t)row_offset;
  a.means = means3D + 3 * o; a.scales = scales + 3 * o; a.rots = rotations + 4 * o; a.opac = opacities + o;
  a.shs = shs + 48 * o; a.objs = p.F > 0 ? sh_objs + (size_t)p.F * o : nullptr;
  a.edit.mode = p.edit_mode; a.edit.s = p.scale_factor;
  for (int k = 0; k < 9; ++k) a.edit.R[k] = p.R[k];
  for (int k = 0; k < 4; ++k) a.edit.q[k] = p.q_edit[k];
  for (int k = 0; k < 3; ++k) a.edit.t[k] = p.offset[k];
  TRASE_LAUNCH("compose_part", stream, 0, compose_part_kernel, dim3((p.m + CMP_THREADS - 1) / CMP_THREADS), dim3(CMP_THREADS), 0, a);
  return TRASE_OK;
}

}  // extern "C"
