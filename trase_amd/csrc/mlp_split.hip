// mlp_split.hip -- the deformation MLP's inference forward at near-fp32 accuracy on the bf16 matrix cores
// (trase_mlp_forward_split; precision="bf16x3" of trase_amd/deform.py).  The network and its call sites are those of mlp.hip.
//
// Arithmetic: every matrix operand v -- encoding, weights, post-ReLU activations, head inputs -- is carried as hi + lo with
// hi = bf16(v), lo = bf16(v - hi) (both round-to-nearest-even; v - hi is exact in fp32), 16 mantissa bits instead of 8.
// A product is hi.hi + hi.lo + lo.hi -- three v_mfma_f32_32x32x16_bf16 into one fp32 accumulator where mlp.hip issues one;
// lo.lo (2^-16 of the product) is dropped.  Biases are the accumulators' initial values (fp32), the head biases are added in
// fp32.  The same split the rasterizer's MFMA forward uses for its exponents (render_fwd_mf.hip).
//
// Organisation: activations through LDS, weights straight into registers, one kernel for the whole network.  mlp.hip's
// register-chained inference kernel keeps 64 rows x 256 columns of bf16 per wave in registers; twice that (hi and lo) does not fit
// in 512.  Here
//   * a WORKGROUP (4 waves, one per SIMD) owns SP_ROWS = 64 rows (two MFMA row groups of 32); wave w owns all 64 rows and the 64
//     output columns w*64.. of every layer: 64 accumulator registers;
//   * the activations live in LDS as two swizzled tiles (hi, lo: 2 x 32 KiB, act_off addressing), rewritten in place by the
//     epilogue (ReLU, split) between two barriers; the encoding is generated once, split, and parked as ready-made fragments
//     (24 KiB) for layers 0 and 5;
//   * the weights are ONE linear stream of 16-KiB slabs (one K-step of 16: hi and lo, [hi|lo][k/8][n][k%8]), written by the
//     pack kernel on every call in consumption order, heads last.  A wave loads the fragments of ITS columns (a quarter of each
//     slab) straight from global memory into registers, two K-steps at a time, a whole pair of MFMAs ahead of their use: nothing is staged in LDS, no two
//     waves load the same bytes, and inside a layer there is no barrier at all (a first version staged whole slabs through LDS
//     behind one barrier per K-step: the 16-KiB register-to-LDS store and the barrier made a K-step 1 400 cycles for 384 of
//     MFMAs -- 1.38 ms at 300 000 rows);
//   * per K-step a wave reads 4 activation fragments (ds_read_b128) and 4 weight fragments (global) for 12 MFMAs.
// LDS: 64 + 24 + 8 (fp32 biases) = 96 KiB per workgroup, so one workgroup per CU.
// Rows past N are computed from row N-1's inputs and never stored.
#include "common.h"
#include "mlp_enc.h"
#include <type_traits>

namespace trase {

constexpr int SP_WROWS = 32;                        // rows of an MFMA row group: the kernel's rows come in groups of 32
constexpr int SP_WCOLS = 64;                        // output columns per wave
constexpr int SP_ROWS = 64;                         // rows per workgroup
constexpr int SP_PE_KS = EMBP / 16;                 // 6 encoding K-steps
constexpr int SP_HID_KS = MW / 16;                  // 16 hidden K-steps
constexpr int SP_SLABS = SP_PE_KS + 6 * SP_HID_KS + (SP_PE_KS + SP_HID_KS);   // 124 K-steps of the eight hidden layers
constexpr int SP_SLAB_ELEMS = 2 * 2 * MW * 8;       // [hi|lo][k half][n][8] bf16: 16 KiB
constexpr int SP_PLANE = 2 * MW * 8;                // elements of a slab's hi (or lo) part
constexpr int SP_HEAD_ELEMS = SP_HID_KS * 2 * 2 * HEADP * 8;   // heads: [ks][hi|lo][k half][32][8]
static_assert(SP_HEAD_ELEMS == 2 * SP_SLAB_ELEMS, "the head weights travel as the stream's last two slabs");
constexpr int SP_STREAM_SLABS = SP_SLABS + 2;
static_assert(SP_PE_KS % 2 == 0 && SP_HID_KS % 2 == 0, "the K loop runs in pairs");

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// first slab of layer l in the stream
__host__ __device__ constexpr int sp_layer_slab0(int l) {
  return l == 0 ? 0 : (l <= SKIP ? SP_PE_KS + (l - 1) * SP_HID_KS : SP_PE_KS + (l - 1) * SP_HID_KS + SP_PE_KS);
}
static_assert(sp_layer_slab0(MD) == SP_SLABS, "stream length");

__device__ __forceinline__ void split_bf16(float v, __bf16& hi, __bf16& lo) {
  hi = (__bf16)v;
  lo = (__bf16)(v - (float)hi);
}

struct SpPackArgs {
  const float* w[MD];
  const float* w_warp; const float* b_warp; const float* w_rot; const float* b_rot; const float* w_scale; const float* b_scale;
  __bf16* stream; __bf16* w_head; float* b_head;
  int emb;               // input columns of layer 0: EMB_T or EMB_B
};

// one thread per weight element: blocks 0 .. SP_SLABS*16-1 write the slabs, the 32 blocks behind them the heads
__global__ __launch_bounds__(256) void mlp_pack_split_kernel(SpPackArgs a) {
  constexpr int SLAB_BLOCKS = SP_SLABS * (SP_PLANE / 256);
  if ((int)blockIdx.x < SLAB_BLOCKS) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int slab = idx / SP_PLANE, r = idx % SP_PLANE, h = r / (MW * 8), n = (r >> 3) & (MW - 1), e = r & 7;
    int l = 0;
    for (int k = 1; k < MD; ++k) if (slab >= sp_layer_slab0(k)) l = k;
    const int ks = slab - sp_layer_slab0(l);
    const int pe_ks = (l == 0 || l == SKIP) ? SP_PE_KS : 0;
    const int EMB = a.emb;
    const int kin = l == 0 ? EMB : (l == SKIP ? EMB + MW : MW);
    float v = 0.f;
    if (ks < pe_ks) {
      const int c = 16 * ks + 8 * h + e;           // encoding columns, zero-padded from EMB to EMBP
      if (c < EMB) v = a.w[l][(size_t)n * kin + c];
    } else {
      v = a.w[l][(size_t)n * kin + (l == SKIP ? EMB : 0) + 16 * (ks - pe_ks) + 8 * h + e];
    }
    __bf16 hi, lo;
    split_bf16(v, hi, lo);
    __bf16* o = a.stream + (size_t)slab * SP_SLAB_ELEMS + r;
    o[0] = hi; o[SP_PLANE] = lo;
  } else {
    const int idx = ((int)blockIdx.x - SLAB_BLOCKS) * 256 + threadIdx.x;     // 0 .. 16*2*32*8-1
    const int ks = idx >> 9, h = (idx >> 8) & 1, n = (idx >> 3) & 31, e = idx & 7, k = 16 * ks + 8 * h + e;
    float v = 0.f;
    if (n < 3) v = a.w_warp[n * MW + k];
    else if (n < 7) v = a.w_rot[(n - 3) * MW + k];
    else if (n < 10) v = a.w_scale[(n - 7) * MW + k];
    __bf16 hi, lo;
    split_bf16(v, hi, lo);
    __bf16* o = a.w_head + (size_t)ks * (4 * HEADP * 8) + h * (HEADP * 8) + n * 8 + e;
    o[0] = hi; o[2 * HEADP * 8] = lo;
    if (idx < HEADP) {
      float b = 0.f;
      if (idx < 3) b = a.b_warp[idx]; else if (idx < 7) b = a.b_rot[idx - 3]; else if (idx < 10) b = a.b_scale[idx - 7];
      a.b_head[idx] = b;
    }
  }
}

struct SpNet {
  const __bf16* stream;  // [SP_SLABS][hi|lo][k half][256][8], then the heads [16][hi|lo][k half][32][8]: rows 0-2 warp, 3-6
                         // rotation, 7-9 scaling, rest 0
  const float* b_head;   // [32]
  const float* b[MD];    // the caller's fp32 biases, read as they are
  const float* temb;     // is_blender: the 30 timenet outputs shared by all rows (columns 63..92); else nullptr
};

// the split fragments of encoding K-step KS for lane (m, h): columns 16 KS + 8 h .. + 7 of the lane's row
template <int KS>
__device__ __forceinline__ void sp_pe_fragment(int h, const float (&p)[4], bool blender, const float (&tb)[32], bf16x8& hi, bf16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int c = KS * 16 + 8 * hh + j;
      const float pv = pe_const(c, p[0], p[1], p[2], p[3], nullptr);
      if (c < 63) v[hh] = pv;
      else {
        const float tv = (c < EMB_B) ? tb[c - 63] : 0.f;
        v[hh] = blender ? tv : pv;
      }
    }
    __bf16 a, b;
    split_bf16(h ? v[1] : v[0], a, b);
    hi[j] = a; lo[j] = b;
  }
}

__global__ __launch_bounds__(256)
void mlp_fwd_split_kernel(SpNet net, const float* __restrict__ x, const float* __restrict__ t, int t_stride, int N,
                          float* __restrict__ d_xyz, float* __restrict__ d_rot, float* __restrict__ d_scale) {
  // one array, so that a fragment's address is ONE offset whichever part it lies in (element offsets of __bf16):
  //   act: hi, lo tiles [2][64 x 256], 64 KiB | s_pe: [row group][ks][hi|lo][lane][8], 24 KiB | biases (fp32), 8 KiB
  constexpr int ACT = 0, ACT_PLANE = SP_ROWS * MW, S_PE = 2 * ACT_PLANE;
  constexpr int S_BIAS = S_PE + 2 * SP_PE_KS * 2 * 512, LDS_ELEMS = S_BIAS + 2 * MD * MW;
  __shared__ __attribute__((aligned(16))) __bf16 lds[LDS_ELEMS];                          // 96 KiB
  float* const s_bias = reinterpret_cast<float*>(lds + S_BIAS);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = lane & 31, h = lane >> 5;
  const int row0 = blockIdx.x * SP_ROWS;

  // ---- weight stream: the wave's own fragments, global -> registers -----------------------------------------------------
  // K-step pair d = slabs 2 d, 2 d + 1; of each slab the wave needs the hi and lo fragments of its two 32-column blocks:
  // q[(i * 2 + nb) * 2 + hl] for slab i of the pair.  A lane's 16 bytes of a fragment: [hl][h][column][8].
  const __bf16* const gw = net.stream + h * (MW * 8) + (wave * SP_WCOLS + m) * 8;
  auto wload = [&](int d, bf16x8 (&q)[8]) {                   // past the end: the last pair again (unused)
    const __bf16* p = gw + (size_t)min(2 * d, SP_SLABS - 2) * SP_SLAB_ELEMS;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int hl = 0; hl < 2; ++hl)
          q[(i * 2 + nb) * 2 + hl] = *reinterpret_cast<const bf16x8*>(p + i * SP_SLAB_ELEMS + hl * SP_PLANE + nb * 256);
  };
  bf16x8 q0[8], q1[8];                                        // pair d travels in q0 (d even) or q1 (d odd)
  wload(0, q0);
  wload(1, q1);
  // the biases (fp32, as the caller holds them) into LDS
  for (int i = threadIdx.x; i < MD * MW; i += 256) s_bias[i] = net.b[i / MW][i % MW];

  // ---- the encoding of the 64 rows: wave w generates K-steps 3 (w / 2) .. + 2 of row group w % 2 -------------------------
  {
    const int rg = wave & 1, kh = wave >> 1;
    const int gm = min(row0 + rg * 32 + m, N - 1);
    float p[4];
    p[0] = x[3 * (size_t)gm]; p[1] = x[3 * (size_t)gm + 1]; p[2] = x[3 * (size_t)gm + 2]; p[3] = t[(size_t)gm * t_stride];
    const bool blender = net.temb != nullptr;
    float tb[32];                                  // is_blender: the 30 shared timenet outputs (scalar loads); else unused
    {
      const float* tp = blender ? net.temb : net.b_head;     // always a valid address: the loads need no branch
#pragma unroll
      for (int i = 0; i < 32; ++i) tb[i] = (i < EMB_B - 63) ? tp[i] : 0.f;
    }
    auto park = [&](auto ks_c) {
      constexpr int KS = decltype(ks_c)::value;
      bf16x8 hi, lo;
      sp_pe_fragment<KS>(h, p, blender, tb, hi, lo);
      *reinterpret_cast<bf16x8*>(lds + S_PE + ((rg * SP_PE_KS + KS) * 2 + 0) * 512 + lane * 8) = hi;
      *reinterpret_cast<bf16x8*>(lds + S_PE + ((rg * SP_PE_KS + KS) * 2 + 1) * 512 + lane * 8) = lo;
    };
    if (kh == 0) { park(std::integral_constant<int, 0>{}); park(std::integral_constant<int, 1>{}); park(std::integral_constant<int, 2>{}); }
    else { park(std::integral_constant<int, 3>{}); park(std::integral_constant<int, 4>{}); park(std::integral_constant<int, 5>{}); }
  }
  lds_barrier();                                   // the encoding fragments and the biases are readable

  f32x16 acc[2][2];                                // [row group][column block]
  // input fragment (row group rg) of K-step ks of a layer with emb_k encoding K-steps in front
  auto afrag = [&](int rg, int ks, int emb_k, int hl) -> bf16x8 {
    const int o = ks < emb_k ? S_PE + ((rg * SP_PE_KS + ks) * 2 + hl) * 512 + lane * 8
                             : ACT + hl * ACT_PLANE + act_off(rg * SP_WROWS + m, (ks - emb_k) * 16 + 8 * h);
    return *reinterpret_cast<const bf16x8*>(lds + o);
  };
  // the biases are the accumulators' initial values (lane (m, h), register 4 q + j <-> column 32 nb + 8 q + 4 h + j)
  auto acc_init = [&](int l) {
    const float* B = s_bias + l * MW + wave * SP_WCOLS + 4 * h;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 bias = *reinterpret_cast<const float4*>(B + nb * 32 + 8 * q);
#pragma unroll
        for (int rg = 0; rg < 2; ++rg) {
          acc[rg][nb][4 * q + 0] = bias.x; acc[rg][nb][4 * q + 1] = bias.y; acc[rg][nb][4 * q + 2] = bias.z; acc[rg][nb][4 * q + 3] = bias.w;
        }
      }
  };
  // epilogue of a layer: ReLU, split, this wave's 64 x 64 block of both tiles
  auto epilogue = [&]() {
#pragma unroll
    for (int rg = 0; rg < 2; ++rg)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bf16x4 vh, vl;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            __bf16 a, b;
            split_bf16(fmaxf(acc[rg][nb][4 * q + j], 0.f), a, b);
            vh[j] = a; vl[j] = b;
          }
          const int o = act_off(rg * 32 + m, wave * SP_WCOLS + nb * 32 + 8 * q + 4 * h);
          *reinterpret_cast<bf16x4*>(lds + ACT + o) = vh;
          *reinterpret_cast<bf16x4*>(lds + ACT + ACT_PLANE + o) = vl;
        }
  };
  // The stream is walked in ONE loop over its 62 K-step pairs, two per trip.  A pair: eight input fragments out of LDS, 24
  // MFMAs, then the request for pair d + 2 into the registers pair d leaves -- a whole pair of MFMAs (another wave's L2 round
  // trip and more) lies between a request and its use.  No barrier inside a layer: the waves share nothing but the tiles.
  // The layer a pair belongs to is wave-uniform bookkeeping (every layer has an even number of K-steps); behind a layer's last
  // pair: barrier (every wave has read the old tiles), epilogue, barrier (the new tiles are complete).
  int l = 0, ks = 0, emb_k = SP_PE_KS, steps = SP_PE_KS;
  acc_init(0);
  auto pair = [&](int d, bf16x8 (&q)[8]) {
    bf16x8 a[2][2][2];                             // [K-step of the pair][row group][hi|lo]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int rg = 0; rg < 2; ++rg)
#pragma unroll
        for (int hl = 0; hl < 2; ++hl) a[i][rg][hl] = afrag(rg, ks + i, emb_k, hl);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int term = 0; term < 3; ++term)         // lo.hi, hi.lo, hi.hi: consecutive MFMAs go to different accumulators
#pragma unroll
        for (int rg = 0; rg < 2; ++rg)
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) {
            const bf16x8 w = q[(i * 2 + nb) * 2 + (term == 0 ? 1 : 0)];
            const bf16x8 v = a[i][rg][term == 1 ? 1 : 0];
            acc[rg][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w, v, acc[rg][nb], 0, 0, 0);
          }
    wload(d + 2, q);
    ks += 2;
    if (ks == steps) {
      lds_barrier();
      epilogue();
      lds_barrier();
      ++l; ks = 0;
      emb_k = l == SKIP ? SP_PE_KS : 0; steps = emb_k + SP_HID_KS;
      if (l < MD) acc_init(l);
    }
  };
  static_assert(SP_SLABS % 4 == 0, "two K-step pairs per trip");
  for (int d = 0; d < SP_SLABS / 2; d += 2) {
    pair(d, q0);
    pair(d + 1, q1);
  }

  // ---- heads: one 32-wide output block (10 used) per 32 rows, by waves 0 and 1 (row groups 0 and 1) ---------------------
  if (wave >= 2) return;
  const __bf16* const hw = net.stream + (size_t)SP_SLABS * SP_SLAB_ELEMS + h * (HEADP * 8) + m * 8;    // [ks][hi|lo][k half][32][8]
  f32x16 hacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) hacc[r] = 0.f;
  bf16x8 hwf[SP_HID_KS][2];                        // all 32 head fragments are requested before the first is used: one round trip
#pragma unroll
  for (int k = 0; k < SP_HID_KS; ++k)
#pragma unroll
    for (int hl = 0; hl < 2; ++hl) hwf[k][hl] = *reinterpret_cast<const bf16x8*>(hw + k * (4 * HEADP * 8) + hl * (2 * HEADP * 8));
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < SP_HID_KS; ++k) {
    const bf16x8 whi = hwf[k][0], wlo = hwf[k][1];
    const bf16x8 ahi = afrag(wave, k, 0, 0), alo = afrag(wave, k, 0, 1);
    hacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo, ahi, hacc, 0, 0, 0);
    hacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, alo, hacc, 0, 0, 0);
    hacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, ahi, hacc, 0, 0, 0);
  }
  // the ten outputs of a row sit in two lanes (h = 0: outputs 0-3, 8, 9; h = 1: 4-7): one cross-half exchange of register 3
  // gives lane h = 0 the rows of d_xyz and d_scaling and lane h = 1 the row of d_rotation (mlp_fwd_blk_body of mlp.hip)
  const int grow = row0 + wave * 32 + m;
  float o[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) o[r] = hacc[r] + net.b_head[8 * (r >> 2) + 4 * h + (r & 3)];
  const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(o[3]), __float_as_uint(o[3]), false, false);
  const float other3 = __uint_as_float(h ? sw[0] : sw[1]);         // h = 0 receives output 7, h = 1 receives output 3
  if (grow < N) {
    if (h == 0) {
      float* px3 = d_xyz + (size_t)grow * 3;
      px3[0] = o[0]; px3[1] = o[1]; px3[2] = o[2];
      float* ps3 = d_scale + (size_t)grow * 3;
      ps3[0] = other3; ps3[1] = o[4]; ps3[2] = o[5];
    } else {
      *reinterpret_cast<float4*>(d_rot + (size_t)grow * 4) = make_float4(other3, o[0], o[1], o[2]);
    }
  }
}

struct SpWs { __bf16* stream; __bf16* w_head; float* b_head; };
static size_t sp_layout(void* ws, SpWs& f) {
  WsCursor c(ws);
  f.stream = c.take<__bf16>((size_t)SP_STREAM_SLABS * SP_SLAB_ELEMS);
  f.w_head = f.stream ? f.stream + (size_t)SP_SLABS * SP_SLAB_ELEMS : nullptr;      // the stream's last two slabs
  f.b_head = c.take<float>(HEADP);
  return c.bytes();
}
static size_t sp_ws_bytes() { SpWs f; return sp_layout(nullptr, f); }

}  // namespace trase

using namespace trase;

extern "C" {

int trase_mlp_split_ws_bytes(size_t* ws_bytes) {
  if (!ws_bytes) { set_error("trase_mlp_split_ws_bytes: null"); return TRASE_ERR_INVALID; }
  *ws_bytes = sp_ws_bytes();
  return TRASE_OK;
}

int trase_mlp_forward_split(const TraseMlpWeights* w, const float* x, const float* t, int32_t t_stride, int32_t N,
                            float* d_xyz, float* d_rotation, float* d_scaling, void* ws, size_t ws_bytes, int32_t device,
                            trase_stream_t stream_) {
  const char* who = "trase_mlp_forward_split";
  // every refusal comes before the device is touched
  if (!w) { set_error("%s: null weights", who); return TRASE_ERR_INVALID; }
  if (N < 0) { set_error("%s: bad arguments (N %d)", who, N); return TRASE_ERR_INVALID; }
  if (w->variant != 0) { set_error("%s: variant must be 0", who); return TRASE_ERR_INVALID; }
  if (w->D != MD || w->W != MW || w->xyz_multires != 10 || w->is_6dof || (w->is_blender ? w->t_multires != 6 : w->t_multires != 10)) {
    set_error("%s: only DeformNetwork(D=8, W=256, multires=10, not 6dof) with t_multires=10 (default) or "
              "is_blender (t_multires=6, timenet) is compiled in", who);
    return TRASE_ERR_INVALID;
  }
  if (N == 0) return TRASE_OK;
  for (int l = 0; l < MD; ++l)
    if (!w->weight[l] || !w->bias[l]) { set_error("%s: null layer %d", who, l); return TRASE_ERR_INVALID; }
  if (!w->w_warp || !w->b_warp || !w->w_rotation || !w->b_rotation || !w->w_scaling || !w->b_scaling) {
    set_error("%s: null head", who); return TRASE_ERR_INVALID;
  }
  if (!x || !t || !d_xyz || !d_rotation || !d_scaling) { set_error("%s: null pointer", who); return TRASE_ERR_INVALID; }
  if (!ws || ws_bytes < sp_ws_bytes()) { set_error("%s: workspace too small (%zu bytes, need %zu)", who, ws_bytes, sp_ws_bytes()); return TRASE_ERR_INVALID; }
  if (t_stride < 0 || (w->is_blender && t_stride != 0)) {
    set_error("%s: t_stride must be >= 0; is_blender takes the timenet output (30 floats) with t_stride 0", who); return TRASE_ERR_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRASE_CHECK(hipSetDevice(device));
  SpWs f; sp_layout(ws, f);
  SpPackArgs pa;
  SpNet net;
  for (int l = 0; l < MD; ++l) { pa.w[l] = w->weight[l]; net.b[l] = w->bias[l]; }
  pa.w_warp = w->w_warp; pa.b_warp = w->b_warp; pa.w_rot = w->w_rotation; pa.b_rot = w->b_rotation;
  pa.w_scale = w->w_scaling; pa.b_scale = w->b_scaling;
  pa.stream = f.stream; pa.w_head = f.w_head; pa.b_head = f.b_head;
  pa.emb = w->is_blender ? EMB_B : EMB_T;
  net.stream = f.stream; net.b_head = f.b_head;
  net.temb = w->is_blender ? t : nullptr;                  // t = the 30 timenet outputs shared by all rows
  TRASE_LAUNCH("mlp_pack_split", stream, 0, mlp_pack_split_kernel, dim3(SP_SLABS * (SP_PLANE / 256) + SP_HEAD_ELEMS / 2 / 256), dim3(256), 0, pa);
  TRASE_LAUNCH("mlp_fwd_split", stream, 0, mlp_fwd_split_kernel, dim3((N + SP_ROWS - 1) / SP_ROWS), dim3(256), 0, net, x, t, t_stride, N,
               d_xyz, d_rotation, d_scaling);
  return TRASE_OK;
}

}  // extern "C"
