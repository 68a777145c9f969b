/*
 * trase_rast.h -- C ABI of the MI355X-native TRASE rasterizer path.
 *
 * Drop-in boundary for the one hot path of yunjinli/TRASE: the native operator
 * behind gaussian_renderer.render().  The reference binds this path through a
 * pybind11/torch CUDA extension (un-vendored submodule, .gitmodules:4-6):
 *
 *   diff_gaussian_rasterization.GaussianRasterizationSettings   gaussian_renderer/__init__.py:58-71
 *   diff_gaussian_rasterization.GaussianRasterizer.forward      gaussian_renderer/__init__.py:137-146
 *   (its autograd backward, triggered by loss.backward())       train.py:299
 *   simple_knn._C.distCUDA2                                     scene/gaussian_model.py:237
 *
 * This header is the C-level equivalent: plain pointers and sizes, no torch
 * types.  All pointers named "device" are HIP device pointers valid on
 * `settings.device`; every call enqueues work on the caller's `stream` and
 * returns without synchronising unless stated.  The library allocates nothing
 * persistent; every call works on the caller's workspaces only and the entry
 * points are re-entrant (PyTorch calls the backward from an autograd worker
 * thread).  Process-wide state is limited to the last-error string (thread-local)
 * and the opt-in profiler (trase_prof_enable; mutex-guarded event records).  The
 * Python wrapper's policy (capacity, variant, strip: trase_amd/rasterizer.py) is
 * per process; a backward always uses what its forward captured.
 *
 * Return codes: 0 ok; <0 invalid argument / HIP error (see trase_strerror);
 * >0 is never returned by enqueue calls (capacity overflow is reported through
 * trase_rast_status, because it is only known on the device).
 */
#ifndef TRASE_RAST_H
#define TRASE_RAST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* trase_stream_t; /* hipStream_t */

enum {
  TRASE_OK = 0,
  TRASE_ERR_INVALID = -1,     /* bad argument combination (mirrors the reference's ValueError cases) */
  TRASE_ERR_UNSUPPORTED = -2, /* e.g. feature width not compiled in */
  TRASE_ERR_WORKSPACE = -3,   /* workspace too small */
  TRASE_ERR_HIP = -4          /* a HIP call failed; message via trase_last_error() */
};

/* GaussianRasterizationSettings (12 fields, gaussian_renderer/__init__.py:58-71).
 * The tensors of the reference record (bg, viewmatrix, projmatrix, campos) stay
 * on the device and are read by the kernels -- no D2H copy.  Matrices are the
 * transposed (row-vector) forms of scene/cameras.py:76-78: flat[4*col+row]. */
typedef struct TraseRastSettings {
  int32_t image_height;
  int32_t image_width;
  float tanfovx;
  float tanfovy;
  const float* bg;         /* device, 3 floats  */
  float scale_modifier;
  const float* viewmatrix; /* device, 16 floats */
  const float* projmatrix; /* device, 16 floats */
  int32_t sh_degree;       /* active degree 0..3 */
  const float* campos;     /* device, 3 floats  */
  int32_t prefiltered;
  int32_t debug;           /* !=0: synchronise + check after every kernel */
  int32_t device;          /* HIP device ordinal of all pointers and of `stream` */
  int32_t variant;         /* 0 = default; a bit set of TraseVariant (below): lineage switches, backward scope, the
                            * VALU cross-check kernels, the list-value form */
  /* Tile-row strip (second multi-GPU axis, SURVEY.md 8e: one view sharded over ranks by rows of 16x16 tiles).  Rows
   * [tile_row_begin, tile_row_end) are binned, composited and differentiated; pixels outside the strip are not written,
   * per-Gaussian gradients are this strip's partial sums (the ranks' strips add up to the full gradient), radii stay
   * whole-image.  begin == end == 0 means the whole image. */
  int32_t tile_row_begin;
  int32_t tile_row_end;
  float feat_bg;           /* background value of every feature channel; read only when variant & TRASE_VARIANT_FEATS_BG */
  int32_t reserved0;
} TraseRastSettings;

/* Bits of TraseRastSettings.variant.  Every other bit is ignored. */
typedef enum TraseVariant {
  /* -- lineage switches (the three places the absent fork of the CUDA extension is most likely to
   *    differ from the public lineage; each flips the HIP kernels AND oracle/raster_oracle.py's OracleOptions) -- */
  TRASE_VARIANT_DEPTH_GRAD = 0x100,          /* dL_ddepth is honoured (lineage: the depth output carries no gradient) */
  TRASE_VARIANT_FEATS_BG = 0x10000,          /* feats[c] += T_final * feat_bg */
  TRASE_VARIANT_DEPTH_NORM = 0x20000,        /* depth = sum(w z) / (1 - T_final) */
  /* -- backward scope -- */
  TRASE_VARIANT_FEATURES_ONLY_BWD = 0x400,   /* F = 32: only dL/dsh_objs is produced (FEATURE state once densification has
                                              * ended); every other gradient is written as zeros */
  /* -- cross-check formulations (same results to fp32 rounding; the tests compare the MFMA kernels against them) -- */
  TRASE_VARIANT_VALU_BACKWARD = 0x40,        /* packed-FP32 compositing backward (render_bwd_gs.hip) also for F = 32 (ignored under
                                              * TRASE_VARIANT_FEATURES_ONLY_BWD: that scope exists in the MFMA backward only) */
  TRASE_VARIANT_VALU_FORWARD = 0x2000,       /* packed-FP32 compositing forward (render.hip) also for F = 32 */
  TRASE_VARIANT_SLOT_LISTS = 0x100000,       /* sub-tile lists always carry emit-order slots (default: packed (id, pair index)
                                              * values whenever every Gaussian has few enough pairs -- decided on the device,
                                              * results identical) */
  /* -- tile-row strips (tile_row_begin / tile_row_end set) -- */
  TRASE_VARIANT_DEPTH32 = 0x400000,          /* depth sort on the raw float32 depth bits (four 8-bit passes) instead of the default 27-bit
                                              * key (three 9-bit passes, exact for view depth < 13 107): selected by the caller after a
                                              * forward has raised bit 1 of the header's overflow word (a saturated depth key) */
  TRASE_VARIANT_FORWARD_ONLY = 0x800000,     /* a forward nobody will differentiate (torch.no_grad()): what only the backward reads -- per-Gaussian
                                              * colour / clamp arrays, per-pixel final transmittance and contributor count -- is not stored.  A
                                              * backward on such a forward's workspaces is refused */
  TRASE_VARIANT_SPARSE_STRIP_GRADS = 0x200000, /* trase_rast_backward_raw writes ONLY the gradient rows of the Gaussians that have a
                                              * pair in the strip (~1 / world of them); the caller guarantees that every other row
                                              * of the gradient tensors is zero -- persistent tensors, zero-filled once, whose
                                              * previously written rows trase_rast_zero_live_rows clears.  Default: dense (every
                                              * row written, zeros included) */
  /* -- diagnostics: compiled only into `make AB=1` builds of the library (-DTRASE_AB), ignored otherwise -- */
  TRASE_VARIANT_AB_TIMING = 0x1000,          /* phase cycle counters of the MFMA backward (geom header words 32..39) */
  TRASE_VARIANT_AB_COUNT = 0x8000,           /* lane-utilisation counters of the MFMA backward (header words 40..47) and K-step
                                              * counters of the MFMA forward (header words 48..49) */
  TRASE_VARIANT_AB_ORDER_IMAGE = 0x40000,    /* compositing kernels visit the sub-tiles in image order ... */
  TRASE_VARIANT_AB_ORDER_8 = 0x80000         /* ... in 8x8 blocks (default: 16x16 blocks) */
} TraseVariant;

/* Inputs of GaussianRasterizer.forward (gaussian_renderer/__init__.py:137-146).
 * Exactly one of shs/colors_precomp and one of (scales,rotations)/cov3D_precomp
 * is non-NULL, as in the reference.  All contiguous float32. */
typedef struct TraseRastInputs {
  int32_t P;                   /* number of Gaussians */
  int32_t M;                   /* SH coefficients stored per Gaussian (16 for degree 3); 0 if shs NULL */
  int32_t F;                   /* feature channels of sh_objs (32 in TRASE); 0 if sh_objs NULL */
  const float* means3D;        /* (P,3)   */
  const float* shs;            /* (P,M,3) coefficient-major */
  const float* sh_objs;        /* (P,1,F) */
  const float* colors_precomp; /* (P,3)   */
  const float* opacities;      /* (P,1)   */
  const float* scales;         /* (P,3)   */
  const float* rotations;      /* (P,4) (r,x,y,z), NOT assumed unit length */
  const float* cov3D_precomp;  /* (P,6)   */
} TraseRastInputs;

/* Outputs: the reference's 4-tuple (image, radii, feats, depth), channel-planar. */
typedef struct TraseRastOutputs {
  float* image;   /* (3,H,W) */
  int32_t* radii; /* (P,)    */
  float* feats;   /* (F,H,W) or NULL when F == 0 */
  float* depth;   /* (1,H,W) */
} TraseRastOutputs;

/* Caller-owned workspaces.  geom/bin/img are saved by the caller between
 * forward and backward (the reference saves geomBuffer/binningBuffer/imgBuffer
 * the same way).  pre is stage-1 scratch that must survive until stage 2 (its
 * size depends on P only); tmp is stage-2 scratch (size depends on capacity) and
 * doubles as the backward's scratch (bwd_tmp_bytes).  Only geom/bin/img sizes
 * depend on nothing else, so a caller may run stage 1, read the pair count with
 * trase_rast_status and only then allocate bin/tmp. */
typedef struct TraseRastWorkspace {
  void* geom; size_t geom_bytes;
  void* bin;  size_t bin_bytes;
  void* img;  size_t img_bytes;
  void* pre;  size_t pre_bytes;
  void* tmp;  size_t tmp_bytes;
  int64_t capacity;            /* max (tile,Gaussian) pairs `bin`/`tmp` were sized for */
} TraseRastWorkspace;

typedef struct TraseRastSizes {
  size_t geom_bytes, bin_bytes, img_bytes, pre_bytes, tmp_bytes, bwd_tmp_bytes;
} TraseRastSizes;

/* Cotangents in, gradients out (A4).  NULL cotangent == that output was unused
 * (ctx.set_materialize_grads(False) semantics); NULL gradient == not needed. */
typedef struct TraseRastGrads {
  const float* dL_dimage;   /* (3,H,W) or NULL */
  const float* dL_dfeats;   /* (F,H,W) or NULL */
  const float* dL_ddepth;   /* (1,H,W) or NULL (lineage: ignored unless settings.variant bit says so) */
  float* dL_dmeans3D;       /* (P,3)   */
  float* dL_dmeans2D;       /* (P,3) x,y = NDC-scaled screen gradient, z = 0 */
  float* dL_dshs;           /* (P,M,3) */
  float* dL_dsh_objs;       /* (P,1,F) */
  float* dL_dcolors;        /* (P,3)   */
  float* dL_dopacities;     /* (P,1)   */
  float* dL_dscales;        /* (P,3)   */
  float* dL_drotations;     /* (P,4)   */
  float* dL_dcov3D;         /* (P,6)   */
} TraseRastGrads;

/* Sizes of every workspace for P Gaussians, a W x H image, F feature channels
 * and room for `capacity` (tile,Gaussian) pairs. */
int trase_rast_sizes(int32_t P, int32_t W, int32_t H, int32_t F, int64_t capacity, TraseRastSizes* out);

/* Stage 1: per-Gaussian projection / EWA / colour + tile counting + depth sort.
 * Writes out->radii and the geom workspace (incl. the device-side pair count). */
int trase_rast_preprocess(const TraseRastSettings* s, const TraseRastInputs* in, const TraseRastOutputs* out,
                          const TraseRastWorkspace* ws, trase_stream_t stream);

/* Blocking read of {num_rendered, overflow, num_rendered_culled} from the geom
 * workspace (the reference's forward returns num_rendered the same way). */
int trase_rast_status(const TraseRastWorkspace* ws, int64_t status[3], trase_stream_t stream);

/* Byte offsets of the per-Gaussian arrays inside the geom workspace sized for P Gaussians (pure host
 * arithmetic): off[0] header (64 u32: [0] lineage pair count, [1] overflow flag, [2] binned pair count),
 * off[1] xy float2[P] (pixel centre), off[2] conic_opacity float4[P], off[3] rgb_depth float4[P] (.w = view-space
 * depth, the blend-order key), off[4] tiles u32[P], off[5] clamp bits u32[P].  Introspection for parity tests and
 * debugging -- the counterpart of reading the reference's geomBuffer; entries of culled Gaussians are undefined. */
int trase_rast_geom_layout(int32_t P, int64_t off[6]);
/* Byte offset, inside the geom workspace, of the (P, 16)-word geometry records ({x, y, first pair slot, radius}, conic + opacity,
 * colour + depth, ...): introspection for the tests (word 2 is the first emit-order slot of the Gaussian's pairs). */
int trase_rast_geom_record_offset(int32_t P, int64_t* off);

/* The same for the bin workspace of `capacity` pairs and T 8x8 sub-tiles: off[0] point_list u32[capacity], off[1] pair_slot
 * u32[capacity], off[2] ranges uint2[T + 1] ([begin, end) of every sub-tile's list, row-major over the sub-tile grid, then
 * the sentinel entry). */
int trase_rast_bin_layout(int64_t capacity, int32_t T, int64_t off[3]);

/* Stage 2: binning (tile lists in depth order) + alpha compositing. */
int trase_rast_render(const TraseRastSettings* s, const TraseRastInputs* in, const TraseRastOutputs* out,
                      const TraseRastWorkspace* ws, trase_stream_t stream);

/* Stage 1 + 2 back to back, no host synchronisation. */
int trase_rast_forward(const TraseRastSettings* s, const TraseRastInputs* in, const TraseRastOutputs* out,
                       const TraseRastWorkspace* ws, trase_stream_t stream);

/* Backward of trase_rast_forward; ws->tmp must hold bwd_tmp_bytes. */
int trase_rast_backward(const TraseRastSettings* s, const TraseRastInputs* in, const TraseRastOutputs* out,
                        const TraseRastWorkspace* ws, const TraseRastGrads* g, trase_stream_t stream);

/* ---- render() with the reference's A1 "prep" fused in --------------------------
 * Takes the RAW GaussianModel parameters (scene/gaussian_model.py:56-63) and the per-view deformation and
 * applies gaussian_renderer/__init__.py:82-121 inside the per-Gaussian kernels: means3D = _xyz + d_xyz,
 * scales = exp(_scaling) + d_scaling, rotations = normalize(_rotation) + d_rotation, opacity =
 * sigmoid(_opacity), shs = cat(_features_dc, _features_rest), sh_objs = f / (||f|| + 1e-9).  d_* may be
 * NULL (warm-up passes the float 0.0, train.py:192-193).  SH layout: features_dc (P,1,3), features_rest
 * (P,15,3).  featn is a caller-owned (P,F) buffer that must live until the backward. */
typedef struct TraseRastRawInputs {
  int32_t P;
  int32_t F;
  int32_t norm_features;            /* norm_gaussian_features flag of render() */
  const float* xyz;                 /* (P,3)    */
  const float* d_xyz;               /* (P,3) or NULL */
  const float* features_dc;         /* (P,1,3)  */
  const float* features_rest;       /* (P,15,3) */
  const float* opacity;             /* (P,1) logits */
  const float* scaling;             /* (P,3) log-scales */
  const float* d_scaling;           /* (P,3) or NULL */
  const float* rotation;            /* (P,4) raw quaternion */
  const float* d_rotation;          /* (P,4) or NULL */
  const float* gaussian_features;   /* (P,1,F) raw, or NULL when F == 0 */
  float* featn;                     /* (P,F) work buffer */
  /* render()'s other call patterns, fused as well (round 6; every pointer may be NULL = not used):
   *   colors_precomp   override_color= (gaussian_renderer/__init__.py:112-113; render.py:240,296,344, gui.py): (P,3) colours taken as
   *                    they are -- no SH evaluation, features_dc / features_rest are not read and may be NULL;
   *   mask             mask= (:123-135): (P) bytes, 0 removes the Gaussian from the view (the reference indexes every input by the
   *                    mask).  out->radii and every gradient stay FULL size (P rows; rows of removed Gaussians: radii 0, gradients
   *                    0 -- what the index's backward scatters); the caller compacts radii to the subset for render()'s dict;
   *   d_xyz_se3        is_6dof (:75-80): (P,4,4) row-major transforms, means3D = from_homogenous(M [xyz, 1]); replaces d_xyz;
   *   sh_dir_undeformed  != 0: pipe.convert_SHs_python (:103-108) -- the SH is evaluated in the direction of the UNDEFORMED xyz
   *                    (the Python fallback uses pc.get_xyz there), colour clamp as in the rasterizer. */
  const float* colors_precomp;
  const uint8_t* mask;
  const float* d_xyz_se3;
  int32_t sh_dir_undeformed;
  int32_t reserved1;
} TraseRastRawInputs;

typedef struct TraseRastRawGrads {
  const float* dL_dimage; const float* dL_dfeats; const float* dL_ddepth;   /* cotangents, NULL if unused */
  float* dL_dxyz; float* dL_dd_xyz; float* dL_dmeans2D;
  float* dL_dfeatures_dc; float* dL_dfeatures_rest; float* dL_dopacity;
  float* dL_dscaling; float* dL_dd_scaling; float* dL_drotation; float* dL_dd_rotation;
  float* dL_dgaussian_features;
  float* dL_dcolors_precomp;        /* (P,3), with colors_precomp */
  float* dL_dd_xyz_se3;             /* (P,4,4), with d_xyz_se3 */
} TraseRastRawGrads;

int trase_rast_preprocess_raw(const TraseRastSettings* s, const TraseRastRawInputs* raw, const TraseRastOutputs* out,
                              const TraseRastWorkspace* ws, trase_stream_t stream);
int trase_rast_render_raw(const TraseRastSettings* s, const TraseRastRawInputs* raw, const TraseRastOutputs* out,
                          const TraseRastWorkspace* ws, trase_stream_t stream);
int trase_rast_backward_raw(const TraseRastSettings* s, const TraseRastRawInputs* raw, const TraseRastOutputs* out,
                            const TraseRastWorkspace* ws, const TraseRastRawGrads* g, trase_stream_t stream);
/* trase_rast_preprocess_raw + trase_rast_render_raw in one call, for callers that know the capacity beforehand (the
 * sync-free policy): one boundary crossing per direction. */
int trase_rast_forward_raw(const TraseRastSettings* s, const TraseRastRawInputs* raw, const TraseRastOutputs* out,
                           const TraseRastWorkspace* ws, trase_stream_t stream);
/* Two views of the SAME Gaussians in one launch sequence (round 5; no counterpart in the reference, whose loop renders one view
 * per iteration, train.py:180).  Identical results to two trase_rast_forward_raw calls -- each view keeps its own settings,
 * per-view deformation (d_*), outputs and workspaces, and its backward is the ordinary trase_rast_backward_raw on those -- but the
 * two depth sorts, the latency-bound part of a view (twelve launches over 1.2 MB of keys at 300k Gaussians), are ONE sort of 2 P
 * keys with the view index in the sign bit of the float32 depth key.  `pair_ws`: scratch of trase_rast_pair_sizes(P) bytes, free
 * again when the call's work has run.  Whole-image views only (no tile-row strips); the sync-free capacity policy (both
 * workspaces sized by the caller beforehand). */
int trase_rast_pair_sizes(int32_t P, size_t* bytes);
int trase_rast_forward_raw_pair(const TraseRastSettings* s0, const TraseRastRawInputs* raw0, const TraseRastOutputs* out0,
                                const TraseRastWorkspace* ws0, const TraseRastSettings* s1, const TraseRastRawInputs* raw1,
                                const TraseRastOutputs* out1, const TraseRastWorkspace* ws1, void* pair_ws, size_t pair_bytes,
                                trase_stream_t stream);

/* Launch-graph replay (hipGraph) for small workloads, where the ~45 kernel launches of a direction cost more host time
 * than the kernels run (BASELINE configs 1 and 2).  With mode != 0, trase_rast_forward / _forward_raw / _backward /
 * _backward_raw capture their launch sequence once per distinct argument record (every scalar and every pointer of the
 * settings, inputs, outputs, workspace and gradient structs) on an internal stream and replay the instantiated graph on
 * the caller's stream when the same record comes back -- which it does in a training loop whose allocator hands out the
 * same blocks every iteration.  Only the sync-free entry points are graphed (nothing in them reads back to the host).
 * The cache holds up to 256 graphs and switches itself off when records stop repeating (a miss costs a capture).
 * mode: 0 = off, 1 = every call, 2 = auto -- calls of at most 200 000 Gaussians (environment TRASE_GRAPH_AUTO_P); the library
 * starts in mode 2 (environment TRASE_GRAPH = 0 | 1 | auto).  trase_rast_graph_stats: {hits, misses, cached, mode}. */
int trase_rast_graph_mode(int mode);
int trase_rast_graph_stats(int64_t stats[4]);

/* The same backward in two phases, for a view-parallel caller that starts exchanging the gradients of the first Gaussians
 * while the last ones are still being reduced (trase_amd/dp.py; the reference is single-process, train.py:303):
 *   _compose    the compositing backward over every sub-tile -- one gradient row per (sub-tile, Gaussian) pair in the
 *               workspace, no per-Gaussian output yet (only dL_dgaussian_features is zero-filled when dL_dfeats is NULL);
 *   _gaussians  the per-Gaussian tail for the ids [p_begin, p_end): sums their pair rows and writes THEIR entries of every
 *               gradient tensor in `g` (same pointers as for the whole call: the tensors' bases).  p_begin must be a
 *               multiple of 64, p_end a multiple of 64 or P.
 * _compose followed by _gaussians over a partition of [0, P) equals trase_rast_backward_raw bit for bit. */
int trase_rast_backward_raw_compose(const TraseRastSettings* s, const TraseRastRawInputs* raw, const TraseRastOutputs* out,
                                    const TraseRastWorkspace* ws, const TraseRastRawGrads* g, trase_stream_t stream);
/* Sparse strip gradients (TRASE_VARIANT_SPARSE_STRIP_GRADS): sets the rows of every non-NULL gradient tensor in `g` to zero for
 * the Gaussians that had a pair in the strip of the forward whose `geom` and `pre` workspaces are given -- i.e. exactly the rows
 * that forward's backward wrote.  Cost: what the strip holds, not what the scene does. */
int trase_rast_zero_live_rows(const TraseRastSettings* s, const TraseRastRawInputs* raw, const TraseRastWorkspace* ws,
                              const TraseRastRawGrads* g, trase_stream_t stream);
int trase_rast_backward_raw_gaussians(const TraseRastSettings* s, const TraseRastRawInputs* raw, const TraseRastOutputs* out,
                                      const TraseRastWorkspace* ws, const TraseRastRawGrads* g, int32_t p_begin, int32_t p_end,
                                      trase_stream_t stream);

/* simple_knn._C.distCUDA2 (scene/gaussian_model.py:237): mean squared distance
 * to the 3 nearest neighbours.  ws_bytes from trase_knn_sizes. */
int trase_knn_sizes(int32_t N, size_t* ws_bytes);
int trase_knn_dist2(const float* points, int32_t N, float* out, void* ws, size_t ws_bytes, int32_t device,
                    trase_stream_t stream);

/* pytorch3d.ops.knn_points replacement (scene/gaussian_model.py:88-92 K=16 self-KNN for feature
 * smoothing; render.py:222, gui.py:1048, utils/loss_utils.py:141,192 cross-KNN): for every point of
 * p1 the K (1 <= K <= 256) nearest points of p2, ascending by (squared distance, index); idx int64 (N1,K),
 * squared distances (N1,K); idx 0 / distance 0 where p2 has fewer than K points.  K <= 16 runs one thread
 * per query, a larger K one wave per query with its list in LDS.  Workspace: trase_knn_sizes(N2) for every K. */
int trase_knn_points(const float* p1, int32_t N1, const float* p2, int32_t N2, int32_t K, int64_t* idx,
                     float* dists, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);

/* ---- losses over a k-NN graph (utils/loss_utils.py:132-152 loss_reg_3d_feature, :179-221
 * loss_rigid_body_motion_reg_loss) without N x k x ... edge tensors --------------------------------------------
 * A graph is idx (N,k) int32: edge e = i*k + slot runs from row i to row idx[e]; N*k < 2^31.  An id outside [0,N)
 * is an edge to nowhere (it contributes nothing and is never dereferenced).
 * trase_graph_reverse transposes it: rev_edges (N*k) holds the edge numbers sorted stably by their target (so
 * ascending among the edges of one target), rev_ranges (N,2) the [begin,end) positions of every target's edges.
 * The backward passes gather over it instead of using float atomics, so they are bitwise reproducible. */
/* (named *_ws_bytes like trase_mlp_split_ws_bytes: the recorded table of the *_sizes functions, tests/golden/workspace_sizes.json,
 * pins the layouts that existed when it was written) */
int trase_graph_reverse_ws_bytes(int32_t N, int32_t k, size_t* ws_bytes);
int trase_graph_reverse(const int32_t* idx, int32_t N, int32_t k, int32_t* rev_ranges, int32_t* rev_edges, void* ws,
                        size_t ws_bytes, int32_t device, trase_stream_t stream);
/* The same transpose for a graph whose `rows` source rows point into `targets` target rows (rows, targets >= 1, rows*k < 2^31):
 * rev_ranges is (targets,2), rev_edges (rows*k); an id outside [0,targets) is an edge to nowhere.  With rows == targets the
 * results are those of trase_graph_reverse bit for bit. */
int trase_graph_reverse_to_ws_bytes(int32_t rows, int32_t k, int32_t targets, size_t* ws_bytes);
int trase_graph_reverse_to(const int32_t* idx, int32_t rows, int32_t k, int32_t targets, int32_t* rev_ranges, int32_t* rev_edges,
                           void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
/* Exact all-pairs top-k at both ends of the distance order without the M x N matrix (dense.hip): for every row of queries (M,D)
 * the k_near nearest and the k_far farthest rows of points (N,D), fp32, 1 <= D <= 64, 0 <= k_near, k_far <= 32 with one of them
 * positive and both <= N.  A squared distance is the chain s = fmaf(q_d - p_d, q_d - p_d, s) in dimension order; a NaN becomes
 * 0x7FC00000.  Near end: ascending (bits(d2) << 32) | id; far end: ascending (~bits(d2) << 32) | id (larger distance first, then
 * lower id); NaN ranks above +inf.  Outputs (M,k) fp32 squared distances and int64 ids; an end with k = 0 takes null pointers.
 * M = 0 launches nothing.  splits (may be null) receives the number of column ranges S; with S > 1 a merge launch follows. */
int trase_dense_topk_ws_bytes(int32_t M, int32_t N, int32_t D, int32_t k_near, int32_t k_far, size_t* ws_bytes, int32_t* splits);
int trase_dense_topk(const float* queries, int32_t M, const float* points, int32_t N, int32_t D, int32_t k_near, int32_t k_far,
                     float* near_d2, int64_t* near_idx, float* far_d2, int64_t* far_idx, void* ws, size_t ws_bytes, int32_t device,
                     trase_stream_t stream);
/* loss_feature3d: lambda_p mean over (i, slot < kp) of sigmoid(1 - c) + lambda_n mean over (i, slot >= kp) of sigmoid(c) with
 * c = u_i . u_j, u = f / max(|f|, 1e-8), j = idx[i,slot], idx (rows, kp + kn) int32: the kp nearest rows, then the kn farthest.
 * The forward writes u_tab (rows, DP), DP = 8 / 16 / 32 / 64 the padded D, and nrm (rows) for the backward, which also reads the
 * transpose of idx; loss and g_loss are device scalars.  1 <= rows < 2^25, D <= 64, 1 <= kp, kn <= 32. */
int trase_feature3d_ws_bytes(int32_t rows, size_t* ws_bytes);
int trase_feature3d_forward(const float* feats, const int32_t* idx, int32_t rows, int32_t D, int32_t kp, int32_t kn, float lambda_p,
                            float lambda_n, float* u_tab, float* nrm, float* loss, void* ws, size_t ws_bytes, int32_t device,
                            trase_stream_t stream);
int trase_feature3d_backward(const float* u_tab, const float* nrm, const int32_t* idx, const int32_t* rev_ranges,
                             const int32_t* rev_edges, int32_t rows, int32_t D, int32_t kp, int32_t kn, float lambda_p, float lambda_n,
                             const float* g_loss, float* g_feats, int32_t device, trase_stream_t stream);
/* loss_cls_3d: lambda / (S k C) sum over (s,slot,c) of p_s (log(p_s + 1e-10) - log(p_j + 1e-10)), p_s = pred[sample[s]], pred (N,C),
 * C <= 256, sample (S) and idx (S,k) int32 row numbers of pred.  The backward writes g_pred (N,C) from the transposes of idx
 * (rev_*: S rows into N targets) and of sample as an (S,1) graph (srev_*). */
int trase_cls3d_ws_bytes(int32_t S, int32_t C, size_t* ws_bytes);
int trase_cls3d_forward(const float* pred, const int32_t* sample, const int32_t* idx, int32_t S, int32_t N, int32_t C, int32_t k,
                        float lambda_val, float* loss, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_cls3d_backward(const float* pred, const int32_t* sample, const int32_t* idx, const int32_t* rev_ranges, const int32_t* rev_edges,
                         const int32_t* srev_ranges, const int32_t* srev_edges, int32_t S, int32_t N, int32_t C, int32_t k,
                         float lambda_val, const float* g_loss, float* g_pred, int32_t device, trase_stream_t stream);
/* loss = mean over (i,slot,d) of s_i (log(s_i + 1e-10) - log(s_j + 1e-10)), s = sigmoid(feats), feats (N,D), D <= 64.
 * The forward writes the tables s_tab, l_tab (N,D each) that the backward reads; loss and g_loss are device scalars.
 * Workspace: trase_feat3d_ws_bytes(N, D). */
int trase_feat3d_ws_bytes(int32_t N, int32_t D, size_t* ws_bytes);
int trase_feat3d_forward(const float* feats, const int32_t* idx, int32_t N, int32_t D, int32_t k, float* s_tab, float* l_tab,
                         float* loss, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_feat3d_backward(const float* s_tab, const float* l_tab, const int32_t* idx, const int32_t* rev_ranges,
                          const int32_t* rev_edges, int32_t N, int32_t D, int32_t k, const float* g_loss, float* g_feats,
                          int32_t device, trase_stream_t stream);
/* With e1 = p1[i] - p1[j], e2 = p2[i] - p2[j], j = idx[i,slot]:  S (N,3,3) = sum_slot e1 e2^T;
 * out (N) = sum_slot |e1 - R[i] e2|^2 with R (N,3,3).  The backward passes take the cotangents gS (N,3,3) / g (N)
 * and write g1, g2 (N,3) and gR (N,3,3). */
int trase_edge_moments_forward(const float* p1, const float* p2, const int32_t* idx, int32_t N, int32_t k, float* S,
                               int32_t device, trase_stream_t stream);
int trase_edge_moments_backward(const float* p1, const float* p2, const int32_t* idx, const int32_t* rev_ranges,
                                const int32_t* rev_edges, int32_t N, int32_t k, const float* gS, float* g1, float* g2,
                                int32_t device, trase_stream_t stream);
int trase_edge_residual_forward(const float* p1, const float* p2, const int32_t* idx, const float* R, int32_t N, int32_t k,
                                float* out, int32_t device, trase_stream_t stream);
int trase_edge_residual_backward(const float* p1, const float* p2, const int32_t* idx, const int32_t* rev_ranges,
                                 const int32_t* rev_edges, const float* R, int32_t N, int32_t k, const float* g, float* g1,
                                 float* g2, float* gR, int32_t device, trase_stream_t stream);
/* The rotation between the two edge sums without leaving the device code (trase_amd/csrc/rigid_math.h).
 * polar3: R (N,3,3) = V U^T of S (N,3,3) = U Sigma V^T, the orthogonal polar factor of S^T, det R = sign(det S) (+1 where det S
 * evaluates to 0); a non-finite S gives a NaN R.  The backward takes the cotangent gR and writes gS: the closed form through
 * (tr(H) I - H)^-1, H = R^T S^T, and ZERO for a degenerate row (sigma_2 + sigma_3 <= 12 * 2^-24 |S|_F).
 * rigid_fit: out (N) = sum_slot |e1 - R[i] e2|^2 with R[i] = polar3(sum_slot e1 e2^T) in one launch; R is written too, and
 * state (N, TRASE_RIGID_STATE_FLOATS) is what the backward reads: it takes the cotangent g (N) of out and writes g1, g2 (N,3),
 * the gradient through the rotation included.  A row is degenerate there when sigma_2 + sigma_3 <= 4 (k + 2) 2^-24 sum_slot |e1| |e2|. */
#define TRASE_RIGID_STATE_FLOATS 16
int trase_polar3_forward(const float* S, int32_t N, float* R, int32_t device, trase_stream_t stream);
int trase_polar3_backward(const float* S, const float* R, const float* gR, int32_t N, float* gS, int32_t device,
                          trase_stream_t stream);
int trase_rigid_fit_forward(const float* p1, const float* p2, const int32_t* idx, int32_t N, int32_t k, float* out, float* R,
                            float* state, int32_t device, trase_stream_t stream);
int trase_rigid_fit_backward(const float* p1, const float* p2, const int32_t* idx, const int32_t* rev_ranges,
                             const int32_t* rev_edges, const float* R, const float* state, const float* g, int32_t N, int32_t k,
                             float* g1, float* g2, int32_t device, trase_stream_t stream);

/* Deformation MLP (utils/time_utils.py:60-131 DeformNetwork.forward, reached through
 * scene/deform_model.py:34-35 DeformModel.step at train.py:202-204, render.py:195, gui.py:965).
 * Weights are the reference's nn.Linear parameters as they are (fp32, [out][in] row-major, device
 * pointers); they are re-packed to bf16 on every call.  trase_mlp_forward serves the no_grad call sites; the training pair is
 * declared further down. */
typedef struct TraseMlpWeights {
  int32_t D;             /* hidden layers (8) */
  int32_t W;             /* hidden width (256) */
  int32_t xyz_multires;  /* 10 -> 63 input channels */
  int32_t t_multires;    /* 10 -> 21 input channels; 6 with is_blender */
  int32_t is_blender;    /* 0: cat(PE(x), PE(t)), 84 inputs.  1 (D-NeRF, utils/time_utils.py:74-86): cat(PE(x),
                          * timenet(PE(t))), 93 inputs -- the caller evaluates the tiny timenet and passes its 30 outputs
                          * as `t` with t_stride 0 (train.py:190-202 feeds the same time to every row when is_blender) */
  int32_t is_6dof;       /* 1: the 3-vector head is a screw-axis branch (branch_w / branch_v); trase_amd/deform.py runs the network twice */
  int32_t variant;       /* reserved, must be 0 (the superseded kernel organisations it used to select are gone) */
  int32_t reserved;
  const float* weight[8];/* linear.{i}.weight: (256, 84|93) / (256, 256) / (256, 340|349) for the skip layer i = 5 */
  const float* bias[8];  /* linear.{i}.bias  : (256,) */
  const float* w_warp;     const float* b_warp;      /* gaussian_warp     (3,256), (3,) */
  const float* w_rotation; const float* b_rotation;  /* gaussian_rotation (4,256), (4,) */
  const float* w_scaling;  const float* b_scaling;   /* gaussian_scaling  (3,256), (3,) */
} TraseMlpWeights;

int trase_mlp_sizes(size_t* ws_bytes);
/* x (N,3); t: one float per row at stride t_stride floats (0 = the same scalar for every row, as the
 * reference's expand() produces at train.py:196; is_blender: the 30 timenet outputs, t_stride 0); outputs d_xyz (N,3), d_rotation (N,4), d_scaling (N,3). */
int trase_mlp_forward(const TraseMlpWeights* w, const float* x, const float* t, int32_t t_stride, int32_t N,
                      float* d_xyz, float* d_rotation, float* d_scaling, void* ws, size_t ws_bytes, int32_t device,
                      trase_stream_t stream);

/* The same inference forward at near-fp32 accuracy ("split bf16"): every matrix operand -- encoding, weights, activations --
 * is carried as hi + lo (two bf16, round-to-nearest-even) and a product is hi.hi + hi.lo + lo.hi on the same MFMA
 * instruction, accumulated in fp32; the weights are re-packed as hi / lo streams on every call.  Forward only; same
 * arguments and the same supported networks as trase_mlp_forward, with a workspace of trase_mlp_split_ws_bytes bytes.
 * Every refusal is TRASE_ERR_INVALID with a message, before the device is touched: null pointers with N > 0, N < 0, a
 * workspace that is too small, D / W / multires values other than the compiled network's, variant != 0.  N == 0 returns 0
 * and launches nothing.  (The size query is not called *_sizes: the recorded table of tests/golden/workspace_sizes.json lists
 * every *_sizes function of this header and is not extended by it.) */
int trase_mlp_split_ws_bytes(size_t* ws_bytes);
int trase_mlp_forward_split(const TraseMlpWeights* w, const float* x, const float* t, int32_t t_stride, int32_t N,
                            float* d_xyz, float* d_rotation, float* d_scaling, void* ws, size_t ws_bytes, int32_t device,
                            trase_stream_t stream);

/* Training pair (train.py:202-204 runs the MLP with gradients in the GAUSSIAN state; loss.backward() at
 * train.py:299 reaches utils/time_utils.py:106-131 through autograd).
 *   trase_mlp_forward_train: the same fused forward; additionally fills the opaque `saved` buffer (bf16
 *     activations and encoding as transposed images, the ReLU gates as bits -- 4.2 KB per Gaussian).
 *   trase_mlp_backward: from the cotangents of the three outputs (any may be NULL = zero) and `saved`, the
 *     gradients of every parameter (fp32, overwritten; NULL entries are skipped).  Fused data chain on the
 *     matrix cores, then one split-N MFMA GEMM per layer input and a partial-sum reduction.  x and t are
 *     detached at the reference's call site, so nothing is propagated into the encoding. */
typedef struct TraseMlpGrads {
  float* weight[8];        /* same shapes as TraseMlpWeights */
  float* bias[8];
  float* w_warp;     float* b_warp;
  float* w_rotation; float* b_rotation;
  float* w_scaling;  float* b_scaling;
} TraseMlpGrads;

int trase_mlp_train_sizes(int32_t N, size_t* fwd_ws_bytes, size_t* saved_bytes, size_t* bwd_ws_bytes);
int trase_mlp_forward_train(const TraseMlpWeights* w, const float* x, const float* t, int32_t t_stride, int32_t N,
                            float* d_xyz, float* d_rotation, float* d_scaling, void* saved, size_t saved_bytes,
                            void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_mlp_backward(const TraseMlpWeights* w, int32_t N, const float* dL_dd_xyz, const float* dL_dd_rotation,
                       const float* dL_dd_scaling, const void* saved, size_t saved_bytes, const TraseMlpGrads* grads,
                       void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
/* The same pair with a ROW ORDER: batch row r evaluates Gaussian row_order[r] (a permutation of 0..N-1, int32, device;
 * NULL = identity = the two entry points above).  Inputs are gathered and outputs / cotangents addressed through it, so the
 * caller sees the reference's row order on both sides; the saved state is in batch order and the same row_order must be
 * handed to the backward.  Why: a Gaussian the view culled (radii == 0, gaussian_renderer/__init__.py:152) sends back an
 * exactly-zero cotangent and contributes nothing to any parameter gradient of utils/time_utils.py:106-131; the backward skips
 * every 32-row tile whose cotangents are all zero (with or without a row order), and culling is spatially coherent, so an
 * order that follows a space-filling curve turns the culled quarter of an orbit view into whole dead tiles. */
int trase_mlp_forward_train_rows(const TraseMlpWeights* w, const float* x, const float* t, int32_t t_stride, int32_t N,
                                 const int32_t* row_order, float* d_xyz, float* d_rotation, float* d_scaling, void* saved,
                                 size_t saved_bytes, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_mlp_backward_rows(const TraseMlpWeights* w, int32_t N, const int32_t* row_order, const float* dL_dd_xyz,
                            const float* dL_dd_rotation, const float* dL_dd_scaling, const void* saved, size_t saved_bytes,
                            const TraseMlpGrads* grads, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
/* Introspection: number of live 32-row tiles the backward that last used `bwd_ws` (N rows) worked on, copied
 * (stream-ordered, device to device) into one int32 of the caller. */
int trase_mlp_live_tiles(const void* bwd_ws, size_t ws_bytes, int32_t N, int32_t* n_live_device, trase_stream_t stream);

/* ---- KNN feature smoothing of the FEATURE state ------------------------------------
 * GaussianModel.get_smoothed_gaussian_features (scene/gaussian_model.py:79-104; gaussian_renderer/__init__.py:118,
 * train.py:274-275):  out[i] = mean_s normalize(features[knn_idx[i][select[s]]]),  F.normalize eps = 1e-12.
 *   features (P,32), knn_idx (P,K) int64 (pytorch3d.ops.knn_points(...).idx), select: S distinct slots of 0..K-1
 *   (the reference's torch.randperm(K)[:int(K*dropout)]), out (P,32).  inv_norm (P floats) is written by the
 *   forward and read by the backward.
 * The backward gathers over the REVERSE adjacency instead of scattering with atomics: rev_src holds the flat
 * positions i*K+k of knn_idx sorted (stably) by the Gaussian they point at, rev_ptr (P+1) the CSR offsets; the host
 * builds both once per KNN map.  select_mask has bit k set for every selected slot. */
int trase_smooth_forward(const float* features, const int64_t* knn_idx, int32_t P, int32_t F, int32_t K,
                         const int32_t* select, int32_t S, float* inv_norm, float* out, int32_t device,
                         trase_stream_t stream);
int trase_smooth_backward(const float* features, const float* inv_norm, int32_t P, int32_t F, int32_t K,
                          uint32_t select_mask, int32_t S, const int32_t* rev_ptr, const int32_t* rev_src,
                          const float* dL_dout, float* dL_dfeatures, int32_t device, trase_stream_t stream);

/* ---- photometric loss heads -----------------------------------------------------------
 * l1_loss (utils/loss_utils.py:30-31) and ssim (utils/loss_utils.py:56-86: 11x11 Gaussian window, sigma 1.5, zero
 * padding, C1 = 0.01^2, C2 = 0.03^2, mean over the map), combined at train.py:235-238.
 *   forward : img, gt (C,H,W) -> out2 = {mean |img - gt|, mean SSIM map} (device floats); keeps the SSIM partial
 *             derivatives in `ws` (trase_loss_sizes bytes; the caller holds it until the backward).
 *   backward: g2 = {dL/dl1, dL/dssim} (device floats, so no host sync) -> dL/dimg (C,H,W), overwritten. */
int trase_loss_sizes(int32_t C, int32_t H, int32_t W, size_t* ws_bytes);
int trase_loss_l1_ssim_forward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, float* out2, void* ws,
                               size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_loss_l1_ssim_backward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, const float* g2,
                                const void* ws, size_t ws_bytes, float* dL_dimg, int32_t device, trase_stream_t stream);
/* The combination train.py:235-238 forms with scalar tensor arithmetic, `(1 - lambda_dssim) * Ll1 + lambda_dssim * (1 - ssim(image,
 * gt))`, inside the same two launches: out3 = {l1, ssim, loss} (device floats); the backward takes ONE cotangent g = dL/dloss (a
 * device float) and scales it by (1 - lambda) and -lambda itself -- the ~10 scalar kernels autograd launches for the composition
 * (and their host time) disappear.  lambda_dssim in [0, 1], a DOUBLE as in the reference's Python: the two weights are (float)(1.0 -
 * lambda) and (float)lambda, what torch's tensor-times-Python-scalar arithmetic multiplies with (1.0f - (float)lambda is one ulp off
 * for lambda = 0.35). */
int trase_loss_photometric_forward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, double lambda_dssim,
                                   float* out3, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_loss_photometric_backward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, double lambda_dssim,
                                    const float* g, const void* ws, size_t ws_bytes, float* dL_dimg, int32_t device,
                                    trase_stream_t stream);

/* ---- contrastive pixel-pair losses (second half) -------------------------------------------
 * positive_pixel_pair_loss / negative_pixel_pair_loss (utils/loss_utils.py:396-406), selected by
 * opt.contrastive_mode (arguments/__init__.py:131; default 'soft') and called at train.py:290-291 on the S x S matrices
 * C (0/1 pixel-mask correspondence), C_F (feature similarity) and weights (may be NULL).
 * kind = TRASE_PAIR_POSITIVE|NEGATIVE + TRASE_PAIR_SOFT|ALL|HARD:
 *   soft: utils/loss_utils.py:304-349   all: :275-302 (threshold unused)   hard: :351-394.
 * out2 = {loss, N} (device floats; N = number of candidate pairs, for 'hard' the selection size); `ws`
 * (trase_contrastive_sizes bytes) keeps the column flags for the backward, which writes the dense dL/dC_F (S x S) for
 * the upstream gradient g (device scalar).  Nothing synchronises (the reference calls torch.nonzero per loss).  An
 * empty candidate set gives loss 0 with a zero gradient (the reference: python 0.0 / tensor(0.) for soft / hard, and
 * 0/0 = nan for 'all'). */
#define TRASE_PAIR_POSITIVE 0
#define TRASE_PAIR_NEGATIVE 1
#define TRASE_PAIR_SOFT 0
#define TRASE_PAIR_ALL 2
#define TRASE_PAIR_HARD 4
int trase_contrastive_sizes(int32_t S, size_t* ws_bytes);
int trase_contrastive_forward(const float* C, const float* C_F, const float* weights, int32_t S, float threshold,
                              int32_t kind, float* out2, void* ws, size_t ws_bytes, int32_t device,
                              trase_stream_t stream);
int trase_contrastive_backward(const float* C, const float* C_F, const float* weights, int32_t S, float threshold,
                               int32_t kind, const float* out2, const float* g, const void* ws, size_t ws_bytes,
                               float* dL_dC_F, int32_t device, trase_stream_t stream);

/* ---- multi-tensor Adam (first half) --------------------------------------------------------
 * One launch steps up to 16 parameter tensors with per-tensor learning rate and step count, in place
 * (param, exp_avg, exp_avg_sq), with torch.optim.Adam's arithmetic (no weight decay, no amsgrad):
 * scene/gaussian_model.py:253-300 builds Adam(l, lr=0.0, eps=1e-15) over per-parameter groups; train.py:376-389
 * steps it.  The tables (pointers to device tensors, sizes, learning rates, steps) are HOST arrays. */
/* ---- nearest-neighbour feature matching style loss (utils/loss_utils.py:223-228; train_style_transfer_nnfm.py:201-203) ----
 * loss = mean_i min_j (1 - cos(feat1[:, i], feats2[:, j])) for feat1 (C, N1), feats2 (C, N2) fp32, C a multiple of 64 up
 * to 512 (VGG conv4_1), N2 <= 2 097 152.  The N1 x N2 cosine matrix is never formed: a bf16 MFMA GEMM with a running
 * two-entry row maximum short-lists two neighbours per row, fp32 cosines of the original data decide between them (ties ->
 * lowest column).  The backward differentiates through the arg-min w.r.t. feat1 only (the style reference carries no
 * graph).  `ws` from the forward is handed back to the backward unchanged. */
int trase_nnfm_sizes(int32_t C, int32_t N1, int32_t N2, size_t* ws_bytes);
int trase_nnfm_forward(const float* feat1, const float* feats2, int32_t C, int32_t N1, int32_t N2, float* loss, void* ws,
                       size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_nnfm_backward(const float* feat1, const float* feats2, int32_t C, int32_t N1, int32_t N2, const float* g_loss,
                        const void* ws, size_t ws_bytes, float* dL_dfeat1, int32_t device, trase_stream_t stream);

int trase_adam_step(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const int64_t* numel, const float* lr, const int64_t* step, double beta1,
                    double beta2, float eps, int32_t device, trase_stream_t stream);
/* The same step behind a DEVICE-side guard: `guard` is the geom workspace of the forward whose gradients the step consumes
 * (its 64-word header holds the overflow flag and the binning guards).  When that forward overflowed its pair buffer the
 * kernel returns without touching parameters or moments -- the reference skips optimizer.step() on a bad iteration
 * (train.py:298-301, :378) after a host-side check; the sync-free policy cannot afford that check, so the decision is
 * taken where the flag lives.  guard == NULL: no guard. */
int trase_adam_step_guarded(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                            float* const* exp_avg_sq, const int64_t* numel, const float* lr, const int64_t* step, double beta1,
                            double beta2, float eps, const void* guard, int32_t device, trase_stream_t stream);

/* Per-kernel timing with HIP events on the caller's stream (used by bench.py's
 * roofline leg).  enable=1 starts recording, the report call synchronises the
 * events and returns averaged milliseconds per kernel name. */
int trase_prof_enable(int enable);
int trase_prof_report(char* buf, size_t buf_bytes); /* JSON object {"kernel": {"ms":..,"n":..}, ...} */

/* On-device self test of the wave64 primitives the kernels rely on
 * (DPP reductions, ballots, MFMA fragment layouts).  Returns 0 when all pass. */
int trase_selftest(int32_t device, trase_stream_t stream, char* msg, size_t msg_bytes);

/* Test entry points of the integer primitives under everything else (binning.hip): the radix sort, the tile ranges and the
 * zero fill, each driven once on the caller's data.  They allocate for themselves and synchronise; not for any hot path.
 *
 * trase_selftest_sort: one radix_sort_pairs call over `cap` items laid out by the library's own sort layout.  keys (cap device
 * words) and vals (cap device words, or NULL for iota values) are copied into ping-pong buffer `start`; the other pair -- and
 * vals[start] under iota -- is filled with `sentinel`; the device-side count is n (may exceed cap: the kernels clamp it).
 * hist_copies 0 = the layout's default rule.  use_flag != 0 passes flag_key and a zeroed flag word.  keys_out / vals_out (cap
 * device words each) receive the WHOLE result buffers; result[0..2] (host) = {index of the result buffers, flag word, 1 when
 * the short sort's fused passes ran}. */
int trase_selftest_sort(const uint32_t* keys, const uint32_t* vals, uint32_t n, uint32_t cap, int32_t bit_lo, int32_t bit_hi,
                        int32_t digit_bits, int32_t hist_copies, int32_t start, uint32_t flag_key, int32_t use_flag,
                        uint32_t sentinel, uint32_t* keys_out, uint32_t* vals_out, uint32_t* result, int32_t device,
                        trase_stream_t stream);
/* trase_selftest_tile_ranges: launch_tile_ranges on the caller's key pointer AS GIVEN (one that is not 16-byte aligned reaches
 * the grid-stride kernel; an aligned one must have cap rounded up to 4 readable words) with the device-side count n.  ranges:
 * T pairs of device words the caller has prefilled (cleared first when clear != 0).  dbg (3 host words) = the out-of-range-key
 * record {seen, index, key}. */
int trase_selftest_tile_ranges(const uint32_t* keys, uint32_t n, uint32_t cap, int32_t T, int32_t clear, uint32_t* ranges,
                               uint32_t* dbg, int32_t device, trase_stream_t stream);
/* trase_selftest_zero_bytes: launch_zero_bytes(p, bytes) on the caller's device pointer, any alignment. */
int trase_selftest_zero_bytes(void* p, size_t bytes, int32_t device, trase_stream_t stream);

/* trase_selftest_compact_live: launch_compact_live over P Gaussians in a geom + pre workspace carved by the library's own layouts
 * and filled with 0xCD.  tiles / keys: P device words each (pairs per Gaussian, depth keys).  keys_out / ids_out / live_ids_out (P
 * device words each) receive the WHOLE arrays: what the kernels did not write still reads 0xCDCDCDCD.  hdr_out (5 host words) =
 * {HDR_R, HDR_OVERFLOW, HDR_R_EFF, HDR_PACK, the length word}. */
int trase_selftest_compact_live(const uint32_t* tiles, const uint32_t* keys, int32_t P, uint32_t* keys_out, uint32_t* ids_out,
                                uint32_t* live_ids_out, uint32_t* hdr_out, int32_t device, trase_stream_t stream);
/* trase_selftest_scan_tiles: launch_scan_tiles in the same poisoned workspace.  tiles, ids (Gaussian ids in depth-rank order, each
 * < P), radii: P device words each; xy: P device float pairs; n_live: the length word (depth ranks that exist); cap, pack_bits, gx,
 * gy (16x16 tiles) as the library passes them; overflow_in: the overflow word before the scan.  offsets_out (P device words) =
 * the block-local inclusive sums, 0xCDCDCDCD behind n_live; block_sums_out (ceil(P / 1024) device words) = every block's
 * exclusive prefix; hdr_out as above. */
int trase_selftest_scan_tiles(const uint32_t* tiles, const uint32_t* ids, const int32_t* radii, const float* xy, int32_t P,
                              uint32_t n_live, uint32_t cap, int32_t pack_bits, int32_t gx, int32_t gy, uint32_t overflow_in,
                              uint32_t* offsets_out, uint32_t* block_sums_out, uint32_t* hdr_out, int32_t device,
                              trase_stream_t stream);

const char* trase_last_error(void);
const char* trase_version(void);

/* ---- densification bookkeeping + densify / prune compaction (second half) -------------------
 * trase_densify_stats: the per-iteration statistics of train.py:362-365 and scene/gaussian_model.py:637-639 in one
 * launch, with visibility_filter = radii > 0 (gaussian_renderer/__init__.py:137):
 *   max_radii2D = max(max_radii2D, radii);  xyz_gradient_accum += |viewspace_grad[:, :2]|;  denom += 1   on visible rows.
 * viewspace_grad is the [P][3] gradient of the screen-space points (means2D.grad).
 *
 * trase_densify_plan + trase_densify_apply replace GaussianModel.densify_and_prune (scene/gaussian_model.py:617-635:
 * densify_and_clone :594-615, densify_and_split :563-592, prune_points :491-509, optimizer surgery :472-489, :511-534).
 * plan: decides clone / split / prune per row from the accumulated statistics and the RAW scaling [P][3] and opacity
 *   [P] parameters, and builds the row map of the final model in `ws` (trase_densify_sizes bytes).
 *   dense_extent = percent_dense * scene_extent; big_extent = 0.1 * scene_extent, applied only when use_screen_size != 0
 *   (the reference's max_screen_size argument; its max_radii2D test is dead code there, see densify.hip).
 *   counts (5 device ints) = {kept originals, kept clones, kept split children per sample, split-selected rows M,
 *   clone-selected rows}; the new row count is counts[0] + counts[1] + 2 * counts[2].  The caller reads them (the one
 *   synchronisation: it has to allocate the new tensors), draws 2M x 3 standard normals and calls
 * apply: gathers `count` (<= 32 per call) row-major tensors of 4-byte elements through the map, dst[r] = src[map[r]],
 *   writing zeros into rows that are not kept originals where zero_new[i] != 0 (the Adam moments), then -- when
 *   normal_samples != NULL -- rewrites the children rows of new_xyz / new_scaling:
 *   xyz' = R(rotation) (z * exp(scaling)) + xyz,  scaling' = log(exp(scaling) / 1.6).  With more than 32 tensors pass
 *   normal_samples on the last call only (after xyz and scaling were gathered); it may be NULL only when M == 0. */
int trase_densify_stats(const float* viewspace_grad, const int32_t* radii, float* xyz_gradient_accum, float* denom,
                        float* max_radii2D, int32_t P, int32_t device, trase_stream_t stream);
/* guard: as for trase_adam_step_guarded -- the statistics of an overflowed view are not taken */
int trase_densify_stats_guarded(const float* viewspace_grad, const int32_t* radii, float* xyz_gradient_accum, float* denom,
                                float* max_radii2D, int32_t P, const void* guard, int32_t device, trase_stream_t stream);
int trase_densify_sizes(int32_t P, size_t* ws_bytes);
int trase_densify_plan(const float* xyz_gradient_accum, const float* denom, const float* scaling, const float* opacity,
                       int32_t P, float grad_threshold, float dense_extent, float min_opacity, int32_t use_screen_size,
                       float big_extent, int32_t* counts, void* ws, size_t ws_bytes, int32_t device,
                       trase_stream_t stream);
int trase_densify_apply(int32_t count, const void* const* src, void* const* dst, const int32_t* row_elems,
                        const int32_t* zero_new, int32_t P, int32_t new_P, const float* xyz, const float* scaling,
                        const float* rotation, const float* normal_samples, float* new_xyz, float* new_scaling,
                        const void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);

/* ---- FEATURE-state loss head without S x S matrices (train.py:251-296) ------------------------
 * trase_mask_stats: one pass over the N bool masks [N][HW] (1 byte each): cover_count[p] = number of masks covering pixel
 *   p (the sampler's non_mask_region is cover_count == 0, utils/feature_utils.py:23) and mask_size[n] = sam_masks[n].sum()
 *   (utils/feature_utils.py:30).
 * trase_pairhead_forward: for the S sampled pixels pix[] (flat indices into HW, ascending = boolean-index order) evaluates
 *   what train.py:272-296 computes through get_pixel_mask_correspondence_matrix (utils/feature_utils.py:40-49),
 *   get_features_correspondence_matrix (:51-57), get_pixel_weights (:28-38), positive_/negative_pixel_pair_loss[mode]
 *   (utils/loss_utils.py:275-406; mode 0 soft, 1 all, 2 hard) and the two mean similarities (train.py:295-296), from
 *   per-pixel factors only: feats is the [F = 32][HW] feature image at mask resolution, sampled_mask the N 0/1 bytes of the
 *   sampled masks (n_sampled_masks = an upper bound of their number, at most 256).
 *   out8 = {loss_pos, N_pos, loss_neg, N_neg, pos_similarity, neg_similarity, S, sampled masks} (device floats).
 *   use_weights = 0 evaluates the losses with weights = None.
 * trase_pairhead_backward: dL/dfeats [F][HW] (zero-filled here, then the S sampled columns) for the upstream gradients
 *   g2 = {dL/dloss_pos, dL/dloss_neg} (device floats), from the forward's workspace.  accumulate != 0 adds the S columns
 *   into an image that already holds a gradient (the regulariser's, trase_featnorm_backward) instead of zero-filling.
 * trase_featnorm_*: the regulariser (1 - mean_p |feats[:, p]|_2)^2 of train.py:281-282; out2 = {value, mean norm}. */
int trase_mask_stats(const uint8_t* sam_masks, int32_t N, int64_t HW, int32_t* cover_count, uint32_t* mask_size, int32_t device,
                     trase_stream_t stream);
int trase_pairhead_sizes(int32_t S, size_t* ws_bytes);
int trase_pairhead_forward(const float* feats, int32_t F, int64_t HW, const uint8_t* sam_masks, int32_t N,
                           const uint8_t* sampled_mask, int32_t n_sampled_masks, const uint32_t* mask_size, const int32_t* pix,
                           int32_t S, int32_t mode, float positive_th, float negative_th, int32_t use_weights, float* out8,
                           void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_pairhead_backward(int32_t F, int64_t HW, const int32_t* pix, int32_t S, int32_t mode, float positive_th,
                            float negative_th, int32_t use_weights, const float* out8, const float* g2, const void* ws,
                            size_t ws_bytes, int32_t accumulate, float* dL_dfeats, int32_t device, trase_stream_t stream);
/* The same head WITHOUT the host knowing the number of sampled pixels (round 5: the reference synchronises at every boolean index of
 * train.py:262-296; the round-4 head still did once, for S).  trase_compact_pixels turns the (H W) byte mask `sampled_pixel` into the
 * ascending pixel indices `pix[0 .. count[0])` -- the order of a boolean index -- entirely on the device: count[0] = min(number of set
 * bytes, cap), count[1] = the number itself (ws: trase_compact_pixels_sizes(HW) bytes).  The _n entry points take S = the CAPACITY the
 * workspace and the launch grids are sized for and S_dev = &count[0] (NULL: S is the count, as in the entry points above); rows at or
 * behind the device count do not exist for any kernel; S_dev == 0 gives zero losses, NaN similarities and a zero gradient. */
int trase_compact_pixels_sizes(int64_t HW, size_t* ws_bytes);
int trase_compact_pixels(const uint8_t* flags, int64_t HW, int32_t* pix, int32_t cap, int32_t* count2, void* ws, size_t ws_bytes,
                         int32_t device, trase_stream_t stream);
int trase_pairhead_forward_n(const float* feats, int32_t F, int64_t HW, const uint8_t* sam_masks, int32_t N,
                             const uint8_t* sampled_mask, int32_t n_sampled_masks, const uint32_t* mask_size, const int32_t* pix,
                             int32_t S, const int32_t* S_dev, int32_t mode, float positive_th, float negative_th, int32_t use_weights,
                             float* out8, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_pairhead_backward_n(int32_t F, int64_t HW, const int32_t* pix, int32_t S, const int32_t* S_dev, int32_t mode, float positive_th,
                              float negative_th, int32_t use_weights, const float* out8, const float* g2, const void* ws,
                              size_t ws_bytes, int32_t accumulate, float* dL_dfeats, int32_t device, trase_stream_t stream);
/* The same head for a feature image of ANOTHER size than the masks: feats is [F = 32][Hr][Wr], the masks, pix, S and S_dev stay at
 * the masks' resolution h x w (pix ascending).  The column of a sampled pixel is the bilinear blend of its four taps in feats --
 * torch's upsample_bilinear2d with align_corners = False (train.py:283-284's `interpolate`), source index fma(in / out, dst + 0.5,
 * -0.5) clamped at 0 -- and the resized map is never formed.  Needs Hr * Wr < 2^31 and h * w < 2^31.
 * trase_pairhead_sizes_resized: bytes of the workspace the two calls below share (the forward's, kept for the backward).
 * trase_pairhead_forward_resized: out8 as trase_pairhead_forward_n.
 * trase_pairhead_backward_resized: writes EVERY element of dL_dfeats [F][Hr][Wr] exactly once (no zero fill, no atomics: a pixel
 *   gathers the sampled mask pixels it is a tap of, in a fixed order).  feats, out2 (of trase_featnorm_forward on the same image) and
 *   g_reg (device float, dL/d regulariser) are all null, or all given: then the regulariser's gradient is added in the same pass.
 * trase_pairhead_columns_resized: columns [S][F] = the un-normalised resized columns of the S pixels pix[] alone. */
int trase_pairhead_sizes_resized(int32_t S, int32_t Hr, int32_t Wr, int32_t h, int32_t w, size_t* ws_bytes);
int trase_pairhead_forward_resized(const float* feats, int32_t F, int32_t Hr, int32_t Wr, int32_t h, int32_t w,
                                   const uint8_t* sam_masks, int32_t N, const uint8_t* sampled_mask, int32_t n_sampled_masks,
                                   const uint32_t* mask_size, const int32_t* pix, int32_t S, const int32_t* S_dev, int32_t mode,
                                   float positive_th, float negative_th, int32_t use_weights, float* out8, void* ws, size_t ws_bytes,
                                   int32_t device, trase_stream_t stream);
int trase_pairhead_backward_resized(int32_t F, int32_t Hr, int32_t Wr, int32_t h, int32_t w, const int32_t* pix, int32_t S,
                                    const int32_t* S_dev, int32_t mode, float positive_th, float negative_th, int32_t use_weights,
                                    const float* out8, const float* g2, const void* ws, size_t ws_bytes, const float* feats,
                                    const float* out2, const float* g_reg, float* dL_dfeats, int32_t device, trase_stream_t stream);
int trase_pairhead_columns_resized(const float* feats, int32_t F, int32_t Hr, int32_t Wr, int32_t h, int32_t w, const int32_t* pix,
                                   int32_t S, float* columns, int32_t device, trase_stream_t stream);
int trase_featnorm_sizes(int64_t HW, size_t* ws_bytes);
int trase_featnorm_forward(const float* feats, int32_t F, int64_t HW, float* out2, void* ws, size_t ws_bytes, int32_t device,
                           trase_stream_t stream);
int trase_featnorm_backward(const float* feats, int32_t F, int64_t HW, const float* out2, const float* g, float* dL_dfeats,
                            int32_t device, trase_stream_t stream);
/* The same head on the masks AS THE REFERENCE STORES THEM (extract_masks.py:91-99): one flat stream of N * HW bits,
 * numpy.packbits(masks.reshape(-1)) = bitarray(...).tobytes() in bitarray's default big-endian bit order.  Stream bit i is bit
 * 7 - (i & 7) of byte i >> 3; mask n starts at stream bit n * HW (in the middle of a byte wherever HW is no multiple of 8); no
 * row or mask is padded, only the last byte.  An eighth of the bool bytes, never expanded (train.py:245-249 does, on the host).
 * Buffer contract of every entry point below: `bits` is 16-byte aligned; bits_bytes is a multiple of 16 and at least
 * ceil(N * HW / 8); no byte at or past bits_bytes is read; bits at or past N * HW are ignored whatever they hold;
 * 1 <= N <= 8192, 1 <= HW < 2^31.  Anything else returns TRASE_ERR_INVALID before a device is touched.
 * trase_mask_stats_bits: cover_count [HW] and mask_size [N] exactly as trase_mask_stats writes them, in one pass over the stream
 *   (integers, no float atomics: bitwise reproducible).
 * trase_pairhead_forward_bits, trase_pairhead_forward_bits_resized: trase_pairhead_forward_n / _forward_resized with
 *   (bits, bits_bytes) in place of sam_masks; workspace of trase_pairhead_sizes / trase_pairhead_sizes_resized, the backward is
 *   trase_pairhead_backward_n / _backward_resized (it never reads the masks).  Same memberships, same arithmetic: the results
 *   are bitwise those of the bool entry points.
 * trase_pack_masks: the N * HW bool bytes (any non-zero byte is set) -> the stream; writes all bits_bytes, padding as zero.
 * trase_unpack_masks: the stream -> N * HW bytes of exactly 0 / 1. */
int trase_mask_stats_bits(const uint8_t* bits, size_t bits_bytes, int32_t N, int64_t HW, int32_t* cover_count, uint32_t* mask_size,
                          int32_t device, trase_stream_t stream);
int trase_pairhead_forward_bits(const float* feats, int32_t F, int64_t HW, const uint8_t* bits, size_t bits_bytes, int32_t N,
                                const uint8_t* sampled_mask, int32_t n_sampled_masks, const uint32_t* mask_size, const int32_t* pix,
                                int32_t S, const int32_t* S_dev, int32_t mode, float positive_th, float negative_th, int32_t use_weights,
                                float* out8, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_pairhead_forward_bits_resized(const float* feats, int32_t F, int32_t Hr, int32_t Wr, int32_t h, int32_t w, const uint8_t* bits,
                                        size_t bits_bytes, int32_t N, const uint8_t* sampled_mask, int32_t n_sampled_masks,
                                        const uint32_t* mask_size, const int32_t* pix, int32_t S, const int32_t* S_dev, int32_t mode,
                                        float positive_th, float negative_th, int32_t use_weights, float* out8, void* ws, size_t ws_bytes,
                                        int32_t device, trase_stream_t stream);
int trase_pack_masks(const uint8_t* sam_masks, int32_t N, int64_t HW, uint8_t* bits, size_t bits_bytes, int32_t device,
                     trase_stream_t stream);
int trase_unpack_masks(const uint8_t* bits, size_t bits_bytes, int32_t N, int64_t HW, uint8_t* sam_masks, int32_t device,
                       trase_stream_t stream);

/* ---- ground truth as bytes: the planar 8-bit frame and the photometric heads that read it --------------------------------------
 * A ground-truth frame of the reference is always the image of a byte array (PILtoTorch, utils/general_utils.py:22-28: every
 * pixel is float32(b) / float32(255)).  The frame: `planes`, 16-byte aligned, 3 planes (r, g, b) of H rows, `pitch` bytes from
 * row to row, pitch = the smallest multiple of 16 >= W; 3 * H * pitch bytes.  No consumer reads a byte of the row padding or
 * anything at or past 3 * H * pitch.  Every refusal is TRASE_ERR_INVALID (a workspace that is too small:
 * TRASE_ERR_WORKSPACE) with a message, before a device is touched: null pointers, H or W < 1, channels other than 3 or 4, a
 * background with 3 channels, a pitch that is no multiple of 16 or below W, planes that are not 16-byte aligned.
 * trase_frame_pack: hwc = (H, W, channels) bytes on the device, what np.array(pil_image) is -> the planes, padding written as 0;
 *   a fourth channel is dropped (utils/camera_utils.py:51).  background (three HOST floats, or null): with 4 channels the
 *   composite of train.py:221-228 per channel, byte = trunc(((v / 255.0) * (a / 255.0) + bg * (1 - a / 255.0)) * 255.0) in float64,
 *   every operation rounded on its own, the fp32 background promoted to double, the result taken modulo 256 as numpy's
 *   conversion to np.byte does.
 * trase_frame_unpack: the planes -> (3, H, W) fp32, each value the true fp32 quotient b / 255: bit for bit the reference's
 *   original_image.
 * trase_frame_black_mask: mask (h, w) bytes of 0 / 1.  h == H and w == W: 1 where r | g | b == 0 (train.py:232).  Otherwise
 *   train.py:267-268: 1 where the frame resized to (h, w) (bilinear, align_corners = False) sums to 0 over the channels, i.e.
 *   where every tap of non-zero weight is 0 in all three planes (all terms are non-negative); integer logic only.
 * trase_loss_*_u8: the four loss entry points above with the planes in place of gt (C = 3; same workspace, same kernels' bodies,
 *   same reduction: the outputs are bitwise those of the float entry points on trase_frame_unpack's tensor).  flags:
 *   TRASE_FRAME_MASK_BLACK fuses train.py:231-234 -- where the frame's pixel is black the rendered value counts as 0 (also in
 *   the window's halo) and receives gradient 0; a non-finite rendered value there is ignored (the reference's image * 0 is NaN). */
#define TRASE_FRAME_MASK_BLACK 1u
int trase_frame_pack(const uint8_t* hwc, int32_t H, int32_t W, int32_t channels, const float* background, uint8_t* planes, int32_t pitch,
                     int32_t device, trase_stream_t stream);
int trase_frame_unpack(const uint8_t* planes, int32_t H, int32_t W, int32_t pitch, float* chw, int32_t device, trase_stream_t stream);
int trase_frame_black_mask(const uint8_t* planes, int32_t H, int32_t W, int32_t pitch, int32_t h, int32_t w, uint8_t* mask, int32_t device,
                           trase_stream_t stream);
/* trase_frame_resize: the frame at another size, bit for bit what PILtoTorch's pil_image.resize(resolution) gives on the RGB bytes
 *   (Pillow, mode "RGB", the default filter BICUBIC, no box, no reducing_gap): per axis ImagingResample's coefficient rows -- double
 *   arithmetic in Pillow's order, normalised by the sum taken in tap order, rounded to 22 fractional bits -- then the horizontal
 *   pass into bytes and the vertical pass on those, each clamp(((1 << 21) + sum coeff * byte) >> 22, 0, 255); an axis whose size
 *   does not change is skipped.  One launch, no workspace.  src (device): src_layout 3 = (src_H, src_W, 3) bytes; 4 =
 *   (src_H, src_W, 4), the alpha dropped or, with a background (three HOST floats), composited first as trase_frame_pack does,
 *   then resized as RGB; TRASE_FRAME_PLANAR = the planes of a frame, rows src_pitch >= src_W bytes apart (src_pitch is ignored
 *   otherwise).  No byte at or past the end of the source is read.  planes, H, W, pitch: the destination frame, padding written as
 *   0.  Refusals: trase_frame_pack's, a layout other than these, and an axis that shrinks by more than 16 (src > 16 * dst).
 *   Equal sizes: layouts 3 and 4 give the bits of trase_frame_pack, a planar source is copied.
 * trase_selftest_resize_tables: the coefficient rows the kernel computes, by the same __device__ function: coeffs (out, ksize)
 *   int32, zero beyond n, ksize = (int)ceil(2 * max(in / out, 1)) * 2 + 1; bounds (out, 2) int32 = (xmin, n).  in <= 16 * out. */
#define TRASE_FRAME_PLANAR 1
int trase_frame_resize(const uint8_t* src, int32_t src_H, int32_t src_W, int32_t src_layout, int32_t src_pitch, const float* background,
                       uint8_t* planes, int32_t H, int32_t W, int32_t pitch, int32_t device, trase_stream_t stream);
int trase_selftest_resize_tables(int32_t in, int32_t out, int32_t* coeffs, int32_t* bounds, int32_t device, trase_stream_t stream);
int trase_loss_l1_ssim_forward_u8(const float* img, const uint8_t* planes, int32_t H, int32_t W, int32_t pitch, uint32_t flags, float* out2,
                                  void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_loss_l1_ssim_backward_u8(const float* img, const uint8_t* planes, int32_t H, int32_t W, int32_t pitch, uint32_t flags,
                                   const float* g2, const void* ws, size_t ws_bytes, float* dL_dimg, int32_t device, trase_stream_t stream);
int trase_loss_photometric_forward_u8(const float* img, const uint8_t* planes, int32_t H, int32_t W, int32_t pitch, uint32_t flags,
                                      double lambda_dssim, float* out3, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_loss_photometric_backward_u8(const float* img, const uint8_t* planes, int32_t H, int32_t W, int32_t pitch, uint32_t flags,
                                       double lambda_dssim, const float* g, const void* ws, size_t ws_bytes, float* dL_dimg, int32_t device,
                                       trase_stream_t stream);

/* ---- segmentation after training: K-means and query masks (gui.py:248-270, render.py:97-105 + :334-345) ------------------
 * trase_kmeans_steps: n_steps Lloyd steps of kmeans_pytorch.kmeans(X, K, distance='euclidean') (gui.py:248-270,
 *   gui_standalone.py:685-707; 0.3's loop, see trase_amd/segment.py), entirely on the device.  X (N,D) fp32, centres_inout
 *   (K,D) fp32 (the start centres in, the step's new centres out), ids_out (N) int32 = the assignment made against the centres
 *   the step started from (argmin of the squared distance, ties to the lowest index).  An empty cluster k in iteration i
 *   (counted from 0) takes row splitmix64(reseed_key ^ (i << 32 | k)) mod N.  state (int32[4], device, zeroed by the caller
 *   before the first step) = {iterations, done, center_shift of the last step as float bits, 0}; a step sets done when
 *   center_shift^2 < tol or iter_limit != 0 and iterations >= iter_limit, and every step of a state with done set does
 *   nothing, so the host may enqueue steps in batches and read the state once per batch.  Per-cluster sums are reduced in a
 *   fixed order without atomics: bitwise reproducible.  Limits: 1 <= K <= 128, 1 <= D <= 64, N >= K.
 *   Workspace: trase_kmeans_sizes(N, D, K).
 * trase_segment_mask: render.py:97-105 postprocessing OR-ed over the selected ids as the loop at render.py:334-345 does, for
 *   fp32 features X (N,D) and int32 cluster ids (N): a point whose id is sel[s] (S <= 128 ids) is scored against
 *   q = normalize(mean of the rows with id sel[s]) as fp16(fp16(x / |x|) . fp16(q)) with fp32 sums; mask_out (N bytes) = score
 *   >= fp16(threshold).  Points with no selected id, negative ids, zero rows and empty clusters give 0.  S = 0: all 0.
 *   Workspace: trase_segment_mask_sizes(N, D, S). */
int trase_kmeans_sizes(int32_t N, int32_t D, int32_t K, size_t* ws_bytes);
int trase_kmeans_steps(const float* X, int32_t N, int32_t D, int32_t K, float* centres_inout, int32_t* ids_out,
                       uint64_t reseed_key, float tol, int32_t iter_limit, int32_t n_steps, int32_t* state, void* ws,
                       size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_segment_mask_sizes(int32_t N, int32_t D, int32_t S, size_t* ws_bytes);
int trase_segment_mask(const float* X, int32_t N, int32_t D, const int32_t* ids, const int32_t* sel, int32_t S, float threshold,
                       uint8_t* mask_out, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);

/* ---- prompt lift: a 2D prompt to cluster votes (render.py:208-229, gui.py:1039-1064; a clicked pixel: gui.py:786-800) -----
 * For every prompted pixel (row r, column c, depth d = depth[r * W + c]; depth is the (H, W) fp32 map the rasterizer wrote):
 *     z = zfar / (zfar - znear) * d - zfar * znear / (zfar - znear)
 *     p = ([((c - 0.5) / W * 2 - 1) * d, ((r - 0.5) / H * 2 - 1) * d, z, d] @ inv_proj)[:3]     (no homogeneous division)
 *   inv_proj is a HOST pointer to the 16 doubles (row-major, row-vector convention) of inverse(full_proj_transform), inverted
 *   in float64 by the caller.  z is folded into rows 2 and 3 of it in float64 before the kernel's coefficients are rounded to
 *   fp32 (the two rows cancel by a factor of about d / znear), and the kernel evaluates p in float64 and rounds it.  The nearest of the N `points` (fp32
 *   (N, 3), exact, ties to the lowest index) gives j; votes_out[cluster_ids[j]] += 1 for 0 <= cluster_ids[j] < bins (int32
 *   ids; a negative id casts no vote).  A pixel of depth 0 still votes; a pixel whose point is not finite finds nothing.
 *   Prompt, one of: prompt_mask (H * W bytes, non-zero = prompted; pixels must be NULL), or pixels (M (col, row) int32 pairs;
 *   prompt_mask NULL; a pair outside the image finds nothing).
 *   Outputs: votes_out (bins int32, zeroed here; integer atomics, so bitwise reproducible); optional index_out (int32, H * W
 *   for a mask -- -1 where not prompted -- or M for a pixel list) and points_out (fp32, 3 per entry of index_out, 0 where
 *   not prompted).  bins = 0 with cluster_ids = votes_out = NULL only looks the indices up.  N = 0: no hash is built, every
 *   index is -1 and no vote is cast; M = 0: nothing is launched but the zeroing of votes_out.
 *   Limits: 0 <= bins <= 4096 (the per-block LDS histogram), W * H < 2^31.  Workspace: trase_lift_sizes(N, bins). */
int trase_lift_sizes(int32_t N, int32_t bins, size_t* ws_bytes);
int trase_lift_votes(const float* depth, int32_t W, int32_t H, const double* inv_proj, double znear, double zfar,
                     const uint8_t* prompt_mask, const int32_t* pixels, int32_t M, const float* points, int32_t N,
                     const int32_t* cluster_ids, int32_t bins, int32_t* votes_out, int32_t* index_out, float* points_out,
                     void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);

/* ---- nearest cluster centre by cosine (gui.py:276 + :288-290, gui_standalone.py:721-727) -----------------------------------
 * trase_assign_clusters: ids_out[n] (int64) = argmax_k <x_n / |x_n|, c_k> for fp32 features X (N,D) and centres (K,D), both on
 *   the device, the centres used as given.  Ties go to the lowest k.  The raw dot products are compared (the division by |x_n|
 *   is common to every k); optional scores_out[n] (fp32) = the winning dot product / max(|x_n|, 1e-12), so a zero row gets
 *   id 0 and score 0.  Fixed-order fmaf chains: bitwise reproducible.  Limits: 1 <= K <= 4096 (the bin limit of
 *   trase_lift_votes), 1 <= D <= 64.  Workspace: trase_assign_clusters_sizes(N, D, K) (which validates the limits; 0 bytes
 *   today, ws may then be NULL). */
int trase_assign_clusters_sizes(int32_t N, int32_t D, int32_t K, size_t* ws_bytes);
int trase_assign_clusters(const float* X, int32_t N, int32_t D, const float* centres, int32_t K, int64_t* ids_out,
                          float* scores_out, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);

/* ---- display stage: point splats and PCA colours (render.py:247-294, :52-59; gui.py:984-1030, :55-62) ----------------------
 * trase_splat_points: every point i of `points` (fp32 (N,3), the deformed positions) with mask == NULL or mask[i] != 0 is
 *   projected in float64, p = [x, y, z, 1] @ full_proj (a HOST pointer to the 16 doubles of full_proj_transform, row-major,
 *   row-vector convention), px = (p.x / p.w + 1) / 2 * W, py = (p.y / p.w + 1) / 2 * H, and lands at column trunc(px), row
 *   trunc(py) if 0 < px < W and 0 < py < H (no near-plane or w > 0 test; a non-finite coordinate lands nowhere).  The winner
 *   of a pixel is the HIGHEST index landing there (integer atomicMax: bitwise reproducible).  For each of the L <= 4 layers
 *   images_out[l] ((3,H,W) fp32, planar) = colors[l][winner] at hit pixels (colors[l] fp32 (N,3); NULL = the dot colour: 1,
 *   or 0 with white_background) and the background (0, or 1 with white_background) elsewhere.  `colors` and `images_out` are
 *   HOST arrays of L device pointers.  Optional index_out (H * W int64): the winner, -1 where no point landed.
 *   Limits: W * H < 2^31.  Workspace: trase_splat_sizes(N, W, H) (the int32 winner map).
 * trase_feature_gram: gram_mean_out (device, D * D + D fp32) = the centred Gram matrix Xc^T Xc of X (N,D) fp32, Xc = X - mean,
 *   then the D column means.  fp32 products and sums within a block, block slabs summed in block order in float64: no float
 *   atomics, bitwise reproducible.  Limits: N >= 2, 1 <= D <= 64.  Workspace: trase_feature_gram_sizes(N, D).
 * trase_feature_project: colors_out (N,3) fp32 = ((X - mean) @ axes^T - min) / (max - min), axes (3,D) and mean (D) fp32 on
 *   the device, min and max taken over all 3 N projections (integer atomics on the ordered-int image of the floats);
 *   max == min gives 0 / 0 = NaN as render.py:58 does.  minmax: 2 int32 words of device scratch. */
int trase_splat_sizes(int32_t N, int32_t W, int32_t H, size_t* ws_bytes);
int trase_splat_points(const float* points, int32_t N, const uint8_t* mask, const double* full_proj, int32_t W, int32_t H,
                       const float* const* colors, int32_t L, int32_t white_background, float* const* images_out,
                       int64_t* index_out, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_feature_gram_sizes(int32_t N, int32_t D, size_t* ws_bytes);
int trase_feature_gram(const float* X, int32_t N, int32_t D, float* gram_mean_out, void* ws, size_t ws_bytes, int32_t device,
                       trase_stream_t stream);
int trase_feature_project(const float* X, int32_t N, int32_t D, const float* axes, const float* mean, float* colors_out,
                          int32_t* minmax, int32_t device, trase_stream_t stream);

/* ---- HDBSCAN over sampled features: the viewer's default clustering mode (gui.py:271-301, gui_standalone.py:721-727) -------
 * The two dense all-pairs passes of HDBSCAN for fp32 rows X (n,D) on the device; the hierarchy over the n - 1 tree edges is the
 * caller's (trase_amd/segment.py).  A squared distance is the fmaf chain over (a_d - b_d)^2 in dimension order, symmetric bit
 * for bit; no n x n buffer is held.  Limits: 2 <= n <= 65536 (16 + 16 index bits in an edge key), 1 <= D <= 64, 1 <= k <= 64,
 * k < n.  Workspace of both: trase_hdbscan_sizes(n, D, k).
 * trase_hdbscan_core: core2_out[i] (fp32) = the SQUARED distance from row i to its k-th nearest OTHER row (the hdbscan
 *   package's min_samples = k; scikit-learn counts the row itself, so its min_samples is k + 1).
 * trase_hdbscan_mst: the minimum spanning tree of w(i,j) = max(core2[i], core2[j], |x_i - x_j|^2) by Boruvka rounds with
 *   64-bit integer atomics on the keys (float bits of w) << 32 | min(i,j) << 16 | max(i,j), a total order on the edges (among
 *   equal weights the lower index pair wins).  edge_keys_out (n uint64): the n - 1 keys of the tree in slots that depend on
 *   the data only, and one ~0; sorted ascending they are the edge list in canonical order.  counts_out (18 int32): the
 *   component count after every round, counts_out[0] = n, the last non-zero entry 1.  Nothing is read by the host; bitwise
 *   reproducible.
 * trase_label_centres: centres_out (C,D) fp32, row c = normalize(mean of the rows of X (N,D) with labels[n] == c), the norm
 *   clamped at 1e-12; labels int32, a label outside [0, C) (noise: -1) belongs nowhere; a label without rows gives NaN.  The
 *   sums are those of K-means and of the query mask (fixed order, no float atomics).  Limits: 1 <= C <= 4096, 1 <= D <= 64.
 *   Workspace: trase_label_centres_sizes(N, D, C). */
int trase_hdbscan_sizes(int32_t n, int32_t D, int32_t k, size_t* ws_bytes);
int trase_hdbscan_core(const float* X, int32_t n, int32_t D, int32_t k, float* core2_out, void* ws, size_t ws_bytes,
                       int32_t device, trase_stream_t stream);
int trase_hdbscan_mst(const float* X, int32_t n, int32_t D, const float* core2, uint64_t* edge_keys_out, int32_t* counts_out,
                      void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_label_centres_sizes(int32_t N, int32_t D, int32_t C, size_t* ws_bytes);
int trase_label_centres(const float* X, int32_t N, int32_t D, const int32_t* labels, int32_t C, float* centres_out, void* ws,
                        size_t ws_bytes, int32_t device, trase_stream_t stream);

/* ---- composited scenes: render_composite and its rigid edits (gaussian_renderer/__init__.py:158-331) ----------------------
 * One part of a composited scene: a model's RAW parameters (n rows), optionally gathered through `rows`, deformed, and moved
 * by a rigid edit.  Per output row i, with r = rows ? rows[i] : i, in fp32 and in the reference's statement order:
 *   means = xyz[r] + d_xyz[r]; scales = exp(scaling[r]) + d_scaling[r]; rot = normalize(rotation[r]) + d_rotation[r];
 *   opacity = sigmoid(opacity[r]); shs = cat(features_dc[r], features_rest[r]); sh_objs = gaussian_features[r] (as stored);
 *   edit_mode >= 1: means *= scale_factor, scales *= scale_factor;
 *   edit_mode == 2: means = R means, rot = normalize(q_edit (x) rot)   (Hamilton product, components (r,x,y,z));
 *   edit_mode >= 1: means += offset.
 * edit_mode 1 is the reference's early return for angles that are all exactly zero: rot stays the un-renormalised sum.
 * Rescale and rotation are about the world origin; SH coefficients are not rotated.  A rows[] entry outside [0, n) is never
 * dereferenced: its output row is all zeros.  exp is the library expf (<= 1 ulp). */
typedef struct TraseComposePart {
  int32_t n;                        /* rows of the model */
  int32_t m;                        /* output rows: entries of `rows`, or n when rows is NULL */
  int32_t F;                        /* feature channels, 0 <= F <= 64 */
  int32_t edit_mode;                /* 0 none, 1 rescale + translate, 2 rescale + rotate + translate */
  const float* xyz;                 /* (n,3)    */
  const float* scaling;             /* (n,3)    */
  const float* rotation;            /* (n,4), 16-byte aligned */
  const float* opacity;             /* (n,1)    */
  const float* features_dc;         /* (n,1,3)  */
  const float* features_rest;       /* (n,15,3) */
  const float* gaussian_features;   /* (n,1,F), 16-byte aligned; NULL when F == 0 */
  const int64_t* rows;              /* (m) device, ascending by convention, or NULL: all rows */
  const float* d_xyz;               /* (n,3) or NULL: indexed by SOURCE row (the reference adds first, masks afterwards) */
  const float* d_rotation;          /* (n,4) or NULL, 16-byte aligned */
  const float* d_scaling;           /* (n,3) or NULL */
  float scale_factor;
  float R[9];                       /* row-major */
  float q_edit[4];                  /* (r,x,y,z), r >= 0 */
  float offset[3];
} TraseComposePart;

/* trase_compose_sizes: validates the part count (1..8), the row counts and F; offsets_out (HOST, n_parts + 1 int64) = the
 *   first output row of every part and the total P (< 2^25).  No workspace is needed.
 * trase_compose_part: one launch; writes rows [row_offset, row_offset + m) of means3D (P,3), scales (P,3), rotations (P,4),
 *   opacities (P,1), shs (P,16,3), sh_objs (P,1,F) -- fp32, contiguous, 16-byte aligned.  Bitwise reproducible; the inputs
 *   are read only. */
int trase_compose_sizes(const int32_t* counts, int32_t n_parts, int32_t F, int64_t* offsets_out);
int trase_compose_part(const TraseComposePart* part, int64_t row_offset, int64_t P_total, float* means3D, float* scales,
                       float* rotations, float* opacities, float* shs, float* sh_objs, int32_t device, trase_stream_t stream);

/* ---- segment output and scoring (render.py:344-366, :380-395; metrics_segmentation.py:33-48, :118-150) ---------------------
 * trase_evaluate_frame: ONE launch over a W x H frame; a thread owns 4 consecutive pixels of a row (16-byte accesses where
 * the planes allow it, scalar ones for row tails and unaligned rows).  Per pixel p:
 *   inside = 1 - T(p) >= threshold   with T = final_T, or the final_T of `ws` (the img workspace of a forward that ran WITHOUT
 *                                    TRASE_VARIANT_FORWARD_ONLY; ws, final_T and pred_in exclude each other); a NaN is outside;
 *          = pred_in[p] != 0         with a given mask; = 1 with neither;
 *   alpha = 1 - T;  pred_mask = inside (bytes 0 / 1);  pred_mask_u8 = 255 * inside in all three channels;
 *   object[c] = inside ? image[c] : outside;  object_u8 = to8b(object) = trunc(255 * clip(x, 0, 1)) in fp32, a NaN gives 0.
 *   image, object, pair_*: (3,H,W) fp32 planes; alpha (H,W) fp32; pred_in, pred_mask, gt_mask (H,W) bytes; *_u8 (H,W,3) bytes.
 *   Every output may be NULL.  image == NULL: only the mask part runs.
 * Scores, added to record[0 .. TRASE_EVAL_RECORD_WORDS) (device, int64, zeroed by the caller before the frame's first call):
 *   gt_mask (non-zero = object): [0] += |inside & gt|, [1] += |inside | gt|, [2] += |inside == gt|, [3] += W * H;
 *   gt_object (kind TRASE_EVAL_GT_*; fp32 values in [0,1]): [5] += 3 * W * H and, with quantize, [4] += sum (q(object) - q(gt))^2
 *     over the 3 W H values, q(x) = trunc(clamp(x * 255 + 0.5, 0, 255)) in fp32 (torchvision's save_image; a NaN gives 0; 8-bit
 *     inputs are used as stored) -- an exact integer.  Without quantize, partials[b] (device, float64,
 *     TRASE_EVAL_MAX_BLOCKS slots, zeroed by the caller) = workgroup b's sum of (object - gt)^2 in float64, gt bytes read as
 *     g / 255; the squared error is the sum of the slots in index order.
 *   Words [6] and [7] are the caller's.  pair_object / pair_gt: the compared pair as fp32 planes (quantised: q / 255).
 *   Counts are reduced per wave and per workgroup and added with one 64-bit integer atomic instruction per workgroup; there
 *   are no float atomics: bitwise reproducible.  The inputs are read only.  Limits: W * H < 2^31. */
#define TRASE_EVAL_RECORD_WORDS 8
#define TRASE_EVAL_MAX_BLOCKS 2048
enum { TRASE_EVAL_GT_NONE = 0, TRASE_EVAL_GT_F32_CHW = 1, TRASE_EVAL_GT_U8_CHW = 2, TRASE_EVAL_GT_U8_HWC = 3 };
typedef struct TraseEvalFrame {
  int32_t W;
  int32_t H;
  float threshold;
  float outside;                    /* the value outside the mask: 0, or 1 with a white background */
  int32_t gt_object_kind;           /* TRASE_EVAL_GT_* */
  int32_t quantize;
  const float* image;
  const float* final_T;
  const uint8_t* pred_in;
  float* object;
  float* alpha;
  uint8_t* pred_mask;
  uint8_t* object_u8;
  uint8_t* pred_mask_u8;
  const uint8_t* gt_mask;
  const void* gt_object;
  float* pair_object;
  float* pair_gt;
  int64_t* record;
  double* partials;
} TraseEvalFrame;
int trase_evaluate_frame(const TraseEvalFrame* f, const TraseRastWorkspace* ws, int32_t device, trase_stream_t stream);

/* ---- colour layers: the view and up to ten per-Gaussian colour tables from one pass (render.py:197, :240, :296) -------------
 * A per-Gaussian colour placed in feature channels 3l .. 3l+2 of an F = 32 forward is composited by exactly the arithmetic
 * of the colour channels; what the feature channels lack is the background term of the colour epilogue.
 * trase_layers_pack: ONE launch; out (P,32) fp32, 16-byte aligned: row i = [tables[0][i].rgb, tables[1][i].rgb, ..., 0 ... 0].
 *   tables: HOST array of L device pointers to (P,3) fp32 tables, contiguous, each only 4-byte aligned.  Columns 3L .. 31
 *   are +0.0f; nothing at or past row P is read or written.  P == 0 launches nothing.
 * trase_layers_finish: ONE launch over a W x H frame, a thread owns 4 consecutive pixels of a row (16-byte accesses where the
 *   planes allow it, scalar ones for row tails and W % 4 != 0).  planes: (32,H,W) fp32, the feature output of that forward.
 *   For l < L, c < 3:  planes[3l + c] = fmaf(T, bg[c], planes[3l + c]) in place, with T the final_T of `ws` -- the img
 *   workspace of a forward that ran WITHOUT TRASE_VARIANT_FORWARD_ONLY (it begins with the W * H fp32 values of final_T) --
 *   and bg 3 fp32 on the device.  Planes 3L .. 31 are not touched.  image_u8 ((H,W,3) bytes, needs image (3,H,W) fp32) and
 *   layers_u8 ((L,H,W,3) bytes), each optional: to8b = trunc(255 * clip(x, 0, 1)) in fp32, a NaN gives 0, of the image and
 *   of the finished layers -- trase_evaluate_frame's quantiser.  ws == NULL: the planes are final already, only the 8-bit
 *   frames are written (bg may be NULL then).  No atomics: bitwise reproducible.  W == 0 or H == 0 launches nothing.
 * Both return TRASE_ERR_INVALID before a device is touched for a NULL pointer, L outside 1 .. TRASE_LAYERS_MAX, a negative
 * size (finish: W * H >= 2^31), an `out` off a 16-byte boundary, tables, planes or image off a 4-byte boundary, an image_u8
 * without an image, or (finish) nothing to do; finish returns TRASE_ERR_WORKSPACE for an img workspace that is too small. */
#define TRASE_LAYERS_MAX 10
int trase_layers_pack(const float* const* tables, int32_t L, int32_t P, float* out, int32_t device, trase_stream_t stream);
int trase_layers_finish(float* planes, const TraseRastWorkspace* ws, const float* bg, int32_t L, int32_t W, int32_t H,
                        const float* image, uint8_t* image_u8, uint8_t* layers_u8, int32_t device, trase_stream_t stream);

/* ---- trajectory view and frame finish (utils/time_utils.py:375-396; gui.py:1154-1191, :1080-1122) ---------------------------
 * Scratch of these entry points is passed as explicit buffers whose sizes are the constants below.
 * trase_fps_sample: farthest-point sampling of the rows of `points` (fp32 (N,3)) with mask == NULL or mask[i] != 0, the
 *   reference's loop at B = 1: out[0] = the start row (start_dev, a DEVICE pointer to one int64 row, if non-NULL, else `start`);
 *   the running minimum distance of every candidate starts at 1e10 and is lowered on strict < to
 *   d = (dx*dx + dy*dy) + dz*dz, every product and sum rounded to fp32 (no fused multiply-add: what numpy float32 gives bit
 *   for bit); out[i + 1] = the arg-max, the LOWEST row among equal distances (once every distance is 0 the lowest candidate
 *   row repeats).  out: npoint int64 rows of `points`.  npoint ordinary launches on the stream (npoint - 1 of up to
 *   TRASE_FPS_MAX_BLOCKS workgroups and a last one of one workgroup), no cooperative launch, no host read.  The start row must
 *   be a candidate (the caller's check).  Scratch: dist, N fp32; partial, 2 * TRASE_FPS_MAX_BLOCKS uint64.  Bitwise
 *   reproducible.  Limits: 1 <= N < 2^31, 1 <= npoint <= TRASE_FPS_MAX_SAMPLES.
 * trase_trajectory_append: slot_out (G,3) fp32 = points[rows[g]] (rows int64 on the device; a row outside [0, N) gives NaN).
 * trase_trajectory_draw: the polylines of G trajectories over S samples, oldest first: sample s is row (first + s) % cap of
 *   coords ((cap,G,3) fp32 world positions; a plain (S,G,3) array has first = 0, cap = S).  Three launches: winner (H * W int32
 *   scratch, left holding the result) = -1; one wave per segment (g; s, s + 1) -- with S == 1 the single sample -- projects both
 *   ends in float64, p = [x, y, z, 1] @ full_proj (HOST pointer, 16 doubles, row-major, row-vector convention), px = (p.x / p.w
 *   + 1) / 2 * W, py likewise with H, no w > 0 test, truncated toward zero to integers, and draws
 *     dx = |bx - ax| >= dy = |by - ay|: for every integer x from ax to bx, y = ay + sign(by - ay) * floor((2 |x - ax| dy + dx) / (2 dx))
 *     (otherwise with the roles of x and y swapped; a == b is one pixel), in 64-bit integers, over the in-image part of the
 *   major axis only, pixels outside the image dropped, with atomicMax(winner, g): the HIGHEST trajectory index wins a pixel.
 *   A sample with a non-finite coordinate or one of magnitude >= 2^20 breaks its polyline: no segment it ends is drawn.
 *   overlay_out (optional, (H,W,4) fp32) = (colors[winner], 1) where a line passes, zeros elsewhere; colors (G,3) fp32.
 *   Limits: S <= cap <= TRASE_TRAJ_MAX_SAMPLES, G <= TRASE_TRAJ_MAX_TRACKS, W * H < 2^31.  Bitwise reproducible.
 * trase_present_frame: out (H,W,3) fp32 = the frame as the viewer shows it, one launch.  image: (3,h,w) fp32 planes, or with
 *   `depth` one (h,w) plane whose values v become (v - min) / (max - min + 1e-20) in all three channels, min and max over the
 *   plane by two launches in front (integer atomics on the ordered-int image of the floats; a NaN takes no part; minmax: 2
 *   int32 words of scratch).  Bilinear resize to (H,W) with ATen's fp32 arithmetic for align_corners = False: scale =
 *   float(in) / out, src = max(fma(scale, dst + 0.5f, -0.5f), 0) (the product fused into the subtraction, as ATen's kernel is
 *   compiled), i0 = int(src), i1 = min(i0 + 1, in - 1), l1 = src - i0,
 *   l0 = 1 - l1, value = h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d); equal sizes copy.  Then clamp to [0,1] (a NaN stays),
 *   control_overlay ((H,W,3) or NULL): b * (sum of its channels == 0) + it; overlay ((H,W,4) or NULL): b * (1 - a) + rgb * a;
 *   tint ((H,W,3) or NULL): b + tint_weight * tint, not clamped.  Every blend product and sum is rounded to fp32 on its own.
 *   The inputs are read only.  Limits: h * w < 2^31, H * W < 2^31. */
#define TRASE_FPS_MAX_BLOCKS 256
#define TRASE_FPS_MAX_SAMPLES 65536
#define TRASE_TRAJ_MAX_TRACKS 65536
#define TRASE_TRAJ_MAX_SAMPLES 1024
int trase_fps_sample(const float* points, int32_t N, const uint8_t* mask, int32_t start, const int64_t* start_dev, int32_t npoint,
                     int64_t* out, float* dist, uint64_t* partial, int32_t device, trase_stream_t stream);
int trase_trajectory_append(const float* points, int32_t N, const int64_t* rows, int32_t G, float* slot_out, int32_t device,
                            trase_stream_t stream);
int trase_trajectory_draw(const float* coords, int32_t S, int32_t G, int32_t first, int32_t cap, const double* full_proj, int32_t W,
                          int32_t H, const float* colors, float* overlay_out, int32_t* winner, int32_t device, trase_stream_t stream);
int trase_present_frame(const float* image, int32_t h, int32_t w, int32_t depth, int32_t H, int32_t W, const float* control_overlay,
                        const float* overlay, const float* tint, float tint_weight, float* out, int32_t* minmax, int32_t device,
                        trase_stream_t stream);

/* ---- VGG16 feature extractor of the style-transfer loop (style_transfer/fx.py; train_style_transfer_nnfm.py:141-215) ----
 * The 3x3 convolutions conv1_1 conv1_2 | conv2_1 conv2_2 | conv3_1 conv3_2 conv3_3 | conv4_1 (| = MaxPool2d(2, 2)), batch 1.
 * `layers` = k in 1..8 cuts the network behind its k-th convolution and returns that convolution's output BEFORE its ReLU:
 * out (C, h * w) fp32 planar, C = 64 64 128 128 256 256 256 512, h = H >> p, w = W >> p behind p pools.  H, W >= 2^p,
 * H * W < 2^25.  image: (3, H, W) fp32 planes, never modified; mean / inv_std: HOST arrays of 3 floats (both NULL: no
 * normalisation): conv1_1 reads (x - mean) * inv_std, the backward multiplies the image gradient by inv_std.
 * Arithmetic: conv1_1 and its gradient in fp32; every other product as bf16x3 (operands split into hi + lo bf16, hi.hi +
 * hi.lo + lo.hi on the matrix cores into an fp32 accumulator that starts at the bias).  No atomics: bitwise reproducible, and a
 * cut at k gives the bits of layers 1..k of a deeper cut.
 * trase_vgg_ws_bytes: the bytes of the pack, of the forward's and the backward's workspace and of the saved decisions, and the
 *   output shape, each from the one walk that also carves the buffer.
 * trase_vgg_pack: weights[l] (Cout, Cin, 3, 3) and biases[l] (Cout) fp32 device tensors of layer l = 0 .. layers - 1 (HOST
 *   arrays of pointers) -> `pack`; once per weight set.  A pack of more layers serves every shorter cut.
 * trase_vgg_forward: `saved` (optional) receives the decisions the backward needs: 1 bit per convolution output (z > 0), 4 bits
 *   per pooled unit where a pool follows (window position in ATen's scan order -- rows, then columns, update on strict > -- and
 *   whether the maximum was positive).  With saved == NULL nothing is kept.  ws: ws_forward_bytes.
 * trase_vgg_backward: d_out (C, h * w) -> d_image (3, H, W), the weights being constants.  ws: ws_backward_bytes.
 * Refusals: TRASE_ERR_INVALID (layers, sizes, null pointers, pack / saved / ws not 16-byte aligned) and TRASE_ERR_WORKSPACE
 * (pack, saved or ws too small), with a message, before a device is touched. */
int trase_vgg_ws_bytes(int32_t layers, int32_t H, int32_t W, size_t* pack_bytes, size_t* ws_forward_bytes, size_t* ws_backward_bytes,
                    size_t* saved_bytes, int32_t* C, int32_t* h, int32_t* w);
int trase_vgg_pack(int32_t layers, const float* const* weights, const float* const* biases, void* pack, size_t pack_bytes,
                   int32_t device, trase_stream_t stream);
int trase_vgg_forward(int32_t layers, const void* pack, size_t pack_bytes, const float* image, int32_t H, int32_t W,
                      const float* mean, const float* inv_std, float* out, void* saved, size_t saved_bytes, void* ws,
                      size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_vgg_backward(int32_t layers, const void* pack, size_t pack_bytes, const float* d_out, int32_t H, int32_t W,
                       const float* inv_std, const void* saved, size_t saved_bytes, float* d_image, void* ws, size_t ws_bytes,
                       int32_t device, trase_stream_t stream);

/* ---- LPIPS with the VGG16 backbone (lpipsPyTorch, net_type='vgg', version 0.1; metrics_segmentation.py:118-165), forward only ----
 * Thirteen 3x3 convolutions conv1_1 conv1_2 | conv2_1 conv2_2 | conv3_1 conv3_2 conv3_3 | conv4_1 conv4_2 conv4_3 | conv5_1
 * conv5_2 conv5_3 (| = MaxPool2d(2, 2)) on two images x, y (3, H, W) fp32, batch 1, with the kernels and the arithmetic of the
 * extractor above.  The taps are the post-ReLU activations relu1_2 relu2_2 relu3_3 relu4_3 relu5_3 BEFORE the pool that follows:
 * C_l = 64 128 256 512 512 channels of h_l x w_l = (H >> l) x (W >> l) pixels, l = 0 .. 4; a tap's value is hi + lo of its
 * split planes.  Per tap and pixel, in float64 and rounded to fp32 once,
 *   d = sum_c lin_c (a_c / (sqrt(sum_c a_c^2) + 1e-10) - b_c / (sqrt(sum_c b_c^2) + 1e-10))^2,
 * norms first, then differences; a pixel whose channels are all 0 gives 0.  A layer's value is the float64 mean of its map, summed
 * in a fixed order (256 chunks, then their partial sums).  No atomics: two calls give the same bits, (x, y) and (y, x) give the same bits, (x, x) gives exactly 0.
 * trase_lpips_ws_bytes: H, W >= 16 (relu5_3 has a pixel), H * W < 2^25.  map_floats = sum_l h_l w_l.  ws_bytes: THREE buffers of
 *   H * W * 64 split values (hi and lo bf16 planes: 256 H W bytes each; every activation behind the first pool is at most half
 *   a buffer, so x's conv1_1 buffer is reused), the five maps and 5 x 256 float64 partial sums of their means.
 * trase_lpips_pack: weights[l] (Cout, Cin, 3, 3), biases[l] (Cout), l = 0 .. 12, and lin[t] (C_t), t = 0 .. 4: fp32 device
 *   tensors (HOST arrays of pointers) -> `pack`: conv1_1 and the lin vectors as fp32, layers 2 .. 13 as forward weight streams.
 * trase_lpips_forward: mean / inv_std as in trase_vgg_forward.  out_layers: 5 float64 on the device, the layers' values; LPIPS is
 *   their sum.  maps (optional): map_floats fp32, the five per-pixel maps one after the other.  taps_x / taps_y (optional,
 *   together): sum_l C_l h_l w_l fp32 each, the five taps as planar (C_l, h_l w_l), one after the other.  All launches go to
 *   `stream`; nothing is allocated or synchronised.
 * trase_lpips_head: the head alone on two fp32 planar (C, hw) activations a, b and lin (C) (device): they are split as the
 *   cotangent of trase_vgg_backward is and go through the same head kernel.  C in {64, 128, 256, 512}, hw >= 1, C * hw < 2^31.
 *   out_layer: 1 float64 (device); map (optional): hw fp32.  ws: 4 r(2 C hw) + r(4 hw) + 2048 bytes, r = rounded up to 256.
 * Refusals: TRASE_ERR_INVALID (sizes, null pointers, pack / ws not 16-byte aligned, out_layers not 8-byte aligned) and
 * TRASE_ERR_WORKSPACE (pack or ws too small), with a message, before a device is touched. */
int trase_lpips_ws_bytes(int32_t H, int32_t W, size_t* pack_bytes, size_t* ws_bytes, size_t* map_floats);
int trase_lpips_pack(const float* const* weights, const float* const* biases, const float* const* lin, void* pack, size_t pack_bytes,
                     int32_t device, trase_stream_t stream);
int trase_lpips_forward(const void* pack, size_t pack_bytes, const float* x, const float* y, int32_t H, int32_t W, const float* mean,
                        const float* inv_std, double* out_layers, float* maps, float* taps_x, float* taps_y, void* ws, size_t ws_bytes,
                        int32_t device, trase_stream_t stream);
int trase_lpips_head(const float* a, const float* b, const float* lin, int32_t C, int32_t hw, double* out_layer, float* map, void* ws,
                     size_t ws_bytes, int32_t device, trase_stream_t stream);

/* ---- the rest of utils/loss_utils.py (style.hip): image-space losses and the style statistics ----------------------------------
 * No float atomics: two calls give the same bits.  Inputs are never modified; nothing is allocated or synchronised.  Every
 * refusal is TRASE_ERR_INVALID (a workspace that is too small: TRASE_ERR_WORKSPACE) with a message, before a device is touched.
 * trase_pixel_loss_*: x (C,H,W) fp32; gt the same (gt_pitch == 0) or the planes of a byte frame (gt_pitch > 0: C = 3, read as
 *   float32(b) / float32(255)); C * H * W < 2^31.  kind / aux:
 *     TRASE_PIXEL_MASKED_L1    sum(|x - gt| * m) / (C * sum(m)), m (H,W) bytes (AUX_U8, the value of the byte) or fp32 (AUX_F32);
 *                              an all-zero mask gives 0 and a zero gradient
 *     TRASE_PIXEL_WEIGHTED_L1  mean(|x - gt| * w), w (H,W) fp32 (AUX_F32) or (C,H,W) fp32 (AUX_F32_FULL)
 *     TRASE_PIXEL_L2           mean((x - gt)^2), no aux
 *   Terms are formed in fp32, each operation rounded on its own, and summed in float64; out: 1 float.  The forward leaves the
 *   denominator in ws; the backward reads it: d_x = sign(x - gt) * (m * s) resp. (2 s) * (x - gt), s = g[0] * float(1 / denominator).
 * trase_style_ws_bytes: the one workspace of the four calls below for (C, n) features, 1 <= C <= 512, 1 <= n < 2^31.
 * trase_gram_matrix: G (C,C) = x x^T on the fp32 MFMA: fp32 chains of 1024 columns, chain results added in float64 in order and
 *   rounded once; G[i][j] and G[j][i] are the same bits.
 * trase_mean_std: per channel the mean and the unbiased standard deviation + eps (added in fp32), two passes in float64; n >= 2.
 * trase_style_node_forward: out4 = {total, gram, adain, content}, each term weighted, formed in float64:
 *     gram    = gram_weight * mean((G - style_gram)^2) / (C * n)
 *     adain   = adain_weight * (mean((mean - style_mean)^2) + mean((std - style_std)^2)), eps = 1e-8      (n >= 2)
 *     content = content_weight * mean((x - content)^2)                                                     (C * n < 2^31)
 *   A term whose weight is 0 is not computed and its targets may be NULL.  saved: C * C + 2 * C floats = D | a | b for
 *   trase_style_grad_gemm, with c = float(2 * content_weight / (C * n)).
 * trase_style_grad_gemm: dx[i][k] = g * (2 * sum_j D[i][j] x[j][k] + a[i] + b[i] * x[i][k] + c * (x[i][k] - y[i][k])), one launch.
 *   D NULL: no product; a, b NULL (together): no AdaIN part; y NULL: no content part; g NULL: 1. */
#define TRASE_PIXEL_MASKED_L1 0
#define TRASE_PIXEL_WEIGHTED_L1 1
#define TRASE_PIXEL_L2 2
#define TRASE_PIXEL_AUX_NONE 0
#define TRASE_PIXEL_AUX_U8 1
#define TRASE_PIXEL_AUX_F32 2
#define TRASE_PIXEL_AUX_F32_FULL 3
int trase_pixel_loss_ws_bytes(size_t* ws_bytes);
int trase_pixel_loss_forward(const float* x, const void* gt, int32_t gt_pitch, int32_t C, int32_t H, int32_t W, int32_t kind,
                             const void* aux, int32_t aux_kind, float* out, void* ws, size_t ws_bytes, int32_t device,
                             trase_stream_t stream);
int trase_pixel_loss_backward(const float* x, const void* gt, int32_t gt_pitch, int32_t C, int32_t H, int32_t W, int32_t kind,
                              const void* aux, int32_t aux_kind, const float* g, const void* ws, size_t ws_bytes, float* d_x,
                              int32_t device, trase_stream_t stream);
int trase_style_ws_bytes(int32_t C, int64_t n, size_t* ws_bytes);
int trase_gram_matrix(const float* x, int32_t C, int64_t n, float* G, void* ws, size_t ws_bytes, int32_t device, trase_stream_t stream);
int trase_mean_std(const float* x, int32_t C, int64_t n, float eps, float* mean, float* std_, void* ws, size_t ws_bytes, int32_t device,
                   trase_stream_t stream);
int trase_style_node_forward(const float* x, int32_t C, int64_t n, const float* style_gram, const float* style_mean,
                             const float* style_std, const float* content, double gram_weight, double adain_weight,
                             double content_weight, float* out4, float* saved, void* ws, size_t ws_bytes, int32_t device,
                             trase_stream_t stream);
int trase_style_grad_gemm(const float* D, const float* a, const float* b, float c, const float* x, const float* y, int32_t C, int64_t n,
                          const float* g, float* dx, int32_t device, trase_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TRASE_RAST_H */
