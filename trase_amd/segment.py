"""Segmentation after training as HIP kernels (trase_amd/csrc/segment.hip): K-means over the per-Gaussian features and the
query masks built from the clusters.

``kmeans(X, K)`` is ``kmeans_pytorch.kmeans(X, K, distance='euclidean')`` as gui.py:248-270 and gui_standalone.py:685-707
call it (kmeans_pytorch 0.3): numpy draws the K distinct start rows on the host exactly as the library does (so the global
numpy RNG advances the same way), then every Lloyd step runs on the device -- assignment, per-cluster means reduced in a
fixed order, center_shift, the stopping test -- and the host reads the device state word once per ``_BATCH`` steps.
Deliberate deviation: an empty cluster k of iteration i (from 0) is re-seeded with row
``splitmix64(key ^ (i << 32 | k)) mod N`` instead of the library's ``X[torch.randint(N, (1,))]``; ``key`` is ``seed`` when
given, else one draw from torch's default CPU generator (so ``torch.manual_seed`` makes runs repeat).

``segment_mask(features, cluster_ids, segment_ids, score_threshold)`` is render.py:97-105 ``postprocessing`` OR-ed over the
ids as the loop at render.py:334-345 does (also :370-380, gui.py:457-464, :598-607).  It is functional: the reference
normalises the features IN PLACE (``get_gaussian_features`` returns the parameter itself), so its first id of its first
frame takes the query mean from raw features and every later call from normalised ones; callers reproduce that by passing
``F.normalize(features)`` after the first call.

``lift_votes`` / ``prompt_clusters`` / ``pick`` lift a 2D prompt (a mask, or clicked pixels) to the clusters it lands on:
render.py:208-229, gui.py:1039-1064 and gui.py:786-800 as one pass on the device (the lift kernels of
trase_amd/csrc/knn.hip, on top of its spatial hash).  Deliberate deviations: the projection is inverted on the host in
float64 and the un-projection evaluated in float64 (the reference's fp32 ``torch.inverse`` of a znear = 0.01 projection moves
points by up to 4e-4 and with them the nearest index of a fraction of a percent of the pixels), and a negative cluster id
casts no vote where ``torch.bincount`` would raise.

``assign_clusters(features, centres)`` gives every Gaussian the id of its nearest cluster centre by cosine, gui.py:276 +
:288-290 (gui_standalone.py:721-727, the viewer's DBSCAN mode, where the reference copies all features to the host and runs
an N x K x D einsum on the CPU), for clusters that are not K-means ones.

Only CUDA tensors are accepted: there is no CPU path."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .rasterizer import _stream

_BATCH = 8          # Lloyd steps enqueued per read of the device state word (results do not depend on it)
_MASK64 = (1 << 64) - 1


def _device_index(dev: torch.device) -> int:
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _kmeans_sizes(N: int, D: int, K: int) -> int:
    sz = C.c_size_t()
    _lib.check(_lib.load().trase_kmeans_sizes(N, D, K, C.byref(sz)), "kmeans")
    return sz.value


def _kmeans_steps(X: torch.Tensor, centres: torch.Tensor, ids: torch.Tensor, key: int, tol: float, iter_limit: int,
                  n_steps: int, state: torch.Tensor, ws: torch.Tensor | None = None) -> None:
    """Enqueue ``n_steps`` Lloyd steps on the current stream: ``centres`` (K,D fp32) are updated in place, ``ids`` (N int32)
    receive the assignment of the last step that ran, ``state`` (int32[4]) = {iterations, done, center_shift bits, 0}."""
    N, D = X.shape
    K = centres.shape[0]
    if ws is None:
        ws = torch.empty(_kmeans_sizes(N, D, K), dtype=torch.uint8, device=X.device)
    _lib.check(_lib.load().trase_kmeans_steps(_lib.ptr(X), N, D, K, _lib.ptr(centres), _lib.ptr(ids), int(key) & _MASK64,
                                              float(tol), int(iter_limit), int(n_steps), _lib.ptr(state), _lib.ptr(ws),
                                              ws.numel(), _device_index(X.device), _stream(X.device)), "kmeans")


def kmeans(X: torch.Tensor, num_clusters: int, *, tol: float = 1e-4, iter_limit: int = 0, seed: int | None = None):
    """-> (ids int64 (N,), centres float32 (K, D), iterations), all on X's device."""
    if not torch.is_tensor(X) or X.device.type != "cuda":
        raise RuntimeError("kmeans runs on the GPU only (there is no CPU path)")
    if X.dim() != 2:
        raise ValueError(f"kmeans: X must be (N, D), got {tuple(X.shape)}")
    X = X.detach().float().contiguous()
    N, D = X.shape
    K = int(num_clusters)
    ws = torch.empty(_kmeans_sizes(N, D, K), dtype=torch.uint8, device=X.device)   # validates K, D, N first
    if seed is None:
        indices = np.random.choice(N, K, replace=False)
        key = int(torch.randint(0, 2 ** 62, (1,)).item())
    else:
        np.random.seed(seed)
        indices = np.random.choice(N, K, replace=False)
        key = int(seed)
    centres = X[torch.from_numpy(np.asarray(indices, dtype=np.int64)).to(X.device)].contiguous()
    ids = torch.zeros(N, dtype=torch.int32, device=X.device)
    state = torch.zeros(4, dtype=torch.int32, device=X.device)
    host = torch.empty(4, dtype=torch.int32, pin_memory=True)
    ev = torch.cuda.Event()
    while True:
        _kmeans_steps(X, centres, ids, key, tol, iter_limit, _BATCH, state, ws)
        host.copy_(state, non_blocking=True)
        ev.record(torch.cuda.current_stream(X.device))
        ev.synchronize()
        if int(host[1]):
            break
    return ids.to(torch.int64), centres, int(host[0])


ASSIGN_MAX_CENTRES = 4096      # == LIFT_MAX_BINS: the ids go to lift_votes unchanged


def assign_clusters(features: torch.Tensor, centres: torch.Tensor, *, return_scores: bool = False):
    """-> int64 (N,) ``argmax_k <f_n / |f_n|, c_k>`` on the features' device: gui.py:276 + :288-290.  ``features`` is (N, D) or
    (N, 1, D) fp32, ``centres`` (K, D) on the device or the host, 1 <= K <= 4096, 1 <= D <= 64; the centres are used as given
    (the viewer normalises them at gui.py:286).  Ties go to the lowest k.  A zero feature row gets id 0 (and score 0, its
    norm clamped at 1e-12 as ``F.normalize`` does).  With ``return_scores`` also the winning score, fp32 (N,).  The ids can
    be passed unchanged to ``lift_votes``, ``segment_mask`` and ``display.splat_points``.  Inputs are read, never modified."""
    if not torch.is_tensor(features) or features.device.type != "cuda":
        raise RuntimeError("assign_clusters runs on the GPU only (there is no CPU path)")
    dev = features.device
    if features.dim() == 3 and features.shape[1] == 1:
        features = features.squeeze(1)
    if features.dim() != 2:
        raise ValueError(f"assign_clusters: features must be (N, D) or (N, 1, D), got {tuple(features.shape)}")
    X = features.detach().float().contiguous()
    N, D = X.shape
    centres = torch.as_tensor(centres)
    if centres.dim() != 2 or centres.shape[1] != D:
        raise ValueError(f"assign_clusters: centres must be (K, {D}), got {tuple(centres.shape)}")
    Cn = centres.detach().to(device=dev, dtype=torch.float32).contiguous()
    K = Cn.shape[0]
    lib = _lib.load()
    sz = C.c_size_t()
    _lib.check(lib.trase_assign_clusters_sizes(N, D, K, C.byref(sz)), "assign_clusters")      # validates K, D first
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    ids = torch.empty(N, dtype=torch.int64, device=dev)
    scores = torch.empty(N, dtype=torch.float32, device=dev) if return_scores else None
    _lib.check(lib.trase_assign_clusters(_lib.ptr(X), N, D, _lib.ptr(Cn), K, _lib.ptr(ids), _lib.ptr(scores),
                                         _lib.ptr(ws) if sz.value else None, ws.numel(), _device_index(dev), _stream(dev)),
               "assign_clusters")
    return (ids, scores) if return_scores else ids


def segment_mask(features: torch.Tensor, cluster_ids: torch.Tensor, segment_ids, score_threshold: float = 0.8) -> torch.Tensor:
    """Boolean (N,) mask of the Gaussians whose cluster is one of ``segment_ids`` and whose fp16 cosine score against that
    cluster's normalised mean feature is >= fp16(score_threshold).  Reads its inputs only."""
    if not torch.is_tensor(features) or features.device.type != "cuda":
        raise RuntimeError("segment_mask runs on the GPU only (there is no CPU path)")
    dev = features.device
    N = features.shape[0]
    X = features.detach().reshape(N, -1).float().contiguous()
    D = X.shape[1]
    ids = cluster_ids.detach().reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    if ids.numel() != N:
        raise ValueError(f"segment_mask: {ids.numel()} cluster ids for {N} features")
    if torch.is_tensor(segment_ids):
        sel = segment_ids.detach().reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    else:
        if isinstance(segment_ids, (int, np.integer)):
            segment_ids = [segment_ids]
        sel = torch.tensor([int(s) for s in segment_ids], dtype=torch.int32)
        if sel.numel():
            sel = sel.pin_memory().to(dev, non_blocking=True)
        else:
            sel = sel.to(dev)
    S = int(sel.numel())
    lib = _lib.load()
    sz = C.c_size_t()
    _lib.check(lib.trase_segment_mask_sizes(N, D, S, C.byref(sz)), "segment_mask")
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    mask = torch.empty(N, dtype=torch.uint8, device=dev)
    thr = float(np.float16(score_threshold))      # as torch rounds a Python float that meets a half tensor
    _lib.check(lib.trase_segment_mask(_lib.ptr(X), N, D, _lib.ptr(ids), _lib.ptr(sel), S, thr, _lib.ptr(mask), _lib.ptr(ws),
                                      ws.numel(), _device_index(dev), _stream(dev)), "segment_mask")
    return mask.view(torch.bool)


# ---- prompt lift: a 2D prompt to cluster votes (render.py:208-229, gui.py:1039-1064; clicked pixels: gui.py:786-800) ---------

LIFT_MAX_BINS = 4096      # the lift kernel's per-block LDS histogram (trase_amd/csrc/knn.hip)


def _lift_call(what, depth, viewpoint_camera, points, *, mask=None, pixels=None, ids=None, bins=0, want_index=False,
               want_points=False):
    """One ``trase_lift_votes`` call -> (votes int32 (bins,) | None, index int32 | None, points fp32 | None)."""
    if not torch.is_tensor(depth) or depth.device.type != "cuda" or not torch.is_tensor(points) or points.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the GPU only (there is no CPU path)")
    dev = depth.device
    W, H = int(viewpoint_camera.image_width), int(viewpoint_camera.image_height)
    if depth.numel() != H * W or depth.dim() not in (2, 3) or tuple(depth.shape[-2:]) != (H, W):
        raise ValueError(f"{what}: depth must be ({H}, {W}) or (1, {H}, {W}), got {tuple(depth.shape)}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what}: points must be (N, 3), got {tuple(points.shape)}")
    depth = depth.detach().float().contiguous()
    pts = points.detach().to(dev).float().contiguous()
    N = pts.shape[0]
    # the inverse in float64 of the matrix as stored (one small device-to-host copy unless the camera keeps it on the CPU)
    full = viewpoint_camera.full_proj_transform.detach().to("cpu", torch.float64).numpy()
    if full.shape != (4, 4):
        raise ValueError(f"{what}: full_proj_transform must be (4, 4), got {full.shape}")
    inv = (C.c_double * 16)(*np.linalg.inv(full).reshape(-1).tolist())
    lib = _lib.load()
    sz = C.c_size_t()
    _lib.check(lib.trase_lift_sizes(N, int(bins), C.byref(sz)), what)        # validates bins first
    M = 0
    if mask is not None:
        if not torch.is_tensor(mask) or mask.device.type != "cuda":
            raise RuntimeError(f"{what} runs on the GPU only (there is no CPU path)")
        if mask.numel() != H * W or tuple(mask.shape[-2:]) != (H, W):
            raise ValueError(f"{what}: prompt_mask must be ({H}, {W}), got {tuple(mask.shape)}")
        mask = mask.detach().to(dev)
        mask = (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous().view(torch.uint8)
        n_out = H * W
    else:
        M = n_out = int(pixels.shape[0])
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    votes = torch.empty(int(bins), dtype=torch.int32, device=dev) if bins else None
    index = torch.empty(n_out, dtype=torch.int32, device=dev) if want_index else None
    out_pts = torch.empty(n_out, 3, dtype=torch.float32, device=dev) if want_points else None
    _lib.check(lib.trase_lift_votes(_lib.ptr(depth), W, H, C.byref(inv), float(viewpoint_camera.znear),
                                    float(viewpoint_camera.zfar), _lib.ptr(mask), _lib.ptr(pixels) if M else None, M,
                                    _lib.ptr(pts) if N else None, N, _lib.ptr(ids) if bins and N else None, int(bins),
                                    _lib.ptr(votes), _lib.ptr(index), _lib.ptr(out_pts), _lib.ptr(ws), ws.numel(),
                                    _device_index(dev), _stream(dev)), what)
    return votes, index, out_pts


def _lift_ids(what, cluster_ids, points, num_clusters):
    ids = cluster_ids.detach().reshape(-1).to(device=points.device, dtype=torch.int32).contiguous()
    if ids.numel() != points.shape[0]:
        raise ValueError(f"{what}: {ids.numel()} cluster ids for {points.shape[0]} points")
    if num_clusters is None:        # as torch.bincount sizes its result: one read-back of the largest id
        bins = max(int(ids.max()) + 1, 1) if ids.numel() else 1
    else:
        bins = int(num_clusters)
    return ids, bins


def lift_votes(depth: torch.Tensor, prompt_mask: torch.Tensor, viewpoint_camera, points: torch.Tensor, cluster_ids: torch.Tensor,
               *, num_clusters: int | None = None, return_index: bool = False, return_points: bool = False):
    """Votes per cluster of a 2D prompt (render.py:208-229, gui.py:1039-1064) in one pass on the device: every pixel of the
    bool / uint8 ``prompt_mask`` (H, W) is un-projected through ``depth`` ((1, H, W) or (H, W), the ``depth`` of ``render()``)
    with the inverse of ``viewpoint_camera.full_proj_transform`` (anything with that, ``image_width``, ``image_height``,
    ``znear``, ``zfar``), its nearest row of ``points`` (N, 3) -- the deformed positions -- is found exactly, and that
    point's cluster id receives one vote.

    -> ``votes`` int64 (bins,), bins = ``num_clusters`` or, when None, the largest id + 1 (one read-back); with
    ``return_index`` also the (H, W) int64 map of nearest indices (-1 where not prompted), with ``return_points`` also the
    (H, W, 3) fp32 un-projected points (0 where not prompted).  At most 4096 bins.  A negative id casts no vote; with
    ``num_clusters`` given, neither does an id >= num_clusters.  Inputs are read, never modified."""
    if not torch.is_tensor(points) or points.device.type != "cuda" or not torch.is_tensor(depth) or depth.device.type != "cuda":
        raise RuntimeError("lift_votes runs on the GPU only (there is no CPU path)")
    ids, bins = _lift_ids("lift_votes", cluster_ids, points, num_clusters)
    H, W = int(viewpoint_camera.image_height), int(viewpoint_camera.image_width)
    votes, index, pts = _lift_call("lift_votes", depth, viewpoint_camera, points, mask=prompt_mask, ids=ids, bins=bins,
                                   want_index=return_index, want_points=return_points)
    votes = votes.to(torch.int64) if votes is not None else torch.zeros(0, dtype=torch.int64, device=depth.device)
    out = (votes,)
    if return_index:
        out += (index.view(H, W).to(torch.int64),)
    if return_points:
        out += (pts.view(H, W, 3),)
    return out[0] if len(out) == 1 else out


def prompt_clusters(depth: torch.Tensor, prompt_mask: torch.Tensor, viewpoint_camera, points: torch.Tensor,
                    cluster_ids: torch.Tensor, threshold, *, num_clusters: int | None = None) -> torch.Tensor:
    """The ids with ``lift_votes(...) > threshold``, ascending, 1-D int64 on the device: what render.py:229-231 prints and
    gui.py:1056-1062 feeds on.  Can be passed straight to ``segment_mask``."""
    votes = lift_votes(depth, prompt_mask, viewpoint_camera, points, cluster_ids, num_clusters=num_clusters)
    return torch.nonzero(votes > threshold).flatten()


def pick(depth: torch.Tensor, pixels, viewpoint_camera, points: torch.Tensor, *, return_points: bool = False):
    """Nearest-point indices, int64 (M,), of the M ``(col, row)`` pixels (an (M, 2) integer tensor, or a sequence of pairs,
    or one pair): the click path of gui.py:786-800.  Pairs given on the host are checked against the image size; a pair
    outside the image in a device tensor gives -1."""
    if not torch.is_tensor(points) or points.device.type != "cuda" or not torch.is_tensor(depth) or depth.device.type != "cuda":
        raise RuntimeError("pick runs on the GPU only (there is no CPU path)")
    dev = depth.device
    W, H = int(viewpoint_camera.image_width), int(viewpoint_camera.image_height)
    if not (torch.is_tensor(pixels) and pixels.device.type == "cuda"):
        host = torch.as_tensor(pixels).reshape(-1, 2).to(torch.int32)
        if host.numel() and (bool((host < 0).any()) or int(host[:, 0].max()) >= W or int(host[:, 1].max()) >= H):
            raise ValueError(f"pick: a pixel lies outside the {W} x {H} image")
        pixels = host.pin_memory().to(dev, non_blocking=True) if host.numel() else host.to(dev)
    if pixels.dim() != 2 or pixels.shape[1] != 2:
        raise ValueError(f"pick: pixels must be (M, 2) (col, row) pairs, got {tuple(pixels.shape)}")
    pixels = pixels.detach().to(torch.int32).contiguous()
    _, index, pts = _lift_call("pick", depth, viewpoint_camera, points, pixels=pixels, want_index=True, want_points=return_points)
    index = index.to(torch.int64)
    return (index, pts) if return_points else index
