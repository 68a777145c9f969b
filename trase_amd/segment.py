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
