"""The display stage of the reference's frame loop as HIP kernels (trase_amd/csrc/display.hip): point splats and the PCA
colours of the per-Gaussian features.

``splat_points(points, camera, colors)`` is render.py:247-294 (gui.py:984-1030, gui_standalone.py:1422-1470): every point is
projected once, and all the images asked for -- white dots, cluster colours, PCA colours -- are written from one winner
map.  Deliberate deviations: where several points land in one pixel the HIGHEST point index wins (what a sequential
assignment gives; torch's ``index_put`` with duplicate indices is unordered, so the reference's images are not
reproducible), the projection is evaluated in float64 from the fp32 inputs (pixel membership then does not depend on fp32
accumulation order), and the pixel scale is render.py:251's ``[W, H]`` (gui.py:993 scales by ``[H, W]``, swapped).

``feature_colors(features)`` is ``feature3d_to_rgb`` (render.py:52-59, gui.py:55-62, gui_standalone.py:490-497): the
reference's ``q @ (U[:, :3] diag(s[:3]))`` of the QR / SVD of the centred matrix Xc equals ``Xc @ V[:, :3]`` with V the top
eigenvectors of ``Xc^T Xc``.  The D x D Gram matrix is reduced on the device in a fixed order, its eigen-decomposition is
``numpy.linalg.eigh`` in float64 on the host (one read-back of D * D + D floats), and the projection, the global min / max
and the normalisation run on the device.  Deliberate deviation: the sign of each axis is fixed so that its component of
largest magnitude is positive (LAPACK's signs are arbitrary, and a flipped axis changes the colours).

Only CUDA tensors are accepted: there is no CPU path."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .rasterizer import _stream
from .segment import _device_index

SPLAT_MAX_LAYERS = 4
FEATURE_MAX_D = 64


def splat_points(points: torch.Tensor, viewpoint_camera, colors=None, *, white_background: bool = False,
                 mask: torch.Tensor | None = None, return_index: bool = False):
    """Point-cloud images of ``points`` (N, 3) fp32 -- the deformed positions ``xyz + d_xyz`` -- seen through
    ``viewpoint_camera`` (anything with ``full_proj_transform``, ``image_width``, ``image_height``).

    ``colors`` is None, one (N, 3) fp32 tensor, or a list / tuple of 1 to 4 entries, each None or an (N, 3) fp32 tensor.
    None is the "Point Cloud" mode: dots of 1 on a black image, of 0 on a white one (render.py:258-260).  ``mask`` (N,) bool
    selects the rows that take part (the viewer's ``points[segmented_mask]``, gui.py:1002-1005).

    A point lands at column ``trunc(px)``, row ``trunc(py)``, ``px = (p.x / p.w + 1) / 2 * W``, ``py`` likewise with H,
    ``p = [x, y, z, 1] @ full_proj_transform``, if ``0 < px < W`` and ``0 < py < H``.  There is no near-plane or ``w > 0``
    test, as in the reference: a point behind the camera lands where its flipped projection falls.  A non-finite ``px`` or
    ``py`` lands nowhere.  The highest point index landing in a pixel wins it.

    -> one (3, H, W) fp32 image per entry of ``colors`` (a list if a list or tuple was given), 0 -- or 1 with
    ``white_background`` -- where no point lands; with ``return_index`` also the (H, W) int64 map of the winning row of
    ``points``, -1 where none landed.  Bitwise reproducible.  Inputs are read, never modified."""
    if not torch.is_tensor(points) or points.device.type != "cuda":
        raise RuntimeError("splat_points runs on the GPU only (there is no CPU path)")
    dev = points.device
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"splat_points: points must be (N, 3), got {tuple(points.shape)}")
    as_list = isinstance(colors, (list, tuple))
    layers = list(colors) if as_list else [colors]
    if not 1 <= len(layers) <= SPLAT_MAX_LAYERS:
        raise ValueError(f"splat_points: 1 to {SPLAT_MAX_LAYERS} colour layers, got {len(layers)}")
    pts = points.detach().float().contiguous()
    N = pts.shape[0]
    W, H = int(viewpoint_camera.image_width), int(viewpoint_camera.image_height)
    for l, c in enumerate(layers):
        if c is None:
            continue
        if not torch.is_tensor(c) or c.device.type != "cuda":
            raise RuntimeError("splat_points runs on the GPU only (there is no CPU path)")
        if tuple(c.shape) != (N, 3):
            raise ValueError(f"splat_points: colors must be ({N}, 3), got {tuple(c.shape)}")
        layers[l] = c.detach().to(dev).float().contiguous()
    if mask is not None:
        if not torch.is_tensor(mask) or mask.device.type != "cuda":
            raise RuntimeError("splat_points runs on the GPU only (there is no CPU path)")
        if mask.numel() != N:
            raise ValueError(f"splat_points: {mask.numel()} mask entries for {N} points")
        mask = mask.detach().reshape(-1).to(dev)
        mask = (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous().view(torch.uint8)
    # the matrix as stored, widened to float64 (one small device-to-host copy unless the camera keeps it on the CPU)
    full = viewpoint_camera.full_proj_transform.detach().to("cpu", torch.float64).numpy()
    if full.shape != (4, 4):
        raise ValueError(f"splat_points: full_proj_transform must be (4, 4), got {full.shape}")
    proj = (C.c_double * 16)(*full.reshape(-1).tolist())
    lib = _lib.load()
    sz = C.c_size_t()
    _lib.check(lib.trase_splat_sizes(N, W, H, C.byref(sz)), "splat_points")
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    L = len(layers)
    images = [torch.empty(3, H, W, dtype=torch.float32, device=dev) for _ in range(L)]
    index = torch.empty(H, W, dtype=torch.int64, device=dev) if return_index else None
    color_ptrs = (C.c_void_p * 4)(*[c.data_ptr() if c is not None and N else None for c in layers])
    image_ptrs = (C.c_void_p * 4)(*[im.data_ptr() for im in images])
    _lib.check(lib.trase_splat_points(_lib.ptr(pts) if N else None, N, _lib.ptr(mask) if N else None, C.byref(proj), W, H,
                                      C.byref(color_ptrs), L, int(bool(white_background)), C.byref(image_ptrs), _lib.ptr(index),
                                      _lib.ptr(ws), ws.numel(), _device_index(dev), _stream(dev)), "splat_points")
    out = images if as_list else images[0]
    return (out, index) if return_index else out


def _fix_signs(axes: np.ndarray) -> np.ndarray:
    """Each row's component of largest magnitude made positive."""
    lead = axes[np.arange(axes.shape[0]), np.abs(axes).argmax(axis=1)]
    return axes * np.where(lead < 0, -1.0, 1.0)[:, None]


def feature_colors(features: torch.Tensor, n_components: int = 3, *, return_basis: bool = False):
    """``feature3d_to_rgb`` (render.py:52-59): the (N, 3) fp32 colours in [0, 1] of features (N, D) or (N, 1, D) fp32,
    1 <= D <= 64, N >= 2 -- the projections on the three principal axes, normalised with the single global
    ``(v - min) / (max - min)`` of render.py:58.  For D < 3 the missing axes are zero.  If ``max == min`` (all centred rows
    zero) the result is what the reference's 0 / 0 gives: NaN everywhere.

    With ``return_basis`` also ``(axes (3, D) float64, mean (D,) float64)``, numpy arrays: the axes as projected on
    (each with its component of largest magnitude positive) and the column means the device computed.  Bitwise reproducible.
    The input is read, never modified."""
    if int(n_components) != 3:
        raise ValueError(f"feature_colors: n_components must be 3 (the reference uses nothing else), got {n_components}")
    if not torch.is_tensor(features) or features.device.type != "cuda":
        raise RuntimeError("feature_colors runs on the GPU only (there is no CPU path)")
    dev = features.device
    if features.dim() == 3 and features.shape[1] == 1:
        features = features.squeeze(1)
    if features.dim() != 2:
        raise ValueError(f"feature_colors: features must be (N, D) or (N, 1, D), got {tuple(features.shape)}")
    X = features.detach().float().contiguous()
    N, D = X.shape
    lib = _lib.load()
    sz = C.c_size_t()
    _lib.check(lib.trase_feature_gram_sizes(N, D, C.byref(sz)), "feature_colors")     # validates N, D first
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    gram_mean = torch.empty(D * D + D, dtype=torch.float32, device=dev)
    idx, stream = _device_index(dev), _stream(dev)
    _lib.check(lib.trase_feature_gram(_lib.ptr(X), N, D, _lib.ptr(gram_mean), _lib.ptr(ws), ws.numel(), idx, stream), "feature_colors")
    host = gram_mean.cpu().numpy().astype(np.float64)             # the one read-back
    gram, mean = host[:D * D].reshape(D, D), host[D * D:]
    _, vec = np.linalg.eigh((gram + gram.T) / 2)                  # ascending eigenvalues
    axes = np.zeros((3, D))
    top = min(3, D)
    axes[:top] = _fix_signs(vec[:, ::-1][:, :top].T)
    dev_axes = torch.from_numpy(axes.astype(np.float32)).pin_memory().to(dev, non_blocking=True)
    out = torch.empty(N, 3, dtype=torch.float32, device=dev)
    minmax = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.check(lib.trase_feature_project(_lib.ptr(X), N, D, _lib.ptr(dev_axes), C.c_void_p(gram_mean.data_ptr() + 4 * D * D),
                                         _lib.ptr(out), _lib.ptr(minmax), idx, stream), "feature_colors")
    return (out, (axes, mean)) if return_basis else out
