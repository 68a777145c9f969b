"""The viewer's trajectory view and the end of its frame loop as HIP kernels (trase_amd/csrc/trajectory.hip).

``farthest_point_sample(points, npoint)`` is utils/time_utils.py:375-396 at B = 1: ``npoint`` launches enqueued back to back,
no host read between the steps (the reference's loop costs about eight torch launches and one host synchronisation per
step).  ``TrajectoryOverlay`` is gui.py:1154-1191 (gui_standalone.py:1592-1629): it picks the tracked Gaussians once, keeps
their last ``samp_num`` world positions in a ring on the device and draws the projected polylines into the (H, W, 4) overlay
there; ``draw_trajectories`` is its stateless form.  ``present_frame`` is gui.py:1080-1122: depth normalisation, bilinear
resize, HWC / clamp and the three blends the reference does in numpy on the host.

Deliberate deviations: equal distances in the sampler go to the lowest row; the line rule is this
repository's own (the reference draws with OpenCV's clipped Bresenham); pixel coordinates are scaled by ``[W, H]``
(gui.py:1179 has them swapped); a sample whose pixel coordinate is non-finite or at least 2^20 in magnitude breaks its
polyline; lines are one pixel thick.  The projection is float64 from the fp32 positions, with no ``w > 0`` test (deviation 6).

Only CUDA tensors are accepted: there is no CPU path."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .rasterizer import _stream
from .segment import _device_index

FPS_MAX_BLOCKS = 256            # TRASE_FPS_MAX_BLOCKS
FPS_MAX_SAMPLES = 65536         # TRASE_FPS_MAX_SAMPLES
TRAJ_MAX_TRACKS = 65536         # TRASE_TRAJ_MAX_TRACKS
TRAJ_MAX_SAMPLES = 1024         # TRASE_TRAJ_MAX_SAMPLES

# matplotlib's "jet": the (x, y) breakpoints of its piecewise-linear red, green and blue
_JET = (((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
        ((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
        ((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0)))


def jet_colors(gs_num: int) -> np.ndarray:
    """gui.py:1183 / :1188 without matplotlib: ``int32(jet(i / max(1, gs_num - 1))[:3] * 255) / 255`` for i < gs_num as a
    (gs_num, 3) fp32 array.  jet is looked up as matplotlib does: a 256-entry table, entry ``min(int(x * 256), 255)``."""
    grid = np.linspace(0.0, 1.0, 256)
    table = np.stack([np.interp(grid, [p[0] for p in ch], [p[1] for p in ch]) for ch in _JET], axis=1)
    x = np.arange(gs_num) / max(1, float(gs_num - 1))
    rows = np.minimum((x * 256).astype(np.int64), 255)
    return ((table[rows] * 255).astype(np.int32) / 255).astype(np.float32)


def _gpu(t, what: str) -> None:
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the GPU only (there is no CPU path)")


def _proj(viewpoint_camera, what: str):
    """(the 16 doubles of full_proj_transform as stored, W, H)"""
    full = viewpoint_camera.full_proj_transform
    full = full.detach().to("cpu", torch.float64).numpy() if torch.is_tensor(full) else np.asarray(full, dtype=np.float64)
    if full.shape != (4, 4):
        raise ValueError(f"{what}: full_proj_transform must be (4, 4), got {full.shape}")
    return (C.c_double * 16)(*full.reshape(-1).tolist()), int(viewpoint_camera.image_width), int(viewpoint_camera.image_height)


def _bool_mask(mask, n: int, dev, what: str) -> torch.Tensor:
    _gpu(mask, what)
    if mask.numel() != n:
        raise ValueError(f"{what}: {mask.numel()} mask entries for {n} points")
    mask = mask.detach().reshape(-1).to(dev)
    return (mask if mask.dtype == torch.bool else mask != 0).contiguous()


def farthest_point_sample(points: torch.Tensor, npoint: int, *, mask: torch.Tensor | None = None, start: int | None = None) -> torch.Tensor:
    """utils/time_utils.py:375-396 at B = 1 over ``points`` (N, 3) or (1, N, 3) fp32 -> (npoint,) int64 rows of ``points``.

    ``mask`` (N,) bool selects the candidate rows (the viewer's ``gs_xyz[opacity_mask]``); the result still indexes
    ``points``.  The running minimum distance starts at 1e10, the update is strict ``<`` on
    ``d = (dx*dx + dy*dy) + dz*dz`` with every product and sum rounded to fp32, the next point is the arg-max and equal
    distances go to the lowest row; with ``npoint`` larger than the number of distinct candidates the lowest candidate row
    repeats once every distance is 0.

    ``start`` is the first row; None draws ``torch.randint(0, M, (1,))`` on torch's default CPU generator, M the number of
    candidates, and takes the r-th candidate -- the reference's draw, reproduced by ``torch.manual_seed``.  With a mask that
    costs one read-back (the candidate count, or ``mask[start]``).  ValueError if there is no candidate or ``start`` is not
    one.  Bitwise reproducible; the inputs are read, never modified."""
    _gpu(points, "farthest_point_sample")
    if points.dim() == 3 and points.shape[0] == 1:
        points = points[0]
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"farthest_point_sample: points must be (N, 3) or (1, N, 3), got {tuple(points.shape)}")
    dev = points.device
    pts = points.detach().float().contiguous()
    N, npoint = pts.shape[0], int(npoint)
    if not 1 <= npoint <= FPS_MAX_SAMPLES:
        raise ValueError(f"farthest_point_sample: need 1 <= npoint <= {FPS_MAX_SAMPLES}, got {npoint}")
    if N < 1:
        raise ValueError("farthest_point_sample: no candidate point")
    if start is not None and not 0 <= int(start) < N:
        raise ValueError(f"farthest_point_sample: start {start} is not a row of {N} points")
    start_dev = None
    if mask is None:
        first = int(start) if start is not None else int(torch.randint(0, N, (1,)))
    else:
        mask = _bool_mask(mask, N, dev, "farthest_point_sample")
        if start is not None:
            first = int(start)
            if not bool(mask[first]):                                   # the one read-back
                raise ValueError(f"farthest_point_sample: start {first} is a masked row")
        else:
            rows = torch.nonzero(mask).reshape(-1)                      # the one read-back: the candidate count
            if rows.numel() == 0:
                raise ValueError("farthest_point_sample: no candidate point")
            first = 0
            start_dev = rows[int(torch.randint(0, rows.numel(), (1,)))].reshape(1).contiguous()    # stays on the device
    out = torch.empty(npoint, dtype=torch.int64, device=dev)
    dist = torch.empty(N, dtype=torch.float32, device=dev)
    partial = torch.empty(2 * FPS_MAX_BLOCKS, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().trase_fps_sample(_lib.ptr(pts), N, _lib.ptr(None if mask is None else mask.view(torch.uint8)), first,
                                            _lib.ptr(start_dev), npoint, _lib.ptr(out), _lib.ptr(dist), _lib.ptr(partial),
                                            _device_index(dev), _stream(dev)), "farthest_point_sample")
    return out


def _colors(colors, gs_num: int, dev, what: str) -> torch.Tensor:
    if colors is None:
        return torch.from_numpy(jet_colors(gs_num)).to(dev)
    colors = torch.as_tensor(colors, dtype=torch.float32).detach().to(dev).contiguous()
    if tuple(colors.shape) != (gs_num, 3):
        raise ValueError(f"{what}: colors must be ({gs_num}, 3), got {tuple(colors.shape)}")
    return colors


def _draw(coords, S, G, first, cap, viewpoint_camera, colors, out, return_index, what):
    proj, W, H = _proj(viewpoint_camera, what)
    dev = coords.device
    if out is None:
        out = torch.empty(H, W, 4, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (H, W, 4) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous ({H}, {W}, 4) fp32 tensor on {dev}")
    winner = torch.empty(H, W, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().trase_trajectory_draw(_lib.ptr(coords), S, G, first, cap, C.byref(proj), W, H, _lib.ptr(colors),
                                                 _lib.ptr(out), _lib.ptr(winner), _device_index(dev), _stream(dev)), what)
    return (out, winner) if return_index else out


def draw_trajectories(coords: torch.Tensor, viewpoint_camera, colors=None, *, out: torch.Tensor | None = None,
                      return_index: bool = False):
    """The (H, W, 4) fp32 overlay gui.py:1177-1191 builds from ``coords`` (S, G, 3) fp32 -- the world positions of G tracked
    points at S samples, oldest first -- seen through ``viewpoint_camera`` (anything with ``full_proj_transform``,
    ``image_width``, ``image_height``): channels 0-2 the colour of the trajectory, channel 3 is 1 where a line passes and 0
    elsewhere.  ``colors`` is (G, 3), default ``jet_colors(G)``.

    A sample lands at ``trunc((p.x / p.w + 1) / 2 * W)``, ``trunc((p.y / p.w + 1) / 2 * H)``, ``p = [x, y, z, 1] @
    full_proj_transform`` in float64, no ``w > 0`` test.  Consecutive samples a, b are joined by: ``dx = |bx - ax| >= dy =
    |by - ay|``: for every integer x from ax to bx, ``y = ay + sign(by - ay) * floor((2 |x - ax| dy + dx) / (2 dx))``;
    otherwise the same with x and y swapped.  Both ends are drawn, one sample draws one pixel, pixels outside the image are
    dropped, and the highest trajectory index passing through a pixel wins it (what drawing i = 0 .. G - 1 in turn leaves).
    A sample with a non-finite pixel coordinate or one of magnitude >= 2^20 breaks its polyline: no segment ending there
    is drawn.

    With ``return_index`` also the (H, W) int32 map of the winning trajectory, -1 where none passes.  Bitwise reproducible."""
    _gpu(coords, "draw_trajectories")
    if coords.dim() != 3 or coords.shape[2] != 3:
        raise ValueError(f"draw_trajectories: coords must be (S, G, 3), got {tuple(coords.shape)}")
    S, G = int(coords.shape[0]), int(coords.shape[1])
    if S > TRAJ_MAX_SAMPLES or not 1 <= G <= TRAJ_MAX_TRACKS:
        raise ValueError(f"draw_trajectories: need S <= {TRAJ_MAX_SAMPLES}, 1 <= G <= {TRAJ_MAX_TRACKS}, got S {S}, G {G}")
    c = coords.detach().float().contiguous()
    return _draw(c, S, G, 0, max(S, 1), viewpoint_camera, _colors(colors, G, c.device, "draw_trajectories"), out, return_index,
                 "draw_trajectories")


class TrajectoryOverlay:
    """gui.py:1154-1191: ``select`` once ("Visualize trajectory"), ``update`` every frame.

    ``gs_num`` trajectories of the last ``samp_num`` positions; ``colors`` (gs_num, 3), default the reference's jet table."""

    def __init__(self, gs_num: int = 512, samp_num: int = 32, colors=None):
        gs_num, samp_num = int(gs_num), int(samp_num)
        if not 1 <= gs_num <= TRAJ_MAX_TRACKS or not 1 <= samp_num <= TRAJ_MAX_SAMPLES:
            raise ValueError(f"TrajectoryOverlay: need 1 <= gs_num <= {TRAJ_MAX_TRACKS}, 1 <= samp_num <= {TRAJ_MAX_SAMPLES}, "
                             f"got {gs_num}, {samp_num}")
        self.gs_num, self.samp_num = gs_num, samp_num
        self._colors_in = colors
        self.colors = None          # (gs_num, 3) fp32 on the device of the points
        self.rows = None            # (gs_num,) int64 rows of the full model
        self.ring = None            # (samp_num, gs_num, 3) fp32 world positions
        self.first = 0              # ring row of the oldest sample
        self.count = 0              # samples held

    def select(self, points: torch.Tensor, opacity: torch.Tensor | None = None, mask: torch.Tensor | None = None, *,
               start: int | None = None) -> torch.Tensor:
        """Picks the tracked rows (gui.py:1158-1166): farthest-point sampling over the rows of ``points`` (N, 3) with
        ``opacity > 0.1`` (opacity (N,) or (N, 1), the activated values) and ``mask`` (N,) bool.  Empties the ring.
        -> the (gs_num,) int64 rows of the full model."""
        _gpu(points, "TrajectoryOverlay.select")
        n = points.shape[-2]
        cand = None
        if opacity is not None:
            _gpu(opacity, "TrajectoryOverlay.select")
            if opacity.numel() != n:
                raise ValueError(f"TrajectoryOverlay.select: {opacity.numel()} opacities for {n} points")
            cand = opacity.detach().reshape(-1).to(points.device) > 0.1
        if mask is not None:
            mask = _bool_mask(mask, n, points.device, "TrajectoryOverlay.select")
            cand = mask if cand is None else cand & mask
        self.rows = farthest_point_sample(points, self.gs_num, mask=cand, start=start)
        self.colors = _colors(self._colors_in, self.gs_num, points.device, "TrajectoryOverlay")
        self.ring = torch.empty(self.samp_num, self.gs_num, 3, dtype=torch.float32, device=points.device)
        self.reset()
        return self.rows

    def reset(self) -> None:
        """Empties the ring; the tracked rows stay."""
        self.first = self.count = 0

    def update(self, points: torch.Tensor, viewpoint_camera, *, out: torch.Tensor | None = None, return_index: bool = False):
        """Appends the tracked rows of ``points`` (N, 3) fp32 -- the deformed positions of this frame -- to the ring, dropping
        the oldest sample once ``samp_num`` are held, and returns the (H, W, 4) fp32 overlay of ``draw_trajectories`` over
        the samples held."""
        if self.rows is None:
            raise RuntimeError("TrajectoryOverlay.update: call select() first")
        _gpu(points, "TrajectoryOverlay.update")
        if points.dim() != 2 or points.shape[1] != 3 or points.device != self.ring.device:
            raise ValueError(f"TrajectoryOverlay.update: points must be (N, 3) on {self.ring.device}, got {tuple(points.shape)}")
        pts = points.detach().float().contiguous()
        dev = pts.device
        slot = (self.first + self.count) % self.samp_num
        _lib.check(_lib.load().trase_trajectory_append(_lib.ptr(pts) if pts.shape[0] else None, pts.shape[0], _lib.ptr(self.rows),
                                                       self.gs_num, C.c_void_p(self.ring[slot].data_ptr()), _device_index(dev),
                                                       _stream(dev)), "TrajectoryOverlay.update")
        if self.count < self.samp_num:
            self.count += 1
        else:
            self.first = (self.first + 1) % self.samp_num
        return _draw(self.ring, self.count, self.gs_num, self.first, self.samp_num, viewpoint_camera, self.colors, out,
                     return_index, "TrajectoryOverlay.update")

    def coords(self) -> torch.Tensor:
        """The samples held, oldest first: (count, gs_num, 3)."""
        order = (self.first + torch.arange(self.count, device=self.ring.device)) % self.samp_num
        return self.ring[order]


def present_frame(image: torch.Tensor, *, size=None, depth: bool = False, control_overlay: torch.Tensor | None = None,
                  overlay: torch.Tensor | None = None, tint: torch.Tensor | None = None, tint_weight: float = 0.3,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """gui.py:1080-1122 in one launch -> the (H, W, 3) fp32 frame, contiguous, on the device (the ``.cpu()`` is the caller's).

    ``image`` is (3, h, w) fp32, or with ``depth`` (1, h, w): all three channels then take
    ``(v - min) / (max - min + 1e-20)`` with the global min and max (two small launches in front).  ``size`` = (H, W),
    default the input's: bilinear resize with ATen's fp32 arithmetic for ``align_corners=False``; equal sizes copy bit for
    bit.  Then, in the reference's order: permute to HWC, clamp to [0, 1], ``control_overlay`` (H, W, 3):
    ``b * (overlay.sum(-1) == 0) + overlay``; ``overlay`` (H, W, 4): ``b * (1 - a) + rgb * a``; ``tint`` (H, W, 3):
    ``b + tint_weight * tint``, not clamped afterwards.  ``out`` reuses a buffer.  The inputs are read, never modified."""
    _gpu(image, "present_frame")
    dev = image.device
    if image.dim() != 3 or image.shape[0] != (1 if depth else 3):
        raise ValueError(f"present_frame: image must be ({1 if depth else 3}, h, w), got {tuple(image.shape)}")
    img = image.detach().float().contiguous()
    h, w = int(img.shape[1]), int(img.shape[2])
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    layers = []
    for name, t, ch in (("control_overlay", control_overlay, 3), ("overlay", overlay, 4), ("tint", tint, 3)):
        if t is not None:
            _gpu(t, "present_frame")
            if tuple(t.shape) != (H, W, ch):
                raise ValueError(f"present_frame: {name} must be ({H}, {W}, {ch}), got {tuple(t.shape)}")
            t = t.detach().to(dev).float().contiguous()
        layers.append(t)
    if out is None:
        out = torch.empty(max(H, 0), max(W, 0), 3, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (H, W, 3) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"present_frame: out must be a contiguous ({H}, {W}, 3) fp32 tensor on {dev}")
    minmax = torch.empty(2, dtype=torch.int32, device=dev) if depth else None
    _lib.check(_lib.load().trase_present_frame(_lib.ptr(img), h, w, int(bool(depth)), H, W, _lib.ptr(layers[0]), _lib.ptr(layers[1]),
                                               _lib.ptr(layers[2]), float(tint_weight), _lib.ptr(out), _lib.ptr(minmax),
                                               _device_index(dev), _stream(dev)), "present_frame")
    return out
