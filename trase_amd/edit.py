"""Editing and compositing of segmented objects: the reference's ``render_composite`` and its rigid-edit helpers
(gaussian_renderer/__init__.py:158-331) on one HIP kernel per part (trase_amd/csrc/compose.hip).

The reference concatenates a background model with a masked, rescaled, rotated and translated dynamic model out of about 40
torch launches (activations, six boolean gathers, a matmul, a quaternion product from split / concatenate, a normalise, six
``torch.cat``) and rasterises once.  Here every part is written from its RAW parameters straight into the six operator-level
input tensors of the rasterizer at its row offset, in fp32 and in the reference's statement order:

    means = xyz + d_xyz;  scales = exp(_scaling) + d_scaling;  rot = normalize(_rotation) + d_rotation
    opacity = sigmoid(_opacity);  shs = cat(dc, rest);  sh_objs = the features as stored (not normalised)
    rescale (means, scales *= s), rotate (means = R means, rot = normalize(q_edit (x) rot)), translate (means += offset)

Two quirks of the reference are kept: with all three angles exactly zero it returns before the rotation, so ``rot`` stays the
un-renormalised ``normalize(q) + d_rotation``; rescale and rotation are about the world origin.  SH coefficients are not
rotated with the object, as there.

The fused kernel runs when gradients are disabled or no input requires one.  Otherwise -- and for a non-zero float
deformation or an SH layout other than (.,1,3) + (.,15,3) -- the same composition runs as torch ops around the HIP
rasterizer, as ``trase_amd.renderer.render`` does for its own uncovered cases.  Only CUDA tensors are accepted."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer, _stream
from .segment import _device_index

MAX_PARTS = 8


# ---- the rigid-edit helpers, written from the mathematics -----------------------------------------------------------------
def _angle(theta) -> float:
    """A Python float or a one-element tensor -> float64 (a device tensor is read back once)."""
    return float(theta.detach().double().reshape(-1)[0]) if torch.is_tensor(theta) else float(theta)


def _rx64(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _ry64(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _rz64(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def rx(theta):
    """Rotation by ``theta`` radians about the x axis, a (3, 3) fp32 CPU tensor.  ry, rz likewise.  Deviation: a Python
    float is accepted (the reference's takes tensors only); the entries are float64 cos / sin rounded once."""
    return torch.from_numpy(_rx64(_angle(theta)).astype(np.float32))


def ry(theta):
    return torch.from_numpy(_ry64(_angle(theta)).astype(np.float32))


def rz(theta):
    return torch.from_numpy(_rz64(_angle(theta)).astype(np.float32))


def _qvec64(R: np.ndarray) -> np.ndarray:
    """The unit quaternion (r, x, y, z), r >= 0, of a (near-)rotation matrix: the eigenvector of the largest eigenvalue of the
    symmetric 4 x 4 matrix K, q^T K q = trace(R(q)^T R) / 3 in the component order (x, y, z, r)."""
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    _, vec = np.linalg.eigh(K)                          # ascending eigenvalues
    q = vec[[3, 0, 1, 2], -1]
    return -q if q[0] < 0 else q


def rotmat2qvec(R):
    """Quaternion (r, x, y, z), r >= 0, of the (3, 3) rotation matrix ``R``; a tensor like ``R``.  Evaluated in float64 on
    the host."""
    q = _qvec64(R.detach().to("cpu", torch.float64).numpy())
    return torch.from_numpy(q).to(R)


def quat_to_rotmat64(q: np.ndarray) -> np.ndarray:
    """R(q) in the (r, x, y, z) convention of utils/general_utils.py:122-154, float64 (no normalisation)."""
    r, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def rescale(means3d, scales, scale_factor: float):
    return means3d * scale_factor, scales * scale_factor


def _rotate(means3d, rotations, R, q):
    means3d = torch.matmul(means3d, R.T)
    w0, x0, y0, z0 = rotations.unbind(-1)
    w1, x1, y1, z1 = q.unbind(-1)
    # the Hamilton product q (x) rotations, components (r, x, y, z), in the reference's term order
    prod = torch.stack((-x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0,
                        x1 * w0 + y1 * z0 - z1 * y0 + w1 * x0,
                        -x1 * z0 + y1 * w0 + z1 * x0 + w1 * y0,
                        x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0), dim=-1)
    return means3d, prod / torch.linalg.norm(prod, dim=-1, keepdim=True)


def rotate_by_matrix(means3d, rotations, rotation_matrix, keep_sh_degree: bool = True):
    """``means3d @ R^T`` and ``normalize(q(R) (x) rotations)``.  SH coefficients are not rotated (``keep_sh_degree`` is
    accepted and, as in the reference, changes nothing)."""
    R = rotation_matrix.to(rotations)
    return _rotate(means3d, rotations, R, rotmat2qvec(rotation_matrix).to(rotations))


def rotate_by_euler_angles(means3d, rotations, rotation_angles):
    """Rotation ``rx(x) @ ry(y) @ rz(z)`` about the world origin, radians.  All three angles exactly zero: both inputs are
    returned as they are (no renormalisation of ``rotations``)."""
    e = rigid_edit(rotation_angles=rotation_angles)
    if e.zero_angles:
        return means3d, rotations
    return _rotate(means3d, rotations, torch.from_numpy(e.R).to(rotations), torch.from_numpy(e.q).to(rotations))


def translation(means3d, offsets):
    means3d += offsets
    return means3d


def transform(means3d, rotations, scales, scale_factor, offsets, rotation_angles):
    means3d, scales = rescale(means3d, scales, scale_factor)
    means3d, rotations = rotate_by_euler_angles(means3d, rotations, rotation_angles)
    means3d = translation(means3d, offsets)
    return means3d, rotations, scales


# ---- parts ----------------------------------------------------------------------------------------------------------------
class RigidEdit(NamedTuple):
    scale_factor: float
    R: np.ndarray            # (3, 3) fp32: rx(x) @ ry(y) @ rz(z) in float64, rounded once
    q: np.ndarray            # (4,) fp32 (r, x, y, z), r >= 0: rotmat2qvec of the float64 R, rounded once
    offset: np.ndarray       # (3,) fp32
    zero_angles: bool        # all three angles exactly zero: the reference skips the rotation AND the renormalisation
    R64: np.ndarray
    q64: np.ndarray
    raw: tuple               # (scale_factor, offsets) as given, for the differentiable torch composition


def rigid_edit(scale_factor=1.0, rotation_angles=(0.0, 0.0, 0.0), offsets=(0.0, 0.0, 0.0)) -> RigidEdit:
    """The record of one rigid edit: ``means = R (s means) + offsets``, ``scales *= s``, ``rot = normalize(q (x) rot)``.
    Angles (radians) and offsets may be Python floats or tensors; device tensors are read back here, once."""
    x, y, z = (_angle(a) for a in rotation_angles)
    R64 = _rx64(x) @ _ry64(y) @ _rz64(z)
    q64 = _qvec64(R64)
    if torch.is_tensor(offsets):
        off = offsets.detach().to("cpu", torch.float64).reshape(-1).numpy()
    else:
        off = np.array([_angle(o) for o in offsets], dtype=np.float64)
    if off.shape != (3,):
        raise ValueError(f"rigid_edit: offsets must have 3 entries, got {off.shape}")
    s = _angle(scale_factor)
    return RigidEdit(s, R64.astype(np.float32), q64.astype(np.float32), off.astype(np.float32),
                     x == 0.0 and y == 0.0 and z == 0.0, R64, q64, (scale_factor, offsets))


class Part:
    """One part of a composited scene: the model ``pc`` (anything with the reference's raw parameters ``_xyz``, ``_scaling``,
    ``_rotation``, ``_opacity``, ``_features_dc``, ``_features_rest``, ``_gaussian_features``), its deformation (tensors
    indexed by the model's rows, or 0.0), the rows that take part and an optional ``rigid_edit``.

    ``rows``: None (all), a bool (n,) mask -- resolved with ``torch.nonzero`` here, ONE host synchronisation, so build the
    part once per prompt and reuse it every frame -- or an ascending integer index tensor (no synchronisation).  An index
    outside [0, n) is never read by the fused kernel: it yields a null Gaussian (all zeros)."""

    def __init__(self, pc, d_xyz=0.0, d_rotation=0.0, d_scaling=0.0, rows=None, edit: Optional[RigidEdit] = None):
        self.pc, self.d_xyz, self.d_rotation, self.d_scaling, self.edit = pc, d_xyz, d_rotation, d_scaling, edit
        n = pc._xyz.shape[0]
        if rows is not None:
            if not torch.is_tensor(rows) or rows.dim() != 1:
                raise ValueError("Part: rows must be a 1-D bool mask or integer index tensor")
            if rows.dtype == torch.bool:
                if rows.shape[0] != n:
                    raise ValueError(f"Part: {rows.shape[0]} mask entries for {n} Gaussians")
                rows = torch.nonzero(rows).squeeze(1)
            elif rows.dtype in (torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8):
                rows = rows.to(torch.int64)
            else:
                raise ValueError(f"Part: rows must be bool or integer, got {rows.dtype}")
            rows = rows.to(pc._xyz.device).contiguous()
        self.rows = rows

    @property
    def count(self) -> int:
        return int(self.rows.shape[0]) if self.rows is not None else int(self.pc._xyz.shape[0])


_PARAMS = ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest", "_gaussian_features")


def _check_parts(parts):
    parts = list(parts)
    if not 1 <= len(parts) <= MAX_PARTS:
        raise ValueError(f"compose: 1 to {MAX_PARTS} parts, got {len(parts)}")
    dev = parts[0].pc._xyz.device
    if dev.type != "cuda":
        raise RuntimeError("compose runs on the GPU only (there is no CPU path)")
    F = parts[0].pc._gaussian_features.shape[-1]
    for p in parts:
        if p.pc._xyz.device != dev:
            raise ValueError("compose: all parts must live on the same device")
        if p.pc._gaussian_features.shape[-1] != F:
            raise ValueError("compose: all parts must have the same feature width")
    return parts, dev, F


def _fusable(parts) -> bool:
    """The fused kernel covers: nothing to differentiate, tensor-or-zero deformations of the right shape, the
    (.,1,3) + (.,15,3) SH layout, (.,1,F) features with F <= 64."""
    for p in parts:
        pc = p.pc
        n = pc._xyz.shape[0]
        tensors = [getattr(pc, k) for k in _PARAMS]
        for d, c in ((p.d_xyz, 3), (p.d_rotation, 4), (p.d_scaling, 3)):
            if torch.is_tensor(d):
                if tuple(d.shape) != (n, c):
                    return False
                tensors.append(d)
            elif float(d) != 0.0:
                return False
        if p.edit is not None:
            tensors += [t for t in p.edit.raw if torch.is_tensor(t)]
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            return False
        if tuple(pc._features_dc.shape[1:]) != (1, 3) or tuple(pc._features_rest.shape[1:]) != (15, 3):
            return False
        gf = pc._gaussian_features
        if gf.dim() != 3 or gf.shape[1] != 1 or gf.shape[2] > 64:
            return False
    return True


def _f32(t, dev):
    """fp32, contiguous, on ``dev``, 16-byte aligned -- the steady-state parameter as it is."""
    t = t.detach()
    if t.dtype is not torch.float32 or t.device != dev or not t.is_contiguous():
        t = t.to(dev, torch.float32).contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


def _compose_fused(parts, dev, F):
    lib = _lib.load()
    counts = (C.c_int32 * len(parts))(*[p.count for p in parts])
    offsets = (C.c_int64 * (len(parts) + 1))()
    _lib.check(lib.trase_compose_sizes(counts, len(parts), F, offsets), "compose_models")
    P = offsets[len(parts)]
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    means, scales, rots, opac, shs, objs = new(P, 3), new(P, 3), new(P, 4), new(P, 1), new(P, 16, 3), new(P, 1, F)
    idx, stream = _device_index(dev), _stream(dev)
    for k, p in enumerate(parts):
        if p.count == 0:
            continue
        keep = [_f32(getattr(p.pc, name), dev) for name in _PARAMS]
        d = [_f32(t, dev) if torch.is_tensor(t) else None for t in (p.d_xyz, p.d_rotation, p.d_scaling)]
        cp = _lib.ComposePart()
        cp.n, cp.m, cp.F = keep[0].shape[0], p.count, F
        (cp.xyz, cp.scaling, cp.rotation, cp.opacity, cp.features_dc, cp.features_rest,
         cp.gaussian_features) = [t.data_ptr() if t.numel() else None for t in keep]
        cp.rows = p.rows.data_ptr() if p.rows is not None else None
        cp.d_xyz, cp.d_rotation, cp.d_scaling = [t.data_ptr() if t is not None and t.numel() else None for t in d]
        e = p.edit
        cp.edit_mode = 0 if e is None else (1 if e.zero_angles else 2)
        if e is not None:
            cp.scale_factor = e.scale_factor
            cp.R = (C.c_float * 9)(*e.R.reshape(-1).tolist())
            cp.q_edit = (C.c_float * 4)(*e.q.tolist())
            cp.offset = (C.c_float * 3)(*e.offset.tolist())
        _lib.check(lib.trase_compose_part(C.byref(cp), offsets[k], P, _lib.ptr(means), _lib.ptr(scales), _lib.ptr(rots),
                                          _lib.ptr(opac), _lib.ptr(shs), _lib.ptr(objs) if F else None, idx, stream),
                   "compose_models")
    return (means, scales, rots, opac, shs, objs), [int(o) for o in offsets]


def _compose_torch(parts, dev):
    """The reference's statements as differentiable torch ops (the path a training loop takes)."""
    cols = [[] for _ in range(6)]
    offsets = [0]
    for p in parts:
        pc = p.pc
        means = pc._xyz + p.d_xyz
        scales = torch.exp(pc._scaling) + p.d_scaling
        rots = torch.nn.functional.normalize(pc._rotation) + p.d_rotation
        opac = torch.sigmoid(pc._opacity)
        shs = torch.cat((pc._features_dc, pc._features_rest), dim=1)
        objs = pc._gaussian_features
        if p.rows is not None:
            means, scales, rots, opac, shs, objs = (t[p.rows] for t in (means, scales, rots, opac, shs, objs))
        e = p.edit
        if e is not None:
            s, off = e.raw
            means, scales = rescale(means, scales, s)
            if not e.zero_angles:
                means, rots = _rotate(means, rots, torch.from_numpy(e.R).to(rots), torch.from_numpy(e.q).to(rots))
            means = means + (off.to(means) if torch.is_tensor(off) else torch.from_numpy(e.offset).to(means))
        for c, t in zip(cols, (means, scales, rots, opac, shs, objs)):
            c.append(t)
        offsets.append(offsets[-1] + means.shape[0])
    return tuple(torch.cat(c, dim=0) for c in cols), offsets


def compose_models(parts):
    """``(means3D (P,3), scales (P,3), rotations (P,4), opacities (P,1), shs (P,16,3), sh_objs (P,1,F), offsets)`` of 1 to 8
    ``Part``s on one device with the same F: the parts' rows one after the other, each part's rows in the order of its
    ``rows``; ``offsets[k]`` is the first row of part k and ``offsets[-1]`` is P.  The inputs are read, never modified; the
    fused result is bitwise reproducible."""
    parts, dev, F = _check_parts(parts)
    out, offsets = _compose_fused(parts, dev, F) if _fusable(parts) else _compose_torch(parts, dev)
    return (*out, offsets)


def render_parts(viewpoint_camera, parts, bg_color, scaling_modifier=1.0):
    """One rasterisation of the composed parts -> ``{"render", "radii", "render_gaussian_features", "depth"}``.  The SH
    degree is the first part's ``active_sh_degree``; features are rendered as stored (not normalised)."""
    parts, dev, _ = _check_parts(parts)
    means, scales, rots, opac, shs, objs, _ = compose_models(parts)
    raster_settings = GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5), bg=bg_color,
        scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform, sh_degree=parts[0].pc.active_sh_degree,
        campos=viewpoint_camera.camera_center, prefiltered=False, debug=False)
    means2D = torch.zeros_like(means, requires_grad=torch.is_grad_enabled())
    image, radii, feats, depth = GaussianRasterizer(raster_settings=raster_settings)(
        means3D=means, means2D=means2D, shs=shs, sh_objs=objs, colors_precomp=None, opacities=opac, scales=scales,
        rotations=rots, cov3D_precomp=None)
    return {"render": image, "radii": radii, "render_gaussian_features": feats, "depth": depth}


def render_composite(viewpoint_camera, background_gaussian, dynamic_gaussian, d_xyz, d_rotation, d_scaling, bg_color,
                     scales_bias, motion_bias, rotation_bias, scaling_modifier=1.0, mask=None, *, background_mask=None):
    """The reference's ``render_composite`` (gaussian_renderer/__init__.py:251-331), same positional order: the background
    model as it is, then the rows ``mask`` of the dynamic model, deformed, rescaled by ``scales_bias``, rotated by the Euler
    angles ``rotation_bias`` and moved by ``motion_bias``, in one rasterisation.  Returns the reference's ``"render"`` and
    ``"radii"``, ``"render_gaussian_features"``, ``"depth"``.

    ``background_mask`` (an extension): the rows of the BACKGROUND model that take part.  With the same model on both sides
    and ``background_mask=~mask`` one call moves the selected object instead of duplicating it.  Masks may be bool (n,)
    tensors (one host synchronisation each per call) or ascending integer index tensors (none)."""
    parts = [Part(background_gaussian, rows=background_mask),
             Part(dynamic_gaussian, d_xyz, d_rotation, d_scaling, rows=mask,
                  edit=rigid_edit(scales_bias, rotation_bias, motion_bias))]
    return render_parts(viewpoint_camera, parts, bg_color, scaling_modifier)
