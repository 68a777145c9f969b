"""``render_layers``: the view and up to ten per-Gaussian colour layers of it from ONE rasterizer pass
(trase_amd/csrc/layers.hip).

The reference rasterises the same geometry once per colouring: render.py:197, :240 and :296 call ``render()`` three times
per view (the image, ``override_color=gaussians_feature_pca``, ``override_color=cluster_point_colors``), gui.py:1067-1068
and :1077 twice per frame.  Every call repeats preprocess, depth sort, pair lists, pair sort and compositing.  The forward
composites 32 feature channels beside the colour, by the colour channels' own arithmetic (DESIGN.md "Colour layers in
the feature channels"), and the display loop never reads them: a colour table placed in channels ``3l .. 3l+2`` comes out
with the bits ``render(override_color=table)`` gives, once the background term of the colour epilogue is added.  So:
``trase_layers_pack`` (the tables -> one (N, 32) feature block), the fused raw forward with that block as its features,
unnormalised, transmittance kept, and ``trase_layers_finish`` (the background term, and the 8-bit frames).

Forward only.  Only CUDA tensors are rendered: there is no CPU path."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import rasterizer as _r
from . import renderer as _rn
from .rasterizer import _prep, _stream
from .segment import _device_index

MAX_LAYERS = _lib.LAYERS_MAX
FEATURE_CHANNELS = 32


def _check_tables(colors, N: int, device) -> list:
    """The refusals of ``colors``; -> the tables as a list.  Nothing is launched."""
    if not isinstance(colors, (list, tuple)):
        raise ValueError("render_layers: colors must be a list of (N, 3) fp32 tensors")
    if not 1 <= len(colors) <= MAX_LAYERS:
        raise ValueError(f"render_layers: between 1 and {MAX_LAYERS} colour tables ({FEATURE_CHANNELS} feature channels carry "
                         f"three each), got {len(colors)}")
    for l, c in enumerate(colors):
        if not torch.is_tensor(c) or c.dtype != torch.float32 or tuple(c.shape) != (N, 3):
            what = f"{c.dtype} {tuple(c.shape)}" if torch.is_tensor(c) else type(c).__name__
            raise ValueError(f"render_layers: colors[{l}] must be an fp32 tensor of shape ({N}, 3), got {what}")
        if c.device != device:
            raise ValueError(f"render_layers: colors[{l}] is on {c.device}, the model on {device}")
    return list(colors)


def pack_tables(tables, out: torch.Tensor = None) -> torch.Tensor:
    """``trase_layers_pack``: 1 to 10 (P, 3) fp32 device tables (any strides or storage offset) -> the (P, 32) fp32 block whose
    row i is ``[tables[0][i], tables[1][i], ..., 0 ... 0]``.  One launch, no synchronisation."""
    if len(tables) == 0 or not torch.is_tensor(tables[0]):
        raise ValueError("pack_tables: colors must be a non-empty list of tensors")
    P, dev = int(tables[0].shape[0]), tables[0].device
    tabs = _check_tables(tables, P, dev)
    if dev.type != "cuda":
        raise RuntimeError("trase_amd.layers runs on the GPU only (there is no CPU path)")
    tabs = [t.detach() if t.is_contiguous() else t.detach().contiguous() for t in tabs]
    if out is None:
        out = torch.empty(P, FEATURE_CHANNELS, device=dev)
    ptrs = (C.c_void_p * len(tabs))(*[t.data_ptr() for t in tabs])
    _lib.check(_lib.load().trase_layers_pack(ptrs, len(tabs), P, _lib.ptr(out), _device_index(dev), _stream(dev)), "trase_layers_pack")
    return out


def finish_planes(planes: torch.Tensor, img_ws, bg, L: int, *, image=None, frames_u8: bool = False):
    """``trase_layers_finish`` on ``planes`` ((>= 3L, H, W) fp32, contiguous; finished in place): with ``img_ws`` (the img workspace
    a forward left its transmittance in) ``planes[3l + c] = fma(T, bg[c], planes[3l + c])``; with ``img_ws=None`` the planes are
    final already.  ``frames_u8``: -> the (1 + L, H, W, 3) uint8 frames of ``image`` and of the layers, else None."""
    dev = planes.device
    H, W = int(planes.shape[1]), int(planes.shape[2])
    u8 = torch.empty(1 + L, H, W, 3, dtype=torch.uint8, device=dev) if frames_u8 else None
    ws = None
    if img_ws is not None:
        ws = _lib.RastWorkspace()
        ws.img, ws.img_bytes = _lib.ptr(img_ws), img_ws.numel()
    _lib.check(_lib.load().trase_layers_finish(
        _lib.ptr(planes), C.byref(ws) if ws is not None else None, _lib.ptr(bg), L, W, H, _lib.ptr(image) if frames_u8 else None,
        _lib.ptr(u8[0]) if frames_u8 else None, _lib.ptr(u8[1:]) if frames_u8 else None, _device_index(dev), _stream(dev)),
        "trase_layers_finish")
    return u8


def _one_pass(pc, pipe, d_xyz, d_rotation, d_scaling, is_6dof, mask) -> bool:
    """Whether ``render()`` of these arguments runs the fused forward on the F = 32 compositing kernel over the whole image --
    the kernel whose feature channels carry the layers.  Anything else is composed of ``render()`` calls."""
    if not _rn._fusable(pc, pipe, d_xyz, d_rotation, d_scaling, is_6dof, None, mask, False):
        return False
    if _rn._FORWARD_SCOPE != "all" or int(pc._gaussian_features.shape[-1]) != FEATURE_CHANNELS:
        return False                     # (render() itself composites on another kernel then)
    return _r._Policy.tile_rows == (0, 0) and not (_r._Policy.variant & _r.VARIANT_VALU_FORWARD)


def render_layers(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, d_xyz, d_rotation, d_scaling, is_6dof=False,
                  scaling_modifier=1.0, *, colors, mask=None, frames_u8=False) -> dict:
    """``render()`` of the view and ``render(override_color=c)["render"]`` for every ``c`` of ``colors`` -- 1 to 10 fp32 (N, 3)
    device tables, any strides or storage offset -- from one rasterizer pass.  Returns
      ``render``, ``depth``, ``radii``, ``visibility_filter``, ``viewspace_points``: what ``render()`` returns for the same
                     arguments (under ``mask`` the subset's radii);
      ``layers``     a list of (3, H, W) fp32 tensors, bit-identical to ``render(..., override_color=colors[l], mask=mask)["render"]``
                     (views of one buffer);
      with ``frames_u8`` also ``render_u8`` and ``layers_u8``: (H, W, 3) uint8, ``to8b(x).transpose(1, 2, 0)`` of render.py:106 --
                     ``trunc(255 * clip(x, 0, 1))`` in fp32, a NaN gives 0.
    There is no ``render_gaussian_features`` entry: the feature channels carry the layers.

    Forward only: it runs as under ``torch.no_grad()`` whatever the caller's grad mode, returns tensors without history and
    never modifies its inputs.  The layers' background is ``bg_color``: a feature background of the lineage switch
    (``rasterizer.set_lineage(feats_bg=...)``) is cleared for this one call and is in place again afterwards.  Arguments whose
    ``render()`` does not run the fused F = 32 forward over the whole image are composed of ``1 + len(colors)`` calls of
    ``render()``: the values are the same either way.  ``ValueError`` before any launch for an empty list, more than ten
    tables, a wrong shape or dtype, a table on another device; ``RuntimeError`` inside ``render_views()``."""
    N = int(pc._xyz.shape[0])
    device = pc._xyz.device
    tabs = _check_tables(colors, N, device)
    if _rn._PAIR is not None:
        raise RuntimeError("render_layers cannot run inside render_views(): its forward is finished by a launch of its own")
    L = len(tabs)
    render = _rn.render
    with torch.no_grad():
        if not _one_pass(pc, pipe, d_xyz, d_rotation, d_scaling, is_6dof, mask):
            base = render(viewpoint_camera, pc, pipe, bg_color, d_xyz, d_rotation, d_scaling, is_6dof, scaling_modifier, mask=mask)
            layers = [render(viewpoint_camera, pc, pipe, bg_color, d_xyz, d_rotation, d_scaling, is_6dof, scaling_modifier,
                             override_color=c, mask=mask)["render"] for c in tabs]
            out = {k: base[k] for k in ("render", "depth", "radii", "visibility_filter", "viewspace_points")}
            out["layers"] = layers
            if frames_u8:
                u8 = finish_planes(torch.cat(layers), None, None, L, image=base["render"].contiguous(), frames_u8=True)
                out["render_u8"], out["layers_u8"] = u8[0], list(u8[1:])
            return out

        if device.type != "cuda":
            raise RuntimeError("trase_amd render runs on the GPU only (there is no CPU path)")
        hold = {"gfeat": pack_tables(tabs)}
        saved = (_r._Policy.variant, _r._Policy.feat_bg)
        _r._Policy.variant, _r._Policy.feat_bg = saved[0] & ~_r.VARIANT_FEATS_BG, 0.0
        try:
            res = render(viewpoint_camera, pc, pipe, bg_color, d_xyz, d_rotation, d_scaling, is_6dof, scaling_modifier,
                         mask=mask, norm_gaussian_features=False, _keep_img=hold)
        finally:
            _r._Policy.variant, _r._Policy.feat_bg = saved
        planes = res["render_gaussian_features"]
        bg = _prep(bg_color, "bg_color", device)
        u8 = finish_planes(planes, hold["img"], bg, L, image=res["render"], frames_u8=frames_u8)
        radii = res["radii"] if mask is None else res["radii"][mask]
        out = {"render": res["render"], "depth": res["depth"], "radii": radii, "visibility_filter": radii > 0,
               "viewspace_points": res["viewspace_points"], "layers": [planes[3 * l:3 * l + 3] for l in range(L)]}
        if frames_u8:
            out["render_u8"], out["layers_u8"] = u8[0], list(u8[1:])
        return out
