"""TEST INFRASTRUCTURE ONLY -- float64 restatement of what ``render()`` does before and around the rasterizer
(gaussian_renderer/__init__.py:75-135 of the reference), on top of ``oracle/raster_oracle.py``: the reference of the fused
per-Gaussian kernels (``trase_amd/csrc/preprocess_raw.hip``), which apply the same prep in registers.

The leaves are float64 copies of the RAW parameters (and of the deformation / override colour / transforms), so
``torch.autograd`` on the oracle output returns raw-parameter gradients, including the ones only some call patterns have.

    means3D   = xyz + d_xyz                      | is_6dof: h = M [xyz, 1], p = h[:3] / h[3]
    scales    = exp(scaling) + d_scaling         rotations = normalize(rotation, eps 1e-12) + d_rotation
    opacity   = sigmoid(opacity)                 shs = cat(f_dc, f_rest)
    sh_objs   = f / (||f|| + 1e-9)               | f as it is when norm_gaussian_features is False
    override_color                               -> colors_precomp
    pipe.convert_SHs_python                      -> colors_precomp = clamp_min(eval_sh(deg, shs, dir of the UNDEFORMED xyz) + 0.5, 0)
    pipe.compute_cov3D_python                    -> cov3D_precomp from the undeformed exp(scaling) * modifier, normalize(rotation)
    mask                                         -> every argument is indexed by it; gradients and radii scatter back through the index

Pinned by tests/test_fused_prep_reference.py against the arguments the reference's own render() produced
(tests/golden/render_prep.npz)."""
from __future__ import annotations

import math
import types

import torch

from oracle import raster_oracle as ro
from trase_amd.rasterizer import GaussianRasterizationSettings

RAW = ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity", "gaussian_features")


def raw_of(scene) -> dict:
    """The seven raw parameter tensors of a SynthScene / SynthGaussianModel, on the CPU."""
    get = lambda k: getattr(scene, k) if hasattr(scene, k) else getattr(scene, "_" + k)
    return {k: get(k).detach().cpu() for k in RAW}


def settings_of(cam, bg, sh_degree=3, scaling_modifier=1.0):
    """The settings record render() builds from a camera (gaussian_renderer/__init__.py:58-71), CPU tensors."""
    c = lambda t: t.detach().cpu()
    return GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=c(torch.as_tensor(bg, dtype=torch.float32)), scale_modifier=float(scaling_modifier),
        viewmatrix=c(cam.world_view_transform), projmatrix=c(cam.full_proj_transform), sh_degree=int(sh_degree),
        campos=c(cam.camera_center), prefiltered=False, debug=False)


def _leaf(t):
    return t.detach().cpu().double().clone().requires_grad_(True)


def make_leaves(raw, d_xyz=0.0, d_rotation=0.0, d_scaling=0.0, override_color=None) -> dict:
    """float64 leaves: the raw parameters, ``means2D`` (the (N,3) zero dummy whose .grad is the screen-space gradient, full size
    also under a mask) and whichever of d_xyz (or the (N,4,4) transforms) / d_rotation / d_scaling / override_color are tensors."""
    leaves = {k: _leaf(raw[k]) for k in RAW}
    n = raw["xyz"].shape[0]
    leaves["means2D"] = torch.zeros(n, 3, dtype=torch.float64, requires_grad=True)
    for k, v in (("d_xyz", d_xyz), ("d_rotation", d_rotation), ("d_scaling", d_scaling), ("override_color", override_color)):
        if torch.is_tensor(v):
            leaves[k] = _leaf(v)
    return leaves


def prep_args(leaves, campos, sh_degree=3, is_6dof=False, scaling_modifier=1.0, mask=None, norm_gaussian_features=True,
              convert_SHs_python=False, compute_cov3D_python=False, with_features=True, smooth=None) -> dict:
    """The nine rasterizer arguments, float64 and differentiable w.r.t. the leaves.  ``smooth`` = (knn_idx (N,K), selected
    neighbour slots): the KNN-smoothed features of scene/gaussian_model.py:95-101 instead of the raw ones."""
    L = leaves
    xyz = L["xyz"]
    if is_6dof:
        if "d_xyz" in L:
            hom = torch.cat([xyz, torch.ones_like(xyz[:, :1])], dim=-1)
            h = torch.bmm(L["d_xyz"], hom.unsqueeze(-1)).squeeze(-1)
            means3D = h[:, :3] / h[:, 3:]
        else:
            means3D = xyz
    else:
        means3D = xyz + L["d_xyz"] if "d_xyz" in L else xyz
    qn = L["rotation"] / L["rotation"].norm(dim=1, keepdim=True).clamp_min(1e-12)
    scales = rotations = cov = None
    if compute_cov3D_python:
        cov = ro.cov3d_from_scale_rot(torch.exp(L["scaling"]), qn, float(scaling_modifier))
    else:
        scales = torch.exp(L["scaling"]) + L["d_scaling"] if "d_scaling" in L else torch.exp(L["scaling"])
        rotations = qn + L["d_rotation"] if "d_rotation" in L else qn
    opacity = torch.sigmoid(L["opacity"])
    shs = torch.cat((L["features_dc"], L["features_rest"]), dim=1)
    colors = None
    if "override_color" in L:
        colors, shs = L["override_color"], None
    elif convert_SHs_python:
        d = xyz - campos.double().reshape(1, 3)
        d = d / d.norm(dim=1, keepdim=True)
        colors, shs = torch.clamp_min(ro.eval_sh_colors(int(sh_degree), shs, d) + 0.5, 0.0), None
    sh_objs = None
    if with_features:
        sh_objs = L["gaussian_features"]
        if smooth is not None:
            idx, sel = smooth
            sh_objs = torch.nn.functional.normalize(sh_objs, dim=-1, p=2)[idx[:, sel], 0, :].mean(dim=1).unsqueeze(1)
        if norm_gaussian_features:
            sh_objs = sh_objs / (sh_objs.norm(dim=2, keepdim=True) + 1e-9)
    args = dict(means3D=means3D, means2D=L["means2D"], shs=shs, sh_objs=sh_objs, colors_precomp=colors, opacities=opacity,
                scales=scales, rotations=rotations, cov3D_precomp=cov)
    if mask is not None:
        m = mask.detach().cpu()
        args = {k: (None if v is None else v[m]) for k, v in args.items()}
    return args


def activations64(raw, d_xyz=0.0, d_rotation=0.0, d_scaling=0.0, **kw):
    """prep_args without gradients: the float64 activations a per-Gaussian forward row is compared with."""
    with torch.no_grad():
        L = make_leaves(raw, d_xyz, d_rotation, d_scaling)
        return {k: (None if v is None else v.detach()) for k, v in prep_args(L, **kw).items()}


def _full_size(o, mask):
    """Per-Gaussian fields of the subset's oracle output scattered back to all N Gaussians (a removed one has radius 0 and is
    not fragile): what the gradient criterion needs when the gradients are full-size tensors."""
    m = mask.detach().cpu()
    n = m.numel()

    def scat(v, fill=0):
        out = torch.full((n,) + tuple(v.shape[1:]), fill, dtype=v.dtype)
        out[m] = v.detach()
        return out
    return types.SimpleNamespace(radii=scat(o.radii), frag_gauss=scat(o.frag_gauss, False), fragile=o.fragile, tile_mask=o.tile_mask,
                                 geom=types.SimpleNamespace(xy=scat(o.geom.xy), valid=scat(o.geom.valid, False)))


def fused_prep_reference(raw, cam, bg, d_xyz=0.0, d_rotation=0.0, d_scaling=0.0, is_6dof=False, scaling_modifier=1.0,
                         override_color=None, mask=None, norm_gaussian_features=True, convert_SHs_python=False,
                         compute_cov3D_python=False, sh_degree=3, with_features=True, device_view=None, tiles=None):
    """float64 ``render()``: -> (OracleOut, leaves).  ``raw``: dict of the seven raw tensors (``raw_of``).  ``device_view`` and
    ``tiles`` are the oracle's (oracle/raster_oracle.py ``rasterize``); under a mask the device view is given at full size and
    indexed here.  Under a mask the OracleOut describes the SUBSET (like the radii render() returns) and ``out.full`` carries its
    per-Gaussian fields scattered back to full size."""
    leaves = make_leaves(raw, d_xyz, d_rotation, d_scaling, override_color)
    st = settings_of(cam, bg, sh_degree, scaling_modifier)
    args = prep_args(leaves, st.campos, sh_degree=sh_degree, is_6dof=is_6dof, scaling_modifier=scaling_modifier, mask=mask,
                     norm_gaussian_features=norm_gaussian_features, convert_SHs_python=convert_SHs_python,
                     compute_cov3D_python=compute_cov3D_python, with_features=with_features)
    if device_view is not None and mask is not None:
        m = mask.detach().cpu()
        device_view = {k: v[m] for k, v in device_view.items()}
    out = ro.rasterize(st, args["means3D"], args["means2D"], shs=args["shs"], sh_objs=args["sh_objs"],
                       colors_precomp=args["colors_precomp"], opacities=args["opacities"], scales=args["scales"],
                       rotations=args["rotations"], cov3D_precomp=args["cov3D_precomp"], device_view=device_view, tiles=tiles)
    out.full = out if mask is None else _full_size(out, mask)
    return out, leaves
