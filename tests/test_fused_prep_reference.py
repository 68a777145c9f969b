"""tests/fused_prep_reference.py (the float64 restatement of render()'s prep that tests/test_gpu_fused_prep_edges.py compares the
fused per-Gaussian kernels with) against the arguments the imported reference's own render() handed to the rasterizer for its
eleven call patterns (tests/golden/render_prep.npz).

Bar: 16 * 2^-24 of each row's largest magnitude -- the fixture is the reference's own float32 arithmetic (a handful of roundings
per entry: exp / sigmoid / normalise / a 4-term dot product and a division under is_6dof), the restatement is float64.
Measured maximum over all patterns and arguments: 12.8 * 2^-24 of the row's largest magnitude (cov3D_precomp of cov_python: two
3x3 products on top of the activations); every other argument stays below 3.2 * 2^-24."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import raster_oracle as ro
from oracle.cpu_preprocess import reference_cpu_preprocess
from tests import fused_prep_reference as FR

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "render_prep.npz"))
KW = ("means3D", "means2D", "shs", "sh_objs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")
CASES = [str(x) for x in G["names"]]
BAR = 16.0 * 2.0 ** -24
T = lambda k: torch.from_numpy(np.asarray(G[k]))


def _raw():
    return {k: T("pc_" + k) for k in FR.RAW}


def _pattern(name):
    """-> (make_leaves keywords, prep_args keywords) of one recorded call pattern (tests/test_gpu_render_prep.py::_call)"""
    d = dict(d_xyz=T("d_xyz"), d_rotation=T("d_rotation"), d_scaling=T("d_scaling"))
    kw = dict(sh_degree=int(G[f"{name}__rs_sh_degree"]), scaling_modifier=float(G[f"{name}__rs_scale_modifier"]),
              convert_SHs_python=name == "shs_python", compute_cov3D_python=name == "cov_python")
    if name == "float0":
        d = {}
    elif name == "sixdof":
        d["d_xyz"] = T("T44"); kw["is_6dof"] = True
    elif name == "sixdof_float":
        d["d_xyz"] = 0.0; kw["is_6dof"] = True
    elif name == "mask":
        kw["mask"] = T("mask")
    elif name == "override":
        d["override_color"] = T("override_color")
    elif name == "nonorm":
        kw["norm_gaussian_features"] = False
    elif name == "smooth":
        torch.manual_seed(int(G["smooth__seed"]))           # scene/gaussian_model.py:98: torch.randperm(K)[:int(K * dropout)]
        kw["smooth"] = (T("smooth__knn_idx").long(), torch.randperm(16)[:8])
    return d, kw


@pytest.mark.parametrize("name", CASES)
def test_restatement_hands_the_rasterizer_what_the_reference_does(name):
    d, kw = _pattern(name)
    leaves = FR.make_leaves(_raw(), **d)
    args = FR.prep_args(leaves, T(f"{name}__rs_campos"), **kw)
    worst = 0.0
    for k in KW:
        got, none = args[k], bool(G[f"{name}__{k}__none"])
        assert (got is None) == none, f"{name}: {k} None-ness differs from the reference"
        if none:
            continue
        want = torch.from_numpy(G[f"{name}__{k}"]).double()
        assert tuple(got.shape) == tuple(want.shape), f"{name}: {k} shape {tuple(got.shape)} vs {tuple(want.shape)}"
        got, want = got.detach().reshape(want.shape[0], -1), want.reshape(want.shape[0], -1)
        scale = want.abs().amax(dim=1, keepdim=True)
        err = ((got - want).abs() / scale.clamp_min(1e-30)).max().item() if bool((scale > 0).any()) else float((got - want).abs().max())
        worst = max(worst, err)
        print(f"{name}: {k}: {err / 2.0 ** -24:.2f} * 2^-24 of the row's largest magnitude")
        assert err <= BAR, f"{name}: {k} differs from the reference's argument by {err:.3e} of the row scale (bar {BAR:.3e})"
    assert worst > 0 or name == "float0"                     # (the comparison is float64 against float32: never trivially exact)


def test_settings_record_is_the_reference_one():
    cam = types.SimpleNamespace(FoVx=float(G["FoVx"]), FoVy=float(G["FoVy"]), image_height=int(G["H"]), image_width=int(G["W"]),
                                world_view_transform=T("world_view_transform"), full_proj_transform=T("full_proj_transform"),
                                camera_center=T("camera_center"))
    st = FR.settings_of(cam, T("bg"), sh_degree=3, scaling_modifier=0.7)
    for k in ("image_height", "image_width", "sh_degree"):
        assert int(getattr(st, k)) == int(G[f"modifier__rs_{k}"]), k
    for k in ("tanfovx", "tanfovy", "scale_modifier"):
        assert abs(float(getattr(st, k)) - float(G[f"modifier__rs_{k}"])) < 1e-7, k
    for k in ("bg", "viewmatrix", "projmatrix", "campos"):
        assert np.array_equal(getattr(st, k).numpy(), G[f"modifier__rs_{k}"]), k


def test_oracle_preprocess_on_these_arguments_reproduces_the_cpu_preprocess_geometry():
    """Plain pattern: the projected centres of oracle/cpu_preprocess.py (the reference's own float32 Python projection,
    render.py:247-251: (ndc + 1) / 2 * size) are the oracle's pixel centres + 0.5, and its activations are the arguments."""
    d, kw = _pattern("plain")
    leaves = FR.make_leaves(_raw(), **d)
    args = FR.prep_args(leaves, T("plain__rs_campos"), **kw)
    cam = types.SimpleNamespace(FoVx=float(G["FoVx"]), FoVy=float(G["FoVy"]), image_height=int(G["H"]), image_width=int(G["W"]),
                                world_view_transform=T("world_view_transform"), full_proj_transform=T("full_proj_transform"),
                                camera_center=T("camera_center"))
    st = FR.settings_of(cam, T("bg"))
    g = ro.preprocess(st, args["means3D"], args["shs"], None, args["opacities"], args["scales"], args["rotations"], None)
    ref = reference_cpu_preprocess(T("pc_xyz"), T("pc_features_dc"), T("pc_features_rest"), T("pc_opacity"), T("pc_scaling"),
                                   T("pc_rotation"), T("pc_gaussian_features"), T("d_xyz"), T("d_rotation"), T("d_scaling"),
                                   T("full_proj_transform"), T("camera_center"), int(G["W"]), int(G["H"]))
    vis = g.valid
    assert int(vis.sum()) > 30
    want = ref["pts2d"].double()[vis]
    got = g.xy.detach()[vis] + 0.5
    # float32 projection: a 4-term dot product per clip coordinate, one division, one affine map; 16 * 2^-24 of the image size
    # (the oracle's own 1e-7 added to the clip w is 3e-8 relative at these depths)
    bar = BAR * max(int(G["W"]), int(G["H"]), float(want.abs().max()))
    err = float((got - want).abs().max())
    print(f"centres: {err:.3e} px (bar {bar:.3e})")
    assert err <= bar
    # the SH colour of the same arguments is the cpu preprocess's Python-route colour when the directions agree (undeformed xyz
    # there, means3D here): checked where it is pinned, tests/test_cpu_preprocess.py; here only the covariance route
    cov = ro.cov3d_from_scale_rot(torch.exp(leaves["scaling"]), leaves["rotation"] / leaves["rotation"].norm(dim=1, keepdim=True), 1.0)
    c_want = ref["cov3D_precomp"].double()
    c_err = ((cov.detach() - c_want).abs() / c_want.abs().amax(dim=1, keepdim=True)).max().item()
    assert c_err <= BAR, c_err
