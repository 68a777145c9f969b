"""Editing and compositing on the GPU (trase_amd/edit.py over trase_amd/csrc/compose.hip).

(1) compose_models against the float64 restatement (tests/compose_reference.py) within its forward-error bounds, with the row
    count, the row order, untouched inputs and bitwise repeatability;
(2) the fused render_composite under no_grad against the grad-enabled torch composition around the same rasterizer, by the
    project's criterion for fused versus composed paths (tests/test_gpu_render_patterns.py);
(3) moving nothing changes nothing: the parts [~m] and [m, identity edit] of one model against render() of that model;
(4) the fused kernel is what runs under no_grad, and the torch composition carries gradients to both models otherwise;
(5) background_mask=~mask with a pure translation moves the object and leaves the rest of the image alone.
Out-of-range rows are exercised on the host build only (tests/test_compose_hostsim.py), never here."""
import numpy as np
import pytest
import torch

from tests import compose_reference as cr

pytestmark = pytest.mark.gpu

N_BG, N_DYN, W, H = 3000, 2000, 160, 96
RAW = ("xyz", "scaling", "rotation", "opacity", "features_dc", "features_rest", "gaussian_features")
ANGLES, SCALE, OFFSET = (0.3, -1.1, 2.0), 1.2, (0.5, -0.25, 0.4)


def _scene(dev, seed=21, n_bg=N_BG, n_dyn=N_DYN):
    from trase_amd.synthetic import SynthGaussianModel, make_scene, orbit_camera
    bg = SynthGaussianModel(make_scene(n_bg, feat_dim=32, seed=seed, scale_mult=0.8).to(dev))
    dyn = SynthGaussianModel(make_scene(n_dyn, feat_dim=32, seed=seed + 1, scale_mult=0.8).to(dev))
    cam = orbit_camera(W, H, angle=0.7, fid=0.4).to(dev)
    g = torch.Generator().manual_seed(seed + 2)
    d = [(0.02 * torch.randn(n_dyn, c, generator=g)).to(dev) for c in (3, 4, 3)]
    mask = (torch.rand(n_dyn, generator=g) < 0.6).to(dev)
    return bg, dyn, cam, d, mask


def _raw(pc):
    return {k: getattr(pc, "_" + k).detach().cpu().numpy() for k in RAW}


def _close(name, a, b):
    """The criterion of tests/test_gpu_render_patterns.py:81-82 for a fused against a composed path."""
    err = (a - b).abs().amax(0)
    share, worst = (err > 2e-5).float().mean().item(), err.max().item()
    print(f"{name}: share of pixels over 2e-5 = {share:.3e}, max {worst:.3e}")
    assert share < 2e-3 and worst < 5e-2, f"{name}: share {share:.3e}, max {worst:.3e}"


def test_compose_models_against_float64():
    from trase_amd.edit import Part, compose_models, rigid_edit
    dev = torch.device("cuda", 0)
    bg, dyn, _, d, mask = _scene(dev)
    edit = rigid_edit(SCALE, ANGLES, OFFSET)
    before = [p.detach().clone() for p in bg.parameters() + dyn.parameters() + d]
    with torch.no_grad():
        parts = [Part(bg), Part(dyn, d[0], d[1], d[2], rows=mask, edit=edit)]
        a = compose_models(parts)
        b = compose_models(parts)
    torch.cuda.synchronize()
    names = ("means", "scales", "rots", "opac", "shs", "objs")
    n_sel = int(mask.sum())
    assert a[6] == [0, N_BG, N_BG + n_sel] and 0.5 < n_sel / N_DYN < 0.7
    for k, t, u in zip(names, a[:6], b[:6]):
        assert t.shape[0] == N_BG + n_sel and t.dtype == torch.float32 and not t.requires_grad
        assert torch.equal(t, u), f"{k}: two calls differ"
    for p, q in zip(bg.parameters() + dyn.parameters() + d, before):
        assert torch.equal(p.detach(), q)                         # inputs unmodified
    e64 = cr.make_edit(SCALE, ANGLES, OFFSET)
    x, bound, offsets = cr.compose([dict(model=_raw(bg)),
                                    dict(model=_raw(dyn), d_xyz=d[0].cpu().numpy(), d_rotation=d[1].cpu().numpy(),
                                         d_scaling=d[2].cpu().numpy(), rows=mask.cpu().numpy(), edit=e64)])
    assert offsets == a[6]
    got = dict(zip(names, (t.cpu().numpy() for t in a[:6])))
    ratios = {}
    for k in ("means", "scales", "rots", "opac"):
        ratios[k], err = cr.worst(got[k], x[k], bound[k])
        print(f"{k}: max error {err:.3e}, {ratios[k]:.3f} of the bound")
    # (roundings + 2 per transcendental) * 2^-24 * sum of |terms|: means 8, scales 4 (2 + the exp), rotations 16, opacity 4
    assert all(r <= 1.0 for r in ratios.values()), ratios
    # background rows first, then the masked rows ascending: the wide payloads are exact copies in that order
    assert np.array_equal(got["shs"], x["shs"]) and np.array_equal(got["objs"], x["objs"])
    sel = torch.nonzero(mask).squeeze(1)
    assert torch.equal(a[5][N_BG:], dyn._gaussian_features.detach()[sel]) and torch.equal(a[0][:N_BG], bg._xyz.detach())
    # an index tensor gives the same rows as the mask
    with torch.no_grad():
        c = compose_models([Part(bg), Part(dyn, d[0], d[1], d[2], rows=sel, edit=edit)])
    assert all(torch.equal(t, u) for t, u in zip(a[:6], c[:6]))


def _composite(dev, seed, grad):
    from gaussian_renderer import render_composite
    bg, dyn, cam, d, mask = _scene(dev, seed=seed)
    bgc = torch.tensor([0.1, 0.2, 0.3], device=dev)
    angles = [torch.tensor(a) for a in ANGLES]
    with torch.set_grad_enabled(grad):
        out = render_composite(cam, bg, dyn, d[0], d[1], d[2], bgc, SCALE, torch.tensor(OFFSET, device=dev), angles, 1.0, mask)
    return {k: v.detach() for k, v in out.items()}


def test_fused_render_composite_matches_the_torch_composition():
    dev = torch.device("cuda", 0)
    a = _composite(dev, 21, grad=False)
    b = _composite(dev, 21, grad=True)
    assert set(a) == {"render", "radii", "render_gaussian_features", "depth"}
    differ = int((a["radii"] != b["radii"]).sum())
    print(f"radii: {differ} of {a['radii'].numel()} rows differ; visible {int((a['radii'] > 0).sum())}")
    assert torch.equal(a["radii"], b["radii"])
    assert int((a["radii"] > 0).sum()) > 100
    for k in ("render", "render_gaussian_features", "depth"):
        _close(k, a[k], b[k])
    assert tuple(a["render"].shape) == (3, H, W) and tuple(a["render_gaussian_features"].shape) == (32, H, W)


def test_moving_nothing_changes_nothing():
    from trase_amd.edit import Part, render_parts, rigid_edit
    from trase_amd.renderer import render
    from trase_amd.synthetic import SynthPipe
    dev = torch.device("cuda", 0)
    _, dyn, cam, d, mask = _scene(dev, seed=31)
    bgc = torch.tensor([0.1, 0.2, 0.3], device=dev)
    with torch.no_grad():
        a = render_parts(cam, [Part(dyn, d[0], d[1], d[2], rows=~mask),
                               Part(dyn, d[0], d[1], d[2], rows=mask, edit=rigid_edit())], bgc)
        b = render(cam, dyn, SynthPipe(), bgc, d[0], d[1], d[2], norm_gaussian_features=False)
    assert int((a["radii"] > 0).sum()) > 100 and a["radii"].numel() == N_DYN
    for k in ("render", "render_gaussian_features", "depth"):
        _close(k, a[k], b[k])


def test_the_fused_kernel_runs_under_no_grad_and_gradients_take_the_torch_path(monkeypatch):
    from trase_amd import _lib, edit
    dev = torch.device("cuda", 0)
    bg, dyn, cam, d, mask = _scene(dev, seed=41)
    bgc = torch.zeros(3, device=dev)
    lib = _lib.load()
    real, calls = lib.trase_compose_part, []
    monkeypatch.setattr(lib, "trase_compose_part", lambda *a: calls.append(1) or real(*a))
    args = (cam, bg, dyn, d[0], d[1], d[2], bgc, SCALE, OFFSET, ANGLES, 1.0, mask)
    with torch.no_grad():
        edit.render_composite(*args)
    assert len(calls) == 2                                       # one launch per part
    out = edit.render_composite(*args)                           # the parameters require a gradient: the torch composition
    assert len(calls) == 2
    for p in bg.parameters() + dyn.parameters():
        p.grad = None
    (out["render"].sum() + out["render_gaussian_features"].sum() + out["depth"].sum()).backward()
    for pc in (bg, dyn):
        g = pc._xyz.grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert float(dyn._xyz.grad[~mask].abs().max()) == 0.0       # rows outside the mask take no part
    # parameters that need no gradient: fused also with gradients enabled
    from trase_amd.synthetic import SynthGaussianModel, make_scene
    frozen = SynthGaussianModel(make_scene(500, feat_dim=32, seed=5).to(dev), requires_grad=False)
    edit.render_composite(cam, frozen, frozen, 0.0, 0.0, 0.0, bgc, 1.0, OFFSET, ANGLES)
    assert len(calls) == 4
    edit.render_composite(cam, frozen, frozen, 0.01, 0.0, 0.0, bgc, 1.0, OFFSET, ANGLES)      # a non-zero float deformation
    assert len(calls) == 4


def test_background_mask_moves_the_object_and_nothing_else():
    from trase_amd.edit import Part, render_composite, render_parts, rigid_edit
    dev = torch.device("cuda", 0)
    _, pc, cam, d, _ = _scene(dev, seed=51, n_dyn=N_BG)
    bgc = torch.zeros(3, device=dev)
    centre = torch.tensor([0.6, 0.0, 0.0], device=dev)
    mask = ((pc._xyz.detach() + d[0]) - centre).norm(dim=1) < 0.5
    assert 20 < int(mask.sum()) < 600
    move = (-1.2, 0.1, 0.0)
    zero = (0.0, 0.0, 0.0)
    with torch.no_grad():
        still = render_composite(cam, pc, pc, d[0], d[1], d[2], bgc, 1.0, zero, zero, 1.0, mask, background_mask=~mask)
        moved = render_composite(cam, pc, pc, d[0], d[1], d[2], bgc, 1.0, move, zero, 1.0, mask, background_mask=~mask)
        # the object alone, before and after: where it can contribute to a pixel at all
        alone0 = render_parts(cam, [Part(pc, d[0], d[1], d[2], rows=mask)], bgc)["depth"][0] > 0
        alone1 = render_parts(cam, [Part(pc, d[0], d[1], d[2], rows=mask, edit=rigid_edit(1.0, zero, move))], bgc)["depth"][0] > 0
    # with the same model on both sides every Gaussian appears exactly once: `still` is the whole model in another order
    assert still["radii"].numel() == N_BG == moved["radii"].numel()
    assert int(alone0.sum()) > 50 and int(alone1.sum()) > 50
    assert int((alone0 ^ alone1).sum()) > 50                     # the support moves
    gone = alone0 & ~alone1
    assert float((still["depth"][0] - moved["depth"][0]).abs()[gone].max()) > 1e-3
    untouched = ~(alone0 | alone1)
    assert float(untouched.float().mean()) > 0.2
    for k in ("render", "render_gaussian_features", "depth"):
        err = (still[k] - moved[k]).abs().amax(0)[untouched]
        share, worst = (err > 2e-5).float().mean().item(), err.max().item()
        print(f"{k} in the untouched region: share over 2e-5 = {share:.3e}, max {worst:.3e}")
        assert share < 2e-3 and worst < 5e-2
