"""The fused per-Gaussian kernels (trase_amd/csrc/preprocess_raw.hip: preprocess_fwd_raw_kernel / preprocess_bwd_raw_kernel)
against float64 (tests/fused_prep_reference.py around oracle/raster_oracle.py) at every launch form: one wave / wave boundary /
ragged last wave and every P mod 4 of the f_rest slab copy, SH degree 0-3 x feature width 32 / 16 / 0, the frustum and colour
clamps and the near cull, an unaligned f_rest pointer, a NaN-poisoned gradient bucket behind the sink (dense and ranged
backward), the 256-thread strip instantiation with the dense and the LIVE sparse backward, the INFER instantiation's call
patterns -- and the operator kernels (preprocess.hip) with SH rows shorter than 16 coefficients.

All scenes: orbit_camera(64, 48, angle=0.4) -- 4 x 3 tiles, 3 tile rows.

Where every bar comes from:
  * maps, radii, per-entry gradients, fragility caps: `_check_maps` / `_check_grads` of tests/test_gpu_parity.py, imported and
    unchanged (maps 1e-4 abs, gradients rtol 1e-3 + 1e-5 max|grad|, at most 1 % / 12 fragile pixels, max(2, 1e-4 P) Gaussians);
  * per-Gaussian forward rows (xy, depth, conic, rgb): the numbers of tests/test_hostsim_math.py::test_forward_matches_oracle
    (same gs_math.h arithmetic); opacity: (|logit| + 4) * 2^-23 relative -- __expf as exp2(x log2 e) (the product's rounding
    grows with |x|), one reciprocal, one addition;
  * exact 0.0: gradient rows of Gaussians without a pair, dL/df_rest beyond the active SH degree, dL/df_dc of a clamped colour
    channel (the lineage's rule), masked-out Gaussians;
  * bit-equality between two runs of the same instantiation: unaligned f_rest, the grad sink, the ranged backward, the strip
    forward's geometry rows;
  * (d) the scene's own preconditions (>= 32 Gaussians of each clamp kind, >= 24 culled) are asserted on the float64 side; a
    pre-clamp colour within 1e-5 of 0 (the rgb bar's atol) may decide either way, at most 2 rows."""
import functools
import math
import types

import pytest
import torch

from oracle import raster_oracle as ro
from tests import fused_prep_reference as FR
from tests.test_gpu_parity import _check_grads, _check_maps, _masked, device_view_of_last_forward   # (_check_maps applies depth_atol)

pytestmark = pytest.mark.gpu

W, H = 64, 48
BG = (0.1, 0.25, 0.4)
BASE = ["xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity", "gaussian_features", "means2D"]
DEFORM = ["d_xyz", "d_rotation", "d_scaling"]
ATTR = {"xyz": "_xyz", "features_dc": "_features_dc", "features_rest": "_features_rest", "scaling": "_scaling",
        "rotation": "_rotation", "opacity": "_opacity", "gaussian_features": "_gaussian_features"}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


def _cam():
    from trase_amd.synthetic import orbit_camera
    return orbit_camera(W, H, angle=0.4)


def _scene(P, F=32, seed=None):
    from trase_amd.synthetic import make_scene
    return make_scene(P, feat_dim=F or 32, seed=30 + P if seed is None else seed, scale_mult=0.9)


def _deformation(P, seed, amp=(0.01, 0.05, 0.001)):
    """(d_xyz, d_rotation, d_scaling) as tests/test_gpu_parity.py::test_fused_render_matches_unfused_composition draws them"""
    g = torch.Generator().manual_seed(seed)
    return [a * torch.randn(P, c, generator=g) for a, c in zip(amp, (3, 4, 3))]


def _cotangents(F, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3, H, W, generator=g), torch.randn(F, H, W, generator=g)


def _pattern_inputs(P, seed):
    """the extra inputs of render()'s call patterns, drawn as tests/test_gpu_render_patterns.py::_setup draws them"""
    g = torch.Generator().manual_seed(seed)
    d = [0.02 * torch.randn(P, c, generator=g) for c in (3, 4, 3)]
    T = torch.eye(4).repeat(P, 1, 1) + 0.03 * torch.randn(P, 4, 4, generator=g)
    T[:, 3, :3] *= 0.1
    oc = torch.rand(P, 3, generator=g)
    mask = torch.rand(P, generator=g) < 0.6
    return d, T, oc, mask


def _case(scene, deg=3, F=32, deform=None, pattern="plain", extra=None, rows=None, sparse=False, scaling_modifier=1.0,
          norm_gaussian_features=True, poison_inactive_sh=False, seed=0):
    """One fused render() forward + backward and its float64 reference.

    deform: None or [d_xyz, d_rotation, d_scaling] (CPU); pattern: "plain" or one of render()'s call patterns with `extra` =
    (T44, override_color, mask); rows: None or a tile-row strip (b, e) -- the device view then comes from a whole-image forward of
    the same inputs, run first; F = 0: set_forward_scope("image").
    -> namespace(out, o, gl, ol, names, radii, gv, gv_full, pc)"""
    from gaussian_renderer import render
    from trase_amd import rasterizer as R
    from trase_amd import renderer
    from trase_amd.synthetic import SynthGaussianModel, SynthPipe
    dev = _dev()
    cam = _cam()
    P = scene.xyz.shape[0]
    pc = SynthGaussianModel(scene.to(dev), sh_degree=deg)
    if poison_inactive_sh and deg < 3:
        # coefficients beyond the active degree are never read (the lineage indexes sh[0 .. (deg + 1)^2) only): whatever they hold
        # must not reach any output -- 0 * NaN would
        with torch.no_grad():
            pc._features_rest[:, (deg + 1) ** 2 - 1:, :] = float("nan")
    pipe = SynthPipe()
    pipe.convert_SHs_python = pattern == "shs_python"
    pipe.compute_cov3D_python = pattern == "cov_python"
    kw, ref_kw = {}, {}
    dleaves = {}
    d = [0.0, 0.0, 0.0] if deform is None else [t.to(dev).clone().requires_grad_(True) for t in deform]
    d_ref = [0.0, 0.0, 0.0] if deform is None else list(deform)
    if deform is not None:
        dleaves.update(zip(DEFORM, d))
    mask = None
    if pattern != "plain":
        T44, oc, mask_cpu = extra
        if "override" in pattern:
            dleaves["override_color"] = oc.to(dev).clone().requires_grad_(True)
            kw["override_color"], ref_kw["override_color"] = dleaves["override_color"], oc
        if "mask" in pattern:
            mask = mask_cpu
            kw["mask"], ref_kw["mask"] = mask.to(dev), mask
        if pattern == "sixdof":
            dleaves["d_xyz"] = T44.to(dev).clone().requires_grad_(True)
            d[0], d_ref[0] = dleaves["d_xyz"], T44
            kw["is_6dof"] = ref_kw["is_6dof"] = True
    if scaling_modifier != 1.0:
        kw["scaling_modifier"] = ref_kw["scaling_modifier"] = scaling_modifier
    if not norm_gaussian_features:
        kw["norm_gaussian_features"] = ref_kw["norm_gaussian_features"] = False
    bg = torch.tensor(BG, device=dev)

    def forward():
        out = render(cam.to(dev), pc, pipe, bg, d[0], d[1], d[2], **kw)
        gv = {k: v.cpu().clone() for k, v in R.last_geom_view(P).items()}
        radii = out["radii"].detach().cpu()
        if mask is not None:                                   # render() returns the subset's radii (as the reference does)
            assert radii.shape[0] == int(mask.sum())
            full = torch.zeros(P, dtype=radii.dtype)
            full[mask] = radii
            radii = full
        return out, gv, radii

    if F == 0:
        renderer.set_forward_scope("image")
    R.set_sparse_strip_grads(bool(sparse))
    try:
        gv_full = None
        if rows is None:
            out, gv, radii = forward()
            dv = device_view_of_last_forward(radii)
        else:
            out, gv_full, radii_full = forward()
            dv = device_view_of_last_forward(radii_full)
            with R.tile_rows(*rows):
                out, gv, radii = forward()
            assert torch.equal(radii, radii_full), "a strip's radii are the whole image's"
        tiles = None if rows is None else [(tx, ty) for ty in range(rows[0], rows[1]) for tx in range((W + 15) // 16)]
        o, ol = FR.fused_prep_reference(FR.raw_of(scene), cam, BG, d_ref[0], d_ref[1], d_ref[2], sh_degree=deg,
                                        convert_SHs_python=pipe.convert_SHs_python, compute_cov3D_python=pipe.compute_cov3D_python,
                                        with_features=F > 0, device_view=dv, tiles=tiles, **ref_kw)
        gi, gf = _cotangents(F, seed + 1000)
        gi, gf = _masked(gi, o), _masked(gf, o)
        (o.image * gi.double()).sum().add((o.feats * gf.double()).sum()).backward()
        if F > 0:
            torch.autograd.backward([out["render"], out["render_gaussian_features"]], [gi.to(dev), gf.to(dev)])
        else:
            assert tuple(out["render_gaussian_features"].shape) == (0, H, W)
            out["render"].backward(gi.to(dev))
        torch.cuda.synchronize()
    finally:
        R.set_sparse_strip_grads(False)
        if F == 0:
            renderer.set_forward_scope("all")
    gl = {k: getattr(pc, a) for k, a in ATTR.items()}
    gl["means2D"] = out["viewspace_points"]
    gl.update(dleaves)
    names = [k for k in BASE if not (k == "gaussian_features" and F == 0)]
    if "override" in pattern:
        names = [k for k in names if not k.startswith("features_")] + ["override_color"]
    names += [k for k in DEFORM if k in dleaves and not (pattern == "cov_python" and k != "d_xyz")]
    maps = (out["render"], out["radii"], out["render_gaussian_features"], out["depth"])
    return types.SimpleNamespace(out=out, maps=maps, o=o, gl=gl, ol=ol, names=names, radii=radii, gv=gv, gv_full=gv_full, pc=pc,
                                 mask=mask, P=P)


def _check(c, zero_rows=True):
    """the criteria of (a): maps and radii, per-entry gradients, exact zeros where a Gaussian has no pair"""
    n_frag, n_reg = _check_maps(c.maps, c.o)
    print(f"P={c.P}: {n_frag} fragile pixels of {n_reg}, {int(c.o.frag_gauss.sum())} fragile Gaussians, "
          f"{int((c.radii > 0).sum())} visible")
    _check_grads(c.gl, c.ol, c.o.full, c.names)
    assert tuple(c.gl["means2D"].grad.shape) == (c.P, 3)
    if zero_rows:
        dead = c.radii == 0
        for k in c.names:
            g = c.gl[k].grad.detach().cpu()
            assert int(torch.count_nonzero(g[dead])) == 0, f"{k}: a Gaussian with radii == 0 has a non-zero (or NaN) gradient row"
            assert bool(torch.isfinite(g).all()), f"{k}: non-finite gradient"


# ---- (a) row counts, (c) per-Gaussian forward rows ----------------------------------------------------------------------------
ROW_COUNTS = [1, 2, 3, 63, 64, 65, 66, 67, 128, 193, 257]


@functools.lru_cache(maxsize=None)
def _row_count_case(P):
    deform = _deformation(P, seed=P) if ROW_COUNTS.index(P) % 2 else None      # plain and deformed scenes alternate
    return _case(_scene(P), deform=deform, seed=P)


@pytest.mark.parametrize("P", ROW_COUNTS)
def test_row_counts_match_float64(P):
    """Every P mod 4 (where the 16-byte tail of the slab copy ends: nfl = rows * 45), one wave, a wave boundary +- 1, several waves
    with a ragged last one."""
    _check(_row_count_case(P))


@pytest.mark.parametrize("P", ROW_COUNTS)
def test_forward_rows_match_float64_preprocess(P):
    c = _row_count_case(P)
    g = c.o.geom                                                 # ro.preprocess on the float64 activations
    ok = ~c.o.frag_gauss
    assert torch.equal(c.radii[ok], c.o.radii[ok])
    both = g.valid & (c.radii > 0) & ok
    assert int(g.valid.sum()) >= 1 and int(both.sum()) >= 0.5 * int(g.valid.sum())

    def close(a, b, rtol, atol, what):
        a, b = a[both].double(), b.detach()[both]
        bad = (a - b).abs() > atol + rtol * b.abs()
        assert not bool(bad.any()), f"{what}: worst {((a - b).abs() - atol - rtol * b.abs()).max().item():.3e} over the bar"

    close(c.gv["xy"], g.xy, 1e-5, 2e-3, "xy")
    close(c.gv["rgb_depth"][:, 3], g.depth, 1e-5, 0.0, "depth")
    close(c.gv["conic_opacity"][:, :3], g.conic, 2e-4, 1e-6, "conic")
    close(c.gv["rgb_depth"][:, :3], g.rgb, 1e-4, 1e-5, "rgb")
    logit = c.ol["opacity"].detach().reshape(-1)
    sig = torch.sigmoid(logit)
    rel = ((c.gv["conic_opacity"][:, 3].double() - sig).abs() / sig)[both]
    bar = ((logit.abs() + 4.0) * 2.0 ** -23)[both]
    print(f"P={P}: opacity worst {float((rel / bar).max()):.3f} of its bar")
    assert bool((rel <= bar).all()), f"opacity: {float((rel / bar).max()):.3f} x the bar"


# ---- (b) SH degree x feature width ----------------------------------------------------------------------------------------------
def _degree_case(deg, F, P, **kw):
    c = _case(_scene(P, F=F), deg=deg, F=F, deform=_deformation(P, seed=7 * P + deg) if (deg + F // 16) % 2 else None,
              poison_inactive_sh=True, seed=100 * deg + F + P, **kw)
    _check(c)
    g_rest = c.gl["features_rest"].grad.detach().cpu()
    n = (deg + 1) ** 2 - 1                                        # active f_rest coefficients
    assert int(torch.count_nonzero(g_rest[:, n:, :])) == 0, "dL/df_rest beyond the active degree is not exactly zero"
    if deg > 0:
        assert float(g_rest[:, :n, :].abs().max()) > 0
    return c


@pytest.mark.parametrize("P", [65, 193])
@pytest.mark.parametrize("F", [32, 16, 0])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_degree_and_feature_width(deg, F, P):
    """Training spends its first 3000 iterations below degree 3 (the SH ramp): the `k < n3` masking of the slab rows and the zero
    tail of dL/df_rest.  The device's f_rest holds NaN beyond the active degree: those coefficients are never read."""
    _degree_case(deg, F, P)


def test_scaling_modifier_case():
    _degree_case(2, 32, 193, scaling_modifier=0.7)


def test_unnormalised_features_case():
    _degree_case(1, 16, 65, norm_gaussian_features=False)


# ---- (d) clamp and cull edges --------------------------------------------------------------------------------------------------
def _clamp_scene():
    from trase_amd.synthetic import make_scene, rgb2sh
    sc = make_scene(256, feat_dim=32, seed=21, extent=2.5, scale_mult=0.8, opacity_mode="init")
    g = torch.Generator().manual_seed(1)
    sc.features_dc[:96] = rgb2sh(torch.rand(96, 1, 3, generator=g) * 0.6 - 0.3)          # colours around 0: clamped channels
    centre = _cam().camera_center
    sc.xyz[224:] = centre * torch.linspace(0.9, 1.3, 32)[:, None] + 0.02 * sc.xyz[224:]  # on and behind the near plane
    return sc


def clamp_census(c, cam, sh_dir_undeformed=False):
    """float64 side: which Gaussians the near plane culls, whose tx/tz (ty/tz) is clamped at 1.3 tan with a non-zero position
    gradient, and which colour channels clamp_min(., 0) clamps on a row that receives gradient; `pre` = the pre-clamp colours
    (pipe.convert_SHs_python: in the direction of the undeformed xyz)"""
    with torch.no_grad():
        L = {k: v.detach() for k, v in c.ol.items()}
        a = FR.prep_args(L, cam.camera_center, sh_degree=3)
        vm = cam.world_view_transform.double()
        t = a["means3D"] @ vm[:3, :3] + vm[3, :3]
        culled = t[:, 2] <= 0.2
        valid = c.o.geom.valid
        tz = torch.where(culled, torch.ones_like(t[:, 2]), t[:, 2])
        cx = (t[:, 0] / tz).abs() > 1.3 * math.tan(cam.FoVx * 0.5)
        cy = (t[:, 1] / tz).abs() > 1.3 * math.tan(cam.FoVy * 0.5)
        moved = (c.ol["xyz"].grad != 0).any(dim=1)
        dirs = (L["xyz"] if sh_dir_undeformed else a["means3D"]) - cam.camera_center.double()[None]
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        pre = ro.eval_sh_colors(3, a["shs"], dirs) + 0.5
        lit = c.ol["opacity"].grad.reshape(-1) != 0
    return types.SimpleNamespace(culled=culled, x=cx & valid & moved, y=cy & valid & moved, colour=(pre < 0) & (valid & lit)[:, None],
                                 pre=pre)


@pytest.mark.parametrize("variant", ["plain", "deformed", "shs_python"])
def test_clamp_and_cull_edges(variant):
    """The frozen tx/tz clamp at 1.3 tan with its zeroed gradient, clamp_min(colour, 0) with the zero gradient it implies, and the
    near cull -- rare or absent in the random cube scenes, the rule here.  "shs_python": the deformed scene with
    pipe.convert_SHs_python, whose colour backward (sh_backward_at) applies the clamp bits on its own."""
    c = _case(_clamp_scene(), deform=None if variant == "plain" else _deformation(256, seed=3),
              pattern="shs_python" if variant == "shs_python" else "plain", extra=(None, None, None), seed=21)
    n = clamp_census(c, _cam(), sh_dir_undeformed=variant == "shs_python")
    counts = {"culled": int(n.culled.sum()), "x": int(n.x.sum()), "y": int(n.y.sum()), "colour rows": int(n.colour.any(dim=1).sum())}
    print(counts)
    assert counts["culled"] >= 24 and counts["x"] >= 32 and counts["y"] >= 32 and counts["colour rows"] >= 32, counts
    _check(c)
    near0 = (n.pre.abs() < 1e-5).any(dim=1)
    assert int(near0.sum()) <= 2
    g_dc = c.gl["features_dc"].grad.detach().cpu().reshape(-1, 3)
    sure = n.colour & ~near0[:, None]
    assert int(torch.count_nonzero(g_dc[sure])) == 0, "dL/df_dc of a clamped colour channel is not exactly zero"


# ---- (e) unaligned f_rest ------------------------------------------------------------------------------------------------------
def _plain_backward(pc, gi, gf, deform=None):
    from gaussian_renderer import render
    from trase_amd.synthetic import SynthPipe
    dev = _dev()
    d = [0.0, 0.0, 0.0] if deform is None else [t.to(dev).clone().requires_grad_(True) for t in deform]
    out = render(_cam().to(dev), pc, SynthPipe(), torch.tensor(BG, device=dev), *d)
    torch.autograd.backward([out["render"], out["render_gaussian_features"]], [gi.to(dev), gf.to(dev)])
    torch.cuda.synchronize()
    maps = [out[k].detach().cpu().clone() for k in ("render", "render_gaussian_features", "depth", "radii")]
    grads = [p.grad.detach().cpu().clone() for p in pc.parameters()] + [out["viewspace_points"].grad.detach().cpu().clone()] + \
            [t.grad.detach().cpu().clone() for t in d if torch.is_tensor(t)]
    return maps, grads


@pytest.mark.parametrize("P", [65, 193])
def test_unaligned_f_rest_is_bit_identical(P):
    """`_features_rest` 1, 2 and 3 floats into a larger buffer: the scalar branch of the slab load instead of the 16-byte one.  Same
    instantiation, same values in the slab: maps, radii and every gradient bit-identical."""
    from trase_amd.synthetic import SynthGaussianModel
    dev = _dev()
    scene = _scene(P).to(dev)
    gi, gf = _cotangents(32, P)
    deform = _deformation(P, seed=P + 1)
    ref_maps, ref_grads = _plain_backward(SynthGaussianModel(scene), gi, gf, deform)
    assert float(ref_grads[2].abs().max()) > 0
    for off in (1, 2, 3):
        pc = SynthGaussianModel(scene)
        buf = torch.zeros(P * 45 + 8, device=dev)
        view = buf[off:off + P * 45].view(P, 15, 3)
        view.copy_(scene.features_rest)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off and pc._features_rest.data_ptr() % 16 == 0
        pc._features_rest = view.requires_grad_(True)
        maps, grads = _plain_backward(pc, gi, gf, deform)
        for a, b in zip(maps + grads, ref_maps + ref_grads):
            assert torch.equal(a, b), f"offset {off}: differs from the aligned call"
        assert float(buf[:off].abs().max()) == 0 and float(buf[off + P * 45:].abs().max()) == 0


# ---- (f) gradient sink into a poisoned bucket -----------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3, 65, 193])
def test_grad_sink_into_a_poisoned_bucket(P):
    """The bucket's slices fall at every 4-byte offset (the f_rest slice never at a 16-byte one here: the scalar branch of the slab
    store).  Everything the bucket holds is NaN before the backward: every payload entry must have been written, with the bits of
    the backward without a sink; the words behind the payload must not have been."""
    from trase_amd.dp import FlatGradBucket
    from trase_amd.renderer import chunk_ranges, set_grad_sink
    from trase_amd.synthetic import SynthGaussianModel
    dev = _dev()
    scene = _scene(P).to(dev)
    gi, gf = _cotangents(32, P + 5)
    _, ref = _plain_backward(SynthGaussianModel(scene), gi, gf)
    for chunks in (1, 2, 3):
        pc = SynthGaussianModel(scene)
        params = pc.parameters()
        bucket = FlatGradBucket(params)
        assert any(v.data_ptr() % 16 for v in bucket._views)
        calls = []
        kw = bucket.overlapped(chunks) if chunks > 1 else dict(sink=bucket.sink())
        if chunks > 1:
            hook = kw["on_chunk"]
            kw["on_chunk"] = lambda a, b, n, ids: (calls.append((a, b)), hook(a, b, n, ids))
        try:
            set_grad_sink(**kw)
            bucket.detach_grads()
            bucket._store.fill_(float("nan"))
            _, got = _plain_backward(pc, gi, gf)
            if chunks > 1:
                bucket.allreduce()
                torch.cuda.synchronize()
        finally:
            set_grad_sink(None)
        if chunks > 1:
            assert calls == [tuple(r) for r in chunk_ranges(P, chunks)]
        assert bucket.adopted(), "a gradient did not land in the bucket"
        assert bool(torch.isfinite(bucket.flat).all()), f"chunks={chunks}: a payload entry of the bucket was never written"
        assert bool(torch.isnan(bucket._store[bucket.numel:]).all()), f"chunks={chunks}: written behind the payload"
        for p, g, r in zip(params, got, ref):
            assert torch.equal(p.grad.detach().cpu(), r) and torch.equal(g, r), f"chunks={chunks}: differs from the backward without a sink"
        assert torch.equal(got[-1], ref[-1])                     # means2D (never a bucket parameter)


# ---- (g) strips ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse-grads"])
@pytest.mark.parametrize("rows", [(0, 1), (1, 3), (2, 3)])
@pytest.mark.parametrize("P", [65, 193, 257])
def test_strips_match_float64(P, rows, sparse):
    """The 256-thread strip instantiation (no slab; P = 65: two of the four waves leave early) with the dense and the LIVE sparse
    backward: the strip's rows of the maps, and the gradients of a cotangent that is zero outside the strip."""
    c = _case(_scene(P), deform=_deformation(P, seed=P) if P == 193 else None, rows=rows, sparse=sparse, seed=P + 10 * rows[0] + rows[1])
    live = (c.gv["tiles"] > 0) & (c.radii > 0)
    # the contract stated in the kernel: a strip reproduces the full render's geometry bit for bit
    assert torch.equal(c.gv["xy"][live], c.gv_full["xy"][live]), "strip forward: xy differs from the whole-image forward"
    assert torch.equal(c.gv["conic_opacity"][live], c.gv_full["conic_opacity"][live]), "strip forward: conic / opacity differ"
    y0, y1 = 16 * rows[0], min(16 * rows[1], H)
    for k in ("render", "render_gaussian_features", "depth"):
        m = c.out[k].detach()
        assert float(m[:, :y0].abs().sum()) == 0 and float(m[:, y1:].abs().sum()) == 0, f"{k} written outside the strip"
    assert bool(c.o.tile_mask[y0:y1].all()) and int(c.o.tile_mask.sum()) == (y1 - y0) * W
    _check(c)
    nolive = ~live
    for k in c.names:                                            # no pair in the strip: exact zero rows
        assert int(torch.count_nonzero(c.gl[k].grad.detach().cpu()[nolive])) == 0, k


# ---- (h) call patterns (INFER instantiation) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [65, 193])
@pytest.mark.parametrize("pattern", ["override", "mask", "sixdof", "shs_python", "cov_python", "mask_override"])
def test_call_patterns_match_float64(pattern, P):
    d, T44, oc, mask = _pattern_inputs(P, seed=P + 6)
    c = _case(_scene(P), deform=d, pattern=pattern, extra=(T44, oc, mask), seed=P + len(pattern))
    _check(c)
    if "override" in pattern:
        assert "override_color" in c.names and float(c.gl["override_color"].grad.abs().max()) > 0
        assert c.pc._features_dc.grad is None or float(c.pc._features_dc.grad.abs().max()) == 0
    if pattern == "sixdof":
        assert "d_xyz" in c.names and tuple(c.gl["d_xyz"].grad.shape) == (P, 4, 4) and float(c.gl["d_xyz"].grad.abs().max()) > 0
    if "mask" in pattern:
        assert c.out["radii"].shape[0] == int(mask.sum()) < P
        assert tuple(c.gl["means2D"].grad.shape) == (P, 3) and float(c.gl["means2D"].grad.abs().max()) > 0
        for k in c.names:                                        # a removed Gaussian: exact zero rows, at full size
            assert int(torch.count_nonzero(c.gl[k].grad.detach().cpu()[~mask])) == 0, k


# ---- (i) operator kernels with short SH rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [255, 257])
@pytest.mark.parametrize("M,deg", [(1, 0), (4, 1), (9, 2), (9, 1)])
def test_operator_kernels_with_short_sh_rows(M, deg, P):
    """preprocess_fwd_kernel / preprocess_bwd_kernel with M != 16: the scalar SH load and store path.  M = 9 at degree 1: the rows
    4..8 are never read (NaN on the device) and their gradient is exactly zero."""
    from tests import test_gpu_parity as TP
    from tests.util import settings_for, small_case
    act, cam = small_case(n=P, w=W, h=H, feat=32, seed=40 + P + M)
    act["shs"] = act["shs"][:, :M].contiguous()
    st = settings_for(cam, sh_degree=deg, bg=BG)
    act_dev = dict(act)
    n_active = (deg + 1) ** 2
    if n_active < M:
        act_dev["shs"] = act["shs"].clone()
        act_dev["shs"][:, n_active:] = float("nan")
    g, gl = TP._gpu_call(act_dev, st)
    o, ol = TP._oracle_call(act, st, gpu=g)
    _check_maps(g, o)
    gi, gf = _cotangents(32, P + M)
    gi, gf = _masked(gi, o), _masked(gf, o)
    (o.image * gi.double()).sum().add((o.feats * gf.double()).sum()).backward()
    torch.autograd.backward([g[0], g[2]], [gi.cuda(), gf.cuda()])
    if n_active < M:
        tail = gl["shs"].grad.detach().cpu()[:, n_active:]
        assert int(torch.count_nonzero(tail)) == 0, "gradient rows beyond the active degree are not exactly zero"
    assert tuple(gl["shs"].grad.shape) == (P, M, 3)
    _check_grads(gl, ol, o, ["means3D", "means2D", "opacities", "scales", "rotations", "shs", "sh_objs"])
