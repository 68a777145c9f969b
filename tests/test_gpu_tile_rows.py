"""Tile-row strips (SURVEY.md 8e second axis, BASELINE config 5) on ONE GPU: rendering k strips and summing what they
produce must equal the full render -- maps bit-identical inside each strip and zero outside, per-Gaussian gradients equal
to fp32 reassociation, radii whole-image -- through the operator and through the fused render()."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _scene(n=6000, w=200, h=150, seed=3, scale_mult=0.9):
    from trase_amd.synthetic import SynthGaussianModel, SynthPipe, make_scene, orbit_camera
    dev = torch.device("cuda", 0)
    scene = make_scene(n, feat_dim=32, seed=seed, scale_mult=scale_mult).to(dev)
    cam = orbit_camera(w, h, angle=0.4).to(dev)
    return scene, cam, dev, SynthGaussianModel, SynthPipe


@pytest.mark.parametrize("world,size,sparse", [(2, "small", False), (3, "small", False), (3, "small", True), (4, "S5", False), (4, "S5", True)],
                         ids=["2", "3", "3-sparse-grads", "S5-4-balanced", "S5-4-balanced-sparse-grads"])
def test_strips_reassemble_the_full_render(world, size, sparse):
    """size "S5": BASELINE config 5's shape (2.5 M Gaussians, 1280x960), four LOAD-BALANCED strips (unequal heights).
    sparse: `set_sparse_strip_grads` -- a strip's backward writes only the rows of the Gaussians with a pair in the strip into
    persistent zero-elsewhere tensors; consecutive strips exercise the re-zeroing of the previous strip's rows."""
    from gaussian_renderer import render
    from trase_amd import rasterizer as R
    from trase_amd.dp import strip_pixel_rows, tile_row_partition
    scene, cam, dev, Model, Pipe = _scene() if size == "small" else _scene(n=2_500_000, w=1280, h=960, seed=0, scale_mult=0.27)
    H, W = cam.image_height, cam.image_width
    bg = torch.tensor([0.2, 0.3, 0.1], device=dev)
    g = torch.Generator().manual_seed(0)
    gi, gf = torch.randn(3, H, W, generator=g).to(dev), torch.randn(32, H, W, generator=g).to(dev)

    def run(rows):
        pc = Model(scene)
        with R.tile_rows(*rows):
            out = render(cam, pc, Pipe(), bg, 0.0, 0.0, 0.0)
        torch.autograd.backward([out["render"], out["render_gaussian_features"]], [gi, gf])   # after the context: the ctx carries the strip
        grads = [p.grad.clone() for p in pc.parameters()] + [out["viewspace_points"].grad.clone()]
        return out, grads

    full, g_full = run((0, 0))
    R.set_sparse_strip_grads(sparse)
    try:
        _check_strips(run, full, g_full, world, size, H, R, tile_row_partition, strip_pixel_rows)
    finally:
        R.set_sparse_strip_grads(False)


def _check_strips(run, full, g_full, world, size, H, R, tile_row_partition, strip_pixel_rows):
    part = tile_row_partition(H, world)
    if size == "S5":
        loads = R.last_tile_row_loads()
        assert int(loads.sum()) == R.last_status()[2] and len(loads) == (H + 15) // 16
        part = tile_row_partition(H, world, loads=loads)
        strip_loads = [int(loads[b:e].sum()) for b, e in part]
        assert max(strip_loads) <= 1.25 * (sum(strip_loads) / world), f"unbalanced strips {part}: {strip_loads}"
    acc = [torch.zeros_like(t) for t in g_full]
    for r in range(world):
        o, gs = run(part[r])
        y0, y1 = strip_pixel_rows(part, r, H)
        assert torch.equal(o["radii"], full["radii"])
        for k in ("render", "render_gaussian_features", "depth"):
            assert torch.equal(o[k][:, y0:y1], full[k][:, y0:y1]), f"rank {r}: {k} differs inside its strip"
            assert float(o[k][:, :y0].abs().sum()) == 0 and float(o[k][:, y1:].abs().sum()) == 0, f"rank {r}: {k} written outside its strip"
        for a, t in zip(acc, gs):
            a += t
    for name, a, b in zip(["xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity", "features", "means2D"], acc, g_full):
        scale = float(b.abs().max()) + 1e-12
        assert float((a - b).abs().max()) <= 2e-5 * scale, f"{name}: strips do not add up ({float((a - b).abs().max()):.3e} vs scale {scale:.3e})"


def test_operator_level_strip_and_empty_strip():
    from diff_gaussian_rasterization import GaussianRasterizer
    from trase_amd import rasterizer as R
    from tests.util import settings_for
    scene, cam, dev, _, _ = _scene(n=1500, w=96, h=70)
    act = scene.activated()
    st = settings_for(cam, bg=(0.5, 0.5, 0.5), device=dev)
    kw = dict(means3D=act["means3D"], means2D=torch.zeros_like(act["means3D"]), shs=act["shs"], sh_objs=act["sh_objs"],
              opacities=act["opacities"], scales=act["scales"], rotations=act["rotations"])
    full = GaussianRasterizer(st)(**kw)
    with R.tile_rows(1, 3):                                # tile rows 1, 2 = pixel rows 16..47
        strip = GaussianRasterizer(st)(**kw)
    assert torch.equal(strip[0][:, 16:48], full[0][:, 16:48]) and torch.equal(strip[2][:, 16:48], full[2][:, 16:48])
    assert float(strip[0][:, :16].abs().sum()) == 0 and float(strip[0][:, 48:].abs().sum()) == 0
    with R.tile_rows(5, 5):                                # an empty range (a rank beyond the last tile row)
        none = GaussianRasterizer(st)(**kw)
    assert float(none[0].abs().sum()) == 0 and torch.equal(none[1], full[1])
    assert R._Policy.tile_rows == (0, 0)


@pytest.mark.parametrize("feat,image_only", [(32, False), (32, True), (16, False), (0, True)])
def test_strips_through_the_operator_entry_point(feat, image_only):
    """Tile-row strips through GaussianRasterizer (trase_rast_forward / trase_rast_backward, not the fused render()): the strips'
    outputs reassemble the whole image and their gradients sum to the whole image's.  Round 5: this entry point's backward
    reduced the gradient rows of all P depth ranks although a strip forward sorts only the Gaussians with a pair in the strip
    -- ids read from the unsorted tail, a GPU memory fault; found by the image-only / F = 16 test ADVICE r4 asked for."""
    from tests import test_gpu_parity as T
    from tests.util import settings_for, small_case
    from trase_amd import rasterizer as R
    H, W = 96, 144
    act, cam = small_case(n=900, w=W, h=H, feat=feat, seed=5)
    st = settings_for(cam)
    g = torch.Generator().manual_seed(3)
    gi = torch.randn(3, H, W, generator=g).cuda()
    gf = torch.randn(max(feat, 1), H, W, generator=g).cuda()

    def run(rows):
        with R.tile_rows(*rows):
            out, leaves = T._gpu_call(act, st)
            if image_only or feat == 0:
                torch.autograd.backward([out[0]], [gi])
            else:
                torch.autograd.backward([out[0], out[2]], [gi, gf])
        grads = {k: (v.grad.clone() if v.grad is not None else None) for k, v in leaves.items() if v is not None}
        return [o.detach().clone() for o in (out[0], out[2], out[3])], grads

    full_out, full_g = run((0, 0))
    acc = {k: (torch.zeros_like(v) if v is not None else None) for k, v in full_g.items()}
    for (b, e) in ((0, 2), (2, 3), (3, 6)):
        outs, gs = run((b, e))
        y0, y1 = 16 * b, min(16 * e, H)
        for o, f in zip(outs, full_out):
            if o.numel():
                assert torch.equal(o[..., y0:y1, :], f[..., y0:y1, :]), f"strip {b, e}: pixels differ from the whole image"
        for k, v in gs.items():
            if v is not None:
                acc[k] += v
    for k, v in full_g.items():
        if v is None:
            assert acc[k] is None
            continue
        scale = float(v.abs().max())
        assert float((acc[k] - v).abs().max()) <= 2e-5 * max(scale, 1e-12) + 1e-9, (k, float((acc[k] - v).abs().max()), scale)


def test_bin_layout_offsets_describe_the_real_workspace():
    """40 x 24: 5 x 3 sub-tiles, an odd number of sub-tile rows.  The `ranges` read through trase_rast_bin_layout partition
    the culled pairs [0, R_eff) among the sub-tiles, and last_tile_row_loads (which reads them the same way) counts every pair."""
    import ctypes as C
    from diff_gaussian_rasterization import GaussianRasterizer
    from tests.util import settings_for, small_case
    from trase_amd import _lib
    from trase_amd import rasterizer as R
    dev = torch.device("cuda", 0)
    w, h, T = 40, 24, 15
    act, cam = small_case(n=64, w=w, h=h, feat=0, seed=5)
    a = {k: v.to(dev) for k, v in act.items() if v is not None}
    R.set_sync(True)
    GaussianRasterizer(raster_settings=settings_for(cam, device=dev))(
        means3D=a["means3D"], means2D=torch.zeros(64, 3, device=dev), shs=a["shs"], opacities=a["opacities"], scales=a["scales"],
        rotations=a["rotations"])
    r_eff = R.last_status()[2]
    assert r_eff > 0
    cap, binb = int(R._Policy.last_capacity), R._Policy.last_bin
    off = (C.c_int64 * 3)()
    assert _lib.load().trase_rast_bin_layout(cap, T, C.byref(off)) == 0
    assert off[0] == 0 and off[1] >= 4 * cap and off[2] >= off[1] + 4 * cap and off[2] + 8 * (T + 1) <= binb.numel()
    rng = binb[off[2]:off[2] + 8 * T].view(torch.int32).reshape(T, 2).cpu().tolist()
    assert all(0 <= b <= e <= r_eff for b, e in rng), rng
    edge = 0
    for b, e in sorted(r for r in rng if r[1] > r[0]):          # the non-empty lists follow each other without a gap
        assert b == edge, rng
        edge = e
    assert edge == r_eff, (rng, r_eff)
    loads = R.last_tile_row_loads()
    assert loads.numel() == 2 and int(loads.sum()) == r_eff
