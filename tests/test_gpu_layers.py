"""render_layers on the GPU: the pack and finish launches against the numpy restatement (tests/layers_reference.py), and the
call itself against this repository's own ``render()`` -- the image, depth and radii of ``render()`` and, for every table,
``render(override_color=table)["render"]`` -- with ``torch.equal``: there is no tolerance anywhere in this file.

Scenes are trase_amd.synthetic's (1000 Gaussians; one of 20 000 at 640 x 360).  The comparator renders of a (size, background,
variant) are made once, for all ten tables, and only read afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import layers_reference as lr

pytestmark = pytest.mark.gpu

N = 1000
SIZES = [(96, 64), (67, 35), (9, 9), (8, 8)]                                     # (W, H)
BGS = {"black": (0.0, 0.0, 0.0), "white": (1.0, 1.0, 1.0), "mixed": (0.2, 0.5, 0.7)}
VARIANTS = ["plain", "mask", "sixdof", "zero", "scale", "shs_python"]
CANARY = 0xCD


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _u32(t):
    return t.contiguous().view(torch.int32)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(_u32(a), _u32(b))


# ---- pack --------------------------------------------------------------------------------------------------------------------
def _pack_tables(P, L, dev, seed):
    """L tables; the even ones are views one float off their storage base, the odd ones own their storage."""
    g = torch.Generator().manual_seed(seed)
    tabs = []
    for l in range(L):
        if l % 2 == 0:
            tabs.append(torch.randn(3 * P + 1, generator=g).to(dev)[1:].view(P, 3))
        else:
            tabs.append(torch.randn(P, 3, generator=g).to(dev))
    return tabs


@pytest.mark.parametrize("L", [1, 2, 3, 10])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_pack_rows_padding_canary_and_reproducibility(dev, P, L):
    from trase_amd.layers import pack_tables
    tabs = _pack_tables(P, L, dev, seed=1000 * L + P)
    assert tabs[0].storage_offset() == 1 and tabs[0].data_ptr() % 16 == 4
    want = lr.pack([t.cpu().numpy() for t in tabs])
    runs = []
    for _ in range(2):
        buf = torch.full(((P + 3) * 32 * 4,), CANARY, dtype=torch.uint8, device=dev)
        out = buf[:P * 128].view(torch.float32).view(P, 32)
        assert pack_tables(tabs, out=out) is out
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))          # rows equal numpy's; -0.0 would show
        assert not got[:, 3 * L:].view(np.uint32).any()                           # padding: exactly +0.0
        assert bool((buf[P * 128:] == CANARY).all())                              # nothing at or past row P
        runs.append(got)
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))


def test_pack_takes_a_column_slice_of_a_wider_tensor(dev):
    from trase_amd.layers import pack_tables
    P = 300
    g = torch.Generator().manual_seed(3)
    wide = torch.randn(P, 7, generator=g).to(dev)
    tall = torch.randn(2 * P, 3, generator=g).to(dev)
    tabs = [wide[:, 2:5], tall[::2], wide[:, 4:7]]
    assert not any(t.is_contiguous() for t in tabs)
    keep = [t.clone() for t in tabs]
    out = pack_tables(tabs)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), lr.pack([t.cpu().numpy() for t in tabs]).view(np.uint32))
    assert all(torch.equal(a, b) for a, b in zip(tabs, keep))


# ---- finish, called directly on random planes --------------------------------------------------------------------------------------
def _img_workspace(W, H, T, dev):
    from trase_amd import _lib
    sz = _lib.RastSizes()
    assert _lib.load().trase_rast_sizes(1, W, H, 32, 1, C.byref(sz)) == 0
    img = torch.full((sz.img_bytes,), CANARY, dtype=torch.uint8, device=dev)
    img[:4 * W * H].view(torch.float32).copy_(T.reshape(-1))                      # the workspace begins with final_T
    return img


@pytest.mark.parametrize("L", [1, 10])
@pytest.mark.parametrize("bgv", [0.0, 1.0])
@pytest.mark.parametrize("W,H", [(1, 1), (5, 7), (9, 9), (67, 35), (96, 64), (64, 31), (6, 6)])
def test_finish_on_random_planes(dev, W, H, bgv, L):
    """(6, 6) is beyond the issue's list: W * H is a multiple of 4 and W is not, so rows begin off a 4-pixel boundary inside
    a frame that takes the wide accesses elsewhere."""
    from trase_amd import _lib
    from trase_amd.rasterizer import _stream
    hw, G = W * H, 64
    g = torch.Generator().manual_seed(W * 131 + H)
    planes0 = torch.rand(32, H, W, generator=g) * 1.6 - 0.3
    image0 = torch.rand(3, H, W, generator=g) * 1.6 - 0.3
    T0 = torch.rand(H, W, generator=g)
    T0.view(-1)[::5] = 0.0
    T0.view(-1)[1::7] = 1.0
    fbuf = torch.full(((2 * G + 35 * hw) * 4,), CANARY, dtype=torch.uint8, device=dev).view(torch.float32)
    planes = fbuf[G:G + 32 * hw].view(32, H, W)
    image = fbuf[G + 32 * hw:G + 35 * hw].view(3, H, W)
    planes.copy_(planes0)
    image.copy_(image0)
    bbuf = torch.full((2 * G + (1 + L) * 3 * hw,), CANARY, dtype=torch.uint8, device=dev)
    u8 = bbuf[G:G + (1 + L) * 3 * hw].view(1 + L, H, W, 3)
    img_ws = _img_workspace(W, H, T0.to(dev), dev)
    bg = torch.full((3,), bgv, device=dev)
    ws = _lib.RastWorkspace()
    ws.img, ws.img_bytes = img_ws.data_ptr(), img_ws.numel()
    rc = _lib.load().trase_layers_finish(planes.data_ptr(), C.byref(ws), bg.data_ptr(), L, W, H, image.data_ptr(), u8[0].data_ptr(),
                                         u8[1:].data_ptr(), 0, _stream(dev))
    assert rc == 0, _lib.last_error()
    want = lr.finish(planes0.numpy(), T0.numpy(), (bgv,) * 3, L)
    got = planes.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[3 * L:].view(np.uint32), planes0.numpy()[3 * L:].view(np.uint32))          # planes >= 3L untouched
    assert torch.equal(image.cpu(), image0) and torch.equal(img_ws[:4 * hw].view(torch.float32).cpu(), T0.reshape(-1))
    raw = fbuf.view(torch.uint8)
    assert bool((raw[:4 * G] == CANARY).all()) and bool((raw[4 * (G + 35 * hw):] == CANARY).all())
    assert bool((img_ws[4 * hw:] == CANARY).all())
    assert bool((bbuf[:G] == CANARY).all()) and bool((bbuf[G + (1 + L) * 3 * hw:] == CANARY).all())
    frames = u8.cpu().numpy()
    assert np.array_equal(frames[0], lr.frames_u8(image0.numpy()))
    for l in range(L):
        assert np.array_equal(frames[1 + l], lr.frames_u8(got[3 * l:3 * l + 3])), l


def test_finish_without_a_workspace_writes_the_frames_only(dev):
    from trase_amd.layers import finish_planes
    g = torch.Generator().manual_seed(8)
    planes = (torch.rand(6, 35, 67, generator=g) * 1.6 - 0.3).to(dev)
    image = (torch.rand(3, 35, 67, generator=g) * 1.6 - 0.3).to(dev)
    keep = planes.clone()
    u8 = finish_planes(planes, None, None, 2, image=image, frames_u8=True)
    assert torch.equal(planes, keep)
    assert np.array_equal(u8[0].cpu().numpy(), lr.frames_u8(image.cpu().numpy()))
    assert np.array_equal(u8[2].cpu().numpy(), lr.frames_u8(keep[3:6].cpu().numpy()))


# ---- the call itself ---------------------------------------------------------------------------------------------------------------
class _Scene:
    def __init__(self, n, dev, seed=5, requires_grad=False):
        from trase_amd.synthetic import SynthGaussianModel, make_scene
        self.n = n
        self.pc = SynthGaussianModel(make_scene(n, feat_dim=32, seed=seed, scale_mult=0.8).to(dev), requires_grad=requires_grad)
        g = torch.Generator().manual_seed(seed + 1)
        self.d = [(0.02 * torch.randn(n, c, generator=g)).to(dev) for c in (3, 4, 3)]
        T = torch.eye(4).repeat(n, 1, 1) + 0.03 * torch.randn(n, 4, 4, generator=g)
        T[:, 3, :3] *= 0.1
        self.T = T.to(dev)
        self.mask = (torch.rand(n, generator=g) < 0.6).to(dev)
        # ten tables: colours in [0, 1], and some beyond on either side (no clamp anywhere on the way)
        self.tables = [(torch.rand(n, 3, generator=g) * (1.0 if l % 3 else 1.5) - (0.0 if l % 3 else 0.25)).to(dev) for l in range(10)]

    def args(self, variant):
        """-> (d_xyz, d_rotation, d_scaling), kwargs of render() / render_layers(), the pipe"""
        from trase_amd.synthetic import SynthPipe
        pipe = SynthPipe()
        d, kw = tuple(self.d), {}
        if variant == "mask":
            kw["mask"] = self.mask
        elif variant == "sixdof":
            d, kw["is_6dof"] = (self.T, self.d[1], self.d[2]), True
        elif variant == "zero":
            d = (0.0, 0.0, 0.0)
        elif variant == "scale":
            kw["scaling_modifier"] = 0.7
        elif variant == "shs_python":
            pipe.convert_SHs_python = True
        return d, kw, pipe


@pytest.fixture(scope="module")
def scene(dev):
    return _Scene(N, dev)


def _camera(W, H, dev):
    from trase_amd.synthetic import orbit_camera
    return orbit_camera(W, H, angle=0.7, fid=0.4).to(dev)


_REF: dict = {}


def _reference(sc, W, H, bgname, variant, dev):
    """render() and the ten render(override_color=) images of one (scene, size, background, variant): made once."""
    from trase_amd.renderer import render
    key = (id(sc), W, H, bgname, variant)
    if key not in _REF:
        d, kw, pipe = sc.args(variant)
        bg = torch.tensor(BGS[bgname], device=dev)
        cam = _camera(W, H, dev)
        with torch.no_grad():
            base = render(cam, sc.pc, pipe, bg, *d, **kw)
            layers = [render(cam, sc.pc, pipe, bg, *d, override_color=t, **kw)["render"].clone() for t in sc.tables]
        _REF[key] = dict(render=base["render"].clone(), depth=base["depth"].clone(), radii=base["radii"].clone(),
                         visibility_filter=base["visibility_filter"].clone(), layers=layers)
    return _REF[key]


def _layers(sc, W, H, bgname, variant, L, dev, **extra):
    from trase_amd.layers import render_layers
    d, kw, pipe = sc.args(variant)
    return render_layers(_camera(W, H, dev), sc.pc, pipe, torch.tensor(BGS[bgname], device=dev), *d, colors=sc.tables[:L], **kw, **extra)


def _count_renders(monkeypatch):
    from trase_amd import renderer
    calls, real = [], renderer.render
    monkeypatch.setattr(renderer, "render", lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


def _assert_same(out, ref, L):
    for k in ("render", "depth", "radii", "visibility_filter"):
        assert out[k].dtype == ref[k].dtype and torch.equal(out[k], ref[k]), k
    assert _bits_equal(out["render"], ref["render"]) and _bits_equal(out["depth"], ref["depth"])
    assert len(out["layers"]) == L and "render_gaussian_features" not in out
    for l in range(L):
        assert tuple(out["layers"][l].shape) == tuple(ref["render"].shape)
        assert torch.equal(out["layers"][l], ref["layers"][l]) and _bits_equal(out["layers"][l], ref["layers"][l]), f"layer {l}"


@pytest.mark.parametrize("L", [1, 2, 10])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("bgname", sorted(BGS))
@pytest.mark.parametrize("W,H", SIZES)
def test_one_pass_equals_render_and_every_override_render(scene, dev, monkeypatch, W, H, bgname, variant, L):
    ref = _reference(scene, W, H, bgname, variant, dev)
    calls = _count_renders(monkeypatch)
    out = _layers(scene, W, H, bgname, variant, L, dev)
    assert len(calls) == 1                                   # one rasterizer pass, not the composition
    _assert_same(out, ref, L)
    assert out["radii"].shape[0] == (int(scene.mask.sum()) if variant == "mask" else N)
    assert tuple(out["viewspace_points"].shape) == (N, 3) and not out["viewspace_points"].any()


def test_scene_is_not_trivial(scene, dev):
    ref = _reference(scene, 96, 64, "mixed", "plain", dev)
    assert int(ref["visibility_filter"].sum()) > 300
    bg = torch.tensor(BGS["mixed"], device=dev)[:, None, None]
    assert float((ref["render"] != bg).float().mean()) > 0.5                     # most pixels are covered
    assert not torch.equal(ref["layers"][0], ref["layers"][1]) and not torch.equal(ref["layers"][0], ref["render"])


def test_larger_case_640x360_20000_gaussians(dev, monkeypatch):
    big = _Scene(20000, dev, seed=11)
    ref = _reference(big, 640, 360, "mixed", "plain", dev)
    calls = _count_renders(monkeypatch)
    out = _layers(big, 640, 360, "mixed", "plain", 10, dev)
    assert len(calls) == 1
    _assert_same(out, ref, 10)
    _REF.pop((id(big), 640, 360, "mixed", "plain"))


@pytest.mark.parametrize("W,H", [(96, 64), (67, 35)])
def test_byte_frames(scene, dev, W, H):
    out = _layers(scene, W, H, "mixed", "plain", 3, dev, frames_u8=True)
    assert out["render_u8"].dtype == torch.uint8 and tuple(out["render_u8"].shape) == (H, W, 3) and len(out["layers_u8"]) == 3
    assert np.array_equal(out["render_u8"].cpu().numpy(), lr.frames_u8(out["render"].cpu().numpy()))
    for l in range(3):
        assert np.array_equal(out["layers_u8"][l].cpu().numpy(), lr.frames_u8(out["layers"][l].cpu().numpy())), l
    _assert_same(out, _reference(scene, W, H, "mixed", "plain", dev), 3)


def test_strided_and_offset_tables_through_the_call(scene, dev):
    g = torch.Generator().manual_seed(21)
    wide = torch.rand(N, 8, generator=g).to(dev)
    off = torch.rand(3 * N + 1, generator=g).to(dev)[1:].view(N, 3)
    tabs = [wide[:, 1:4], off, wide[:, 5:8]]
    keep = [t.clone() for t in tabs]
    from trase_amd.layers import render_layers
    from trase_amd.renderer import render
    from trase_amd.synthetic import SynthPipe
    cam, bg = _camera(67, 35, dev), torch.tensor(BGS["mixed"], device=dev)
    out = render_layers(cam, scene.pc, SynthPipe(), bg, *scene.d, colors=tabs)
    with torch.no_grad():
        for l, t in enumerate(tabs):
            assert torch.equal(out["layers"][l], render(cam, scene.pc, SynthPipe(), bg, *scene.d, override_color=t)["render"]), l
    assert all(torch.equal(a, b) for a, b in zip(tabs, keep))                   # the inputs are never modified


# ---- state ------------------------------------------------------------------------------------------------------------------------
def _probe(sc, cam, bg):
    """render() under no_grad, and a training forward plus backward: every map and every gradient, cloned."""
    from trase_amd.renderer import render
    from trase_amd.synthetic import SynthPipe
    with torch.no_grad():
        a = render(cam, sc.pc, SynthPipe(), bg, *sc.d)
        got = {f"nograd.{k}": a[k].clone() for k in ("render", "render_gaussian_features", "depth", "radii")}
    for p in sc.pc.parameters():
        p.grad = None
    b = render(cam, sc.pc, SynthPipe(), bg, *sc.d)
    g = torch.Generator().manual_seed(2)
    gi = torch.randn(b["render"].shape, generator=g).to(bg.device)
    gf = torch.randn(b["render_gaussian_features"].shape, generator=g).to(bg.device)
    torch.autograd.backward([b["render"], b["render_gaussian_features"]], [gi, gf])
    got.update({f"train.{k}": b[k].detach().clone() for k in ("render", "render_gaussian_features", "depth", "radii")})
    got.update({f"grad.{i}": p.grad.clone() for i, p in enumerate(sc.pc.parameters())})
    got["grad.m2d"] = b["viewspace_points"].grad.clone()
    return got


@pytest.mark.parametrize("feats_bg", [None, 0.25])
def test_render_and_training_are_untouched_by_a_call(dev, feats_bg):
    from trase_amd import rasterizer as r
    from trase_amd.layers import render_layers
    from trase_amd.renderer import render
    from trase_amd.synthetic import SynthPipe
    sc = _Scene(N, dev, requires_grad=True)
    cam, bg = _camera(96, 64, dev), torch.tensor(BGS["mixed"], device=dev)
    before_policy = (r._Policy.variant, r._Policy.feat_bg)
    try:
        r.set_lineage(feats_bg=feats_bg)
        policy = (r._Policy.variant, r._Policy.feat_bg)
        assert bool(policy[0] & r.VARIANT_FEATS_BG) == (feats_bg is not None)
        before = _probe(sc, cam, bg)
        with torch.no_grad():
            want = [render(cam, sc.pc, SynthPipe(), bg, *sc.d, override_color=t)["render"].clone() for t in sc.tables[:2]]
        keep = [t.clone() for t in sc.tables[:2]]
        out = render_layers(cam, sc.pc, SynthPipe(), bg, *sc.d, colors=sc.tables[:2])          # grad mode on, parameters require grad
        assert (r._Policy.variant, r._Policy.feat_bg) == policy                              # the policy is what it was
        for k, v in out.items():
            for t in (v if isinstance(v, list) else [v]):
                assert t.grad_fn is None and (k == "viewspace_points" or not t.requires_grad), k          # no history
        for l in range(2):                                                                   # the layers' background is bg_color
            assert torch.equal(out["layers"][l], want[l]), l
        assert torch.equal(out["render"], before["nograd.render"]) and torch.equal(out["depth"], before["nograd.depth"])
        assert all(torch.equal(a, b) for a, b in zip(sc.tables[:2], keep))
        again = render_layers(cam, sc.pc, SynthPipe(), bg, *sc.d, colors=sc.tables[:2])
        for k in ("render", "depth", "radii"):
            assert _bits_equal(out[k], again[k]), k
        assert all(_bits_equal(a, b) for a, b in zip(out["layers"], again["layers"]))          # two calls: identical bits
        after = _probe(sc, cam, bg)
        assert set(before) == set(after)
        for k in before:
            assert _bits_equal(before[k], after[k]), k
        if feats_bg is not None:                         # the feature background did reach render()'s own features
            r.set_lineage(feats_bg=None)
            with torch.no_grad():
                plain = render(cam, sc.pc, SynthPipe(), bg, *sc.d)["render_gaussian_features"]
            assert not torch.equal(plain, before["nograd.render_gaussian_features"])
    finally:
        r._Policy.variant, r._Policy.feat_bg = before_policy


def test_arguments_the_fused_forward_rejects_return_the_compositions_values(scene, dev, monkeypatch):
    from trase_amd import renderer
    monkeypatch.setattr(renderer, "_fusable", lambda *a, **k: False)
    from trase_amd.synthetic import SynthPipe
    cam, bg = _camera(67, 35, dev), torch.tensor(BGS["mixed"], device=dev)
    with torch.no_grad():
        base = renderer.render(cam, scene.pc, SynthPipe(), bg, *scene.d, mask=scene.mask)
        want = [renderer.render(cam, scene.pc, SynthPipe(), bg, *scene.d, override_color=t, mask=scene.mask)["render"] for t in scene.tables[:3]]
    calls = _count_renders(monkeypatch)
    from trase_amd.layers import render_layers
    out = render_layers(cam, scene.pc, SynthPipe(), bg, *scene.d, colors=scene.tables[:3], mask=scene.mask, frames_u8=True)
    assert len(calls) == 1 + 3
    for k in ("render", "depth", "radii", "visibility_filter"):
        assert torch.equal(out[k], base[k]), k
    for l in range(3):
        assert torch.equal(out["layers"][l], want[l]), l
        assert np.array_equal(out["layers_u8"][l].cpu().numpy(), lr.frames_u8(want[l].cpu().numpy())), l
    assert np.array_equal(out["render_u8"].cpu().numpy(), lr.frames_u8(base["render"].cpu().numpy()))
    assert "render_gaussian_features" not in out


def test_other_compositing_kernels_take_the_composition(scene, dev, monkeypatch):
    """The image-only forward scope composites on the F = 0 kernel: render_layers must return ITS bits, so it composes."""
    from trase_amd import renderer
    from trase_amd.layers import render_layers
    from trase_amd.synthetic import SynthPipe
    cam, bg = _camera(67, 35, dev), torch.tensor(BGS["mixed"], device=dev)
    renderer.set_forward_scope("image")
    try:
        with torch.no_grad():
            want = renderer.render(cam, scene.pc, SynthPipe(), bg, *scene.d, override_color=scene.tables[0])["render"]
        calls = _count_renders(monkeypatch)
        out = render_layers(cam, scene.pc, SynthPipe(), bg, *scene.d, colors=scene.tables[:1])
        assert len(calls) == 2 and torch.equal(out["layers"][0], want)
    finally:
        renderer.set_forward_scope("all")


def test_refusals_on_the_device(scene, dev, monkeypatch):
    from trase_amd import renderer
    from trase_amd.layers import render_layers
    from trase_amd.synthetic import SynthPipe
    cam, bg = _camera(8, 8, dev), torch.zeros(3, device=dev)
    with pytest.raises(ValueError, match="between 1 and 10"):
        render_layers(cam, scene.pc, SynthPipe(), bg, *scene.d, colors=scene.tables + scene.tables[:1])          # L = 11
    with pytest.raises(ValueError, match="is on"):
        render_layers(cam, scene.pc, SynthPipe(), bg, *scene.d, colors=[scene.tables[0], scene.tables[1].cpu()])
    monkeypatch.setattr(renderer, "_PAIR", [])
    with pytest.raises(RuntimeError, match="render_views"):
        render_layers(cam, scene.pc, SynthPipe(), bg, *scene.d, colors=scene.tables[:1])
