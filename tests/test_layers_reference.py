"""render_layers without a GPU: the numpy statement of the pack layout and of the finish rule (tests/layers_reference.py), the
8-bit frames against the existing ``to8b`` restatement, every refusal of ``trase_layers_pack`` / ``trase_layers_finish`` (they
return before a device is touched, so the pointers handed over here are never followed) and every refusal of
``render_layers``' arguments, with nothing launched."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import evaluate_reference as er
from tests import layers_reference as lr

INVALID, WORKSPACE = -1, -3


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 10])
def test_pack_layout(L):
    g = np.random.default_rng(L)
    P = 37
    tabs = [g.standard_normal((P, 3)).astype(np.float32) for _ in range(L)]
    out = lr.pack(tabs)
    assert out.shape == (P, 32) and out.dtype == np.float32
    for i in (0, 1, P - 1):
        for l in range(L):
            for c in range(3):
                assert out[i, 3 * l + c] == tabs[l][i, c]
    assert np.array_equal(out[:, :3 * L], np.concatenate(tabs, axis=1))
    pad = out[:, 3 * L:]
    assert pad.shape[1] == 32 - 3 * L and not pad.view(np.uint32).any()          # +0.0, bit for bit
    with pytest.raises(AssertionError):
        lr.pack([tabs[0]] * 11)


def _is_nearest(r, exact):
    """r (fp32) is a nearest fp32 of the rational `exact`."""
    r = np.float32(r)
    err = abs(Fraction(float(r)) - exact)
    return all(err <= abs(Fraction(float(np.nextafter(r, np.float32(s)))) - exact) for s in (-np.inf, np.inf))


def test_finish_rule_for_black_and_white():
    g = np.random.default_rng(5)
    H, W, L = 5, 7, 2
    planes = (g.standard_normal((32, H, W)) * np.exp(g.uniform(-12, 3, (32, H, W)))).astype(np.float32)
    T = g.uniform(0, 1, (H, W)).astype(np.float32)
    T[0, :3] = (0.0, 1.0, 1e-30)
    black = lr.finish(planes, T, (0.0, 0.0, 0.0), L)
    assert np.array_equal(black.view(np.uint32), planes.view(np.uint32))         # fma(T, 0, x) = x: nothing at all
    white = lr.finish(planes, T, (1.0, 1.0, 1.0), L)
    assert np.array_equal(white[3 * L:].view(np.uint32), planes[3 * L:].view(np.uint32))
    assert not np.array_equal(white[:3 * L], planes[:3 * L])
    for k in range(3 * L):                                                       # fma(T, 1, x): the exact sum, rounded once
        for y in range(H):
            for x in range(W):
                assert _is_nearest(white[k, y, x], Fraction(float(T[y, x])) + Fraction(float(planes[k, y, x])))
    mixed = lr.finish(planes, T, (1.0, 0.0, 1.0), L)
    assert np.array_equal(mixed[0::3][:L], white[0::3][:L]) and np.array_equal(mixed[1::3][:L], planes[1::3][:L])
    with pytest.raises(ValueError):
        lr.finish(planes, T, (0.2, 0.5, 0.7), L)


def test_byte_frames_are_to8b_transposed():
    g = np.random.default_rng(6)
    x = g.uniform(-0.2, 1.2, (3, 6, 9)).astype(np.float32)
    x[0, 0, :4] = (np.nan, 0.0, 1.0, 254.5 / 255)
    f = lr.frames_u8(x)
    assert f.shape == (6, 9, 3) and f.dtype == np.uint8 and f.flags["C_CONTIGUOUS"]
    assert np.array_equal(f, er.to8b(x).transpose(1, 2, 0))
    ok = ~np.isnan(x)
    assert np.array_equal(er.to8b(x)[ok], (255 * np.clip(x[ok], 0, 1)).astype(np.uint8))          # render.py:106
    assert f[0, 0, 0] == 0 and f[0, 1, 0] == 0 and f[0, 2, 0] == 255 and f[0, 3, 0] == 254


# ---- the entry points' refusals (no device is touched) -------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from trase_amd import _lib
    return _lib.load()


def _tables(*addrs):
    return (C.c_void_p * len(addrs))(*addrs)


A16 = 0x10000          # a 16-byte aligned address that is never followed


def test_pack_refusals(lib):
    ok = [A16 + 4 * l for l in range(10)]                # tables are only 4-byte aligned
    cases = {
        "null tables": (None, 1, 8, A16),
        "null out": (_tables(*ok), 1, 8, None),
        "L = 0": (_tables(*ok), 0, 8, A16),
        "L = 11": (_tables(*(ok + [A16])), 11, 8, A16),
        "negative P": (_tables(*ok), 2, -1, A16),
        "a null table": (_tables(A16, None, A16), 3, 8, A16),
        "a table off a 4-byte boundary": (_tables(A16, A16 + 2), 2, 8, A16),
        "out off a 16-byte boundary": (_tables(*ok), 2, 8, A16 + 8),
        "out off a 16-byte boundary, P = 0": (_tables(*ok), 2, 0, A16 + 4),
    }
    for name, (tabs, L, P, out) in cases.items():
        assert lib.trase_layers_pack(tabs, L, P, out, 0, None) == INVALID, name
        assert b"trase_layers_pack" in lib.trase_last_error(), name
    assert lib.trase_layers_pack(_tables(*ok), 10, 0, A16, 0, None) == 0          # nothing to do: no launch, no device


def test_finish_refusals(lib):
    from trase_amd import _lib
    ws = _lib.RastWorkspace()
    ws.img, ws.img_bytes = A16, 1 << 40
    w = C.byref(ws)
    cases = {
        "null planes": (None, w, A16, 1, 8, 8, None, None, None),
        "L = 0": (A16, w, A16, 0, 8, 8, None, None, None),
        "L = 11": (A16, w, A16, 11, 8, 8, None, None, None),
        "negative W": (A16, w, A16, 1, -1, 8, None, None, None),
        "negative H": (A16, w, A16, 1, 8, -8, None, None, None),
        "W * H = 2^31": (A16, w, A16, 1, 1 << 16, 1 << 15, None, None, None),
        "a workspace without bg": (A16, w, None, 1, 8, 8, None, None, None),
        "nothing to do": (A16, None, None, 1, 8, 8, A16, None, None),
        "image_u8 without the image": (A16, w, A16, 1, 8, 8, None, A16, None),
        "planes off a 4-byte boundary": (A16 + 2, w, A16, 1, 8, 8, None, None, None),
        "image off a 4-byte boundary": (A16, w, A16, 1, 8, 8, A16 + 1, A16, None),
        "bg off a 4-byte boundary": (A16, w, A16 + 3, 1, 8, 8, None, None, None),
    }
    for name, (planes, wsp, bg, L, W, H, image, image_u8, layers_u8) in cases.items():
        assert lib.trase_layers_finish(planes, wsp, bg, L, W, H, image, image_u8, layers_u8, 0, None) == INVALID, name
        assert b"trase_layers_finish" in lib.trase_last_error(), name
    small = _lib.RastWorkspace()
    small.img, small.img_bytes = A16, 8 * 8 * 4                  # final_T alone: the img workspace holds more than that
    assert lib.trase_layers_finish(A16, C.byref(small), A16, 1, 8, 8, None, None, None, 0, None) == WORKSPACE
    absent = _lib.RastWorkspace()
    assert lib.trase_layers_finish(A16, C.byref(absent), A16, 1, 8, 8, None, None, None, 0, None) == WORKSPACE
    assert lib.trase_layers_finish(A16, w, A16, 1, 0, 8, None, None, None, 0, None) == 0          # an empty frame: no launch


# ---- render_layers' refusals ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def cpu_call(monkeypatch):
    """A model and a camera on the host, and the library's loader replaced by one that fails: whatever is refused here is
    refused before anything could have been launched."""
    import trase_amd.layers as ly
    from trase_amd import _lib
    from trase_amd.synthetic import SynthGaussianModel, SynthPipe, make_scene, orbit_camera

    def no_load():
        raise AssertionError("the library was loaded: a launch was on its way")
    monkeypatch.setattr(_lib, "load", no_load)
    pc = SynthGaussianModel(make_scene(8, feat_dim=32, seed=0), requires_grad=False)
    cam = orbit_camera(16, 16)

    def call(colors, **kw):
        return ly.render_layers(cam, pc, SynthPipe(), torch.zeros(3), 0.0, 0.0, 0.0, colors=colors, **kw)
    return call


def test_render_layers_refusals(cpu_call):
    t = torch.rand(8, 3)
    bad = {
        "an empty list": [],
        "eleven tables": [t] * 11,
        "not a list": t,
        "an entry that is no tensor": [t, None],
        "a wrong width": [torch.rand(8, 4)],
        "a wrong row count": [t, torch.rand(7, 3)],
        "a flat table": [torch.rand(24)],
        "float64": [t.double()],
        "float16": [t, t.half()],
        "int32": [torch.zeros(8, 3, dtype=torch.int32)],
        "another device": [t, torch.empty(8, 3, device="meta")],
    }
    for name, colors in bad.items():
        with pytest.raises(ValueError, match="render_layers"):
            cpu_call(colors)


def test_render_layers_inside_render_views_raises(cpu_call, monkeypatch):
    import trase_amd.renderer as rn
    monkeypatch.setattr(rn, "_PAIR", [])
    with pytest.raises(RuntimeError, match="render_views"):
        cpu_call([torch.rand(8, 3)])


def test_render_layers_has_no_cpu_path(cpu_call):
    with pytest.raises(RuntimeError, match="GPU only"):
        cpu_call([torch.rand(8, 3)] * 10)


def test_exports():
    import gaussian_renderer
    import trase_amd
    from trase_amd.layers import MAX_LAYERS, render_layers
    assert trase_amd.render_layers is render_layers and gaussian_renderer.render_layers is render_layers
    assert "render_layers" in trase_amd.__all__ and "render_layers" in gaussian_renderer.__all__
    assert MAX_LAYERS == lr.MAX_LAYERS == 10
