"""LPIPS (VGG) without a GPU: tests/lpips_reference.py against the fixture the reference's own ``forward`` wrote
(tests/golden/lpips.npz, tests/golden/make_lpips.py), the properties the GPU bars of tests/test_gpu_lpips.py rest on, and every
refusal of the four C entry points, of the Python interface and of the ``lpipsPyTorch`` shim (all of them happen before a device
is touched).

Measured here (seed 20, sizes 16x16, 24x40, 67x35, 256x320, the three kinds of pair): per layer, the one-product emulation's
``max|map - f64| / max|f64|`` is 245 to 97000 times the three-product emulation's; the factor asserted is 64, the margin
tests/test_gpu_vgg.py takes below its measured 350 to 760.  The smallest share of a layer in a total is 2.2e-3."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import lpips_reference as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips.npz")
MARGIN = 4.0                    # the GPU bar: device error / emulation error
FACTOR = 64.0                   # one-product emulation error / three-product emulation error, asserted
SMALL_CASES = [(kind, hw) for hw in ((16, 16), (24, 40), (67, 35)) for kind in ("independent", "quantised", "patch")]
INVALID, WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def seeded(golden):
    return L.weights(int(golden["seed"]))


def test_random_weights_are_deterministic_and_match_the_fixtures_checksums(golden, seeded):
    pairs, lins = seeded
    again_pairs, again_lins = L.weights(int(golden["seed"]))
    assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(pairs, again_pairs))
    assert all(torch.equal(a, b) for a, b in zip(lins, again_lins))
    other, _ = L.weights(int(golden["seed"]) + 1)
    assert not torch.equal(other[0][0], pairs[0][0])
    assert len(pairs) == 13 and [tuple(w.shape[:2]) for w, _ in pairs] == [(L.CHANNELS[l], L.CHANNELS[l - 1]) for l in range(1, 14)]
    assert [v.numel() for v in lins] == list(L.TAP_CHANNELS) and all(bool((v >= 0).all()) and float(v.sum()) > 0 for v in lins)
    assert all(w.device.type == "cpu" for w, _ in pairs)
    got, want = L.checksums(pairs, lins).numpy(), golden["checksums"]
    assert got.shape == want.shape
    assert np.allclose(got, want, rtol=1e-12, atol=0), "lpips_random_weights drifted from the generator the fixture was written with"


@pytest.mark.parametrize("i", (0, 1))
def test_forward_f64_reproduces_the_reference(golden, seeded, i):
    pairs, lins = seeded
    x, y = torch.from_numpy(golden[f"x{i}"]), torch.from_numpy(golden[f"y{i}"])
    assert tuple(x.shape[1:]) == ((35, 67), (16, 16))[i] and torch.equal((x * 255).round() / 255, x)
    f = L.forward_f64(pairs, lins, x, y)
    want_layers, want_total = golden[f"layers_f64_{i}"], float(golden[f"total_f64_{i}"])
    assert np.allclose(f["layers"].numpy(), want_layers, rtol=1e-12, atol=0)
    assert abs(float(f["total"]) - want_total) <= 1e-12 * want_total
    # the reference's own fp32 run agrees with its float64 run as fp32 does; this pins that the fixture's two runs are one network
    assert abs(float(golden[f"total_f32_{i}"]) - want_total) <= 1e-4 * want_total
    assert float((f["layers"] / f["total"]).min()) >= 1e-3


@pytest.mark.parametrize("kind,hw", SMALL_CASES, ids=[f"{k}-{h}x{w}" for k, (h, w) in SMALL_CASES])
def test_emulations_against_float64(kind, hw):
    """the bars of the GPU test discriminate: every layer counts, three products beat one by FACTOR, one product misses the bar"""
    c = L.real_case(kind, *hw)
    f, e3, e1 = c["f64"], c["emu3"], c["emu1"]
    share = f["layers"] / f["total"]
    assert float(share.min()) >= 1e-3, share.tolist()
    for l in range(5):
        r3, r1 = L.map_err(e3["maps"][l], f["maps"][l]), L.map_err(e1["maps"][l], f["maps"][l])
        print(f"{kind} {hw} layer {l}: three products {r3:.3e}, one product {r1:.3e}, factor {r1 / r3:.0f}")
        assert r1 >= FACTOR * r3
        assert r1 > MARGIN * r3, "the one-product emulation must miss the GPU bar"
    bar = MARGIN * L.total_bar(e3, f)
    assert abs(float(e1["total"] - f["total"])) > bar, "the one-product emulation must miss the bar of the total"
    assert abs(float(e3["total"] - f["total"])) <= bar


@pytest.mark.parametrize("kind,hw", SMALL_CASES[3:6], ids=[f"{k}-{h}x{w}" for k, (h, w) in SMALL_CASES[3:6]])
def test_emulated_head_within_its_bound(kind, hw):
    """the device's head arithmetic against the float64 head on the SAME taps, inside the bound derived in lpips_reference.py"""
    c = L.real_case(kind, *hw)
    _, lins = L.weights(L.CASE_SEED)
    for a, b, lin, m in zip(c["emu3"]["taps_x"], c["emu3"]["taps_y"], lins, c["emu3"]["maps"]):
        d = L.head_f64(a, b, lin)
        assert bool(((m.double() - d).abs() <= L.head_bound(d, lin)).all())


def test_head_zero_pixel_equal_inputs_and_symmetry():
    g = torch.Generator().manual_seed(5)
    a, b = torch.rand(64, 3, 5, generator=g), torch.rand(64, 3, 5, generator=g)
    lin = torch.rand(64, generator=g)
    a[:, 0, 0] = 0                  # a zero pixel in one image
    a[:, 1, 1] = 0
    b[:, 1, 1] = 0                  # and in both
    for head in (L.head_f64, L.head_device):
        m = head(a, b, lin)
        assert bool(torch.isfinite(m).all()) and float(m[1, 1]) == 0.0
        assert float(m[0, 0]) == pytest.approx(float((lin.double() * (b[:, 0, 0].double() / b[:, 0, 0].double().norm()) ** 2).sum()), rel=1e-6)
        assert torch.equal(head(b, a, lin), m)
        assert float(head(a, a, lin).abs().max()) == 0.0


def test_lattice_premises_hold_at_every_exact_size():
    """the int64 statement to layer 13 asserts its premises on the data; the small sizes here, the rest in the GPU test"""
    for hw in ((16, 16), (17, 31), (32, 48)):
        pairs, x, y, tx, ty = L.lattice_case(*hw)
        assert [tuple(t.shape) for t in tx] == [(c, hw[0] >> l, hw[1] >> l) for l, c in enumerate(L.TAP_CHANNELS)]
        assert all(t.dtype == torch.int64 and int(t.max()) > 0 for t in tx + ty)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
P = 1 << 20                       # a non-null, 16-byte aligned address that is never dereferenced: every refusal comes first


def _lib():
    from trase_amd import _lib as lib
    return lib, lib.load()


def _refused(rc, code, *words):
    lib, _ = _lib()
    assert rc == code, (rc, lib.last_error())
    msg = lib.last_error()
    assert all(w in msg for w in words), msg


def test_ws_bytes_sizes_and_refusals():
    lib, so = _lib()
    sz = [C.c_size_t() for _ in range(3)]
    refs = [C.byref(v) for v in sz]
    assert so.trase_lpips_ws_bytes(35, 67, *refs) == 0
    pack, ws, maps = (v.value for v in sz)
    assert maps == 35 * 67 + 17 * 33 + 8 * 16 + 4 * 8 + 2 * 4
    r = lambda n: (n + 255) // 256 * 256
    assert ws == 6 * r(35 * 67 * 64 * 2) + r(4 * maps) + 5 * 256 * 8    # three split activations of 64 channels, maps, partial sums
    n_w = sum(9 * L.CHANNELS[l - 1] * L.CHANNELS[l] for l in range(2, 14))
    assert pack >= 4 * n_w + 4 * 64 * 27 and pack <= 4 * n_w + (1 << 16)    # hi and lo bf16 per weight: no backward streams
    for H, W in ((15, 16), (16, 15), (0, 64), (8192, 4096)):
        _refused(so.trase_lpips_ws_bytes(H, W, *refs), INVALID, "trase_lpips_ws_bytes", "H, W >= 16")
    for i in range(3):
        args = list(refs)
        args[i] = None
        _refused(so.trase_lpips_ws_bytes(32, 32, *args), INVALID, "null pointer")


def test_pack_refusals():
    lib, so = _lib()
    w13, l5 = (C.c_void_p * 13)(*[P] * 13), (C.c_void_p * 5)(*[P] * 5)
    big = 1 << 30
    _refused(so.trase_lpips_pack(None, w13, l5, P, big, 0, None), INVALID, "null pointer")
    _refused(so.trase_lpips_pack(w13, None, l5, P, big, 0, None), INVALID, "null pointer")
    _refused(so.trase_lpips_pack(w13, w13, None, P, big, 0, None), INVALID, "null pointer")
    _refused(so.trase_lpips_pack(w13, w13, l5, None, big, 0, None), INVALID, "null pointer")
    hole = (C.c_void_p * 13)(*([P] * 12 + [None]))
    _refused(so.trase_lpips_pack(hole, w13, l5, P, big, 0, None), INVALID, "null layer 12")
    _refused(so.trase_lpips_pack(w13, w13, (C.c_void_p * 5)(P, P, None, P, P), P, big, 0, None), INVALID, "null lin 2")
    _refused(so.trase_lpips_pack(w13, w13, l5, P + 8, big, 0, None), INVALID, "16-byte aligned")
    _refused(so.trase_lpips_pack(w13, w13, l5, P, 1024, 0, None), WORKSPACE, "pack buffer too small")


def _forward_args(**over):
    a = dict(pack=P, pack_bytes=1 << 30, x=P, y=P, H=32, W=32, mean=None, inv_std=None, out=P, maps=None, tx=None, ty=None, ws=P,
             ws_bytes=1 << 30)
    a.update(over)
    return [a[k] for k in ("pack", "pack_bytes", "x", "y", "H", "W", "mean", "inv_std", "out", "maps", "tx", "ty", "ws", "ws_bytes")] + [0, None]


def test_forward_refusals():
    lib, so = _lib()
    f3 = (C.c_float * 3)(0, 0, 0)
    for H, W in ((15, 32), (32, 15), (8192, 4096)):
        _refused(so.trase_lpips_forward(*_forward_args(H=H, W=W)), INVALID, "H, W >= 16")
    for name in ("pack", "x", "y", "out", "ws"):
        _refused(so.trase_lpips_forward(*_forward_args(**{name: None})), INVALID, "null pointer")
    _refused(so.trase_lpips_forward(*_forward_args(mean=f3)), INVALID, "mean and inv_std come together")
    _refused(so.trase_lpips_forward(*_forward_args(inv_std=f3)), INVALID, "mean and inv_std come together")
    _refused(so.trase_lpips_forward(*_forward_args(tx=P)), INVALID, "taps_x and taps_y come together")
    _refused(so.trase_lpips_forward(*_forward_args(ty=P)), INVALID, "taps_x and taps_y come together")
    _refused(so.trase_lpips_forward(*_forward_args(pack=P + 8)), INVALID, "16-byte aligned")
    _refused(so.trase_lpips_forward(*_forward_args(ws=P + 4)), INVALID, "16-byte aligned")
    _refused(so.trase_lpips_forward(*_forward_args(out=P + 4)), INVALID, "8-byte aligned")
    for name in ("x", "y", "maps"):
        _refused(so.trase_lpips_forward(*_forward_args(**{name: P + 2})), INVALID, "4-byte aligned")
    _refused(so.trase_lpips_forward(*_forward_args(tx=P + 2, ty=P)), INVALID, "4-byte aligned")
    _refused(so.trase_lpips_forward(*_forward_args(pack_bytes=1 << 20)), WORKSPACE, "pack buffer too small")
    sz = [C.c_size_t() for _ in range(3)]
    assert so.trase_lpips_ws_bytes(32, 32, *[C.byref(v) for v in sz]) == 0
    _refused(so.trase_lpips_forward(*_forward_args(ws_bytes=sz[1].value - 1)), WORKSPACE, "workspace too small")


def test_head_refusals():
    from trase_amd.lpips import head_ws_bytes
    lib, so = _lib()
    ok = dict(a=P, b=P, lin=P, C=64, hw=10, out=P, map=None, ws=P, ws_bytes=1 << 30)

    def call(**over):
        a = dict(ok)
        a.update(over)
        return so.trase_lpips_head(*[a[k] for k in ("a", "b", "lin", "C", "hw", "out", "map", "ws", "ws_bytes")], 0, None)

    for c in (0, 32, 96, 192, 1024):
        _refused(call(C=c), INVALID, "C in {64, 128, 256, 512}")
    _refused(call(hw=0), INVALID, "hw >= 1")
    _refused(call(C=512, hw=1 << 22), INVALID, "C * hw < 2^31")
    for name in ("a", "b", "lin", "out", "ws"):
        _refused(call(**{name: None}), INVALID, "null pointer")
    _refused(call(ws=P + 8), INVALID, "16-byte aligned")
    _refused(call(out=P + 4), INVALID, "8-byte aligned")
    for name in ("a", "b", "lin", "map"):
        _refused(call(**{name: P + 2}), INVALID, "4-byte aligned")
    for c, hw in ((64, 1), (128, 65), (512, 67 * 35)):
        _refused(call(C=c, hw=hw, ws_bytes=head_ws_bytes(c, hw) - 1), WORKSPACE, "workspace too small")


def test_python_interface_refusals(seeded):
    from trase_amd.lpips import LPIPSVGG, lin_vectors, lpips_head, weight_pairs
    pairs, lins = seeded
    with pytest.raises(ValueError, match="13"):
        weight_pairs(pairs[:8])
    with pytest.raises(ValueError, match="conv4_2"):
        weight_pairs(pairs[:8] + [pairs[7]] + pairs[9:])
    with pytest.raises(KeyError, match="features.28.weight"):
        weight_pairs({f"features.{i}.{n}": t for i, (w, b) in zip(L.FEATURE_INDEX[:12], pairs) for n, t in (("weight", w), ("bias", b))})
    with pytest.raises(ValueError, match="five"):
        lin_vectors(lins[:4])
    with pytest.raises(ValueError, match="lin3"):
        lin_vectors(lins[:3] + [lins[2], lins[4]])
    with pytest.raises(KeyError, match="lin4.model.1.weight"):
        lin_vectors({f"lin{k}.model.1.weight": v for k, v in enumerate(lins[:4])})
    published = {f"lin{k}.model.1.weight": v.view(1, -1, 1, 1) for k, v in enumerate(lins)}
    renamed = {f"{k}.1.weight": v.view(1, -1, 1, 1) for k, v in enumerate(lins)}
    for d in (published, renamed):
        assert all(torch.equal(a, b) for a, b in zip(lin_vectors(d), lins))
    sd = {f"{i}.{n}": t for i, (w, b) in zip(L.FEATURE_INDEX, pairs) for n, t in (("weight", w), ("bias", b))}
    net = LPIPSVGG(sd, published)                  # CPU weights, no device: nothing is packed yet
    assert net.pack is None and net.packs == 0
    x = torch.rand(3, 32, 32)
    with pytest.raises(RuntimeError, match="GPU only"):
        net(x, x)
    with pytest.raises(RuntimeError, match="GPU only"):
        net.to("cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        lpips_head(torch.rand(64, 4), torch.rand(64, 4), torch.rand(64))


def test_shim_refusals(monkeypatch, tmp_path):
    import lpipsPyTorch as shim
    x = torch.rand(3, 32, 32)
    for net_type in ("alex", "squeeze"):
        with pytest.raises(NotImplementedError, match="net_type='vgg', version='0.1'"):
            shim.LPIPS(net_type)
        with pytest.raises(NotImplementedError, match="net_type='vgg', version='0.1'"):
            shim.lpips(x, x, net_type=net_type)
    with pytest.raises(NotImplementedError, match="supported"):
        shim.lpips(x, x)                            # the signature's default is 'alex'
    with pytest.raises(NotImplementedError, match="supported"):
        shim.LPIPS("vgg", version="0.0")
    with pytest.raises(NotImplementedError, match="supported"):
        shim.LPIPS("resnet")
    monkeypatch.delenv(shim.VGG_ENV, raising=False)
    monkeypatch.delenv(shim.LIN_ENV, raising=False)
    with pytest.raises(RuntimeError, match="TRASE_VGG16_WEIGHTS.*TRASE_LPIPS_VGG_WEIGHTS"):
        shim.LPIPS("vgg")
    with pytest.raises(RuntimeError, match="TRASE_VGG16_WEIGHTS.*TRASE_LPIPS_VGG_WEIGHTS"):
        shim.lpips(x, x, net_type="vgg")
    monkeypatch.setenv(shim.VGG_ENV, str(tmp_path / "vgg16.pt"))
    with pytest.raises(RuntimeError, match="TRASE_LPIPS_VGG_WEIGHTS"):
        shim.LPIPS("vgg")                           # one of the two is not enough
    assert not hasattr(shim, "get_state_dict") and "hub" not in open(shim.__file__).read()      # nothing that could download
