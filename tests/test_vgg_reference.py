"""What the GPU tests of the VGG16 feature extractor (tests/test_gpu_vgg.py) stand on, checked without a GPU: the emulation of
the split arithmetic, the premises of the exact lattice tests, the pool tie rule, weight intake, every refusal of the four C
entry points and of the ``style_transfer`` shim, and the coverage of the GPU tests' size plan."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from tests import vgg_reference as R

SMALL = ((24, 40), (67, 35))


@pytest.fixture(scope="module")
def seeded():
    from trase_amd.vgg import vgg16_random_weights
    return vgg16_random_weights(1, "conv4_1")


def _image(H, W):
    return torch.rand(3, H, W, generator=torch.Generator().manual_seed(H * 1000 + W))


@pytest.mark.parametrize("hw", SMALL, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_three_products_are_64_times_closer_than_one(seeded, hw):
    """the bar of tests/test_mlp_split_reference.py, at conv4_1 and for the image gradient under fixed decisions"""
    H, W = hw
    img = _image(H, W)
    zf = R.forward_f64(seeded, img)
    e3 = R.rel_err(R.forward_emulated(seeded, img)[-1], zf[-1])
    e1 = R.rel_err(R.forward_emulated(seeded, img, products=1)[-1], zf[-1])
    print(f"forward conv4_1 {hw}: bf16x3 {e3:.2e}, bf16 {e1:.2e}")
    assert 64 * e3 <= e1
    dec = R.with_shapes(R.decisions_from(zf[:-1]), H, W)
    cot = torch.randn(zf[-1].shape, generator=torch.Generator().manual_seed(5))
    gf = R.backward_f64(seeded, cot, dec)
    b3 = R.rel_err(R.backward_emulated(seeded, cot, dec), gf)
    b1 = R.rel_err(R.backward_emulated(seeded, cot, dec, products=1), gf)
    print(f"backward {hw}: bf16x3 {b3:.2e}, bf16 {b1:.2e}")
    assert 64 * b3 <= b1


@pytest.mark.parametrize("hw", SMALL + ((64, 96),), ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_emulated_decisions_flip_rarely(seeded, hw):
    img = _image(*hw)
    d64 = R.decisions_from(R.forward_f64(seeded, img)[:-1])
    d3 = R.decisions_from(R.forward_emulated(seeded, img)[:-1])
    relu, pool = R.flip_shares(d3, d64)
    print(f"{hw}: relu flips {relu:.2e}, live pool flips {pool:.2e}")
    assert relu <= 1e-4 and pool <= 1e-4


def test_split_is_exact_for_integers_below_2_16():
    v = torch.arange(-65535, 65536, dtype=torch.float32)
    hi, lo = R.split(v)
    assert torch.equal(hi + lo, v)
    w = torch.arange(-128, 129, dtype=torch.float32)
    assert torch.equal(R.split(w)[1], torch.zeros_like(w))         # small integer weights: lo = 0


@pytest.mark.parametrize("k", range(1, 9), ids=lambda k: R.KEYS[k - 1])
def test_premises_of_the_exact_tests(k):
    """lattice_forward / lattice_backward assert, in int64: every split activation and cotangent below 2^16, every weight a
    small integer, every output's sum |w| max|a| below 2^24 -- here on the GPU tests' own cases"""
    for hw in SMALL + ((8 << R.pools_before(k), 8 << R.pools_before(k)),):
        pairs, img, z, cot, g = R.lattice_case(k, (k,), *hw)
        assert z.dtype == torch.int64 and g.dtype == torch.int64
        assert int(z.abs().max()) > 0 and int(g.abs().max()) > 0
        assert int(z.abs().max()) < 2 ** 24 and int(g.abs().max()) < 2 ** 24
        for w, b in pairs:
            assert torch.equal(w, w.round()) and float(w.abs().max()) <= 2


def test_premises_of_the_whole_stack_and_its_pool_ties():
    for hw in SMALL + ((256, 320),):
        pairs, img, z, cot, g = R.lattice_case(8, (), *hw)
        assert int(z.abs().max()) > 0 and int(g.abs().max()) > 0
    zs = R.lattice_forward(pairs, img)
    ties = 0
    for l in R.POOL_AFTER:
        a = torch.relu(zs[l - 1])
        best, _ = R.pool_decide(a)
        h, w = best.shape[1:]
        count = sum((a[:, dy:2 * h:2, dx:2 * w:2] == best).to(torch.int64) for dy in (0, 1) for dx in (0, 1))
        ties += int(((count > 1) & (best > 0)).sum())
    assert ties > 1000                                             # the tie rule is exercised, not avoided


def test_pool_tie_rule_is_atens():
    g = torch.Generator().manual_seed(9)
    a = torch.randint(0, 3, (16, 13, 18), generator=g).double()   # few values: most windows tie
    best, idx = R.pool_decide(a)
    ref, flat = F.max_pool2d(a[None], 2, 2, return_indices=True)
    assert torch.equal(best, ref[0])
    y, x = torch.meshgrid(torch.arange(6), torch.arange(9), indexing="ij")
    mine = (2 * y + idx // 2) * 18 + (2 * x + idx % 2)
    assert torch.equal(mine, flat[0])
    assert int((idx > 0).sum()) > 0 and int((idx == 0).sum()) > 0
    # a pooled maximum of 0 passes no gradient
    gsc = R.unpool(torch.ones(16, 6, 9, dtype=torch.float64), idx, best > 0, 13, 18)
    assert float(gsc.sum()) == float((best > 0).sum()) and float(gsc[:, 12].abs().sum()) == 0


def test_fp32_chain_of_conv1_1_is_close_to_float64(seeded):
    x = R.normalise_fp32(_image(9, 15))
    w, b = seeded[0]
    z = R.conv1_fp32_chain(x, w, b)
    ref = F.conv2d(x.double()[None], w.double(), b.double(), padding=1)[0]
    assert z.dtype == torch.float32 and R.rel_err(z, ref) < 27 * 2.0 ** -24


def test_backward_f64_is_autograd_under_its_own_decisions(seeded):
    H, W = 24, 40
    img = _image(H, W)
    x = R.normalise_fp32(img).double().requires_grad_(True)
    a = x
    for l, (w, b) in enumerate(seeded, start=1):
        z = F.conv2d(a[None], w.double(), b.double(), padding=1)[0]
        a = torch.relu(z)
        if l in R.POOL_AFTER:
            a = F.max_pool2d(a[None], 2, 2)[0]
    cot = torch.randn(z.shape, generator=torch.Generator().manual_seed(2)).double()
    (z * cot).sum().backward()
    zf = R.forward_f64(seeded, img)
    assert torch.equal(zf[-1], z.detach())
    g = R.backward_f64(seeded, cot, R.with_shapes(R.decisions_from(zf[:-1]), H, W), normalize=False)
    assert R.rel_err(g, x.grad) < 1e-12


# ---- weight intake ----------------------------------------------------------------------------------------------------------
def test_weight_intake(seeded):
    from trase_amd.vgg import FEATURE_INDEX, key_layers, vgg16_random_weights, weight_pairs
    full, bare = {"classifier.0.weight": torch.zeros(1)}, {}
    for idx, (w, b) in zip(FEATURE_INDEX, seeded):
        full[f"features.{idx}.weight"], full[f"features.{idx}.bias"] = w, b
        bare[f"{idx}.weight"], bare[f"{idx}.bias"] = w, b
    for src in (full, bare, seeded, [list(p) for p in seeded]):
        for key in ("conv1_1", "conv3_2", "conv4_1"):
            got = weight_pairs(src, key_layers(key))
            assert len(got) == key_layers(key)
            assert all(torch.equal(a, w) and torch.equal(c, b) for (a, c), (w, b) in zip(got, seeded))
    with pytest.raises(KeyError, match="features.17.weight"):
        weight_pairs({k: v for k, v in full.items() if not k.startswith("features.17")}, 8)
    with pytest.raises(ValueError, match="pairs are needed"):
        weight_pairs(seeded[:3], 8)
    with pytest.raises(ValueError, match="conv2_1 expects"):
        weight_pairs(seeded[:2] + [(torch.zeros(128, 3, 3, 3), torch.zeros(128))], 3)
    with pytest.raises(NotImplementedError, match="conv4_1"):
        key_layers("conv4_2")
    again = vgg16_random_weights(1, "conv2_2")
    assert all(torch.equal(a, w) and torch.equal(c, b) for (a, c), (w, b) in zip(again, seeded))      # a shorter key: the same numbers
    cin = 64
    assert abs(float(seeded[1][0].std()) - (2.0 / (9 * cin)) ** 0.5) < 0.02 * (2.0 / (9 * cin)) ** 0.5
    assert abs(float(seeded[7][1].std()) - 0.05) < 0.01


# ---- refusals of the C entry points, before a device is touched -----------------------------------------------------------
INVALID, WORKSPACE = -1, -3


def _lib():
    from trase_amd import _lib
    return _lib, _lib.load()


def _sizes_call(lib, layers, H, W, null=None):
    out = [C.c_size_t() for _ in range(4)] + [C.c_int32() for _ in range(3)]
    args = [None if i == null else C.byref(v) for i, v in enumerate(out)]
    return lib.trase_vgg_ws_bytes(layers, H, W, *args), out


def test_sizes_and_their_refusals():
    _l, lib = _lib()
    rc, out = _sizes_call(lib, 8, 1080, 1920)
    assert rc == 0 and [v.value for v in out[4:]] == [512, 135, 240]
    pack, wsf, wsb, saved = [v.value for v in out[:4]]
    units = [1080 * 1920 * 64, 540 * 960 * 64, 540 * 960 * 128, 270 * 480 * 128, 270 * 480 * 256, 270 * 480 * 256, 135 * 240 * 256]
    bits = sum(u // 2 if l in R.POOL_AFTER else u // 8 for l, u in zip(range(1, 8), units))      # 4 bits per pooled unit, 1 per unit
    assert bits <= saved <= bits + 7 * 256 and saved < 64e6
    assert wsf <= wsb and wsb <= 2 * 2 * 2 * 1080 * 1920 * 64 + 4 * 256      # two buffers of hi and lo bf16 planes
    assert pack >= 2 * 2 * 2 * 9 * sum(a * b for a, b in zip(R.CHANNELS[1:-1], R.CHANNELS[2:]))
    for k in range(1, 9):
        p = R.pools_before(k)
        rc, out = _sizes_call(lib, k, 1 << p, 1 << p)
        assert rc == 0 and [v.value for v in out[4:]] == [R.CHANNELS[k], 1, 1]
        if p:
            assert _sizes_call(lib, k, (1 << p) - 1, 64)[0] == INVALID and _sizes_call(lib, k, 64, (1 << p) - 1)[0] == INVALID
    for layers in (0, 9, -1):
        assert _sizes_call(lib, layers, 64, 64)[0] == INVALID
        assert b"layers" in lib.trase_last_error()
    assert _sizes_call(lib, 8, 4096, 8192)[0] == INVALID                       # H * W = 2^25
    assert b"2^25" in lib.trase_last_error()
    assert _sizes_call(lib, 8, 4096, 8191)[0] == 0
    for null in range(7):
        assert _sizes_call(lib, 8, 64, 64, null=null)[0] == INVALID


def _host_ptrs(n, null_at=None):
    return (C.c_void_p * n)(*[None if i == null_at else 4096 + 64 * i for i in range(n)])


def test_pack_refusals():
    _l, lib = _lib()
    rc, out = _sizes_call(lib, 8, 64, 64)
    pack_b = out[0].value
    good = 1 << 20                                                              # an aligned address that is never dereferenced
    w, b = _host_ptrs(8), _host_ptrs(8)
    assert lib.trase_vgg_pack(0, w, b, good, pack_b, 0, None) == INVALID
    assert lib.trase_vgg_pack(9, w, b, good, pack_b, 0, None) == INVALID
    assert lib.trase_vgg_pack(8, None, b, good, pack_b, 0, None) == INVALID
    assert lib.trase_vgg_pack(8, w, None, good, pack_b, 0, None) == INVALID
    assert lib.trase_vgg_pack(8, w, b, None, pack_b, 0, None) == INVALID
    assert lib.trase_vgg_pack(8, _host_ptrs(8, null_at=5), b, good, pack_b, 0, None) == INVALID
    assert b"null layer 5" in lib.trase_last_error()
    assert lib.trase_vgg_pack(8, w, _host_ptrs(8, null_at=7), good, pack_b, 0, None) == INVALID
    assert lib.trase_vgg_pack(8, w, b, good + 4, pack_b, 0, None) == INVALID
    assert b"aligned" in lib.trase_last_error()
    assert lib.trase_vgg_pack(8, w, b, good, pack_b - 1, 0, None) == WORKSPACE
    assert lib.trase_vgg_pack(8, w, b, good, _sizes_call(lib, 7, 64, 64)[1][0].value, 0, None) == WORKSPACE


def test_forward_refusals():
    _l, lib = _lib()
    H = W = 64
    pack_b, wsf, wsb, saved_b = [v.value for v in _sizes_call(lib, 8, H, W)[1][:4]]
    p = 1 << 20
    mean = (C.c_float * 3)(*R.MEAN)

    def call(layers=8, pack=p, pack_bytes=pack_b, image=p, H=H, W=W, mean=None, inv_std=None, out=p, saved=p, saved_bytes=saved_b,
             ws=p, ws_bytes=wsf):
        return lib.trase_vgg_forward(layers, pack, pack_bytes, image, H, W, mean, inv_std, out, saved, saved_bytes, ws, ws_bytes, 0, None)

    assert call(layers=0) == INVALID and call(layers=9) == INVALID
    assert call(H=7) == INVALID and call(W=7) == INVALID and call(H=4096, W=8192) == INVALID
    assert call(pack=None) == INVALID and call(image=None) == INVALID and call(out=None) == INVALID
    assert call(mean=mean) == INVALID and call(inv_std=mean) == INVALID
    assert b"come together" in lib.trase_last_error()
    assert call(pack=p + 8) == INVALID and call(ws=p + 2) == INVALID and call(saved=p + 4) == INVALID
    assert call(pack_bytes=pack_b - 1) == WORKSPACE
    assert call(ws=None) == WORKSPACE and call(ws_bytes=wsf - 1) == WORKSPACE
    assert b"workspace too small" in lib.trase_last_error()
    assert call(saved_bytes=saved_b - 1) == WORKSPACE
    assert b"saved buffer too small" in lib.trase_last_error()


def test_backward_refusals():
    _l, lib = _lib()
    H = W = 64
    pack_b, wsf, wsb, saved_b = [v.value for v in _sizes_call(lib, 8, H, W)[1][:4]]
    p = 1 << 20

    def call(layers=8, pack=p, pack_bytes=pack_b, d_out=p, H=H, W=W, inv_std=None, saved=p, saved_bytes=saved_b, d_image=p, ws=p,
             ws_bytes=wsb):
        return lib.trase_vgg_backward(layers, pack, pack_bytes, d_out, H, W, inv_std, saved, saved_bytes, d_image, ws, ws_bytes, 0, None)

    assert call(layers=0) == INVALID and call(layers=9) == INVALID
    assert call(H=7) == INVALID and call(W=7) == INVALID and call(H=4096, W=8192) == INVALID
    for name in ("pack", "d_out", "d_image", "ws", "saved"):
        assert call(**{name: None}) == INVALID, name
    assert call(pack=p + 8) == INVALID and call(ws=p + 2) == INVALID and call(saved=p + 4) == INVALID
    assert call(pack_bytes=pack_b - 1) == WORKSPACE
    assert call(ws_bytes=wsb - 1) == WORKSPACE and call(ws_bytes=wsf) == WORKSPACE        # the forward's workspace is the smaller one
    assert call(saved_bytes=saved_b - 1) == WORKSPACE


# ---- the style_transfer shim --------------------------------------------------------------------------------------------------
def test_shim_refusals_and_weight_sources(seeded, tmp_path, monkeypatch):
    from style_transfer import fx
    from trase_amd.vgg import FEATURE_INDEX
    monkeypatch.delenv("TRASE_VGG16_WEIGHTS", raising=False)
    with pytest.raises(RuntimeError, match="TRASE_VGG16_WEIGHTS"):
        fx.VGG16FeatureExtractor(["conv4_1"])
    for keys, what in ((["conv4_1", "conv3_1"], "one key"), (["relu4_1"], "relu"), ("relu2_2", "relu"), (["conv3"], "block keys"),
                       (["conv4_2"], "conv4_1"), (["conv5_1"], "conv4_1"), ([], "one key")):
        with pytest.raises(NotImplementedError, match=what) as e:
            fx.VGG16FeatureExtractor(keys, weights=seeded)
        assert "conv1_1" in str(e.value) and "conv4_1" in str(e.value)               # names what is supported
    with pytest.raises(ValueError, match="invalid identifier"):
        fx.VGG16FeatureExtractor(["pool3"], weights=seeded)
    with pytest.raises(NotImplementedError, match="VGG19"):
        fx.VGG19FeatureExtractor(["conv4_1"], weights=seeded)
    sd = {}
    for idx, (w, b) in zip(FEATURE_INDEX, seeded):
        sd[f"features.{idx}.weight"], sd[f"features.{idx}.bias"] = w, b
    path = tmp_path / "vgg16.pt"
    torch.save(sd, path)
    monkeypatch.setenv("TRASE_VGG16_WEIGHTS", str(path))
    for ext in (fx.VGG16FeatureExtractor(["conv4_1"]), fx.VGGFeatureExtractor("conv4_1", weights=sd),
                fx.VGG16FeatureExtractor(["conv4_1"], weights=seeded)):
        assert isinstance(ext, torch.nn.Module) and ext.eval() is ext
        assert torch.equal(ext.w8, seeded[7][0]) and torch.equal(ext.b1, seeded[0][1])
        assert not ext.state_dict()                                                   # constants, not parameters
    x = torch.rand(3, 8, 8).requires_grad_(True)
    n = ext.normalize(x)
    ref = (x - torch.tensor(R.MEAN).view(3, 1, 1)) / torch.tensor(R.STD).view(3, 1, 1)
    assert torch.allclose(n, ref, rtol=0, atol=1e-6) and n.requires_grad
    with pytest.raises(RuntimeError, match="GPU only"):
        ext(x)


def test_features_refuse_the_cpu_and_bad_shapes(seeded):
    from trase_amd.vgg import VGG16Features
    net = VGG16Features(seeded, "conv1_2")
    assert net.layers == 2 and net.pack is None and net.out_shape(67, 35) == (1, 64, 67, 35)
    assert VGG16Features(seeded, "conv4_1").out_shape(67, 35) == (1, 512, 8, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        net(torch.rand(3, 8, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        net.to("cpu")
    with pytest.raises(NotImplementedError, match="supported keys"):
        VGG16Features(seeded, "relu1_1")


# ---- the GPU tests' size plan -------------------------------------------------------------------------------------------------
def test_size_plan_covers_every_class():
    """tile constants of csrc/vgg.hip: a 16 x 16 pixel tile per workgroup, 4 rows per wave, 64 output channels per workgroup"""
    T = R.VG_TILE
    assert (T, R.VG_NB) == (16, 64)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "trase_amd", "csrc", "vgg.hip")).read()
    assert "constexpr int VG_TILE = 16;" in src and "constexpr int VG_NB = 64;" in src
    for k in range(1, 9):
        p = R.pools_before(k)
        sizes = R.exact_sizes(k)
        at_layer = [(h >> p, w >> p) for h, w in sizes]
        assert (8, 8) in sizes and (9, 15) in sizes and (24, 40) in sizes and (67, 35) in sizes and (256, 320) in sizes
        assert all(h >= 1 << p and w >= 1 << p for h, w in sizes)
        for d in (-1, 0, 1):                                      # one tile -1 / 0 / +1 pixels, in each direction
            assert any(h == T + d for h, _ in at_layer) and any(w == T + d for _, w in at_layer)
        assert any(h == 2 * T + 1 and w == 2 * T + 1 for h, w in at_layer)                     # two tiles + 1
        if k > 1:                                                 # many workgroups: tiles x channel blocks
            assert any(((h + T - 1) // T) * ((w + T - 1) // T) * (R.CHANNELS[k] // R.VG_NB) >= 48 for h, w in at_layer)
    # 256 x 320 gives many workgroups at every layer, conv4_1 included: 2 x 3 tiles x 8 channel blocks
    assert (32 // T) * ((40 + T - 1) // T) * (512 // R.VG_NB) == 48
    # 67 x 35 is odd at the first two pools (67 -> 33 -> 16 -> 8, 35 -> 17 -> 8 -> 4), 44 x 52 at the third (-> 11 x 13)
    assert (67 % 2, 33 % 2, 35 % 2, 17 % 2) == (1, 1, 1, 1) and (67 >> 3, 35 >> 3) == (8, 4)
    assert (44, 52) in R.IMAGE_SIZES and ((44 >> 2) % 2, (52 >> 2) % 2) == (1, 1)
