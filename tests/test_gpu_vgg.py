"""The VGG16 feature extractor of the style-transfer loop on the GPU (trase_amd/vgg.py, csrc/vgg.hip) against
tests/vgg_reference.py.

* exact: lattice data (integer images, integer weights and cotangents) has one right fp32 answer in any summation order;
  every layer through its truncation and the whole stack, forward and backward, ``torch.equal`` against the int64 statement,
  every case twice for identical bits, with a 0xCD canary behind every output;
* real-valued: seeded weights, images in [0, 1]: ``max|gpu - f64| / max|f64|`` at most 4 times the emulation's own figure
  (the margin of tests/test_gpu_mlp_precise.py), which the one-product bf16 emulation misses; the backward under the device's
  own decisions, read off its truncated forwards;
* the Python interface, the ``style_transfer`` shim and a style-transfer iteration on the real topology."""
import ctypes as C
import functools
import json
import os
import warnings

import pytest
import torch

from tests import vgg_reference as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CANARY = 0xCD
PAD = 256                      # canary bytes behind every output
MARGIN = 4.0                   # device error / emulation error (tests/test_gpu_mlp_precise.py)
FLIP_CAP = 1e-4
REAL_SIZES = ((24, 40), (67, 35), (256, 320))
BWD_SIZES = ((24, 40), (67, 35))


def _record(name, share):
    """shares of the bars for profiles/bench_vgg.py: appended to the file TRASE_VGG_RECORD names, when it is set"""
    path = os.environ.get("TRASE_VGG_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": name, "share_of_bar": share}) + "\n")


# ---- the C ABI with canaries ------------------------------------------------------------------------------------------------
def _guarded(nbytes):
    """a byte buffer of nbytes + PAD, all 0xCD"""
    return torch.full((nbytes + PAD,), CANARY, dtype=torch.uint8, device=DEV)


def _intact(buf, nbytes):
    return bool((buf[nbytes:] == CANARY).all())


def _abi_run(pairs, k, img, cot=None, pack_layers=None):
    """forward (and, with a cotangent, backward) of the network cut at layer k through the C entry points, on a pack of
    pack_layers >= k layers; every output lives in front of a canary.
    -> (out (C, h, w), d_img (3, H, W) or None, saved bytes), all on the CPU"""
    from trase_amd import _lib
    from trase_amd.vgg import sizes
    lib = _lib.load()
    H, W = img.shape[-2:]
    kp = pack_layers or k
    pack_b = sizes(kp, H, W)[0]
    _, wsf_b, wsb_b, saved_b, c, h, w = sizes(k, H, W)
    ws_t = [t.to(DEV).contiguous() for t, _ in pairs[:kp]]
    bs_t = [t.to(DEV).contiguous() for _, t in pairs[:kp]]
    wp = (C.c_void_p * kp)(*[t.data_ptr() for t in ws_t])
    bp = (C.c_void_p * kp)(*[t.data_ptr() for t in bs_t])
    pack = _guarded(pack_b)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(lib.trase_vgg_pack(kp, wp, bp, _lib.ptr(pack), pack_b, 0, st), "trase_vgg_pack")
    x = img.to(DEV)
    x0 = x.clone()
    out, saved, d_img = _guarded(c * h * w * 4), _guarded(saved_b), _guarded(3 * H * W * 4)
    wsf, wsb = _guarded(wsf_b), _guarded(wsb_b)
    _lib.check(lib.trase_vgg_forward(k, _lib.ptr(pack), pack_b, _lib.ptr(x), H, W, None, None, _lib.ptr(out), _lib.ptr(saved), saved_b,
                                     _lib.ptr(wsf), wsf_b, 0, st), "trase_vgg_forward")
    if cot is not None:
        g = cot.to(DEV).contiguous()
        g0 = g.clone()
        _lib.check(lib.trase_vgg_backward(k, _lib.ptr(pack), pack_b, _lib.ptr(g), H, W, None, _lib.ptr(saved), saved_b, _lib.ptr(d_img),
                                          _lib.ptr(wsb), wsb_b, 0, st), "trase_vgg_backward")
    torch.cuda.synchronize()
    for name, buf, n in (("pack", pack, pack_b), ("out", out, c * h * w * 4), ("saved", saved, saved_b), ("d_image", d_img, 3 * H * W * 4),
                         ("ws forward", wsf, wsf_b), ("ws backward", wsb, wsb_b)):
        assert _intact(buf, n), f"{name}: written past its stated size"
    assert torch.equal(x, x0) and (cot is None or torch.equal(g, g0)), "an input was modified"
    return (out[:c * h * w * 4].view(torch.float32).view(c, h, w).cpu(),
            d_img[:3 * H * W * 4].view(torch.float32).view(3, H, W).cpu() if cot is not None else None, saved[:saved_b].cpu())


def _exact_case(k, dense, H, W):
    pairs, img, z, cot, g = R.lattice_case(k, dense, H, W)
    out_a, d_a, saved_a = _abi_run(pairs, k, img, cot)
    out_b, d_b, saved_b = _abi_run(pairs, k, img, cot)
    assert torch.equal(out_a.to(torch.int64), z) and torch.equal(out_a, z.float()), \
        f"forward: {int((out_a.double() != z.double()).sum())} of {z.numel()} differ"
    assert torch.equal(d_a.to(torch.int64), g) and torch.equal(d_a, g.float()), \
        f"backward: {int((d_a.double() != g.double()).sum())} of {g.numel()} differ"
    assert torch.equal(out_a, out_b) and torch.equal(d_a, d_b) and torch.equal(saved_a, saved_b), "two calls differ"


_LAYER_CASES = [(k, hw) for k in range(1, 9) for hw in R.exact_sizes(k)]


@pytest.mark.parametrize("k,hw", _LAYER_CASES, ids=[f"{R.KEYS[k - 1]}-{h}x{w}" for k, (h, w) in _LAYER_CASES])
def test_layer_exact_on_lattice(k, hw):
    """layer k with dense weights from {-2 .. 2} behind sparse layers 1 .. k - 1 (layer 1 is always dense), cut at k"""
    _exact_case(k, (k,), *hw)


@pytest.mark.parametrize("hw", R.exact_sizes(8), ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_stack_exact_on_lattice(hw):
    """the whole stack to conv4_1 with sparse weights: decisions are deterministic, pool ties included"""
    _exact_case(8, (), *hw)


def test_image_view_off_alignment():
    """an image whose base is 4 bytes off 16-byte alignment, through the Python interface"""
    from trase_amd.vgg import VGG16Features
    pairs, img, z, cot, g = R.lattice_case(8, (), 24, 40)
    flat = torch.zeros(img.numel() + 1, device=DEV)
    view = flat[1:].view(3, 24, 40)
    view.copy_(img)
    assert view.data_ptr() % 16 == 4
    view.requires_grad_(True)
    net = VGG16Features(pairs, "conv4_1", normalize=False, device=DEV)
    out = net(view)
    out.backward(cot.to(DEV)[None])
    assert torch.equal(out[0].cpu(), z.float()) and torch.equal(view.grad.cpu(), g.float())


# ---- real-valued ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nets():
    from trase_amd.vgg import VGG16Features, vgg16_random_weights
    pairs = vgg16_random_weights(1, "conv4_1")
    return pairs, [VGG16Features(pairs, key, device=DEV) for key in R.KEYS]


@functools.lru_cache(maxsize=None)
def _real_case(H, W):
    """(image, f64 outputs, emulated outputs, one-product outputs, device outputs of the eight truncations)"""
    pairs, nets = _nets()
    img = torch.rand(3, H, W, generator=torch.Generator().manual_seed(H * 1000 + W))
    zf = R.forward_f64(pairs, img)
    z3 = R.forward_emulated(pairs, img)
    z1 = R.forward_emulated(pairs, img, products=1)
    with torch.no_grad():
        zg = [net(img.to(DEV))[0].cpu() for net in nets]
    return img, zf, z3, z1, zg


@pytest.mark.parametrize("hw", REAL_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("k", range(1, 9), ids=lambda k: R.KEYS[k - 1])
def test_forward_within_the_emulations_margin(k, hw):
    img, zf, z3, z1, zg = _real_case(*hw)
    bar = MARGIN * R.rel_err(z3[k - 1], zf[k - 1])
    err, err1 = R.rel_err(zg[k - 1], zf[k - 1]), R.rel_err(z1[k - 1], zf[k - 1])
    print(f"{R.KEYS[k - 1]} {hw}: device {err:.3e}, bar {bar:.3e} (emulation {bar / MARGIN:.3e}), one-product emulation {err1:.3e}")
    _record(f"forward {R.KEYS[k - 1]} {hw[0]}x{hw[1]}", err / bar)
    assert err <= bar
    if k > 1:                   # conv1_1 is fp32: no matrix product there for a one-product variant to differ in
        assert err1 > bar, "the one-product bf16 emulation must miss the bar"


@pytest.mark.parametrize("hw", BWD_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("k", range(1, 9), ids=lambda k: R.KEYS[k - 1])
def test_backward_under_the_devices_decisions(k, hw):
    H, W = hw
    pairs, nets = _nets()
    img, zf, z3, z1, zg = _real_case(H, W)
    dec = R.with_shapes(R.decisions_from(zg[:k - 1]), H, W)          # the truncated forwards' bits are the full run's
    relu_flips, pool_flips = R.flip_shares(dec, R.decisions_from(zf[:k - 1]))
    cot = torch.randn(zg[k - 1].shape, generator=torch.Generator().manual_seed(7 + k))
    x = img.to(DEV).requires_grad_(True)
    out = nets[k - 1](x)
    assert torch.equal(out[0].cpu(), zg[k - 1])
    out.backward(cot.to(DEV)[None])
    gf = R.backward_f64(pairs[:k], cot, dec)
    bar = MARGIN * R.rel_err(R.backward_emulated(pairs[:k], cot, dec), gf)
    err, err1 = R.rel_err(x.grad.cpu(), gf), R.rel_err(R.backward_emulated(pairs[:k], cot, dec, products=1), gf)
    print(f"{R.KEYS[k - 1]} {hw}: device {err:.3e}, bar {bar:.3e}, one-product emulation {err1:.3e}; flips relu {relu_flips:.2e} "
          f"pool {pool_flips:.2e}")
    _record(f"backward {R.KEYS[k - 1]} {H}x{W}", err / bar)
    assert err <= bar
    if k > 1:
        assert err1 > bar
    assert relu_flips <= FLIP_CAP and pool_flips <= FLIP_CAP


def _saved_words(z, pooled):
    """the words csrc/vgg.hip keeps of a layer with pre-ReLU output z (C, H, W): uint16 [pixel][C / 16] of z > 0 bits, or, where a
    pool follows, uint64 [pooled pixel][C / 16] of 4-bit codes (window position | 4 * (maximum > 0)); channel c sits at bit /
    nibble 4 ((c >> 3) & 3) + (c & 3) of word 2 (c >> 5) + ((c >> 2) & 1).  As int64."""
    c = torch.arange(z.shape[0])
    word, pos = 2 * (c >> 5) + ((c >> 2) & 1), 4 * ((c >> 3) & 3) + (c & 3)
    if pooled:
        best, idx = R.pool_decide(torch.relu(z))
        v, step = idx + 4 * (best > 0).to(torch.int64), 4
    else:
        v, step = (z > 0).to(torch.int64), 1
    v = v.flatten(1).t() << (step * pos)[None]                      # (pixels, C)
    return torch.zeros(v.shape[0], z.shape[0] // 16, dtype=torch.int64).index_add_(1, word, v)


def test_truncations_are_the_deeper_cuts_layers():
    """a cut at k returns the bits layers 1 .. k of a deeper cut compute: the decisions the conv4_1 run keeps of layers 1 .. 7
    are, word for word, those of the seven truncations' outputs (all on one pack of eight layers); this also pins the saved
    format: 1 bit per convolution output, 4 bits per pooled unit"""
    pairs, _ = _nets()
    H, W = 67, 35
    img = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3))
    _, _, saved = _abi_run(pairs, 8, img)
    off = 0
    for l in range(1, 8):
        z, _, _ = _abi_run(pairs, l, img, pack_layers=8)
        words = _saved_words(z, l in R.POOL_AFTER)
        size = 8 if l in R.POOL_AFTER else 2
        got = saved[off:off + words.numel() * size].view(torch.int64 if size == 8 else torch.int16).to(torch.int64).view(words.shape)
        if size == 2:
            got = got & 0xFFFF
        assert torch.equal(got, words), R.KEYS[l - 1]
        off += (words.numel() * size + 255) // 256 * 256
    assert off == saved.numel()


# ---- interface --------------------------------------------------------------------------------------------------------------
def test_shim_equals_the_features_bit_for_bit(tmp_path, monkeypatch):
    from style_transfer.fx import VGG16FeatureExtractor
    from trase_amd.vgg import FEATURE_INDEX
    pairs, nets = _nets()
    sd = {}
    for idx, (w, b) in zip(FEATURE_INDEX, pairs):
        sd[f"features.{idx}.weight"], sd[f"features.{idx}.bias"] = w, b
    path = tmp_path / "vgg16.pt"
    torch.save(sd, path)
    monkeypatch.setenv("TRASE_VGG16_WEIGHTS", str(path))
    img = torch.rand(3, 40, 56, generator=torch.Generator().manual_seed(11)).to(DEV)
    ext = VGG16FeatureExtractor(["conv4_1"]).cuda().eval()
    x = img.clone().requires_grad_(True)
    d = ext(x)
    assert list(d.keys()) == ["conv4_1"] and d["conv4_1"].shape == (1, 512, 5, 7)
    y = img.clone().requires_grad_(True)
    ref = nets[7](y[None])
    assert torch.equal(d["conv4_1"], ref)
    cot = torch.randn(ref.shape, generator=torch.Generator().manual_seed(12)).to(DEV)
    d["conv4_1"].backward(cot)
    ref.backward(cot)
    assert x.grad.shape == (3, 40, 56) and y.grad.shape == (3, 40, 56) and torch.equal(x.grad, y.grad)
    assert not ext(img, detach=True)["conv4_1"].requires_grad
    ext2 = VGG16FeatureExtractor("conv2_1", weights=pairs).to(DEV)
    with torch.no_grad():
        assert torch.equal(ext2(img)["conv2_1"], nets[2](img))
    n = ext.normalize(img)
    mean, std = torch.tensor(R.MEAN, device=DEV).view(3, 1, 1), torch.tensor(R.STD, device=DEV).view(3, 1, 1)
    assert torch.allclose(n, (img - mean) / std, rtol=0, atol=1e-6)


def test_no_grad_keeps_nothing():
    pairs, nets = _nets()
    img = torch.rand(3, 64, 96, device=DEV)
    for x, ctx in ((img, torch.enable_grad()), (img.clone().requires_grad_(True), torch.no_grad())):
        with ctx:
            out = nets[7](x)
        assert out.grad_fn is None or not out.grad_fn.saved_tensors
        assert not out.requires_grad
    out = nets[7](img.clone().requires_grad_(True))
    assert out.requires_grad and len(out.grad_fn.saved_tensors) == 1


def test_weights_that_require_grad_are_detached_with_one_warning():
    import trase_amd.vgg as V
    pairs = [(w.clone().requires_grad_(True), b.clone().requires_grad_(True)) for w, b in V.vgg16_random_weights(2, "conv1_2")]
    V._WEIGHTS_WARNED = False
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        net = V.VGG16Features(pairs, "conv1_2", device=DEV)
        V.VGG16Features(pairs, "conv1_2", device=DEV)
    assert len([r for r in rec if "require grad" in str(r.message)]) == 1
    x = torch.rand(1, 3, 16, 16, device=DEV, requires_grad=True)
    net(x).sum().backward()
    assert x.grad is not None and all(w.grad is None and b.grad is None for w, b in pairs)


def test_repack_follows_a_weight_change():
    from trase_amd.vgg import VGG16Features, vgg16_random_weights
    pairs = vgg16_random_weights(3, "conv2_1", device=DEV)
    net = VGG16Features(pairs, "conv2_1")
    x = torch.rand(3, 24, 24, device=DEV)
    with torch.no_grad():
        a = net(x)
        pairs[2][0].mul_(2.0)
        pairs[2][1].mul_(2.0)
        assert torch.equal(net(x), a)                      # packed at construction
        net.repack()
        b = net(x)
    assert torch.equal(b, 2.0 * a)                          # the last layer is linear in its weights and bias; doubling is exact


def test_memory_of_a_forward_and_backward():
    from trase_amd.vgg import sizes
    pairs, nets = _nets()
    H, W = 256, 320
    _, wsf, wsb, saved, c, h, w = sizes(8, H, W)
    x = torch.rand(3, H, W, device=DEV, requires_grad=True)
    cot = torch.randn(1, c, h, w, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = nets[7](x)
    out.backward(cot)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    io = 4 * (c * h * w + 2 * 3 * H * W)                    # the output, the image's contiguous fp32 copy (none here) and its gradient
    slack = 6 << 20                                         # the caching allocator leaves a remainder under 1 MiB in a block: six blocks live
    print(f"peak {peak / 1e6:.1f} MB; workspace {max(wsf, wsb) / 1e6:.1f} MB, saved bits {saved / 1e6:.1f} MB, in/out {io / 1e6:.1f} MB")
    assert peak <= max(wsf, wsb) + saved + io + slack


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_style_transfer_iteration_on_the_real_topology():
    """tests/test_gpu_nnfm.py::test_style_transfer_iteration_config5_size with VGG16Features in place of the stand-in stack, at
    small size: rendered frame -> conv4_1 -> loss_nnfm_style -> backward -> masked colour gradients -> FusedAdam"""
    from gaussian_renderer import render
    from trase_amd.losses import loss_nnfm_style
    from trase_amd.optim import FusedAdam
    from trase_amd.synthetic import SynthGaussianModel, SynthPipe, make_scene, orbit_camera
    pairs, nets = _nets()
    net = nets[7]
    torch.manual_seed(0)
    n, w, h = 20_000, 240, 136
    pc = SynthGaussianModel(make_scene(n, feat_dim=32, seed=5, scale_mult=0.9).to(DEV))
    cam = orbit_camera(w, h, angle=1.1).to(DEV)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        style = net(torch.rand(3, h, w, device=DEV))[0]
    segmented = torch.rand(n, device=DEV) < 0.3
    opt = FusedAdam([{"params": [pc._features_dc], "lr": 0.0025, "name": "f_dc"},
                     {"params": [pc._features_rest], "lr": 0.0025 / 20.0, "name": "f_rest"}], lr=0.0, eps=1e-15)
    before = {k: getattr(pc, k).detach().clone() for k in ("_features_dc", "_xyz", "_opacity")}
    losses = []
    for it in range(3):
        image = render(cam, pc, SynthPipe(), bg, 0.0, 0.0, 0.0)["render"]
        feats = net(image)[0]
        loss = loss_nnfm_style(feats.reshape(512, -1), style.reshape(512, -1))
        assert torch.isfinite(loss)
        loss.backward()
        pc._features_dc.grad[~segmented] = 0
        pc._features_rest.grad[~segmented] = 0
        assert torch.isfinite(pc._features_dc.grad).all() and float(pc._features_dc.grad.abs().max()) > 0
        assert pc._xyz.grad is not None and torch.isfinite(pc._xyz.grad).all()
        opt.step()
        for p in pc.parameters():
            p.grad = None
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses
    assert torch.equal(pc._xyz.detach(), before["_xyz"]) and torch.equal(pc._opacity.detach(), before["_opacity"])
    moved = (pc._features_dc.detach() - before["_features_dc"]).abs().amax(dim=(1, 2)) > 0
    assert not bool(moved[~segmented].any()) and bool(moved[segmented].any())
