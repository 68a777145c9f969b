"""The FEATURE-state head on a feature image of another size than the SAM masks (trase_amd.feature_head.contrastive_head with
(Hr, Wr) != (h, w); the *_resized kernels of trase_amd/csrc/pairhead.hip).

The oracle is the pinned float64 head (oracle/feature_head_oracle.py) on ``resample64(features)`` -- the float64 bilinear blend
from ATen's fp32 coordinates of tests/feature_resample_reference.py -- with autograd through the blend giving the gradient of the
FULL-resolution features.  Bars: the project's own for this head (test_contrastive_head_large_matches_float64_oracle): losses
1e-5 relative, similarities 1e-6, gradient 1e-4 of its largest magnitude.  Every figure is printed before it is asserted.
Scenes and oracle results are computed once per (shape, mode) and shared.
"""
import os

import numpy as np
import pytest
import torch

from tests import feature_resample_reference as fr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RESIZE_BOUND = 8 * 2.0 ** -24
# render (Hr, Wr) -> masks (h, w): non-integral, x2 (weights exactly 0.5), x4, masks larger than the render, tiny
SMALL = [((67, 35), (33, 17)), ((64, 96), (32, 48)), ((64, 96), (16, 24)), ((48, 64), (80, 100)), ((5, 7), (3, 2))]
FULL = ((1080, 1920), (270, 480))

_scenes, _oracles = {}, {}


def _scene(src, dst, every=False):
    """(features (32, Hr, Wr), masks (N, h, w), sampled_pixel (h, w), sampled_mask (N,)) on the GPU.  ``every``: all h * w mask pixels
    are sampled (mask 0 then covers the whole frame and is not itself sampled, so both kinds of pair exist)."""
    key = (src, dst, every)
    if key not in _scenes:
        (Hr, Wr), (h, w) = src, dst
        g = torch.Generator(device="cuda").manual_seed(Hr * 1000 + w + (7 if every else 0))
        N = 3 if h * w < 16 else (90 if h * w > 50_000 else 14)
        yy, xx = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
        cy, cx = torch.randint(0, h, (N,), device="cuda", generator=g), torch.randint(0, w, (N,), device="cuda", generator=g)
        ry = torch.randint(max(1, h // 10), max(2, h // 3), (N,), device="cuda", generator=g)
        rx = torch.randint(max(1, w // 10), max(2, w // 3), (N,), device="cuda", generator=g)
        sam = ((yy[None] - cy[:, None, None]).abs() <= ry[:, None, None]) & ((xx[None] - cx[:, None, None]).abs() <= rx[:, None, None])
        sm = torch.rand(N, device="cuda", generator=g) < 0.5
        sm[1] = True
        if every:
            sam[0] = True
            sm[0] = False
        base = torch.randn(N, 32, device="cuda", generator=g)
        big = torch.nn.functional.interpolate(sam.float()[None], size=(Hr, Wr), mode="nearest")[0]
        feat = (big.permute(1, 2, 0) @ base).permute(2, 0, 1) * 0.5 + 0.8 * torch.randn(32, Hr, Wr, device="cuda", generator=g)
        if every:
            sp = torch.ones(h, w, dtype=torch.bool, device="cuda")
        else:
            target = 3000 if h * w > 50_000 else min(400, max(4, h * w // 3))
            sp = (torch.rand(h, w, device="cuda", generator=g) < target / (h * w)) & (sam.sum(dim=0) != 0)
        assert int(sp.sum()) >= 2
        _scenes[key] = (feat, sam, sp, sm)
    return _scenes[key]


def _oracle(src, dst, mode, every=False):
    """float64: (loss_pos, loss_neg, pos_similarity, neg_similarity, d(loss_pos + 0.5 loss_neg) / d features)."""
    key = (src, dst, mode, every)
    if key not in _oracles:
        from oracle import feature_head_oracle as O
        feat, sam, sp, sm = _scene(src, dst, every)
        fa = feat.double().requires_grad_(True)
        rp, rn, rps, rns = O.head(fr.resample64(fa, dst), sam, sp, sm, mode, 0.75, 0.5, True, dtype=torch.float64)
        grad, = torch.autograd.grad(rp + 0.5 * rn, fa)
        _oracles[key] = (float(rp.detach()), float(rn.detach()), float(rps), float(rns), grad)
    return _oracles[key]


def _run(feat, sam, sp, sm, mode, **kw):
    """(loss_pos, loss_neg, pos_similarity, neg_similarity[, reg], gradient of loss_pos + 0.5 loss_neg [+ 0.3 reg])."""
    from trase_amd.feature_head import contrastive_head
    f = feat.clone().requires_grad_(True)
    out = contrastive_head(f, sam, sp, sm, mode, 0.75, 0.5, **kw)
    loss = out[0] + 0.5 * out[1] + (0.3 * out[4] if len(out) == 5 else 0.0)
    grad, = torch.autograd.grad(loss, f)
    return tuple(o.detach() for o in out) + (grad,)


def _same(a, b):
    """bitwise, NaN equal to NaN"""
    return torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))


def _check_against_oracle(src, dst, mode, every=False):
    feat, sam, sp, sm = _scene(src, dst, every)
    rp, rn, rps, rns, rgrad = _oracle(src, dst, mode, every)
    lp, ln, ps, ns, grad = _run(feat, sam, sp, sm, mode)
    gmax = float(rgrad.abs().max())
    gerr = float((grad.double() - rgrad).abs().max())
    print(f"{src}->{dst} {mode} S={int(sp.sum())}: loss_pos {float(lp):.7g} / {rp:.7g}, loss_neg {float(ln):.7g} / {rn:.7g}, "
          f"sims {float(ps):.7g} / {rps:.7g}, {float(ns):.7g} / {rns:.7g}, gradient error {gerr:.3e} of max {gmax:.3e}")
    assert grad.shape == feat.shape
    assert abs(float(lp) - rp) <= 1e-5 * abs(rp) and abs(float(ln) - rn) <= 1e-5 * abs(rn)
    for got, want in ((float(ps), rps), (float(ns), rns)):
        assert (np.isnan(got) and np.isnan(want)) or abs(got - want) < 1e-6
    assert gerr <= 1e-4 * gmax
    assert bool(torch.isfinite(grad).all())


@pytest.mark.parametrize("mode", ["soft", "all", "hard"])
@pytest.mark.parametrize("src,dst", SMALL, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SMALL])
def test_resized_head_matches_float64_oracle(src, dst, mode):
    _check_against_oracle(src, dst, mode)


def test_resized_head_full_size_matches_float64_oracle():
    """1080p render, masks of --downsample_mask 4, ~3000 samples, 90 masks (two membership words)."""
    _check_against_oracle(*FULL, "soft")


@pytest.mark.parametrize("src,dst", [((48, 64), (80, 100)), ((67, 35), (33, 17))], ids=["up", "down"])
def test_every_mask_pixel_sampled(src, dst):
    """The worst collision: S = h * w, so every tap of every source pixel carries a gradient -- at 48 x 64 -> 80 x 100 a source
    pixel gathers from up to sixteen mask pixels, and the last row and column take both weights of the clamped axis."""
    _check_against_oracle(src, dst, "soft", every=True)


@pytest.mark.parametrize("src,dst", SMALL + [((1014, 1352), (253, 338))])
def test_resized_columns_equal_interpolate(src, dst):
    from trase_amd.feature_head import resized_columns
    feat, _, sp, _ = _scene(*(FULL if src[0] > 1000 else (src, dst)))
    if src[0] > 1000:                                       # an odd frame cut out of the full-size scene: 1014 // 4 = 253
        feat, sp = feat[:, :src[0], :src[1]], sp[:dst[0], :dst[1]]
    want = torch.nn.functional.interpolate(feat[None], size=dst, mode="bilinear", align_corners=False)[0][:, sp].T
    got = resized_columns(feat, dst, sp)
    err, scale = float((got - want).abs().max()), float(feat.abs().max())
    print(f"{src}->{dst}: {err / scale:.3e} of max|v| (bound {RESIZE_BOUND:.3e})")
    assert got.shape == want.shape and got.dtype == torch.float32
    assert err <= RESIZE_BOUND * scale
    same = torch.rand(*src, device="cuda") < 0.2
    assert torch.equal(resized_columns(feat, src, same), feat[:, same].T)               # equal sizes: plain indexing
    assert resized_columns(feat, dst, torch.zeros_like(sp)).shape == (0, 32)


@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_equal_sizes_run_the_existing_kernels_bit_for_bit(mode):
    """With equal sizes ``contrastive_head`` is the existing path; and the resized kernels, forced onto the same input, reproduce
    it bit for bit: the weights are exactly 1 and 0, so a blend is its first tap and a pixel's gathered sum is its own sample."""
    from trase_amd import feature_head as FH
    d = np.load(os.path.join(HERE, "golden", "feature_head.npz"))
    sam = torch.from_numpy(d["sam_masks"]).cuda()
    sp, sm = torch.from_numpy(d["sampled_pixel"]).cuda(), torch.from_numpy(d["sampled_mask"]).cuda()
    feat = torch.from_numpy(d["features"]).cuda()
    a = _run(feat, sam, sp, sm, mode)
    assert abs(float(a[0]) - float(d[f"{mode}_loss_pos"])) < 2e-6 and abs(float(a[1]) - float(d[f"{mode}_loss_neg"])) < 2e-6
    _, size = FH.mask_stats(sam)
    pix = torch.nonzero(sp.reshape(-1)).reshape(-1).to(torch.int32)
    for with_reg in (False, True):
        a = _run(feat, sam, sp, sm, mode, with_norm_reg=with_reg)
        f = feat.clone().requires_grad_(True)
        res = FH._PairHead.apply(f, FH._masks_u8(sam), sm.view(torch.uint8), sam.shape[0], size, pix, FH._MODES[mode], 0.75, 0.5, 1,
                                 with_reg, None, True)
        loss = res[0] + 0.5 * res[1] + (0.3 * res[3] if with_reg else 0.0)
        grad, = torch.autograd.grad(loss, f)
        b = (res[0].detach(), res[1].detach(), res[2][0], res[2][1]) + ((res[3].detach(),) if with_reg else ()) + (grad,)
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert _same(x, y)


@pytest.mark.parametrize("mode", ["soft", "all", "hard"])
def test_resized_head_matches_reference_golden(mode):
    """The reference's own composition (tests/golden/feature_resized.npz: the regulariser, ``interpolate``, the helpers of
    utils/feature_utils.py, the pair losses) at the tolerances of test_contrastive_head_matches_reference_golden."""
    from trase_amd.feature_head import contrastive_head
    d = np.load(os.path.join(HERE, "golden", "feature_resized.npz"))
    sam = torch.from_numpy(d["sam_masks"]).cuda()
    sp, sm = torch.from_numpy(d["sampled_pixel"]).cuda(), torch.from_numpy(d["sampled_mask"]).cuda()
    f = torch.from_numpy(d["features"]).cuda().requires_grad_(True)
    assert tuple(f.shape[1:]) != tuple(sam.shape[1:])
    lp, ln, ps, ns, reg = contrastive_head(f, sam, sp, sm, mode, float(d["positive_th"]), float(d["negative_th"]), True, with_norm_reg=True)
    print(mode, float(lp.detach()), float(d[f"{mode}_loss_pos"]), float(ln.detach()), float(d[f"{mode}_loss_neg"]), float(ps), float(ns),
          float(reg.detach()))
    assert abs(float(lp.detach()) - float(d[f"{mode}_loss_pos"])) < 2e-6
    assert abs(float(ln.detach()) - float(d[f"{mode}_loss_neg"])) < 2e-6
    assert abs(float(ps) - float(d["pos_similarity"])) < 2e-6 and abs(float(ns) - float(d["neg_similarity"])) < 2e-6
    assert abs(float(reg.detach()) - float(d["reg"])) < 1e-5 * float(d["reg"])
    if mode == "soft":
        (lp + ln).backward()
        want = torch.from_numpy(d["soft_grad"]).cuda()
        err = float((f.grad - want).abs().max())
        print("gradient error", err, "of", float(want.abs().max()))
        assert err < 1e-5 * float(want.abs().max())
        assert torch.equal(f.grad == 0, want == 0)                                       # the same support


def test_norm_reg_is_taken_at_render_resolution_and_shares_the_dense_pass():
    from trase_amd.feature_head import feature_norm_reg
    src, dst = SMALL[0]
    feat, sam, sp, sm = _scene(src, dst)
    alone = _run(feat, sam, sp, sm, "soft")
    both = _run(feat, sam, sp, sm, "soft", with_norm_reg=True)
    fd = feat.clone().requires_grad_(True)
    r = feature_norm_reg(fd)
    rgrad, = torch.autograd.grad(0.3 * r, fd)
    assert torch.equal(both[4], r.detach())
    for k in range(4):
        assert _same(both[k], alone[k])
    err = float((both[5] - (alone[4] + rgrad)).abs().max())
    print("combined - (head + regulariser):", err, "of", float(both[5].abs().max()))
    assert err <= 1e-6 * float(both[5].abs().max()) + 1e-12
    away = ~((alone[4] != 0).any(dim=0))                     # pixels no sampled tap touches: the regulariser's own bits
    assert bool(away.any()) and torch.equal(both[5][:, away], rgrad[:, away])


def test_sync_free_draw_equals_the_plain_boolean_mask():
    from trase_amd import feature_head as FH
    feat, sam, _, _ = _scene(*FULL)
    cover, size = FH.mask_stats(sam)
    sp, sm = FH.get_sample_pixel_and_mask(sam, 3000, 45, cover_count=cover, rng="cuda")
    assert getattr(sp, "_trase_expected_count", None) is not None and 500 < int(sp.sum()) < 4000
    a = _run(feat, sam, sp, sm, "soft", mask_size=size, with_norm_reg=True)
    plain = sp.clone()
    assert getattr(plain, "_trase_expected_count", None) is None
    b = _run(feat, sam, plain, sm, "soft", mask_size=size, with_norm_reg=True)
    FH.check_sampled_counts()
    for x, y in zip(a, b):
        assert _same(x, y)


def test_two_runs_are_bitwise_identical():
    for src, dst, every in ((FULL[0], FULL[1], False), ((48, 64), (80, 100), True)):
        feat, sam, sp, sm = _scene(src, dst, every)
        a = _run(feat, sam, sp, sm, "soft", with_norm_reg=True)
        b = _run(feat, sam, sp, sm, "soft", with_norm_reg=True)
        for x, y in zip(a, b):
            assert _same(x, y)


def test_forward_and_backward_replay_from_one_graph():
    """One capture of forward + backward (sync-free draw, so nothing is read back), replayed twice: both equal the eager result
    bit for bit -- no memset node, and nothing of the gradient is left over from the replay before."""
    from trase_amd.bench_iterations import capture_iteration
    from trase_amd.feature_head import contrastive_head
    src, dst = SMALL[0]
    feat, sam, sp, sm = _scene(src, dst)
    f = feat.clone().requires_grad_(True)
    count = int(sp.sum())

    def step(_):
        spx = sp.clone()
        spx._trase_expected_count = (count, spx.numel(), spx._version)         # the sampler's tag: (target, pixels, version)
        lp, ln, ps, ns, reg = contrastive_head(f, sam, spx, sm, "soft", 0.75, 0.5, with_norm_reg=True)
        grad, = torch.autograd.grad(lp + 0.5 * ln + 0.3 * reg, f)
        return lp.detach(), ln.detach(), ps, ns, reg.detach(), grad

    eager = tuple(t.clone() for t in step(0))
    torch.cuda.synchronize()
    graph, out = capture_iteration(step, warm=2)
    for _ in range(2):
        for t in out:
            t.fill_(float("nan"))                            # whatever the replay does not write would stay NaN
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(out, eager):
            assert torch.equal(x, y)
    from trase_amd import feature_head as FH
    FH.check_sampled_counts()


def test_degenerate_inputs():
    from trase_amd.feature_head import contrastive_head
    src, dst = SMALL[0]
    feat, sam, sp, sm = _scene(src, dst)
    f = feat.clone().requires_grad_(True)
    none = torch.zeros_like(sp)
    lp, ln, ps, ns = contrastive_head(f, sam, none, sm)
    assert float(lp.detach()) == 0.0 and float(ln.detach()) == 0.0 and bool(torch.isnan(ps)) and bool(torch.isnan(ns))
    g, = torch.autograd.grad(lp + ln, f)
    assert g.shape == f.shape and float(g.abs().max()) == 0.0
    tagged = none.clone()                                    # the sync-free form of the same: the kernels see a device count of 0
    tagged._trase_expected_count = (50, tagged.numel(), tagged._version)
    lp, ln, ps, ns, reg = contrastive_head(f, sam, tagged, sm, with_norm_reg=True)
    g, = torch.autograd.grad(lp + ln, f)
    assert float(lp.detach()) == 0.0 and bool(torch.isnan(ps)) and float(g.abs().max()) == 0.0 and bool(torch.isfinite(reg))
    one = none.clone()
    one[dst[0] - 1, dst[1] - 1] = True
    lp, ln, ps, ns = contrastive_head(f, sam, one, sm)
    g, = torch.autograd.grad(lp + ln, f)
    assert float(lp.detach()) == 0.0 and float(ln.detach()) == 0.0 and float(g.abs().max()) == 0.0
    # a sampled pixel whose four taps are all-zero columns (F.normalize's eps clamp): finite losses and gradient
    ys, xs = torch.nonzero(sp)[0].tolist()
    y0, y1, _, _ = fr.axis_table(src[0], dst[0])
    x0, x1, _, _ = fr.axis_table(src[1], dst[1])
    fz = feat.clone()
    for yy in (int(y0[ys]), int(y1[ys])):
        for xx in (int(x0[xs]), int(x1[xs])):
            fz[:, yy, xx] = 0.0
    fz.requires_grad_(True)
    lp, ln, _, _ = contrastive_head(fz, sam, sp, sm)
    g, = torch.autograd.grad(lp + ln, fz)
    assert bool(torch.isfinite(lp.detach())) and bool(torch.isfinite(ln.detach())) and bool(torch.isfinite(g).all())
    # a non-contiguous view gives what its contiguous copy gives
    wide = torch.zeros(32, src[0], 2 * src[1], device="cuda")
    wide[:, :, ::2] = feat
    wide.requires_grad_(True)
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    a = contrastive_head(view, sam, sp, sm, "soft", 0.75, 0.5)
    ga, = torch.autograd.grad(a[0] + 0.5 * a[1], wide)
    b = _run(feat, sam, sp, sm, "soft")
    for x, y in zip(a, b[:4]):
        assert _same(x.detach(), y)
    assert torch.equal(ga[:, :, ::2], b[4]) and float(ga[:, :, 1::2].abs().max()) == 0.0
    # features that do not require grad: the forward alone
    c = contrastive_head(feat, sam, sp, sm, "soft", 0.75, 0.5)
    assert not c[0].requires_grad
    for x, y in zip(c, b[:4]):
        assert _same(x, y)
    # the checks that stay: channel count, the 256 membership bits, devices
    with pytest.raises(ValueError):
        contrastive_head(feat[:16], sam, sp, sm)
    many = torch.rand(300, *dst, device="cuda") < 0.5
    with pytest.raises(ValueError):
        contrastive_head(feat, many, sp, torch.ones(300, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError):
        contrastive_head(feat.cpu(), sam, sp, sm)
