"""The photometric loss kernels (trase_amd/csrc/loss.hip: ssim_fwd_kernel, loss_reduce_kernel, ssim_bwd_kernel) against the
float64 evaluation of tests/photometric_reference.py at the edges of their 32x32 tiles, their 11-tap halo and the
8 x 256 stride of the reduction, through every entry point of trase_amd.losses and every cotangent.

Comparison: always per pixel (max-abs).  A failure names the worst pixel and where it sits in its tile.

Tolerance: none is fixed in advance.  Every case also evaluates the reference module in float32 on the CPU -- the
reference project's own composition of five 11x11 convolutions -- and measures ITS distance to float64: for the two scalars,
and as the largest per-pixel distance of the gradient.  The kernel's bar is

    MARGIN * (float32 composition's error)  +  FLOOR_ULPS * 2^-23 * scale

MARGIN = 4: the kernel applies the window separably and with fmaf, the same 121 products summed in another order, so it
belongs to the class of the float32 composition, not ten times above it.  FLOOR_ULPS = 4 covers what stays when the
composition's error happens to vanish: the kernel rounds 1 / (C H W) to float32 once (half an ulp on every output), rounds
each scalar once more, sums up to 1024 terms per block in float32 before the double-precision reduction, and forms the
gradient from three products and two sums.  scale: for l1 the largest |pixel| of the pair, for ssim 1, for the gradient the
largest |float64 gradient| of the case -- for the "identical" kind, whose float64 gradient is zero, that of the "random"
case of the same shape.  No number below is derived from the kernel's output.

Measured (`l1`, `ssim` absolute, `grad` as a fraction of the gradient's scale, cotangents (0.8, -0.2); `f32` is the float32
composition on the CPU, `hip` the kernel on an MI355X; every test prints its figures as
`LOSSEDGE <case> <quantity> f32=... hip=... bar=...` before it asserts; margin 4 throughout):

    case                     l1 f32   l1 hip    ssim f32 ssim hip  grad f32 grad hip  margin
    3x1x1-random             1.5e-08  0.0e+00   1.6e-08  4.3e-08   3.4e-08  4.0e-08   4
    1x5x7-random             7.7e-09  2.1e-10   2.9e-08  3.0e-08   1.8e-07  1.5e-07   4
    3x10x11-random           3.2e-09  3.2e-09   3.5e-08  2.4e-08   5.4e-07  3.1e-07   4
    3x32x32-random           8.3e-09  8.3e-10   3.9e-08  2.1e-08   8.2e-07  4.8e-07   4
    1x64x31-random           1.3e-09  6.2e-09   4.8e-09  1.1e-07   1.0e-06  4.6e-07   4
    3x33x65-random           2.8e-09  2.8e-09   1.5e-07  8.5e-08   8.1e-07  5.7e-07   4
    4x64x96-random           5.8e-09  1.7e-09   7.1e-08  1.1e-08   1.1e-06  5.1e-07   4
    8x32x1024-random         3.0e-09  3.0e-09   5.1e-08  6.8e-08   1.4e-06  7.0e-07   4
    3x96x960-random          5.8e-09  1.6e-09   3.0e-08  8.9e-08   1.0e-06  6.1e-07   4
    8x1x8352-random          2.0e-09  2.0e-09   2.7e-08  3.2e-08   1.6e-07  2.0e-07   4
    3x40x40-random           1.0e-08  4.4e-09   8.1e-08  3.8e-08   9.0e-07  6.4e-07   4
    3x33x65-identical        0.0e+00  0.0e+00   0.0e+00  6.0e-08   2.8e-07  2.0e-07   4
    3x33x65-flat_bright      2.1e-11  2.1e-11   2.1e-04  5.1e-07   4.6e-04  2.4e-04   4
    3x33x65-zero_patch       1.3e-09  6.1e-09   5.0e-08  6.9e-08   9.8e-07  5.7e-07   4
    3x33x65-out_of_range     1.1e-08  1.1e-08   5.0e-08  6.9e-08   4.3e-07  3.0e-07   4
    3x33x65-impulses         5.3e-12  5.3e-12   1.1e-07  1.3e-07   9.9e-08  8.6e-08   4
    3x40x40-identical        0.0e+00  0.0e+00   0.0e+00  0.0e+00   2.1e-07  2.1e-07   4
    3x40x40-flat_bright      9.5e-11  2.2e-11   2.0e-04  3.7e-07   4.8e-04  2.3e-04   4
    3x40x40-zero_patch       3.1e-09  4.4e-09   5.8e-08  1.4e-09   8.7e-07  5.3e-07   4
    3x40x40-out_of_range     4.2e-08  1.8e-08   6.2e-08  2.4e-09   4.3e-07  2.9e-07   4
    3x40x40-impulses         5.6e-11  5.6e-11   6.3e-08  6.3e-08   1.2e-07  1.5e-07   4
"""
import functools

import pytest
import torch

from tests import photometric_reference as pr

pytestmark = pytest.mark.gpu

MARGIN = 4.0
MARGINS = {}                     # (shape, kind) -> a larger margin, with the reason from loss.hip: none needed
FLOOR_ULPS = 4.0
ULP = 2.0 ** -23
TILE = 32

SHAPES = [
    (3, 1, 1),          # far below the window
    (1, 5, 7),          # both axes below the window
    (3, 10, 11),        # one axis one short of the window
    (3, 32, 32),        # exactly one tile
    (1, 64, 31),        # a multiple of 32 against one short of 32
    (3, 33, 65),        # one-pixel last tile on both axes
    (4, 64, 96),        # exact tiles, C = 4
    (8, 32, 1024),      # nblocks = 256 exactly
    (3, 96, 960),       # nblocks = 270: masked rows of the eight-wide unroll
    (8, 1, 8352),       # nblocks = 2088: second trip of the reduce loop
]
KIND_SHAPES = [(3, 33, 65), (3, 40, 40)]
KINDS = ("random", "identical", "flat_bright", "zero_patch", "out_of_range", "impulses")
CASES = [(s, "random") for s in SHAPES + [(3, 40, 40)]] + [(s, k) for s in KIND_SHAPES for k in KINDS[1:]]
COTANGENTS = [(0.8, -0.2), (1.0, 0.0), (0.0, 1.0), (-3.0, 2.5)]
_ids = lambda case: "x".join(map(str, case[0])) + "-" + case[1]


def make_inputs(shape, kind):
    """-> (x, y) float32 CPU tensors from a generator seeded by the shape."""
    c, h, w = shape
    g = torch.Generator().manual_seed(1000 * c + 31 * h + w)
    x = torch.rand(c, h, w, generator=g)
    y = (x + 0.15 * torch.randn(c, h, w, generator=g)).clamp(0, 1)
    if kind == "random":
        pass
    elif kind == "identical":
        y = x.clone()
    elif kind == "flat_bright":                 # cancellation of E[x^2] - mu^2 against C2 = 9e-4
        x = 0.999 + 1e-4 * (2 * torch.rand(c, h, w, generator=g) - 1)
        y = 0.998 + 1e-4 * (2 * torch.rand(c, h, w, generator=g) - 1)
    elif kind == "zero_patch":                  # exact zeros of x - y across a tile corner: sign(0) = 0
        y[:, 28:min(h, 36), 27:min(w, 35)] = x[:, 28:min(h, 36), 27:min(w, 35)]
        y[0, 0, :5] = x[0, 0, :5]
    elif kind == "out_of_range":
        x, y = 4 * x, 4 * y
    elif kind == "impulses":                    # any halo offset shows up as a shifted blur
        x, y = torch.zeros(c, h, w), torch.zeros(c, h, w)
        for py, px in ((0, 0), (31, 31), (32, 32), (h - 1, w - 1)):
            if py < h and px < w:
                x[:, py, px] = 1.0
    else:
        raise KeyError(kind)
    return x.float().contiguous(), y.float().contiguous()


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    """The case evaluated once at float64 and once at float32 on the CPU; shared by every test, never modified."""
    x, y = make_inputs(shape, kind)
    l1, ss, d_l1, d_ss = pr.evaluate(x, y, torch.float64)
    l1_32, ss_32, d_l1_32, d_ss_32 = pr.evaluate(x, y, torch.float32)
    return dict(x=x, y=y, l1=l1, ss=ss, d_l1=d_l1, d_ss=d_ss, l1_32=l1_32, ss_32=ss_32, d_l1_32=d_l1_32, d_ss_32=d_ss_32,
                l1_scale=float(max(x.abs().max(), y.abs().max())))


def _grads(ref, g_l1, g_ss):
    """(float64 gradient, float32 composition's gradient) for a pair of cotangents: both heads are linear in theirs."""
    return g_l1 * ref["d_l1"] + g_ss * ref["d_ss"], g_l1 * ref["d_l1_32"] + g_ss * ref["d_ss_32"]


def _grad_scale(case, ref, g_l1, g_ss):
    shape, kind = case
    if kind == "identical":
        ref = reference(shape, "random")
    return float(_grads(ref, g_l1, g_ss)[0].abs().max())


def _margin(case):
    return MARGINS.get(case, MARGIN)


def _check_scalar(case, what, got, want, want32, scale):
    err32, err = abs(want32 - want), abs(float(got) - want)
    bar = _margin(case) * err32 + FLOOR_ULPS * ULP * scale
    print(f"LOSSEDGE {_ids(case)} {what} f32={err32:.3e} hip={err:.3e} bar={bar:.3e} scale={scale:.3e}")
    assert err <= bar, (case, what, f"kernel {float(got)!r}, float64 {want!r}: off by {err:.3e}, bar {bar:.3e} "
                        f"(float32 composition off by {err32:.3e})")


def _check_grad(case, what, got, want, want32, scale):
    got = got.detach().cpu().double()
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), (case, what)
    err32 = float((want32 - want).abs().max())
    diff = (got - want).abs()
    err = float(diff.max())
    bar = _margin(case) * err32 + FLOOR_ULPS * ULP * scale
    rel = lambda v: v / scale if scale > 0 else v
    print(f"LOSSEDGE {_ids(case)} {what} f32={rel(err32):.3e} hip={rel(err):.3e} bar={rel(bar):.3e} scale={scale:.3e}")
    if err > bar:
        h, w = want.shape[1:]
        i = int(diff.argmax())
        c, y, x = i // (h * w), (i // w) % h, i % w
        raise AssertionError(f"{case} {what}: worst pixel (c, y, x) = ({c}, {y}, {x}), row {y % TILE} column {x % TILE} of tile "
                             f"({y // TILE}, {x // TILE}): kernel {float(got[c, y, x])!r}, float64 {float(want[c, y, x])!r}; "
                             f"off by {err:.3e}, bar {bar:.3e} = {_margin(case)} x {err32:.3e} + {FLOOR_ULPS} ulp of {scale:.3e}")


def _device_pair(ref):
    dev = torch.device("cuda", 0)
    return ref["x"].clone().to(dev), ref["y"].clone().to(dev)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_l1_ssim_matches_float64_for_every_cotangent(case):
    from trase_amd.losses import l1_ssim
    ref = reference(*case)
    x, y = _device_pair(ref)
    for g_l1, g_ss in COTANGENTS:
        xa = x.clone().requires_grad_(True)
        l1, ss = l1_ssim(xa, y)
        torch.autograd.backward([l1, ss], [torch.tensor(g_l1, device=x.device), torch.tensor(g_ss, device=x.device)])
        tag = f"[{g_l1:g},{g_ss:g}]"
        if (g_l1, g_ss) == COTANGENTS[0]:
            _check_scalar(case, "l1", l1.detach(), ref["l1"], ref["l1_32"], ref["l1_scale"])
            _check_scalar(case, "ssim", ss.detach(), ref["ss"], ref["ss_32"], 1.0)
            first = (l1.detach().clone(), ss.detach().clone())
        else:
            assert torch.equal(l1.detach(), first[0]) and torch.equal(ss.detach(), first[1])     # deterministic reductions
        want, want32 = _grads(ref, g_l1, g_ss)
        _check_grad(case, "grad" + tag, xa.grad, want, want32, _grad_scale(case, ref, g_l1, g_ss))
    if case[1] == "identical":
        assert float(l1.detach()) == 0.0
    if case[1] == "zero_patch":                 # sign(0) = 0: with the ssim head switched off the patch has no gradient at all
        xa = x.clone().requires_grad_(True)
        l1_ssim(xa, y)[0].backward()
        assert float(xa.grad[x == y].abs().max()) == 0.0 and int((x == y).sum()) >= 5


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_l1_loss_alone_backpropagates_without_an_ssim_cotangent(case):
    """Only l1_loss is used, so the backward receives g_ssim = None."""
    from trase_amd.losses import l1_loss
    ref = reference(*case)
    x, y = _device_pair(ref)
    xa = x.clone().requires_grad_(True)
    l1 = l1_loss(xa, y)
    (l1 * 2.0).backward()
    _check_scalar(case, "l1_loss", l1.detach(), ref["l1"], ref["l1_32"], ref["l1_scale"])
    want, want32 = _grads(ref, 2.0, 0.0)
    _check_grad(case, "grad[l1_loss]", xa.grad, want, want32, _grad_scale(case, ref, 2.0, 0.0))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_photometric_loss_matches_float64_and_the_composition_bit_for_bit(case):
    """train.py:235-238 for lambda in {0, 0.2, 1} under an upstream factor of 3: the scalar and the gradient against float64,
    and both bit-identical to the same combination formed with tensor arithmetic around l1_ssim."""
    from trase_amd.losses import l1_ssim, photometric_loss
    ref = reference(*case)
    x, y = _device_pair(ref)
    up = 3.0
    for lam in (0.0, 0.2, 1.0):
        xa = x.clone().requires_grad_(True)
        la, sa = l1_ssim(xa, y)
        ta = (1.0 - lam) * la + lam * (1.0 - sa)
        (ta * up).backward()
        xb = x.clone().requires_grad_(True)
        tb, l1, ss = photometric_loss(xb, y, lam, with_parts=True)
        (tb * up).backward()
        assert torch.equal(ta.detach(), tb.detach()), (case, lam, float(ta), float(tb))
        assert torch.equal(l1, la.detach()) and torch.equal(ss, sa.detach()), (case, lam)
        assert torch.equal(xa.grad, xb.grad), (case, lam, float((xa.grad - xb.grad).abs().max()))
        want_t = (1.0 - lam) * ref["l1"] + lam * (1.0 - ref["ss"])
        f32 = lambda v: torch.tensor(v, dtype=torch.float32)
        want_t32 = float((1.0 - lam) * f32(ref["l1_32"]) + lam * (1.0 - f32(ref["ss_32"])))
        _check_scalar(case, f"total[{lam:g}]", tb.detach(), want_t, want_t32, (1.0 - lam) * ref["l1_scale"] + lam)
        g_l1, g_ss = up * (1.0 - lam), -up * lam
        want, want32 = _grads(ref, g_l1, g_ss)
        _check_grad(case, f"grad[photometric {lam:g}]", xb.grad, want, want32, _grad_scale(case, ref, g_l1, g_ss))


def test_wrappers_accept_strided_and_float64_ground_truth():
    """A permuted HWC ground truth and a float64 one give the bits of their contiguous float32 copies."""
    from trase_amd.losses import l1_ssim, photometric_loss
    ref = reference((3, 33, 65), "random")
    x, y = _device_pair(ref)
    y_hwc = y.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert not y_hwc.is_contiguous() and torch.equal(y_hwc, y)
    out = []
    for gt in (y, y_hwc, y.double()):
        xa = x.clone().requires_grad_(True)
        l1, ss = l1_ssim(xa, gt)
        (0.8 * l1 - 0.2 * ss).backward()
        xb = x.clone().requires_grad_(True)
        t = photometric_loss(xb, gt, 0.2)
        t.backward()
        out.append((l1.detach(), ss.detach(), xa.grad, t.detach(), xb.grad))
        assert l1.dtype == ss.dtype == t.dtype == xa.grad.dtype == torch.float32
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert torch.equal(a, b)


def test_wrappers_refuse_mismatched_shapes_and_batches():
    from trase_amd.losses import l1_loss, l1_ssim, photometric_loss, ssim
    dev = torch.device("cuda", 0)
    x = torch.rand(3, 12, 16, device=dev)
    for fn in (l1_ssim, photometric_loss, l1_loss, ssim):
        with pytest.raises(ValueError):
            fn(x, torch.rand(3, 12, 17, device=dev))
        with pytest.raises(ValueError):
            fn(x, torch.rand(1, 12, 16, device=dev))
        with pytest.raises(ValueError):
            fn(x[None], x[None])


@pytest.mark.parametrize("requires_grad", [False, True])
def test_shared_evaluation_follows_in_place_edits(requires_grad):
    """l1_loss and ssim share one evaluation for the same tensor objects at the same version counters -- and only then."""
    from trase_amd import losses
    ref = reference((3, 33, 65), "random")
    x, y = _device_pair(ref)
    x.requires_grad_(requires_grad)
    l1 = losses.l1_loss(x, y)
    val = losses._last["val"]
    ss = losses.ssim(x, y)
    assert losses._last["val"] is val and l1 is val[0] and ss is val[1]            # one launch served both
    _check_scalar(((3, 33, 65), "random"), "ssim[shared]", ss.detach(), ref["ss"], ref["ss_32"], 1.0)
    # the ground truth edited in place between the two calls: the ssim is that of the edited image
    y2 = y.clone()
    losses.l1_loss(x, y2)
    val = losses._last["val"]
    y2[:, 5:20, 7:40] = 0.25
    ss2 = losses.ssim(x, y2)
    assert losses._last["val"] is not val
    fresh = losses.l1_ssim(x.detach().clone(), y2.clone())[1]
    assert torch.equal(ss2.detach(), fresh) and not torch.equal(ss2.detach(), ss.detach())
    edited = pr.evaluate(x, y2, torch.float64)[1]
    edited32 = pr.evaluate(x, y2, torch.float32)[1]
    _check_scalar(((3, 33, 65), "random"), "ssim[edited gt]", ss2.detach(), edited, edited32, 1.0)
    # and the image edited in place (an optimiser step between a logging call and the next loss)
    with torch.no_grad():
        x.mul_(0.5)
    l3 = losses.l1_loss(x, y2)
    assert torch.equal(l3.detach(), losses.l1_ssim(x.detach().clone(), y2.clone())[0]) and not torch.equal(l3.detach(), l1.detach())
