"""csrc/style.hip on the GPU against tests/style_reference.py: the image-space losses, the Gram matrix and the gradient GEMM on
the exact-fp32 matrix instruction, the channel statistics and the style_statistics_loss node.

* exact: integer-valued data has one right fp32 answer in any summation order: ``torch.equal`` against the integer statement;
* real-valued: bounds derived from the kernels' restated constants (chain length, K) and the unit roundoff, never measured;
* every C-ABI case runs twice for identical bits, with a 0xCD canary behind every output and workspace, inputs unmodified.
The real-valued tests print the share of their bound that the device used (pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import style_reference as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CANARY, PAD = 0xCD, 256
U = R.U
HERE = os.path.dirname(os.path.abspath(__file__))


def _guarded(nbytes):
    return torch.full((nbytes + PAD,), CANARY, dtype=torch.uint8, device=DEV)


def _intact(buf, nbytes):
    return bool((buf[nbytes:] == CANARY).all())


def _f32(buf, n):
    return buf[:4 * n].view(torch.float32).clone()


def _lib():
    from trase_amd import _lib
    return _lib, _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _twice(fn):
    """fn() -> tuple of tensors; run twice, identical bits"""
    a, b = fn(), fn()
    for s, t in zip(a, b):
        assert torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s, t.view(torch.int32) if t.dtype == torch.float32 else t), \
            "two calls differ"
    return a


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


# ---- image-space losses ---------------------------------------------------------------------------------------------------------------
def _px_abi(kind, x, gt, pitch, aux, aux_kind, g=1.0):
    """forward + backward through the C entry points -> (value (1,), gradient like x) on the device"""
    _l, lib = _lib()
    c, h, w = x.shape
    n = c * h * w
    nb = C.c_size_t()
    _l.check(lib.trase_pixel_loss_ws_bytes(C.byref(nb)), "sizes")
    keep = [t.clone() for t in (x, gt) + (() if aux is None else (aux,))]

    def run():
        out, ws, dx = _guarded(4), _guarded(nb.value), _guarded(4 * n)
        gt_ = torch.tensor([g], device=DEV)
        _l.check(lib.trase_pixel_loss_forward(_l.ptr(x), _l.ptr(gt), pitch, c, h, w, kind, _l.ptr(aux), aux_kind, _l.ptr(out), _l.ptr(ws),
                                              nb.value, 0, _stream()), "forward")
        _l.check(lib.trase_pixel_loss_backward(_l.ptr(x), _l.ptr(gt), pitch, c, h, w, kind, _l.ptr(aux), aux_kind, _l.ptr(gt_), _l.ptr(ws),
                                               nb.value, _l.ptr(dx), 0, _stream()), "backward")
        torch.cuda.synchronize()
        assert _intact(out, 4) and _intact(ws, nb.value) and _intact(dx, 4 * n), "written past a stated size"
        return _f32(out, 1), _f32(dx, n).view(c, h, w)
    val, grad = _twice(run)
    for t, k in zip((x, gt) + (() if aux is None else (aux,)), keep):
        assert torch.equal(t, k), "an input was modified"
    return val, grad


def _aux_of(kind, shape, rng, integer):
    c, h, w = shape
    if kind == R.L2:
        return None, 0
    if kind == R.MASKED:
        m = rng.integers(0, 4, size=(h, w)) if integer else (rng.random((h, w)) * (rng.random((h, w)) > 0.3))
        return m.astype(np.float32), 2
    wgt = rng.integers(0, 4, size=(c, h, w)) if integer else rng.random((c, h, w))
    return wgt.astype(np.float32), 3


@pytest.mark.parametrize("shape", R.PIXEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", [R.MASKED, R.WEIGHTED, R.L2], ids=["masked", "weighted", "l2"])
def test_pixel_losses_exact_on_integers(kind, shape):
    rng = np.random.default_rng(sum(shape) + kind)
    x, gt = rng.integers(0, 8, size=shape).astype(np.float32), rng.integers(0, 8, size=shape).astype(np.float32)
    aux, ak = _aux_of(kind, shape, rng, True)
    if kind == R.MASKED:
        aux[0, 0] = 1                                              # (never all zero)
    val, grad = _px_abi(kind, _dev(x), _dev(gt), 0, None if aux is None else _dev(aux), ak)
    d = x.astype(np.int64) - gt.astype(np.int64)
    a = None if aux is None else np.broadcast_to(aux.astype(np.int64), shape)
    num = int((d * d).sum()) if kind == R.L2 else int((np.abs(d) * a).sum())
    den = int(a.sum()) if kind == R.MASKED else d.size
    inv = np.float32(1.0 / den)
    want_g = (np.float32(2.0) * inv) * d.astype(np.float32) if kind == R.L2 else (np.sign(d) * a).astype(np.float32) * inv
    assert torch.equal(val.cpu(), torch.tensor([np.float32(num / den)]))
    assert torch.equal(grad.cpu(), torch.from_numpy(want_g.astype(np.float32)))


@pytest.mark.parametrize("shape", R.PIXEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", [R.MASKED, R.WEIGHTED, R.L2], ids=["masked", "weighted", "l2"])
def test_pixel_losses_on_random_data(kind, shape):
    rng = np.random.default_rng(7 * sum(shape) + kind)
    x, gt = rng.random(shape, dtype=np.float32), rng.random(shape, dtype=np.float32)
    gt.reshape(-1)[::5] = x.reshape(-1)[::5]                        # sign(0) = 0
    aux, ak = _aux_of(kind, shape, rng, False)
    if kind == R.MASKED:
        aux[0, 0] = 0.5
    for g in (1.0, 0.7):
        val, grad = _px_abi(kind, _dev(x), _dev(gt), 0, None if aux is None else _dev(aux), ak, g)
        want = R.pixel_value(kind, x, gt, aux)
        ulp = np.spacing(np.abs(want)) if want != 0 else np.float32(1e-45)
        print(f"value {float(val[0]):.9g} want {float(want):.9g}")
        assert abs(np.float64(val.cpu().numpy()[0]) - np.float64(want)) <= np.float64(ulp)
        wg = R.pixel_grad(kind, x, gt, aux, np.float32(g))
        assert np.array_equal(grad.cpu().numpy().view(np.int32), wg.view(np.int32))
    if kind == R.WEIGHTED and shape[0] > 1:                         # an (H, W) weight is the (C, H, W) weight that repeats it
        w2 = aux[0]
        v1, g1 = _px_abi(kind, _dev(x), _dev(gt), 0, _dev(w2), 2)
        v2, g2 = _px_abi(kind, _dev(x), _dev(gt), 0, _dev(np.broadcast_to(w2, shape)), 3)
        assert torch.equal(v1, v2) and torch.equal(g1, g2)


def _api(fn, x, *rest):
    xl = x.detach().clone().requires_grad_(True)
    v = fn(xl, *rest)
    v.backward()
    return v.detach(), xl.grad


@pytest.mark.parametrize("shape", [(3, 5, 7), (3, 33, 257), (3, 64, 65)], ids=lambda s: "x".join(map(str, s)))
def test_byte_frame_ground_truth_is_bitwise_the_float_call(shape):
    from trase_amd import losses as L
    from trase_amd.frames import ByteFrame
    rng = np.random.default_rng(shape[2])
    c, h, w = shape
    pitch = ByteFrame.pitch_for(w)
    x = _dev(rng.random(shape, dtype=np.float32))
    mask, wgt = _dev(rng.random((h, w)) > 0.4, torch.bool), _dev(rng.random(shape, dtype=np.float32))
    for pad in (0, 0xFF):
        planes = np.full((3, h, pitch), pad, np.uint8)
        planes[:, :, :w] = rng.integers(0, 256, size=(3, h, w))
        frame = ByteFrame(_dev(planes.reshape(-1), torch.uint8), h, w)
        gt = frame.to_float()
        assert np.array_equal(gt.cpu().numpy(), R.byte_gt(planes[:, :, :w]))
        for fn, rest in ((L.masked_l1_loss, (mask,)), (L.weighted_l1_loss, (wgt,)), (L.l2_loss, ())):
            va, ga = _api(fn, x, frame, *rest)
            vb, gb = _api(fn, x, gt, *rest)
            assert torch.equal(va, vb) and torch.equal(ga, gb), fn.__name__


def test_masks_all_zero_and_of_every_type():
    from trase_amd import losses as L
    rng = np.random.default_rng(1)
    x, gt = _dev(rng.random((3, 31, 33), dtype=np.float32)), _dev(rng.random((3, 31, 33), dtype=np.float32))
    for zero in (torch.zeros(31, 33, device=DEV), torch.zeros(31, 33, device=DEV, dtype=torch.bool)):
        v, g = _api(L.masked_l1_loss, x, gt, zero)
        assert float(v) == 0.0 and not g.any()
    m = _dev(rng.random((31, 33)) > 0.5, torch.bool)
    res = [_api(L.masked_l1_loss, x, gt, mm) for mm in (m, m.to(torch.uint8), m.float(), m.double(), m.half())]
    for v, g in res[1:]:
        assert torch.equal(v, res[0][0]) and torch.equal(g, res[0][1])
    # the value of a uint8 mask counts, as mask.float() does
    v255, g255 = _api(L.masked_l1_loss, x, gt, m.to(torch.uint8) * 255)
    vf, gf = _api(L.masked_l1_loss, x, gt, m.float() * 255)
    assert torch.equal(v255, vf) and torch.equal(g255, gf)


def test_constants_that_require_grad_are_detached_with_one_warning():
    from trase_amd import losses as L
    L._CONST_WARNED.discard("l2_loss")
    x, y = torch.rand(3, 4, 5, device=DEV, requires_grad=True), torch.rand(3, 4, 5, device=DEV, requires_grad=True)
    with pytest.warns(UserWarning, match="detaching"):
        L.l2_loss(x, y).backward()
    assert y.grad is None and x.grad is not None
    import warnings
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        L.l2_loss(x, y)
    assert not [w for w in seen if "detaching" in str(w.message)]


# ---- Gram matrix ------------------------------------------------------------------------------------------------------------------------------
def _gram_abi(x):
    _l, lib = _lib()
    c, n = x.shape
    nb = C.c_size_t()
    _l.check(lib.trase_style_ws_bytes(c, n, C.byref(nb)), "sizes")
    keep = x.clone()

    def run():
        G, ws = _guarded(4 * c * c), _guarded(nb.value)
        _l.check(lib.trase_gram_matrix(_l.ptr(x), c, n, _l.ptr(G), _l.ptr(ws), nb.value, 0, _stream()), "gram")
        torch.cuda.synchronize()
        assert _intact(G, 4 * c * c) and _intact(ws, nb.value), "written past a stated size"
        return (_f32(G, c * c).view(c, c),)
    (G,) = _twice(run)
    assert torch.equal(x, keep), "the input was modified"
    assert torch.equal(G, G.t().contiguous()), "G != G.T"
    return G


def _gram_exact(c, n, seed):
    x = torch.from_numpy(R.lattice_rows(c, n, seed)).to(DEV)                 # float64 integers: every product and sum is exact
    want = x @ x.t()
    G = _gram_abi(x.float().contiguous())
    bad = int((G.double() != want).sum())
    assert bad == 0 and torch.equal(G.to(torch.int64), want.to(torch.int64)), f"C {c} n {n}: {bad} of {c * c} differ"


@pytest.mark.parametrize("c", R.GRAM_C)
def test_gram_exact_on_lattice_rows(c):
    for n in [n for cc, n in R.GRAM_CASES if cc == c]:
        _gram_exact(c, n, c * 7919 + n)


@pytest.mark.parametrize("c,n", R.GRAM_CAP_CASES, ids=lambda v: str(v))
def test_gram_exact_at_the_slice_cap(c, n):
    _gram_exact(c, n, c + n)


@pytest.mark.parametrize("c,n", [(33, R.GR_CHAIN + 1), (129, 2 * R.GR_CHAIN + 1), (512, 3000), (64, 401 * R.GR_CHAIN + 3)], ids=lambda v: str(v))
def test_gram_real_rows_inside_the_derived_bound(c, n):
    g = torch.Generator(device="cpu").manual_seed(c + n)
    x = (torch.randn(c, n, generator=g) + 0.3).to(DEV)
    G = _gram_abi(x)
    xd = x.double()
    G64, bound = xd @ xd.t(), R.gamma(R.GR_CHAIN + 1) * (xd.abs() @ xd.abs().t())
    share = float(((G.double() - G64).abs() / bound).max())
    print(f"C {c} n {n}: largest share of the bound {share:.3g}")
    assert share <= 1.0


# ---- the gradient GEMM alone --------------------------------------------------------------------------------------------------------------------
def _gemm_abi(D, a, b, cc, x, y, g=None):
    _l, lib = _lib()
    c, n = x.shape
    t = [None if v is None else _dev(v) for v in (D, a, b, x, y)]
    gt_ = None if g is None else torch.tensor([g], device=DEV)
    keep = [None if v is None else v.clone() for v in t]

    def run():
        dx = _guarded(4 * c * n)
        _l.check(lib.trase_style_grad_gemm(_l.ptr(t[0]), _l.ptr(t[1]), _l.ptr(t[2]), float(cc), _l.ptr(t[3]), _l.ptr(t[4]), c, n, _l.ptr(gt_),
                                           _l.ptr(dx), 0, _stream()), "grad_gemm")
        torch.cuda.synchronize()
        assert _intact(dx, 4 * c * n), "written past the stated size"
        return (_f32(dx, c * n).view(c, n),)
    (dx,) = _twice(run)
    for v, k in zip(t, keep):
        assert v is None or torch.equal(v, k), "an input was modified"
    return dx.cpu().numpy()


GEMM_SHAPES = [(1, 1), (31, 33), (33, 127), (64, 128), (65, 129), (129, 257), (512, 130)]
GEMM_PARTS = {"all": (1, 1, 1), "product": (1, 0, 0), "adain": (0, 1, 0), "content": (0, 0, 1), "product+content": (1, 0, 1)}


@pytest.mark.parametrize("parts", list(GEMM_PARTS))
@pytest.mark.parametrize("c,n", GEMM_SHAPES, ids=lambda v: str(v))
def test_grad_gemm_exact_on_integers(c, n, parts):
    rng = np.random.default_rng(c * n + len(parts))
    use_d, use_ab, use_y = GEMM_PARTS[parts]
    D = rng.integers(-2, 3, size=(c, c)).astype(np.float64) if use_d else None
    a = rng.integers(-4, 5, size=c).astype(np.float64) if use_ab else None
    b = rng.integers(-4, 5, size=c).astype(np.float64) if use_ab else None
    x, y = R.lattice_rows(c, n, 1), (R.lattice_rows(c, n, 2) if use_y else None)
    for g in (None, 2.0):
        got = _gemm_abi(D, a, b, 2.0, x, y, g)
        want = R.grad_gemm(D, a, b, 2.0, x, y) * (1.0 if g is None else g)
        assert np.abs(want).max() < 2 ** 24 and np.array_equal(got.astype(np.float64), want), f"{int((got != want).sum())} differ"


@pytest.mark.parametrize("c,n", GEMM_SHAPES, ids=lambda v: str(v))
def test_grad_gemm_real_data_inside_the_derived_bound(c, n):
    rng = np.random.default_rng(c + n)
    f = lambda *s: rng.normal(size=s).astype(np.float32).astype(np.float64)          # noqa: E731
    D, a, b, x, y, cc = f(c, c), f(c), f(c), f(c, n), f(c, n), float(np.float32(0.37))
    got = _gemm_abi(D, a, b, cc, x, y)
    err = np.abs(got - R.grad_gemm(D, a, b, cc, x, y))
    bound = R.gamma(c + 4) * R.grad_gemm_abs(D, a, b, cc, x, y)
    print(f"C {c} n {n}: largest share of the bound {float((err / bound).max()):.3g}")
    assert (err <= bound).all()


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------------
def _stats_abi(x, eps=1e-8):
    _l, lib = _lib()
    c, n = x.shape
    nb = C.c_size_t()
    _l.check(lib.trase_style_ws_bytes(c, n, C.byref(nb)), "sizes")
    keep = x.clone()

    def run():
        mean, std, ws = _guarded(4 * c), _guarded(4 * c), _guarded(nb.value)
        _l.check(lib.trase_mean_std(_l.ptr(x), c, n, eps, _l.ptr(mean), _l.ptr(std), _l.ptr(ws), nb.value, 0, _stream()), "mean_std")
        torch.cuda.synchronize()
        assert _intact(mean, 4 * c) and _intact(std, 4 * c) and _intact(ws, nb.value), "written past a stated size"
        return _f32(mean, c), _f32(std, c)
    mean, std = _twice(run)
    assert torch.equal(x, keep)
    return mean.cpu().numpy(), std.cpu().numpy()


@pytest.mark.parametrize("n", R.STATS_N)
@pytest.mark.parametrize("c", R.STATS_C)
def test_mean_std_within_two_units_of_float64(c, n):
    rng = np.random.default_rng(c * 1000 + n)
    scale = np.exp(rng.normal(size=(c, 1)))
    cases = {"random": rng.normal(size=(c, n)) * scale + rng.normal(size=(c, 1)),
             "offset": (rng.normal(size=(c, n)) + 1024.0) * scale,                     # |mean| = 2^10 * std
             "constant": np.broadcast_to(rng.normal(size=(c, 1)), (c, n))}
    eps32 = np.float32(1e-8)
    for name, x in cases.items():
        x = np.ascontiguousarray(x, np.float32)
        mean, std = _stats_abi(_dev(x))
        mu, sd = R.mean_std(x.astype(np.float64), 0.0)
        if name == "constant":
            assert np.array_equal(mean, x[:, 0]) and (std == eps32).all()
            continue
        want_sd = sd + 1e-8
        sm, ss = float((np.abs(mean - mu) / np.abs(mu)).max() / (2 * U)), float((np.abs(std - want_sd) / want_sd).max() / (2 * U))
        print(f"C {c} n {n} {name}: shares of 2u: mean {sm:.3g} std {ss:.3g}")
        assert sm <= 1.0 and ss <= 1.0


# ---- the whole node -------------------------------------------------------------------------------------------------------------------------------
def _node_abi(x, gram, mean, std, content, weights):
    """-> (out4, saved (C*C + 2C), dx) numpy, through the C entry points"""
    _l, lib = _lib()
    c, n = x.shape
    gw, aw, cw = weights
    nb = C.c_size_t()
    _l.check(lib.trase_style_ws_bytes(c, n, C.byref(nb)), "sizes")
    ns = c * c + 2 * c
    keep = x.clone()

    def run():
        out4, saved, ws, dx = _guarded(16), _guarded(4 * ns), _guarded(nb.value), _guarded(4 * c * n)
        _l.check(lib.trase_style_node_forward(_l.ptr(x), c, n, _l.ptr(gram), _l.ptr(mean), _l.ptr(std), _l.ptr(content), gw, aw, cw,
                                              _l.ptr(out4), _l.ptr(saved), _l.ptr(ws), nb.value, 0, _stream()), "node_forward")
        sv = saved[:4 * ns].view(torch.float32)
        D = sv[:c * c] if gw else None
        a, b = (sv[c * c:c * c + c], sv[c * c + c:]) if aw else (None, None)
        _l.check(lib.trase_style_grad_gemm(_l.ptr(D), _l.ptr(a), _l.ptr(b), 2.0 * cw / (float(c) * float(n)), _l.ptr(x),
                                           _l.ptr(content if cw else None), c, n, None, _l.ptr(dx), 0, _stream()), "grad_gemm")
        torch.cuda.synchronize()
        assert _intact(out4, 16) and _intact(saved, 4 * ns) and _intact(ws, nb.value) and _intact(dx, 4 * c * n), "written past a stated size"
        live = torch.cat([sv[:c * c] if gw else sv[:0], sv[c * c:] if aw else sv[:0]]).clone()     # a term that is off leaves its part unwritten
        return _f32(out4, 4), live, _f32(dx, c * n).view(c, n)
    out4, live, dx = _twice(run)
    assert torch.equal(x, keep)
    return out4.cpu().numpy().astype(np.float64), live.cpu().numpy().astype(np.float64), dx.cpu().numpy().astype(np.float64)


def _node_bounds(x, S, B_S, s_mean, s_std, content, weights, targets_exact=False):
    """float64 value and gradient of the node and the bounds of the device's deviation from them.  x, S, ...: float64 copies of what
    the device was given.  When S, s_mean, s_std are the EXACT statistics of a style map whose targets the device computed itself
    (targets_exact), the targets' own bars enter: B_S, the Gram bound of the style map, and 2u of its mean and std."""
    gw, aw, cw = weights
    c, n = x.shape
    total, lg, la, lc = R.node(x, S, s_mean, s_std, content, gw, aw, cw)
    grad = R.node_grad(x, S, s_mean, s_std, content, gw, aw, cw)
    vb, gb = 0.0, np.zeros_like(x)
    D = a = b = None
    if gw:
        scale = gw / (c * c) / (c * n)
        G = R.gram(x)
        B = R.gram_bound(x) + B_S
        vb += scale * (2.0 * np.abs(G - S) * B + B * B).sum() + U * abs(lg)
        D = 2.0 * scale * (G - S)
        dD = 2.0 * scale * B + 3.0 * U * np.abs(D)                  # the Gram error, and the roundings of coef, G - S and their product
        gb += 2.0 * dD @ np.abs(x)
    if aw:
        mu, sd = R.mean_std(x)
        dm, ds = np.abs(mu - s_mean), np.abs(sd - s_std)
        em, es = 2 * U * np.abs(mu), 2 * U * sd                     # the statistics' own bar
        if targets_exact:
            em, es = em + 2 * U * np.abs(s_mean), es + 2 * U * s_std
        vb += aw / c * (2 * dm * em + em * em + 2 * ds * es + es * es).sum() + U * abs(la)
        k = aw * 2.0 / c
        sd0 = sd - 1e-8
        b = k * (sd - s_std) / ((n - 1) * sd0)
        a = k * (mu - s_mean) / n - b * mu
        db = k * es / ((n - 1) * sd0) + U * np.abs(b)
        da = k * em / n + db * np.abs(mu) + U * (np.abs(k * (mu - s_mean) / n) + np.abs(b * mu))
        gb += da[:, None] + db[:, None] * np.abs(x)
    if cw:
        vb += (R.gamma(3) + U) * abs(lc)
    vb += U * abs(total)
    cc = 2.0 * cw / (c * n)
    gb += R.gamma(c + 4) * R.grad_gemm_abs(D, a, b, cc, x, content if cw else None) + (U * np.abs(cc * (x - content)) if cw else 0.0)
    return (total, lg, la, lc), grad, vb, gb


NODE_WEIGHTS = {"gram": (3e4, 0.0, 0.0), "adain": (0.0, 1.5, 0.0), "content": (0.0, 0.0, 0.75), "all": (3e4, 1.5, 0.75)}


@pytest.fixture(scope="module")
def node_data():
    """per shape: x, the style targets of a style map of ANOTHER size (computed on the device, once), the content map"""
    from trase_amd import losses as L
    out = {}
    for c, h, w in R.NODE_SHAPES:
        g = torch.Generator().manual_seed(c + h)
        x = torch.relu(torch.randn(1, c, h, w, generator=g) + 0.3).to(DEV)
        style = torch.relu(torch.randn(1, c, h + 3, w - 2, generator=g) * 1.5 + 0.1).to(DEV)
        content = torch.relu(torch.randn(1, c, h, w, generator=g) + 0.3).to(DEV)
        out[c] = (x, style, content, L.StyleTargets.from_features(style, content))
    return out


@pytest.mark.parametrize("term", list(NODE_WEIGHTS))
@pytest.mark.parametrize("shape", R.NODE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_node_value_and_gradient_inside_the_bounds(node_data, shape, term):
    c = shape[0]
    x4, style, content4, T = node_data[c]
    x, content = x4.reshape(c, -1).contiguous(), T.content
    weights = NODE_WEIGHTS[term]
    out4, _, dx = _node_abi(x, T.gram, T.mean, T.std, content, weights)
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)      # noqa: E731
    vals, grad, vb, gb = _node_bounds(f64(x), f64(T.gram), 0.0, f64(T.mean), f64(T.std), f64(content), weights)
    print(f"{shape} {term}: value share {abs(out4[0] - vals[0]) / vb:.3g}, gradient share {float((np.abs(dx - grad) / np.maximum(gb, 1e-300)).max()):.3g}")
    assert abs(out4[0] - vals[0]) <= vb
    for got, want in zip(out4[1:], vals[1:]):
        assert abs(got - want) <= vb and (want != 0.0 or got == 0.0)
    assert (np.abs(dx - grad) <= gb).all()
    # the targets of the style map were computed from a map of another size: they are the ABI's own results
    sx = style.reshape(c, -1).contiguous()
    assert torch.equal(T.gram, _gram_abi(sx))
    m, s = _stats_abi(sx)
    assert np.array_equal(f64(T.mean), m) and np.array_equal(f64(T.std), s)


@pytest.mark.parametrize("shape", R.NODE_SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_reference_named_functions_are_the_node_with_one_weight(node_data, shape):
    from trase_amd import losses as L
    c = shape[0]
    x4, style, content4, T = node_data[c]
    pairs = [
        (lambda t: L.cal_style_loss(t, style, 2.5), lambda t: L.style_statistics_loss(t, T, gram_weight=2.5)),
        (lambda t: L.cal_style_loss(t, T.gram, 2.5), lambda t: L.style_statistics_loss(t, T, gram_weight=2.5)),
        (lambda t: L.cal_adain_style_loss(t, style), lambda t: L.style_statistics_loss(t, T, adain_weight=1.0)),
        (lambda t: L.cal_adain_style_loss(t, (T.mean, T.std)), lambda t: L.style_statistics_loss(t, T, adain_weight=1.0)),
        (lambda t: L.cal_mse_content_loss(t, content4), lambda t: L.style_statistics_loss(t, T, content_weight=1.0)),
    ]
    for k, (named, node) in enumerate(pairs):
        va, ga = _api(named, x4)
        vb, gb = _api(node, x4)
        assert torch.equal(va, vb) and torch.equal(ga, gb), k
        assert ga.shape == x4.shape
    # the two functions that return statistics are the ABI's results; the (C, n) form gives the same bits
    x2 = x4.reshape(c, -1).contiguous()
    assert torch.equal(L.gram_matrix(x4), _gram_abi(x2)) and torch.equal(L.gram_matrix(x2), L.gram_matrix(x4))
    mean, std = L.calc_mean_std(x4)
    m, s = _stats_abi(x2)
    assert mean.shape == std.shape == (1, c, 1)
    assert np.array_equal(mean.reshape(-1).cpu().numpy(), m) and np.array_equal(std.reshape(-1).cpu().numpy(), s)
    # parts, and the sum of three nodes against the node of three terms
    total, lg, la, lc = L.style_statistics_loss(x4, T, gram_weight=3e4, adain_weight=1.5, content_weight=0.75, with_parts=True)
    assert not (lg.requires_grad or la.requires_grad or lc.requires_grad)
    assert torch.equal(lg, L.style_statistics_loss(x4, T, gram_weight=3e4)) and torch.equal(la, L.style_statistics_loss(x4, T, adain_weight=1.5))
    assert torch.equal(lc, L.style_statistics_loss(x4, T, content_weight=0.75))
    assert abs(float(total) - (float(lg) + float(la) + float(lc))) <= 2 * U * abs(float(total))


@pytest.mark.parametrize("tag", ["f8", "f64"])
def test_fixture_under_the_same_bars(tag):
    """the reference's own float64 results (tests/golden/style_losses.npz) through the Python functions"""
    from trase_amd import losses as L
    fx = np.load(os.path.join(HERE, "golden", "style_losses.npz"))
    x4, style4, content4 = (_dev(fx[tag + k]) for k in ("_x", "_style", "_content"))
    c = x4.shape[1]
    f64 = lambda a: np.asarray(a, np.float64)                        # noqa: E731
    x, style, content = (f64(fx[tag + k]).reshape(c, -1) for k in ("_x", "_style", "_content"))
    w = float(fx["style_weight"])
    S, (s_mean, s_std) = R.gram(style), R.mean_std(style)
    # the style targets are computed on the device too: their own bars enter the bound (targets_exact)
    for name, fn, weights in (("_style_loss", lambda t: L.cal_style_loss(t, style4, w), (w, 0.0, 0.0)),
                              ("_adain", lambda t: L.cal_adain_style_loss(t, style4), (0.0, 1.0, 0.0)),
                              ("_content_loss", lambda t: L.cal_mse_content_loss(t, content4), (0.0, 0.0, 1.0))):
        v, g = _api(fn, x4)
        vals, grad, vb, gb = _node_bounds(x, S, R.gram_bound(style), s_mean, s_std, content, weights, targets_exact=True)
        assert abs(vals[0] - float(fx[tag + name])) <= 1e-12 * max(1.0, abs(vals[0]))
        assert abs(float(v) - float(fx[tag + name])) <= vb, name
        assert (np.abs(g.cpu().numpy().astype(np.float64).reshape(c, -1) - f64(fx[tag + name + "_grad"]).reshape(c, -1)) <= gb).all(), name
    # the statistics and the Gram matrix themselves, and their gradients under the fixture's cotangents
    mean, std = L.calc_mean_std(x4)
    assert (np.abs(f64(mean.cpu()) - fx[tag + "_mean"]) <= 2 * U * np.abs(fx[tag + "_mean"])).all()
    assert (np.abs(f64(std.cpu()) - fx[tag + "_std"]) <= 2 * U * np.abs(fx[tag + "_std"])).all()
    assert (np.abs(f64(L.gram_matrix(x4).cpu()) - fx[tag + "_gram"]) <= R.gram_bound(x)).all()
    cm, cs = _dev(fx[tag + "_cot_mean"]), _dev(fx[tag + "_cot_std"])
    cg = torch.outer(_dev(fx[tag + "_cot_gram_u"]), _dev(fx[tag + "_cot_gram_v"]))
    _, g = _api(lambda t: sum((p * q).sum() for p, q in zip(L.calc_mean_std(t), (cm, cs))), x4)
    n = x.shape[1]
    mu, sd = R.mean_std(x, 0.0)
    gm, gs = f64(fx[tag + "_cot_mean"]).reshape(-1), f64(fx[tag + "_cot_std"]).reshape(-1)
    bterm = np.abs(gs / ((n - 1) * sd))
    # b from the fp32 std - eps (2u + the subtraction), a = g_mean / n - b * mean in fp32: a dozen roundings on the terms' magnitudes
    bound = R.gamma(16) * (np.abs(gm / n)[:, None] + bterm[:, None] * (np.abs(mu)[:, None] + np.abs(x)))
    assert (np.abs(f64(g.cpu()).reshape(c, -1) - f64(fx[tag + "_mean_std_dot_grad"]).reshape(c, -1)) <= bound).all()
    _, g = _api(lambda t: (L.gram_matrix(t) * cg).sum(), x4)
    cg64 = f64(cg.cpu())
    bound = R.gamma(c + 8) * (np.abs(cg64) + np.abs(cg64.T)) @ np.abs(x)
    assert (np.abs(f64(g.cpu()).reshape(c, -1) - f64(fx[tag + "_gram_dot_grad"]).reshape(c, -1)) <= bound).all()


def test_constant_channel_takes_no_gradient_from_the_std_term():
    from trase_amd import losses as L
    x = torch.rand(1, 4, 6, 7, device=DEV)
    x[0, 1] = 0.75
    T = L.StyleTargets(mean=torch.rand(4, device=DEV), std=torch.rand(4, device=DEV) + 0.5)
    v, g = _api(lambda t: L.style_statistics_loss(t, T, adain_weight=1.0), x)
    assert torch.isfinite(v) and torch.isfinite(g).all()
    want = 2.0 / 4 * (0.75 - float(T.mean[1])) / 42                  # the mean term alone
    assert (g[0, 1] == g[0, 1, 0, 0]).all() and abs(float(g[0, 1, 0, 0]) - want) <= 8 * U * abs(want)
