"""tests/style_reference.py against the fixture of the reference's own functions (tests/golden/style_losses.npz), its closed-form
gradients against float64 autograd, the statistics' accuracy claim, the GPU test's case plan against the kernels' tiling, and
every refusal of the new entry points and Python functions.  No GPU."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

from tests import style_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-12


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "style_losses.npz")))


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape or a.size == b.size == 1, (a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a.reshape(b.shape) - b).max()) if b.ndim else abs(float(a) - float(b))
    assert err <= TOL * scale, err


def _f64(a):
    return np.asarray(a, np.float64)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def test_fixture_is_small_and_holds_arrays_only(fx):
    assert os.path.getsize(os.path.join(HERE, "golden", "style_losses.npz")) < 100 * 1024
    assert all(isinstance(v, np.ndarray) and v.dtype.kind in "fb" for v in fx.values())


def test_pixel_statements_equal_the_fixture(fx):
    img, gt = _f64(fx["img"]), _f64(fx["gt"])
    for name, mask in (("masked_bool", fx["mask_bool"]), ("masked_float", fx["mask_float"])):
        _close(R.masked_l1(img, gt, mask), fx[name])
        _close(R.masked_l1_grad(img, gt, mask), fx[name + "_grad"])
    for name, w in (("weighted_hw", fx["weight_hw"]), ("weighted_chw", fx["weight_chw"])):
        _close(R.weighted_l1(img, gt, _f64(w)), fx[name])
        _close(R.weighted_l1_grad(img, gt, _f64(w)), fx[name + "_grad"])
    _close(R.l2(img, gt), fx["l2"])
    _close(R.l2_grad(img, gt), fx["l2_grad"])


@pytest.mark.parametrize("tag", ["f8", "f64"])
def test_feature_statements_equal_the_fixture(fx, tag):
    x4, style4, content4 = _f64(fx[tag + "_x"]), _f64(fx[tag + "_style"]), _f64(fx[tag + "_content"])
    c = x4.shape[1]
    x, style, content = x4.reshape(c, -1), style4.reshape(c, -1), content4.reshape(c, -1)
    mu, sd = R.mean_std(x)
    _close(mu, fx[tag + "_mean"].reshape(-1))
    _close(sd, fx[tag + "_std"].reshape(-1))
    _close(R.gram(x), fx[tag + "_gram"])
    cm, cs = _f64(fx[tag + "_cot_mean"]).reshape(-1), _f64(fx[tag + "_cot_std"]).reshape(-1)
    _close(R.mean_std_grad(x, cm, cs).reshape(x4.shape), fx[tag + "_mean_std_dot_grad"])
    cg = np.outer(_f64(fx[tag + "_cot_gram_u"]), _f64(fx[tag + "_cot_gram_v"]))
    _close(R.gram_grad(x, cg).reshape(x4.shape), fx[tag + "_gram_dot_grad"])
    s_mean, s_std = R.mean_std(style)
    _close(R.adain(x, s_mean, s_std), fx[tag + "_adain"])
    _close(R.adain_grad(x, s_mean, s_std).reshape(x4.shape), fx[tag + "_adain_grad"])
    w = float(fx["style_weight"])
    _close(R.style_loss(x, R.gram(style), w), fx[tag + "_style_loss"])
    _close(R.style_loss_grad(x, R.gram(style), w).reshape(x4.shape), fx[tag + "_style_loss_grad"])
    _close(R.l2(x, content), fx[tag + "_content_loss"])
    _close(R.l2_grad(x, content).reshape(x4.shape), fx[tag + "_content_loss_grad"])


# ---- closed-form gradients against float64 autograd of the reference's expressions ------------------------------------------------------------
def _ref_node(x, s_gram, s_mean, s_std, content, gw, aw, cw):
    """utils/loss_utils.py:230-272 as written there, on (C, n) float64 tensors"""
    c, n = x.shape
    mean = torch.mean(x, dim=-1, keepdim=True)
    std = torch.std(x, dim=-1, keepdim=True) + 1e-8
    adain = torch.nn.functional.mse_loss(mean, s_mean[:, None]) + torch.nn.functional.mse_loss(std, s_std[:, None])
    style = gw * torch.mean((torch.mm(x, x.t()) - s_gram) ** 2) / (c * n)
    return style + aw * adain + cw * torch.nn.functional.mse_loss(x, content)


@pytest.mark.parametrize("weights", [(2.5, 0, 0), (0, 1.5, 0), (0, 0, 0.75), (3e3, 0.5, 2.0)])
@pytest.mark.parametrize("c,n", [(5, 7), (33, 20)])
def test_node_gradient_equals_autograd(c, n, weights):
    rng = np.random.default_rng(c * 100 + n)
    x, style, content = rng.normal(size=(c, n)) + 0.5, rng.normal(size=(c, n + 3)) * 1.5, rng.normal(size=(c, n))
    s_gram, (s_mean, s_std) = R.gram(style), R.mean_std(style)
    gw, aw, cw = weights
    xt = torch.tensor(x, requires_grad=True)
    v = _ref_node(xt, torch.tensor(s_gram), torch.tensor(s_mean), torch.tensor(s_std), torch.tensor(content), gw, aw, cw)
    v.backward()
    kw = dict(s_gram=s_gram, s_mean=s_mean, s_std=s_std, content=content, gw=gw, aw=aw, cw=cw)
    _close(R.node(x, **kw)[0], v.item())
    _close(R.node_grad(x, **kw), xt.grad.numpy())


def test_pixel_gradients_equal_autograd():
    rng = np.random.default_rng(3)
    x, gt, m, w = rng.random((3, 6, 5)), rng.random((3, 6, 5)), (rng.random((6, 5)) > 0.3).astype(np.float64), rng.random((3, 6, 5))
    for fn, grad, aux in ((lambda t: (torch.abs(t - torch.tensor(gt)) * torch.tensor(m)[None].repeat(3, 1, 1)).sum() / (3 * m.sum()), R.masked_l1_grad, m),
                          (lambda t: (torch.abs(t - torch.tensor(gt)) * torch.tensor(w)).mean(), R.weighted_l1_grad, w)):
        xt = torch.tensor(x, requires_grad=True)
        fn(xt).backward()
        _close(grad(x, gt, aux), xt.grad.numpy())
    assert R.masked_l1(x, gt, np.zeros((6, 5))) == 0.0 and not R.masked_l1_grad(x, gt, np.zeros((6, 5))).any()


def test_grad_gemm_statement_is_the_node_gradient():
    """the backward launch's formula with D = 2 gw scale (G - S) and the AdaIN coefficients a, b reproduces node_grad"""
    rng = np.random.default_rng(11)
    c, n = 9, 14
    x, style, content = rng.normal(size=(c, n)) + 0.3, rng.normal(size=(c, 6)), rng.normal(size=(c, n))
    s_gram, (s_mean, s_std) = R.gram(style), R.mean_std(style)
    gw, aw, cw = 40.0, 0.7, 1.3
    D = 2.0 * gw / (c * c) / (c * n) * (R.gram(x) - s_gram)
    mu = x.mean(axis=1)
    sd0 = np.sqrt(((x - mu[:, None]) ** 2).sum(axis=1) / (n - 1))
    b = aw * 2.0 / c * (sd0 + 1e-8 - s_std) / ((n - 1) * sd0)
    a = aw * 2.0 / (c * n) * (mu - s_mean) - b * mu
    _close(R.grad_gemm(D, a, b, 2.0 * cw / (c * n), x, content),
           R.node_grad(x, s_gram=s_gram, s_mean=s_mean, s_std=s_std, content=content, gw=gw, aw=aw, cw=cw))


def test_constant_channel_takes_no_std_gradient():
    x = np.vstack([np.full(6, 2.5), np.arange(6.0)])
    g = R.mean_std_grad(x, np.array([1.0, 1.0]), np.array([1.0, 1.0]))
    assert np.array_equal(g[0], np.full(6, 1.0 / 6)) and np.isfinite(g).all()
    assert R.mean_std(x)[1][0] == 1e-8


# ---- the fp32 restatement ---------------------------------------------------------------------------------------------------------------
def test_fp32_restatement_is_close_to_float64_and_has_sign_zero():
    rng = np.random.default_rng(5)
    x, gt, m = rng.random((3, 9, 8), dtype=np.float32), rng.random((3, 9, 8), dtype=np.float32), (rng.random((9, 8)) > 0.5).astype(np.float32)
    gt[0, 0, :4] = x[0, 0, :4]                                     # sign(0) = 0
    for kind, aux, ref, gref in ((R.MASKED, m, R.masked_l1, R.masked_l1_grad), (R.WEIGHTED, m, R.weighted_l1, R.weighted_l1_grad)):
        assert abs(float(R.pixel_value(kind, x, gt, aux)) - ref(_f64(x), _f64(gt), _f64(aux))) < 1e-6
        g = R.pixel_grad(kind, x, gt, aux)
        assert g.dtype == np.float32 and not g[0, 0, :4].any()
        assert np.abs(g - gref(_f64(x), _f64(gt), _f64(aux))).max() < 1e-8
    assert abs(float(R.pixel_value(R.L2, x, gt)) - R.l2(_f64(x), _f64(gt))) < 1e-7
    assert np.abs(R.pixel_grad(R.L2, x, gt) - R.l2_grad(_f64(x), _f64(gt))).max() < 1e-8
    planes = rng.integers(0, 256, size=(3, 4, 5), dtype=np.uint8)
    assert R.byte_gt(planes).dtype == np.float32 and np.array_equal(R.byte_gt(planes), (planes.astype(np.float64) / 255).astype(np.float32))


# ---- the statistics' accuracy claim -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 257, 32400, 2 ** 22])
def test_two_pass_statistics_keep_their_error_below_2_to_minus_30(n):
    """two passes in float64 in the kernel's summation order, at |mean| = 2^10 * std: relative to std, the mean and the standard
    deviation are within 2^-30 of the extended-precision values"""
    rng = np.random.default_rng(n)
    row = (rng.normal(size=n) + 1024.0).astype(np.float32)
    ld = row.astype(np.longdouble)
    mean_ref = ld.sum() / n
    sd_ref = np.sqrt(((ld - mean_ref) ** 2).sum() / (n - 1))
    assert abs(float(mean_ref)) >= 2 ** 9.9 * float(sd_ref) or n < 10
    mean, sd = R.emulated_mean_sd(row)
    assert abs(np.longdouble(mean) - mean_ref) <= 2.0 ** -30 * sd_ref
    assert abs(np.longdouble(sd) - sd_ref) <= 2.0 ** -30 * sd_ref


# ---- the case plan of the GPU test meets every class of the kernels' tiling --------------------------------------------------------------------
def test_gram_case_plan_meets_every_class():
    cs, ns = {c for c, _ in R.GRAM_CASES}, {n for _, n in R.GRAM_CASES}
    for edge in (R.MFMA_BLOCK, R.GR_TILE):                          # C below, at and above an MFMA block and a workgroup tile
        assert {edge - 1, edge, edge + 1} <= cs
    assert {1, 64, 65, 512} <= cs
    assert {1, 2, 3} <= ns
    assert {R.GR_KT - 1, R.GR_KT, R.GR_KT + 1} <= ns                # the staging tile
    assert {R.GR_CHAIN - 1, R.GR_CHAIN, R.GR_CHAIN + 1} <= ns       # one chain
    assert any(R.gram_plan(c, n)[3] == 3 and n == 2 * R.GR_CHAIN + 1 for c, n in R.GRAM_CASES)      # two slices + 1
    # a diagonal and an off-diagonal workgroup tile, and inside a diagonal tile an off-diagonal MFMA block
    assert any(R.gram_tiles(c) == 1 for c in cs) and any(R.gram_tiles(c) > 1 for c in cs) and any(R.MFMA_BLOCK < c <= R.GR_TILE for c in cs)
    # the slice cap: more chains than slices (several chains per slice), at one, three and ten tiles
    assert {R.gram_tiles(c) for c, _ in R.GRAM_CAP_CASES} == {1, 3, 10}
    for c, n in R.GRAM_CAP_CASES:
        tiles, nchain, cps, s = R.gram_plan(c, n)
        assert nchain > R.gram_slice_cap(c) and cps >= 2 and s <= R.gram_slice_cap(c) and tiles * s <= R.GR_SLICE_BUDGET
    # every case keeps the plan's invariants: every chain belongs to exactly one slice
    for c, n in R.GRAM_CASES + R.GRAM_CAP_CASES:
        tiles, nchain, cps, s = R.gram_plan(c, n)
        assert (s - 1) * cps < nchain <= s * cps and s <= R.gram_slice_cap(c)


def test_gram_workspace_is_bounded():
    assert R.gram_ws_bytes(512, 2 ** 21) < 64 * 2 ** 20
    for c in (1, 64, 128, 129, 256, 384, 385, 512):
        assert R.gram_ws_bytes(c, 2 ** 31 - 1) < 64 * 2 ** 20


def test_plans_equal_the_library():
    """the restated constants are the library's: the workspace of trase_style_ws_bytes is what the restated plan gives"""
    from trase_amd import _lib
    lib = _lib.load()

    def up(b):
        return -(-b // 256) * 256
    for c, n in [(1, 1), (31, 33), (129, 5000), (512, 32400), (64, 960 * 1280), (512, 2 ** 21)] + R.GRAM_CAP_CASES:
        got = C.c_size_t()
        assert lib.trase_style_ws_bytes(c, n, C.byref(got)) == 0
        ss = R.st_slices(n)
        want = (up(R.gram_ws_bytes(c, n)) + 2 * up(8 * c * ss) + 2 * up(8 * c) + up(4 * c * c) + 2 * up(4 * c) + up(16 * R.PX_WG_MAX) + up(16) + up(8 * -(-c * c // R.GD_PER)))
        assert got.value == want, (c, n)
    got = C.c_size_t()
    assert lib.trase_pixel_loss_ws_bytes(C.byref(got)) == 0 and got.value == up(16 * R.PX_WG_MAX) + up(16)


def test_pixel_and_statistics_case_plans():
    nb = [R.px_blocks(c * h * w) for c, h, w in R.PIXEL_SHAPES]
    assert nb[0] == 1 and max(nb) > 1                              # one workgroup and several
    assert any((c * h * w) % 256 for c, h, w in R.PIXEL_SHAPES) and any(w % 16 for _, _, w in R.PIXEL_SHAPES)
    assert R.px_blocks(3 * 1080 * 1920) == R.PX_WG_MAX
    assert {255, 256, 257} <= set(R.STATS_N) and 2 in R.STATS_N and any(R.st_slices(n) > 1 for n in R.STATS_N)
    assert {1, 3, 64, 512} == set(R.STATS_C)
    assert [c for c, _, _ in R.NODE_SHAPES] == [64, 128, 256, 512]


def test_lattice_premises_hold():
    """every sum of the exact cases stays below 2^24 in int64: the fp32 result is the integer"""
    big = 2 ** 24
    for c, n in R.GRAM_CASES + R.GRAM_CAP_CASES:
        assert np.int64(R.LATTICE) ** 2 * n < big
    x = R.lattice_rows(33, R.GR_CHAIN + 1, 0).astype(np.int64)
    assert np.abs(x).max() == R.LATTICE and np.abs(x @ x.T).max() <= R.LATTICE ** 2 * (R.GR_CHAIN + 1) < big
    # the gradient GEMM's exact case: D from {-2 .. 2}, x from the lattice, a, b, c small integers: C <= 512
    assert 2 * 512 * 2 * R.LATTICE + 8 + 8 * R.LATTICE + 4 * 2 * R.LATTICE < big
    # the pixel cases: images and masks from {0 .. 7}
    assert max(c * h * w for c, h, w in R.PIXEL_SHAPES) * 7 * 7 < big


def test_error_bounds_come_from_the_constants():
    assert R.gamma(R.GR_CHAIN + 1) == (R.GR_CHAIN + 1) * R.U / (1 - (R.GR_CHAIN + 1) * R.U)
    x = np.random.default_rng(0).normal(size=(4, 50))
    want = R.gamma(R.GR_CHAIN + 1) * np.einsum("ik,jk->ij", np.abs(x), np.abs(x))
    assert np.allclose(R.gram_bound(x), want, rtol=1e-13, atol=0)


# ---- refusals of the entry points: before a device is touched (the pointers below are never followed) --------------------------------------
P = C.c_void_p(0x1000)
INVALID, WORKSPACE = -1, -3


def _lib_():
    from trase_amd import _lib
    return _lib.load()


def test_pixel_loss_refusals():
    lib = _lib_()
    ws = 1 << 20

    def fwd(x=P, gt=P, pitch=0, c=3, h=4, w=5, kind=2, aux=None, ak=0, out=P, wsp=P, wsb=ws):
        return lib.trase_pixel_loss_forward(x, gt, pitch, c, h, w, kind, aux, ak, out, wsp, wsb, 0, None)

    def bwd(x=P, gt=P, pitch=0, c=3, h=4, w=5, kind=2, aux=None, ak=0, g=P, wsp=P, wsb=ws, dx=P):
        return lib.trase_pixel_loss_backward(x, gt, pitch, c, h, w, kind, aux, ak, g, wsp, wsb, dx, 0, None)
    assert lib.trase_pixel_loss_ws_bytes(None) == INVALID
    for f in (fwd, bwd):
        assert f(x=None) == INVALID and f(gt=None) == INVALID and f(wsp=None) == INVALID
        assert f(c=0) == INVALID and f(h=0) == INVALID and f(w=-1) == INVALID and f(c=2, h=1 << 15, w=1 << 15) == INVALID
        assert f(kind=3) == INVALID and f(kind=-1) == INVALID
        assert f(kind=2, aux=P, ak=2) == INVALID                      # l2 takes no aux
        assert f(kind=0) == INVALID and f(kind=0, aux=P, ak=3) == INVALID and f(kind=0, aux=P, ak=0) == INVALID      # masked: u8 or (H,W) f32
        assert f(kind=1) == INVALID and f(kind=1, aux=P, ak=1) == INVALID      # weighted: fp32 only
        assert f(pitch=16, c=1) == INVALID and f(pitch=8, w=5) == INVALID and f(pitch=16, w=17) == INVALID
        assert f(pitch=16, gt=C.c_void_p(0x1004)) == INVALID
        assert f(wsb=64) == WORKSPACE
        assert b"workspace too small" in lib.trase_last_error()
    assert fwd(out=None) == INVALID and bwd(g=None) == INVALID and bwd(dx=None) == INVALID


def test_style_refusals():
    lib = _lib_()
    n_ = C.c_size_t()
    ws = 1 << 30
    assert lib.trase_style_ws_bytes(8, 10, None) == INVALID
    for c, n in ((0, 10), (513, 10), (8, 0), (8, 2 ** 31)):
        assert lib.trase_style_ws_bytes(c, n, C.byref(n_)) == INVALID
        assert lib.trase_gram_matrix(P, c, n, P, P, ws, 0, None) == INVALID
        assert lib.trase_mean_std(P, c, n, 1e-8, P, P, P, ws, 0, None) == INVALID
        assert lib.trase_style_node_forward(P, c, n, P, P, P, P, 1.0, 1.0, 1.0, P, P, P, ws, 0, None) == INVALID
        assert lib.trase_style_grad_gemm(P, P, P, 0.0, P, P, c, n, None, P, 0, None) == INVALID
    assert lib.trase_mean_std(P, 8, 1, 1e-8, P, P, P, ws, 0, None) == INVALID          # the unbiased std needs two positions
    assert lib.trase_style_node_forward(P, 8, 1, P, P, P, P, 0.0, 1.0, 0.0, P, P, P, ws, 0, None) == INVALID
    for args in ((None, P, P), (P, None, P), (P, P, None)):
        assert lib.trase_gram_matrix(args[0], 8, 10, args[1], args[2], ws, 0, None) == INVALID
    for k in range(4):
        a = [P] * 4
        a[k] = None
        assert lib.trase_mean_std(a[0], 8, 10, 1e-8, a[1], a[2], a[3], ws, 0, None) == INVALID
    assert lib.trase_gram_matrix(P, 8, 10, P, P, 64, 0, None) == WORKSPACE
    assert lib.trase_mean_std(P, 8, 10, 1e-8, P, P, P, 64, 0, None) == WORKSPACE
    assert lib.trase_style_node_forward(P, 8, 10, P, P, P, P, 1.0, 1.0, 1.0, P, P, P, 64, 0, None) == WORKSPACE

    def node(x=P, sg=P, sm=P, ss=P, y=P, w=(1.0, 1.0, 1.0), out=P, saved=P, wsp=P, c=8, n=10):
        return lib.trase_style_node_forward(x, c, n, sg, sm, ss, y, w[0], w[1], w[2], out, saved, wsp, ws, 0, None)
    assert node(x=None) == INVALID and node(out=None) == INVALID and node(saved=None) == INVALID and node(wsp=None) == INVALID
    assert node(sg=None) == INVALID and node(sm=None) == INVALID and node(ss=None) == INVALID and node(y=None) == INVALID
    assert node(c=512, n=2 ** 22) == INVALID                        # the content term: C * n < 2^31
    assert lib.trase_style_grad_gemm(P, P, P, 0.0, None, P, 8, 10, None, P, 0, None) == INVALID
    assert lib.trase_style_grad_gemm(P, P, P, 0.0, P, P, 8, 10, None, None, 0, None) == INVALID
    assert lib.trase_style_grad_gemm(P, P, None, 0.0, P, P, 8, 10, None, P, 0, None) == INVALID      # a without b
    assert lib.trase_style_grad_gemm(P, None, P, 0.0, P, P, 8, 10, None, P, 0, None) == INVALID


# ---- refusals of the Python functions (shapes and types are checked before the device) -----------------------------------------------------------
def test_python_argument_checks():
    from trase_amd import losses as L
    img, gt = torch.zeros(3, 4, 5), torch.zeros(3, 4, 5)
    with pytest.raises(RuntimeError, match="GPU only"):
        L.masked_l1_loss(img, gt, torch.ones(4, 5))
    with pytest.raises(RuntimeError, match="GPU only"):
        L.weighted_l1_loss(img, gt, torch.ones(1, 4, 5))
    with pytest.raises(RuntimeError, match="GPU only"):
        L.l2_loss(torch.zeros(7), torch.zeros(7))
    with pytest.raises(RuntimeError, match="GPU only"):
        L.cal_mse_content_loss(torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2))
    for bad in (torch.ones(5, 4), torch.ones(1, 4, 5), torch.ones(3, 4, 5), "mask"):
        with pytest.raises(ValueError, match="mask"):
            L.masked_l1_loss(img, gt, bad)
    with pytest.raises(TypeError, match="bool, uint8 or float"):
        L.masked_l1_loss(img, gt, torch.ones(4, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match="equal shape"):
        L.masked_l1_loss(img, torch.zeros(3, 4, 6), torch.ones(4, 5))
    for bad in (torch.ones(5, 4), torch.ones(2, 4, 5), torch.ones(1, 1, 4, 5), None):
        with pytest.raises(ValueError, match="weight"):
            L.weighted_l1_loss(img, gt, bad)
    with pytest.raises(TypeError, match="float"):
        L.weighted_l1_loss(img, gt, torch.ones(4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="equal shape"):
        L.weighted_l1_loss(img, torch.zeros(3, 5, 5), torch.ones(4, 5))
    with pytest.raises(ValueError, match="equal shape"):
        L.l2_loss(img, torch.zeros(3, 4, 6))
    with pytest.raises(ValueError, match="equal shape"):
        L.l2_loss(torch.zeros(0), torch.zeros(0))
    for fn in (L.gram_matrix, L.calc_mean_std):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(torch.zeros(1, 8, 3, 3))
        for bad in (torch.zeros(2, 8, 3, 3), torch.zeros(8, 3, 3), torch.zeros(513, 4), torch.zeros(1, 0, 2, 2), torch.zeros(4, 0), [1.0]):
            with pytest.raises(ValueError, match="features|channels"):
                fn(bad)
    f = torch.zeros(1, 8, 3, 3)
    with pytest.raises(TypeError, match="StyleTargets"):
        L.style_statistics_loss(f, (f, f), gram_weight=1.0)
    with pytest.raises(ValueError, match="every weight is 0"):
        L.style_statistics_loss(f, L.StyleTargets())
    with pytest.raises(RuntimeError, match="GPU only"):
        L.style_statistics_loss(f, L.StyleTargets(gram=torch.zeros(8, 8)), gram_weight=1.0)
    with pytest.raises(ValueError, match="features"):
        L.style_statistics_loss(torch.zeros(8, 3, 3), L.StyleTargets(), gram_weight=1.0)
    with pytest.raises(ValueError, match="features"):
        L.cal_style_loss(torch.zeros(8, 3, 3), f, 1.0)
    with pytest.raises(ValueError, match="pair"):
        L.cal_adain_style_loss(f, (f, f, f))


def test_the_new_names_are_declared_bound_and_exported():
    from trase_amd import _lib, losses as L
    names = ("trase_pixel_loss_ws_bytes", "trase_pixel_loss_forward", "trase_pixel_loss_backward", "trase_style_ws_bytes", "trase_gram_matrix",
             "trase_mean_std", "trase_style_node_forward", "trase_style_grad_gemm")
    header = open(os.path.join(os.path.dirname(HERE), "include", "trase_rast.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for n in names:
        assert n + "(" in header and n in bound and hasattr(lib, n)
    for n in ("masked_l1_loss", "weighted_l1_loss", "l2_loss", "calc_mean_std", "gram_matrix", "cal_adain_style_loss", "cal_style_loss",
              "cal_mse_content_loss", "style_statistics_loss", "StyleTargets"):
        assert callable(getattr(L, n))
    assert (L.PIXEL_MASKED_L1, L.PIXEL_WEIGHTED_L1, L.PIXEL_L2) == (R.MASKED, R.WEIGHTED, R.L2)
    for line in ("#define TRASE_PIXEL_MASKED_L1 0", "#define TRASE_PIXEL_WEIGHTED_L1 1", "#define TRASE_PIXEL_L2 2", "#define TRASE_PIXEL_AUX_U8 1",
                 "#define TRASE_PIXEL_AUX_F32 2", "#define TRASE_PIXEL_AUX_F32_FULL 3"):
        assert line in header
