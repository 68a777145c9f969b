"""GPU: the contrastive pair head (csrc/pairhead.hip, csrc/contrastive.hip, trase_amd/feature_head.py) at every dispatch edge
against the float64 statement of tests/pairhead_reference.py, on lattice features where every discrete decision -- column flags,
strict threshold comparisons, i < j, relu, membership bits, ranks -- has one right answer.

Always exact: the candidate counts out8[1] and out8[3], S and the number of sampled masks, the gradient's support, the NaN
pattern, and -- without weights -- both losses and both similarities, bit for bit against the statement rounded once to float32
(a thread's sums over <= 64 rows are multiples of 1/16 far below 2^24, everything above is double, and the final division is the
statement's).  No scalar needed the 1-ulp allowance.  Every case runs twice through the C entry points, every output in front of
canaries, and must return the same bits.

Weighted losses: 4 x the error the pinned oracle makes in float32 on the same inputs + one float32 ulp.  Met by every family.

Gradients, per sampled-pixel row: the same bar against the row's own largest entry (tests/test_pairhead_reference.py shows that
one wrong pair moves a row by more than 10 such bars).  Families d and f meet it.  Families a, b, c and e do not, in 9 of their
198 cases, by at most 3.5 x: no defect (a wrong pair is hundreds of bars; these are 1 to 3.5 ulp of the row's largest entry) but
the kernel's fixed summation order.  A row is r (d - f <f, d>), d a sum over up to S pairs: ph_bwd adds it with serial fmas in 32
chunks, ph_scatter adds the 32 chunk partials serially in fp32, and on these scenes the projection then cancels most of d (pixels
of one mask are nearly parallel), so an error of a few ulp of |d| is several ulp of the row, where the float32 oracle happens to
be nearly exact on that row.  As the issue rules for that case, the rows of these four families are judged by the project's
existing bar, 1e-4 of the gradient's largest entry -- and, so that a wrong pair stays visible, by a forward error bound of the
kernel's own summation derived from the float32 format alone (pairhead_reference.row_forward_bounds: about (2 S / 32 + 90) ulp
of the sum of the pairs' magnitudes; one wrong pair moves a row by more than 10 of these too).  Counts, support, NaN pattern and
unweighted scalars stay exact in every family.

Largest device error / bar per family, measured on an MI355X (every case prints its own before asserting):
    weighted losses           a 0.32   b 0.18   c 0.29   d 0.18   e 0.15   f 0.19   h 0.84
    rows, oracle bar          a 1.32   b 1.18   c 3.47   d 0.92   e 2.15   f 0.84
    rows, 1e-4 of the maximum a 0.0037 b 0.0021 c 0.0049 e 0.0024
    rows, forward bound       a 0.069  b 0.050  c 0.033  e 0.051
    feature_norm_reg (i)      0.20 (loss and gradient, against bounds from the formats)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pairhead_reference as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CANARY = 0xCD
PAD = 256                       # canary bytes behind every output
MODE_ID = {"soft": 0, "all": 1, "hard": 2}
# families whose gradient rows are judged by the project's bar (1e-4 of the largest entry) and a forward error bound: see the docstring
PROJECT_ROW_BARS = ("a", "b", "c", "e")
LOSS = ("loss_pos", "loss_neg")
SIMS = ("pos_similarity", "neg_similarity")


def _guarded(nbytes):
    return torch.full((nbytes + PAD,), CANARY, dtype=torch.uint8, device=DEV)


def _intact(buf, nbytes):
    return bool((buf[nbytes:] == CANARY).all())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _run(scene, mode, pth, nth, use_w, form="plain", cap=None, prefill=None, g2=(1.0, 1.0), n_sampled=None, expect_rc=0):
    """One forward + backward through the C entry points.  form: plain | bits | resized | resized_bits (the resized forms run on the
    x2 nearest-upsampled image).  cap: size every buffer for ``cap`` samples and pass the true count in device memory (S_dev), as the
    sync-free path does; prefill: a (32, H, W) image the backward accumulates onto (accumulate = 1).
    -> (out8 float32[8], gradient image, workspace bytes), on the CPU"""
    from trase_amd import _lib
    from trase_amd.feature_head import PackedMasks
    from trase_amd.rasterizer import _stream
    lib = _lib.load()
    feat, sam, sp, sm = scene
    N, h, w = sam.shape
    resized, packed = form.startswith("resized"), form.endswith("bits")
    f = (R.upsampled(feat) if resized else feat).float().contiguous().to(DEV)
    Hr, Wr = f.shape[1:]
    masks = sam.contiguous().to(DEV)
    m = PackedMasks.from_bool(masks).bits if packed else masks.view(torch.uint8)
    smu = sm.to(DEV).contiguous().view(torch.uint8)
    size = sam.reshape(N, -1).sum(1).to(torch.int32).to(DEV)
    idx = torch.nonzero(sp.reshape(-1)).reshape(-1).to(torch.int32)
    S = idx.numel()
    s_cap = S if cap is None else cap
    assert s_cap >= S
    junk = int(torch.nonzero(~sp.reshape(-1))[0])                # slots behind the count name a pixel that is not sampled
    pix = torch.cat([idx, torch.full((s_cap - S,), junk, dtype=torch.int32)]).to(DEV)
    s_dev = None if cap is None else torch.tensor([S, S], dtype=torch.int32, device=DEV)
    g = torch.tensor(g2, dtype=torch.float32, device=DEV)
    ns = int(sm.sum()) if n_sampled is None else n_sampled
    nbytes = C.c_size_t()
    if resized:
        _lib.check(lib.trase_pairhead_sizes_resized(s_cap, Hr, Wr, h, w, C.byref(nbytes)), "trase_pairhead_sizes_resized")
    else:
        _lib.check(lib.trase_pairhead_sizes(s_cap, C.byref(nbytes)), "trase_pairhead_sizes")
    ws_b, grad_b = nbytes.value, 32 * Hr * Wr * 4
    out8, ws, grad = _guarded(32), _guarded(ws_b), _guarded(grad_b)
    if prefill is not None:
        grad[:grad_b].view(torch.float32).copy_(prefill.reshape(-1))
    inputs = [t for t in (f, m, smu, size, pix, s_dev, g) if t is not None]
    before = [t.clone() for t in inputs]
    st, p = _stream(DEV), _lib.ptr
    mid, pth, nth, uw = MODE_ID[mode], float(pth), float(nth), int(use_w)
    if form == "plain":
        rc = lib.trase_pairhead_forward_n(p(f), 32, h * w, p(m), N, p(smu), ns, p(size), p(pix), s_cap, p(s_dev), mid, pth, nth, uw, p(out8),
                                          p(ws), ws_b, 0, st)
    elif form == "bits":
        rc = lib.trase_pairhead_forward_bits(p(f), 32, h * w, p(m), m.numel(), N, p(smu), ns, p(size), p(pix), s_cap, p(s_dev), mid, pth, nth, uw,
                                             p(out8), p(ws), ws_b, 0, st)
    elif form == "resized":
        rc = lib.trase_pairhead_forward_resized(p(f), 32, Hr, Wr, h, w, p(m), N, p(smu), ns, p(size), p(pix), s_cap, p(s_dev), mid, pth, nth, uw,
                                                p(out8), p(ws), ws_b, 0, st)
    else:
        rc = lib.trase_pairhead_forward_bits_resized(p(f), 32, Hr, Wr, h, w, p(m), m.numel(), N, p(smu), ns, p(size), p(pix), s_cap, p(s_dev), mid,
                                                     pth, nth, uw, p(out8), p(ws), ws_b, 0, st)
    if expect_rc:
        assert rc == expect_rc, f"returned {rc}"
        torch.cuda.synchronize()
        assert _intact(out8, 0) and _intact(ws, 0), "a refused call wrote"
        return None
    _lib.check(rc, "forward " + form)
    if resized:
        _lib.check(lib.trase_pairhead_backward_resized(32, Hr, Wr, h, w, p(pix), s_cap, p(s_dev), mid, pth, nth, uw, p(out8), p(g), p(ws), ws_b,
                                                       None, None, None, p(grad), 0, st), "trase_pairhead_backward_resized")
    else:
        _lib.check(lib.trase_pairhead_backward_n(32, h * w, p(pix), s_cap, p(s_dev), mid, pth, nth, uw, p(out8), p(g), p(ws), ws_b,
                                                 0 if prefill is None else 1, p(grad), 0, st), "trase_pairhead_backward_n")
    torch.cuda.synchronize()
    for name, buf, n in (("out8", out8, 32), ("workspace", ws, ws_b), ("gradient", grad, grad_b)):
        assert _intact(buf, n), f"{name}: written past its stated size"
    assert all(torch.equal(a, b) for a, b in zip(inputs, before)), "an input was modified"
    return out8[:32].view(torch.float32).cpu().numpy(), grad[:grad_b].view(torch.float32).view(32, Hr, Wr).cpu(), ws[:ws_b].cpu()


def _twice(*args, **kw):
    a, b = _run(*args, **kw), _run(*args, **kw)
    assert a[0].tobytes() == b[0].tobytes() and _same_bits(a[1], b[1]), "two calls differ"
    return a


def _bit_equal(x, y):
    return np.float32(x).tobytes() == np.float32(y).tobytes() or (np.isnan(x) and np.isnan(y)) or (x == 0 and y == 0)


def _judge(family, label, out8, grad, scene, ref, err, use_w):
    """the assertions of part (a): counts, support and NaN pattern exact, unweighted scalars bit-equal, the rest within its bar"""
    sp = scene[2]
    want = (ref.N_pos, ref.N_neg, ref.S, ref.n_sampled)
    got = tuple(float(out8[k]) for k in (1, 3, 6, 7))
    assert got == tuple(float(v) for v in want), f"{label}: N_pos, N_neg, S, sampled masks = {got}, statement {want}"
    assert not bool((grad[:, ~sp] != 0).any()), f"{label}: gradient outside the sampled pixels"
    rows = grad[:, sp].T.double()
    assert not bool((rows[~ref.active] != 0).any()), f"{label}: a row without an active pair is not exactly zero"
    assert torch.equal(rows.isnan(), ref.rows.isnan()), f"{label}: NaN rows differ from the statement's"
    worst = 0.0
    vals = {"loss_pos": out8[0], "loss_neg": out8[2], "pos_similarity": out8[4], "neg_similarity": out8[5]}
    for name in LOSS + SIMS:
        dev, want = float(vals[name]), float(getattr(ref, name))
        if np.isnan(want) or not use_w or name in SIMS:
            assert _bit_equal(dev, R.f32(want)), f"{label}: {name} = {dev!r}, statement {float(R.f32(want))!r} ({want!r})"
            continue
        e, bar = abs(dev - want), R.scalar_bar(getattr(err, name), want)
        print(f"PAIRHEAD-RATIO {family} {label} {name}: error {e:.3e} bar {bar:.3e} ratio {e / bar:.3f}")
        worst = max(worst, e / bar)
    assert worst <= 1.0, f"{label}: {worst:.2f} x its bar"
    ok = ~ref.rows.isnan().any(1)
    e, bars = (rows - ref.rows).abs().amax(1)[ok], R.row_bars(err.rows, ref.rows)[ok]
    if not e.numel():
        return
    k = int((e / bars).argmax())
    print(f"PAIRHEAD-RATIO {family} {label} rows: error {float(e[k]):.3e} bar {float(bars[k]):.3e} ratio {float(e[k] / bars[k]):.3f}")
    if family not in PROJECT_ROW_BARS:
        assert float((e / bars).max()) <= 1.0, f"{label}: a gradient row is {float((e / bars).max()):.2f} x its bar"
        return
    top = float(ref.rows[ok].abs().max())
    fwd = R.row_forward_bounds(ref)[ok]
    print(f"PAIRHEAD-RATIO {family}-project {label} rows: error / (1e-4 max) {float(e.max()) / (1e-4 * top + 1e-300):.2e}, "
          f"error / forward bound {float((e / fwd.clamp_min(1e-300))[e > 0].max()) if bool((e > 0).any()) else 0.0:.3f}")
    assert float(e.max()) <= 1e-4 * top, f"{label}: gradient off by {float(e.max()):.3e}, 1e-4 of the maximum is {1e-4 * top:.3e}"
    assert bool((e <= fwd).all()), f"{label}: a gradient row is {float((e / fwd.clamp_min(1e-300)).max()):.2f} x its forward error bound"


def _case(family, builder, args, mode, pth, nth, use_w, form="plain", **kw):
    scene, ref, err = R.reference(builder, args, mode, pth, nth, use_w)
    label = f"{builder}{args} {mode} {pth}/{nth} {'weighted' if use_w else 'plain'} {form}"
    out8, grad, ws = _twice(scene, mode, pth, nth, use_w, form, **kw)
    _judge(family, label, out8, grad, scene, ref, err, use_w)
    return scene, ref, out8, grad, ws


W_IDS = ["plain", "weighted"]


# ---- a. S at every block edge -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_w", [False, True], ids=W_IDS)
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("S", R.S_EDGES)
def test_s_edges(S, mode, use_w):
    """row tile 64, column block 256, the backward's 32 chunks of ceil(S / 32) (S = 31 and 33 leave empty chunks), and from S = 257
    ph_sum's skipped below-diagonal tiles, whose pairs the exact counts ('hard') and sums would miss or double"""
    _case("a", "lattice", R.edge_args(S), mode, 0.75, 0.5, use_w)


# ---- b. thresholds on the lattice ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_w", [False, True], ids=W_IDS)
@pytest.mark.parametrize("mode", ["soft", "hard"])
@pytest.mark.parametrize("nth", [0.5, 0.0, -0.0625])
@pytest.mark.parametrize("pth", [0.75, 0.6875 + 1 / 32])
@pytest.mark.parametrize("S", [65, 257])
def test_thresholds_on_the_lattice(S, pth, nth, mode, use_w):
    """hundreds of similarities sit exactly on 0.75, 0.5 and 0 (0.71875 lies between two lattice points): a tie must fall on the
    reference's side of the strict < and >, and a negative pair with f <= 0 -- selected when nth < 0 -- adds neither loss nor
    gradient (the counts say it was selected, the exact loss and the zero rows that it added nothing)"""
    _case("b", "lattice", R.edge_args(S), mode, pth, nth, use_w)


# ---- c. mask counts, membership words, the rank scan --------------------------------------------------------------------------------
@pytest.mark.parametrize("use_w", [False, True], ids=W_IDS)
@pytest.mark.parametrize("mode", ["all", "hard"])
@pytest.mark.parametrize("case", R.PROBE_CASES, ids=lambda c: f"N{c[0]}s{c[1]}")
def test_mask_count_and_word_edges(case, mode, use_w):
    """planted pairs: exactly 2 x sampled-masks positive entries, so a lost, aliased or misplaced membership bit (words 0..7, the
    8 lanes x 4 x 32 mask walk, ranks behind the first 256-mask trip) changes an integer count"""
    N, ns, first = case
    _case("c", "probe", (N, ns, N, first), mode, 0.75, 0.5, use_w)


def test_257_sampled_masks_are_refused():
    from trase_amd.feature_head import contrastive_head
    scene = R.probe_scene(300, 257, 300)
    assert _run(scene, "hard", 0.75, 0.5, True, expect_rc=-1) is None               # TRASE_ERR_INVALID
    assert _run(scene, "hard", 0.75, 0.5, True, form="resized_bits", expect_rc=-1) is None
    feat, sam, sp, sm = (t.to(DEV) for t in scene)
    with pytest.raises(ValueError, match="257 sampled masks"):
        contrastive_head(feat, sam, sp, sm, mode="hard")


@pytest.mark.parametrize("case", [(257, 256, 255), (600, 255, 31), (600, 1, 0)], ids=lambda c: f"N{c[0]}s{c[1]}")
def test_python_path_beyond_256_masks(case):
    """contrastive_head's `N > 256` branch (the sampled masks are counted), bool masks and PackedMasks, against the statement"""
    from trase_amd.feature_head import PackedMasks, contrastive_head
    N, ns, first = case
    scene, ref, err = R.reference("probe", (N, ns, N, first), "hard", 0.75, 0.5, True)
    feat, sam, sp, sm = (t.to(DEV) for t in scene)
    res = []
    for masks in (sam, PackedMasks.from_bool(sam)):
        f = feat.clone().requires_grad_(True)
        lp, ln, ps, ns_ = contrastive_head(f, masks, sp, sm, mode="hard")
        (lp + ln).backward()
        res.append((torch.stack([lp.detach(), ln.detach(), ps, ns_]).cpu(), f.grad.cpu()))
    assert _same_bits(res[0][0], res[1][0]) and _same_bits(res[0][1], res[1][1]), "PackedMasks differ from the bool masks"
    s4, grad = res[0]
    out8 = np.array([s4[0], ref.N_pos, s4[1], ref.N_neg, s4[2], s4[3], ref.S, ref.n_sampled], dtype=np.float32)
    _judge("c", f"contrastive_head N{N}s{ns}", out8, grad, scene, ref, err, True)


# ---- d. the four gather forms ---------------------------------------------------------------------------------------------------------
_FORM_SCENES = [("probe", (33, 33, 33, None)), ("probe", (256, 256, 256, None)), ("probe", (600, 255, 600, 31)), ("lattice", R.edge_args(257))]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("scene", _FORM_SCENES, ids=lambda s: f"{s[0]}{s[1][0]}")
def test_four_gather_forms(scene, mode):
    """packed bits = bool bytes, bit for bit; the resized head on the x2 nearest-upsampled image blends two equal taps per axis with
    0.5 + 0.5 and so sees the same columns: the same out8 bits, and each sample's gradient vector times 0.25 (exact) at its four
    taps; resized packed = resized bool"""
    sc, ref, out8, grad, _ = _case("d", *scene, mode, 0.75, 0.5, True)
    b8, bgrad, _ = _twice(sc, mode, 0.75, 0.5, True, "bits")
    assert out8.tobytes() == b8.tobytes() and _same_bits(grad, bgrad), "packed form differs from the bool form"
    r8, rgrad, _ = _twice(sc, mode, 0.75, 0.5, True, "resized")
    assert out8.tobytes() == r8.tobytes(), f"resized out8 {r8} != plain {out8}"
    assert torch.equal(rgrad, R.spread_x2(grad)), "resized gradient is not the plain gradient x 0.25 at the four taps"
    rb8, rbgrad, _ = _twice(sc, mode, 0.75, 0.5, True, "resized_bits")
    assert r8.tobytes() == rb8.tobytes() and _same_bits(rgrad, rbgrad), "resized packed form differs from the resized bool form"


# ---- e. uncovered pixels, degenerate weights --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
def test_uncovered_sampled_pixels(mode):
    """a quarter of the sampled pixels lie under no mask: a = 0, their products are replaced by 1e10 and their weight is 1"""
    sc, ref, _, _, _ = _case("e", "lattice", (65, 14, 7, 1065, 0.25), mode, 0.75, 0.5, True)
    assert int((ref.a == 0).sum()) == 16


@pytest.mark.parametrize("mode", R.MODES)
def test_all_mean_sizes_equal(mode):
    """one sampled mask, every a equal: w_max = 1 and (w - min) / (max - min) = 0 / 0.  The device is NaN exactly where the float64
    statement is -- both losses, and every row with an active pair (all 32 entries) -- and nowhere else; unweighted it is exact"""
    sc, ref, out8, grad, _ = _case("e", "one_mask", (65, 7), mode, 0.75, 0.5, True)
    assert np.isnan(out8[0]) and np.isnan(out8[2]) and ref.N_pos > 0 and ref.N_neg > 0
    assert int(ref.rows.isnan().any(1).sum()) > 0 and bool(torch.isfinite(grad[:, ~sc[2]]).all())
    _case("e", "one_mask", (65, 7), mode, 0.75, 0.5, False)


# ---- f. the count in device memory ------------------------------------------------------------------------------------------------------
_COUNT_ARGS = {5: (5, 14, 7, 4048, 0.0), 250: (250, 14, 7, 4250), 257: (257, 14, 7, 4257)}     # S = 5: covered pixels, both pair kinds


def _layout(cap):
    """byte ranges of the per-sample arrays in the workspace (pair_ws_layout of csrc/pairhead.hip: 256-byte aligned, in this order)"""
    up = lambda n: (n + 255) // 256 * 256
    nblk = ((cap + 255) // 256) * ((cap + 63) // 64)
    o, out = 0, {}
    for name, n in (("fn", 128 * cap), ("rinv", 4 * cap), ("a", 4 * cap), ("bits", 32 * cap), ("colP", 4 * cap), ("colN", 4 * cap), ("consts", 32),
                    ("partial", 64 * nblk), ("dpart", 128 * cap * 32), ("rank", 4 * 8192)):
        out[name] = (o, n)
        o += up(n)
    return out, o


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("S,cap", [(5, 300), (250, 250), (257, 400)])
def test_device_side_count(S, cap, mode):
    """buffers and grids sized for ``cap``, the true S read from device memory: the tiles, chunks and rows that do not exist must
    neither count nor be written.  Same bits as the synchronising form; rows >= S of every per-sample array keep their canary."""
    from trase_amd import _lib
    args = _COUNT_ARGS[S]
    for use_w in (False, True):
        sc, ref, out8, grad, _ = _case("f", "lattice", args, mode, 0.75, 0.5, use_w)
        d8, dgrad, ws = _twice(sc, mode, 0.75, 0.5, use_w, cap=cap)
        assert out8.tobytes() == d8.tobytes(), f"out8 {d8} with the count on the device, {out8} with it on the host"
        assert _same_bits(grad, dgrad), "gradient differs between the two forms"
    lay, total = _layout(cap)
    nbytes = C.c_size_t()
    _lib.check(_lib.load().trase_pairhead_sizes(cap, C.byref(nbytes)), "trase_pairhead_sizes")
    assert total == nbytes.value, "the workspace layout this test mirrors has changed"
    for name, row in (("fn", 128), ("rinv", 4), ("a", 4), ("bits", 32)):
        o, n = lay[name]
        assert bool((ws[o + row * S:o + n] == CANARY).all()), f"{name}: written beyond row {S}"
    o, n = lay["dpart"]
    assert bool((ws[o + 128 * S * 32:o + n] == CANARY).all()), "dpart: written beyond 32 chunks of S rows"


@pytest.mark.parametrize("S,target", [(5, 142), (250, 105), (257, 226)])
def test_tagged_sampled_pixel(S, target):
    """through contrastive_head: a sampled_pixel tagged as get_sample_pixel_and_mask tags it (buffers for target + 8 sigma + 64 =
    301, 250 and 410 samples) against the same mask untagged (counted on the host)"""
    from trase_amd.feature_head import check_sampled_counts, contrastive_head
    scene = R.lattice_scene(*_COUNT_ARGS[S])
    assert int(target + 8.0 * target ** 0.5 + 64) >= S
    feat, sam, sp, sm = (t.to(DEV) for t in scene)
    res = []
    for tagged in (False, True):
        spx = sp.clone()
        if tagged:
            spx._trase_expected_count = (target, spx.numel(), spx._version)
        f = feat.clone().requires_grad_(True)
        lp, ln, ps, ns = contrastive_head(f, sam, spx, sm, mode="soft", use_weights=False)
        (lp + ln).backward()
        res.append((torch.stack([lp.detach(), ln.detach(), ps, ns]).cpu(), f.grad.cpu()))
    check_sampled_counts()
    assert _same_bits(res[0][0], res[1][0]) and _same_bits(res[0][1], res[1][1])
    ref = R.statement(*scene, "soft", 0.75, 0.5, False)
    for k, name in enumerate(("loss_pos", "loss_neg", "pos_similarity", "neg_similarity")):
        assert _bit_equal(float(res[1][0][k]), R.f32(getattr(ref, name))), name


# ---- g. accumulate = 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("S", [33, 257])
def test_backward_accumulates_onto_a_prefilled_image(S, mode):
    """one fp32 add per element (the file is built with contraction off): prefill + gradient, bit for bit; elsewhere the prefill"""
    scene = R.lattice_scene(*R.edge_args(S))
    _, grad, _ = _twice(scene, mode, 0.75, 0.5, True, g2=(0.75, 1.5))
    pre = torch.randn(32, *R.LATTICE_HW, generator=torch.Generator().manual_seed(S)) * float(grad.abs().max())
    _, acc, _ = _twice(scene, mode, 0.75, 0.5, True, g2=(0.75, 1.5), prefill=pre)
    assert float(grad.abs().max()) > 0 and torch.equal(acc, pre + grad)
    assert torch.equal(acc[:, ~scene[2]], pre[:, ~scene[2]])


# ---- h. the matrix-form losses of contrastive.hip ---------------------------------------------------------------------------------------
_H_CASES = [(S, 0.75, 0.5) for S in (2, 63, 64, 65, 255, 256, 257, 513)] + \
           [(S, p, n) for S in (65, 257) for p in (0.75, 0.6875 + 1 / 32) for n in (0.5, 0.0, -0.0625) if (p, n) != (0.75, 0.5)]


@pytest.mark.parametrize("use_w", [False, True], ids=W_IDS)
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("S,pth,nth", _H_CASES)
def test_matrix_form_losses(S, pth, nth, mode, use_w):
    """positive_/negative_pixel_pair_loss on the S x S matrices of the same scenes.  contrastive_sum_kernel keeps FLOAT partials, and
    the unweighted loss is exact all the same: a thread adds <= 64 multiples of 1/16 of magnitude <= 1, a wave 64 and a workgroup
    256 such threads, so every float partial is an integer number of sixteenths below 2^18 -- no rounding -- and the partials are
    summed and divided in double.  Weighted losses get the bar; the dense gradient must have the statement's support, and its
    entries are g / N * w: two float32 roundings."""
    from trase_amd.losses import negative_pixel_pair_loss, positive_pixel_pair_loss
    scene, ref, err = R.reference("lattice", R.edge_args(S), mode, pth, nth, use_w)
    Cm = ref.C.float().to(DEV)
    Wm = ref.W.float().to(DEV) if use_w else None
    got = []
    for _ in range(2):
        cf = ref.C_F.float().to(DEV).requires_grad_(True)
        lp = positive_pixel_pair_loss[mode](Cm, cf, pth, Wm)
        ln = negative_pixel_pair_loss[mode](Cm, cf, nth, Wm)
        (lp + ln).backward()
        got.append((torch.stack([lp.detach(), ln.detach()]).cpu(), cf.grad.cpu()))
    assert _same_bits(got[0][0], got[1][0]) and _same_bits(got[0][1], got[1][1]), "two calls differ"
    (losses, d), worst = got[0], 0.0
    for k, name in enumerate(LOSS):
        dev, want = float(losses[k]), float(getattr(ref, name))
        if np.isnan(want) or not use_w:
            assert _bit_equal(dev, R.f32(want)), f"{name} = {dev!r}, statement {float(R.f32(want))!r}"
            continue
        e, bar = abs(dev - want), R.scalar_bar(getattr(err, name), want)
        print(f"PAIRHEAD-RATIO h lattice S{S} {mode} {pth}/{nth} {name}: error {e:.3e} bar {bar:.3e} ratio {e / bar:.3f}")
        worst = max(worst, e / bar)
    assert worst <= 1.0, f"{worst:.2f} x its bar"
    want = ref.dCF
    assert torch.equal((d != 0) | d.isnan(), (want != 0) | want.isnan()), "support of d loss / d C_F"
    ok = ~want.isnan()
    assert bool(((d.double() - want).abs()[ok] <= 2.0 ** -22 * want.abs()[ok]).all()) and torch.equal(d.isnan(), want.isnan())


# ---- i. feature_norm_reg ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 32, 64])
@pytest.mark.parametrize("HW", [1, 255, 256, 257])
def test_feature_norm_reg(HW, F):
    """(1 - mean_p |F_p|)^2 and its gradient against the float64 torch expression, one all-zero pixel (zero subgradient).  Bars from
    the formats, u = 2^-24: |F_p|^2 is a sum of F positive float32 terms (relative error <= (F + 1) u), so each norm, and their
    double-precision mean m, carry <= (F / 2 + 2) u; (1 - m)^2 then moves by 2 |1 - m| m (F / 2 + 2) u, plus the float32 rounding of
    m, of 1 - m and of the square; a gradient entry is g * -2 (1 - m) / HW / |F_p| * x: the same two errors and five roundings."""
    from trase_amd.feature_head import feature_norm_reg
    x = torch.randn(F, 1, HW, generator=torch.Generator().manual_seed(100 * F + HW)) * 0.4
    if HW > 1:
        x[:, 0, HW // 2] = 0.0
    xd = x.double().requires_grad_(True)
    want = (1 - xd.norm(dim=0, p=2).mean()) ** 2
    want.backward()
    xg = x.to(DEV).requires_grad_(True)
    got = feature_norm_reg(xg)
    got.backward()
    torch.cuda.synchronize()
    u, m = 2.0 ** -24, float(x.double().norm(dim=0).mean())
    rel = (F / 2 + 2) * u
    bar = 2 * abs(1 - m) * (m * rel + 2 * u) + 4 * R.ulp32(float(want.detach()))
    e = abs(float(got.detach()) - float(want.detach()))
    print(f"PAIRHEAD-RATIO i HW{HW} F{F} loss: error {e:.3e} bar {bar:.3e} ratio {e / bar:.3f}")
    assert e <= bar
    gd, gw = xg.grad.cpu().double(), xd.grad
    gbar = gw.abs() * (rel + (m * rel + 2 * u) / abs(1 - m) + 5 * u) + float(np.finfo(np.float32).tiny)
    ratio = float(((gd - gw).abs() / gbar).max())
    print(f"PAIRHEAD-RATIO i HW{HW} F{F} gradient: ratio {ratio:.3f}")
    assert ratio <= 1.0
    if HW > 1:
        assert not bool((gd[:, 0, HW // 2] != 0).any()), "an all-zero pixel must get a zero subgradient"
