"""CPU: the float64 statement of the contrastive pair head (tests/pairhead_reference.py) against the pinned oracle
(oracle/feature_head_oracle.py) and the golden vectors of the imported reference (tests/golden/feature_head.npz), and the premises
of every scene tests/test_gpu_pairhead_edges.py runs: that the features are on the lattice, that ties at both thresholds occur,
that both pair kinds are populated, that the planted pixels do what they were planted for, and that one wrongly in- or
excluded pair would move a gradient row by more than ten times its bar."""
import os

import numpy as np
import pytest
import torch

from oracle import feature_head_oracle as O
from tests import pairhead_reference as R

GOLD = os.path.join(os.path.dirname(__file__), "golden", "feature_head.npz")
LATTICE_ARGS = [R.edge_args(S) for S in R.S_EDGES]                     # the S-edge scenes of the GPU tests
UNCOVERED_ARGS = (65, 14, 7, 1065, 0.25)


# ---- the statement is the oracle's, and the reference's ------------------------------------------------------------------------
@pytest.mark.parametrize("mode,use_w", [("soft", True), ("all", True), ("hard", True), ("soft", False)])
def test_statement_matches_golden(mode, use_w):
    d = np.load(GOLD)
    sam, sp, sm = torch.from_numpy(d["sam_masks"]), torch.from_numpy(d["sampled_pixel"]), torch.from_numpy(d["sampled_mask"])
    ref = R.statement(torch.from_numpy(d["features"]), sam, sp, sm, mode, float(d["positive_th"]), float(d["negative_th"]), use_w)
    assert np.array_equal(ref.C.numpy(), d["C"] != 0)
    assert np.array_equal(ref.W.numpy().astype(np.float32), d["weights"] if use_w else np.ones_like(d["weights"]))
    assert np.array_equal(R.weights_from_a(ref.a).numpy(), d["weights"]), "a does not reproduce the reference's weights"
    np.testing.assert_allclose(ref.C_F.numpy(), d["C_F"], rtol=0, atol=1e-6)
    tag = mode + ("" if use_w else "_noweights")
    assert abs(float(ref.loss_pos) - float(d[f"{tag}_loss_pos"])) < 1e-6 and abs(float(ref.loss_neg) - float(d[f"{tag}_loss_neg"])) < 1e-6
    assert abs(float(ref.pos_similarity) - float(d["pos_similarity"])) < 1e-6
    assert abs(float(ref.neg_similarity) - float(d["neg_similarity"])) < 1e-6
    np.testing.assert_allclose(ref.grad.numpy(), d[f"{tag}_grad"], rtol=1e-5, atol=1e-8)
    assert float(ref.grad.abs().sum()) > 0 and torch.equal(ref.grad[:, ~sp], torch.zeros_like(ref.grad[:, ~sp]))


def _oracle64(scene, mode, pth, nth, use_w):
    f = scene[0].double().clone().requires_grad_(True)
    lp, ln, ps, ns = O.head(f, *scene[1:], mode, pth, nth, use_w, dtype=torch.float64)
    (lp + ln).backward()
    return lp.detach(), ln.detach(), ps, ns, f.grad


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("use_w", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("scene", [("lattice", (65, 14, 7, 65)), ("lattice", (257, 14, 7, 257)), ("lattice", UNCOVERED_ARGS),
                                   ("probe", (33, 33, 33, None)), ("probe", (300, 37, 300, None))], ids=lambda s: f"{s[0]}{s[1][0]}")
def test_statement_matches_oracle_in_float64(scene, mode, use_w):
    """the two were written separately; on the lattice they must agree to the last few float64 bits"""
    sc, ref, _ = R.reference(*scene, mode, 0.75, 0.5, use_w)
    lp, ln, ps, ns, grad = _oracle64(sc, mode, 0.75, 0.5, use_w)
    for name, a, b in (("loss_pos", ref.loss_pos, lp), ("loss_neg", ref.loss_neg, ln), ("pos_similarity", ref.pos_similarity, ps),
                       ("neg_similarity", ref.neg_similarity, ns)):
        assert abs(float(a) - float(b)) <= 1e-14 * max(1.0, abs(float(b))), name
    assert float((ref.grad - grad).abs().max()) <= 1e-13 * max(float(grad.abs().max()), 1e-30)
    C = O.correspondence_matrix(sc[1], sc[2], sc[3])
    assert torch.equal(ref.C, C != 0)
    # the counts are the oracle's npair / selection sizes
    cf = O.feature_matrix(sc[0], sc[2], torch.float64)
    diag = torch.eye(ref.S, dtype=torch.bool)
    for neg, n_ref in ((False, ref.N_pos), (True, ref.N_neg)):
        cv = 0 if neg else 1
        if mode == "hard":
            n = int(torch.triu(((cf > 0.5) if neg else (cf < 0.75)) & (C == cv) & ~diag).sum())
        else:
            cond = (C == cv) if mode == "all" else (((cf > 0.5) if neg else (cf < 0.75)) & (C == cv))
            n = int(torch.triu(cond.any(0)[None, :] & ~diag).sum())
        assert n == n_ref


@pytest.mark.parametrize("pth,nth", [(0.75, 0.0), (0.6875 + 1 / 32, -0.0625), (0.6875 + 1 / 32, 0.5)])
def test_statement_matches_oracle_at_other_thresholds(pth, nth):
    for mode in ("soft", "hard"):
        sc, ref, _ = R.reference("lattice", (65, 14, 7, 65), mode, pth, nth, True)
        lp, ln, _, _, grad = _oracle64(sc, mode, pth, nth, True)
        assert abs(float(ref.loss_pos) - float(lp)) <= 1e-14 and abs(float(ref.loss_neg) - float(ln)) <= 1e-14
        assert float((ref.grad - grad).abs().max()) <= 1e-13 * float(grad.abs().max())


# ---- premises of the GPU scenes -----------------------------------------------------------------------------------------------------
def _on_lattice(scene):
    c32, c64 = O.feature_matrix(scene[0], scene[2], torch.float32), O.feature_matrix(scene[0], scene[2], torch.float64)
    assert torch.equal(c32.double(), c64), "C_F in float32 is not C_F in float64"
    assert bool(((c64 * 16).round() == c64 * 16).all()) and float(c64.abs().max()) == 1.0 and torch.equal(c64.diag(), torch.ones(c64.shape[0], dtype=torch.float64))
    x = scene[0]
    assert bool(((x == 0) | (x.abs() == 1)).all()) and bool(((x != 0).sum(0) == 16).all())
    return c64


@pytest.mark.parametrize("args", LATTICE_ARGS + [UNCOVERED_ARGS], ids=lambda a: f"S{a[0]}" + ("u" if a == UNCOVERED_ARGS else ""))
def test_lattice_scene_premises(args):
    scene = R.lattice_scene(*args)
    feat, sam, sp, sm = scene
    S = args[0]
    assert int(sp.sum()) == S and int(sm.sum()) == 7 and sam.shape == (14, *R.LATTICE_HW)
    cf = _on_lattice(scene)
    ref = R.statement(*scene, "soft", 0.75, 0.5, True)
    cover = sam.sum(0)[sp]
    if args == UNCOVERED_ARGS:
        assert int((cover == 0).sum()) == round(0.25 * S) >= 16, "a quarter of the sampled pixels must be uncovered"
        assert bool((ref.a[cover == 0] == 0).all()) and bool((ref.a[cover != 0] > 0).all())
    if S < 31:                                      # too few entries for ties and plants: these two are there for the dispatch
        assert ref.N_pos > 0 and (S == 2 or ref.N_neg > 0) and bool(ref.grad.isfinite().all()) and ref.a.unique().numel() >= 2
        return
    up = torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1)
    assert int((ref.C & up).sum()) > 0 and int((~ref.C & up).sum()) > 0, "both pair kinds among i < j"
    assert int((cf[up] < 0).sum()) > 0 and int((cf[up] == 0).sum()) > 0, "negative and exactly zero similarities"
    assert ref.a.unique().numel() >= 3
    assert int((cover == 0).sum()) >= 1, "a sampled pixel no mask covers"
    if S >= 65:
        assert int((cf == 0.75).sum()) >= 50 and int((cf == 0.5).sum()) >= 50, "ties at both thresholds"
        for mode in R.MODES:
            r = R.statement(*scene, mode, 0.75, 0.5, False)
            assert r.N_pos > 0 and r.N_neg > 0 and float(r.loss_pos) < 0 < float(r.loss_neg), f"{mode}: a pair kind is empty"
    # the planted pixel: in no sampled mask, and its 'soft' negative flag comes from its own diagonal entry alone
    _, j = R.planted_pixel(*scene)
    assert not bool(ref.member[j].any()) and not bool(ref.C[:, j].any())
    off = torch.arange(S) != j
    assert float(cf[off, j].max()) <= 0.5 and bool(ref.colN[j]) and j > 0
    assert not bool((~ref.C[off, j] & (cf[off, j] > 0.5)).any())
    # ... so a head that skips the diagonal counts j pairs fewer
    assert ref.N_neg - int(torch.arange(S)[ref.colN & (torch.arange(S) != j)].sum()) == j


@pytest.mark.parametrize("case", R.PROBE_CASES, ids=lambda c: f"N{c[0]}s{c[1]}")
def test_probe_scene_premises(case):
    N, ns, first = case
    scene = R.probe_scene(N, ns, N, first)
    feat, sam, sp, sm = scene
    _on_lattice(scene) if N <= 65 else None
    S = int(sp.sum())
    assert S == 2 * min(N, 640) <= 1200 and int(sm.sum()) == ns <= 256
    ref = R.statement(*scene, "hard", 0.75, 0.5, True)
    assert int(ref.C.sum() - ref.C.diag().sum()) == 2 * ns, "the planted-pair count"
    assert ref.member.shape == (S, ns) and bool((ref.member.sum(0) == 2).all()) and int(ref.member.sum(1).max()) == 1
    if N > 1:
        assert ref.a.unique().numel() >= 3
    rank = torch.cumsum(sm.long(), 0) - 1
    where = {int(rank[n]): n for n in range(N) if sm[n]}
    if (N, ns) == (257, 256):
        assert where[255] == 256 and not bool(sm[:256].all())
    if (N, ns) == (600, 255):
        assert where[30] < 256 <= where[31] < where[32] and where[254] >= 512, "ranks 31 and 32 lie behind the first carry"
        assert int(sm[256:512].sum()) > 0 and int(sm[512:].sum()) > 0
    if (N, ns) == (600, 1):
        assert where[0] >= 256


def test_rank_edges_fall_behind_the_first_trip():
    """ranks 0, 31, 32 and 255 each lie on a mask with index >= 256 in at least one probe case"""
    seen = set()
    for N, ns, first in R.PROBE_CASES:
        sm = R.probe_scene(N, ns, N, first)[3]
        rank = torch.cumsum(sm.long(), 0) - 1
        seen |= {int(rank[n]) for n in range(256, N) if sm[n]}
    assert {0, 31, 32, 255} <= seen


def test_one_mask_scene_has_no_defined_weights():
    scene = R.one_mask_scene(65, 7)
    ref = R.statement(*scene, "soft", 0.75, 0.5, True)
    assert ref.a.unique().numel() == 1 and bool(ref.W.isnan().all())
    assert bool(ref.loss_pos.isnan()) and bool(ref.loss_neg.isnan())
    rows = ref.rows.isnan().any(1)
    assert bool((rows == ref.rows.isnan().all(1)).all()) and bool((rows == ref.active).all()) and 0 < int(rows.sum())
    plain = R.statement(*scene, "soft", 0.75, 0.5, False)
    assert bool(plain.grad.isfinite().all()) and plain.N_pos > 0 and plain.N_neg > 0


def test_resize_reproduces_the_lattice():
    """nearest x2 up, ATen bilinear (align_corners=False) down: both taps of an axis lie in one source block, weights 0.5 + 0.5"""
    feat = R.lattice_scene(257, 14, 7, 257)[0]
    up = R.upsampled(feat)
    assert up.shape == (32, 48, 80)
    down = torch.nn.functional.interpolate(up[None], size=R.LATTICE_HW, mode="bilinear", align_corners=False)[0]
    assert torch.equal(down, feat)
    g = torch.arange(32 * 24 * 40, dtype=torch.float32).view(32, 24, 40)
    assert torch.equal(R.spread_x2(g)[:, 1::2, 0::2], g * 0.25)


@pytest.mark.parametrize("S", [65, 257])
def test_threshold_cases_hold_ties_and_silenced_pairs(S):
    """what the threshold cases of the GPU tests rely on: pairs exactly on 0.75, 0.5 and 0 exist among i < j in both kinds; at
    nth = -0.0625 'hard' selects negative pairs with f = 0, which the relu leaves without loss and without gradient; 0.71875
    separates the lattice points 0.6875 and 0.75"""
    sc, ref, _ = R.reference("lattice", R.edge_args(S), "hard", 0.75, -0.0625, False)
    up = torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1)
    cf = ref.C_F
    assert int((up & ref.C & (cf == 0.75)).sum()) > 0 and int((up & ~ref.C & (cf == 0.5)).sum()) > 0
    sel = up & ~ref.C & (cf > -0.0625)
    assert ref.N_neg == int(sel.sum()) and int((sel & (cf == 0)).sum()) > 0 and int((up & ~ref.C & (cf == -0.0625)).sum()) > 0
    assert bool((ref.dCF[sel & (cf <= 0)] == 0).all()) and bool((ref.dCF[sel & (cf > 0)] > 0).all())
    tie = R.statement(*sc, "hard", 0.75, 0.5, False)
    assert tie.N_pos == int((up & ref.C & (cf <= 0.6875)).sum()) and tie.N_neg == int((up & ~ref.C & (cf >= 0.5625)).sum())
    mid = R.statement(*sc, "hard", 0.6875 + 1 / 32, 0.0, False)
    assert mid.N_pos == tie.N_pos and mid.N_neg == int((up & ~ref.C & (cf >= 0.0625)).sum()) > tie.N_neg


# ---- sensitivity: a single wrong pair is visible ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("use_w", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("S", [2, 31, 513])
def test_one_pair_moves_a_row_by_ten_bars(S, mode, use_w):
    """Removing any single active pair from the float64 statement moves the gradient row of one of its two pixels by more than
    10 x that row's bar (4 x the float32 oracle's error on the row + one ulp of the row's largest entry), on the smallest scene,
    on the smallest with ties and plants, and on the largest.  A pair of parallel vectors (similarity +-1) has a zero
    gradient contribution by the normalisation's projection and is seen by the exact loss instead: those are excluded here."""
    sc, ref, err = R.reference("lattice", R.edge_args(S), mode, 0.75, 0.5, use_w)
    bars = R.row_bars(err.rows, ref.rows)
    mi, mj = R.pair_moves(ref)
    act = (ref.dCF != 0) & (ref.C_F.abs() < 1)
    assert int(act.sum()) > (100 if S > 100 else 10 if S > 2 else 0)
    ratio = torch.maximum(mi / bars[:, None], mj / bars[None, :])[act]
    print(f"S {S} {mode} weights {use_w}: {int(act.sum())} active pairs, smallest move / bar = {float(ratio.min()):.1f}")
    assert float(ratio.min()) > 10.0
    # ... and by more than 10 x the rows' forward error bound, which judges the families whose rows cancel too far for the first bar
    fwd = R.row_forward_bounds(ref)
    ratio = torch.maximum(mi / fwd[:, None], mj / fwd[None, :])[act]
    print(f"    smallest move / forward bound = {float(ratio.min()):.1f}")
    assert float(ratio.min()) > 10.0
    # the closed form is what dropping the pair does
    pairs = torch.nonzero(act)
    for k in (0, pairs.shape[0] // 2, pairs.shape[0] - 1):
        i, j = int(pairs[k, 0]), int(pairs[k, 1])
        moved = (R.statement(*sc, mode, 0.75, 0.5, use_w, drop=(i, j)).rows - ref.rows).abs().amax(1)
        assert abs(float(moved[i]) - float(mi[i, j])) <= 1e-12 * float(mi[i, j]) + 1e-18
        assert abs(float(moved[j]) - float(mj[i, j])) <= 1e-12 * float(mj[i, j]) + 1e-18
        assert int((moved != 0).sum()) <= 2
