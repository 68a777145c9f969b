"""tests/nnfm_reference.py without a GPU: the float64 statement against the committed fixture and autograd, the short-list
emulation against the float64 argmax, and the premises of every input of tests/test_gpu_nnfm_forms.py -- the share of rows below
the fp32 margin, the rows whose outcome the emulation decides, and how many of those leave the float64 argmax."""
import os

import numpy as np
import pytest
import torch

from tests import nnfm_reference as R

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "nnfm.npz"))


# ---- the float64 statement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "vgg"])
def test_reference_reproduces_the_fixture(name):
    """The fixture is the reference implementation's fp32 evaluation: a few fp32 ulps of O(1) cosines (loss, margins) and of the
    gradient's scale."""
    ref = R.reference(G[f"{name}_f1"], G[f"{name}_f2"])
    assert abs(ref["loss"] - float(G[f"{name}_loss"])) < 1e-6
    assert np.array_equal(ref["argmax"], G[f"{name}_argmin"])
    assert np.abs(ref["margin2"] - G[f"{name}_margin"]).max() < 1e-6
    assert np.abs(ref["grad"] - G[f"{name}_grad"]).max() < 2e-6 * np.abs(ref["grad"]).max()
    assert (ref["margin3"] >= ref["margin2"]).all()


@pytest.mark.parametrize("c,n1,n2,relu", [(64, 33, 17, False), (192, 20, 1, True), (128, 7, 2, False)])
def test_analytic_gradient_equals_autograd(c, n1, n2, relu):
    f1, f2 = R.features(c, n1, 1, relu), R.features(c, n2, 2, relu)
    ref = R.reference(f1, f2)
    x = torch.tensor(f1, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(f2, dtype=torch.float64)
    cos = (x / x.norm(dim=0)).T @ (b / b.norm(dim=0))
    loss = (1.0 - cos.max(dim=1).values).mean()
    loss.backward()
    assert abs(float(loss.detach()) - ref["loss"]) < 1e-14
    assert np.abs(x.grad.numpy() - ref["grad"]).max() < 1e-13 * np.abs(ref["grad"]).max()
    assert np.array_equal(cos.argmax(dim=1).numpy(), ref["argmax"])
    # grad_toward another column is the gradient of that column's cosine
    cols = (ref["argmax"] + 1) % n2
    x.grad = None
    (1.0 - ((x / x.norm(dim=0)).T @ (b / b.norm(dim=0)))[torch.arange(n1), torch.tensor(cols)]).mean().backward()
    assert np.abs(x.grad.numpy() - R.grad_toward(f1, f2, cols)).max() < 1e-13 * np.abs(ref["grad"]).max()


def test_margins_and_ties_on_a_hand_written_case():
    f1 = np.array([[1.0, 0.0], [0.0, 2.0]], np.float32)                       # rows e0 and e1 (columns of f1)
    f2 = np.array([[1.0, 3.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]], np.float32)   # e0, 3 e0, e1, (e0 + e1)
    ref = R.reference(f1, f2)
    assert ref["argmax"].tolist() == [0, 2]                                   # row 0 ties columns 0 and 1: the lowest wins
    np.testing.assert_allclose(ref["margin2"], [0.0, 1 - 2 ** -0.5], atol=1e-15)
    np.testing.assert_allclose(ref["margin3"], [1 - 2 ** -0.5, 1.0], atol=1e-15)
    em = R.emulate(f1, f2)
    assert em["pred"].tolist() == [0, 2] and em["decided"].tolist() == [False, True]
    assert R.reference(f1, f2[:, :1])["margin2"].tolist() == [np.inf, np.inf]
    one = R.emulate(f1, f2[:, 3:])
    assert one["pred"].tolist() == [0, 0] and one["decided"].all()


# ---- the emulation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.NEAR_DUP)
def test_a_short_list_of_everything_is_the_float64_argmax(c):
    f1, f2, ref, em = R.near_duplicate_case(c)
    full = R.emulate(f1, f2, keep=None)
    assert np.array_equal(full["pred"], ref["argmax"]) and (full["deficit"] == 0).all()
    assert (em["pred"] != ref["argmax"]).any()                       # which two candidates do not give on this input


def test_nudged_inputs_round_the_same_under_any_fp32_norm():
    """No element of a nudged input normalises to within 4 fp32 ulps of a bf16 tie, the nudge moved the elements it touched by
    2^-12 of themselves, and a norm that is one fp32 ulp larger or smaller rounds every element to the same bf16."""
    for c in (64, 512):
        raw = R.features(c, 257, 5, True)
        x = R.nudge(raw)
        v = R.normalise_fp32(x)
        assert not bool(R.near_bf16_tie(v).any())
        moved = x != raw
        assert 0 < moved.mean() < 1e-3 and np.abs(x[moved] / raw[moved] - 1).max() < 2.0 ** -11
        t = torch.as_tensor(x)
        inv = 1.0 / torch.sqrt((t * t).sum(dim=0))
        for other in (torch.nextafter(inv, torch.zeros(())), torch.nextafter(inv, torch.full((), np.inf))):
            assert torch.equal((t * other).bfloat16(), v.bfloat16())


@pytest.mark.parametrize("c", R.NEAR_DUP)
def test_near_duplicate_inputs_decide_enough_rows(c):
    """The premises of the short-list test: at least a quarter of the rows decided, at least 20 decided rows predicted to leave
    the float64 argmax, and no decided row's predicted cosine more than 2 e below the best."""
    f1, f2, ref, em = R.near_duplicate_case(c)
    n1, n2 = R.NEAR_DUP[c][:2]
    assert f1.shape == (c, n1) and f2.shape == (c, n2) and max(n1, n2) <= 257
    dec = em["decided"]
    leaves = dec & (em["pred"] != ref["argmax"])
    print(f"C = {c}: decided {dec.mean():.3f}, decided rows leaving the argmax {int(leaves.sum())}, all rows leaving "
          f"{(em['pred'] != ref['argmax']).mean():.3f}, largest deficit {em['deficit'].max():.3e}, e {em['e']:.3e}, rows with a "
          f"float64 margin above 1e-6 among those leaving {(ref['margin2'][leaves] > R.FP32_MARGIN).mean():.3f}")
    assert dec.mean() >= 0.25
    assert int(leaves.sum()) >= 20
    assert em["deficit"][dec].max() <= 2 * em["e"]
    assert (em["deficit"] >= 0).all()
    # the old contract ("follows the float64 neighbour above a 1e-6 margin") is false here
    assert (ref["margin2"][leaves] > R.FP32_MARGIN).sum() >= 20


# ---- the inputs that must follow the float64 neighbour ------------------------------------------------------------------------
def _plain_cases():
    cases = [(c, 129, 97, relu) for c in R.FORMS for relu in (False, True)]
    cases += [(c, n1, 97, True) for c in (64, 512) for n1 in R.ROW_EDGES]
    cases += [(c, 129, n2, True) for c in (64, 512) for n2 in R.COL_EDGES]
    return sorted(set(cases))


@pytest.mark.parametrize("c,n1,n2,relu", _plain_cases())
def test_plain_inputs_follow_the_float64_neighbour_by_the_emulation(c, n1, n2, relu):
    f1, f2, ref = R.plain_case(c, n1, n2, relu)
    assert f1.shape == (c, n1) and f2.shape == (c, n2)
    clear = ref["margin2"] > R.FP32_MARGIN
    assert (~clear).mean() <= R.MAX_EXCLUDED
    assert (R.follows_float64(f1, f2) | ~clear).all()
    em = R.emulate(f1, f2)
    assert np.array_equal(em["pred"][clear], ref["argmax"][clear])
    if relu:
        assert (f1 >= 0).all() and (f1 == 0).mean() > 0.2            # post-ReLU: exact zeros


@pytest.mark.parametrize("runner", ["lane", "merge"])
def test_planted_inputs(runner):
    f1, f2, j, r, ref = R.planted_case(runner=runner)
    n2 = f2.shape[1]
    assert np.array_equal(np.sort(j), np.arange(n2))                 # every column, so every lane, tile and the ragged tile
    order = np.argsort(-ref["cos"], axis=1)
    assert np.array_equal(order[:, 0], j) and np.array_equal(order[:, 1], r)
    step = 32 if runner == "lane" else 1
    assert (np.abs(r - j) == step).all() and (r > j).sum() >= 30 and (r < j).sum() >= 30
    # gaps above 2 e keep the order of the float64 cosines in the bf16 products: the match leads by tens of e, the runner-up
    # is ahead of the rest by at least 4 e, so the device's short-list is (j, r)
    em = R.emulate(f1, f2)
    print(runner, ref["margin2"].min(), (ref["margin3"] - ref["margin2"]).min(), em["e"])
    assert ref["margin2"].min() > 20 * em["e"] and (ref["margin3"] - ref["margin2"]).min() > 4 * em["e"]
    assert np.array_equal(em["top"][:, :2], np.stack([j, r], axis=1))
    assert np.array_equal(em["pred"], j) and em["decided"].all() and R.follows_float64(f1, f2).all()


def test_duplicate_input():
    f1, f2, unique, copy_of, ref = R.duplicate_case()
    assert f2.shape[1] == 2 * unique.shape[1]
    assert np.array_equal(f2, unique[:, copy_of]) and np.array_equal(np.bincount(copy_of), np.full(unique.shape[1], 2))
    em = R.emulate(f1, f2)
    assert ref["margin2"].min() > 20 * em["e"]                       # the next DISTINCT column is far behind
    assert np.array_equal(copy_of[em["pred"]], ref["argmax"])
    # the short-list is the two copies; the lower column wins the tie
    first = np.array([np.flatnonzero(copy_of == u).min() for u in ref["argmax"]])
    assert np.array_equal(em["pred"], first) and np.array_equal(np.sort(copy_of[em["top"][:, :2]], axis=1)[:, 0], ref["argmax"])


@pytest.mark.parametrize("c", R.NEAR_DUP)
def test_matched_columns_reads_the_column_off_a_gradient(c):
    f1, f2, ref, em = R.near_duplicate_case(c)
    want = R.grad_toward(f1, f2, em["pred"])
    cols, res = R.matched_columns(want.astype(np.float32), f1, f2)
    assert np.array_equal(cols, em["pred"]) and res.max() < 1e-6
    # the gradient rows of the other columns among a row's three largest products lie more than two row bars from the predicted
    # column's: a device row within one bar of a column is further than a bar from its copies, so the reading is unambiguous
    scale = np.abs(ref["grad"]).max()
    for k in range(3):
        col = em["top"][:, k]
        gap = np.abs(R.grad_toward(f1, f2, col) - want).max(axis=0) / scale
        assert gap[col != em["pred"]].min() > 2 * R.ROW_BAR
