"""Every form of the NNFM style loss (trase_amd/csrc/nnfm.hip) against tests/nnfm_reference.py.

* the eight nnfm_match_kernel instantiations (C = 64 ... 512), the row edges of a wave (32), a workgroup (128) and an
  nnfm_finish block (256), the column edges of a B tile (32) and of nnfm_prep (64), on inputs whose premises
  tests/test_nnfm_reference.py asserts without a GPU: every row with a float64 margin above 1e-6 follows the float64 neighbour;
  bars as tests/test_gpu_nnfm.py (loss 2e-7 max(1, |ref|) + 1e-7, gradient rows 1e-4 of the gradient's scale);
* planted matches in every column with a planted runner-up in the same lane or in a neighbouring one; exact duplicates;
* near-duplicate style columns, where the kernel's real contract shows: the match is the float64-better of the two columns
  with the largest bf16 products.  Every row the emulation decides carries the predicted column's gradient -- also where that
  is not the float64 argmax -- and every row's cosine is within 2 e of its best, e the largest bf16 product error of the input.
  Measured on an MI355X (C: rows off the float64 argmax, largest deficit, e):
      64: 47.1 %, 2.5e-4, 2.4e-3    192: 43.2 %, 1.4e-4, 1.2e-3    320: 40.9 %, 1.3e-4, 8.8e-4    512: 37.7 %, 1.1e-4, 7.9e-4
  (almost all of them with a float64 margin above 1e-6; the loss lies 1.4e-5 ... 2.5e-5 above the float64 loss)
* the interface: upstream gradients other than 1, two forwards alive before one backward, transposed views, refusals."""
import numpy as np
import pytest
import torch

from tests import nnfm_reference as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _run(f1, f2, upstream=None):
    """-> (loss as float, gradient (C, N1) float64 numpy)"""
    from trase_amd.losses import loss_nnfm_style
    x = torch.as_tensor(f1).to(DEV).requires_grad_(True)
    loss = loss_nnfm_style(x, torch.as_tensor(f2).to(DEV))
    (loss if upstream is None else upstream * loss).backward()
    return float(loss.detach()), x.grad.double().cpu().numpy()


def _row_err(got, want, scale=None):
    scale = np.abs(want).max() if scale is None else scale
    return np.abs(got - want).max(axis=0) / scale


def _check_follows(f1, f2, ref, upstream=None):
    """loss and every row with a float64 margin above 1e-6 against float64"""
    loss, grad = _run(f1, f2, upstream)
    k = 1.0 if upstream is None else upstream
    clear = ref["margin2"] > R.FP32_MARGIN
    assert (~clear).mean() <= R.MAX_EXCLUDED
    err = _row_err(grad, k * ref["grad"])
    print(f"loss error {abs(loss - ref['loss']):.2e} (bar {R.loss_tol(ref['loss']):.2e}), largest row error {err[clear].max():.2e}")
    assert abs(loss - ref["loss"]) <= R.loss_tol(ref["loss"])
    assert np.isfinite(grad).all()
    assert err[clear].max() < R.ROW_BAR, (int((err > R.ROW_BAR).sum()), np.flatnonzero(err > R.ROW_BAR)[:8])
    return loss, grad


# ---- forms and shape edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["randn", "relu"])
@pytest.mark.parametrize("c", R.FORMS)
def test_every_channel_form(c, relu):
    """N1 = 129: a ragged last wave and workgroup; N2 = 97: four B tiles, the last with one live column."""
    _check_follows(*R.plain_case(c, 129, 97, relu))


@pytest.mark.parametrize("n1", R.ROW_EDGES)
@pytest.mark.parametrize("c", [64, 512])
def test_row_edges(c, n1):
    _check_follows(*R.plain_case(c, n1, 97, True))


@pytest.mark.parametrize("n2", R.COL_EDGES)
@pytest.mark.parametrize("c", [64, 512])
def test_column_edges(c, n2):
    """2 <= N2 <= 33: lanes that never update, the min(c, N2 - 1) clamp and the `no second candidate` rule together."""
    f1, f2, ref = R.plain_case(c, 129, n2, True)
    _, grad = _check_follows(f1, f2, ref)
    cols, res = R.matched_columns(grad, f1, f2)
    assert (cols < n2).all() and res.max() < R.ROW_BAR


# ---- planted matches, duplicates -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("runner", ["lane", "merge"])
def test_planted_matches_in_every_column(runner):
    f1, f2, j, r, ref = R.planted_case(runner=runner)
    _, grad = _check_follows(f1, f2, ref)
    cols, res = R.matched_columns(grad, f1, f2)
    assert res.max() < R.ROW_BAR
    assert np.array_equal(cols, j), np.flatnonzero(cols != j)


def test_exact_duplicates():
    """Either copy has the same gradient: the reference is taken on the distinct columns."""
    from trase_amd.losses import loss_nnfm_style
    f1, f2, unique, copy_of, ref = R.duplicate_case()
    loss, grad = _check_follows(f1, f2, ref)
    cols, res = R.matched_columns(grad, f1, unique)
    assert np.array_equal(cols, ref["argmax"]) and res.max() < R.ROW_BAR
    x = torch.as_tensor(f1).to(DEV).requires_grad_(True)
    again = loss_nnfm_style(x, torch.as_tensor(f2).to(DEV))
    again.backward()
    assert float(again.detach()) == loss and np.array_equal(x.grad.double().cpu().numpy(), grad)


# ---- the short-list contract ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.NEAR_DUP)
def test_near_duplicate_columns_follow_the_short_list(c):
    f1, f2, ref, em = R.near_duplicate_case(c)
    loss, grad = _run(f1, f2)
    assert np.isfinite(grad).all()
    cols, res = R.matched_columns(grad, f1, f2)
    dec, rows = em["decided"], np.arange(f1.shape[1])
    deficit = ref["best"] - ref["cos"][rows, cols]
    off = cols != ref["argmax"]
    print(f"C = {c}: {off.mean():.3f} of the rows off the float64 argmax ({(off & (ref['margin2'] > R.FP32_MARGIN)).mean():.3f} with "
          f"a float64 margin above 1e-6), largest deficit {deficit.max():.3e}, e {em['e']:.3e}; decided {dec.mean():.3f}, "
          f"{int((cols != em['pred']).sum())} rows differ from the emulation, {int((dec & (cols != em['pred'])).sum())} decided; "
          f"loss - L64 = {loss - ref['loss']:.3e}")
    # every row carries the gradient of ONE column ...
    assert res.max() < R.ROW_BAR
    # ... a decided row that of the predicted column, also where it is not the float64 argmax
    assert np.array_equal(cols[dec], em["pred"][dec]), np.flatnonzero(dec & (cols != em["pred"]))
    err = _row_err(grad, R.grad_toward(f1, f2, em["pred"]), np.abs(ref["grad"]).max())
    assert err[dec].max() < R.ROW_BAR
    assert int((dec & off).sum()) >= 20
    # ... and no row one whose cosine is more than 2 e below its best
    assert deficit.max() <= 2 * em["e"]
    d = np.where(dec, em["deficit"], 2 * em["e"])
    tol = R.loss_tol(ref["loss"])
    assert ref["loss"] - tol <= loss <= ref["loss"] + d.mean() + tol
    # the loss is the mean over the matched columns
    assert abs(loss - float((1.0 - ref["cos"][rows, cols]).mean())) <= tol


# ---- interface -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,c", [(2.5, 128), (-0.125, 256)])
def test_upstream_gradient_scales_the_rows(k, c):
    _check_follows(*R.plain_case(c, 129, 97, True), upstream=k)


def test_two_forwards_alive_before_one_backward():
    from trase_amd.losses import loss_nnfm_style
    a1, a2, ra = R.plain_case(448, 129, 97, True)
    b1, b2, rb = R.plain_case(64, 257, 97, True)
    xa, xb = torch.as_tensor(a1).to(DEV).requires_grad_(True), torch.as_tensor(b1).to(DEV).requires_grad_(True)
    la = loss_nnfm_style(xa, torch.as_tensor(a2).to(DEV))
    lb = loss_nnfm_style(xb, torch.as_tensor(b2).to(DEV))
    (la + 3.0 * lb).backward()
    for x, ref, k, l in ((xa, ra, 1.0, la), (xb, rb, 3.0, lb)):
        assert abs(float(l.detach()) - ref["loss"]) <= R.loss_tol(ref["loss"])
        clear = ref["margin2"] > R.FP32_MARGIN
        assert _row_err(x.grad.double().cpu().numpy(), k * ref["grad"])[clear].max() < R.ROW_BAR


@pytest.mark.parametrize("which", ["feat1", "feats2", "both"])
def test_transposed_views(which):
    from trase_amd.losses import loss_nnfm_style
    f1, f2, ref = R.plain_case(384, 129, 97, True)
    t1 = torch.as_tensor(np.ascontiguousarray(f1.T)).to(DEV).requires_grad_(True)      # (N1, C) leaf
    t2 = torch.as_tensor(np.ascontiguousarray(f2.T)).to(DEV)
    x1 = t1.T if which in ("feat1", "both") else t1.T.contiguous()
    x2 = t2.T if which in ("feats2", "both") else t2.T.contiguous()
    assert x1.is_contiguous() == (which == "feats2") and x2.is_contiguous() == (which == "feat1")
    loss = loss_nnfm_style(x1, x2)
    loss.backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= R.loss_tol(ref["loss"])
    clear = ref["margin2"] > R.FP32_MARGIN
    assert t1.grad.shape == (129, 384)
    assert _row_err(t1.grad.T.double().cpu().numpy(), ref["grad"])[clear].max() < R.ROW_BAR


@pytest.mark.parametrize("c,n1,n2,exc,wording", [
    (32, 10, 10, RuntimeError, "nnfm: C = 32 channels (supported: multiples of 64 up to 512)"),
    (96, 10, 10, RuntimeError, "nnfm: C = 96 channels (supported: multiples of 64 up to 512)"),
    (576, 10, 10, RuntimeError, "nnfm: C = 576 channels (supported: multiples of 64 up to 512)"),
    (64, 0, 10, ValueError, "nnfm: empty feature maps"),
    (64, 10, 0, ValueError, "nnfm: empty feature maps")])
def test_refusals(c, n1, n2, exc, wording):
    """nn_check answers before any launch or allocation of a workspace."""
    from trase_amd.losses import loss_nnfm_style
    x = torch.ones(c, n1, device=DEV, requires_grad=True)
    with pytest.raises(exc) as info:
        loss_nnfm_style(x, torch.ones(c, n2, device=DEV))
    assert wording in str(info.value)
    assert x.grad is None
