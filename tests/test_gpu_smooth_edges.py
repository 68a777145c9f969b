"""The KNN feature smoothing (trase_amd/smooth.py, csrc/smooth.hip) on hand-built graphs against tests/smooth_reference.py:
every P around the eight-lane groups and the 32-Gaussian block, K and S up to 32 with slot 31 (the top bit of the selection
mask), in-degrees 0 ... 9 (every remainder of the backward's four-edge loop), a hub of in-degree 2056, a repeated target, a
self-loop, and both halves of the ``||x|| < eps`` branch.

Bars: the device may differ from float64 by 4 times the error of the fp32 evaluation of tests/smooth_reference.py on the same
input plus one fp32 ulp of the result's scale (over the tensor; row by row where the rows' magnitudes span 1e12).
Largest shares of the bar (device error / bar) measured on an MI355X: forward 0.22, backward 0.24 (K 32 S 32 forward, hub
backward; hub forward 0.20; norm branches, row by row: forward 0.19, backward 0.20)."""
import numpy as np
import pytest
import torch

from tests import smooth_reference as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _run(x, w, idx, sel, sel_on_gpu=False, transposed=False):
    """-> (out (P, 32), gradient (P, 32), gradient of a second backward), float64 numpy"""
    from trase_amd.smooth import smooth_features
    P = len(x)
    it = torch.as_tensor(idx, dtype=torch.int64).to(DEV)
    st = torch.as_tensor(sel, dtype=torch.int64)
    st = st.to(DEV) if sel_on_gpu else st
    wt = torch.as_tensor(w).to(DEV)
    outs, grads = [], []
    for _ in range(2):
        f = torch.as_tensor(x).to(DEV).requires_grad_(True)
        out = smooth_features(f, it, st)
        assert out.shape == (P, 1, R.F) and out.dtype == torch.float32
        if transposed:
            (out.transpose(0, 2) * wt.transpose(0, 2).contiguous()).sum().backward()    # the upstream gradient is a view
        else:
            (out * wt).sum().backward()
        assert f.grad.shape == (P, 1, R.F)
        outs.append(out.detach().reshape(P, R.F))
        grads.append(f.grad.reshape(P, R.F))
    assert torch.equal(outs[0], outs[1])
    return outs[0].double().cpu().numpy(), grads[0].double().cpu().numpy(), grads[1].double().cpu().numpy()


def _check(name, x, w, idx, sel, per_row=False, grad_rows=None, **kw):
    out, grad, again = _run(x, w, idx, sel, **kw)
    assert np.array_equal(grad, again)                   # the backward is bit-reproducible
    o64, g64 = R.forward64(x, idx, sel), R.backward64(x, idx, sel, w)
    o32, g32 = R.forward32(x, idx, sel), R.backward32(x, idx, sel, w)
    fs = R.share(out, o32, o64, per_row)
    gs = R.share(grad, g32, g64, per_row, grad_rows)
    print(f"{name}: share of the bar, forward {fs:.3f}, backward {gs:.3f}")
    assert np.isfinite(out).all() and np.isfinite(grad).all()
    assert fs <= 1.0
    assert gs <= 1.0
    nobody = np.bincount(np.asarray(idx)[:, sel].reshape(-1), minlength=len(x)) == 0
    assert (grad[nobody] == 0).all()                     # a node no selected slot names gets exactly zero
    return out, grad


@pytest.mark.parametrize("P", R.RING_P)
def test_ring_at_the_grouping_boundaries(P):
    _check(f"ring {P}", *R.data(P, P), *R.ring(P))


@pytest.mark.parametrize("sel_on_gpu", [False, True], ids=["sel_cpu", "sel_cuda"])
@pytest.mark.parametrize("K,S", R.KS_CASES)
def test_k_and_s(K, S, sel_on_gpu):
    idx, sel = R.ks_graph(K, S)
    _check(f"K {K} S {S}", *R.data(67, 10 * K + S), idx, sel, sel_on_gpu=sel_on_gpu)


def test_in_degree_ladder():
    idx, sel = R.ladder()
    assert np.bincount(idx.reshape(-1), minlength=24)[:10].tolist() == list(range(10))
    _check("ladder", *R.data(24, 2), idx, sel)


def test_hub():
    idx, sel = R.hub()
    out, grad = _check("hub", *R.data(257, 3), idx, sel)
    assert (grad[1:] == 0).all() and np.abs(grad[0]).max() > 0
    assert (out == out[0]).all()                         # every row is the normalised node 0


def test_repeated_target_and_self_loop():
    x, w = R.data(9, 4)
    idx, sel = R.repeats()
    out, _ = _check("repeats", x, w, idx, sel)
    # the repeated node counts twice
    n = x.reshape(9, 32).astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs(out - (n + 2 * n[(np.arange(9) + 2) % 9]) / 3).max() < 1e-6


def test_norm_branches_row_by_row():
    """Norms 0, 1e-20, 5e-13 (below eps: x / eps, Jacobian I / eps), 2e-12 and 1e-3 (above): the forward on every row, the
    gradient on every row but the exact zero (d normalize at 0 is a convention), each against its own magnitude."""
    x, w, idx, sel = R.norm_branches()
    rows = np.arange(12) != 0
    out, grad = _check("norm branches", x, w, idx, sel, per_row=True, grad_rows=rows)
    g64 = R.backward64(x, idx, sel, w)
    mag = np.abs(g64).max(axis=1)
    assert mag[1] > 1e10 and mag[2] > 1e10 and mag[3] > 1e9 and mag[5:].max() < 1e3      # the magnitudes do span 1e12
    assert np.abs(out[0]).max() == 0 and 1e-9 < np.abs(out[1]).max() < 1e-7 and 0.05 < np.abs(out[2]).max() < 0.5


@pytest.mark.parametrize("graph", ["ladder", "hub"])
def test_reverse_adjacency_is_the_stable_sort(graph):
    from trase_amd.smooth import reverse_adjacency
    idx = getattr(R, graph)()[0]
    ptr, src = reverse_adjacency(torch.as_tensor(idx, dtype=torch.int64).to(DEV))
    want_ptr, want_src = R.reverse_adjacency_np(idx)
    assert ptr.dtype == torch.int32 and src.dtype == torch.int32
    assert torch.equal(ptr.cpu(), torch.as_tensor(want_ptr)) and torch.equal(src.cpu(), torch.as_tensor(want_src))


def test_non_contiguous_upstream_gradient():
    idx, sel = R.ks_graph(16, 16)
    _check("transposed upstream", *R.data(67, 9), idx, sel, transposed=True)


def test_empty_input():
    from trase_amd.smooth import smooth_features
    f = torch.zeros(0, 1, 32, device=DEV, requires_grad=True)
    out = smooth_features(f, torch.zeros(0, 4, dtype=torch.int64, device=DEV), torch.tensor([1, 0]))
    assert out.shape == (0, 1, 32) and out.dtype == torch.float32
    out.sum().backward()
    assert f.grad.shape == (0, 1, 32)
