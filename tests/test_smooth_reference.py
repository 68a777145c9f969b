"""tests/smooth_reference.py without a GPU: the float64 forward and transpose against float64 autograd of the reference's
composition, the reverse adjacency on a hand-written graph and against ``trase_amd.smooth.reverse_adjacency`` on CPU tensors,
the fp32 evaluation against float64, and the premises of the graphs of tests/test_gpu_smooth_edges.py."""
import numpy as np
import pytest
import torch

from tests import smooth_reference as R


def _autograd(x, idx, sel, w):
    """normalize -> index -> mean (scene/gaussian_model.py:95-101) in float64"""
    xt = torch.tensor(np.asarray(x, np.float64).reshape(-1, 1, R.F), requires_grad=True)
    normed = torch.nn.functional.normalize(xt, dim=-1, p=2)
    out = normed[torch.as_tensor(idx)[:, torch.as_tensor(sel)], 0, :].mean(dim=1)
    (out * torch.tensor(np.asarray(w, np.float64).reshape(-1, R.F))).sum().backward()
    return out.detach().numpy(), xt.grad.numpy().reshape(-1, R.F)


def _cases():
    yield ("ring 33",) + R.data(33, 1) + R.ring(33)
    yield ("ladder",) + R.data(24, 2) + R.ladder()
    yield ("hub",) + R.data(257, 3) + R.hub()
    yield ("repeats",) + R.data(9, 4) + R.repeats()
    yield ("K 32 S 16",) + R.data(67, 5) + R.ks_graph(32, 16)
    yield ("norms",) + R.norm_branches()


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_reference_equals_float64_autograd(case):
    name, x, w, idx, sel = case
    out, grad = _autograd(x, idx, sel, w)
    assert np.abs(R.forward64(x, idx, sel) - out).max() <= 1e-15 * max(1.0, np.abs(out).max())
    mine = R.backward64(x, idx, sel, w)
    norm = np.linalg.norm(np.asarray(x, np.float64).reshape(-1, R.F), axis=1)
    rows = norm >= R.EPS                                 # above eps; below it the reference states the documented I / eps
    assert rows.sum() >= len(norm) - 3
    scale = np.abs(grad[rows]).max(axis=1) + 1e-300
    assert (np.abs(mine - grad)[rows].max(axis=1) <= 1e-12 * scale + 1e-15 * np.abs(grad[rows]).max()).all()
    below = (norm < R.EPS) & (norm > 0)
    if below.any():                                      # clamp_min passes no gradient to the norm: autograd agrees with I / eps
        assert np.abs(mine - grad)[below].max() <= 1e-12 * np.abs(grad[below]).max()


def test_reverse_adjacency_on_a_hand_written_graph():
    idx = np.array([[1, 2], [0, 2], [2, 2], [0, 1], [2, 0]])
    ptr, src = R.reverse_adjacency_np(idx)
    assert ptr.tolist() == [0, 3, 5, 10, 10, 10]
    assert src.tolist() == [2, 6, 9, 0, 7, 1, 3, 4, 5, 8]
    assert ptr.dtype == np.int32 and src.dtype == np.int32


@pytest.mark.parametrize("graph", [R.ladder, R.hub, R.repeats, lambda: R.ring(1), lambda: R.ks_graph(32, 32)])
def test_library_reverse_adjacency_on_cpu_tensors(graph):
    from trase_amd.smooth import reverse_adjacency
    idx = graph()[0]
    ptr, src = reverse_adjacency(torch.as_tensor(idx, dtype=torch.int64))
    want_ptr, want_src = R.reverse_adjacency_np(idx)
    assert ptr.dtype == torch.int32 and src.dtype == torch.int32
    assert torch.equal(ptr, torch.as_tensor(want_ptr)) and torch.equal(src, torch.as_tensor(want_src))


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_fp32_evaluation_is_close_to_float64(case):
    """The bars are multiples of this evaluation's error: it must be an fp32 error, not zero and not a different formula."""
    name, x, w, idx, sel = case
    out, grad = R.forward64(x, idx, sel), R.backward64(x, idx, sel, w)
    o32, g32 = R.forward32(x, idx, sel), R.backward32(x, idx, sel, w)
    assert o32.dtype == np.float32 and g32.dtype == np.float32
    n_in = np.bincount(np.asarray(idx)[:, sel].reshape(-1)).max()
    assert 0 < np.abs(o32 - out).max() <= (len(sel) + 8) * 2.0 ** -24 * max(np.abs(out).max(), 1e-30)
    row = np.abs(g32 - grad).max(axis=1)
    live = np.abs(grad).max(axis=1) > 0
    # a row is (G - n (n . G)) / max(||x||, eps): n_in additions into G, 32 into the dot product, the norm and a few products,
    # each 2^-24 of the sum of the absolute terms over the norm
    norm = np.maximum(np.linalg.norm(np.asarray(x, np.float64).reshape(-1, R.F), axis=1), R.EPS)
    g_abs = R.gathered64(idx, sel, np.abs(w)).max(axis=1)
    assert (row <= (n_in + 80) * 2.0 ** -24 * g_abs / norm).all()
    assert row.max() > 0
    assert (g32[~live] == 0).all()


def test_graph_premises():
    for P in R.RING_P:
        idx, sel = R.ring(P)
        assert idx.shape == (P, 4) and idx.min() >= 0 and idx.max() < P
    seen31 = 0
    for K, S in R.KS_CASES:
        idx, sel = R.ks_graph(K, S)
        assert idx.shape == (67, K) and len(sel) == S and len(set(sel.tolist())) == S and sel.min() >= 0 and sel.max() < K
        assert S == 1 or not (np.diff(sel) > 0).all(), (K, S, sel)                # unsorted
        if K == 32:
            assert 31 in sel
            seen31 += 1
    assert seen31 == 3 and R.ks_graph(32, 1)[1].tolist() == [31]
    idx, sel = R.ladder()
    deg = np.bincount(idx.reshape(-1), minlength=24)
    assert deg[:10].tolist() == list(range(10)) and deg.sum() == 96
    on = np.isin(np.arange(4), sel)
    mixed = 0
    for t in range(2, 10):
        slots = np.nonzero(idx == t)[1]
        mixed += bool(on[slots].any() and not on[slots].all())
    assert mixed >= 6                                    # selected and unselected slots among the incoming edges
    idx, sel = R.hub()
    assert np.bincount(idx.reshape(-1), minlength=257).tolist() == [2056] + [0] * 256
    idx, sel = R.repeats()
    assert (idx[:, 0] == np.arange(9)).all() and (idx[:, 1] == idx[:, 3]).all() and {0, 1, 3} == set(sel.tolist())
    x, w, idx, sel = R.norm_branches()
    norm = np.linalg.norm(x.astype(np.float64).reshape(12, 32), axis=1)
    np.testing.assert_allclose(norm[1:5], R.NORMS[1:], rtol=1e-6)
    assert norm[0] == 0 and (norm[5:] > 1).all()
    assert float(np.float32(x[1].max()) ** 2) < 2.0 ** -126          # the squares of the 1e-20 row are below the normal range
    picked = idx[:, sel]
    assert (picked[:5] == np.arange(5)[:, None]).all()
    for t in range(5):
        assert (picked[5:] == t).any()
