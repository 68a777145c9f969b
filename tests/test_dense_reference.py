"""tests/dense_reference.py against the fixture of the imported reference (tests/golden/dense_losses.npz), the key order on
hand-made ties and NaNs, every refusal of the dense entry points before a device is touched, the exact case plan of
tests/test_gpu_dense.py against the classes it has to meet, and the near-tie counts of the random scenes.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import dense_reference as dr

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "dense_losses.npz"))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_restatement_reproduces_the_fixture(fx):
    r = dr.feature3d(fx["f3d_feats"], fx["f3d_near_idx"], fx["f3d_far_idx"])
    assert rel(r["loss"], fx["f3d_loss_f64"]) <= 1e-12 and rel(r["grad"], fx["f3d_grad_f64"]) <= 1e-12
    ref = dr.topk_f64(fx["f3d_xyz"], fx["f3d_xyz"], 16, 4)
    assert np.array_equal(ref["near_idx"], fx["f3d_near_idx"]) and np.array_equal(ref["far_idx"], fx["f3d_far_idx"])
    assert np.array_equal(fx["f3d_near_idx"][:, 0], np.arange(300))          # the row itself is the nearest
    r = dr.cls3d(fx["cls_predictions"], fx["cls_sample"], fx["cls_idx"])
    assert rel(r["loss"], fx["cls_loss_f64"]) <= 1e-12 and rel(r["grad"], fx["cls_grad_f64"]) <= 1e-12
    torch.manual_seed(5)
    assert np.array_equal(torch.randperm(500)[:100].numpy(), fx["cls_sample"])
    assert np.array_equal(fx["cls_idx"][:, 0], fx["cls_sample"])


def test_gradients_are_the_derivatives_of_the_losses(fx):
    """Central differences in float64 on a few elements, a self edge, a clamped row and a p = 0 entry among them."""
    g = np.random.default_rng(1)
    f = g.normal(size=(12, 5))
    f[3] = 1e-9 * g.normal(size=5)
    near, far = g.integers(0, 12, (12, 3)), g.integers(0, 12, (12, 2))
    near[:, 0] = np.arange(12)
    r = dr.feature3d(f, near, far, 0.7, 1.3)
    for i, d, h in ((0, 0, 1e-6), (3, 2, 1e-12), (7, 4, 1e-6)):
        fp, fm = f.copy(), f.copy()
        fp[i, d] += h
        fm[i, d] -= h
        num = (dr.feature3d(fp, near, far, 0.7, 1.3)["loss"] - dr.feature3d(fm, near, far, 0.7, 1.3)["loss"]) / (2 * h)
        assert abs(num - r["grad"][i, d]) <= 1e-5 * max(abs(num), 1e-3), (i, d, num, r["grad"][i, d])
    p = g.uniform(0.05, 1.0, (9, 4))
    sample, idx = np.array([2, 5, 7]), g.integers(0, 9, (3, 3))
    idx[:, 0] = sample
    r = dr.cls3d(p, sample, idx, 2.0)
    for n, c in ((2, 0), (int(idx[1, 2]), 1), (7, 3)):
        pp, pm = p.copy(), p.copy()
        pp[n, c] += 1e-6
        pm[n, c] -= 1e-6
        num = (dr.cls3d(pp, sample, idx, 2.0)["loss"] - dr.cls3d(pm, sample, idx, 2.0)["loss"]) / 2e-6
        assert abs(num - r["grad"][n, c]) <= 1e-6 * max(abs(num), 1e-3), (n, c)


def test_key_order_on_ties_and_nans():
    inf, nan = np.inf, np.nan
    d2 = np.array([[4.0, 1.0, 4.0, nan, 0.0, inf, 1.0, -nan]], dtype=np.float32)
    nd, ni, fd, fi = dr.topk_by_keys(d2, 8, 8)
    assert ni[0].tolist() == [4, 1, 6, 0, 2, 5, 3, 7]                      # distance, then id; +inf, then the NaNs by id
    assert fi[0].tolist() == [3, 7, 5, 0, 2, 1, 6, 4]                      # the NaNs first, then +inf, then larger distance, lower id
    assert nd.view(np.uint32)[0, 6:].tolist() == [dr.NAN_BITS] * 2         # either NaN comes back as the canonical bits
    assert fd.view(np.uint32)[0, :2].tolist() == [dr.NAN_BITS] * 2
    near, far = dr.keys_of(d2)
    assert len(set(near[0].tolist())) == 8 and len(set(far[0].tolist())) == 8
    assert near.max() < 2 ** 64 - 1 and far.max() < 2 ** 64 - 1            # the empty-slot key ~0 is no key
    same = np.zeros((3, 7), dtype=np.float32)                              # all coincident: ids 0 .. k-1 at both ends
    nd, ni, fd, fi = dr.topk_by_keys(same, 4, 3)
    assert (ni == np.arange(4)).all() and (fi == np.arange(3)).all() and not nd.any() and not fd.any()
    # torch's topk puts NaN above +inf as well
    t = torch.tensor([1.0, nan, inf, 0.0])
    assert set(t.topk(2, largest=True)[1].tolist()) == {1, 2} and t.topk(1, largest=True)[1].item() == 1
    assert t.topk(3, largest=False)[1].tolist() == [3, 0, 2]


def test_distance_chain_is_exact_on_the_lattice():
    q, p = dr.lattice(40, 64, 1), dr.lattice(50, 64, 2)
    a, b = dr.dist2(q, p, np.float32), dr.dist2(q, p, np.float64)
    assert np.array_equal(a.astype(np.float64), b) and b.max() <= 64 * 64 and np.array_equal(b, np.round(b))
    assert np.array_equal(dr.dist2(p, q, np.float32), a.T)                 # d(i, j) == d(j, i)


def test_exact_plan_meets_every_class():
    from trase_amd.neighbors import dense_topk_splits
    cases = dr.EXACT_CASES
    Ms, Ns = {c[0] for c in cases}, {c[1] for c in cases}
    assert {1, 255, 256, 257} <= Ms and max(Ms) > 257
    assert {63, 64, 65} <= Ns
    assert any(c[1] == max(c[3], c[4]) for c in cases)                                        # N = k exactly
    assert {c[2] for c in cases} >= set(dr.EXACT_D)
    assert {c[3] for c in cases if c[3]} >= set(dr.EXACT_K) and {c[4] for c in cases if c[4]} >= set(dr.EXACT_K)
    assert any(c[3] and c[4] for c in cases) and any(c[3] and not c[4] for c in cases) and any(c[4] and not c[3] for c in cases)
    assert {c[5] for c in cases} == {"self", "cross", "coincident", "nan_query", "nan_point"}
    assert any(c[6] and c[2] % 4 == 0 for c in cases)                                         # off alignment where float4 loads would run
    splits = [dense_topk_splits(*c[:5]) for c in cases]
    assert 1 in splits and max(splits) > 1
    assert any(s == 1 and c[1] > 64 for s, c in zip(splits, cases))                           # S = 1 over several tiles
    ragged = [c for s, c in zip(splits, cases) if s > 1 and c[1] % 64 != 0 and c[1] > 64 * (s - 1)]
    assert ragged                                                                             # a short last column range at S > 1
    for c in cases:                                                                           # the premise of exactness
        q, p = dr.exact_case(c)
        ok = np.isfinite(q).all(1)[:, None] & np.isfinite(p).all(1)[None, :] if c[0] * c[1] <= 10 ** 6 else None
        if ok is not None:
            d = dr.dist2(q, p)
            assert np.array_equal(d[ok], np.round(d[ok])) and d[ok].max() < 2 ** 24
    # the three list widths: 256, 128 and 64 rows per workgroup
    assert {min(256, 128 if c[3] + c[4] > 24 else 256, 64 if c[3] + c[4] > 48 else 256) for c in cases} == {64, 128, 256}


def test_random_scenes_have_few_near_ties():
    for name, (q, p, kn, kf) in dr.random_scenes().items():
        ref = dr.topk_f64(q, p, kn, kf)
        tie = dr.near_tie_rows(ref, q.shape[1], kn, kf)
        print(f"{name}: {int(tie.sum())} of {len(q)} rows set aside")
        assert tie.sum() <= max(3, len(q) / 100), name


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_come_before_any_device():
    from trase_amd import _lib
    lib = _lib.load()
    nbytes, splits = C.c_size_t(), C.c_int32()
    ok = lib.trase_dense_topk_ws_bytes(800, 200000, 32, 5, 0, C.byref(nbytes), C.byref(splits))
    assert ok == 0 and splits.value == 64 and nbytes.value >= 800 * 64 * 5 * 8
    assert lib.trase_dense_topk_ws_bytes(300000, 300000, 3, 16, 4, C.byref(nbytes), C.byref(splits)) == 0
    assert splits.value == 1 and nbytes.value == 0
    assert lib.trase_dense_topk_ws_bytes(10, 10, 3, 1, 1, None, None) == INVALID
    p = C.c_void_p(4096)          # never dereferenced: every call below returns before a device is touched
    for M, N, D, kn, kf in ((-1, 10, 3, 1, 1), (10, 0, 3, 1, 0), (10, 10, 0, 1, 1), (10, 10, 65, 1, 1), (10, 10, 3, 0, 0),
                            (10, 10, 3, 33, 0), (10, 10, 3, 0, 33), (10, 10, 3, -1, 2), (10, 5, 3, 6, 0), (10, 5, 3, 1, 6)):
        assert lib.trase_dense_topk_ws_bytes(M, N, D, kn, kf, C.byref(nbytes), None) == INVALID, (M, N, D, kn, kf)
        assert lib.trase_dense_topk(p, M, p, N, D, kn, kf, p, p, p, p, p, 1 << 30, 0, None) == INVALID, (M, N, D, kn, kf)
    assert b"trase_dense_topk" in lib.trase_last_error()
    assert lib.trase_dense_topk(None, 10, p, 10, 3, 1, 1, p, p, p, p, p, 1 << 30, 0, None) == INVALID
    assert lib.trase_dense_topk(p, 10, p, 10, 3, 1, 1, p, None, p, p, p, 1 << 30, 0, None) == INVALID
    assert lib.trase_dense_topk(p, 10, p, 10, 3, 1, 1, p, p, None, p, p, 1 << 30, 0, None) == INVALID
    assert b"null pointer" in lib.trase_last_error()
    assert lib.trase_dense_topk(p, 0, p, 10, 3, 1, 1, p, p, p, p, None, 0, 0, None) == 0               # M = 0: nothing to do
    assert lib.trase_dense_topk(p, 10, p, 1000, 3, 1, 1, p, p, p, p, p, 64, 0, None) == WORKSPACE     # S > 1 needs its lists
    assert lib.trase_dense_topk(p, 10, p, 1000, 3, 1, 1, p, p, p, p, None, 1 << 30, 0, None) == WORKSPACE
    # the transpose with two counts
    assert lib.trase_graph_reverse_to_ws_bytes(800, 5, 200000, C.byref(nbytes)) == 0 and nbytes.value > 0
    sq = C.c_size_t()
    assert lib.trase_graph_reverse_ws_bytes(300, 7, C.byref(sq)) == 0
    assert lib.trase_graph_reverse_to_ws_bytes(300, 7, 300, C.byref(nbytes)) == 0 and nbytes.value == sq.value
    for rows, k, targets in ((0, 5, 10), (10, 0, 10), (10, 5, 0), (10, 5, -1), (10, 5, 2 ** 31 - 1), (2 ** 30, 2, 10)):
        assert lib.trase_graph_reverse_to_ws_bytes(rows, k, targets, C.byref(nbytes)) == INVALID, (rows, k, targets)
        assert lib.trase_graph_reverse_to(p, rows, k, targets, p, p, p, 1 << 30, 0, None) == INVALID
    assert lib.trase_graph_reverse_to_ws_bytes(10, 5, 10, None) == INVALID
    assert lib.trase_graph_reverse_to(None, 10, 5, 10, p, p, p, 1 << 30, 0, None) == INVALID
    assert lib.trase_graph_reverse_to(p, 10, 5, 10, p, p, p, 8, 0, None) == WORKSPACE
    # the two losses
    assert lib.trase_feature3d_ws_bytes(300000, C.byref(nbytes)) == 0 and nbytes.value >= 8 * (300000 // 256 + 1)
    assert lib.trase_feature3d_ws_bytes(0, C.byref(nbytes)) == INVALID and lib.trase_feature3d_ws_bytes(10, None) == INVALID
    for rows, D, kp, kn in ((0, 8, 1, 1), (2 ** 25, 8, 1, 1), (10, 0, 1, 1), (10, 65, 1, 1), (10, 8, 0, 1), (10, 8, 1, 0), (10, 8, 33, 1),
                            (10, 8, 1, 33)):
        assert lib.trase_feature3d_forward(p, p, rows, D, kp, kn, 1.0, 1.0, p, p, p, p, 1 << 30, 0, None) == INVALID
        assert lib.trase_feature3d_backward(p, p, p, p, p, rows, D, kp, kn, 1.0, 1.0, p, p, 0, None) == INVALID
    assert lib.trase_feature3d_forward(p, None, 10, 8, 1, 1, 1.0, 1.0, p, p, p, p, 1 << 30, 0, None) == INVALID
    assert lib.trase_feature3d_forward(p, p, 10, 8, 1, 1, 1.0, 1.0, p, p, p, p, 8, 0, None) == WORKSPACE
    assert lib.trase_feature3d_backward(p, p, p, p, None, 10, 8, 1, 1, 1.0, 1.0, p, p, 0, None) == INVALID
    assert lib.trase_cls3d_ws_bytes(800, 256, C.byref(nbytes)) == 0 and nbytes.value >= 8 * 800
    assert lib.trase_cls3d_ws_bytes(800, 257, C.byref(nbytes)) == INVALID and lib.trase_cls3d_ws_bytes(0, 4, C.byref(nbytes)) == INVALID
    for S, N, Cn, k in ((0, 10, 4, 1), (5, 0, 4, 1), (5, 10, 0, 1), (5, 10, 257, 1), (5, 10, 4, 0), (5, 2 ** 24, 256, 1)):
        assert lib.trase_cls3d_forward(p, p, p, S, N, Cn, k, 2.0, p, p, 1 << 30, 0, None) == INVALID, (S, N, Cn, k)
        assert lib.trase_cls3d_backward(p, p, p, p, p, p, p, S, N, Cn, k, 2.0, p, p, 0, None) == INVALID, (S, N, Cn, k)
    assert lib.trase_cls3d_forward(p, p, p, 11, 10, 4, 1, 2.0, p, p, 1 << 30, 0, None) == INVALID      # more samples than rows
    assert lib.trase_cls3d_forward(p, p, None, 5, 10, 4, 1, 2.0, p, p, 1 << 30, 0, None) == INVALID
    assert lib.trase_cls3d_forward(p, p, p, 5, 10, 4, 1, 2.0, p, p, 8, 0, None) == WORKSPACE
    assert lib.trase_cls3d_backward(p, p, p, p, p, p, None, 5, 10, 4, 1, 2.0, p, p, 0, None) == INVALID


def test_python_refusals_come_before_any_device():
    from trase_amd.losses import dense_topk, loss_cls_3d, loss_feature3d
    from trase_amd.neighbors import NeighborGraph
    q, p = torch.zeros(4, 3), torch.zeros(10, 3)
    for args in ((q, p, 0, 0), (q, p, 33, 0), (q, p, 0, 33), (q, p, -1, 1), (q, p, 11, 0), (q, p, 0, 11), (q, torch.zeros(10, 4), 1, 0),
                 (q.double(), p.double(), 1, 0), (torch.zeros(4, 65), torch.zeros(10, 65), 1, 0), (torch.zeros(4), p, 1, 0),
                 (torch.zeros(4, 0), torch.zeros(10, 0), 1, 0)):
        with pytest.raises(ValueError, match="dense_topk"):
            dense_topk(*args)
    with pytest.raises(ValueError, match="larger than the 10 points"):
        dense_topk(q, p, 11)
    with pytest.raises(RuntimeError, match="GPU only"):
        dense_topk(q, p, 1)
    f, x = torch.zeros(20, 8), torch.zeros(20, 3)
    for kw in (dict(kp=0), dict(kn=0), dict(kp=33), dict(kn=33), dict(kp=21, kn=4), dict(max_points=0), dict(max_points=-1),
               dict(max_points=2.5), dict(kp=16, max_points=10), dict(neighbors=(torch.zeros(20, 3), torch.zeros(20, 4))),
               dict(neighbors=(torch.zeros(20, 16),))):
        with pytest.raises(ValueError, match="loss_feature3d"):
            loss_feature3d(f, x, **kw)
    for a, b in ((torch.zeros(20, 65), x), (torch.zeros(20), x), (f, torch.zeros(19, 3)), (f, torch.zeros(20, 65))):
        with pytest.raises(ValueError, match="loss_feature3d"):
            loss_feature3d(a, b)
    with pytest.raises(RuntimeError, match="GPU only"):
        loss_feature3d(f, x)
    pr = torch.zeros(20, 4)
    for kw in (dict(k=0), dict(k=33), dict(k=21), dict(max_points=0), dict(sample_size=0), dict(k=5, max_points=4),
               dict(sample=torch.zeros(0, dtype=torch.int64)), dict(sample=torch.zeros(3)), dict(sample=torch.zeros(3, 1, dtype=torch.int64))):
        with pytest.raises(ValueError, match="loss_cls_3d"):
            loss_cls_3d(f, pr, **kw)
    for a, b in ((torch.zeros(20, 65), pr), (f, torch.zeros(19, 4)), (f, torch.zeros(20, 257)), (f, torch.zeros(20, 0)), (f, torch.zeros(20))):
        with pytest.raises(ValueError, match="loss_cls_3d"):
            loss_cls_3d(a, b)
    with pytest.raises(RuntimeError, match="GPU only"):
        loss_cls_3d(f, pr)
    with pytest.raises(RuntimeError, match="GPU only"):
        NeighborGraph.from_idx(torch.zeros(4, 2, dtype=torch.int32), num_targets=9)
