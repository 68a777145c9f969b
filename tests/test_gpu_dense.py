"""dense_topk, the transpose with two counts, loss_feature3d and loss_cls_3d on the GPU against tests/dense_reference.py.

Exact search: lattice rows (integers in {-4..4}), so every squared distance is an integer below 2^24 and fp32 is exact in any
order (tests/test_dense_reference.py asserts the premise and that the plan meets every size class): distances and indices must
EQUAL the numpy selection by the two 64-bit keys, with a 0xCD canary behind every output and a bit-identical second call.

Random clouds: distances within (D + 3) 2^-24 relative of float64; every row's index set equal to float64's except rows whose
float64 gap at the k-th place is at most 4 (D + 1) 2^-24 of the larger distance, at most max(3, M / 100) of them.

Losses and gradients on the indices the device found, against the float64 restatement; the bar is four times the error of the
reference's own fp32 torch statements on the same inputs and indices, floor 2^-22 of the float64 abs-sum, by the groups that
tests/dense_reference.py describes.  The measured ratios are kept in profiles/dense_losses_bench.json under "tests".

Measured on an MI355X (this file's own output): random clouds: largest relative distance error 2.07e-7 / 3.11e-7 / 5.51e-7 at
D = 3 / 32 / 64 (bounds 3.58e-7 / 2.09e-6 / 3.99e-6), 0, 1 and 1 rows set aside, no other row's index set differing; 65 537
rows: 15 (row, end) pairs set aside, no other differing; the losses at most 0.442 of the bar, the gradients at most 0.765 (the
16 elements of the two clamped rows at rows = 255, D = 32; the other rows at most 0.409)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import dense_reference as dr

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY32, CANARY64 = -0x32323233, -0x3232323232323233          # 0xCD bytes
HERE = os.path.dirname(os.path.abspath(__file__))


def dev_tensor(a, misaligned=False):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not misaligned:
        return torch.from_numpy(a).to(DEV)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)          # the base pointer 4 bytes off 16-byte alignment
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def topk_raw(q, p, kn, kf, tail=64):
    """trase_dense_topk into buffers with `tail` elements of 0xCD behind all four outputs."""
    from trase_amd import _lib
    from trase_amd.rasterizer import _bytes, _stream
    lib = _lib.load()
    dev = torch.device(DEV, torch.cuda.current_device())
    (M, D), N = q.shape, p.shape[0]
    nd = torch.full((M * kn + tail,), CANARY32, dtype=torch.int32, device=DEV)
    fd = torch.full((M * kf + tail,), CANARY32, dtype=torch.int32, device=DEV)
    ni = torch.full((M * kn + tail,), CANARY64, dtype=torch.int64, device=DEV)
    fi = torch.full((M * kf + tail,), CANARY64, dtype=torch.int64, device=DEV)
    nbytes, splits = C.c_size_t(), C.c_int32()
    _lib.check(lib.trase_dense_topk_ws_bytes(M, N, D, kn, kf, C.byref(nbytes), C.byref(splits)), "trase_dense_topk_ws_bytes")
    assert (splits.value > 1) == (nbytes.value > 0)
    ws = _bytes(nbytes.value, dev)
    _lib.check(lib.trase_dense_topk(_lib.ptr(q), M, _lib.ptr(p), N, D, kn, kf, _lib.ptr(nd), _lib.ptr(ni), _lib.ptr(fd), _lib.ptr(fi),
                                    _lib.ptr(ws), nbytes.value, dev.index, _stream(dev)), "trase_dense_topk")
    torch.cuda.synchronize()
    out = {}
    intact = True
    for name, t, k, can in (("near_d2", nd, kn, CANARY32), ("near_idx", ni, kn, CANARY64), ("far_d2", fd, kf, CANARY32),
                            ("far_idx", fi, kf, CANARY64)):
        a = t.cpu().numpy()
        intact &= bool((a[M * k:] == can).all())
        out[name] = a[:M * k].reshape(M, k).copy()
    out["intact"], out["splits"] = intact, splits.value
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("case", dr.EXACT_CASES, ids=lambda c: f"M{c[0]}-N{c[1]}-D{c[2]}-k{c[3]}+{c[4]}-{c[5]}" + ("-off16" if c[6] else ""))
def test_dense_topk_exact(case):
    from trase_amd.neighbors import dense_topk_splits
    M, N, D, kn, kf, kind, mis = case
    q, p = dr.exact_case(case)
    pd = dev_tensor(p, mis)
    qd = pd if q is p else dev_tensor(q, mis)
    a, b = topk_raw(qd, pd, kn, kf), topk_raw(qd, pd, kn, kf)
    assert a["intact"] and b["intact"], "a write behind the outputs"
    for name in ("near_d2", "near_idx", "far_d2", "far_idx"):
        assert a[name].tobytes() == b[name].tobytes(), name
    assert a["splits"] == dense_topk_splits(M, N, D, kn, kf) and (a["splits"] == 1 or N > 64)
    rd, ri, fd, fi = dr.topk_by_keys(dr.dist2(q, p, np.float32), kn, kf)
    assert np.array_equal(a["near_idx"], ri) and np.array_equal(a["far_idx"], fi)
    assert np.array_equal(a["near_d2"].view(np.uint32), bits(rd)) and np.array_equal(a["far_d2"].view(np.uint32), bits(fd))
    if kind == "coincident":
        assert (a["near_idx"] == np.arange(kn)).all() and (a["far_idx"] == np.arange(kf)).all()
    if kind == "nan_query":
        r = M // 2
        assert (a["near_idx"][r] == np.arange(kn)).all() and (a["far_idx"][r] == np.arange(kf)).all()
        assert (a["near_d2"].view(np.uint32)[r] == dr.NAN_BITS).all() and (a["far_d2"].view(np.uint32)[r] == dr.NAN_BITS).all()
    if kind == "nan_point":
        assert (a["far_idx"][:, 0] == N // 3).all() and not (a["near_idx"] == N // 3).any()
    assert np.array_equal(bits(qd.cpu().numpy()), bits(q)) and np.array_equal(bits(pd.cpu().numpy()), bits(p))      # inputs unmodified


def test_both_launch_forms_run():
    """S = 1 is the sweep alone, S > 1 the sweep and the merge: read off the profiler's scopes."""
    from trase_amd import rasterizer as R
    from trase_amd.losses import dense_topk
    seen = {}
    for M, N in ((200, 64), (200, 1000)):
        q, p = dev_tensor(dr.lattice(M, 3, 1)), dev_tensor(dr.lattice(N, 3, 2))
        R.profile_enable(1)
        try:
            out = dense_topk(q, p, 4, 2)
            torch.cuda.synchronize()
            rep = R.profile_report()
        finally:
            R.profile_enable(0)
        seen[N] = {k: int(v["n"]) for k, v in rep.items()}
        ref = dr.topk_by_keys(dr.dist2(q.cpu().numpy(), p.cpu().numpy(), np.float32), 4, 2)
        assert all(np.array_equal(g.cpu().numpy(), r) for g, r in zip(out, ref))
        assert out[1].dtype == torch.int64 and out[0].dtype == torch.float32
    assert seen[64] == {"dense_topk_sweep": 1} and seen[1000] == {"dense_topk_sweep": 1, "dense_topk_merge": 1}


def test_dense_topk_empty_ends_and_no_queries():
    from trase_amd.losses import dense_topk
    p = dev_tensor(dr.lattice(50, 5, 3))
    nd, ni, fd, fi = dense_topk(p[:7], p, k_near=3)
    assert nd.shape == (7, 3) and fd.shape == (7, 0) and fi.shape == (7, 0) and fi.dtype == torch.int64
    nd, ni, fd, fi = dense_topk(p[:0], p, 2, 2)
    assert nd.shape == (0, 2) and ni.shape == (0, 2) and fd.shape == (0, 2) and fi.shape == (0, 2)
    assert dense_topk(p, p, 0, 32)[3].shape == (50, 32)
    with pytest.raises(ValueError, match="larger than the 20 points"):
        dense_topk(p[:20], p[:20], 0, 21)


@pytest.mark.parametrize("name", ("cloud3", "unit32", "wide64"))
def test_dense_topk_random_clouds(name):
    q, p, kn, kf = dr.random_scenes()[name]
    M, D = q.shape
    pd = dev_tensor(p)
    qd = pd if q is p else dev_tensor(q)
    got = topk_raw(qd, pd, kn, kf)
    assert got["intact"]
    ref = dr.topk_f64(q, p, kn, kf)
    d64 = dr.dist2(q.astype(np.float64), p.astype(np.float64))
    tie = dr.near_tie_rows(ref, D, kn, kf)
    differ = np.zeros(M, dtype=bool)
    worst = 0.0
    for end, k in (("near", kn), ("far", kf)):
        if not k:
            continue
        idx, d2 = got[end + "_idx"], got[end + "_d2"].view(np.float32).astype(np.float64)
        exact = np.take_along_axis(d64, idx, axis=1)
        err = np.abs(d2 - exact) / np.maximum(exact, 1e-300)
        err[exact == 0] = np.abs(d2)[exact == 0]
        worst = max(worst, float(err.max()))
        order = np.diff(d2, axis=1)
        assert (order >= 0).all() if end == "near" else (order <= 0).all()
        differ |= np.array([set(a) != set(b) for a, b in zip(idx.tolist(), ref[end + "_idx"].tolist())])
    print(f"{name}: largest relative distance error {worst:.3e} (bound {(D + 3) * dr.U:.3e}); rows set aside {int(tie.sum())} of {M}; "
          f"rows whose index set differs {int(differ.sum())}")
    assert worst <= (D + 3) * dr.U
    assert tie.sum() <= max(3, M / 100)
    assert not differ[~tie].any()


# ---- the transposed graph with two counts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,k,targets", ((1, 1, 5), (800, 5, 3000), (63, 128, 10), (1025, 3, 64), (64, 7, 65)))
def test_reversal_to(rows, k, targets):
    from trase_amd.neighbors import NeighborGraph
    g = np.random.default_rng(rows * 131 + k)
    idx = g.integers(0, targets, size=(rows, k)).astype(np.int32)
    if rows * k >= 8:                                        # edges to nowhere: -1, the target count, a large id
        flat = idx.reshape(-1)
        flat[g.choice(rows * k, 3, replace=False)] = (-1, targets, 2 ** 31 - 1)
    graph = NeighborGraph.from_idx(torch.from_numpy(idx).to(DEV), num_targets=targets)
    ranges, edges = dr.reverse_graph_to(idx, targets)
    got_r, got_e = graph.rev_ranges.cpu().numpy(), graph.rev_edges.cpu().numpy()
    valid = int(ranges[:, 1].max())
    assert got_r.shape == (targets, 2) and got_e.shape == (rows * k,) and graph.num_targets == targets
    assert np.array_equal(got_r, ranges)
    assert np.array_equal(got_e[:valid], edges[:valid])
    again = NeighborGraph.from_idx(torch.from_numpy(idx.astype(np.int64)).to(DEV), num_targets=targets)
    assert np.array_equal(again.rev_edges.cpu().numpy(), got_e) and np.array_equal(again.idx.cpu().numpy(), idx)


@pytest.mark.parametrize("N,k", ((1, 1), (65, 5), (1025, 128)))
def test_reversal_to_equals_the_square_entry(N, k):
    from trase_amd.neighbors import NeighborGraph
    idx = torch.from_numpy(np.random.default_rng(N + k).integers(-1, N + 1, size=(N, k)).astype(np.int32)).to(DEV)
    a, b = NeighborGraph.from_idx(idx), NeighborGraph.from_idx(idx, num_targets=N)
    valid = int(a.rev_ranges[:, 1].max())
    assert torch.equal(a.rev_ranges, b.rev_ranges) and torch.equal(a.rev_edges[:valid], b.rev_edges[:valid])


# ---- the two losses -----------------------------------------------------------------------------------------------------------------
def held(name, got, ref, t32, abs_sum, groups=None):
    """The largest error in units of its bar, group by group: (elements held, elements whose torch error is the measure)."""
    got, ref, t32, abs_sum = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in (got, ref, t32, abs_sum))
    if groups is None:
        groups = [(np.ones(ref.shape, dtype=bool),) * 2]
    worst = 0.0
    for sel, meas in groups:
        if not sel.any():
            continue
        measured = float(np.abs(t32 - ref)[meas].max()) if meas.any() else 0.0
        bar = np.maximum(4.0 * measured, 2.0 ** -22 * abs_sum[sel])
        err = np.abs(got - ref)[sel]
        ratio = float((err / np.maximum(bar, 1e-300)).max())
        print(f"  {name} ({int(sel.sum())} elements): kernels {err.max():.3e}, fp32 torch statements {measured:.3e}, "
              f"{ratio:.3f} of the bar")
        worst = max(worst, ratio)
    return worst


def torch_feature3d(f, near, far, lp, ln, dtype=torch.float32):
    """The reference's statements on the device in `dtype`, around given indices -> (loss, gradient)."""
    from torch.nn.functional import cosine_similarity
    t = torch.tensor(np.asarray(f), dtype=dtype, device=DEV, requires_grad=True)
    rows, kp, kn = len(f), near.shape[1], far.shape[1]
    nn_i, fn_i = torch.from_numpy(near.astype(np.int64)).to(DEV), torch.from_numpy(far.astype(np.int64)).to(DEV)
    an = torch.arange(rows, device=DEV).unsqueeze(-1).expand(rows, kp).reshape(-1)
    af = torch.arange(rows, device=DEV).unsqueeze(-1).expand(rows, kn).reshape(-1)
    loss = lp * torch.sigmoid(1 - cosine_similarity(t[an, :], t[nn_i.reshape(-1), :], dim=1)).mean() \
        + ln * torch.sigmoid(cosine_similarity(t[af, :], t[fn_i.reshape(-1), :], dim=1)).mean()
    loss.backward()
    return float(loss.detach()), t.grad.cpu().numpy()


def torch_cls3d(pred, sample, idx, lam, dtype=torch.float32):
    p = torch.tensor(np.asarray(pred), dtype=dtype, device=DEV, requires_grad=True)
    s = torch.from_numpy(np.asarray(sample).astype(np.int64)).to(DEV)
    j = torch.from_numpy(np.asarray(idx).astype(np.int64)).to(DEV)
    sp = p[s]
    kl = sp.unsqueeze(1) * (torch.log(sp.unsqueeze(1) + 1e-10) - torch.log(p[j] + 1e-10))
    loss = lam * (kl.sum(dim=-1).mean() / p.size(1))
    loss.backward()
    return float(loss.detach()), p.grad.cpu().numpy()


def run_feature3d(f, xyz, kp, kn, lp, ln, neighbors, g_out=0.75):
    """Two runs (bitwise equal, inputs unmodified) -> (loss, gradient)."""
    from trase_amd.losses import loss_feature3d
    outs = []
    for _ in range(2):
        ft = torch.from_numpy(f).to(DEV).requires_grad_(True)
        xt = torch.from_numpy(xyz).to(DEV)
        loss = loss_feature3d(ft, xt, kp, kn, None, lp, ln, neighbors=neighbors)
        (g_out * loss).backward()
        assert np.array_equal(bits(ft.detach().cpu().numpy()), bits(f)) and np.array_equal(bits(xt.cpu().numpy()), bits(xyz))
        outs.append((loss.detach().cpu().numpy().copy(), ft.grad.cpu().numpy().copy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    return float(outs[0][0]), outs[0][1] / g_out


def clamp_groups(f, special):
    rows = np.zeros(f.shape, dtype=bool)
    rows[list(special)] = True
    zero = np.zeros(f.shape, dtype=bool)
    zero[[r for r in special if not f[r].any()]] = True          # torch agrees with the rule on a zero row only
    return [(~rows, ~rows), (rows, zero)]


# rows, D, kp, kn, lambda_p, lambda_n, with a zero row and a row below the clamp
F3D_CASES = [(1, 1, 1, 1, 1.0, 1.0, False), (2, 8, 1, 1, 1.0, 1.0, False), (2, 32, 2, 2, 0.5, 2.0, False),
             (255, 32, 16, 4, 1.0, 1.0, True), (256, 64, 16, 4, 1.0, 1.0, False), (257, 1, 16, 4, 1.0, 1.0, False),
             (1025, 8, 16, 4, 0.7, 1.3, True), (300, 64, 1, 1, 1.0, 1.0, True), (257, 8, 1, 4, 1.0, 1.0, False)]


@pytest.mark.parametrize("rows,D,kp,kn,lp,ln,special", F3D_CASES)
def test_loss_feature3d(rows, D, kp, kn, lp, ln, special):
    from trase_amd.losses import dense_topk
    g = np.random.default_rng(1000 * rows + D + kp)
    xyz = g.uniform(-1, 1, (rows, 3)).astype(np.float32)
    f = g.normal(size=(rows, D)).astype(np.float32)
    rows_special = ()
    if special:
        f[5] = 0.0
        f[9] = (1e-9 * g.normal(size=D)).astype(np.float32)
        rows_special = (5, 9)
    xt = torch.from_numpy(xyz).to(DEV)
    _, near, _, far = dense_topk(xt, xt, kp, kn)
    near_np, far_np = near.cpu().numpy(), far.cpu().numpy()
    loss, grad = run_feature3d(f, xyz, kp, kn, lp, ln, (near, far))
    ref = dr.feature3d(f, near_np, far_np, lp, ln)
    t_loss, t_grad = torch_feature3d(f, near_np, far_np, lp, ln)
    print(f"loss_feature3d rows {rows} D {D} kp {kp} kn {kn}: {loss:.7f} (float64 {ref['loss']:.7f})")
    assert held("value", loss, ref["loss"], t_loss, ref["loss_abs"]) <= 1.0
    assert held("gradient", grad, ref["grad"], t_grad, ref["grad_abs"], clamp_groups(f, rows_special)) <= 1.0


# N, D, C, k, S, lambda, with p = 0 entries
CLS_CASES = [(1, 4, 1, 1, 1, 2.0, False), (2, 8, 16, 1, 2, 2.0, False), (255, 32, 16, 5, 100, 2.0, True), (256, 64, 256, 5, 256, 2.0, False),
             (257, 1, 1, 5, 50, 0.5, False), (1025, 8, 16, 5, 800, 2.0, True), (300, 32, 256, 1, 300, 2.0, True)]


def cls_scene(N, D, Cn, S, zeros, seed):
    g = np.random.default_rng(seed)
    feat = g.normal(size=(N, D)).astype(np.float32)
    if Cn == 1:
        pred = g.uniform(0.05, 1.0, (N, 1))
    else:
        logits = g.normal(0.0, 2.0, (N, Cn))
        pred = np.exp(logits) / np.exp(logits).sum(1, keepdims=True)
    pred = pred.astype(np.float32)
    if zeros:
        pred[g.random((N, Cn)) < 0.05] = 0.0
    sample = g.permutation(N)[:S].astype(np.int64)
    return feat, pred, sample


def run_cls3d(feat, pred, k, lam, sample, g_out=0.75):
    from trase_amd.losses import loss_cls_3d
    outs = []
    for _ in range(2):
        ft, pt = torch.from_numpy(feat).to(DEV), torch.from_numpy(pred).to(DEV).requires_grad_(True)
        loss = loss_cls_3d(ft, pt, k, lam, sample=torch.from_numpy(sample).to(DEV))
        (g_out * loss).backward()
        assert np.array_equal(bits(ft.cpu().numpy()), bits(feat)) and np.array_equal(bits(pt.detach().cpu().numpy()), bits(pred))
        outs.append((loss.detach().cpu().numpy().copy(), pt.grad.cpu().numpy().copy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    return float(outs[0][0]), outs[0][1] / g_out


@pytest.mark.parametrize("N,D,Cn,k,S,lam,zeros", CLS_CASES)
def test_loss_cls_3d(N, D, Cn, k, S, lam, zeros):
    from trase_amd.losses import dense_topk
    feat, pred, sample = cls_scene(N, D, Cn, S, zeros, 77 * N + Cn)
    ft = torch.from_numpy(feat).to(DEV)
    idx = dense_topk(ft[torch.from_numpy(sample).to(DEV)], ft, k_near=k)[1].cpu().numpy()
    assert np.array_equal(idx[:, 0], sample)                       # the sampled row itself is slot 0
    loss, grad = run_cls3d(feat, pred, k, lam, sample)
    ref = dr.cls3d(pred, sample, idx, lam)
    t_loss, t_grad = torch_cls3d(pred, sample, idx, lam)
    print(f"loss_cls_3d N {N} D {D} C {Cn} k {k} S {S}: {loss:.7f} (float64 {ref['loss']:.7f})")
    assert held("value", loss, ref["loss"], t_loss, ref["loss_abs"]) <= 1.0
    zero = pred == 0
    assert held("gradient", grad, ref["grad"], t_grad, ref["grad_abs"], [(~zero, ~zero), (zero, zero)]) <= 1.0
    untouched = np.ones(N, dtype=bool)
    untouched[idx.reshape(-1)] = False
    assert not grad[untouched].any()


def test_fixture_cases_meet_the_bar():
    from trase_amd.losses import dense_topk
    fx = np.load(os.path.join(HERE, "golden", "dense_losses.npz"))
    xt = torch.from_numpy(fx["f3d_xyz"]).to(DEV)
    _, near, _, far = dense_topk(xt, xt, 16, 4)
    assert np.array_equal(np.sort(near.cpu().numpy(), 1), np.sort(fx["f3d_near_idx"], 1))
    assert np.array_equal(np.sort(far.cpu().numpy(), 1), np.sort(fx["f3d_far_idx"], 1))
    loss, grad = run_feature3d(fx["f3d_feats"], fx["f3d_xyz"], 16, 4, 1.0, 1.0, (near, far))
    ref = dr.feature3d(fx["f3d_feats"], fx["f3d_near_idx"], fx["f3d_far_idx"])
    print("fixture, loss_feature3d (the bar from the reference's own fp32 CPU run):")
    assert held("value", loss, fx["f3d_loss_f64"], fx["f3d_loss_f32"], ref["loss_abs"]) <= 1.0
    assert held("gradient", grad, fx["f3d_grad_f64"], fx["f3d_grad_f32"], ref["grad_abs"]) <= 1.0
    ft = torch.from_numpy(fx["cls_features"]).to(DEV)
    sample = fx["cls_sample"].astype(np.int64)
    idx = dense_topk(ft[torch.from_numpy(sample).to(DEV)], ft, k_near=5)[1].cpu().numpy()
    assert np.array_equal(np.sort(idx, 1), np.sort(fx["cls_idx"], 1))
    loss, grad = run_cls3d(fx["cls_features"], fx["cls_predictions"], 5, 2.0, sample)
    ref = dr.cls3d(fx["cls_predictions"], sample, fx["cls_idx"])
    print("fixture, loss_cls_3d:")
    assert held("value", loss, fx["cls_loss_f64"], fx["cls_loss_f32"], ref["loss_abs"]) <= 1.0
    assert held("gradient", grad, fx["cls_grad_f64"], fx["cls_grad_f32"], ref["grad_abs"]) <= 1.0


def test_given_neighbours_and_sample_equal_the_searched_ones():
    from trase_amd.losses import dense_topk, loss_cls_3d, loss_feature3d
    g = np.random.default_rng(21)
    xyz, f = g.uniform(-1, 1, (700, 3)).astype(np.float32), g.normal(size=(700, 16)).astype(np.float32)
    xt = torch.from_numpy(xyz).to(DEV)

    def f3d(**kw):
        ft = torch.from_numpy(f).to(DEV).requires_grad_(True)
        loss = loss_feature3d(ft, xt, **kw)
        loss.backward()
        return loss.detach().cpu().numpy().tobytes(), ft.grad.cpu().numpy().tobytes(), ft.grad.cpu().numpy()
    _, near, _, far = dense_topk(xt, xt, 16, 4)
    assert f3d()[:2] == f3d(neighbors=(near, far))[:2] == f3d(max_points=None)[:2] == f3d(max_points=700)[:2]
    torch.manual_seed(11)
    sub = f3d(max_points=100)
    torch.manual_seed(11)
    pick = torch.randperm(700)[:100]
    ft = torch.from_numpy(f[pick.numpy()]).to(DEV).requires_grad_(True)
    loss = loss_feature3d(ft, xt[pick.to(DEV)])
    loss.backward()
    assert loss.detach().cpu().numpy().tobytes() == sub[0]
    rows = np.zeros(700, dtype=bool)
    rows[pick.numpy()] = True
    assert not sub[2][~rows].any() and np.array_equal(sub[2][pick.numpy()], ft.grad.cpu().numpy())
    feat, pred, _ = cls_scene(900, 32, 16, 1, False, 4)

    def cls(seed, **kw):
        pt = torch.from_numpy(pred).to(DEV).requires_grad_(True)
        torch.manual_seed(seed)
        loss = loss_cls_3d(torch.from_numpy(feat).to(DEV), pt, **kw)
        loss.backward()
        return loss.detach().cpu().numpy().tobytes(), pt.grad.cpu().numpy().tobytes()
    torch.manual_seed(3)
    sample = torch.randperm(900)[:800]
    assert cls(3) == cls(99, sample=sample.to(DEV)) == cls(99, sample=sample.to(torch.int32))
    twice = torch.cat([sample[:10], sample[:10]])                     # a row sampled twice counts twice
    a, b = cls(0, sample=twice), cls(0, sample=sample[:10])
    assert np.allclose(np.frombuffer(a[1], np.float32), np.frombuffer(b[1], np.float32), rtol=1e-5, atol=1e-9)
    assert np.allclose(np.frombuffer(a[0], np.float32), np.frombuffer(b[0], np.float32), rtol=1e-5)


def test_loss_feature3d_on_every_row():
    """max_points=None at 65 537 rows (two column ranges) against a chunked float64 evaluation of the same rule."""
    from trase_amd.losses import dense_topk, loss_feature3d
    rows, D, kp, kn = 65537, 8, 16, 4
    g = np.random.default_rng(65537)
    xyz, f = g.uniform(-1, 1, (rows, 3)).astype(np.float32), g.normal(size=(rows, D)).astype(np.float32)
    xt = torch.from_numpy(xyz).to(DEV)
    ft = torch.from_numpy(f).to(DEV).requires_grad_(True)
    loss = loss_feature3d(ft, xt, kp, kn, max_points=None)
    loss.backward()
    nd, near, fd, far = dense_topk(xt, xt, kp, kn)
    # float64 selection in query chunks on the device: (distance, id) order at both ends
    x64 = xt.double()
    set_aside = wrong = 0
    for lo in range(0, rows, 2048):
        d = ((x64[lo:lo + 2048, None, :] - x64[None, :, :]) ** 2).sum(-1)
        for k, idx, largest in ((kp, near, False), (kn, far, True)):
            v, i = d.topk(k + 1, dim=1, largest=largest)
            gap = (v[:, k] - v[:, k - 1]).abs() <= 4 * (3 + 1) * dr.U * torch.maximum(v[:, k], v[:, k - 1])
            same = (i[:, :k].sort(1)[0] == idx[lo:lo + 2048].sort(1)[0]).all(1)
            set_aside += int(gap.sum())
            wrong += int((~same & ~gap).sum())
    print(f"65 537 rows: {set_aside} (row, end) pairs set aside as near ties, {wrong} other index sets differ")
    assert wrong == 0 and set_aside <= rows / 100
    near_np, far_np = near.cpu().numpy(), far.cpu().numpy()
    ref = dr.feature3d(f, near_np, far_np)
    t_loss, t_grad = torch_feature3d(f, near_np, far_np, 1.0, 1.0)
    assert held("value", float(loss.detach()), ref["loss"], t_loss, ref["loss_abs"]) <= 1.0
    assert held("gradient", ft.grad.cpu().numpy(), ref["grad"], t_grad, ref["grad_abs"]) <= 1.0
