"""The in-kernel rotation of the rigid-motion loss on the GPU: polar_rotation, rigid_fit and
loss_rigid_body_motion_reg_loss(..., rotation="polar") against tests/rigid_reference.py (float64) within its derived bounds, the fused
kernel pinned bit for bit to the tested operators, and the scenes the SVD path cannot be asked to pass.  The premises of the
scenes are counted in float64 by tests/test_rigid_reference.py.

Measured on an MI355X (this file's own output, kept in profiles/rigid_bench.json under "tests"): R at 0.500 of its bound (the final
rounding), gS at most 0.003; rigid_fit: r at most 0.172 of its bound, a gradient at most 0.087, fused and composition alike; the
whole loss 1.3e-13 to 9.4e-6 from float64 where the fp32 compositions are 2.1e-12 to 2.0e-5, gradients 6.0e-8 to 2.4e-4 against
2.4e-7 to 3.0e-4; on the three scenes held to the derived bound alone at most 0.012 of it."""
import os

import numpy as np
import pytest
import torch

from tests import neighbors_reference as nr
from tests import rigid_reference as rg
from tests import test_gpu_neighbors as tgn

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = -0x32323233            # 0xCDCDCDCD
TAIL = 64


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def canary_buf(n):
    return torch.full((n + TAIL,), CANARY, dtype=torch.int32, device=DEV).view(torch.float32)


def intact(buf, n):
    return bool((buf.view(torch.int32)[n:] == CANARY).all())


def frac(tag, got, want, bound):
    f = float((np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(bound, 1e-300)).max()) if np.size(want) else 0.0
    print(f"  {tag}: {f:.3f} of the bound")
    return f


def raw_polar(S, G):
    """trase_polar3_forward / _backward into buffers with a 0xCD tail -> (R, gS) numpy."""
    from trase_amd import _lib
    from trase_amd.rasterizer import _stream
    lib = _lib.load()
    n = len(S)
    d = torch.device(DEV, torch.cuda.current_device())
    s, g = dev(S.reshape(-1)), dev(G.reshape(-1))
    R, gS = canary_buf(9 * n), canary_buf(9 * n)
    _lib.check(lib.trase_polar3_forward(_lib.ptr(s), n, _lib.ptr(R), d.index, _stream(d)), "trase_polar3_forward")
    _lib.check(lib.trase_polar3_backward(_lib.ptr(s), _lib.ptr(R), _lib.ptr(g), n, _lib.ptr(gS), d.index, _stream(d)),
               "trase_polar3_backward")
    torch.cuda.synchronize()
    assert intact(R, 9 * n) and intact(gS, 9 * n)
    return R[:9 * n].cpu().numpy().reshape(n, 3, 3), gS[:9 * n].cpu().numpy().reshape(n, 3, 3)


def api_polar(S, G):
    from trase_amd.losses import polar_rotation
    s = dev(S, True)
    R = polar_rotation(s)
    R.backward(dev(G))
    return R.detach().cpu().numpy(), s.grad.cpu().numpy()


def polar_both(S, G):
    """The operator through the C ABI (canaries) and twice through the Python API: one set of bits."""
    S, G = np.ascontiguousarray(S, dtype=np.float32), np.ascontiguousarray(G, dtype=np.float32)
    R, gS = raw_polar(S, G)
    for _ in range(2):
        R2, g2 = api_polar(S, G)
        assert R2.tobytes() == R.tobytes() and g2.tobytes() == gS.tobytes()
    return R, gS


@pytest.mark.parametrize("name", tuple(rg.polar_cases()))
def test_polar_rotation(name):
    S = rg.polar_cases()[name]
    G = np.random.default_rng(len(name)).normal(size=S.shape).astype(np.float32)
    R, gS = polar_both(S, G)
    R64, sig = rg.polar3(S)
    print(f"polar_rotation, {name}: cond up to {rg.cond_of(sig)[1].max():.2e}")
    assert np.array_equal(np.sign(np.linalg.det(R.astype(np.float64))), np.sign(np.linalg.det(S.astype(np.float64))))
    assert frac("R", R.reshape(len(S), -1), R64.reshape(len(S), -1), rg.polar3_bound(sig)[:, None]) <= 1.0
    want = rg.polar3_bwd(S, R64, G)
    assert frac("gS", gS.reshape(len(S), -1), want.reshape(len(S), -1), rg.polar3_bwd_bound(sig, G)[:, None]) <= 1.0


@pytest.mark.parametrize("N", (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1025))
def test_polar_rotation_sizes(N):
    cases = rg.polar_cases()
    pool = np.concatenate([cases["random"], cases["reflections"], cases["near_equal"], cases["equal"]])
    S = pool[(np.arange(N) * 7) % len(pool)]
    G = np.random.default_rng(N).normal(size=S.shape).astype(np.float32)
    R, gS = polar_both(S, G)
    R64, sig = rg.polar3(S)
    assert frac(f"N {N}: R", R.reshape(N, -1), R64.reshape(N, -1), rg.polar3_bound(sig)[:, None]) <= 1.0
    assert frac(f"N {N}: gS", gS.reshape(N, -1), rg.polar3_bwd(S, R64, G).reshape(N, -1), rg.polar3_bwd_bound(sig, G)[:, None]) <= 1.0


def test_polar_rotation_degenerate_and_non_finite_rows():
    g = np.random.default_rng(41)
    rank1 = np.einsum("na,nb->nab", g.normal(size=(40, 3)), g.normal(size=(40, 3)))
    rank2 = rg.matrices_with_sigma((1.0, 0.5, 0.0), 60, 23)
    rank2[:20, :, 2] = 0.0
    rank2[20:40, 2, :] = 0.0
    generic = g.normal(size=(30, 3, 3))
    bad = g.normal(size=(3, 3, 3))
    bad[0, 0, 0], bad[1, 2, 1], bad[2, 1, 1] = np.nan, np.inf, -np.inf
    S = np.concatenate([np.zeros((2, 3, 3)), rank1, rank2, bad, generic]).astype(np.float32)
    G = g.normal(size=S.shape).astype(np.float32)
    R, gS = polar_both(S, G)
    # rank <= 1: an orthogonal R (I for S = 0), a zero gradient
    z, r1 = slice(0, 2), slice(2, 42)
    assert np.array_equal(R[z], np.stack([np.eye(3, dtype=np.float32)] * 2)) and not gS[z].any() and not gS[r1].any()
    Rr = R[r1].astype(np.float64)
    assert np.abs(np.einsum("nab,ncb->nac", Rr, Rr) - np.eye(3)).max() < 4 * rg.U
    Um, _, Vt = np.linalg.svd(S[r1].astype(np.float64))
    assert np.abs(np.einsum("nab,nb->na", Rr, Um[:, :, 0]) - Vt[:, 0, :]).max() < 8 * rg.U
    # rank 2: either float64 candidate; the gradient within the bound on the candidate chosen; det R = +1 where det S is exactly 0
    r2 = slice(42, 102)
    S2, R2 = S[r2], R[r2].astype(np.float64)
    Um, sig, Vt = np.linalg.svd(S2.astype(np.float64))
    base = np.einsum("nba,ncb->nac", Vt[:, :2, :], Um[:, :, :2])
    last = np.einsum("na,nc->nac", Vt[:, 2, :], Um[:, :, 2])
    sig[:, 2] = 0.0
    worst_R, worst_g = 0.0, 0.0
    for i in range(60):
        cands = [base[i] + last[i], base[i] - last[i]]
        errs = [np.abs(R2[i] - c).max() for c in cands]
        pick = int(np.argmin(errs))
        worst_R = max(worst_R, errs[pick] / rg.polar3_bound(sig[i:i + 1])[0])
        want = rg.polar3_bwd(S2[i], cands[pick], G[r2][i])[0]
        worst_g = max(worst_g, np.abs(gS[r2][i].astype(np.float64) - want).max() / rg.polar3_bwd_bound(sig[i:i + 1], G[r2][i])[0])
    print(f"  rank 2: R at {worst_R:.3f} of its bound, gS at {worst_g:.3f}")
    assert worst_R <= 1.0 and worst_g <= 1.0
    assert (np.linalg.det(R2[:40]) > 0).all()
    # non-finite rows: a non-finite R there and nowhere else
    nf = slice(102, 105)
    assert not np.isfinite(R[nf]).any()
    gen = slice(105, 135)
    R64, sg = rg.polar3(S[gen])
    assert np.isfinite(R[gen]).all() and np.isfinite(gS[gen]).all()
    assert frac("generic rows beside them: R", R[gen].reshape(30, -1), R64.reshape(30, -1), rg.polar3_bound(sg)[:, None]) <= 1.0
    assert frac("gS", gS[gen].reshape(30, -1), rg.polar3_bwd(S[gen], R64, G[gen]).reshape(30, -1), rg.polar3_bwd_bound(sg, G[gen])[:, None]) <= 1.0


def test_polar_rotation_is_once_differentiable():
    from trase_amd.losses import polar_rotation
    s = dev(rg.polar_cases()["random"][:8], True)
    R = polar_rotation(s)
    (gS,) = torch.autograd.grad(R.sum(), s, create_graph=True)
    with pytest.raises(RuntimeError):
        gS.sum().backward()


# ---- the fused kernels -----------------------------------------------------------------------------------------------------------
def raw_fit(x1, x2, graph, gcot):
    """trase_rigid_fit_forward / _backward into buffers with a 0xCD tail -> (r, R, g1, g2) numpy."""
    from trase_amd import _lib
    from trase_amd.rasterizer import _stream
    lib = _lib.load()
    N, k = graph.N, graph.k
    d = torch.device(DEV, torch.cuda.current_device())
    a, b, g = dev(x1.reshape(-1)), dev(x2.reshape(-1)), dev(gcot)
    W = _lib.RIGID_STATE_FLOATS
    out, R, st, g1, g2 = canary_buf(N), canary_buf(9 * N), canary_buf(W * N), canary_buf(3 * N), canary_buf(3 * N)
    _lib.check(lib.trase_rigid_fit_forward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(graph.idx), N, k, _lib.ptr(out), _lib.ptr(R), _lib.ptr(st),
                                           d.index, _stream(d)), "trase_rigid_fit_forward")
    _lib.check(lib.trase_rigid_fit_backward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(graph.idx), _lib.ptr(graph.rev_ranges),
                                            _lib.ptr(graph.rev_edges), _lib.ptr(R), _lib.ptr(st), _lib.ptr(g), N, k, _lib.ptr(g1),
                                            _lib.ptr(g2), d.index, _stream(d)), "trase_rigid_fit_backward")
    torch.cuda.synchronize()
    assert intact(out, N) and intact(R, 9 * N) and intact(st, W * N) and intact(g1, 3 * N) and intact(g2, 3 * N)
    return (out[:N].cpu().numpy(), R[:9 * N].cpu().numpy().reshape(N, 3, 3), g1[:3 * N].cpu().numpy().reshape(N, 3),
            g2[:3 * N].cpu().numpy().reshape(N, 3))


def check_open_rotations(R, fit):
    """What a degenerate row leaves open is only the completion: R is orthogonal and R u_1 = v_1 where sigma_1 > 0."""
    deg = fit["degenerate"]
    if not deg.any():
        return
    Rd = R[deg].astype(np.float64)
    assert np.abs(np.einsum("nab,ncb->nac", Rd, Rd) - np.eye(3)).max() < 4 * rg.U
    has = fit["sigma"][deg, 0] > 0
    moved = np.einsum("nab,nb->na", Rd, fit["U1"][deg]) - fit["V1"][deg]
    # u_1 and v_1 of the fp32 S are those of the exact one to the gap sigma_1: (k + 3) u-sized, beside R's own rounding
    assert not has.any() or np.abs(moved[has]).max() < 1e-4


def fit_check(tag, x1, x2, idx, seed):
    """rigid_fit on one graph: bits of two runs and of the C ABI, the two exact pins, value and gradients (fused and the autograd
    composition of the tested operators) against float64 -> the largest fraction of a bound."""
    from trase_amd.losses import polar_rotation, rigid_fit
    from trase_amd.neighbors import NeighborGraph, edge_moments, edge_residual
    N = len(x1)
    graph = NeighborGraph.from_idx(dev(idx))
    gcot = np.random.default_rng(seed).normal(size=N).astype(np.float32)
    raw = raw_fit(x1, x2, graph, gcot)
    for _ in range(2):
        a, b = dev(x1, True), dev(x2, True)
        r, R = rigid_fit(a, b, graph, return_rotation=True)
        assert not R.requires_grad
        r.backward(dev(gcot))
        got = (r.detach().cpu().numpy(), R.cpu().numpy(), a.grad.cpu().numpy(), b.grad.cpu().numpy())
        for x, y in zip(got, raw):
            assert x.tobytes() == y.tobytes()
    # the pins: the fused kernel IS the composition of the tested operators, bit for bit, in R and r
    a2, b2 = dev(x1, True), dev(x2, True)
    R2 = polar_rotation(edge_moments(a2, b2, graph))
    assert torch.equal(R, R2.detach())
    r2 = edge_residual(a2, b2, graph, R2)
    assert torch.equal(r.detach(), r2.detach())
    r2.backward(dev(gcot))
    comp = (a2.grad.cpu().numpy(), b2.grad.cpu().numpy())
    fit = rg.rigid_fit(x1, x2, idx, gcot, R_dev=got[1])
    print(f"rigid_fit, {tag}: {int(fit['degenerate'].sum())} degenerate rows, {int(fit['open_sign'].sum())} of rank 2")
    check_open_rotations(got[1], fit)
    worst = max(frac("r", got[0], fit["r"], fit["b_r"]),
                frac("gradient to p1", got[2], fit["g1"], fit["b1"]), frac("gradient to p2", got[3], fit["g2"], fit["b2"]),
                frac("composition, gradient to p1", comp[0], fit["g1"], fit["b1"]),
                frac("composition, gradient to p2", comp[1], fit["g2"], fit["b2"]))
    return worst, got, fit


@pytest.mark.parametrize("N,k", rg.FIT_PLAN)
def test_rigid_fit(N, k):
    kind, x1, x2, idx = rg.fit_case(N, k)
    worst, _, _ = fit_check(f"{kind} N {N} k {k}", x1, x2, idx, 100 * N + k)
    assert worst <= 1.0


def test_rigid_fit_near_isotropic():
    """Singular values closer than 1e-3 sigma_1 (down to 4e-6) on a third of the rows: no premise on them is needed."""
    x1, x2, idx = rg.near_isotropic_case()
    worst, _, _ = fit_check("near-isotropic lattice", x1, x2, idx, 5)
    assert worst <= 1.0


def test_rigid_fit_lattice_translation():
    """e1 = e2 on every edge, exactly: r = 0 and R = I exactly on the interior rows (S is diagonal there: no Jacobi step is taken),
    and everything within the derived bound, whose only terms left are those of an exactly rigid motion."""
    x1, x2, interior = rg.lattice_translation()
    idx = nr.knn_lex(x1.astype(np.float64), x1.astype(np.float64), 7)[1][:, 1:].astype(np.int32)
    worst, got, fit = fit_check("lattice under a translation", x1, x2, idx, 6)
    assert worst <= 1.0
    assert not got[0][interior].any() and np.array_equal(got[1][interior], np.stack([np.eye(3, dtype=np.float32)] * int(interior.sum())))
    print(f"  largest |r| {np.abs(got[0]).max():.3e}, largest |gradient| {max(np.abs(got[2]).max(), np.abs(got[3]).max()):.3e}")


def test_rigid_fit_checks():
    from trase_amd.losses import polar_rotation, rigid_fit
    from trase_amd.neighbors import NeighborGraph
    kind, x1, x2, idx = rg.fit_case(63, 4)
    graph = NeighborGraph.from_idx(dev(idx))
    with pytest.raises(RuntimeError, match="GPU only"):
        polar_rotation(torch.zeros(4, 3, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        rigid_fit(torch.from_numpy(x1), torch.from_numpy(x2), graph)
    with pytest.raises(ValueError):
        polar_rotation(torch.zeros(4, 9, device=DEV))
    with pytest.raises(ValueError):
        rigid_fit(dev(x1), dev(x2[:10]), graph)
    with pytest.raises(ValueError):
        rigid_fit(dev(x1[:10]), dev(x2[:10]), graph)
    with pytest.raises(TypeError):
        rigid_fit(dev(x1), dev(x2), dev(idx))
    assert rigid_fit(dev(x1), dev(x2), graph).shape == (63,)


# ---- the whole loss --------------------------------------------------------------------------------------------------------------
def loss_run(x1, x2, cid, k, **kw):
    from trase_amd.losses import loss_rigid_body_motion_reg_loss
    a, b = dev(x1, True), dev(x2, True)
    loss = loss_rigid_body_motion_reg_loss(a, b, dev(cid), num_neighbors=k, **kw)
    loss.backward()
    return loss.detach().cpu().numpy(), a.grad.cpu().numpy(), b.grad.cpu().numpy()


def graphs_of(x1, cid, k):
    from trase_amd.neighbors import NeighborGraph
    return [NeighborGraph.build(dev(x1[cid == c]), k).idx.cpu().numpy() for c in np.unique(cid)]


def polar_loss_check(x1, x2, cid, k, exact=False, fixture_fp32=None):
    """tests/test_gpu_neighbors.py's rigid_check for rotation="polar": no farther from float64 than max(4 x the fp32 torch
    composition's error on the same neighbours, the floor of rigid_floors)."""
    graphs = graphs_of(x1, cid, k)
    ref = nr.rigid_loss(x1, x2, cid, k, idx_of=lambda pos, p1: graphs[pos])
    got = loss_run(x1, x2, cid, k, rotation="polar")
    sides = [tgn.torch_composition(x1, x2, cid, graphs)] + ([fixture_fp32] if fixture_fp32 is not None else [])
    want = (ref["loss"], ref["g1"], ref["g2"])
    floors = list(tgn.rigid_floors(x1, x2, cid, k, graphs, exact))
    if exact:
        floors[0] = max(floors[0], (k + 3) * nr.U * ref["edge_scale"])
    worst = 0.0
    for i, name in enumerate(("loss", "gradient to xyz1", "gradient to xyz2")):
        measured = [float(np.abs(np.asarray(side[i], dtype=np.float64) - want[i]).max()) for side in sides]
        bar = max(4.0 * max(measured), floors[i])
        err = float(np.abs(np.asarray(got[i], dtype=np.float64) - want[i]).max())
        print(f"  {name}: polar {err:.3e}; fp32 compositions {', '.join(f'{m:.3e}' for m in measured)}; floor {floors[i]:.3e}; "
              f"bar {bar:.3e}; scale {float(np.abs(want[i]).max()):.3e}")
        worst = max(worst, err / max(bar, 1e-300))
    return worst


@pytest.mark.parametrize("name", tuple(tgn.RIGID_SCENES))
def test_rigid_loss_polar(name):
    x1, x2, cid, k, exact = tgn.rigid_scene(name)
    print(f"rigid loss, rotation polar, {name}")
    assert polar_loss_check(x1, x2, cid, k, exact=exact) <= 1.0


@pytest.mark.parametrize("name", ("rigid2", "rigid1"))
def test_rigid_loss_polar_fixture(name):
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "neighbors.npz"))
    x1, x2, cid = fx[f"{name}_xyz1"], fx[f"{name}_xyz2"], fx[f"{name}_cluster_ids"]
    print(f"rigid loss, rotation polar, fixture {name}")
    fixture = (float(fx[f"{name}_loss_f32"]), fx[f"{name}_g1_f32"], fx[f"{name}_g2_f32"])
    assert polar_loss_check(x1, x2, cid, 128, fixture_fp32=fixture) <= 1.0


def derived_loss_check(tag, x1, x2, cid, k):
    """The loss with rotation="polar" against rigid_reference's float64 loss within its derived bound alone."""
    from trase_amd.losses import rigid_fit
    from trase_amd.neighbors import NeighborGraph
    graphs = graphs_of(x1, cid, k)
    R_dev = [rigid_fit(dev(x1[cid == c]), dev(x2[cid == c]), NeighborGraph.from_idx(dev(graphs[pos])), return_rotation=True)[1].cpu().numpy()
             for pos, c in enumerate(np.unique(cid))]
    ref = rg.rigid_loss_polar(x1, x2, cid, graphs, R_dev=R_dev)
    got = loss_run(x1, x2, cid, k, rotation="polar")
    print(f"rigid loss, rotation polar, {tag}: loss {float(got[0]):.6e} (float64 {ref['loss']:.6e})")
    worst = max(frac("loss", got[0], ref["loss"], ref["b_loss"]), frac("gradient to xyz1", got[1], ref["g1"], ref["b1"]),
                frac("gradient to xyz2", got[2], ref["g2"], ref["b2"]))
    return worst, got, ref


def test_rigid_loss_polar_isotropic_cloud():
    g = np.random.default_rng(51)
    x1, x2 = rg.cloud("isotropic", 500, 52)
    cid = g.permutation(np.concatenate([np.full(200, 3), np.full(300, 8)])).astype(np.int64)
    worst, _, ref = derived_loss_check("isotropic cloud", x1, x2, cid, 16)
    assert not any(f["degenerate"].any() for f in ref["fits"])
    assert worst <= 1.0


def test_rigid_loss_polar_lattice_translation():
    x1, x2, interior = rg.lattice_translation()
    cid = np.zeros(len(x1), dtype=np.int64)
    worst, got, ref = derived_loss_check("lattice under a translation", x1, x2, cid, 6)
    assert ref["loss"] <= 1e-25 and worst <= 1.0
    print(f"  loss {float(got[0]):.3e}, largest |gradient| {max(np.abs(got[1]).max(), np.abs(got[2]).max()):.3e}")


def test_rigid_loss_polar_four_neighbour_gradients():
    """The gradients that test_rigid_loss_tiny_clusters of tests/test_gpu_neighbors.py leaves out: with 4 edges some rows have
    singular values too close for the SVD's autograd; the closed form needs no premise on them."""
    x1, x2, cid, _, _ = tgn.rigid_scene("deformation")
    worst, _, ref = derived_loss_check("three clusters, 4 neighbours", x1, x2, cid, 4)
    sig = np.concatenate([f["sigma"] for f in ref["fits"]])
    gap = np.minimum(sig[:, 0] - sig[:, 1], sig[:, 1] - sig[:, 2]) / sig[:, 0]
    print(f"  {int((gap < 1e-2).sum())} of {len(gap)} rows with singular values < 1e-2 sigma_1 apart")
    assert worst <= 1.0


def test_rigid_loss_polar_tiny_clusters():
    """As test_rigid_loss_tiny_clusters: a single point adds 0; a pair's rows have rank <= 1, are degenerate by the rule (no
    gradient through R) and add at most (1 + 4) / 2 (|d1| + |d2|)^2; everything stays finite."""
    x1, x2, cid, _, _ = tgn.rigid_scene("deformation")
    g = np.random.default_rng(8)
    t1, t2 = g.uniform(-1, 1, (3, 3)).astype(np.float32), g.uniform(-1, 1, (3, 3)).astype(np.float32)
    y1, y2, cid2 = np.concatenate([x1, t1]), np.concatenate([x2, t2]), np.concatenate([cid, [0, 20, 20]])
    base, more = loss_run(x1, x2, cid, 4, rotation="polar"), loss_run(y1, y2, cid2, 4, rotation="polar")
    extra = 5.0 * float(more[0]) - 3.0 * float(base[0])
    d1, d2 = np.linalg.norm(t1[1] - t1[2]), np.linalg.norm(t2[1] - t2[2])
    cap = 2.5 * (d1 + d2) ** 2
    print(f"tiny clusters add {extra:.6f} (at most {cap:.6f})")
    assert all(np.isfinite(m).all() for m in more)
    assert -64 * nr.U * abs(float(base[0])) <= extra <= cap * (1 + 64 * nr.U) + 64 * nr.U * abs(float(base[0]))
    n = len(x1)
    assert not more[1][n].any() and not more[2][n].any()                  # the single point
    # the pair: R is constant in the gradient, which is then that of edge_residual at the rotation rigid_fit chose
    from trase_amd.losses import rigid_fit
    from trase_amd.neighbors import NeighborGraph, edge_residual
    p1, p2 = dev(t1[1:], True), dev(t2[1:], True)
    graph = NeighborGraph.build(p1.detach(), 4)
    r, R = rigid_fit(p1, p2, graph, return_rotation=True)
    r.sum().backward()
    q1, q2 = dev(t1[1:], True), dev(t2[1:], True)
    edge_residual(q1, q2, graph, R).sum().backward()
    scale = float(max(q1.grad.abs().max(), q2.grad.abs().max()))
    assert float((p1.grad - q1.grad).abs().max()) <= 32 * nr.U * scale and float((p2.grad - q2.grad).abs().max()) <= 32 * nr.U * scale


def test_rigid_loss_polar_nan_cluster():
    """Deviation 29 with rotation="polar": the NaN cluster adds 0 and its rows get zero gradients; the other cluster's share is
    that of a run without it, halved."""
    g = np.random.default_rng(29)
    x1 = (g.uniform(-1, 1, (70, 3)) * np.array([1.0, 0.6, 0.3])).astype(np.float32)
    x2 = (x1 + 0.1 * g.normal(size=(70, 3))).astype(np.float32)
    cid = np.array([3] * 40 + [7] * 30, dtype=np.int64)
    x2[50, 1] = np.nan
    good = cid == 3
    alone, a1, a2 = loss_run(x1[good], x2[good], cid[good], 8, rotation="polar")
    both, g1, g2 = loss_run(x1, x2, cid, 8, rotation="polar")
    assert np.isfinite(alone) and alone > 0 and a1.any() and a2.any()
    assert both == np.float32(0.5) * alone
    assert not g1[~good].any() and not g2[~good].any()
    assert np.array_equal(g1[good], np.float32(0.5) * a1) and np.array_equal(g2[good], np.float32(0.5) * a2)


def test_rotation_svd_is_the_default_call():
    x1, x2, cid, k, _ = tgn.rigid_scene("few_neighbors")
    for x, y in zip(loss_run(x1, x2, cid, k), loss_run(x1, x2, cid, k, rotation="svd")):
        assert x.tobytes() == y.tobytes()
    with pytest.raises(ValueError, match="rotation must be"):
        loss_run(x1, x2, cid, k, rotation="qr")
