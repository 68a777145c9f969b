"""The rotation of the rigid-motion loss without a GPU: tests/rigid_reference.py against scipy, torch's float64 SVD autograd and
central differences; trase_amd/csrc/rigid_math.h compiled for the host against float64 within the bounds of rigid_reference's
docstring (u + C_R cond per entry of R, C_G (1 + cond) |G|_F / s per entry of gS; C_R = 1024 * 2^-53, C_G = 256 u), its policy on
degenerate input; the premises of the scenes of tests/test_gpu_rigid.py counted in float64; every refusal of the entry points."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import neighbors_reference as nr
from tests import rigid_reference as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the float64 statements ----------------------------------------------------------------------------------------------------
def test_polar3_is_the_polar_factor_of_the_transpose():
    import scipy.linalg
    for name, S in rg.polar_cases().items():
        R, sig = rg.polar3(S)
        for i in range(0, len(S), 7):
            want = scipy.linalg.polar(S[i].astype(np.float64).T)[0]
            assert np.abs(R[i] - want).max() <= 1e-9 * sig[i, 0] / (sig[i, 1] + sig[i, 2]), name
        assert np.abs(np.einsum("nab,ncb->nac", R, R) - np.eye(3)).max() < 1e-12
        assert np.array_equal(np.sign(np.linalg.det(R)), np.sign(np.linalg.det(S.astype(np.float64)))), name


def svd_autograd(S, G):
    St = torch.tensor(S, dtype=torch.float64, requires_grad=True)
    Um, _, V = torch.svd(St)
    R = torch.bmm(V, Um.transpose(1, 2))
    R.backward(torch.tensor(G, dtype=torch.float64))
    return R.detach().numpy(), St.grad.numpy()


def test_closed_form_equals_the_svd_autograd_in_float64():
    g = np.random.default_rng(12)
    S = np.concatenate([rg.matrices_with_sigma(np.sort(g.uniform(0.2, 2.0, (200, 3)), axis=1)[:, ::-1], 200, 8),
                        rg.matrices_with_sigma((1.0, 0.6, 0.3), 50, 9, reflect=True), rg.matrices_with_sigma((1.0, 0.6, 0.3), 50, 10, reflect=False)])
    sig = np.linalg.svd(S, compute_uv=False)
    keep = np.minimum(sig[:, 0] - sig[:, 1], sig[:, 1] - sig[:, 2]) >= 1e-2 * sig[:, 0]
    S, sig = S[keep], sig[keep]
    det = np.linalg.det(S)
    assert (det < 0).sum() >= 50 and (det > 0).sum() >= 50 and len(S) >= 150
    G = g.normal(size=S.shape)
    R, want = svd_autograd(S, G)
    assert np.abs(R - rg.polar3(S)[0]).max() < 1e-13
    got = rg.polar3_bwd(S, R, G)
    rel = np.abs(got - want).max((1, 2)) / np.abs(want).max((1, 2))
    print(f"closed form against float64 SVD autograd: {rel.max():.2e} relative, {len(S)} matrices, {(det < 0).sum()} reflections")
    assert rel.max() <= 1e-12


@pytest.mark.parametrize("sig", ((1.0, 1.0 + 1e-5, 0.7), (0.9, 0.9, 0.9)))
def test_closed_form_against_central_differences(sig):
    g = np.random.default_rng(13)
    S = rg.matrices_with_sigma(sig, 6, 14)
    G = g.normal(size=S.shape)
    got = rg.polar3_bwd(S, rg.polar3(S)[0], G)
    h = 1e-6
    num = np.zeros_like(S)
    for a in range(3):
        for b in range(3):
            d = np.zeros((1, 3, 3))
            d[0, a, b] = h
            num[:, a, b] = ((rg.polar3(S + d)[0] - rg.polar3(S - d)[0]) * G).sum((1, 2)) / (2 * h)
    err = np.abs(got - num).max() / np.abs(num).max()
    print(f"sigma {sig}: closed form {err:.2e} relative from central differences")
    assert err <= 1e-8          # the differences' own truncation and rounding: h^2 |R'''| + 2^-53 / h


# ---- the host build ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    out = os.path.join(tempfile.gettempdir(), f"libtrase_rigid_hostsim_{os.getpid()}.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "hostsim", "rigid_hostsim.cpp")])
    lib = C.CDLL(out)
    lib.hs_polar3.restype = None
    lib.hs_polar3_bwd.restype = None
    lib.hs_polar3_is_degenerate.restype = C.c_int
    lib.hs_polar3_is_degenerate.argtypes = [C.c_double, C.c_double, C.c_double]
    return lib


def host_polar3(lib, S):
    S = np.ascontiguousarray(S, dtype=np.float32).reshape(-1, 3, 3)
    n = len(S)
    R, s23, deg = np.full((n, 3, 3), 7.0, dtype=np.float32), np.zeros(n), np.zeros(n, dtype=np.int32)
    lib.hs_polar3(S.ctypes.data_as(C.c_void_p), C.c_int(n), R.ctypes.data_as(C.c_void_p), s23.ctypes.data_as(C.c_void_p),
                  deg.ctypes.data_as(C.c_void_p))
    return R, s23, deg.astype(bool)


def host_polar3_bwd(lib, S, R, G):
    S, R, G = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3, 3) for a in (S, R, G))
    gS = np.full(S.shape, 7.0, dtype=np.float32)
    lib.hs_polar3_bwd(S.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), G.ctypes.data_as(C.c_void_p), C.c_int(len(S)),
                      gS.ctypes.data_as(C.c_void_p))
    return gS


def check_operator(tag, S, R, gS, G, deg):
    """R and gS of fp32 matrices S against float64 within the two bounds -> the largest fractions of them."""
    R64, sig = rg.polar3(S)
    assert not deg.any(), f"{tag}: a generic matrix counts as degenerate"
    fr = (np.abs(R.astype(np.float64) - R64).max((1, 2)) / rg.polar3_bound(sig)).max()
    want = rg.polar3_bwd(S, R64, G)
    fg = (np.abs(gS.astype(np.float64) - want).max((1, 2)) / rg.polar3_bwd_bound(sig, G)).max()
    print(f"  {tag}: R at {fr:.3f} of its bound, gS at {fg:.3f}; cond up to {rg.cond_of(sig)[1].max():.2e}")
    return fr, fg


def test_host_build_lies_inside_the_bounds(sim):
    g = np.random.default_rng(21)
    seen_neg = 0
    for name, S in rg.polar_cases().items():
        G = g.normal(size=S.shape).astype(np.float32)
        R, s23, deg = host_polar3(sim, S)
        gS = host_polar3_bwd(sim, S, R, G)
        sig = np.linalg.svd(S.astype(np.float64), compute_uv=False)
        assert np.abs(s23 - (sig[:, 1] + sig[:, 2])).max() <= 1e-12 * sig[:, 0].max()
        det = np.linalg.det(S.astype(np.float64))
        assert np.array_equal(np.sign(np.linalg.det(R.astype(np.float64))), np.sign(det)), name
        seen_neg += int((det < 0).sum())
        fr, fg = check_operator(name, S, R, gS, G, deg)
        assert fr <= 1.0 and fg <= 1.0, name
    assert seen_neg >= 100
    assert (np.linalg.det(rg.polar_cases()["reflections"].astype(np.float64)) < 0).all()


def test_host_build_on_degenerate_input(sim):
    g = np.random.default_rng(22)
    a, b = g.normal(size=(40, 3)), g.normal(size=(40, 3))
    rank1 = np.einsum("na,nb->nab", a, b).astype(np.float32)
    S = np.concatenate([np.zeros((1, 3, 3), dtype=np.float32), rank1])
    G = g.normal(size=S.shape).astype(np.float32)
    R, s23, deg = host_polar3(sim, S)
    gS = host_polar3_bwd(sim, S, R, G)
    assert deg.all() and not gS.any()                                           # rank <= 1: a zero gradient
    assert np.array_equal(R[0], np.eye(3, dtype=np.float32))
    assert np.abs(np.einsum("nab,ncb->nac", R.astype(np.float64), R.astype(np.float64)) - np.eye(3)).max() < 4 * rg.U
    # ... and what is determined is right: R^T u_1 = v_1, i.e. R S^T = (S S^T)^(1/2) = |b| a a^T / |a|
    S64 = rank1.astype(np.float64)
    Um, sig, Vt = np.linalg.svd(S64)
    assert np.abs(np.einsum("nab,nb->na", R[1:].astype(np.float64), Um[:, :, 0]) - Vt[:, 0, :]).max() < 8 * rg.U
    # rank 2: one of the two float64 candidates, and on that candidate the gradient within its bound
    S2 = rg.matrices_with_sigma((1.0, 0.5, 0.0), 60, 23)
    S2[:20, :, 2] = 0.0                                                          # an exactly zero column: det evaluates to 0
    S2[20:40, 2, :] = 0.0
    S2 = S2.astype(np.float32)
    G2 = g.normal(size=S2.shape).astype(np.float32)
    R2, _, deg2 = host_polar3(sim, S2)
    g2 = host_polar3_bwd(sim, S2, R2, G2)
    assert not deg2.any()
    Um, sig, Vt = np.linalg.svd(S2.astype(np.float64))
    base = np.einsum("nba,ncb->nac", Vt[:, :2, :], Um[:, :, :2])
    last = np.einsum("na,nc->nac", Vt[:, 2, :], Um[:, :, 2])
    sig[:, 2] = 0.0
    worst = 0.0
    for i in range(len(S2)):
        cands = [base[i] + last[i], base[i] - last[i]]
        errs = [np.abs(R2[i].astype(np.float64) - c).max() for c in cands]
        pick = int(np.argmin(errs))
        assert errs[pick] <= rg.polar3_bound(sig[i:i + 1])[0], (i, errs)
        want = rg.polar3_bwd(S2[i], cands[pick], G2[i])[0]
        worst = max(worst, np.abs(g2[i].astype(np.float64) - want).max() / rg.polar3_bwd_bound(sig[i:i + 1], G2[i])[0])
    print(f"  rank 2: gS at {worst:.3f} of its bound on the chosen candidate")
    assert worst <= 1.0
    exact = np.linalg.det(R2[:40].astype(np.float64))
    assert (exact > 0).all()                                                     # det S evaluates to exactly 0: det R = +1
    # non-finite input leaves the loop and gives a non-finite R
    for bad in (np.nan, np.inf, -np.inf):
        Sn = g.normal(size=(3, 3, 3)).astype(np.float32)
        Sn[1, 1, 2] = bad
        Rn, _, _ = host_polar3(sim, Sn)
        assert np.isfinite(Rn[0]).all() and np.isfinite(Rn[2]).all() and not np.isfinite(Rn[1]).any()
        host_polar3_bwd(sim, Sn, Rn, g.normal(size=(3, 3, 3)).astype(np.float32))     # terminates
    # extreme magnitudes neither overflow nor underflow in the float64 body
    Sx = np.stack([np.full((3, 3), 3e38), np.eye(3) * 1e-45, np.diag([3e38, 1e-45, 1.0])]).astype(np.float32)
    Rx, _, _ = host_polar3(sim, Sx)
    assert np.isfinite(Rx).all()
    assert np.abs(np.einsum("nab,ncb->nac", Rx.astype(np.float64), Rx.astype(np.float64)) - np.eye(3)).max() < 4 * rg.U


def test_degenerate_rule_of_the_host_build_is_the_reference_rule(sim):
    g = np.random.default_rng(24)
    for _ in range(200):
        s23, k, m = 10.0 ** g.uniform(-9, 0), float(g.integers(1, 257)), 10.0 ** g.uniform(-3, 3)
        assert bool(sim.hs_polar3_is_degenerate(s23, k, m)) == bool(rg.degenerate(s23, k, m))
    assert not sim.hs_polar3_is_degenerate(float("nan"), 4.0, 1.0)


# ---- the premises of the GPU scenes, in float64 --------------------------------------------------------------------------------
def test_premises_of_the_gradient_scenes():
    names, saw_reflection = [], False
    for name, x1, x2, idx in rg.gradient_scenes():
        fit = rg.rigid_fit(x1, x2, idx)
        live = ~fit["degenerate"]
        share = max(float((np.abs(fit["z1"]) / fit["b1"]).max()), float((np.abs(fit["z2"]) / fit["b2"]).max()))
        print(f"  {name}: through-R share up to {share:.0f} x the bound; {int(fit['degenerate'].sum())} degenerate rows; "
              f"margins {fit['margin'][live].min():.1e} / {fit['margin'][~live].max() if (~live).any() else 0:.1e}")
        assert min(float((np.abs(fit["z1"]) / fit["b1"]).max()), float((np.abs(fit["z2"]) / fit["b2"]).max())) >= 100.0, name
        saw_reflection |= name.startswith("reflection") and bool((np.linalg.det(fit["S"]) < 0).any())
        names.append(name)
    assert saw_reflection and len(names) >= 10


def test_premises_of_every_fit_case():
    """No row sits near the degenerate threshold (the device decides nothing the float64 count could decide otherwise), and a
    degenerate row is one whose valid edges are all the same edge (an edge to the row itself is the zero edge)."""
    cases = [(f"N{N}-k{k}",) + rg.fit_case(N, k)[1:] for N, k in rg.FIT_PLAN] + [("near_isotropic",) + rg.near_isotropic_case()]
    x1, x2, _ = rg.lattice_translation()
    cases.append(("lattice", x1, x2, nr.knn_lex(x1.astype(np.float64), x1.astype(np.float64), 7)[1][:, 1:].astype(np.int32)))
    for name, x1, x2, idx in cases:
        fit = rg.rigid_fit(x1, x2, idx)
        deg = fit["degenerate"]
        assert (fit["margin"][~deg] >= 4.0).all() and (fit["margin"][deg] <= 0.25).all(), name
        N = len(x1)
        for i in np.nonzero(deg)[0]:
            row = idx[i].astype(np.int64)
            assert len(set(row[(row >= 0) & (row < N) & (row != i)].tolist())) <= 1, (name, i)
        if name in ("near_isotropic", "lattice"):
            assert not deg.any()
    # generic scenes without holes have no degenerate row at all
    for N, k in rg.FIT_PLAN:
        pos = rg.FIT_PLAN.index((N, k))
        if pos % 3 != 1 and 3 <= k < N - 1:
            kind, x1, x2, idx = rg.fit_case(N, k)
            assert not rg.rigid_fit(x1, x2, idx)["degenerate"].any(), (N, k)


def test_premises_of_the_special_scenes():
    x1, x2, idx = rg.near_isotropic_case()
    sig = rg.rigid_fit(x1, x2, idx)["sigma"]
    gap = np.minimum(sig[:, 0] - sig[:, 1], sig[:, 1] - sig[:, 2]) / sig[:, 0]
    print(f"  near-isotropic: {(gap < 1e-3).sum()} of {len(gap)} rows with singular values < 1e-3 sigma_1 apart, closest {gap.min():.1e}")
    assert (gap < 1e-3).sum() >= 50
    kind, x1, x2, idx = rg.fit_case(1025, 16)
    assert kind == "reflection" and (np.linalg.det(rg.rigid_fit(x1, x2, idx)["S"]) < 0).sum() >= 500
    x1, x2, interior = rg.lattice_translation()
    idx = nr.knn_lex(x1.astype(np.float64), x1.astype(np.float64), 7)[1][:, 1:]
    fit = rg.rigid_fit(x1, x2, idx)
    assert interior.sum() >= 27 and np.array_equal((x2.astype(np.float64) - x1)[0], [0.5, -0.25, 0.125])
    assert float(np.abs(fit["r"]).max()) <= 1e-25 and float(np.abs(fit["g1"]).max()) <= 1e-12


def test_reference_gradient_is_the_float64_autograd_of_the_whole_fit():
    kind, x1, x2, idx = rg.fit_case(255, 4)
    gcot = np.random.default_rng(31).normal(size=len(x1))
    fit = rg.rigid_fit(x1, x2, idx, gcot)
    a = torch.tensor(x1.astype(np.float64), requires_grad=True)
    b = torch.tensor(x2.astype(np.float64), requires_grad=True)
    j = torch.from_numpy(idx.astype(np.int64))
    e1, e2 = a[:, None] - a[j], b[:, None] - b[j]
    S = torch.bmm(e1.transpose(1, 2), e2)
    Um, _, V = torch.svd(S)
    Rm = torch.bmm(V, Um.transpose(1, 2))
    r = (e1 - torch.bmm(Rm, e2.transpose(1, 2)).transpose(1, 2)).pow(2).sum((1, 2))
    r.backward(torch.from_numpy(gcot))
    assert np.abs(fit["r"] - r.detach().numpy()).max() <= 1e-12 * np.abs(fit["r"]).max()
    for got, want in ((fit["g1"], a.grad.numpy()), (fit["g2"], b.grad.numpy())):
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_touching_a_device():
    from trase_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p).value
    INVALID = lib.trase_polar3_forward(None, 1, p, 0, None)
    assert INVALID != 0
    calls = []
    # polar3
    calls += [lambda: lib.trase_polar3_forward(p, -1, p, 0, None), lambda: lib.trase_polar3_forward(p, 1, None, 0, None),
              lambda: lib.trase_polar3_backward(p, p, p, -1, p, 0, None)]
    for hole in range(4):
        a = [p, p, p, p]
        a[hole] = None
        calls.append(lambda a=a: lib.trase_polar3_backward(a[0], a[1], a[2], 1, a[3], 0, None))
    # rigid_fit forward: p1, p2, idx, N, k, out, R, state
    for N, k in ((-1, 4), (4, 0), (4, -3), (2 ** 20, 2 ** 11)):
        calls.append(lambda N=N, k=k: lib.trase_rigid_fit_forward(p, p, p, N, k, p, p, p, 0, None))
        calls.append(lambda N=N, k=k: lib.trase_rigid_fit_backward(p, p, p, p, p, p, p, p, N, k, p, p, 0, None))
    for hole in range(6):
        a = [p] * 6
        a[hole] = None
        calls.append(lambda a=a: lib.trase_rigid_fit_forward(a[0], a[1], a[2], 1, 1, a[3], a[4], a[5], 0, None))
    for hole in range(10):
        a = [p] * 10
        a[hole] = None
        calls.append(lambda a=a: lib.trase_rigid_fit_backward(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], 1, 1, a[8], a[9], 0, None))
    for call in calls:
        assert call() == INVALID
        assert lib.trase_last_error()
    # nothing to do is not an error, whatever the pointers
    assert lib.trase_polar3_forward(None, 0, None, 0, None) == 0 and lib.trase_polar3_backward(None, None, None, 0, None, 0, None) == 0
    assert lib.trase_rigid_fit_forward(None, None, None, 0, 3, None, None, None, 0, None) == 0
    assert not buf.any()


def test_python_checks():
    from trase_amd.losses import loss_rigid_body_motion_reg_loss, polar_rotation, rigid_fit
    from trase_amd.neighbors import NeighborGraph
    x = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="rotation must be"):
        loss_rigid_body_motion_reg_loss(x, x, torch.zeros(5, dtype=torch.int64), rotation="jacobi")
    with pytest.raises(RuntimeError, match="GPU only"):
        polar_rotation(torch.zeros(4, 3, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        rigid_fit(x, x, NeighborGraph(None, None, None))
