"""K-means, the query mask and the label sums at every shape trase_amd/csrc/segment.hip dispatches on: the four padded
widths, float4 and scalar row loads, 3 to 8 accumulating waves with tiles that end either side of a wave's sub-range, one
block to 256 blocks of more than one tile, the 16 runs of the reduction with some of them empty.

Most of it is exact.  One Lloyd step on small-integer rows (tests/segment_reference.py: ``lattice_step``, ``SHAPE_PLAN``) has
one right answer in fp32 whatever the order of the sums, so ids and centres are compared bit for bit, ties and re-seeded
empty clusters included; masks are compared bit for bit at a threshold no score is near.  What carries a bar: center_shift
(the bar of tests/test_gpu_segment.py), and the steps on real-valued rows, whose near-tie bar follows from the kernel's
arithmetic (``near_tie_gap``) with the share of rows it may set aside capped and counted without a GPU
(tests/test_segment_reference.py)."""
import numpy as np
import pytest
import torch

from tests import segment_reference as sr

pytestmark = pytest.mark.gpu

CENTRE_TOL = 2e-6       # tests/test_gpu_segment.py, for rows of norm 1
F16_ULP = 2.0 ** -11    # fp16 spacing in [0.5, 1)
KEY = 0x5EED5EED


def _dev():
    return torch.device("cuda", 0)


def _offset_copy(X):
    """The same rows, contiguous, starting 4 bytes into their storage: no row is 16-byte aligned."""
    buf = torch.empty(X.numel() + 1, dtype=X.dtype, device=X.device)
    view = buf[1:1 + X.numel()].view(X.shape)
    view.copy_(X)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _bits(t):
    return t.contiguous().view(torch.int32)


def _one_step(X, start, key=KEY):
    from trase_amd.segment import _kmeans_steps
    centres = start.clone()
    ids = torch.full((X.shape[0],), -7, dtype=torch.int32, device=X.device)
    state = torch.zeros(4, dtype=torch.int32, device=X.device)
    _kmeans_steps(X, centres, ids, key, 0.0, 0, 1, state)
    return ids, centres, state.cpu()


def _shift(state):
    return float(state[2:3].view(torch.float32)[0])


# ---- 1. one exact step at every shape of the plan -----------------------------------------------------------------------------

@pytest.mark.parametrize("case", sr.SHAPE_PLAN, ids=lambda c: c.id)
def test_one_step_is_exact_on_the_lattice(case):
    X_cpu, start_cpu = sr.lattice_case(case)
    r_ids, r_centres, r_empty, shift64 = sr.lattice_step(X_cpu, start_cpu, 0, KEY)
    X, start = X_cpu.to(_dev()), start_cpu.to(_dev())
    ids, centres, state = _one_step(X, start)
    assert torch.equal(ids.cpu().long(), r_ids), f"{int((ids.cpu().long() != r_ids).sum())} ids differ"
    wrong = (_bits(centres.cpu()) != _bits(r_centres)).any(1)
    assert not bool(wrong.any()), f"centres of clusters {torch.nonzero(wrong).flatten().tolist()[:8]} differ"
    for k in torch.nonzero(r_empty).flatten().tolist():
        assert torch.equal(centres[k], X[sr.reseed_row(KEY, 0, k, case.N)])
    assert not case.dup or bool(r_empty[case.K - 1])
    assert int(state[0]) == 1 and int(state[1]) == 0
    assert abs(_shift(state) - shift64) <= 1e-4 * shift64 + 1e-5, (_shift(state), shift64)
    runs = [_one_step(X, start)]                       # again from the same start, on a fresh state
    if case.offset:
        runs.append(_one_step(_offset_copy(X), start))
    for ids2, centres2, state2 in runs:
        assert torch.equal(ids2, ids) and torch.equal(_bits(centres2), _bits(centres)) and torch.equal(state2, state)


# ---- 2. query masks and label sums at the same corners ----------------------------------------------------------------------

# S, D, N.  (128, 64) accumulates in 3 waves; N = 512 is the one full tile, where the third wave's sub-range is cut short
MASK_CASES = [(1, 1, 255), (2, 3, 256), (127, 17, 257), (128, 32, 513), (1, 33, 513), (2, 64, 257), (127, 1, 256),
              (128, 64, 255), (128, 3, 257), (2, 17, 513), (1, 64, 256), (127, 33, 255), (128, 64, 513), (2, 32, 255),
              (128, 64, 512)]


def _mask_case(S, D, N):
    """-> rows, ids, sel on the CPU.  Ids run from -1 to S + 3, so some present ids are not selected; id 0 has exactly two
    members, x and -x (mean zero: NaN scores); two members of id 1 are zero rows; sel holds (room permitting) the zero-mean
    id, a duplicate and an id without members."""
    g = np.random.default_rng(1000 * S + 10 * D + N)
    ids = g.integers(-1, S + 4, N)
    # a direction per id plus noise of 0.2 to 1.7 times its length, then a scale per row: scores either side of any threshold
    rows = g.standard_normal((S + 5, D))[ids + 1]
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows += g.uniform(0.2, 1.7, (N, 1)) / np.sqrt(D) * g.standard_normal((N, D))
    rows = (rows * g.uniform(0.3, 3.0, (N, 1))).astype(np.float32)
    ids[ids == 0] = 1
    ids[[3, N - 2]] = 0
    rows[N - 2] = -rows[3]
    ids[[5, 6, N - 5, N - 4]] = 1
    rows[[5, N - 4]] = 0.0
    if S == 1:
        sel = [1]
    elif S == 2:
        sel = [[10_000, 1], [1, 1], [0, 1]][(D + N) % 3]
    else:
        sel = [0, 1, 1, 10_000] + list(range(2, S - 2))
    assert len(sel) == S and (ids == -1).any()
    return torch.from_numpy(rows), torch.from_numpy(ids), sel


def _free_threshold(score32):
    """The first fp16 value in [0.6, 0.95) that no score is within one fp16 ulp of."""
    s = score32[~torch.isnan(score32)].cpu()
    cands = [float(v) for v in np.arange(0.6, 0.95, F16_ULP).astype(np.float16)]
    return next(v for v in cands if not bool(((s - v).abs() <= F16_ULP).any()))


@pytest.mark.parametrize("S,D,N", MASK_CASES)
def test_segment_mask_bit_for_bit(S, D, N):
    from trase_amd.segment import segment_mask
    rows, ids, sel = _mask_case(S, D, N)
    _, s32 = sr.query_mask(rows, rows, ids, sel, 0.8)
    thr = _free_threshold(s32)
    ref, _ = sr.query_mask(rows, rows, ids, sel, thr)
    X, dev_ids = rows.to(_dev()), ids.to(_dev())
    keep = X.clone()
    mask = segment_mask(X, dev_ids, sel, thr)
    assert mask.dtype == torch.bool and torch.equal(mask.cpu(), ref), f"{int((mask.cpu() != ref).sum())} mask bits differ"
    chosen = torch.from_numpy(np.isin(ids.numpy(), [s for s in sel if s >= 0]))
    assert not bool(mask.cpu()[~chosen].any()) and not bool(mask.cpu()[ids == 0].any())
    assert not bool(mask.cpu()[(rows == 0).all(1)].any())
    assert 0 < int(ref.sum()) < int(chosen.sum()) and torch.equal(X, keep)
    assert torch.equal(segment_mask(X, dev_ids, sel, thr), mask)
    if D % 4 == 0:
        assert torch.equal(segment_mask(_offset_copy(X), dev_ids, sel, thr), mask)


@pytest.mark.parametrize("D,C,N", [(64, 128, 512), (64, 129, 1025), (3, 2, 513)])
def test_label_centres_on_the_lattice(D, C, N):
    """One pass of 128 labels at D = 64 (3 accumulating waves, one full tile), a second pass of one label, and two labels
    at D = 3."""
    from trase_amd.segment import label_centres
    X = sr.lattice_rows(N, D, seed=C)
    lab = torch.from_numpy(np.random.default_rng(C).integers(-1, C, N))
    got = label_centres(X.to(_dev()), lab.to(_dev()), C).cpu().double()
    members = lab >= 0
    sums = torch.zeros(C, D, dtype=torch.float64).index_add_(0, lab[members], X.double()[members])
    counts = torch.bincount(lab[members], minlength=C)
    assert bool((lab == -1).any()) and int(counts.min()) > 0
    mean = sums / counts[:, None]
    norm = mean.norm(dim=1, keepdim=True)
    assert float(norm.min()) > 0.05
    assert float((got - mean / norm).abs().max()) <= 2e-6


# ---- 3. six steps in lockstep with float64 away from D = 32 -----------------------------------------------------------------

@pytest.mark.parametrize("K,D,unit", sr.LOCKSTEP_CASES)
def test_lloyd_steps_lockstep_with_float64(K, D, unit):
    from trase_amd.segment import _kmeans_steps
    X_cpu, start = sr.lockstep_rows(K, D, unit)
    N, tol, key = sr.LOCKSTEP_N, 1e-4, 12345
    gap_bar = sr.near_tie_gap(X_cpu)
    M = float(X_cpu.double().norm(dim=-1).max())
    X = X_cpu.to(_dev())
    centres = X[torch.as_tensor(start, device=X.device)].contiguous()
    ids = torch.zeros(N, dtype=torch.int32, device=X.device)
    state = torch.zeros(4, dtype=torch.int32, device=X.device)
    for it in range(sr.LOCKSTEP_ITERS):
        before = centres.clone()
        _kmeans_steps(X, centres, ids, key, tol, 0, 1, state)
        st = state.cpu()
        assert int(st[0]) == it + 1
        o_ids, gap, _, _ = sr.lloyd_step(X, before, it, key)
        g_ids = ids.long()
        differ = g_ids != o_ids
        near = gap < gap_bar
        print(f"K={K} D={D} it={it}: {int(differ.sum())} ids differ, {int(near.sum())} rows under the gap bar {gap_bar:.2e}")
        assert not bool((differ & ~near).any()), f"it={it}: {int((differ & ~near).sum())} ids differ away from a tie"
        assert int(near.sum()) <= sr.near_tie_cap(N)
        c64, shift64 = sr.update(X, g_ids, before, it, key)
        err = float((centres.double() - c64).abs().max())
        assert err < CENTRE_TOL * M, f"it={it}: centres differ from float64 means of the GPU's ids by {err:.3e}"
        shift = _shift(st)
        assert abs(shift - shift64) <= 1e-4 * shift64 + 1e-5, (it, shift, shift64)
        if abs(shift64 ** 2 - tol) > 1e-2 * tol:
            assert bool(st[1]) == (shift64 ** 2 < tol), (it, shift64)
        state[1] = 0                        # keep stepping past convergence: the lockstep covers all six iterations


# ---- 4. the public kmeans() at odd inputs -----------------------------------------------------------------------------------

def _distinct_lattice_rows(n, d, seed):
    rows = torch.unique(sr.lattice_rows(4 * n, d, seed), dim=0)
    return rows[torch.randperm(rows.shape[0], generator=torch.Generator().manual_seed(seed))[:n]].contiguous()


@pytest.mark.parametrize("N,D", [(1, 3), (128, 17), (128, 64)])
def test_kmeans_with_every_row_its_own_centre(N, D):
    from trase_amd.segment import kmeans
    X = _distinct_lattice_rows(N, D, seed=N + D).to(_dev())
    assert X.shape[0] == N
    ids, centres, iters = kmeans(X, N, seed=5)
    start = torch.as_tensor(sr.init_indices(N, N, 5), device=X.device)
    assert iters == 1 and torch.equal(centres, X[start])
    assert torch.equal(ids[start], torch.arange(N, device=X.device))          # ids: the inverse of the start permutation


def test_kmeans_with_as_many_clusters_as_rows_and_a_repeated_row():
    """Two equal rows leave the higher of their two clusters empty: the re-seed through the public call, step for step
    the float64 loop (means of equal integer rows are exact)."""
    from trase_amd.segment import kmeans
    N, D, seed, limit = 16, 9, 4, 12
    X = _distinct_lattice_rows(N, D, seed=1)
    X[11] = X[2]
    start = sr.init_indices(N, N, seed)
    o_ids, o_c, o_iters = sr.kmeans_loop(X, start, key=seed, iter_limit=limit)
    assert o_iters > 1                                  # the first step moved the re-seeded centre
    ids, centres, iters = kmeans(X.to(_dev()), N, seed=seed, iter_limit=limit)
    assert iters == o_iters and torch.equal(ids.cpu(), o_ids) and torch.equal(centres.cpu().double(), o_c)


def test_kmeans_with_one_cluster():
    from trase_amd.segment import kmeans
    N, D = 1000, 7
    X = sr.lattice_rows(N, D, seed=8)
    ids, centres, iters = kmeans(X.to(_dev()), 1, seed=2)
    assert iters == 2 and not bool(ids.any()) and ids.dtype == torch.int64
    mean = torch.from_numpy(X.double().sum(0).numpy().astype(np.float32) / np.float32(N))
    assert torch.equal(_bits(centres.cpu()), _bits(mean[None]))


@pytest.mark.parametrize("K,D,noise,seed", sr.BLOB_CASES)
def test_kmeans_on_separated_blobs(K, D, noise, seed):
    from trase_amd.segment import kmeans
    X, labels, start = sr.blob_rows(sr.BLOB_N, K, D, noise, seed)
    ids, centres, iters = kmeans(X.to(_dev()), K, seed=seed)
    o_ids, o_c, o_iters = sr.kmeans_loop(X, start, key=seed)
    assert torch.equal(ids.cpu(), o_ids) and iters == o_iters
    M = float(X.double().norm(dim=-1).max())
    assert float((centres.cpu().double() - o_c).abs().max()) < CENTRE_TOL * M
    assert len(set(zip(labels.tolist(), ids.tolist()))) == K


def test_kmeans_input_forms_give_the_same_bits():
    from trase_amd.segment import kmeans
    N, D, K = 3000, 12, 9
    wide = torch.nn.functional.normalize(torch.randn(N, D + 5, generator=torch.Generator().manual_seed(6)), dim=-1).to(_dev())
    X = wide[:, 2:2 + D].contiguous()
    want = kmeans(X, K, seed=3, iter_limit=10)
    assert want[2] > 1
    column_slice = wide[:, 2:2 + D]
    assert not column_slice.is_contiguous()
    for form in (column_slice, X.double(), _offset_copy(X)):
        ids, centres, iters = kmeans(form, K, seed=3, iter_limit=10)
        assert torch.equal(ids, want[0]) and torch.equal(_bits(centres), _bits(want[1])) and iters == want[2]
        assert centres.dtype == torch.float32


def test_kmeans_batching_gives_the_same_bits_at_d17(monkeypatch):
    from trase_amd import segment
    X = torch.nn.functional.normalize(torch.randn(4000, 17, generator=torch.Generator().manual_seed(9)), dim=-1).to(_dev())
    runs = []
    for batch in (8, 1):
        monkeypatch.setattr(segment, "_BATCH", batch)
        runs.append(segment.kmeans(X, 6, seed=11, iter_limit=25))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1])) and runs[0][2] == runs[1][2]
    assert 1 < runs[0][2] <= 25
