"""HDBSCAN on the GPU (trase_amd/csrc/hdbscan.hip) EXACTLY, at every dispatch shape, against tests/hdbscan_exact_reference.py.

On lattice rows (multiples of 1/4 in [-8, 8) or of 1/64 in [-4, 4); ``assert_exact`` checks the premise for every cloud) every
difference, square and partial sum of the kernel's fmaf chain is an fp32 number, so the squared core distances must equal
integer arithmetic, and under the key (weight bits << 32 | min(i, j) << 16 | max(i, j)) the minimum spanning tree is unique:
the device's n - 1 keys have one right answer.  ``np.array_equal`` and ``torch.equal`` only; the one inequality is the 2e-6 bar
of the label centres, taken from tests/test_gpu_hdbscan.py.

What the plan runs that tests/test_gpu_hdbscan.py does not: hd_core_kernel<16, 16>, <16, 64> and <32, 64> and
hd_min_edge_kernel<16> (D 9, 12, 16; k 17, 63, 64 at every row width, checked on every row); k = 1, 16 | 17 and 64 with n = 65;
chunk 64 with 1 to 16 live column ranges of 16 (n <= 1024), chunk 128 with a last range of one row (n 1025), S = 15 (n 16385);
hd_load_row's scalar path for a base that is not 16-byte aligned while D % 4 == 0."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import hdbscan_exact_reference as hx

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 256
CANARY = 0xCD


@functools.lru_cache(maxsize=None)
def reference(n, D, k, grid, kind):
    """-> (Q, X, squared core distances in units, sorted keys, step): computed once per cloud, shared, read-only."""
    Q, X = hx.lattice_points(kind, n, D, grid, hx.case_seed(n, D, k))
    hx.assert_exact(Q)                                   # the premise: every squared distance is exact in fp32
    step = hx.GRIDS[grid][0]
    core = hx.core2_units(Q, k)
    keys = hx.mst_keys(Q, core, step)
    for a in (Q, X, core, keys):
        a.setflags(write=False)
    return Q, X, core, keys, step


def on_device(X, offset=0):
    """X as a contiguous fp32 (n, D) tensor that starts `offset` floats behind a 16-byte boundary."""
    n, D = X.shape
    buf = torch.zeros(n * D + 4, dtype=torch.float32, device=DEV)
    t = buf[offset:offset + n * D].view(n, D)
    t.copy_(torch.from_numpy(np.array(X, dtype=np.float32, order="C")))          # a copy: the shared reference is read-only
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * offset
    return t


def run(X, k, offset=0):
    from trase_amd.segment import hdbscan
    t = on_device(X, offset)
    keep = t.clone()
    labels, edges, core = hdbscan(t, min_cluster_size=max(k, 2), min_samples=k, return_mst=True)
    assert torch.equal(t, keep)
    assert labels.dtype == torch.int64 and edges.dtype == torch.float64 and core.dtype == torch.float64
    return labels.cpu().numpy(), edges.cpu().numpy(), core.cpu().numpy()


def check_against_reference(got, n, k, core_units, keys, step):
    from trase_amd.segment import hdbscan_hierarchy
    labels, edges, core = got
    want_core = np.sqrt(hx.units_to_f32(core_units, step).astype(np.float64))
    assert np.array_equal(core, want_core), f"core distances: {int((core != want_core).sum())} of {n} rows differ"
    want_edges = hx.decode_keys(keys)
    assert edges.shape == (n - 1, 3)
    assert np.array_equal(edges, want_edges), f"edges: {int((edges != want_edges).any(1).sum())} of {n - 1} differ"
    with np.errstate(all="ignore"):                      # zero weights: infinite lambdas, as in the wrapper's own run
        want_labels = hdbscan_hierarchy(want_edges, n, min_cluster_size=max(k, 2))
    assert np.array_equal(labels, want_labels)


def _id(c):
    return f"n{c[0]}-D{c[1]}-k{c[2]}-{c[3]}-{c[4]}" + ("-off1" if c[5] else "")


@pytest.mark.parametrize("case", [c for c in hx.exact_plan() if c[0] != hx.N_SPLIT15], ids=_id)
def test_core_distances_tree_and_labels_are_exact(case):
    n, D, k, grid, kind, offset = case
    Q, X, core_units, keys, step = reference(n, D, k, grid, kind)
    first = run(X, k, offset)
    second = run(X, k, offset)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    check_against_reference(first, n, k, core_units, keys, step)
    if kind == "coincident" and k == 1:
        # zero core distances for every row that has a twin (an odd n leaves one without), zero weights
        assert (first[2] == 0).sum() >= n - n % 2 and (first[1][:, 2] == 0).sum() >= n // 2
    if offset:                                           # the scalar row loads against the vector ones
        for a, b in zip(first, run(X, k, 0)):
            assert a.tobytes() == b.tobytes()


def test_fifteen_column_ranges():
    """n = 16385: 65 row blocks, so hd_splits gives 1024 / 65 = 15 ranges of 1152 columns, the last one of 257.  The one case
    beyond 4000 rows; the reference is nearly all of its time: 2.6 s for the core distances and 4.0 s for Prim's 16384 steps
    on a slow CPU when this was written, and the whole test 2.7 s on the machine with the MI355X."""
    n, D, k, grid, kind, offset = [c for c in hx.exact_plan() if c[0] == hx.N_SPLIT15][0]
    Q, X, core_units, keys, step = reference(n, D, k, grid, kind)
    first, second = run(X, k, offset), run(X, k, offset)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    check_against_reference(first, n, k, core_units, keys, step)


# ---- the C entry points, every output and the workspace in front of a canary ---------------------------------------------
def _guarded(nbytes):
    """a byte buffer of nbytes + PAD, all 0xCD"""
    return torch.full((nbytes + PAD,), CANARY, dtype=torch.uint8, device=DEV)


def _intact(buf, nbytes):
    return bool((buf[nbytes:] == CANARY).all())


def abi_run(X, k, core2=None):
    """trase_hdbscan_core (unless the caller brings squared core distances, fp32 (n,)) and trase_hdbscan_mst on a workspace of
    exactly trase_hdbscan_sizes(n, D, k) bytes -> (core2 fp32 bits as uint32 (n,), keys int64 (n,), counts int32 (18,))."""
    from trase_amd import _lib
    lib = _lib.load()
    n, D = X.shape
    sz = C.c_size_t()
    _lib.check(lib.trase_hdbscan_sizes(n, D, k, C.byref(sz)), "trase_hdbscan_sizes")
    x = on_device(X)
    x0 = x.clone()
    ws, core_buf, keys, counts = _guarded(sz.value), _guarded(4 * n), _guarded(8 * n), _guarded(4 * 18)
    dev = torch.cuda.current_device()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if core2 is None:
        _lib.check(lib.trase_hdbscan_core(_lib.ptr(x), n, D, k, _lib.ptr(core_buf), _lib.ptr(ws), sz.value, dev, st),
                   "trase_hdbscan_core")
    else:
        core_buf[:4 * n].view(torch.float32).copy_(torch.from_numpy(np.ascontiguousarray(core2, dtype=np.float32)))
    _lib.check(lib.trase_hdbscan_mst(_lib.ptr(x), n, D, _lib.ptr(core_buf), _lib.ptr(keys), _lib.ptr(counts), _lib.ptr(ws), sz.value,
                                     dev, st), "trase_hdbscan_mst")
    torch.cuda.synchronize()
    for name, buf, nb in (("workspace", ws, sz.value), ("core2_out", core_buf, 4 * n), ("edge keys", keys, 8 * n),
                          ("counts", counts, 4 * 18)):
        assert _intact(buf, nb), f"{name}: written past its stated size"
    assert torch.equal(x, x0), "X was modified"
    return (core_buf[:4 * n].cpu().numpy().view(np.uint32).copy(), keys[:8 * n].cpu().numpy().view(np.int64).copy(),
            counts[:4 * 18].cpu().numpy().view(np.int32).copy())


def check_keys_and_counts(keys, counts, want, n):
    assert (keys == hx.NO_EDGE).sum() == 1               # an index stops being a root exactly once; the last root never does
    got = np.sort(keys.view(np.uint64)).view(np.int64)
    assert got[-1] == hx.NO_EDGE and np.array_equal(got[:n - 1], want)
    assert counts[0] == n
    live = int(np.count_nonzero(counts))
    assert (counts[:live] > 0).all() and not counts[live:].any() and counts[live - 1] == 1
    for r in range(1, live):                             # every component hooks to another one: at least halved
        assert counts[r] <= (counts[r - 1] + 1) // 2


@pytest.mark.parametrize("n,D,k", [(2, 1, 1), (257, 16, 17), (1025, 64, 64), (4000, 32, 10)])
def test_entry_points_stay_inside_their_bytes(n, D, k):
    Q, X, core_units, want, step = reference(n, D, k, "fine" if D == 64 else "coarse", "volume")
    bits, keys, counts = abi_run(X, k)
    assert np.array_equal(bits, hx.units_to_f32(core_units, step).view(np.uint32))
    check_keys_and_counts(keys, counts, want, n)
    bits2, keys2, counts2 = abi_run(X, k)
    assert np.array_equal(bits, bits2) and np.array_equal(np.sort(keys), np.sort(keys2)) and np.array_equal(counts, counts2)


@pytest.mark.parametrize("n,D", [(257, 3), (1025, 16)])
def test_a_core_distance_of_the_callers_choosing(n, D):
    Q, X, core_units, _, step = reference(n, D, 2, "coarse", "volume")
    # (a) zeros: the Euclidean minimum spanning tree
    zeros = np.zeros(n, dtype=np.int64)
    _, keys, counts = abi_run(X, 2, hx.units_to_f32(zeros, step))
    check_keys_and_counts(keys, counts, hx.mst_keys(Q, zeros, step), n)
    # (b) one constant above every distance (at most D * 63^2 units): every edge ties, the index part of the key decides, and
    # the tree is the star around row 0 -- every row's lightest edge is (0, i), row 0's is (0, 1), one round
    const = np.full(n, 1 << 23, dtype=np.int64)
    assert D * 63 * 63 < 1 << 23
    w = hx.units_to_f32(const, step)
    _, keys, counts = abi_run(X, 2, w)
    star = (np.int64(w.view(np.uint32)[0]) << 32) | np.arange(1, n, dtype=np.int64)
    check_keys_and_counts(keys, counts, star, n)
    assert counts[1] == 1
    # (c) a constant on the odd rows (the median second-neighbour distance of the cloud), zero on the even ones
    c = int(np.median(core_units))
    half = np.where(np.arange(n) % 2 == 1, c, 0).astype(np.int64)
    _, keys, counts = abi_run(X, 2, hx.units_to_f32(half, step))
    want = hx.mst_keys(Q, half, step)
    at_c = (want >> 32) == hx.units_to_f32(c, step).view(np.uint32)
    assert at_c.sum() >= n // 8 and (~at_c).sum() >= n // 8          # the constant and plain distances both carry the tree
    check_keys_and_counts(keys, counts, want, n)


def test_on_a_stream_of_the_callers():
    n, D, k = 513, 12, 16
    Q, X, core_units, keys, step = reference(n, D, k, "coarse", "volume")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = run(X, k)
    s.synchronize()
    check_against_reference(got, n, k, core_units, keys, step)


# ---- error paths and conversions of the wrapper -----------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_row_that_is_not_finite_is_refused(bad):
    """By the code: every distance to or from such a row is NaN or +inf and is never inserted (``d2 < worst`` fails), so its
    own list stays +inf: its core distance is +inf, every edge into it weighs fmaxf(+inf, .) = +inf, the tree still closes
    through one of them and ``_mst_edges`` sees weight bits that are not finite."""
    from trase_amd.segment import hdbscan
    Q, X = hx.lattice_points("volume", 300, 8, "coarse", 77)
    X = X.copy()
    X[123, 5] = bad
    with pytest.raises(ValueError, match="not finite"):
        hdbscan(torch.from_numpy(X).to(DEV), min_cluster_size=5)


def test_input_conversions():
    """fp16, fp64 and a transposed view hold the same lattice numbers (multiples of 1/4 below 8 are fp16 numbers): the same
    bytes out as for the fp32 contiguous copy."""
    from trase_amd.segment import hdbscan
    n, D, k = 257, 9, 15
    Q, X, core_units, keys, step = reference(n, D, k, "coarse", "volume")
    base = run(X, k)
    check_against_reference(base, n, k, core_units, keys, step)
    x = on_device(X)
    transposed = torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV).T
    assert not transposed.is_contiguous() and torch.equal(transposed, x)
    for t in (x.half(), x.double(), transposed):
        assert torch.equal(t.float().contiguous(), x)
        labels, edges, core = hdbscan(t, min_cluster_size=k, min_samples=k, return_mst=True)
        assert np.array_equal(labels.cpu().numpy(), base[0]) and np.array_equal(edges.cpu().numpy(), base[1])
        assert np.array_equal(core.cpu().numpy(), base[2])


# ---- label_centres at its own edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,D,N", [(1, 1, 5), (1, 64, 300), (128, 64, 1000), (128, 1, 50), (129, 1, 1000), (129, 64, 100),
                                    (4096, 64, 3000), (4096, 1, 5000)])
def test_label_centres_at_the_batch_edges(C_, D, N):
    """C = 128 | 129 is the step from one batch of label sums to two, 4096 the limit; with N < C most labels are empty.  An
    empty label's row: hd_centre_kernel divides its zero sums by its zero count, 0 / 0 = NaN in every dimension, the norm is NaN,
    fmaxf(NaN, 1e-12) = 1e-12 and NaN / 1e-12 = NaN -- the float64 mean of no rows is NaN as well, so the row is pinned as NaN.
    Lattice rows: the per-label sums are exact whatever their order, so two calls give the same bytes."""
    from trase_amd.segment import label_centres
    Q, X = hx.lattice_points("volume", N, D, "coarse", 1000 * C_ + D)
    g = np.random.default_rng(C_ + D + N)
    lab = g.integers(-1, C_, N)
    lab[N // 4:N // 2] = -1                              # a stretch of rows that belong nowhere
    x, l = torch.from_numpy(X).to(DEV), torch.from_numpy(lab).to(DEV)
    out = label_centres(x, l, C_)
    assert out.shape == (C_, D) and out.dtype == torch.float32
    assert label_centres(x, l, C_).cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
    got = out.cpu().double().numpy()
    count = np.bincount(lab[lab >= 0], minlength=C_)
    if N < C_:
        assert (count == 0).sum() >= C_ - N
    X64 = X.astype(np.float64)
    worst = 0.0
    for c in range(C_):
        if count[c] == 0:
            assert np.isnan(got[c]).all()
            continue
        m = X64[lab == c].mean(0)
        worst = max(worst, float(np.abs(got[c] - m / max(np.linalg.norm(m), 1e-12)).max()))     # F.normalize's clamp
    print(f"label_centres C {C_} D {D} N {N}: {int((count == 0).sum())} empty labels, max abs error {worst:.3e}")
    assert worst <= 2e-6
