"""tests/hdbscan_exact_reference.py against scipy, a brute-force Kruskal and direct integer loops; the case plan of
tests/test_gpu_hdbscan_exact.py; the error paths of ``trase_amd.segment._mst_edges``.  No GPU."""
import numpy as np
import pytest

from tests import hdbscan_exact_reference as hx

# (n, D, k, grid, kind): the last one must contain zero-weight edges
SCIPY_CASES = [(257, 3, 5, "coarse", "volume"), (300, 16, 17, "fine", "volume"), (130, 4, 2, "coarse", "coincident"),
               (130, 4, 1, "coarse", "coincident")]


def _case(n, D, k, grid, kind):
    Q, X = hx.lattice_points(kind, n, D, grid, hx.case_seed(n, D, k))
    hx.assert_exact(Q)                                   # the premise of everything below
    return Q, X, hx.core2_units(Q, k), hx.GRIDS[grid][0]


@pytest.mark.parametrize("grid", sorted(hx.GRIDS))
@pytest.mark.parametrize("kind", hx.KINDS)
def test_every_cloud_is_exact_at_64_dimensions(kind, grid):
    step, lo, levels = hx.GRIDS[grid]
    for n in (2, 3, 1025):
        Q, X = hx.lattice_points(kind, n, 64, grid, n)
        hx.assert_exact(Q)
        assert X.dtype == np.float32 and X.flags["C_CONTIGUOUS"] and X.min() >= lo and X.max() < -lo
        assert np.array_equal((X.astype(np.float64) - lo) / step, Q.astype(np.float64))
        again = hx.lattice_points(kind, n, 64, grid, n)
        assert np.array_equal(again[0], Q) and again[1].tobytes() == X.tobytes()
    if kind == "coincident":
        assert np.array_equal(Q[513:], Q[:512])
    if kind == "line":
        assert ((Q.max(0) - Q.min(0)) > 0).sum() == 1
    if kind == "plane":
        assert ((Q.max(0) - Q.min(0)) > 0).sum() == 2


def test_assert_exact_refuses_a_cloud_beyond_fp32():
    Q = np.zeros((2, 64), dtype=np.int64)
    Q[1] = 512                                           # 64 * 512^2 == 2^24
    with pytest.raises(AssertionError, match="not exact"):
        hx.assert_exact(Q)
    Q[1, 0] = 511
    hx.assert_exact(Q)


@pytest.mark.parametrize("n,D,k,grid,kind", [(2, 1, 1, "coarse", "volume"), (40, 3, 1, "coarse", "coincident"),
                                             (65, 64, 64, "fine", "volume"), (61, 5, 17, "coarse", "blobs")])
def test_core_distances_equal_an_integer_loop(n, D, k, grid, kind):
    Q, _, core, _ = _case(n, D, k, grid, kind)
    for i in range(n):
        d = sorted(sum((int(Q[i, c]) - int(Q[j, c])) ** 2 for c in range(D)) for j in range(n) if j != i)
        assert core[i] == d[k - 1]
    assert core.dtype == np.int64
    if kind == "coincident":
        assert (core[:n // 2] == 0).all()                # a duplicate is another row


def _pairs(n):
    return np.triu_indices(n, 1)


def _scipy_tree(weights, n):
    from scipy.sparse.csgraph import minimum_spanning_tree
    iu, ju = _pairs(n)
    G = np.zeros((n, n), dtype=np.float64)
    G[iu, ju] = weights
    T = minimum_spanning_tree(G).tocoo()
    return T.row.astype(np.int64), T.col.astype(np.int64), T.data


@pytest.mark.parametrize("n,D,k,grid,kind", SCIPY_CASES)
def test_the_tree_equals_scipy_on_rank_unique_weights(n, D, k, grid, kind):
    """scipy on the dense graph whose weights are 1 + the rank of each pair's key: unique and never zero (scipy reads a
    zero as no edge), so its tree is THE tree under the key order."""
    Q, _, core, step = _case(n, D, k, grid, kind)
    keys, w = hx.key_matrix(Q, core, step)
    iu, ju = _pairs(n)
    flat = keys[iu, ju]
    assert len(np.unique(flat)) == flat.size             # a strict total order
    rank = np.empty(flat.size, dtype=np.int64)
    rank[np.argsort(flat)] = np.arange(flat.size)
    a, b, _ = _scipy_tree(1.0 + rank, n)
    want = np.sort(keys[np.minimum(a, b), np.maximum(a, b)])
    got = hx.mst_keys(Q, core, step)
    assert got.dtype == np.int64 and got.shape == (n - 1,)
    assert np.array_equal(got, want)
    if kind == "coincident" and k == 1:
        assert (got >> 32 == 0).sum() >= n // 2          # every duplicated pair is a zero-weight edge of the tree
        assert (core == 0).all()
    edges = hx.decode_keys(got)
    assert (edges[:, 0] < edges[:, 1]).all() and np.array_equal(edges[:, 2], np.sqrt(w[edges[:, 0].astype(int), edges[:, 1].astype(int)]) * step)


@pytest.mark.parametrize("n,D,k,grid,kind", [(2, 1, 1, "coarse", "volume"), (3, 2, 2, "coarse", "plane"),
                                             (64, 2, 3, "coarse", "volume"), (64, 1, 2, "coarse", "line"),
                                             (50, 9, 1, "coarse", "coincident"), (64, 64, 16, "fine", "blobs")])
def test_the_tree_equals_a_brute_force_kruskal(n, D, k, grid, kind):
    Q, _, core, step = _case(n, D, k, grid, kind)
    keys, _ = hx.key_matrix(Q, core, step)
    iu, ju = _pairs(n)
    up = list(range(n))

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x
    want = []
    for e in np.argsort(keys[iu, ju]):
        a, b = find(int(iu[e])), find(int(ju[e]))
        if a != b:
            up[a] = b
            want.append(int(keys[iu[e], ju[e]]))
    assert len(want) == n - 1
    assert np.array_equal(hx.mst_keys(Q, core, step), np.asarray(want, dtype=np.int64))


@pytest.mark.parametrize("n,D,k,grid,kind", SCIPY_CASES[:2] + [(200, 8, 3, "coarse", "blobs")])
def test_tree_weights_equal_scipy_on_the_float64_graph(n, D, k, grid, kind):
    """As the fixture of tests/test_gpu_hdbscan.py is made: scipy's tree of the float64 mutual-reachability DISTANCES, ties
    and all.  Every minimum spanning tree of a graph has the same sorted weights; sqrt(units) * step is the distance bit for
    bit (step is a power of two), so the sorted weights and their sum are equal, not close."""
    Q, _, core, step = _case(n, D, k, grid, kind)
    _, w = hx.key_matrix(Q, core, step)
    iu, ju = _pairs(n)
    assert w[iu, ju].min() > 0                           # scipy would read a zero weight as no edge
    _, _, data = _scipy_tree(np.sqrt(w[iu, ju].astype(np.float64)) * step, n)
    got = hx.decode_keys(hx.mst_keys(Q, core, step))[:, 2]
    assert np.array_equal(np.sort(data), got)
    assert np.sort(data).sum() == got.sum()


def test_a_core_distance_of_the_callers_choosing():
    """With one constant above every distance every edge ties and the key's index part decides: the star around row 0."""
    Q, _ = hx.lattice_points("volume", 40, 3, "coarse", 4)
    hx.assert_exact(Q)
    keys = hx.mst_keys(Q, np.full(40, 1 << 23), 0.25)
    edges = hx.decode_keys(keys)
    assert np.array_equal(edges[:, 0], np.zeros(39)) and np.array_equal(edges[:, 1], np.arange(1, 40))
    assert (edges[:, 2] == np.sqrt(float(1 << 23) / 16)).all()


def test_the_plan_meets_every_listed_value():
    plan = hx.exact_plan()
    assert 55 <= len(plan) <= 65 and len(set(plan)) == len(plan)
    for n, D, k, grid, kind, offset in plan:
        assert 1 <= k < n and k in hx.KS and offset in (0, 1)
    assert {c[0] for c in plan} == set(hx.NS) | {hx.N_SPLIT15}
    assert {c[1] for c in plan} == set(hx.DS)
    assert {c[2] for c in plan} == set(hx.KS)
    assert {(c[3], c[4]) for c in plan} >= set(hx.CLOUDS)
    assert {k for k in hx.KINDS} == {c[4] for c in plan if c[3] == "coarse"}
    # every list size beside every row width: (DP, KC) of hd_core_kernel
    dp = lambda D: 8 if D <= 8 else 16 if D <= 16 else 32 if D <= 32 else 64
    assert {(dp(c[1]), c[2] <= 16) for c in plan} == {(p, s) for p in (8, 16, 32, 64) for s in (True, False)}
    assert sum(c[0] > 1025 for c in plan) <= 4 and sum(c[0] == hx.N_SPLIT15 for c in plan) == 1
    assert (hx.N_SPLIT15, 4, 2, "coarse", "volume", 0) in plan
    assert any(c[1] == 64 and c[2] == 64 for c in plan)
    assert any(c[2] == 64 and c[0] == 65 for c in plan) and any(c[2] == 63 and c[0] >= 65 for c in plan)
    assert any(c[4] == "coincident" and c[2] == 1 for c in plan) and any(c[4] == "line" and c[1] == 1 for c in plan)
    for D in (4, 32):                                    # the misaligned runs, each with its aligned twin
        off = [c for c in plan if c[1] == D and c[5] == 1]
        assert off and all(c[:5] + (0,) in plan for c in off)
    assert all(c[5] == 0 or c[1] % 4 == 0 for c in plan)


# ---- trase_amd.segment._mst_edges on hand-made read-backs -----------------------------------------------------------------
def _read_back(keys, counts):
    """int64 (n + 9,) as ``_hdbscan_device`` leaves it: n key slots (one keeps no edge), then 18 int32 counts."""
    c = np.zeros(18, dtype=np.int32)
    c[:len(counts)] = counts
    return np.concatenate([np.asarray(keys, dtype=np.int64), [hx.NO_EDGE], c.view(np.int64)])


def test_mst_edges_decodes_what_the_reference_encodes():
    from trase_amd.segment import _mst_edges
    Q, _, core, step = _case(130, 4, 1, "coarse", "coincident")
    keys = hx.mst_keys(Q, core, step)
    shuffled = np.random.default_rng(0).permutation(np.concatenate([keys, [hx.NO_EDGE]]))
    out = _read_back(keys, [130, 50, 9, 1])
    out[:130] = shuffled                                 # the slots are in no order on the device
    edges = _mst_edges(out, 130)
    assert edges.dtype == np.float64 and np.array_equal(edges, hx.decode_keys(keys))


def test_mst_edges_raises_when_the_tree_did_not_close():
    from trase_amd.segment import _mst_edges
    Q, _, core, step = _case(64, 2, 3, "coarse", "volume")
    keys = hx.mst_keys(Q, core, step)
    for counts in ([64, 30, 12, 5, 2], [64], []):
        with pytest.raises(RuntimeError, match="did not close"):
            _mst_edges(_read_back(keys, counts), 64)
    assert _mst_edges(_read_back(keys, [64, 30, 12, 5, 1]), 64).shape == (63, 3)


def test_mst_edges_raises_on_an_infinite_weight():
    from trase_amd.segment import _mst_edges
    Q, _, core, step = _case(64, 2, 3, "coarse", "volume")
    keys = hx.mst_keys(Q, core, step)
    keys[-1] = (np.int64(0x7f800000) << 32) | (keys[-1] & 0xffffffff)
    with pytest.raises(ValueError, match="not finite"):
        _mst_edges(_read_back(keys, [64, 20, 1]), 64)
