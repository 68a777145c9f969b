"""The host half of HDBSCAN (trase_amd.segment.hdbscan_hierarchy) against scikit-learn's labels, without a GPU: fed the
float64 scipy minimum spanning tree of every fixture case, the partition must equal the fixture's on every point up to a
renaming of the cluster ids, noise matching noise.  Also the ``hdbscan`` shim's argument checks."""
import os

import numpy as np
import pytest

from tests.hdbscan_reference import CASES, MIN_CLUSTER_SIZE, same_partition

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdbscan.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hierarchy_reproduces_the_fixture_partition(golden, name):
    from trase_amd.segment import hdbscan_hierarchy
    case = CASES[name]
    ij, w = golden[f"{name}_mst_ij"], golden[f"{name}_mst_w"]
    want = golden[f"{name}_labels"].astype(np.int64)
    n = want.shape[0]
    assert ij.shape == (n - 1, 2)
    edges = np.concatenate([ij.astype(np.float64), w[:, None]], 1)
    got = hdbscan_hierarchy(edges, n, min_cluster_size=MIN_CLUSTER_SIZE, cluster_selection_epsilon=case["eps"],
                            allow_single_cluster=case["single"])
    assert got.shape == (n,) and got.dtype == np.int64
    assert same_partition(got, want), f"{name}: {(got < 0).sum()} noise points against {(want < 0).sum()}"
    # the documented numbering: 0..C-1 by the smallest member index
    firsts = [int(np.nonzero(got == c)[0][0]) for c in range(int(got.max()) + 1)]
    assert firsts == sorted(firsts) and set(np.unique(got)) <= set(range(-1, len(firsts)))


def test_hierarchy_does_not_depend_on_the_order_or_direction_of_the_edges(golden):
    from trase_amd.segment import hdbscan_hierarchy
    name = "noisy1500"
    ij, w = golden[f"{name}_mst_ij"], golden[f"{name}_mst_w"]
    n = ij.shape[0] + 1
    edges = np.concatenate([ij.astype(np.float64), w[:, None]], 1)
    rng = np.random.default_rng(0)
    shuffled = edges[rng.permutation(n - 1)]
    flip = rng.random(n - 1) < 0.5
    shuffled[flip, 0], shuffled[flip, 1] = shuffled[flip, 1].copy(), shuffled[flip, 0].copy()
    a = hdbscan_hierarchy(edges, n, cluster_selection_epsilon=0.01)
    b = hdbscan_hierarchy(shuffled, n, cluster_selection_epsilon=0.01)
    assert np.array_equal(a, b)


def test_hierarchy_rejects_what_is_not_a_spanning_tree():
    from trase_amd.segment import hdbscan_hierarchy
    with pytest.raises(ValueError, match="3 edges"):
        hdbscan_hierarchy(np.zeros((2, 3)), 4)
    with pytest.raises(ValueError, match="spanning tree"):
        hdbscan_hierarchy(np.array([[0, 1, 1.0], [1, 0, 2.0], [2, 3, 1.0]]), 4, min_cluster_size=2)


def test_all_noise_when_nothing_reaches_min_cluster_size():
    from trase_amd.segment import hdbscan_hierarchy
    edges = np.array([[i, i + 1, 1.0 + i] for i in range(5)], dtype=np.float64)
    assert (hdbscan_hierarchy(edges, 6, min_cluster_size=10) == -1).all()


def test_shim_rejects_unsupported_metrics_and_selection_methods():
    import hdbscan
    with pytest.raises(NotImplementedError, match="only 'euclidean'"):
        hdbscan.HDBSCAN(min_cluster_size=10, metric="manhattan")
    with pytest.raises(NotImplementedError, match="only 'eom'"):
        hdbscan.HDBSCAN(min_cluster_size=10, cluster_selection_method="leaf")
    c = hdbscan.HDBSCAN(min_cluster_size=10, cluster_selection_epsilon=0.01, allow_single_cluster=False, core_dist_n_jobs=64,
                        prediction_data=False)
    assert c.labels_ is None and c.min_samples is None


def test_device_functions_reject_cpu_tensors():
    import torch
    from trase_amd import segment
    with pytest.raises(RuntimeError, match="GPU only"):
        segment.hdbscan(torch.zeros(20, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        segment.density_clusters(torch.zeros(20, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        segment.label_centres(torch.zeros(20, 4), torch.zeros(20, dtype=torch.int64), 1)


def test_limits_are_checked_by_the_library_without_a_gpu():
    import ctypes as C
    from trase_amd import _lib
    lib = _lib.load()
    sz = C.c_size_t()
    assert lib.trase_hdbscan_sizes(6000, 32, 10, C.byref(sz)) == 0 and sz.value > 0
    for n, D, k, word in ((1, 32, 1, "2 <= n <= 65536"), (65537, 32, 10, "2 <= n <= 65536"), (100, 65, 10, "1 <= D <= 64"),
                          (100, 0, 10, "1 <= D <= 64"), (100, 32, 65, "1 <= k <= 64"), (100, 32, 0, "1 <= k <= 64"),
                          (8, 32, 8, "k < n")):
        assert lib.trase_hdbscan_sizes(n, D, k, C.byref(sz)) != 0
        assert word in _lib.last_error(), (n, D, k, _lib.last_error())
    assert lib.trase_label_centres_sizes(100, 32, 4097, C.byref(sz)) != 0 and "1 <= C <= 4096" in _lib.last_error()
