"""Writes tests/golden/hdbscan.npz: the HDBSCAN fixture, from scikit-learn 1.7.2 and scipy in float64.

    python tests/golden/make_hdbscan.py

Per case of tests/hdbscan_reference.CASES: the labels of
``sklearn.cluster.HDBSCAN(min_cluster_size=10, min_samples=11, cluster_selection_epsilon=..., allow_single_cluster=...,
algorithm="brute")`` on the float64 image of the fp32 rows; the float64 core distances; the minimum spanning tree of the
dense mutual-reachability matrix from ``scipy.sparse.csgraph.minimum_spanning_tree`` as (i, j) and weights, ascending in
weight (so the weight column is the sorted weights); a SHA-256 of the rows, and the rows themselves for the small sets.

scikit-learn counts the point itself among its neighbours and the ``hdbscan`` package (and trase_amd) do not: sklearn's
min_samples = 11 is the package's and our 10.

Every case must be robust: scikit-learn has to return the same partition on the rows, on the rows perturbed by 1e-6
relative and on the rows in two other orders, or the script stops and the case has to be replaced.  The last matters because
mutual-reachability weights tie EXACTLY wherever a point's core distance exceeds its distance to several others, and which
of the tied edges a spanning tree takes follows the scan order of whoever builds it.  A sparse point that reaches two
clusters at its own core distance belongs to either; scikit-learn itself moves such points when the rows are permuted."""
import os
import sys

import numpy as np
from scipy.sparse.csgraph import minimum_spanning_tree
from sklearn.cluster import HDBSCAN

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.hdbscan_reference import (CASES, MIN_CLUSTER_SIZE, MIN_SAMPLES, STORE_X_UP_TO, digest, make_points,  # noqa: E402
                                     same_partition)


def sk_labels(X64, eps, single):
    return HDBSCAN(min_cluster_size=MIN_CLUSTER_SIZE, min_samples=MIN_SAMPLES + 1, cluster_selection_epsilon=eps,
                   allow_single_cluster=single, algorithm="brute").fit_predict(X64)


def main():
    out = {}
    for name, case in CASES.items():
        X = make_points(**case)
        X64 = X.astype(np.float64)
        n = X.shape[0]
        labels = sk_labels(X64, case["eps"], case["single"])
        rng = np.random.default_rng(1000 + case["seed"])
        moved = X64 * (1.0 + 1e-6 * rng.uniform(-1.0, 1.0, X64.shape))
        assert same_partition(labels, sk_labels(moved, case["eps"], case["single"])), f"{name}: not robust, replace it"
        for _ in range(2):                          # nor may it hang on the order in which equal weights are met
            perm = rng.permutation(n)
            back = np.empty_like(labels)
            back[perm] = sk_labels(X64[perm], case["eps"], case["single"])
            assert same_partition(labels, back), f"{name}: depends on the row order, replace it"
        d = np.zeros((n, n))
        for k in range(X.shape[1]):                 # sum (a - b)^2, never |a|^2 + |b|^2 - 2ab
            diff = X64[:, k, None] - X64[None, :, k]
            d += diff * diff
        d = np.sqrt(d)
        core = np.sort(d, axis=1)[:, MIN_SAMPLES]   # column 0 is the point itself
        mr = np.maximum(np.maximum(core[:, None], core[None, :]), d)
        np.fill_diagonal(mr, 0.0)
        assert (mr[~np.eye(n, dtype=bool)] > 0).all()
        tree = minimum_spanning_tree(mr).tocoo()
        assert tree.nnz == n - 1
        order = np.argsort(tree.data, kind="stable")
        out[f"{name}_labels"] = labels.astype(np.int16)
        out[f"{name}_core"] = core
        out[f"{name}_mst_ij"] = np.stack([tree.row[order], tree.col[order]], 1).astype(np.int32)
        out[f"{name}_mst_w"] = tree.data[order]
        out[f"{name}_sha256"] = np.array(digest(X))
        if n <= STORE_X_UP_TO:
            out[f"{name}_X"] = X
        print(f"{name}: n {n}, clusters {labels.max() + 1}, noise {(labels < 0).sum()}")
    path = os.path.join(HERE, "hdbscan.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
