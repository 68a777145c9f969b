"""HDBSCAN on the GPU (trase_amd.segment.hdbscan, trase_amd/csrc/hdbscan.hip) against the scikit-learn / scipy float64 fixture
tests/golden/hdbscan.npz, and ``density_clusters`` against the gui.py:274-290 statements composed in torch.

The bound on every squared distance is REL = 2 (D + 2) 2^-24 relative: the fp32 difference form sum (a_d - b_d)^2 in a fixed
order has the forward error bound (D + 2) 2^-24 (one rounding of each difference, doubled by the square, one of each product
and D - 1 of the sum, first order), and one factor of 2 is margin.  The k-th smallest of perturbed values and the sorted
weights of a minimum spanning tree move no further than the largest single perturbation, so the same bound holds for the
core distances and for the sorted tree weights."""
import os
import types

import numpy as np
import pytest
import torch

from tests.hdbscan_reference import CASES, MIN_CLUSTER_SIZE, MIN_SAMPLES, case_points, same_partition

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _dev():
    return torch.device("cuda", 0)


def _rel(D):
    return 2.0 * (D + 2) * 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "hdbscan.npz"))


@pytest.fixture(scope="module")
def runs(golden):
    """name -> (X fp32 ndarray, labels, edges, core) of one ``hdbscan(..., return_mst=True)`` call per case."""
    from trase_amd.segment import hdbscan
    out = {}
    for name, case in CASES.items():
        X = case_points(name, golden)
        labels, edges, core = hdbscan(torch.from_numpy(X).to(_dev()), min_cluster_size=MIN_CLUSTER_SIZE, min_samples=MIN_SAMPLES,
                                      cluster_selection_epsilon=case["eps"], allow_single_cluster=case["single"],
                                      return_mst=True)
        assert labels.dtype == torch.int64 and labels.device.type == "cuda" and edges.dtype == torch.float64
        out[name] = (X, labels.cpu().numpy(), edges.cpu().numpy(), core.cpu().numpy())
    return out


def _sq_dist64(X, i, j):
    d = X[i].astype(np.float64) - X[j].astype(np.float64)
    return (d * d).sum(-1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_core_distances_within_the_fp32_bound(golden, runs, name):
    X, _, _, core = runs[name]
    want2 = golden[f"{name}_core"] ** 2
    err = np.abs(core ** 2 - want2) / want2
    print(f"{name}: squared core distances, max relative error {err.max():.3e} (bound {_rel(X.shape[1]):.3e})")
    assert err.max() <= _rel(X.shape[1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_edges_are_a_spanning_tree_of_the_mutual_reachability_graph(golden, runs, name):
    X, _, edges, core = runs[name]
    n, D = X.shape
    assert edges.shape == (n - 1, 3)
    i, j, w = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64), edges[:, 2]
    assert (i >= 0).all() and (i < j).all() and (j < n).all()
    assert (np.diff(w) >= 0).all()                                   # canonical order: ascending weight, then (i, j)
    tie = np.diff(w) == 0
    assert (np.diff(i * n + j)[tie] > 0).all()
    up = np.arange(n)
    for a, b in zip(i.tolist(), j.tolist()):                         # union-find must join everything: no cycle in n - 1 edges
        while up[a] != a:
            up[a] = up[up[a]]
            a = up[a]
        while up[b] != b:
            up[b] = up[up[b]]
            b = up[b]
        assert a != b, "cycle"
        up[a] = b
    mr2 = np.maximum(np.maximum(core[i] ** 2, core[j] ** 2), _sq_dist64(X, i, j))
    err = np.abs(w ** 2 - mr2) / mr2
    print(f"{name}: edge weights against the float64 mutual reachability, max relative error {err.max():.3e}")
    assert err.max() <= _rel(D)
    want2 = golden[f"{name}_mst_w"] ** 2
    err = np.abs(np.sort(w) ** 2 - want2) / want2
    print(f"{name}: sorted tree weights against scipy's, max relative error {err.max():.3e} (bound {_rel(D):.3e})")
    assert err.max() <= _rel(D)


@pytest.mark.parametrize("name", sorted(CASES))
def test_labels_equal_the_fixture_partition(golden, runs, name):
    import hdbscan
    X, labels, _, _ = runs[name]
    case = CASES[name]
    want = golden[f"{name}_labels"].astype(np.int64)
    assert same_partition(labels, want), f"{name}: {(labels < 0).sum()} noise points against {(want < 0).sum()}"
    clusterer = hdbscan.HDBSCAN(min_cluster_size=MIN_CLUSTER_SIZE, min_samples=MIN_SAMPLES,
                                cluster_selection_epsilon=case["eps"], allow_single_cluster=case["single"], core_dist_n_jobs=16)
    shim = clusterer.fit_predict(X)
    assert isinstance(shim, np.ndarray) and shim is clusterer.labels_ and np.array_equal(shim, labels)


def test_default_min_samples_is_min_cluster_size(golden, runs):
    from trase_amd.segment import hdbscan
    X, labels, _, _ = runs["blobs2000"]
    got = hdbscan(torch.from_numpy(X).to(_dev()), min_cluster_size=MIN_CLUSTER_SIZE, cluster_selection_epsilon=0.01)
    assert np.array_equal(got.cpu().numpy(), labels)


@pytest.mark.parametrize("name", ["blobs6000b", "noisy1500", "small3d"])
def test_two_calls_bit_identical(golden, runs, name):
    from trase_amd.segment import hdbscan
    X, labels, edges, core = runs[name]
    case = CASES[name]
    l2, e2, c2 = hdbscan(torch.from_numpy(X).to(_dev()), min_cluster_size=MIN_CLUSTER_SIZE, min_samples=MIN_SAMPLES,
                         cluster_selection_epsilon=case["eps"], allow_single_cluster=case["single"], return_mst=True)
    assert np.array_equal(l2.cpu().numpy(), labels)
    assert e2.cpu().numpy().tobytes() == edges.tobytes() and c2.cpu().numpy().tobytes() == core.tobytes()


@pytest.mark.parametrize("n,D,k", [(65536, 8, 64), (5000, 64, 17), (777, 5, 3), (2, 1, 1)])
def test_limits_and_odd_shapes_against_float64(n, D, k):
    """The corners of the limits and shapes that are no multiple of anything: core distances against a float64 brute force on
    a sample of the rows, the edges a spanning tree."""
    from trase_amd.segment import hdbscan
    g = np.random.default_rng(n + D)
    X = g.standard_normal((n, D)).astype(np.float32)
    _, edges, core = hdbscan(torch.from_numpy(X).to(_dev()), min_cluster_size=max(k, 2), min_samples=k, return_mst=True)
    edges, core = edges.cpu().numpy(), core.cpu().numpy()
    rows = g.choice(n, min(n, 64), replace=False)
    X64 = X.astype(np.float64)
    d2 = ((X64[rows, None, :] - X64[None, :, :]) ** 2).sum(-1)
    d2[np.arange(len(rows)), rows] = np.inf
    want2 = np.sort(d2, axis=1)[:, k - 1]
    assert (np.abs(core[rows] ** 2 - want2) / want2).max() <= _rel(D)
    assert edges.shape == (n - 1, 3)
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    i, j = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    assert connected_components(sp.coo_matrix((np.ones(n - 1), (i, j)), shape=(n, n)), directed=False)[0] == 1
    mr2 = np.maximum(np.maximum(core[i] ** 2, core[j] ** 2), _sq_dist64(X, i, j))
    assert (np.abs(edges[:, 2] ** 2 - mr2) / mr2).max() <= _rel(D)


def test_duplicate_rows_and_exact_ties():
    """Rows on a grid (every distance tied many times over) with duplicates: still a spanning tree, twice the same one."""
    from trase_amd.segment import hdbscan
    a = np.arange(12, dtype=np.float32)
    X = np.stack(np.meshgrid(a, a, indexing="ij"), -1).reshape(-1, 2)
    X = np.concatenate([X, X[:30]])
    t = torch.from_numpy(X).to(_dev())
    l1, e1, c1 = hdbscan(t, min_cluster_size=5, return_mst=True)
    l2, e2, c2 = hdbscan(t, min_cluster_size=5, return_mst=True)
    assert torch.equal(e1, e2) and torch.equal(c1, c2) and torch.equal(l1, l2)
    n = X.shape[0]
    up = list(range(n))

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x
    for i, j, _ in e1.cpu().numpy():
        ri, rj = find(int(i)), find(int(j))
        assert ri != rj
        up[ri] = rj
    assert float(c1.max()) <= 2.0 and float(e1[:, 2].min()) >= 1.0   # the 5th nearest other row of a grid row lies within 1 .. 2


def test_density_clusters_equals_the_reference_statements():
    """gui.py:274-290 composed in torch around our own ``hdbscan`` labels, for the same seed, apart from the centre indexing."""
    from trase_amd import segment
    N, D, K = 300_000, 32, 9
    g = np.random.default_rng(21)
    centres = g.standard_normal((K, D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    rows = centres[g.integers(0, K, N)] + 0.05 * g.standard_normal((N, D))
    rows *= g.uniform(0.5, 2.0, (N, 1))
    feats = torch.from_numpy(rows.astype(np.float32)).to(_dev())
    before = feats.clone()
    torch.manual_seed(1234)
    ids, cen, index, labels = segment.density_clusters(feats.unsqueeze(1), return_sample=True)
    assert torch.equal(feats, before)
    # the reference's statements
    torch.manual_seed(1234)
    percent = 0.02
    point_features = feats
    keep = torch.rand(point_features.shape[0]) > 1 - percent
    sampled_point_features = point_features[keep.to(_dev())]
    normed_sampled = sampled_point_features / torch.norm(sampled_point_features, dim=-1, keepdim=True)
    assert torch.equal(index.cpu(), torch.nonzero(keep).flatten())
    cluster_labels = segment.hdbscan(normed_sampled, min_cluster_size=10, cluster_selection_epsilon=0.01)
    assert torch.equal(cluster_labels, labels)
    C = int(cluster_labels.max()) + 1
    assert C == K and cen.shape == (C, D) and cen.dtype == torch.float32
    want = torch.stack([torch.nn.functional.normalize(normed_sampled[cluster_labels == c].double().mean(dim=0), dim=-1)
                        for c in range(C)])            # labels 0..C-1, not the reference's i - 1
    err = float((cen.double() - want).abs().max())
    print(f"density_clusters: centres against float64 means, max abs error {err:.3e}")
    assert err <= 2e-6          # fp32 sums of up to ~1000 unit-scale terms per cluster and dimension, then one division
    score = torch.nn.functional.normalize(point_features.double(), dim=-1) @ cen.double().T
    top = score.topk(2, dim=-1)
    decided = (top.values[:, 0] - top.values[:, 1]) > 1e-5      # fp32 dot products of 32 terms of unit rows: error < 2e-6
    assert ids.dtype == torch.int64 and ids.shape == (N,)
    assert torch.equal(ids[decided], top.indices[:, 0][decided]) and float(decided.float().mean()) > 0.999
    assert torch.equal(ids, segment.assign_clusters(feats, cen))
    # the ids go on unchanged
    mask = segment.segment_mask(feats, ids, [0, C - 1], 0.8)
    assert mask.dtype == torch.bool and bool(mask.any()) and bool((ids[mask] == 0).any())
    z = np.load(os.path.join(HERE, "golden", "lift.npz"))
    H, W = z["depth"].shape
    cam = types.SimpleNamespace(full_proj_transform=torch.from_numpy(z["full_proj_transform"]).to(_dev()), image_width=W,
                                image_height=H, znear=float(z["znear"]), zfar=float(z["zfar"]))
    pts = torch.from_numpy(g.uniform(-1.0, 1.0, (N, 3)).astype(np.float32)).to(_dev())
    votes = segment.lift_votes(torch.from_numpy(z["depth"]).to(_dev()), torch.from_numpy(z["prompt_mask"]).to(_dev()), cam, pts, ids)
    assert votes.dtype == torch.int64 and 1 <= votes.numel() <= C and int(votes.sum()) > 0


def test_label_centres_beyond_one_chunk_of_labels():
    """300 labels: three passes of the 128-label sums; noise rows belong nowhere."""
    from trase_amd.segment import label_centres
    g = np.random.default_rng(3)
    N, D, C = 20_000, 17, 300
    X = g.standard_normal((N, D)).astype(np.float32)
    lab = g.integers(-1, C, N)
    got = label_centres(torch.from_numpy(X).to(_dev()), torch.from_numpy(lab).to(_dev()), C).cpu().double().numpy()
    for c in (0, 127, 128, 255, 256, 299):
        m = X[lab == c].astype(np.float64).mean(0)
        assert np.abs(got[c] - m / np.linalg.norm(m)).max() <= 2e-6


def test_argument_errors():
    from trase_amd import segment
    dev = _dev()
    with pytest.raises(ValueError, match="2 <= n <= 65536"):
        segment.hdbscan(torch.zeros(65537, 4, device=dev))
    with pytest.raises(ValueError, match="2 <= n <= 65536"):
        segment.hdbscan(torch.zeros(1, 4, device=dev), min_cluster_size=2, min_samples=1)
    with pytest.raises(ValueError, match="1 <= D <= 64"):
        segment.hdbscan(torch.zeros(100, 65, device=dev))
    with pytest.raises(ValueError, match="1 <= k <= 64"):
        segment.hdbscan(torch.zeros(100, 4, device=dev), min_samples=65)
    with pytest.raises(ValueError, match="1 <= k <= 64"):
        segment.hdbscan(torch.zeros(100, 4, device=dev), min_samples=0)
    with pytest.raises(ValueError, match="k < n"):
        segment.hdbscan(torch.zeros(10, 4, device=dev), min_cluster_size=10)
    with pytest.raises(ValueError, match="must be"):
        segment.hdbscan(torch.zeros(10, device=dev))
    with pytest.raises(RuntimeError, match="GPU only"):
        segment.hdbscan(torch.zeros(100, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        segment.density_clusters(torch.zeros(100, 4))
