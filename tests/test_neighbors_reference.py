"""The float64 restatements of tests/neighbors_reference.py against the reference's own results (tests/golden/neighbors.npz,
written by tests/golden/make_neighbors.py), the transposed graph against a brute-force transpose, the refusals of the new
entry points, and the premise of the exact k-NN tests on the GPU.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import neighbors_reference as nr

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "neighbors.npz"))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_knn_with_the_tie_rule(fx):
    assert np.array_equal(nr.knn_lex(fx["feat_xyz"], fx["feat_xyz"], 6)[1][:, 1:], fx["feat_idx_f64"])
    for name, clusters in (("rigid2", 2), ("rigid1", 1)):
        ids = fx[f"{name}_cluster_ids"]
        for c, cid in enumerate(np.unique(ids)[:clusters]):
            p = fx[f"{name}_xyz1"][ids == cid]
            dist, idx = nr.knn_lex(p, p, 129)
            assert np.array_equal(idx[:, 1:], fx[f"{name}_idx{c}_f64"])
            if len(p) < 129:           # the padded case: index 0, distance 0 behind the cloud's own points
                assert not idx[:, len(p):].any() and not dist[:, len(p):].any()
    # ties: equal distances come out in ascending index order
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, 0]], dtype=np.float32)
    dist, idx = nr.knn_lex(p[:1], p, 5)
    assert idx.tolist() == [[0, 4, 1, 2, 3]] and dist.tolist() == [[0, 0, 1, 1, 1]]


def test_feature_loss_restatement(fx):
    r = nr.feat3d(fx["feat_feats"], fx["feat_idx_f64"])
    assert rel(r["loss"], fx["feat_loss_f64"]) <= 1e-12
    assert rel(r["grad"], fx["feat_grad_f64"]) <= 1e-12
    # the reference's own fp32 run lies inside the bounds the kernels are held to
    assert abs(float(fx["feat_loss_f32"]) - r["loss"]) <= r["loss_bound"]
    assert (np.abs(fx["feat_grad_f32"] - r["grad"]) <= r["grad_bound"]).all()


@pytest.mark.parametrize("name", ("rigid2", "rigid1"))
def test_rigid_loss_restatement(fx, name):
    ids = fx[f"{name}_cluster_ids"]
    sel = ids == np.unique(ids)[0]
    p1, p2, idx = fx[f"{name}_xyz1"][sel], fx[f"{name}_xyz2"][sel], fx[f"{name}_idx0_f64"]
    assert rel(nr.edge_moments(p1, p2, idx)[0], fx[f"{name}_S0_f64"]) <= 1e-12
    assert rel(nr.edge_residual(p1, p2, idx, fx[f"{name}_R0_f64"])[0], fx[f"{name}_res0_f64"]) <= 1e-12
    r = nr.rigid_loss(fx[f"{name}_xyz1"], fx[f"{name}_xyz2"], ids, 128)
    assert rel(r["loss"], fx[f"{name}_loss_f64"]) <= 1e-12
    assert rel(r["g1"], fx[f"{name}_g1_f64"]) <= 1e-12 and rel(r["g2"], fx[f"{name}_g2_f64"]) <= 1e-12


def test_edge_gradients_match_finite_differences():
    g = np.random.default_rng(0)
    N, k = 12, 4
    p1, p2 = g.normal(size=(N, 3)), g.normal(size=(N, 3))
    idx = g.integers(0, N, size=(N, k)).astype(np.int32)
    idx[3, 1] = -1
    gS, R, w = g.normal(size=(N, 3, 3)), g.normal(size=(N, 3, 3)), g.normal(size=N)
    g1, g2, _, _ = nr.edge_moments_grad(p1, p2, idx, gS)
    rr = nr.edge_residual_grad(p1, p2, idx, R, w)
    h = 1e-6

    def fd(fun, x):
        out = np.zeros_like(x)
        for i in np.ndindex(x.shape):
            a, b = x.copy(), x.copy()
            a[i] += h
            b[i] -= h
            out[i] = (fun(a) - fun(b)) / (2 * h)
        return out
    assert rel(g1, fd(lambda x: (nr.edge_moments(x, p2, idx)[0] * gS).sum(), p1)) < 1e-8
    assert rel(g2, fd(lambda x: (nr.edge_moments(p1, x, idx)[0] * gS).sum(), p2)) < 1e-8
    assert rel(rr["g1"], fd(lambda x: (nr.edge_residual(x, p2, idx, R)[0] * w).sum(), p1)) < 1e-8
    assert rel(rr["g2"], fd(lambda x: (nr.edge_residual(p1, x, idx, R)[0] * w).sum(), p2)) < 1e-8
    assert rel(rr["gR"], fd(lambda x: (nr.edge_residual(p1, p2, idx, x)[0] * w).sum(), R)) < 1e-8
    f = g.normal(size=(N, 5))
    r = nr.feat3d(f, idx, g_out=0.5)
    assert rel(r["grad"], fd(lambda x: 0.5 * nr.feat3d(x, idx)["loss"], f)) < 1e-7


def test_reversal_equals_a_brute_force_transpose():
    g = np.random.default_rng(1)
    for N, k in ((1, 1), (7, 3), (64, 5), (65, 128)):
        idx = g.integers(0, N, size=(N, k)).astype(np.int32)
        if N * k >= 8:
            idx.reshape(-1)[g.choice(N * k, 3, replace=False)] = (-1, N, 2 ** 31 - 1)       # edges to nowhere
        ranges, edges = nr.reverse_graph(idx)
        lists = nr.reverse_brute(idx)
        for j in range(N):
            assert edges[ranges[j, 0]:ranges[j, 1]].tolist() == lists[j]
        assert sum(len(x) for x in lists) == int((ranges[:, 1] - ranges[:, 0]).sum())
        assert sorted(edges.tolist()) == list(range(N * k))


def test_refusals_come_before_a_device_is_touched():
    """This machine may have no GPU at all: a call that reached hipSetDevice would return TRASE_ERR_HIP (-4)."""
    from trase_amd import _lib
    lib = _lib.load()
    n = C.c_size_t()
    one = C.c_void_p(256)           # a non-null pointer that is never dereferenced
    big = 1 << 24
    assert lib.trase_knn_points(one, 1, one, 1, 0, one, one, one, 1 << 20, 0, None) == -1
    assert lib.trase_knn_points(one, 1, one, 1, 257, one, one, one, 1 << 20, 0, None) == -1
    assert b"1 <= K <= 256" in lib.trase_last_error()
    assert lib.trase_knn_points(one, 1, one, 1, 17, None, one, one, 1 << 20, 0, None) == -1
    assert lib.trase_knn_points(one, 1, one, 100, 129, one, one, one, 16, 0, None) == -3
    assert lib.trase_knn_points(one, 0, one, 100, 256, one, one, None, 0, 0, None) == 0            # nothing to do
    assert lib.trase_graph_reverse_ws_bytes(10, 5, None) == -1
    assert lib.trase_graph_reverse_ws_bytes(-1, 5, C.byref(n)) == -1 and lib.trase_graph_reverse_ws_bytes(10, 0, C.byref(n)) == -1
    assert lib.trase_graph_reverse_ws_bytes(big, 128, C.byref(n)) == -1 and b"2^31" in lib.trase_last_error()
    assert lib.trase_graph_reverse_ws_bytes(1000, 128, C.byref(n)) == 0 and n.value >= 1000 * 128 * 16
    assert lib.trase_graph_reverse(None, 10, 5, one, one, one, n.value, 0, None) == -1
    assert lib.trase_graph_reverse(one, 10, 5, one, one, one, 16, 0, None) == -3
    assert lib.trase_graph_reverse(one, 10, 5, one, one, None, n.value, 0, None) == -3
    assert lib.trase_graph_reverse(one, big, 128, one, one, one, n.value, 0, None) == -1
    assert lib.trase_feat3d_ws_bytes(10, 65, C.byref(n)) == -1 and lib.trase_feat3d_ws_bytes(10, 0, C.byref(n)) == -1
    assert lib.trase_feat3d_ws_bytes(1 << 26, 64, C.byref(n)) == -1 and lib.trase_feat3d_ws_bytes(10, 8, None) == -1
    assert lib.trase_feat3d_ws_bytes(300, 8, C.byref(n)) == 0 and n.value >= 8 * 10
    assert lib.trase_feat3d_forward(one, one, 300, 65, 5, one, one, one, one, n.value, 0, None) == -1
    assert lib.trase_feat3d_forward(one, one, 0, 8, 5, one, one, one, one, n.value, 0, None) == -1
    assert lib.trase_feat3d_forward(one, one, 300, 8, 5, one, None, one, one, n.value, 0, None) == -1
    assert lib.trase_feat3d_forward(one, one, 300, 8, 5, one, one, one, one, 8, 0, None) == -3
    assert lib.trase_feat3d_backward(one, one, one, one, one, 300, 8, 0, one, one, 0, None) == -1
    assert lib.trase_feat3d_backward(one, one, one, None, one, 300, 8, 5, one, one, 0, None) == -1
    assert lib.trase_edge_moments_forward(one, one, one, 10, 0, one, 0, None) == -1
    assert lib.trase_edge_moments_forward(one, None, one, 10, 4, one, 0, None) == -1
    assert lib.trase_edge_moments_backward(one, one, one, one, one, big, 128, one, one, one, 0, None) == -1
    assert lib.trase_edge_moments_backward(one, one, one, one, one, 10, 4, one, one, None, 0, None) == -1
    assert lib.trase_edge_residual_forward(one, one, one, None, 10, 4, one, 0, None) == -1
    assert lib.trase_edge_residual_forward(one, one, one, one, -1, 4, one, 0, None) == -1
    assert lib.trase_edge_residual_backward(one, one, one, one, one, one, 10, 4, one, one, one, None, 0, None) == -1
    assert lib.trase_edge_residual_backward(one, one, one, one, one, one, 10, 0, one, one, one, one, 0, None) == -1


def test_k_above_the_limit_is_refused_in_python():
    import torch
    from trase_amd.rasterizer import KNN_MAX_K, knn_points
    assert KNN_MAX_K == 256
    p = torch.zeros(1, 4, 3)
    for K in (257, 0, 1000):
        with pytest.raises(ValueError, match=r"knn_points: need 1 <= K <= 256 \(got %d\)" % K):
            knn_points(p, p, K=K)
    with pytest.raises(RuntimeError, match="GPU only"):
        knn_points(p, p, K=17)          # the limit itself is lifted: what refuses a CPU tensor is the device check
    import trase_amd.losses as losses
    import trase_amd.neighbors as nb
    assert losses.loss_reg_3d_feature is nb.loss_reg_3d_feature
    assert losses.loss_rigid_body_motion_reg_loss is nb.loss_rigid_body_motion_reg_loss


def test_dist2_lex_equals_the_kdtree():
    from scipy.spatial import cKDTree
    g = np.random.default_rng(4)
    p = g.normal(size=(1500, 3)) * [1.0, 0.3, 2.0]
    sums, f32 = nr.dist2_lex(p)
    d, _ = cKDTree(p).query(p, k=4)
    want = (d[:, 1:] ** 2).sum(axis=1)
    assert np.abs(sums - want).max() <= 1e-12 * want.max()
    assert f32.dtype == np.float32 and np.array_equal(f32, sums.astype(np.float32) / np.float32(3))
    # copies are other points (distance 0); fewer than 4 rows: what exists
    q = np.array([[0, 0, 0], [2, 0, 0], [0, 0, 0], [0, 1, 0]], dtype=np.float64)
    assert nr.dist2_lex(q)[0].tolist() == [1.0 + 4.0, 4.0 + 4.0 + 5.0, 1.0 + 4.0, 1.0 + 1.0 + 5.0]
    assert nr.dist2_lex(q[:3])[0].tolist() == [4.0, 8.0, 4.0] and nr.dist2_lex(q[:2])[0].tolist() == [4.0, 4.0]
    assert nr.dist2_lex(q[:1])[0].tolist() == [0.0] and nr.dist2_lex(q[:1])[1].tolist() == [0.0]


def test_axis_lines_and_their_cell_width():
    for axis in (0, 1, 2):
        c = nr.axis_line_cloud(24, axis, -4.0, 4.0, 1.0 / 256, 9, include=(4.0, 4.0 - 1.0 / 256))
        ext = c.max(axis=0) - c.min(axis=0)
        assert c.dtype == np.float32 and c.shape == (24, 3)
        assert ext[axis] == 8.0 and ext[(axis + 1) % 3] == 0.0 and ext[(axis + 2) % 3] == 0.0
        assert c[0, axis] == -4.0 and c[1, axis] == 4.0 and len(np.unique(c[:, axis])) == 24
        assert 0.0 in c[:, axis] and np.float32(-1.0 / 256) in c[:, axis]
        assert np.array_equal(c * 256, np.round(c * 256))
    assert nr.line_cell_width(32, 8.0) == 1.0 and nr.line_cell_width(32, 8.0).dtype == np.float32
    assert nr.line_cell_width(24, 8.0) == np.float32(32.0) / np.float32(24.0)
    assert nr.line_cell_width(1, 8.0, occ=1e-9) == np.float32(8.0) * np.float32(2.0 ** -20)        # the 2^20-cells floor


def test_face_lines_have_positions_on_the_wrong_side_of_a_face():
    """The premise of the cell-face cases: with 24 or 48 points on a line of extent 8 some positions of the 1/256 lattice get an
    fp32 cell that is not floor(x / h) (h = 4/3, 2/3 rounded up, 1/h rounded to 0.75, 1.5); with 32 points h = 1 and none does."""
    from tests.test_gpu_knn_narrow import FACE_LINE, FACE_NS, face_case, face_offsets
    step, lo, hi = FACE_LINE
    assert FACE_NS == (24, 32, 48)
    assert nr.line_face_disagreements(24, hi - lo, step)[0].tolist() == [4.0, 8.0]
    assert nr.line_face_disagreements(48, hi - lo, step)[0].tolist() == [2.0, 4.0, 6.0, 8.0]
    wrong, h = nr.line_face_disagreements(32, hi - lo, step)
    assert len(wrong) == 0 and h == 1.0
    for n in FACE_NS:
        near, wrong = face_offsets(n)
        for axis in (0, 1, 2):
            cloud, q = face_case(n, axis)
            assert len(cloud) == n and cloud[:, axis].max() - cloud[:, axis].min() == hi - lo
            assert set((wrong + lo).tolist()) <= set(cloud[:, axis].astype(np.float64).tolist())      # points ON those faces
            assert set((near + lo).tolist()) <= set(q[:, axis].astype(np.float64).tolist())
            both = np.concatenate([cloud, q]).astype(np.float64) / step
            assert np.array_equal(both, np.round(both))
            assert ((both.max(axis=0) - both.min(axis=0)) ** 2).sum() < 2 ** 24            # the largest squared distance


def test_narrow_lattices_keep_fp32_sums_exact():
    """distCUDA2 adds three squared distances in fp32: in units of step^2 the sum is an integer that must stay below 2^24, in
    every exact case of tests/test_gpu_knn_narrow.py (the squared distances themselves: the test below and the one above)."""
    from tests.test_gpu_knn_narrow import FACE_LINE, FACE_NS, dist2_cloud, dist2_plan, face_case
    clouds = [dist2_cloud(kind, n, grid) for kind, n, grid in dist2_plan()]
    clouds += [(face_case(n, axis)[0], FACE_LINE[0]) for n in FACE_NS for axis in (0, 1, 2)]
    for cloud, step in clouds:
        sums, f32 = nr.dist2_lex(cloud)
        units = sums / (step * step)
        assert np.array_equal(units, np.round(units)) and units.max() < 2 ** 24
        assert np.array_equal(sums.astype(np.float32).astype(np.float64), sums)


def test_grid_scenes_keep_fp32_distances_exact():
    """The premise of the exact k-NN tests: in units of the grid step every squared distance is an integer below 2^24, so
    fp32 holds every difference, product and partial sum exactly, in any order and with or without fused multiply-adds."""
    from tests.test_gpu_neighbors import GRIDS
    for step, lo, hi, reach in GRIDS:
        assert nr.max_grid_distance_units(lo, hi, step) < 2 ** 24
        assert nr.max_grid_distance_units(-reach, reach, step) < 2 ** 24            # the cross queries' larger box
        assert float(np.float32(step)) == step and (1.0 / step) == int(1.0 / step)
    step, lo, hi, reach = GRIDS[1]
    cloud = nr.grid_cloud("volume", 4000, step, lo, hi, 0)
    q = nr.grid_cloud("volume", 64, step, -reach, reach, 1)
    for a in (cloud[:256], q):
        d32, i32 = nr.knn_lex(a, cloud, 256, dtype=np.float32)
        d64, i64 = nr.knn_lex(a, cloud, 256, dtype=np.float64)
        assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), d64) and np.array_equal(i32, i64)
    d = cloud[:, None, :].astype(np.float32) - cloud[None, :512, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    e = cloud[:, None, :].astype(np.float64) - cloud[None, :512, :]
    assert np.array_equal(d2.astype(np.float64), (e * e).sum(-1))
