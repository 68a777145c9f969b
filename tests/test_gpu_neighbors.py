"""The wide k-NN (17 <= K <= 256), the transposed graph and the k-NN graph losses on the GPU, against tests/neighbors_reference.py.

Exact k-NN: on clouds whose coordinates are multiples of 1/4 in [-8, 8) or of 1/256 in [-4, 4) every difference, product and sum
of a squared distance is exact in fp32 in any evaluation order (tests/test_neighbors_reference.py asserts the premise), so
distances and indices must EQUAL the lexicographic (distance, index) selection of numpy.

Measured on an MI355X (this file's own output, kept in profiles/neighbors_bench.json under "tests"):
random clouds: largest relative distance error 5.96e-8 = 2^-24 in all 27 cases, 0 to 7 near-tie rows of 5000, no other row's
index set differing; feature loss and edge sums: at most 0.371 of a bound (the moments at N 65, k 128; the feature loss's
gradient at most 0.138); rigid loss: kernels 1.9e-12 to 2.0e-5 from float64
where the fp32 compositions are 2.1e-12 to 2.0e-5, gradients 2.6e-7 to 1.4e-4 against 2.4e-7 to 3.0e-4."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import neighbors_reference as nr

pytestmark = pytest.mark.gpu

DEV = "cuda"
KS = (17, 31, 32, 33, 64, 65, 128, 129, 255, 256)
KINDS = ("volume", "plane", "line", "coincident", "blobs")
N2S = (1, 16, 17, 18, 129, 130, 257, 1000, 5000)
N1S = (1, 3, 4, 5, 257)
GRIDS = ((0.25, -8.0, 8.0, 12.0), (1.0 / 256, -4.0, 4.0, 4.5))      # step, lo, hi, reach of the cross queries


def knn_raw(p1, p2, K, tail=64):
    """trase_knn_points into buffers with `tail` extra elements of 0xCD behind both outputs -> (dists, idx, canaries intact)."""
    from trase_amd import _lib
    from trase_amd.rasterizer import _bytes, _stream
    lib = _lib.load()
    a, b = torch.from_numpy(p1).to(DEV).contiguous(), torch.from_numpy(p2).to(DEV).contiguous()
    n1, n2 = len(p1), len(p2)
    dist = torch.full((n1 * K + tail,), -0x32323233, dtype=torch.int32, device=DEV).view(torch.float32)
    idx = torch.full((n1 * K + tail,), -0x3232323232323233, dtype=torch.int64, device=DEV)
    nbytes = C.c_size_t()
    _lib.check(lib.trase_knn_sizes(n2, C.byref(nbytes)), "trase_knn_sizes")
    ws = _bytes(nbytes.value, torch.device(DEV, torch.cuda.current_device()))
    _lib.check(lib.trase_knn_points(_lib.ptr(a), n1, _lib.ptr(b), n2, K, _lib.ptr(idx), _lib.ptr(dist), _lib.ptr(ws), ws.numel(),
                                    torch.cuda.current_device(), _stream(torch.device(DEV, torch.cuda.current_device()))),
               "trase_knn_points")
    torch.cuda.synchronize()
    d_bits = dist.view(torch.int32).cpu().numpy()
    i_np = idx.cpu().numpy()
    intact = bool((d_bits[n1 * K:] == -0x32323233).all() and (i_np[n1 * K:] == -0x3232323232323233).all())
    return d_bits[:n1 * K].view(np.float32).reshape(n1, K).copy(), i_np[:n1 * K].reshape(n1, K).copy(), intact


def exact_plan():
    """Every K with every cloud kind once (50 cases) while the sizes, the two grids and the query forms rotate."""
    plan = []
    for ki, K in enumerate(KS):
        for ci, kind in enumerate(KINDS):
            n2 = 200 if kind == "blobs" else N2S[(ki + 2 * ci) % len(N2S)]
            cross = n2 == 5000 or (ki + ci) % 3 == 0
            n1 = N1S[(ki + ci) % len(N1S)] if cross else None
            plan.append(pytest.param(K, kind, n2, n1, (ki + ci) % 2, id=f"K{K}-{kind}-n{n2}-" + (f"q{n1}" if cross else "self")))
    return plan


def test_exact_plan_meets_every_size():
    cases = [p.values for p in exact_plan()]
    assert {c[2] for c in cases} >= set(N2S) and {c[3] for c in cases if c[3]} == set(N1S)
    assert {(c[0], c[1]) for c in cases} == {(K, kind) for K in KS for kind in KINDS}
    assert any(c[3] is None and c[2] >= 1000 for c in cases) and any(c[2] < c[0] for c in cases)      # a large self query; padding


@pytest.mark.parametrize("K,kind,n2,n1,grid", exact_plan())
def test_wide_knn_exact(K, kind, n2, n1, grid):
    step, lo, hi, reach = GRIDS[grid]
    seed = 1000 * K + n2
    cloud = nr.grid_cloud(kind, n2, step, lo, hi, seed)
    if n1 is None:
        q = cloud
    else:       # cross queries: grid points of a larger box, so some lie outside the cloud's bounding box; one far corner
        q = nr.grid_cloud("volume", n1, step, -reach, reach, seed + 1)
        q[0] = reach - step
    dist, idx, intact = knn_raw(q, cloud, K)
    ref_d, ref_i = nr.knn_lex(q, cloud, K)
    assert intact, "a write behind the outputs"
    assert np.array_equal(idx, ref_i)
    assert np.array_equal(dist.astype(np.float64), ref_d)
    if n2 < K:
        assert not idx[:, n2:].any() and not dist[:, n2:].any()


def test_wide_knn_repeats_and_extends_the_narrow_kernel():
    cloud = nr.grid_cloud("volume", 1000, 0.25, -8.0, 8.0, 5)
    d17, i17, ok17 = knn_raw(cloud, cloud, 17)
    d17b, i17b, _ = knn_raw(cloud, cloud, 17)
    d16, i16, ok16 = knn_raw(cloud, cloud, 16)
    assert ok17 and ok16
    assert np.array_equal(d17.view(np.int32), d17b.view(np.int32)) and np.array_equal(i17, i17b)
    assert np.array_equal(i17[:, :16], i16) and np.array_equal(d17[:, :16].view(np.int32), d16.view(np.int32))


@pytest.mark.parametrize("K", (96, 97, 224, 225))
def test_wide_knn_list_size_steps(K):
    """The LDS list is 128 keys to K = 32, 256 to K = 96 and 512 beyond (KS has 32 | 33); from K = 225 the staging area is at its
    smallest.  A dense cloud, so that a shell brings several times the staging area."""
    cloud = nr.grid_cloud("volume", 3000, 0.25, -8.0, 8.0, K)
    dist, idx, intact = knn_raw(cloud[:300], cloud, K)
    ref_d, ref_i = nr.knn_lex(cloud[:300], cloud, K)
    assert intact and np.array_equal(idx, ref_i) and np.array_equal(dist.astype(np.float64), ref_d)


def test_wide_knn_through_the_shim_and_its_limit():
    import pytorch3d.ops
    cloud = nr.grid_cloud("volume", 300, 0.25, -8.0, 8.0, 6)
    p = torch.from_numpy(cloud).to(DEV)[None]
    out = pytorch3d.ops.knn_points(p, p, K=129)
    ref_d, ref_i = nr.knn_lex(cloud, cloud, 129)
    assert out.idx.dtype == torch.int64 and np.array_equal(out.idx[0].cpu().numpy(), ref_i)
    assert np.array_equal(out.dists[0].cpu().numpy().astype(np.float64), ref_d)
    with pytest.raises(ValueError, match="1 <= K <= 256"):
        pytorch3d.ops.knn_points(p, p, K=257)
    bad = cloud.copy()
    bad[0, 1] = np.nan
    bad[1, 0] = np.inf
    d, i, ok = knn_raw(bad[:2], cloud, 40)
    assert ok and not d.any() and not i.any()          # a non-finite query finds nothing


def random_cloud(kind, n, seed):
    g = np.random.default_rng(seed)
    if kind == "volume":
        p = g.uniform(-1, 1, (n, 3))
    elif kind == "plane":
        p = np.concatenate([g.uniform(-1, 1, (n, 2)), 0.01 * g.normal(size=(n, 1))], axis=1)
    else:
        p = g.normal(size=(n, 3)) * 0.1 + np.where(g.random((n, 1)) < 0.5, -2.0, 2.0)
    return p.astype(np.float32)


@pytest.mark.parametrize("K", (17, 129, 256))
@pytest.mark.parametrize("seed", (0, 1, 2))
@pytest.mark.parametrize("kind", ("volume", "plane", "blobs"))
def test_wide_knn_random_clouds(kind, seed, K):
    from scipy.spatial import cKDTree
    n = 5000
    cloud = random_cloud(kind, n, seed)
    dist, idx, intact = knn_raw(cloud, cloud, K)
    assert intact
    c64 = cloud.astype(np.float64)
    rd, ri = cKDTree(c64).query(c64, k=K + 1)
    rd2 = rd * rd
    assert (np.diff(dist, axis=1) >= 0).all()
    err = np.abs(dist.astype(np.float64) - rd2[:, :K]) / np.maximum(rd2[:, :K], 1e-300)
    err[rd2[:, :K] == 0] = np.abs(dist.astype(np.float64))[rd2[:, :K] == 0]
    print(f"{kind} seed {seed} K {K}: largest relative distance error {err.max():.3e} (bound {4 * nr.U:.3e})")
    assert err.max() <= 4 * nr.U
    near_tie = (rd2[:, K] - rd2[:, K - 1]) < 2.0 ** -20 * rd2[:, K]
    same = np.array([set(a) == set(b) for a, b in zip(idx.tolist(), ri[:, :K].tolist())])
    print(f"  rows with a near-tie at the K-th place: {int(near_tie.sum())}; rows whose index set differs: {int((~same).sum())}")
    assert near_tie.sum() <= 0.002 * n
    assert same[~near_tie].all()


# ---- the transposed graph -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 5, 128))
@pytest.mark.parametrize("N", (1, 63, 64, 65, 1025))
def test_reversal(N, k):
    from trase_amd.neighbors import NeighborGraph
    g = np.random.default_rng(N * 131 + k)
    idx = g.integers(0, N, size=(N, k)).astype(np.int32)
    if N * k >= 8:                                         # edges to nowhere: -1, N, a large id
        flat = idx.reshape(-1)
        flat[g.choice(N * k, 3, replace=False)] = (-1, N, 2 ** 31 - 1)
    graph = NeighborGraph.from_idx(torch.from_numpy(idx).to(DEV))
    ranges, edges = nr.reverse_graph(idx)
    got_r, got_e = graph.rev_ranges.cpu().numpy(), graph.rev_edges.cpu().numpy()
    valid = int(ranges[:, 1].max()) if N else 0
    assert np.array_equal(got_r, ranges)
    assert np.array_equal(got_e[:valid], edges[:valid])
    again = NeighborGraph.from_idx(torch.from_numpy(idx.astype(np.int64)).to(DEV))
    assert np.array_equal(again.rev_edges.cpu().numpy(), got_e) and np.array_equal(again.idx.cpu().numpy(), idx)


# ---- the feature loss and the two edge sums -------------------------------------------------------------------------------
# every N, every D and every k at least once; graphs from the GPU k-NN (N <= k: the padded rows point at row 0)
LOSS_CASES = [(1, 1, 1), (2, 3, 5), (63, 32, 16), (64, 64, 1), (65, 1, 128), (300, 32, 5), (1025, 64, 16), (1025, 3, 128),
              (300, 64, 128), (64, 3, 16)]


def cloud_and_graph(N, k, seed):
    from trase_amd.neighbors import NeighborGraph
    g = np.random.default_rng(seed)
    xyz = g.uniform(-1, 1, (N, 3)).astype(np.float32)
    graph = NeighborGraph.build(torch.from_numpy(xyz).to(DEV), k)
    idx = graph.idx.cpu().numpy()
    assert idx.shape == (N, k) and idx.dtype == np.int32
    return g, xyz, graph, idx


def report(name, got, ref, bound):
    """The largest error in units of its bound."""
    got, ref, bound = (np.asarray(x, dtype=np.float64) for x in (got, ref, bound))
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"  {name}: largest error {err.max() if err.size else 0.0:.3e}, {ratio:.3f} of its bound")
    return ratio


@pytest.mark.parametrize("N,D,k", LOSS_CASES)
def test_feature_loss(N, D, k):
    from trase_amd.losses import loss_reg_3d_feature
    g, xyz, graph, idx = cloud_and_graph(N, k, 17 * N + D + k)
    f = g.normal(0.0, 1.5, (N, D)).astype(np.float32)
    ref = nr.feat3d(f, idx, g_out=0.75)
    outs = []
    for _ in range(2):
        ft = torch.from_numpy(f).to(DEV).requires_grad_(True)
        keep = ft.detach().clone()
        loss = loss_reg_3d_feature(ft, torch.from_numpy(xyz).to(DEV), k, graph=graph)
        (0.75 * loss).backward()
        assert torch.equal(ft.detach(), keep)
        outs.append((loss.detach().cpu().numpy().copy(), ft.grad.cpu().numpy().copy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    print(f"feature loss N {N} D {D} k {k}: {float(outs[0][0]):.6f} (float64 {ref['loss']:.6f})")
    assert report("value", outs[0][0], ref["loss"], ref["loss_bound"]) <= 1.0
    assert report("gradient", outs[0][1], ref["grad"], ref["grad_bound"]) <= 1.0


def test_feature_loss_builds_its_own_graph_and_subsamples():
    from trase_amd.losses import loss_reg_3d_feature
    g = np.random.default_rng(3)
    xyz, f = g.uniform(-1, 1, (300, 3)).astype(np.float32), g.normal(size=(300, 8)).astype(np.float32)
    ft = torch.from_numpy(f).to(DEV).requires_grad_(True)
    loss = loss_reg_3d_feature(ft, torch.from_numpy(xyz).to(DEV), 5)
    idx = nr.knn_lex(xyz.astype(np.float64), xyz.astype(np.float64), 6)[1][:, 1:]
    ref = nr.feat3d(f, idx)
    assert abs(float(loss.detach()) - ref["loss"]) <= ref["loss_bound"]
    torch.manual_seed(11)
    sub = loss_reg_3d_feature(ft, torch.from_numpy(xyz).to(DEV), 5, max_points=100)
    torch.manual_seed(11)
    pick = torch.randperm(300)[:100].numpy()
    idx = nr.knn_lex(xyz[pick].astype(np.float64), xyz[pick].astype(np.float64), 6)[1][:, 1:]
    ref = nr.feat3d(f[pick], idx)
    assert abs(float(sub.detach()) - ref["loss"]) <= ref["loss_bound"]
    sub.backward()
    rows = np.zeros(300, dtype=bool)
    rows[pick] = True
    assert not ft.grad.cpu().numpy()[~rows].any()


def test_fixture_fp32_results_meet_the_bounds():
    """The reference's own fp32 run (CPU torch) against the same bounds, and the kernels on the fixture's case."""
    import os
    from trase_amd.losses import loss_reg_3d_feature
    from trase_amd.neighbors import NeighborGraph
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "neighbors.npz"))
    ref = nr.feat3d(fx["feat_feats"], fx["feat_idx_f64"])
    print("fixture, reference fp32:")
    assert report("value", fx["feat_loss_f32"], ref["loss"], ref["loss_bound"]) <= 1.0
    assert report("gradient", fx["feat_grad_f32"], ref["grad"], ref["grad_bound"]) <= 1.0
    ft = torch.from_numpy(fx["feat_feats"]).to(DEV).requires_grad_(True)
    graph = NeighborGraph.build(torch.from_numpy(fx["feat_xyz"]).to(DEV), 5)
    assert np.array_equal(graph.idx.cpu().numpy(), fx["feat_idx_f64"])
    loss = loss_reg_3d_feature(ft, torch.from_numpy(fx["feat_xyz"]).to(DEV), 5, graph=graph)
    loss.backward()
    print("fixture, kernels:")
    assert report("value", loss.detach().cpu().numpy(), fx["feat_loss_f64"], ref["loss_bound"]) <= 1.0
    assert report("gradient", ft.grad.cpu().numpy(), fx["feat_grad_f64"], ref["grad_bound"]) <= 1.0


@pytest.mark.parametrize("N,D,k", LOSS_CASES)
def test_edge_ops(N, D, k):
    from trase_amd.neighbors import edge_moments, edge_residual
    g, xyz, graph, idx = cloud_and_graph(N, k, 29 * N + k)
    p2 = (xyz @ np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]]) + 0.1 * g.normal(size=(N, 3))).astype(np.float32)
    gS = g.normal(size=(N, 3, 3)).astype(np.float32)
    R = np.linalg.qr(g.normal(size=(N, 3, 3)))[0].astype(np.float32)
    gr = g.normal(size=N).astype(np.float32)
    outs = []
    for _ in range(2):
        a = torch.from_numpy(xyz).to(DEV).requires_grad_(True)
        b = torch.from_numpy(p2).to(DEV).requires_grad_(True)
        S = edge_moments(a, b, graph)
        S.backward(torch.from_numpy(gS).to(DEV))
        m = [S.detach().cpu().numpy(), a.grad.cpu().numpy().copy(), b.grad.cpu().numpy().copy()]
        a.grad = b.grad = None
        Rt = torch.from_numpy(R).to(DEV).requires_grad_(True)
        r = edge_residual(a, b, graph, Rt)
        r.backward(torch.from_numpy(gr).to(DEV))
        m += [r.detach().cpu().numpy(), a.grad.cpu().numpy().copy(), b.grad.cpu().numpy().copy(), Rt.grad.cpu().numpy().copy()]
        assert np.array_equal(a.detach().cpu().numpy(), xyz) and np.array_equal(b.detach().cpu().numpy(), p2)
        outs.append(m)
    for x, y in zip(*outs):
        assert x.tobytes() == y.tobytes()
    S, g1, g2, r, h1, h2, hR = outs[0]
    print(f"edge ops N {N} k {k}")
    ref_S, b_S = nr.edge_moments(xyz, p2, idx)
    rg1, rg2, bg1, bg2 = nr.edge_moments_grad(xyz, p2, idx, gS)
    ref_r, b_r = nr.edge_residual(xyz, p2, idx, R)
    rr = nr.edge_residual_grad(xyz, p2, idx, R, gr)
    worst = max(report("moments", S, ref_S, b_S), report("moments, gradient to p1", g1, rg1, bg1),
                report("moments, gradient to p2", g2, rg2, bg2), report("residual", r, ref_r, b_r),
                report("residual, gradient to p1", h1, rr["g1"], rr["b1"]), report("residual, gradient to p2", h2, rr["g2"], rr["b2"]),
                report("residual, gradient to R", hR, rr["gR"], rr["bR"]))
    assert worst <= 1.0


# ---- the whole rigid loss -----------------------------------------------------------------------------------------------
# name -> (cluster sizes, cluster ids (with gaps), num_neighbors, exactly rigid motion)
RIGID_SCENES = {"rigid": ((129, 130, 400), (2, 5, 11), 128, True), "translation": ((129, 130, 400), (2, 5, 11), 128, True),
                "deformation": ((129, 130, 400), (2, 5, 11), 128, False), "reflection": ((129, 130, 400), (2, 5, 11), 128, False),
                "few_neighbors": ((6, 9), (1, 4), 4, False)}
FEW_NEIGHBORS_SEED = 0


def rigid_scene(name):
    """-> (xyz1, xyz2, cluster ids, num_neighbors, exactly rigid)."""
    sizes, ids, k, exact = RIGID_SCENES[name]
    g = np.random.default_rng(FEW_NEIGHBORS_SEED if name == "few_neighbors" else sum(map(ord, name)))
    n = sum(sizes)
    x1 = g.uniform(-1, 1, (n, 3)) * np.array([1.0, 0.6, 0.3])      # anisotropic clouds keep the singular values of S_i apart
    cid = g.permutation(np.concatenate([np.full(s, i) for s, i in zip(sizes, ids)]))
    c, s = np.cos(0.6), np.sin(0.6)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if name == "rigid":
        x2 = x1 @ rot.T + 0.25
    elif name == "translation":
        x2 = x1 + np.array([0.5, -0.25, 0.125])
    elif name in ("deformation", "few_neighbors"):
        x2 = x1 @ rot.T + 0.2 * g.normal(size=(n, 3))
    elif name == "reflection":
        x2 = x1 * np.array([1.0, 1.0, -1.0]) + 0.05 * g.normal(size=(n, 3))
    else:
        raise ValueError(name)
    return x1.astype(np.float32), x2.astype(np.float32), cid.astype(np.int64), k, exact


def torch_composition(x1, x2, cid, graphs):
    """The reference's statements in fp32 on the device, around the same neighbour indices."""
    a = torch.from_numpy(x1).to(DEV).requires_grad_(True)
    b = torch.from_numpy(x2).to(DEV).requires_grad_(True)
    ids = torch.from_numpy(cid).to(DEV)
    loss = 0
    uniq = torch.unique(ids)
    for pos, c in enumerate(uniq):
        p1, p2 = a[ids == c], b[ids == c]
        j = torch.from_numpy(graphs[pos].astype(np.int64)).to(DEV)
        e1, e2 = p1[:, None] - p1[j], p2[:, None] - p2[j]
        S = torch.bmm(e1.transpose(1, 2), e2)
        Um, _, V = torch.svd(S)
        Rm = torch.bmm(V, Um.transpose(1, 2))
        loss = loss + (e1 - torch.bmm(Rm, e2.transpose(1, 2)).transpose(1, 2)).pow(2).sum(2).sum(1).mean()
    loss = loss / len(uniq)
    loss.backward()
    return float(loss.detach()), a.grad.cpu().numpy(), b.grad.cpu().numpy()


def rigid_floors(x1, x2, cid, k, graphs, exact):
    """The bar's floors (loss, gradient to xyz1, gradient to xyz2): the edge sums' own derived bound on the float64 rotations,
    averaged like the loss.  For an exactly rigid motion loss and gradients vanish and what is left is the rounding of the
    fp32 rotation and of v = e1 - R e2 itself; the bound is then relative to the edges: (k + 3) u (sum |e1|^2 + sum |e2|^2) for
    the loss and, with 16u m for the error of a component of v (5 from its arithmetic, the rest for the fp32 rotation),
    16u * 2 sum over a row's outgoing and incoming edges of m (through |R|^T for xyz2) for the gradients."""
    uniq = np.unique(cid)
    f_loss, f_g1, f_g2 = 0.0, 0.0, 0.0
    for pos, c in enumerate(uniq):
        sel = cid == c
        n = int(sel.sum())
        S, _ = nr.edge_moments(x1[sel], x2[sel], graphs[pos])
        Um, _, Vt = np.linalg.svd(S)
        Rm = np.einsum("nab,nbc->nac", Vt.transpose(0, 2, 1), Um.transpose(0, 2, 1))
        f_loss += nr.edge_residual(x1[sel], x2[sel], graphs[pos], Rm)[1].mean() / len(uniq)
        if exact:
            w = np.full(n, 1.0 / (n * len(uniq)))
            rr = nr.edge_residual_grad(x1[sel], x2[sel], graphs[pos], Rm, w)
            # (b = (k + n_in + c) u a + 5 u m-sum, and the a-terms vanish with v: what remains is the 5 u m-sum)
            f_g1, f_g2 = max(f_g1, 16.0 / 5.0 * rr["b1"].max()), max(f_g2, 16.0 / 5.0 * rr["b2"].max())
    return f_loss, f_g1, f_g2


def rigid_check(x1, x2, cid, k, exact=False, fixture_fp32=None, fixture_idx=None):
    from trase_amd.losses import loss_rigid_body_motion_reg_loss
    from trase_amd.neighbors import NeighborGraph
    uniq = np.unique(cid)
    graphs = [NeighborGraph.build(torch.from_numpy(x1[cid == c]).to(DEV), k).idx.cpu().numpy() for c in uniq]
    if fixture_idx is not None:
        # the fixture's fp32 run counts towards the bar only on the same neighbours: every row the same set, and the same index
        # at every place but where two float64 distances round to one fp32 number -- there the kernel's key orders by index
        # (in rigid2 row 68 of the second cluster has one such pair); a row's order is only its order of summation
        assert len(graphs) == len(fixture_idx)
        for c, got, want in zip(uniq, graphs, fixture_idx):
            p = x1[cid == c].astype(np.float64)
            d32 = ((p[:, None] - p[None]) ** 2).sum(-1).astype(np.float32)
            assert np.array_equal(np.sort(got, axis=1), np.sort(want, axis=1))
            assert np.array_equal(np.take_along_axis(d32, got.astype(np.int64), 1), np.take_along_axis(d32, want.astype(np.int64), 1))
    ref = nr.rigid_loss(x1, x2, cid, k, idx_of=lambda pos, p1: graphs[pos])
    for sig in ref["sigma"]:           # the premise: distinct singular values keep the SVD's gradient well-conditioned
        gap = np.minimum(sig[:, 0] - sig[:, 1], sig[:, 1] - sig[:, 2]) / sig[:, 0]
        assert gap.min() >= 1e-2, f"singular values {gap.min():.2e} apart"
    a = torch.from_numpy(x1).to(DEV).requires_grad_(True)
    b = torch.from_numpy(x2).to(DEV).requires_grad_(True)
    loss = loss_rigid_body_motion_reg_loss(a, b, torch.from_numpy(cid).to(DEV), num_neighbors=k)
    loss.backward()
    got = (float(loss.detach()), a.grad.cpu().numpy(), b.grad.cpu().numpy())
    sides = [torch_composition(x1, x2, cid, graphs)] + ([fixture_fp32] if fixture_fp32 is not None else [])
    want = (ref["loss"], ref["g1"], ref["g2"])
    floors = list(rigid_floors(x1, x2, cid, k, graphs, exact))
    if exact:
        floors[0] = max(floors[0], (k + 3) * nr.U * ref["edge_scale"])
    worst = 0.0
    for i, name in enumerate(("loss", "gradient to xyz1", "gradient to xyz2")):
        measured = [float(np.abs(np.asarray(side[i], dtype=np.float64) - want[i]).max()) for side in sides]
        bar = max(4.0 * max(measured), floors[i])
        err = float(np.abs(np.asarray(got[i], dtype=np.float64) - want[i]).max())
        print(f"  {name}: kernels {err:.3e}; fp32 compositions {', '.join(f'{m:.3e}' for m in measured)}; floor {floors[i]:.3e}; "
              f"bar {bar:.3e}; scale {float(np.abs(want[i]).max()):.3e}; edge scale {ref['edge_scale']:.3e}")
        worst = max(worst, err / max(bar, 1e-300))
    return worst


@pytest.mark.parametrize("name", tuple(RIGID_SCENES))
def test_rigid_loss(name):
    x1, x2, cid, k, exact = rigid_scene(name)
    print(f"rigid loss, {name}")
    assert rigid_check(x1, x2, cid, k, exact=exact) <= 1.0


@pytest.mark.parametrize("name", ("rigid2", "rigid1"))
def test_rigid_loss_fixture(name):
    import os
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "neighbors.npz"))
    x1, x2, cid = fx[f"{name}_xyz1"], fx[f"{name}_xyz2"], fx[f"{name}_cluster_ids"]
    print(f"rigid loss, fixture {name}")
    fixture = (float(fx[f"{name}_loss_f32"]), fx[f"{name}_g1_f32"], fx[f"{name}_g2_f32"])
    idx = [fx[f"{name}_idx{c}_f64"] for c in range(len(np.unique(cid)))]
    assert rigid_check(x1, x2, cid, 128, fixture_fp32=fixture, fixture_idx=idx) <= 1.0


def test_rigid_loss_tiny_clusters():
    """Clusters of 1 and 2 points: every edge is padding or one vector and its reverse, the moment matrix has rank <= 1 and
    the rotation is not unique -- the reference's own value depends on its SVD's choice.  What holds for every choice (R is
    orthogonal): the single point adds 0; of the pair, one row has one edge of the pair's length and three to itself, the other
    four edges of that length, so the cluster adds at most (1 + 4) / 2 * (|d1| + |d2|)^2; the other clusters' share is unchanged."""
    from trase_amd.losses import loss_rigid_body_motion_reg_loss
    x1, x2, cid, _, _ = rigid_scene("deformation")
    g = np.random.default_rng(8)
    t1, t2 = g.uniform(-1, 1, (3, 3)).astype(np.float32), g.uniform(-1, 1, (3, 3)).astype(np.float32)
    y1, y2, cid2 = np.concatenate([x1, t1]), np.concatenate([x2, t2]), np.concatenate([cid, [0, 20, 20]])

    def run(a, b, c):
        return float(loss_rigid_body_motion_reg_loss(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV),
                                                     torch.from_numpy(c).to(DEV), num_neighbors=4))
    base, more = run(x1, x2, cid), run(y1, y2, cid2)
    # the 4-neighbour value of the three large clusters against float64 on the same neighbours.  The value is
    # sum |e1|^2 + sum |e2|^2 - 2 (sum of S_i's singular values), Lipschitz in S_i whether or not singular values are close, so
    # it needs no premise on them (the gradients do, and with 4 edges some of the 659 rows miss it: they are not compared here)
    from trase_amd.neighbors import NeighborGraph
    graphs = [NeighborGraph.build(torch.from_numpy(x1[cid == c]).to(DEV), 4).idx.cpu().numpy() for c in np.unique(cid)]
    ref = nr.rigid_loss(x1, x2, cid, 4, idx_of=lambda pos, p1: graphs[pos])["loss"]
    measured = abs(torch_composition(x1, x2, cid, graphs)[0] - ref)
    bar = max(4.0 * measured, rigid_floors(x1, x2, cid, 4, graphs, False)[0])
    print(f"three clusters, 4 neighbours: kernels {abs(base - ref):.3e} from float64; fp32 composition {measured:.3e}; bar {bar:.3e}")
    assert abs(base - ref) <= bar
    extra = 5.0 * more - 3.0 * base
    d1, d2 = np.linalg.norm(t1[1] - t1[2]), np.linalg.norm(t2[1] - t2[2])
    cap = 2.5 * (d1 + d2) ** 2
    print(f"tiny clusters add {extra:.6f} (at most {cap:.6f}); three clusters {base:.6f}, five {more:.6f}")
    assert np.isfinite(more) and -64 * nr.U * abs(base) <= extra <= cap * (1 + 64 * nr.U) + 64 * nr.U * abs(base)


def test_rigid_loss_nan_cluster():
    """Deviation 29: a cluster whose loss is NaN (here through one NaN coordinate at time 2) adds 0 and its rows get a zero
    gradient, as in the reference, which leaves such a cluster out of the sum; the other cluster's share and gradients are
    those of a run without the NaN cluster, halved by the cluster count (a power of two: the same bits)."""
    from trase_amd.losses import loss_rigid_body_motion_reg_loss
    g = np.random.default_rng(29)
    x1 = (g.uniform(-1, 1, (70, 3)) * np.array([1.0, 0.6, 0.3])).astype(np.float32)
    x2 = (x1 + 0.1 * g.normal(size=(70, 3))).astype(np.float32)
    cid = np.array([3] * 40 + [7] * 30, dtype=np.int64)
    x2[50, 1] = np.nan
    good = cid == 3

    def run(a, b, c):
        a, b = torch.from_numpy(a).to(DEV).requires_grad_(True), torch.from_numpy(b).to(DEV).requires_grad_(True)
        loss = loss_rigid_body_motion_reg_loss(a, b, torch.from_numpy(c).to(DEV), num_neighbors=8)
        loss.backward()
        return loss.detach().cpu().numpy(), a.grad.cpu().numpy(), b.grad.cpu().numpy()
    alone, a1, a2 = run(x1[good], x2[good], cid[good])
    both, g1, g2 = run(x1, x2, cid)
    assert np.isfinite(alone) and alone > 0 and a1.any() and a2.any()
    assert both == np.float32(0.5) * alone
    assert not g1[~good].any() and not g2[~good].any()          # zeros, not NaN
    assert np.array_equal(g1[good], np.float32(0.5) * a1) and np.array_equal(g2[good], np.float32(0.5) * a2)
