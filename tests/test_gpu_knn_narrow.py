"""The narrow k-NN (K <= 16: knn_points_kernel<KT>, KT in 1, 4, 8, 16) and distCUDA2 (knn_query_kernel) on the GPU, exactly, against
tests/neighbors_reference.py: every K with every cloud kind, clouds smaller than K or than the template width, 1 to 3 points,
duplicates, degenerate clouds, far queries, block edges and lattice points on cell faces.

Exact cases: on clouds whose coordinates are multiples of 1/4 in [-8, 8) or of 1/256 in [-4, 4] every difference, product and sum
of a squared distance is exact in fp32 in any order (tests/test_neighbors_reference.py asserts the premises, also that the sum
of the three distances of distCUDA2 is exact), so indices and distances must EQUAL numpy's (distance, index) selection and
distCUDA2 must equal float32(sum) / float32(3) bit for bit: the build has no fast-math and its division is correctly rounded.

Measured on an MI355X (this file's own output):
* exact cases: the 80 of the plan, the empty cloud, the copies, 9 face lines x 4 K x (self, cross), and for distCUDA2 50 clouds,
  9 face lines and the pinned small clouds: all bit-equal, canaries intact; the device's division is correctly rounded.
* the collinear cell width (K = 16 self query of 1000 collinear lattice points against the same cloud with one point moved off
  the line): with `c < h2` / `b < h1` in knn_params_kernel 114.7 ms against 0.255 ms on the 1/4 lattice and 33.4 ms against
  0.153 ms on the 1/256 lattice, ratios 450 and 218, results exact all the same; with `<=` 0.177 ms against 0.253 ms and
  0.172 ms against 0.165 ms, ratios 0.70 and 1.04.
* random clouds, 48 runs (2 kinds x 3 seeds x 4 K x self, cross): with knn_walk's distance all in fp32 (dx*dx + dy*dy + dz*dz
  of ROUNDED differences, which the bound 3 * 2^-24 does not allow for) the largest relative distance error was 2.12e-7 =
  3.56 * 2^-24 and 12 of the 24 tests missed the bound; with the float64 expression of the wide kernel, rounded once, it is
  5.95e-8 = 0.998 * 2^-24.  Near-tie rows: 0 or 1 of 2000 in every run (1 in 8 of the 48); rows whose indices differ: none."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import neighbors_reference as nr
from tests.test_gpu_neighbors import DEV, GRIDS, knn_raw, random_cloud

pytestmark = pytest.mark.gpu

KS = tuple(range(1, 17))
KINDS = ("volume", "plane", "line", "coincident", "blobs")
N2S = (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 255, 256, 257, 1000, 5000)
N1S = (1, 3, 255, 256, 257)
DIST2_NS = (1, 2, 3, 4, 5, 255, 256, 257, 1000, 4097)
FACE_NS = (24, 32, 48)                       # lattice positions on a cell face whose fp32 cell is not floor(x / h): 2, 0 and 4
FACE_KS = (1, 3, 4, 16)
FACE_LINE = (1.0 / 256, -4.0, 4.0)           # step, lo, hi: extent 8, so 32 points give h = 1 exactly


def kt_of(K):
    """The template width trase_knn_points launches for K."""
    return 1 if K <= 1 else 4 if K <= 4 else 8 if K <= 8 else 16


def narrow_plan():
    """Every K with every cloud kind once (80 cases) while the sizes, the two lattices and the query forms rotate:
    (K, kind, n2, n1 or None for a self query, lattice)."""
    plan = []
    for K in KS:
        for ci, kind in enumerate(KINDS):
            n2 = N2S[(K + ci + 11) % len(N2S)]
            cross = n2 == 5000 or (K + ci) % 3 == 0
            n1 = N1S[(K + 2 * ci) % len(N1S)] if cross else None
            plan.append((K, kind, n2, n1, (K + ci) % 2))
    return plan


def plan_ids(plan):
    return [f"K{K}-{kind}-n{n2}-" + (f"q{n1}" if n1 else "self") for K, kind, n2, n1, _ in plan]


def narrow_case(K, kind, n2, n1, grid):
    """-> (queries, cloud) of a case of the plan."""
    step, lo, hi, reach = GRIDS[grid]
    seed = 1000 * K + n2
    cloud = nr.grid_cloud(kind, n2, step, lo, hi, seed)
    if n1 is None:
        return cloud, cloud
    # cross queries: lattice points of a larger box, so some lie outside the cloud's bounding box; one far corner
    q = nr.grid_cloud("volume", n1, step, -reach, reach, seed + 1)
    q[0] = reach - step
    return q, cloud


def test_narrow_plan_meets_every_shape():
    cases = narrow_plan()
    assert len(cases) == len(KS) * len(KINDS)
    assert {(c[0], c[1]) for c in cases} == {(K, kind) for K in KS for kind in KINDS}
    assert {c[2] for c in cases} == set(N2S) and {c[3] for c in cases if c[3]} == set(N1S)
    assert any(c[3] is None and c[2] >= 1000 for c in cases)                  # a large self query
    assert any(c[2] < c[0] for c in cases)                                       # padding
    for KT in (4, 8, 16):
        # a list that never fills: the walk has no early exit and runs to the last shell
        assert any(kt_of(c[0]) == KT and c[0] <= c[2] < KT for c in cases), KT
        assert any(kt_of(K) == KT and K < KT for K in KS), KT                   # K strictly inside the template width
    for g in (0, 1):
        assert any(c[4] == g and c[3] for c in cases) and any(c[4] == g and c[3] is None for c in cases)


def lowest_copy(cloud):
    """For every row the lowest index among the rows at its position."""
    _, inv = np.unique(cloud, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    first = np.full(inv.max() + 1, len(cloud), dtype=np.int64)
    np.minimum.at(first, inv, np.arange(len(cloud)))
    return first[inv]


def assert_exact(q, cloud, K, self_query):
    dist, idx, intact = knn_raw(q, cloud, K)
    ref_d, ref_i = nr.knn_lex(q, cloud, K)
    assert intact, "a write behind the outputs"
    assert np.array_equal(idx, ref_i)
    assert np.array_equal(dist.view(np.int32), ref_d.astype(np.float32).view(np.int32))
    assert np.array_equal(dist.astype(np.float64), ref_d)
    n2 = len(cloud)
    if n2 < K:
        assert not idx[:, n2:].any() and not dist[:, n2:].view(np.int32).any()
    if self_query:
        assert np.array_equal(idx[:, 0], lowest_copy(cloud)) and not dist[:, 0].view(np.int32).any()


@pytest.mark.parametrize("K,kind,n2,n1,grid", narrow_plan(), ids=plan_ids(narrow_plan()))
def test_narrow_knn_exact(K, kind, n2, n1, grid):
    q, cloud = narrow_case(K, kind, n2, n1, grid)
    assert_exact(q, cloud, K, n1 is None)


def test_narrow_knn_empty_cloud():
    q = nr.grid_cloud("volume", 257, 0.25, -8.0, 8.0, 0)
    for K in (1, 3, 16):
        dist, idx, intact = knn_raw(q, np.zeros((0, 3), dtype=np.float32), K)
        assert intact and not idx.any() and not dist.view(np.int32).any()


def test_narrow_knn_duplicates_come_in_index_order():
    """Three copies of one point, in rows 5, 2 and 9 of a cloud of ten: a query at that point gets 2, 5, 9 first (distance 0), a
    K = 1 query ends on the first shell with the lowest of them, and a query elsewhere sees the copies as one tie."""
    cloud = nr.grid_cloud("volume", 10, 0.25, -8.0, 8.0, 77)
    cloud[5] = cloud[9] = cloud[2]
    q = np.stack([cloud[9], cloud[2] + np.float32(0.25), cloud[0]])
    for K in (1, 2, 3, 4, 5, 10, 12, 16):
        assert_exact(q, cloud, K, False)
        assert_exact(cloud, cloud, K, True)
    dist, idx, _ = knn_raw(q, cloud, 4)
    assert idx[0, :3].tolist() == [2, 5, 9] and not dist[0, :3].any()


# ---- lattice points on cell faces ------------------------------------------------------------------------------------------------
def face_offsets(n):
    """The offsets from the line's first point at which the fp32 cell index of a collinear cloud of n points steps up, each
    with its two lattice neighbours (inside the line), and among them those whose fp32 cell is not floor(x / h)."""
    step, lo, hi = FACE_LINE
    h = nr.line_cell_width(n, hi - lo)
    x = np.arange(int(round((hi - lo) / step)) + 1, dtype=np.float64) * step
    cell = (x.astype(np.float32) * (np.float32(1.0) / h)).astype(np.int64)
    faces = x[1:][np.diff(cell) > 0]
    near = np.unique(np.concatenate([faces - step, faces, faces + step]))
    return near[(near >= 0) & (near <= hi - lo)], nr.line_face_disagreements(n, hi - lo, step)[0]


def face_case(n, axis):
    """-> (cloud, cross queries): a collinear cloud with points on every cell face and next to it; queries on the faces, on
    the line's ends, beyond them (the clamped cell), and beside the line."""
    step, lo, hi = FACE_LINE
    near, wrong = face_offsets(n)
    assert set(wrong.tolist()) <= set(near.tolist())
    # as many faces as fit: every disagreeing one, then the others from the far end
    rest = [o for o in near.tolist()[::-1] if o not in set(wrong.tolist())]
    include = (wrong.tolist() + rest)[:n - 6]
    cloud = nr.axis_line_cloud(n, axis, lo, hi, step, 100 * n + axis, include=include)
    along = np.concatenate([near + lo, [lo, hi, lo - step, hi + step, lo - 1.0, hi + 1.0, hi + 0.5, lo - 0.5]])
    q = np.repeat(cloud[:1], len(along), axis=0)
    q[:, axis] = along.astype(np.float32)
    q[-2:, (axis + 1) % 3] += np.float32(step)            # two queries beside the line
    q[-1, (axis + 2) % 3] -= np.float32(3 * step)
    return cloud, q


@pytest.mark.parametrize("axis", (0, 1, 2))
@pytest.mark.parametrize("n", FACE_NS)
def test_narrow_knn_exact_on_cell_faces(n, axis):
    cloud, q = face_case(n, axis)
    for K in FACE_KS:
        assert_exact(cloud, cloud, K, True)
        assert_exact(q, cloud, K, False)


# ---- distCUDA2 ---------------------------------------------------------------------------------------------------------------
def dist2_raw(points, tail=64):
    """trase_knn_dist2 into a buffer with `tail` extra elements of 0xCD behind the output -> (out, canary intact)."""
    from trase_amd import _lib
    from trase_amd.rasterizer import _bytes, _stream
    lib = _lib.load()
    dev = torch.device(DEV, torch.cuda.current_device())
    a = torch.from_numpy(points).to(DEV).contiguous()
    n = len(points)
    out = torch.full((n + tail,), -0x32323233, dtype=torch.int32, device=DEV).view(torch.float32)
    nbytes = C.c_size_t()
    _lib.check(lib.trase_knn_sizes(n, C.byref(nbytes)), "trase_knn_sizes")
    ws = _bytes(nbytes.value, dev)
    _lib.check(lib.trase_knn_dist2(_lib.ptr(a), n, _lib.ptr(out), _lib.ptr(ws), ws.numel(), dev.index, _stream(dev)),
               "trase_knn_dist2")
    torch.cuda.synchronize()
    bits = out.view(torch.int32).cpu().numpy()
    return bits[:n].view(np.float32).copy(), bool((bits[n:] == -0x32323233).all())


def dist2_plan():
    """Every size with every cloud kind (50 cases), the lattice alternating: (kind, n, lattice).  Up to 5 points the coarse
    lattice only: three distances across the fine one can add up to more than 2^24 steps^2, and the fp32 sum would round."""
    return [(kind, n, (ni + ci) % 2 if n > 5 else 0) for ni, n in enumerate(DIST2_NS) for ci, kind in enumerate(KINDS)]


def dist2_cloud(kind, n, grid):
    step, lo, hi, _ = GRIDS[grid]
    return nr.grid_cloud(kind, n, step, lo, hi, 7000 + 10 * n + grid), step


def assert_dist2_exact(cloud):
    out, intact = dist2_raw(cloud)
    sums, want = nr.dist2_lex(cloud)
    assert intact, "a write behind the output"
    assert want.dtype == np.float32 and np.array_equal(out.view(np.int32), want.view(np.int32))
    return out, sums


@pytest.mark.parametrize("kind,n,grid", dist2_plan(), ids=[f"{k}-n{n}-g{g}" for k, n, g in dist2_plan()])
def test_dist2_exact(kind, n, grid):
    cloud, _ = dist2_cloud(kind, n, grid)
    out, _ = assert_dist2_exact(cloud)
    if kind == "coincident":
        assert not out.view(np.int32).any()


@pytest.mark.parametrize("axis", (0, 1, 2))
@pytest.mark.parametrize("n", FACE_NS)
def test_dist2_exact_on_cell_faces(n, axis):
    assert_dist2_exact(face_case(n, axis)[0])


def test_dist2_of_one_two_and_three_points_and_of_copies():
    """Fewer than 4 points: the sum of the distances that exist, divided by 3.  Copies count with distance 0."""
    third = np.float32(3)
    p = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0]], dtype=np.float32) + np.float32(0.25)
    out, _ = assert_dist2_exact(p[:1])
    assert out.tolist() == [0.0]
    out, _ = assert_dist2_exact(p[:2])
    assert out.tolist() == [np.float32(4) / third] * 2
    out, _ = assert_dist2_exact(p)
    assert out.tolist() == [np.float32(4 + 1) / third, np.float32(4 + 5) / third, np.float32(1 + 5) / third]
    # a point with two copies and one distinct neighbour: (0 + 0 + d) / 3; the neighbour sees three points at d
    out, _ = assert_dist2_exact(np.stack([p[0], p[1], p[0], p[0]]))
    assert out.tolist() == [np.float32(4) / third, np.float32(4), np.float32(4) / third, np.float32(4) / third]
    # with three copies the third distance is 0 as well
    out, _ = assert_dist2_exact(np.stack([p[0], p[1], p[0], p[0], p[2], p[0]]))
    assert out.tolist() == [0.0, 4.0, 0.0, 0.0, 1.0, 0.0]


# ---- clouds off the lattice ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 4, 7, 16))
@pytest.mark.parametrize("seed", (0, 1, 2))
@pytest.mark.parametrize("kind", ("volume", "plane"))
def test_narrow_knn_random_clouds(kind, seed, K):
    """Against float64 brute force.  The bar is that of three products and two sums of non-negative terms in fp32: within
    3 * 2^-24 of the float64 value, relatively (the kernel evaluates in float64 and rounds once; with fp32 differences, which
    round as well, it missed this bar).  Two float64 distances closer than twice that may come out in the other order: a row
    with such a pair among its first K + 1 is a near-tie, every other row's indices must be equal."""
    n = 2000
    cloud = random_cloud(kind, n, seed)
    cross = (random_cloud(kind, n, seed + 100) * np.float32(1.2)).astype(np.float32)        # partly outside the box
    c64 = cloud.astype(np.float64)
    for name, q in (("self", cloud), ("cross", cross)):
        dist, idx, intact = knn_raw(q, cloud, K)
        assert intact
        ref_d, ref_i = nr.knn_lex(q, cloud, K + 1)
        rd = ref_d[:, :K]
        d = dist.astype(np.float64)
        err = np.abs(d - rd) / np.maximum(rd, 1e-300)
        err[rd == 0] = d[rd == 0]
        near = (np.diff(ref_d, axis=1) < 6 * nr.U * ref_d[:, 1:]).any(axis=1)
        differs = (idx != ref_i[:, :K]).any(axis=1)
        print(f"{kind} seed {seed} K {K} {name}: largest relative distance error {err.max():.3e} (bound {3 * nr.U:.3e}); "
              f"near-tie rows {int(near.sum())} of {n}; rows whose indices differ {int(differs.sum())}")
        assert err.max() <= 3 * nr.U
        assert near.sum() <= 0.01 * n
        assert not differs[~near].any()
        # what was returned is what was measured: the float64 distance of every returned index, within the bound of the
        # returned distance; in a differing row these are the reference's distances as a multiset
        own = ((q.astype(np.float64)[:, None, :] - c64[idx]) ** 2).sum(-1)
        assert (np.abs(d - own) <= 3 * nr.U * own).all()
        assert (np.abs(np.sort(own[differs], axis=1) - rd[differs]) <= 3 * nr.U * rd[differs]).all()
        assert (np.sort(idx, axis=1)[:, 1:] != np.sort(idx, axis=1)[:, :-1]).all()
        if name == "self":
            assert np.array_equal(idx[:, 0], np.arange(n))


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_shims_batch_gather_and_input_forms():
    import pytorch3d.ops
    from simple_knn._C import distCUDA2
    a = nr.grid_cloud("volume", 300, 0.25, -8.0, 8.0, 1)
    b = random_cloud("plane", 300, 2)
    qa, qb = nr.grid_cloud("volume", 257, 0.25, -12.0, 12.0, 3), random_cloud("volume", 257, 4)
    p2 = torch.from_numpy(np.stack([a, b])).to(DEV)
    p1 = torch.from_numpy(np.stack([qa, qb])).to(DEV)
    for K in (1, 6, 16):
        both = pytorch3d.ops.knn_points(p1, p2, K=K, return_nn=True)
        assert both.idx.shape == (2, 257, K) and both.idx.dtype == torch.int64 and both.dists.dtype == torch.float32
        for i in range(2):
            one = pytorch3d.ops.knn_points(p1[i:i + 1], p2[i:i + 1], K=K)
            assert torch.equal(one.idx[0], both.idx[i])
            assert torch.equal(one.dists[0].view(torch.int32), both.dists[i].view(torch.int32))
            assert torch.equal(both.knn[i], p2[i][both.idx[i]])
        ref_d, ref_i = nr.knn_lex(qa, a, K)
        assert np.array_equal(both.idx[0].cpu().numpy(), ref_i)
        assert np.array_equal(both.dists[0].cpu().numpy().astype(np.float64), ref_d)
    # a float64, non-contiguous input that requires a gradient is read as its fp32 contiguous copy
    g = np.random.default_rng(5)
    wide = torch.from_numpy(g.uniform(-1, 1, (1000, 6))).to(DEV)
    x = wide[:, ::2].requires_grad_(True)
    assert x.dtype == torch.float64 and not x.is_contiguous()
    plain = x.detach().float().contiguous()
    got, want = distCUDA2(x), distCUDA2(plain)
    assert got.dtype == torch.float32 and not got.requires_grad and got.shape == (1000,)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    out, intact = dist2_raw(plain.cpu().numpy())
    assert intact and np.array_equal(want.cpu().numpy().view(np.int32), out.view(np.int32))


# ---- the cell width of a collinear cloud -----------------------------------------------------------------------------------------
def knn_time(cloud, K, reps=5):
    """Milliseconds of one trase_knn_points self query between two events on its stream: one warm-up, the median of `reps`."""
    from trase_amd import _lib
    from trase_amd.rasterizer import _bytes, _stream
    lib = _lib.load()
    dev = torch.device(DEV, torch.cuda.current_device())
    a = torch.from_numpy(cloud).to(DEV).contiguous()
    n = len(cloud)
    dist = torch.empty(n * K, dtype=torch.float32, device=DEV)
    idx = torch.empty(n * K, dtype=torch.int64, device=DEV)
    nbytes = C.c_size_t()
    _lib.check(lib.trase_knn_sizes(n, C.byref(nbytes)), "trase_knn_sizes")
    ws = _bytes(nbytes.value, dev)
    times = []
    for rep in range(reps + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _lib.check(lib.trase_knn_points(_lib.ptr(a), n, _lib.ptr(a), n, K, _lib.ptr(idx), _lib.ptr(dist), _lib.ptr(ws), ws.numel(),
                                        dev.index, _stream(dev)), "trase_knn_points")
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return float(np.median(times[1:]))


def collinear_pair(grid):
    """A collinear cloud of 1000 lattice points and the same cloud with one point moved one lattice step off the line in both
    other axes: that one has three non-zero extents and takes knn_params_kernel's ordinary branches."""
    step, lo, hi, _ = GRIDS[grid]
    line = nr.grid_cloud("line", 1000, step, lo, hi, 42 + grid)
    moved = line.copy()
    moved[0, 1:] += np.float32(step)
    return line, moved


@pytest.mark.parametrize("grid", (0, 1))
def test_collinear_cloud_costs_what_its_neighbour_costs(grid):
    """An exactly collinear cloud has two extents of 0; its cells must come from the one extent it has (h1), not from the
    2^20-cells floor under a cell width of 0, which makes every query walk thousands of empty shells.  The margin of 10 is
    generous on purpose: the two clouds differ legitimately by small factors, the defect by orders of magnitude."""
    line, moved = collinear_pair(grid)
    assert_exact(line, line, 16, True)
    assert_exact(moved, moved, 16, True)
    t_line, t_moved = knn_time(line, 16), knn_time(moved, 16)
    print(f"lattice {grid}: collinear {t_line:.4f} ms, one point off the line {t_moved:.4f} ms, ratio {t_line / t_moved:.2f}")
    assert t_line <= 10 * t_moved and t_moved <= 10 * t_line
