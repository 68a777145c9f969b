"""CPU checks of the segmentation restatement (tests/segment_reference.py) and of the kmeans_pytorch shim's plumbing:
the float64 restatement reproduces the masks the reference's render.py computes (tests/golden/segment.npz, written by
tests/golden/make_segment.py), the re-seed hash gives its known values, and ``import kmeans_pytorch`` lands on this
repository's shim.  For tests/test_gpu_segment_shapes.py: its shape plan meets every dispatch class of segment.hip, the
exact lattice step agrees with the float64 one, and the near ties of its real-valued cases stay under their cap."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests import segment_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "segment.npz")


def _fixture():
    z = np.load(GOLD)
    lists = [[int(i) for i in l if i >= 0] for l in z["id_lists"]] * int(z["frames"])
    return z, torch.from_numpy(z["features"]), torch.from_numpy(z["cluster_ids"]), lists, float(z["threshold"])


def test_restatement_reproduces_render_py_masks_bit_for_bit():
    z, f, ids, lists, thr = _fixture()
    masks = sr.render_frames(f, ids, lists, thr)
    assert len(masks) == len(z["masks"]) == 4
    for n, (m, ref) in enumerate(zip(masks, z["masks"])):
        assert np.array_equal(m.numpy(), ref), f"call list {n}: {int((m.numpy() != ref).sum())} bits differ"
        assert 0 < ref.sum() < ref.size


def test_fixture_holds_the_in_place_first_call_effect():
    """Scoring the first list against normalised features throughout gives a different mask: the first id's query
    came from the raw rows, and the restatement only matches because it reproduces that."""
    z, f, ids, lists, thr = _fixture()
    fn = f / f.norm(dim=-1, keepdim=True)
    m, _ = sr.query_mask(fn, fn, ids, lists[0], thr)
    assert not np.array_equal(m.numpy(), z["masks"][0])
    # later frames: every query from normalised rows
    m2, _ = sr.query_mask(fn, fn, ids, lists[2], thr)
    assert np.array_equal(m2.numpy(), z["masks"][2])


def test_restatement_scores_match_the_recorded_fp16_scores():
    z, f, ids, lists, thr = _fixture()
    fn = f / f.norm(dim=-1, keepdim=True)
    sid = lists[1][0]                      # a call whose query came from normalised rows
    _, s32 = sr.query_mask(fn, fn, ids, [sid], thr)
    pre = (ids == sid).numpy()
    rec = z["scores"][2][pre].astype(np.float64)       # call order: [2], [5], [0], [3], [7], ...
    ours = s32.numpy()[pre].astype(np.float32).astype(np.float16).astype(np.float64)
    assert np.mean(ours == rec) > 0.99 and np.abs(ours - rec).max() <= 2.0 ** -10


def test_fp16_threshold_rounding():
    assert float(np.float16(0.8)) == 0.7998046875
    assert float(torch.tensor(0.7998046875, dtype=torch.float16)) >= 0.7998046875


def test_reseed_hash_known_values():
    # SplitMix64 seeded with 0: its first outputs (the state advances by the golden-ratio increment)
    g = 0x9E3779B97F4A7C15
    assert [sr.splitmix64((i * g) & ((1 << 64) - 1)) for i in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4,
                                                                             0x06C45D188009454F]
    assert sr.reseed_row(0, 0, 0, 1 << 20) == 0xE220A8397B1DCDAF % (1 << 20)
    key = 0xDEADBEEF
    assert sr.reseed_row(key, 3, 5, 300_000) == sr.splitmix64(key ^ (3 << 32 | 5)) % 300_000
    assert sr.reseed_row(-1, 0, 0, 7) == sr.splitmix64((1 << 64) - 1) % 7


def test_restated_loop_on_blobs():
    g = np.random.default_rng(0)
    c = g.standard_normal((4, 8))
    lab = g.integers(0, 4, 2000)
    X = torch.from_numpy((c[lab] + 0.05 * g.standard_normal((2000, 8))).astype(np.float32))
    seed = next(s for s in range(100) if len(set(lab[sr.init_indices(2000, 4, s)])) == 4)
    ids, C, it = sr.kmeans_loop(X, sr.init_indices(2000, 4, seed), key=seed)
    assert it == 2 and len(set(zip(lab.tolist(), ids.tolist()))) == 4
    ids3, _, it3 = sr.kmeans_loop(X, sr.init_indices(2000, 4, seed), key=seed, tol=0.0, iter_limit=3)
    assert it3 == 3 and torch.equal(ids3, ids)


def test_kmeans_pytorch_resolves_to_the_shim():
    import kmeans_pytorch
    assert os.path.dirname(os.path.abspath(kmeans_pytorch.__file__)) == os.path.join(ROOT, "kmeans_pytorch")
    sig = inspect.signature(kmeans_pytorch.kmeans)
    assert list(sig.parameters) == ["X", "num_clusters", "distance", "cluster_centers", "tol", "tqdm_flag", "iter_limit",
                                    "device", "gamma_for_soft_dtw", "seed"]
    assert sig.parameters["distance"].default == "euclidean" and sig.parameters["tol"].default == 1e-4
    assert sig.parameters["iter_limit"].default == 0 and sig.parameters["seed"].default is None


def test_shim_rejects_what_it_does_not_provide():
    from kmeans_pytorch import kmeans
    X = torch.zeros(10, 4)
    with pytest.raises(NotImplementedError):
        kmeans(X, 2, distance="cosine", device=torch.device("cuda:0"))
    with pytest.raises(NotImplementedError):
        kmeans(X, 2, cluster_centers=torch.zeros(2, 4), device=torch.device("cuda:0"))
    with pytest.raises(RuntimeError, match="GPU only"):
        kmeans(X, 2, device=torch.device("cpu"))


def test_segment_entry_points_reject_cpu_tensors():
    from trase_amd.segment import kmeans, segment_mask
    with pytest.raises(RuntimeError, match="GPU only"):
        kmeans(torch.zeros(10, 4), 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        segment_mask(torch.zeros(10, 4), torch.zeros(10), [0])


# ---- the shape plan of tests/test_gpu_segment_shapes.py and the premises of its bars -----------------------------------------

# trase_amd/csrc/segment.hip, restated: seg_dpad, seg_blocks, the chunk of seg_launch_accum, seg_head_floats /
# seg_slab_floats / seg_wacc, and the tile walk of seg_assign_accum_kernel
def _dpad(D):
    return 8 if D <= 8 else 16 if D <= 16 else 32 if D <= 32 else 64


def _blocks(N):
    return min(max((N + 511) // 512, 1), 256)


def _chunk(N):
    return (N + _blocks(N) - 1) // _blocks(N)


def _wacc(K, D):
    return min((34816 - (K * _dpad(D) + K + 512)) // (K * (D + 1)), 8)


def _tile_rows(N):
    """The row counts of every tile any block walks."""
    out = set()
    for b in range(_blocks(N)):
        lo, hi = b * _chunk(N), min(N, (b + 1) * _chunk(N))
        out |= {min(512, hi - t0) for t0 in range(lo, hi, 512)}
    return out


def test_shape_plan_meets_every_class():
    plan = sr.SHAPE_PLAN
    assert len({c.id for c in plan}) == len(plan)
    assert all(1 <= c.K <= 128 and 1 <= c.D <= 64 and c.K <= c.N <= 200_000 for c in plan)
    assert {c.D for c in plan} >= {1, 3, 4, 8, 9, 12, 16, 17, 31, 32, 33, 36, 63, 64}
    assert {c.K for c in plan} >= {1, 2, 3, 127, 128}
    # every padded width below and at the padding, through the float4 loads and through the scalar ones
    # (a D that is a multiple of 4 loads by scalars only from an unaligned base: the offset cases, D = 4, 32 and 64)
    assert {c.D for c in plan if c.offset} >= {4, 32, 64} and all(c.D % 4 == 0 for c in plan if c.offset)
    paths = {(_dpad(c.D), c.D == _dpad(c.D), c.D % 4 == 0) for c in plan} | \
            {(_dpad(c.D), c.D == _dpad(c.D), False) for c in plan if c.offset}
    assert paths == {(dp, full, vec) for dp in (8, 16, 32, 64) for full in (False, True) for vec in (False, True)} - \
        {(8, True, False), (16, True, False)}
    # the waves that accumulate, with the table of the sub-range lengths
    assert [(_wacc(K, D), -(-512 // _wacc(K, D))) for K, D in ((128, 64), (96, 64), (80, 64), (72, 64), (64, 64), (128, 32), (3, 8))] == \
        [(3, 171), (4, 128), (5, 103), (6, 86), (7, 74), (7, 74), (8, 64)]
    assert {_wacc(c.K, c.D) for c in plan} == {3, 4, 5, 6, 7, 8}
    for w in (3, 5, 6, 7):
        per = -(-512 // w)
        tiles = set().union(*(_tile_rows(c.N) for c in plan if _wacc(c.K, c.D) == w))
        assert tiles >= {per - 1, per, per + 1, 1, 2, 3, 5, 512}, (w, sorted(tiles))
    # rows against the tile, blocks against the 16 runs of the reduction, blocks of more than one tile
    ns = {c.N for c in plan}
    assert ns >= {511, 512, 513, 1024, 1025, 16 * 512 + 1, 131072, 131073, 200_000}
    assert any(c.N == c.K == 1 for c in plan) and any(c.N == c.K == 128 for c in plan)
    assert {_blocks(n) for n in ns} >= {1, 2, 3, 16, 17, 256}
    assert _chunk(131072) == 512 and _chunk(131073) == 513 and _chunk(200_000) == 782
    assert _tile_rows(131073) == {512, 1, 258}                         # a second tile of one row; the last block is short
    assert {(c.K, c.D) for c in plan if c.N == 131073} >= {(5, 8), (128, 64)}
    # tie families and empty clusters in every padded width and at K = 128
    assert {_dpad(c.D) for c in plan if c.dup} == {8, 16, 32, 64} and any(c.dup and c.K == 128 for c in plan)
    for c in plan:
        if c.dup:
            _, _, empty, _ = sr.lattice_step(*sr.lattice_case(c), 0, 1)
            assert bool(empty[c.K - 1]) and (c.K < 4 or bool(empty[2]))


@pytest.mark.parametrize("K,D,N", [(4, 3, 300), (7, 17, 1000), (16, 64, 2000)])
def test_lattice_step_agrees_with_the_float64_step(K, D, N):
    X = sr.lattice_rows(N, D, seed=K)
    case = sr.ShapeCase(K, D, N, dup=K >= 7)
    C = sr.lattice_start(X, case)
    ids, new, empty, shift = sr.lattice_step(X, C, 2, 99)
    o_ids, gap, o_new, o_shift = sr.lloyd_step(X, C, 2, 99)
    assert torch.equal(ids, o_ids)                              # both take the first of equal minima
    assert not case.dup or bool((gap == 0).any())               # the duplicates tie exactly
    assert torch.equal(empty, torch.bincount(o_ids, minlength=K) == 0) and bool(empty.any()) == case.dup
    assert new.dtype == torch.float32 and torch.equal(new, o_new.float())     # the rounded float64 mean is the fp32 quotient here
    assert abs(shift - o_shift) <= 1e-6 * o_shift
    rows = sr.lattice_rows(50, 5, seed=0, span=2)
    assert rows.dtype == torch.float32 and float(rows.abs().max()) == 2 and torch.equal(rows, rows.round())
    assert torch.equal(rows, sr.lattice_rows(50, 5, seed=0, span=2))


@pytest.mark.parametrize("K,D,unit", sr.LOCKSTEP_CASES)
def test_near_ties_of_the_lockstep_cases_stay_under_the_cap(K, D, unit):
    """The rows a lockstep iteration may leave out: counted on the float64 gaps alone, for the seeds the GPU test uses."""
    X, start = sr.lockstep_rows(K, D, unit)
    bar = sr.near_tie_gap(X)
    assert bar == pytest.approx(8 * (D + 1) * 2.0 ** -24 * float(X.double().norm(dim=-1).max()) ** 2)
    if unit:
        assert bar == pytest.approx(8 * (D + 1) * 2.0 ** -24, rel=1e-5)
    C = X.double()[torch.from_numpy(start)]
    for it in range(sr.LOCKSTEP_ITERS):
        _, gap, C, _ = sr.lloyd_step(X, C, it, 12345)
        assert int((gap < bar).sum()) <= sr.near_tie_cap(sr.LOCKSTEP_N) == 5, (K, D, it, int((gap < bar).sum()))


@pytest.mark.parametrize("K,D,noise,seed", sr.BLOB_CASES)
def test_blob_cases_are_decided_away_from_every_bar(K, D, noise, seed):
    """The public kmeans() must reproduce ids and iteration count of the float64 loop on these: no assignment of the loop
    is a near tie and no stopping test is close."""
    X, labels, start = sr.blob_rows(sr.BLOB_N, K, D, noise, seed)
    assert len(set(labels[start].tolist())) == K
    bar, tol = sr.near_tie_gap(X), 1e-4
    C = X.double()[torch.from_numpy(start)]
    for it in range(50):
        ids, gap, C, shift = sr.lloyd_step(X, C, it, seed)
        assert float(gap.min()) > 10 * bar, (it, float(gap.min()), bar)
        assert abs(shift ** 2 - tol) > 0.5 * tol
        if shift ** 2 < tol:
            break
    assert 2 <= it + 1 < 50 and len(set(zip(labels.tolist(), ids.tolist()))) == K
