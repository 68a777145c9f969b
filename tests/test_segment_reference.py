"""CPU checks of the segmentation restatement (tests/segment_reference.py) and of the kmeans_pytorch shim's plumbing:
the float64 restatement reproduces the masks the reference's render.py computes (tests/golden/segment.npz, written by
tests/golden/make_segment.py), the re-seed hash gives its known values, and ``import kmeans_pytorch`` lands on this
repository's shim."""
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
