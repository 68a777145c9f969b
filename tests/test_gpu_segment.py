"""K-means and query masks on the GPU (trase_amd/segment.py, trase_amd/csrc/segment.hip) against the float64 restatement
of tests/segment_reference.py and the render.py fixture tests/golden/segment.npz."""
import os

import numpy as np
import pytest
import torch

from tests import segment_reference as sr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GAP = 2e-5              # squared-distance gap below which an assignment is a near tie (fp32 error measured <= 8e-7)
CENTRE_TOL = 2e-6
F16_ULP = 2.0 ** -11    # fp16 spacing in [0.5, 1)


def _dev():
    return torch.device("cuda", 0)


def _unit_rows(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g)
    return torch.nn.functional.normalize(x, dim=-1).to(_dev())


def _blobs(n, k, d, noise, seed, scale=None, distinct_at=None):
    g = np.random.default_rng(seed)
    centres = g.standard_normal((k, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    labels = g.integers(0, k, n)
    if distinct_at is not None:             # these rows (the start rows numpy will draw) lie in k distinct blobs
        labels[distinct_at] = np.arange(k)
    sig = noise if not callable(noise) else noise(g, n)
    rows = centres[labels] + sig * g.standard_normal((n, d))
    if scale is not None:
        rows *= g.uniform(scale[0], scale[1], (n, 1))
    return torch.from_numpy(rows.astype(np.float32)).to(_dev()), labels


def _state(dev):
    return torch.zeros(4, dtype=torch.int32, device=dev)


def _shift(state):
    return float(state[2:3].cpu().view(torch.float32)[0])


# ---- 1. lockstep at full size -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [16, 64])
def test_lloyd_steps_lockstep_with_float64(K):
    from trase_amd.segment import _kmeans_steps
    N, D, tol, key = 300_000, 32, 1e-4, 12345
    X = _unit_rows(N, D, seed=K)
    centres = X[torch.as_tensor(sr.init_indices(N, K, seed=7), device=X.device)].contiguous()
    ids = torch.zeros(N, dtype=torch.int32, device=X.device)
    state = _state(X.device)
    excluded_max = 0.0
    for it in range(20):
        before = centres.clone()
        _kmeans_steps(X, centres, ids, key, tol, 0, 1, state)
        st = state.cpu()
        assert int(st[0]) == it + 1
        o_ids, gap, _, _ = sr.lloyd_step(X, before, it, key)
        g_ids = ids.long()
        differ = g_ids != o_ids
        near = gap < GAP
        assert not bool((differ & ~near).any()), f"K={K} it={it}: {int((differ & ~near).sum())} ids differ away from a tie"
        excluded_max = max(excluded_max, float(near.double().mean()))
        c64, shift64 = sr.update(X, g_ids, before, it, key)
        err = float((centres.double() - c64).abs().max())
        assert err < CENTRE_TOL, f"K={K} it={it}: centres differ from float64 means of the GPU's ids by {err:.3e}"
        shift = _shift(st)
        assert abs(shift - shift64) <= 1e-4 * shift64 + 1e-5, (K, it, shift, shift64)
        if abs(shift64 ** 2 - tol) > 1e-2 * tol:
            assert bool(st[1]) == (shift64 ** 2 < tol), (K, it, shift64)
        state[1] = 0                        # keep stepping past convergence: the lockstep covers all 20 iterations
    print(f"K={K}: near-tie share excluded at most {100 * excluded_max:.4f} %")
    assert excluded_max < 1e-3


# ---- 2. end to end on separated blobs, through the kmeans_pytorch shim --------------------------------------------------

def test_kmeans_end_to_end_blobs_through_the_shim():
    from kmeans_pytorch import kmeans as shim_kmeans
    from trase_amd.segment import kmeans
    N, K, D = 300_000, 16, 32
    seed = 3
    X, labels = _blobs(N, K, D, 0.05, seed=3, distinct_at=sr.init_indices(N, K, seed))
    ids, centres = shim_kmeans(X, num_clusters=K, distance='euclidean', device=torch.device('cuda:0'), seed=seed,
                               tqdm_flag=False)
    assert ids.device.type == "cpu" and centres.device.type == "cpu"
    assert ids.dtype == torch.int64 and centres.dtype == torch.float32 and tuple(centres.shape) == (K, D)
    _, _, iters = kmeans(X, K, seed=seed)
    o_ids, o_c, o_iters = sr.kmeans_loop(X, sr.init_indices(N, K, seed), key=seed)
    assert torch.equal(ids, o_ids.cpu())
    assert iters == o_iters
    assert float((centres.double() - o_c.cpu()).abs().max()) < CENTRE_TOL
    # every blob recovered as one cluster
    assert len(set(zip(labels.tolist(), ids.tolist()))) == K


# ---- 3. reproducibility -----------------------------------------------------------------------------------------------

def test_kmeans_bitwise_reproducible_and_batch_independent(monkeypatch):
    from trase_amd import segment
    X = _unit_rows(100_000, 32, seed=5)
    runs = []
    for batch in (8, 8, 1):
        monkeypatch.setattr(segment, "_BATCH", batch)
        runs.append(segment.kmeans(X, 16, seed=11, iter_limit=40))
    for ids, c, it in runs[1:]:
        assert torch.equal(ids, runs[0][0]) and torch.equal(c, runs[0][1]) and it == runs[0][2]
    assert 1 < runs[0][2] <= 40


# ---- 4. empty cluster -------------------------------------------------------------------------------------------------

def test_empty_cluster_takes_the_hash_row():
    from trase_amd.segment import _kmeans_steps
    N, D, K, key = 5000, 32, 8, 0xDEADBEEF
    X = _unit_rows(N, D, seed=9)
    X[1] = X[0]                                    # centre 1 duplicates centre 0: it loses every point on the tie
    centres = X[:K].clone().contiguous()
    ids = torch.zeros(N, dtype=torch.int32, device=X.device)
    state = _state(X.device)
    before = centres.clone()
    _kmeans_steps(X, centres, ids, key, 0.0, 0, 1, state)
    assert not bool((ids == 1).any())
    row = sr.reseed_row(key, 0, 1, N)
    assert torch.equal(centres[1], X[row])
    c64, _ = sr.update(X, ids.long(), before, 0, key)
    assert torch.equal(c64[1], X[row].double())
    # the reseed index is the iteration: a second empty step draws row (key, 1, k)
    centres[1] = centres[0]
    _kmeans_steps(X, centres, ids, key, 0.0, 0, 1, state)
    if not bool((ids == 1).any()):
        assert torch.equal(centres[1], X[sr.reseed_row(key, 1, 1, N)])


# ---- 5. iter_limit: the returned ids are the pre-update assignment --------------------------------------------------------

def test_iter_limit_returns_the_last_assignment():
    from trase_amd.segment import _kmeans_steps, kmeans
    N, K = 200_000, 16
    X = _unit_rows(N, 32, seed=13)
    ids, centres, it = kmeans(X, K, iter_limit=3, tol=0.0, seed=21)
    assert it == 3
    # the same three steps one at a time: the centres the third step started from
    c = X[torch.as_tensor(sr.init_indices(N, K, 21), device=X.device)].contiguous()
    step_ids = torch.zeros(N, dtype=torch.int32, device=X.device)
    state = _state(X.device)
    for _ in range(2):
        _kmeans_steps(X, c, step_ids, 21, 0.0, 3, 1, state)
    c2 = c.clone()
    _kmeans_steps(X, c, step_ids, 21, 0.0, 3, 1, state)
    assert torch.equal(c, centres) and torch.equal(step_ids.long(), ids)
    _kmeans_steps(X, c, step_ids, 21, 0.0, 3, 1, state)             # done: frozen
    assert torch.equal(c, centres) and torch.equal(step_ids.long(), ids) and int(state[0]) == 3
    pre, gap = sr.assign(X, c2)                     # float64 assignment against the centres iteration 3 started from
    assert not bool(((ids != pre) & (gap >= GAP)).any())
    post, _ = sr.assign(X, centres)                 # against the RETURNED centres: not what is returned
    assert int((post != ids).sum()) > 0


# ---- 6. query masks ---------------------------------------------------------------------------------------------------

def _allowed(mask, ref_mask, score32, thr):
    bad = mask.cpu() != ref_mask.cpu()
    near = (score32.cpu() - float(np.float16(thr))).abs() <= F16_ULP
    return bad, near


def test_segment_mask_reproduces_the_render_py_fixture():
    from trase_amd.segment import segment_mask
    z = np.load(os.path.join(HERE, "golden", "segment.npz"))
    raw = torch.from_numpy(z["features"]).to(_dev())
    ids = torch.from_numpy(z["cluster_ids"]).to(_dev())          # float ids, as render.py holds them
    thr = float(z["threshold"])
    lists = [[int(i) for i in l if i >= 0] for l in z["id_lists"]] * int(z["frames"])
    normed = torch.nn.functional.normalize(raw, dim=-1)
    raw_copy, ids_copy = raw.clone(), ids.clone()
    first = True
    for n, segment_ids in enumerate(lists):
        if first:       # render.py normalises in place inside the first call: its first id saw the raw rows
            mask = segment_mask(raw, ids, segment_ids[:1], thr) | segment_mask(normed, ids, segment_ids[1:], thr)
            first = False
        else:
            mask = segment_mask(normed, ids, segment_ids, thr)
        assert mask.dtype == torch.bool and tuple(mask.shape) == (raw.shape[0],)
        ref = torch.from_numpy(z["masks"][n])
        _, s32 = sr.query_mask(normed, normed, ids, segment_ids[1:] if n == 0 else segment_ids, thr)
        if n == 0:
            _, s_first = sr.query_mask(normed, raw, ids, segment_ids[:1], thr)
            s32 = torch.where(torch.isnan(s_first), s32, s_first)
        bad, near = _allowed(mask, ref, s32, thr)
        assert not bool((bad & ~near).any()), f"frame list {n}: {int(bad.sum())} mask bits differ"
    assert torch.equal(raw, raw_copy) and torch.equal(ids, ids_copy)      # inputs untouched


@pytest.mark.parametrize("S", [1, 3, 8])
def test_segment_mask_full_size_against_float64(S):
    from trase_amd.segment import segment_mask
    N, K, D, thr = 300_000, 16, 32, 0.8
    X, labels = _blobs(N, K, D, lambda g, n: g.uniform(0.04, 0.3, (n, 1)), seed=20 + S, scale=(0.3, 3.0))
    ids = torch.from_numpy(labels).to(_dev())
    sel = list(range(0, 2 * S, 2))
    mask = segment_mask(X, ids, sel, thr)
    ref, s32 = sr.query_mask(X, X, ids, sel, thr)
    bad, near = _allowed(mask, ref, s32, thr)
    print(f"S={S}: {int(mask.sum())} selected, {int(bad.sum())} near-threshold mismatches")
    assert not bool((bad & ~near).any())
    assert int(ref.sum()) > 1000


def test_segment_mask_edge_cases():
    from trase_amd.segment import segment_mask
    N, K, D, thr = 20_000, 6, 32, 0.8
    X, labels = _blobs(N, K, D, lambda g, n: g.uniform(0.04, 0.3, (n, 1)), seed=31)
    ids = torch.from_numpy(labels).to(_dev()).to(torch.int32)
    members = torch.nonzero(ids == 2).flatten()
    X[members[:7]] = 0.0                             # zero rows of a selected cluster
    ids[:50] = -1                                    # noise points (HDBSCAN's -1)
    sel = [2, -1, 99, 4]                             # -1 never matches, 99 has no members
    mask = segment_mask(X, ids, sel, thr)
    ref, s32 = sr.query_mask(X, X, ids, sel, thr)
    bad, near = _allowed(mask, ref, s32, thr)
    assert not bool((bad & ~near).any())
    assert not bool(mask[members[:7]].any()) and not bool(mask[:50].any())
    assert not bool(mask[(ids != 2) & (ids != 4)].any())
    assert bool(mask[ids == 2].any()) and bool(mask[ids == 4].any())
    assert not bool(segment_mask(X, ids, [99], thr).any())
    assert not bool(segment_mask(X, ids, [], thr).any())


# ---- 7. into the renderer ---------------------------------------------------------------------------------------------

def test_mask_and_ids_into_the_renderer():
    from gaussian_renderer import render
    from trase_amd.segment import kmeans, segment_mask
    from trase_amd.synthetic import SynthGaussianModel, SynthPipe, make_scene, orbit_camera
    dev = _dev()
    n, K = 3000, 8
    scene = make_scene(n, feat_dim=32, seed=4, scale_mult=0.9).to(dev)
    feats, _ = _blobs(n, K, 32, lambda g, m: g.uniform(0.05, 0.25, (m, 1)), seed=41)
    pc = SynthGaussianModel(scene, requires_grad=False)
    pc._gaussian_features = feats.reshape(n, 1, 32)
    normed = torch.nn.functional.normalize(pc.get_gaussian_features.squeeze(1), dim=-1, p=2)
    ids, _, _ = kmeans(normed, K, seed=2)
    o_ids, _, _ = sr.kmeans_loop(normed, sr.init_indices(n, K, 2), key=2)
    assert torch.equal(ids, o_ids)
    sel = [1, 4]
    _, s32 = sr.query_mask(normed, normed, ids, sel, 0.8)
    # a threshold no score is within one fp16 ulp of, so the two masks must agree bit for bit
    cands = [float(v) for v in np.arange(0.6, 0.95, F16_ULP).astype(np.float16)]
    s = s32[~torch.isnan(s32)].cpu()
    thr = next(v for v in cands if not bool(((s - v).abs() <= F16_ULP).any()))
    mask = segment_mask(normed, ids, sel, thr)
    ref, _ = sr.query_mask(normed, normed, ids, sel, thr)
    assert torch.equal(mask.cpu(), ref.cpu()) and 0 < int(mask.sum()) < n
    cam = orbit_camera(160, 96, angle=0.3).to(dev)
    bg = torch.zeros(3, device=dev)
    ones = torch.ones(n, 3, device=dev)
    with torch.no_grad():
        a = render(cam, pc, SynthPipe(), bg, 0.0, 0.0, 0.0, mask=mask, override_color=ones)["render"]
        b = render(cam, pc, SynthPipe(), bg, 0.0, 0.0, 0.0, mask=ref.to(dev), override_color=ones)["render"]
        assert torch.equal(a, b) and float(a.sum()) > 0
        palette = torch.rand(K, 3, generator=torch.Generator().manual_seed(0)).to(dev)
        c = render(cam, pc, SynthPipe(), bg, 0.0, 0.0, 0.0, override_color=palette[ids])["render"]
        d = render(cam, pc, SynthPipe(), bg, 0.0, 0.0, 0.0, override_color=palette[o_ids.to(dev)])["render"]
        assert torch.equal(c, d) and float(c.sum()) > 0


# ---- 8. argument errors -----------------------------------------------------------------------------------------------

def test_argument_errors():
    from kmeans_pytorch import kmeans as shim_kmeans
    from trase_amd.segment import kmeans, segment_mask
    X = _unit_rows(100, 32, seed=1)
    with pytest.raises(ValueError, match="N >= K"):
        kmeans(X, 101)
    with pytest.raises(ValueError, match="K <= 128"):
        kmeans(_unit_rows(1000, 32, seed=1), 129)
    with pytest.raises(ValueError, match="D <= 64"):
        kmeans(_unit_rows(1000, 65, seed=1), 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        kmeans(X.cpu(), 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        segment_mask(X.cpu(), torch.zeros(100), [0])
    with pytest.raises(ValueError, match="S <= 128"):
        segment_mask(X, torch.zeros(100, device=X.device), list(range(129)))
    with pytest.raises(NotImplementedError):
        shim_kmeans(X, 8, distance='cosine', device=torch.device('cuda:0'))
    with pytest.raises(RuntimeError, match="GPU only"):
        shim_kmeans(X, 8, device=torch.device('cpu'))
