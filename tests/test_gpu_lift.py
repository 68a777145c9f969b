"""The prompt lift on the GPU (trase_amd.segment.lift_votes / prompt_clusters / pick, the lift kernels of
trase_amd/csrc/knn.hip) against the render.py fixture tests/golden/lift.npz and the float64 restatement of
tests/lift_reference.py.

The full-size bar is the reference's, not the kernel's: ``ref_bar`` is the largest Euclidean distance between the point the
reference's all-fp32 statements (fp32 ``torch.inverse``, fp32 products; restated below with torch on the CPU) give for a
prompted pixel and the float64 point.  A query displaced by at most ``bar`` sees every distance change by at most ``bar``,
so its nearest index cannot change while the float64 gap between second-nearest and nearest distance exceeds 2 * bar:
such a query is *decided* and must return the float64 index; any other must return a point at most 2 * bar farther than
the nearest.  Measured on one MI355X (1 % / 10 % / 100 % masks): reference bar 1.66e-4 / 1.76e-4 / 2.27e-4 (1.30e-4 ..
1.51e-4 with another CPU's LAPACK), our points 7.8e-8 / 9.6e-8 / 1.4e-7 from float64, undecided 1.4 / 1.9 / 2.2 % of the
prompt, no decided query with another index, every index equal to the float64 one."""
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import lift_reference as lr
from tests import segment_reference as sr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
UNDECIDED_MAX = 0.10        # condition on the scene, asserted: at most this share of a prompt may be undecided


def _dev():
    return torch.device("cuda", 0)


def _fixture():
    z = np.load(os.path.join(HERE, "golden", "lift.npz"))
    H, W = z["depth"].shape
    cam = types.SimpleNamespace(full_proj_transform=torch.from_numpy(z["full_proj_transform"]).to(_dev()), image_width=W,
                                image_height=H, znear=float(z["znear"]), zfar=float(z["zfar"]))
    t = {k: torch.from_numpy(z[k]).to(_dev()) for k in ("depth", "prompt_mask", "points", "cluster_ids")}
    return z, cam, t


def reference_points_fp32(depth, mask, cam):
    """render.py:213-220 restated with torch in fp32 on the CPU (the grid of generate_grid_index is int64)."""
    depth = depth.detach().cpu().float().reshape(cam.image_height, cam.image_width)
    mask = mask.detach().cpu().bool()
    rows, cols = torch.nonzero(mask, as_tuple=True)
    d = depth[mask]
    z = cam.zfar / (cam.zfar - cam.znear) * d - cam.zfar * cam.znear / (cam.zfar - cam.znear)
    uvz = torch.stack([((cols - 0.5) / cam.image_width * 2 - 1) * d, ((rows - 0.5) / cam.image_height * 2 - 1) * d, z, d], 1)
    return (uvz @ torch.inverse(cam.full_proj_transform.detach().cpu().float())[:, :3]).double().numpy()


def _check_against_float64(what, depth, mask, cam, points, index, pts, o):
    """The bars of the module docstring for one lift; -> the share of undecided queries."""
    m = mask.cpu().numpy().astype(bool)
    ref32 = reference_points_fp32(depth, mask, cam)
    ref_bar = float(np.linalg.norm(ref32 - o["points"], axis=1).max())
    ours = pts.cpu().numpy()[m].astype(np.float64)
    our_err = float(np.linalg.norm(ours - o["points"], axis=1).max())
    decided = (o["d2"] - o["d1"]) > 2 * ref_bar
    undecided_share = 1.0 - float(decided.mean())
    got = index.cpu().numpy()[m]
    assert bool((got >= 0).all())
    wrong = int((got[decided] != o["index"][decided]).sum())
    p64 = points.cpu().numpy().astype(np.float64)
    excess = np.linalg.norm(o["points"] - p64[got], axis=1) - o["d1"]
    print(f"{what}: {len(got)} queries; reference fp32 bar {ref_bar:.3e}, our points off by {our_err:.3e}; undecided "
          f"{100 * undecided_share:.2f} %; decided queries with another index: {wrong}; largest excess distance "
          f"{float(excess.max()):.3e}; indices equal to float64 overall {100 * float((got == o['index']).mean()):.4f} %")
    assert our_err <= ref_bar
    assert wrong == 0
    assert float(excess.max()) <= 2 * ref_bar
    return undecided_share


# ---- 1. the render.py fixture ----------------------------------------------------------------------------------------------

def test_fixture_votes_ids_and_index_map_exact():
    from trase_amd.segment import lift_votes, prompt_clusters
    z, cam, t = _fixture()
    before = {k: v.clone() for k, v in t.items()}
    votes, index = lift_votes(t["depth"], t["prompt_mask"], cam, t["points"], t["cluster_ids"], return_index=True)
    assert votes.dtype == torch.int64 and index.dtype == torch.int64 and tuple(index.shape) == tuple(z["depth"].shape)
    nref = len(z["ref_votes"])
    assert votes.numel() == int(z["cluster_ids"].max()) + 1          # sized as bincount over all ids would be
    assert np.array_equal(votes.cpu().numpy()[:nref], z["ref_votes"]) and not bool(votes[nref:].any())
    want = np.full(z["depth"].shape, -1, dtype=np.int64)
    want[z["prompt_mask"]] = z["ref_index"]
    assert np.array_equal(index.cpu().numpy(), want)
    ids = prompt_clusters(t["depth"].unsqueeze(0), t["prompt_mask"], cam, t["points"], t["cluster_ids"], int(z["threshold"]))
    assert ids.dtype == torch.int64 and ids.dim() == 1 and np.array_equal(ids.cpu().numpy(), z["ref_ids"])
    assert all(torch.equal(t[k], before[k]) for k in t)                # inputs untouched


# ---- 2, 3. full size against float64 ------------------------------------------------------------------------------------------

N_FULL, W_FULL, H_FULL, K_FULL = 300_000, 1920, 1080, 16


def _full_scene():
    """300k points uniform in a cube of half-width 3 seen from 3.2 away at 1080p (the undecided share grows with point density
    times depth, and the reference's fp32 bar differs by up to 2x between CPUs: this scene keeps the share near 4 %); the depth map is a smooth surface through the
    cloud's interior with a small zero-depth rectangle and scattered zero-depth pixels (0.5 % of the image)."""
    from trase_amd.synthetic import make_scene, orbit_camera
    cam = orbit_camera(W_FULL, H_FULL, angle=0.3, radius=3.2)
    g = np.random.default_rng(5)
    points = make_scene(N_FULL, feat_dim=1, seed=3, extent=3.0).xyz
    rr, cc = np.meshgrid(np.arange(H_FULL), np.arange(W_FULL), indexing="ij")
    depth = 2.6 + 0.7 * np.sin(cc / 310.0) * np.cos(rr / 190.0) + 0.2 * np.sin((rr + 2 * cc) / 77.0)
    depth[525:535, 960:1000] = 0.0
    depth.reshape(-1)[g.choice(depth.size, depth.size // 200, replace=False)] = 0.0
    ids = g.integers(0, K_FULL, N_FULL)
    return cam, torch.from_numpy(depth.astype(np.float32)), points, torch.from_numpy(ids), (rr, cc)


def _blob(rr, cc, share):
    """An elliptical prompt covering about `share` of the image, centred on the zero-depth rectangle."""
    if share >= 1.0:
        return np.ones(rr.shape, dtype=bool)
    a = math.sqrt(share * W_FULL * H_FULL / math.pi * 16 / 9)
    return ((cc - 980.0) / a) ** 2 + ((rr - 530.0) / (a * 9 / 16)) ** 2 <= 1.0


_full_cache = {}


def _full(share):
    if "scene" not in _full_cache:
        _full_cache["scene"] = _full_scene()
    if share not in _full_cache:
        from trase_amd.segment import lift_votes
        cam, depth, points, ids, (rr, cc) = _full_cache["scene"]
        mask = torch.from_numpy(_blob(rr, cc, share))
        dev = _dev()
        out = lift_votes(depth.to(dev), mask.to(dev), cam, points.to(dev), ids.to(dev), num_clusters=K_FULL, return_index=True,
                         return_points=True)
        _full_cache[share] = (mask, out, lr.lift(depth, mask, cam, points, ids, bins=K_FULL))
    return _full_cache["scene"], _full_cache[share]


@pytest.mark.parametrize("share", [0.01, 0.10, 1.0])
def test_full_size_against_float64(share):
    """The bars of the module docstring at 300k points and 1080p; the figures are printed before they are asserted."""
    (cam, depth, points, ids, _), (mask, (votes, index, pts), o) = _full(share)
    m = mask.numpy()
    assert abs(m.mean() - share) < 0.1 * share and int((depth.numpy()[m] == 0).sum()) > 400
    undecided_share = _check_against_float64(f"share {share}", depth, mask, cam, points, index, pts, o)
    assert undecided_share <= UNDECIDED_MAX
    assert bool((index.cpu().numpy()[~m] == -1).all())
    assert not bool(pts.cpu()[~mask].any())


@pytest.mark.parametrize("share", [0.01, 0.10, 1.0])
def test_votes_are_the_bincount_of_the_index_map(share):
    (_, _, _, ids, _), (mask, (votes, index, _), _) = _full(share)
    want = torch.bincount(ids[index.cpu()[mask]], minlength=K_FULL)
    assert torch.equal(votes.cpu(), want) and int(votes.sum()) == int(mask.sum())


# ---- 4. clicks --------------------------------------------------------------------------------------------------------------

def test_pick_equals_the_mask_form_and_the_click_path():
    from trase_amd.segment import pick
    (cam, depth, points, _, _), (mask, (_, index, pts), o) = _full(0.10)
    dev = _dev()
    rows, cols = o["rows"], o["cols"]
    sel = np.random.default_rng(2).choice(len(rows), 5000, replace=False)
    pixels = torch.from_numpy(np.stack([cols[sel], rows[sel]], 1))
    got, got_pts = pick(depth.to(dev), pixels.to(dev), cam, points.to(dev), return_points=True)
    assert got.dtype == torch.int64 and tuple(got.shape) == (5000,)
    assert torch.equal(got.cpu(), index.cpu()[rows[sel], cols[sel]])
    assert torch.equal(got_pts.cpu(), pts.cpu()[rows[sel], cols[sel]])
    # one click at a time, given on the host, against gui.py:786-797 in fp32 on the CPU
    inv32 = torch.inverse(cam.full_proj_transform.float())
    ref32 = reference_points_fp32(depth, mask, cam)
    bar = float(np.linalg.norm(ref32 - o["points"], axis=1).max())
    decided_clicks = 0
    for s in sel[:12]:
        pw, ph = int(cols[s]), int(rows[s])
        d = depth[ph, pw]
        z = cam.zfar / (cam.zfar - cam.znear) * d - cam.zfar * cam.znear / (cam.zfar - cam.znear)
        uvz = torch.stack([((pw - .5) / W_FULL * 2 - 1) * d, ((ph - .5) / H_FULL * 2 - 1) * d, z, d]).float().view(1, 4)
        p3d = (uvz @ inv32)[0, :3]
        want = int((p3d - points).norm(dim=-1).argmin())
        one = pick(depth.to(dev), (pw, ph), cam, points.to(dev))
        assert tuple(one.shape) == (1,) and int(one[0]) == int(index[ph, pw])
        if o["d2"][s] - o["d1"][s] > 2 * bar:
            decided_clicks += 1
            assert int(one[0]) == want
    assert decided_clicks >= 6


# ---- 5. reproducibility --------------------------------------------------------------------------------------------------------

def test_two_runs_bit_identical():
    from trase_amd.segment import lift_votes
    (cam, depth, points, ids, _), (mask, first, _) = _full(0.10)
    dev = _dev()
    again = lift_votes(depth.to(dev), mask.to(dev), cam, points.to(dev), ids.to(dev), num_clusters=K_FULL, return_index=True,
                       return_points=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


# ---- 6. id types, sizes, edge cases, argument errors ---------------------------------------------------------------------------

def test_cluster_id_types_and_bin_count():
    from trase_amd.segment import lift_votes, prompt_clusters
    z, cam, t = _fixture()
    base, index = lift_votes(t["depth"], t["prompt_mask"], cam, t["points"], t["cluster_ids"], return_index=True)
    for dtype in (torch.float32, torch.float64, torch.int32, torch.int64):
        assert torch.equal(lift_votes(t["depth"], t["prompt_mask"], cam, t["points"], t["cluster_ids"].to(dtype)), base)
    wide = lift_votes(t["depth"], t["prompt_mask"], cam, t["points"], t["cluster_ids"], num_clusters=64)
    assert wide.numel() == 64 and torch.equal(wide[:base.numel()], base) and not bool(wide[base.numel():].any())
    narrow = lift_votes(t["depth"], t["prompt_mask"], cam, t["points"], t["cluster_ids"], num_clusters=3)
    assert torch.equal(narrow, base[:3])                          # ids at or above num_clusters cast no vote
    # negative ids (HDBSCAN noise) cast no vote and do not disturb the others
    noisy = t["cluster_ids"].clone()
    noisy[noisy == 5] = -1
    v = lift_votes(t["depth"], t["prompt_mask"], cam, t["points"], noisy)
    assert int(base[5]) > 0 and v.numel() == base.numel() and torch.equal(v[:5], base[:5]) and int(v[5:].sum()) == 0
    v2, index2 = lift_votes(t["depth"], t["prompt_mask"], cam, t["points"], noisy.long(), num_clusters=7, return_index=True)
    assert torch.equal(v2[:5], base[:5]) and int(v2[5:].sum()) == 0 and torch.equal(index2, index)
    all_noise = torch.full_like(noisy, -1)
    assert lift_votes(t["depth"], t["prompt_mask"], cam, t["points"], all_noise).tolist() == [0]
    assert prompt_clusters(t["depth"], t["prompt_mask"], cam, t["points"], all_noise, 0).numel() == 0


def test_empty_prompts_zero_depth_and_points_outside_the_cloud():
    from trase_amd.segment import lift_votes, pick
    z, cam, t = _fixture()
    H, W = z["depth"].shape
    nb = int(z["cluster_ids"].max()) + 1
    empty = torch.zeros_like(t["prompt_mask"])
    votes, index = lift_votes(t["depth"], empty, cam, t["points"], t["cluster_ids"], return_index=True)
    assert votes.tolist() == [0] * nb and bool((index == -1).all())
    assert pick(t["depth"], torch.zeros(0, 2, dtype=torch.int32, device=_dev()), cam, t["points"]).numel() == 0
    assert pick(t["depth"], [], cam, t["points"]).numel() == 0
    none = torch.zeros(0, 3, device=_dev())
    votes, index = lift_votes(t["depth"], t["prompt_mask"], cam, none, torch.zeros(0, device=_dev()), num_clusters=nb,
                              return_index=True)
    assert votes.tolist() == [0] * nb and bool((index == -1).all())
    assert lift_votes(t["depth"], t["prompt_mask"], cam, none, torch.zeros(0, device=_dev())).tolist() == [0]
    # depth 0 everywhere: every pixel un-projects to one point and votes for its nearest
    zero = torch.zeros_like(t["depth"])
    o = lr.lift(zero, z["prompt_mask"], cam, z["points"], z["cluster_ids"])
    votes, index = lift_votes(zero, t["prompt_mask"], cam, t["points"], t["cluster_ids"], return_index=True)
    assert np.array_equal(votes.cpu().numpy(), o["votes"]) and int(votes.max()) == int(z["prompt_mask"].sum())
    assert np.array_equal(index.cpu().numpy(), lr.index_map(o, H, W))
    # prompts whose points fall far outside the cloud's bounding box: the whole image at five times the depth, and a cloud
    # shrunk into a corner; a pixel of the device list outside the image finds nothing
    full = torch.ones_like(t["prompt_mask"])
    for depth, pts in ((t["depth"] * 5, t["points"]), (t["depth"], t["points"] * 0.01 + 3.0)):
        o = lr.lift(depth, full, cam, pts, z["cluster_ids"])
        votes, index, out_pts = lift_votes(depth, full, cam, pts, t["cluster_ids"], return_index=True, return_points=True)
        _check_against_float64("outside the cloud", depth, full, cam, pts, index, out_pts, o)
        assert int(votes.sum()) == H * W
    px = torch.tensor([[3, 4], [W, 4], [3, -1], [W - 1, H - 1]], dtype=torch.int32, device=_dev())
    got = pick(t["depth"], px, cam, t["points"])
    assert int(got[1]) == -1 and int(got[2]) == -1 and int(got[0]) >= 0 and int(got[3]) >= 0


def test_argument_errors():
    from trase_amd.segment import lift_votes, pick, prompt_clusters
    z, cam, t = _fixture()
    H, W = z["depth"].shape
    with pytest.raises(RuntimeError, match="GPU only"):
        lift_votes(t["depth"].cpu(), t["prompt_mask"], cam, t["points"], t["cluster_ids"])
    with pytest.raises(RuntimeError, match="GPU only"):
        lift_votes(t["depth"], t["prompt_mask"], cam, t["points"].cpu(), t["cluster_ids"])
    with pytest.raises(RuntimeError, match="GPU only"):
        lift_votes(t["depth"], t["prompt_mask"].cpu(), cam, t["points"], t["cluster_ids"])
    with pytest.raises(RuntimeError, match="GPU only"):
        pick(t["depth"].cpu(), [(1, 1)], cam, t["points"])
    with pytest.raises(ValueError, match="depth must be"):
        lift_votes(t["depth"][:-1], t["prompt_mask"], cam, t["points"], t["cluster_ids"])
    with pytest.raises(ValueError, match="prompt_mask must be"):
        lift_votes(t["depth"], t["prompt_mask"][:, :-1], cam, t["points"], t["cluster_ids"])
    with pytest.raises(ValueError, match=r"points must be \(N, 3\)"):
        lift_votes(t["depth"], t["prompt_mask"], cam, t["points"][:, :2], t["cluster_ids"])
    with pytest.raises(ValueError, match="cluster ids for"):
        lift_votes(t["depth"], t["prompt_mask"], cam, t["points"], t["cluster_ids"][:-1])
    with pytest.raises(ValueError, match="bins <= 4096"):
        lift_votes(t["depth"], t["prompt_mask"], cam, t["points"], t["cluster_ids"], num_clusters=4097)
    big = t["cluster_ids"].clone()
    big[0] = 4096                                     # inferred bins: an id at the limit is an error, not dropped
    with pytest.raises(ValueError, match="bins <= 4096"):
        prompt_clusters(t["depth"], t["prompt_mask"], cam, t["points"], big, 0)
    with pytest.raises(ValueError, match="outside the"):
        pick(t["depth"], [(W, 0)], cam, t["points"])
    with pytest.raises(ValueError, match=r"\(M, 2\)"):
        pick(t["depth"], torch.zeros(4, 3, dtype=torch.int32, device=_dev()), cam, t["points"])


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------

IOU_BAR = 0.9       # the float64 pipeline reaches 1.0 on this scene (asserted >= 0.97 below): two separated objects


def _iou(a, b):
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    return float((a & b).sum()) / float((a | b).sum())


def test_prompt_in_mask_out_selects_the_prompted_object():
    from gaussian_renderer import render
    from trase_amd.segment import kmeans, prompt_clusters, segment_mask
    from trase_amd.synthetic import SynthGaussianModel, SynthPipe, make_scene, orbit_camera
    dev = _dev()
    n, K, W, H = 3000, 2, 160, 96
    g = np.random.default_rng(8)
    scene = make_scene(n, feat_dim=32, seed=6, scale_mult=0.9)
    is_a = np.arange(n) < n // 2
    centre = np.where(is_a[:, None], [[-0.8, 0.0, 0.0]], [[0.8, 0.0, 0.0]])
    xyz = centre + 0.45 * g.uniform(-1, 1, (n, 3))
    dirs = g.standard_normal((2, 32))
    feats = dirs[(~is_a).astype(int)] + 0.05 * g.standard_normal((n, 32))
    scene.xyz = torch.from_numpy(xyz.astype(np.float32))
    scene.gaussian_features = torch.from_numpy(feats.astype(np.float32)).reshape(n, 1, 32)
    scene.opacity = torch.full((n, 1), 4.0)
    scene = scene.to(dev)
    pc = SynthGaussianModel(scene, requires_grad=False)
    cam = orbit_camera(W, H, angle=0.0).to(dev)
    normed = torch.nn.functional.normalize(pc.get_gaussian_features.squeeze(1), dim=-1, p=2)
    ids, _, _ = kmeans(normed, K, seed=1)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        out = render(cam, pc, SynthPipe(), bg, 0.0, 0.0, 0.0)
    depth = out["depth"]
    # the prompt: every covered pixel on object A's side of the image
    ca = torch.tensor([[-0.8, 0.0, 0.0, 1.0]], device=dev) @ cam.full_proj_transform
    a_left = float(ca[0, 0] / ca[0, 3]) < 0
    cols = torch.arange(W, device=dev)[None, :].expand(H, W)
    prompt = (depth.reshape(H, W) > 0) & ((cols < W // 2) if a_left else (cols >= W // 2))
    threshold = int(prompt.sum()) // 10
    assert threshold > 20
    chosen = prompt_clusters(depth, prompt, cam, pc.get_xyz, ids, threshold)
    mask = segment_mask(normed, ids, chosen, 0.8)
    iou = _iou(mask.cpu().numpy(), is_a)
    # the same chain in float64 on the CPU, from the same rendered depth
    o_ids, _, _ = sr.kmeans_loop(normed.cpu(), sr.init_indices(n, K, 1), key=1)
    o = lr.lift(depth.cpu(), prompt.cpu(), cam, xyz.astype(np.float32), o_ids.numpy(), threshold=threshold)
    o_mask, _ = sr.query_mask(normed.cpu(), normed.cpu(), o_ids, o["chosen"].tolist(), 0.8)
    iou64 = _iou(o_mask.numpy(), is_a)
    print(f"prompt of {int(prompt.sum())} pixels, votes threshold {threshold}: chosen {chosen.tolist()} (float64 "
          f"{o['chosen'].tolist()}), IoU {iou:.4f} (float64 pipeline {iou64:.4f})")
    assert iou64 >= 0.97
    assert chosen.numel() == 1 and iou > IOU_BAR
    # into the renderer: the mask draws what the object's own Gaussians draw, and they cover the prompt
    ones = torch.ones(n, 3, device=dev)
    with torch.no_grad():
        img = render(cam, pc, SynthPipe(), bg, 0.0, 0.0, 0.0, mask=mask, override_color=ones)["render"]
        want = render(cam, pc, SynthPipe(), bg, 0.0, 0.0, 0.0, mask=torch.from_numpy(is_a).to(dev), override_color=ones)["render"]
    if iou == 1.0:
        assert torch.equal(img, want)
    assert float(img[0][prompt].mean()) > 0.5 and float((img - want).abs().mean()) < 0.05
