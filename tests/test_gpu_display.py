"""The display stage on the GPU (trase_amd.display.splat_points / feature_colors, trase_amd.segment.assign_clusters; the
kernels of trase_amd/csrc/display.hip and seg_assign_cosine_kernel of segment.hip) against the render.py fixture
tests/golden/display.npz and the float64 restatement of tests/display_reference.py.

Every full-size bar is the reference's, measured inside the test and never taken from the kernel:

* splat: ``bar`` is the largest distance between the reference's all-fp32 pixel coordinates (restated below with torch on
  the CPU) and the float64 ones over the in-image points.  A point is *fragile* if either float64 coordinate lies within
  2 * bar of an integer (that covers the image borders); a pixel is *excluded* if a fragile point lies within 2 * bar of
  its square.  On every other pixel the winner must be the float64 highest-index winner; on an excluded pixel it must be -1
  or a point within 2 * bar of that pixel.  Every layer must be bit-equal to the gather of the winner map.
* PCA colours: ``ref_bar`` is the largest distance between the reference's fp32 QR / SVD colours (torch on the CPU, re-signed
  to the float64 axes) and the float64 colours; ours must be within it.
* assignment: ``ref_bar`` is the largest distance between the fp32 ``einsum`` scores of gui.py:288 (torch, CPU) and the
  float64 scores.  A row is *decided* if its float64 top-2 gap exceeds 2 * ref_bar and must then return the float64 argmax;
  any other row must return a centre scoring within 2 * ref_bar of the best.

The figures are printed before they are asserted.  Measured on one MI355X: splat bar 2.19e-4 px, 214 265 in-image points on
201 205 pixels, 0.13 % fragile points, 777 excluded pixels (0.39 % of the hit ones), the fp32 reference moves 15 points to
another bucket, every winner equal to the float64 one; PCA at 300k x 32: reference bar 5.5e-6, ours 3.5e-7 (D = 1 / 3 / 64 at
N = 5000: 1.9e-7 / 8.8e-7 / 1.6e-6 against 8.1e-8 / 1.5e-7 / 3.2e-7), axes within 1e-14 of the float64 ones; assignment at
K = 64 / 4096: reference bar 2.6e-7 / 3.2e-7, 7e-6 / 2e-5 of the rows undecided, every id equal to the float64 argmax."""
import os
import types

import numpy as np
import pytest
import torch

from tests import display_reference as dr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXCLUDED_MAX = 0.02         # condition on the scene, asserted: excluded pixels over hit pixels
UNDECIDED_MAX = 0.001       # condition on the centres, asserted: undecided rows over all rows
EIGEN_GAP_MIN = 0.05        # condition on the features, asserted: relative gaps between the top four eigenvalues


def _dev():
    return torch.device("cuda", 0)


def _fixture():
    z = np.load(os.path.join(HERE, "golden", "display.npz"))
    cam = types.SimpleNamespace(full_proj_transform=torch.from_numpy(z["full_proj_transform"]).to(_dev()),
                                image_width=int(z["width"]), image_height=int(z["height"]), znear=0.01, zfar=100.0)
    t = {k: torch.from_numpy(z[k]).to(_dev()) for k in ("points", "features", "cluster_colors", "centres")}
    return z, cam, t


def _cam(matrix, W, H):
    return types.SimpleNamespace(full_proj_transform=torch.tensor(matrix, dtype=torch.float32, device=_dev()), image_width=W,
                                 image_height=H)


def _np(t):
    return t.detach().cpu().numpy()


def _check_exact(points, cam, colors=None, white_background=False, mask=None):
    """splat_points against the restatement where no coordinate is near an integer (or all are exact): everything equal."""
    from trase_amd.display import splat_points
    layers = list(colors) if isinstance(colors, (list, tuple)) else [colors]
    images, index = splat_points(points, cam, colors, white_background=white_background, mask=mask, return_index=True)
    images = images if isinstance(colors, (list, tuple)) else [images]
    want = dr.winner_map(points, cam, mask=mask)
    assert index.dtype == torch.int64 and np.array_equal(_np(index), want)
    for img, c in zip(images, layers):
        assert img.dtype == torch.float32 and tuple(img.shape) == (3,) + want.shape
        assert np.array_equal(_np(img), dr.gather_image(want, c, white_background))
    return want


# ---- 1. the render.py fixture ----------------------------------------------------------------------------------------------

def test_fixture_winner_map_images_colours_and_ids():
    from trase_amd.display import feature_colors, splat_points
    from trase_amd.segment import assign_clusters
    z, cam, t = _fixture()
    before = {k: v.clone() for k, v in t.items()}
    colors, (axes, mean) = feature_colors(t["features"], return_basis=True)
    o = dr.pca_colors(z["features"])
    err = float(np.abs(_np(colors).astype(np.float64) - o["colors"]).max())
    cos = np.abs((axes * o["axes"]).sum(axis=1))
    print(f"fixture: our PCA colours off float64 by {err:.3e} (the reference, re-signed: {float(z['pca_gap']):.3e}); "
          f"axes 1 - |cos| {float((1 - cos).max()):.3e}")
    assert colors.dtype == torch.float32 and tuple(colors.shape) == (len(z["points"]), 3)
    assert err <= float(z["pca_gap"])
    assert axes.dtype == np.float64 and axes.shape == (3, 32) and mean.shape == (32,) and float(cos.min()) >= 1 - 1e-6
    for white in (False, True):
        images, index = splat_points(t["points"], cam, [None, t["cluster_colors"], colors], white_background=white, return_index=True)
        assert np.array_equal(_np(index), z["winner"].astype(np.int64))              # the float64 winner map, exactly
        for img, c in zip(images, (None, z["cluster_colors"], _np(colors))):
            assert np.array_equal(_np(img), dr.gather_image(z["winner"].astype(np.int64), c, white))
    assert np.array_equal(_np(images[0]), 1 - z["ref_dots"])                       # the reference's own dots (white: inverted)
    single = splat_points(t["points"], cam)
    assert torch.is_tensor(single) and np.array_equal(_np(single), z["ref_dots"])
    ids, scores = assign_clusters(t["features"], t["centres"], return_scores=True)
    assert ids.dtype == torch.int64 and np.array_equal(_np(ids), z["ids"].astype(np.int64))
    s64 = dr.cosine_scores(z["features"], z["centres"]).max(axis=1)
    assert scores.dtype == torch.float32 and float(np.abs(_np(scores) - s64).max()) < 1e-5
    assert torch.equal(assign_clusters(t["features"].unsqueeze(1), t["centres"].cpu()), ids)      # (N, 1, D), host centres
    assert all(torch.equal(t[k], before[k]) for k in t)                # inputs untouched


# ---- 2. the splat at full size -----------------------------------------------------------------------------------------------

N_FULL, W_FULL, H_FULL = 300_000, 1920, 1080
_splat_cache = {}


def reference_pixels_fp32(points, cam):
    """render.py:247-251 restated with torch in fp32 on the CPU."""
    xyz = points.detach().cpu().float()
    cur_pts = torch.cat([xyz, torch.ones_like(xyz[..., :1])], dim=-1)
    cur_pts2d = cur_pts @ cam.full_proj_transform.detach().cpu().float()
    cur_pts2d = cur_pts2d[..., :2] / cur_pts2d[..., -1:]
    cur_pts2d = (cur_pts2d + 1) / 2 * torch.tensor([cam.image_width, cam.image_height])
    return cur_pts2d.double().numpy()


def _splat_scene():
    if not _splat_cache:
        from trase_amd.synthetic import make_scene, orbit_camera
        cam = orbit_camera(W_FULL, H_FULL, angle=0.3, radius=4.0)
        points = make_scene(N_FULL, feat_dim=1, seed=3).xyz
        g = torch.Generator().manual_seed(17)
        table = torch.rand(16, 3, generator=g)
        cluster_colors = table[torch.randint(0, 16, (N_FULL,), generator=g)]
        random_colors = torch.rand(N_FULL, 3, generator=g)
        mask = torch.rand(N_FULL, generator=g) < 0.4
        full, W, H = dr.camera_fields(cam)
        px, py = dr.project(points, full, W, H)
        ok, _, _ = dr.landing(px, py, W, H)
        p32 = reference_pixels_fp32(points, cam)
        bar = float(max(np.abs(p32[ok, 0] - px[ok]).max(), np.abs(p32[ok, 1] - py[ok]).max()))
        ok32, c32, r32 = dr.landing(p32[:, 0], p32[:, 1], W, H)
        _, c64, r64 = dr.landing(px, py, W, H)
        moved = int(((ok32 != ok) | (c32 != c64) | (r32 != r64)).sum())
        _splat_cache.update(cam=cam, points=points, layers=[None, cluster_colors, random_colors], mask=mask, px=px, py=py, ok=ok,
                            bar=bar, moved=moved)
    return _splat_cache


def _excluded_pixels(px, py, take, bar, W, H):
    """-> (fragile bool (N,), excluded bool (H * W,), near: dict pixel -> set of fragile points within 2 * bar of it)."""
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(px) & np.isfinite(py) & take
        fragile = finite & ((np.abs(px - np.round(px)) <= 2 * bar) | (np.abs(py - np.round(py)) <= 2 * bar))
        fragile &= (px > -1) & (px < W + 1) & (py > -1) & (py < H + 1)
    excluded = np.zeros(H * W, dtype=bool)
    near = {}
    for i in np.nonzero(fragile)[0]:
        for c in {int(np.floor(px[i] - 2 * bar)), int(np.floor(px[i] + 2 * bar))}:
            for r in {int(np.floor(py[i] - 2 * bar)), int(np.floor(py[i] + 2 * bar))}:
                if 0 <= c < W and 0 <= r < H:
                    excluded[r * W + c] = True
                    near.setdefault(r * W + c, set()).add(int(i))
    return fragile, excluded, near


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("white", [False, True])
def test_splat_full_size_against_float64(white, masked):
    from trase_amd.display import splat_points
    s = _splat_scene()
    dev = _dev()
    cam, W, H, bar = s["cam"], W_FULL, H_FULL, s["bar"]
    mask = s["mask"] if masked else None
    take = _np(mask) if masked else np.ones(N_FULL, dtype=bool)
    points = s["points"].to(dev)
    layers = [None if c is None else c.to(dev) for c in s["layers"]]
    images, index = splat_points(points, cam, layers, white_background=white, mask=None if mask is None else mask.to(dev),
                                 return_index=True)
    again, index2 = splat_points(points, cam, layers, white_background=white, mask=None if mask is None else mask.to(dev),
                                 return_index=True)
    want = dr.winner_map(s["points"], cam, mask=mask).reshape(-1)
    got = _np(index).reshape(-1)
    fragile, excluded, near = _excluded_pixels(s["px"], s["py"], take, bar, W, H)
    hit = want >= 0
    share = float(excluded.sum()) / float(hit.sum())
    wrong = int((got[~excluded] != want[~excluded]).sum())
    print(f"white {white}, masked {masked}: bar {bar:.3e} px; in-image points {int((s['ok'] & take).sum())}, hit pixels "
          f"{int(hit.sum())}; fragile points {100 * float(fragile.sum()) / float(take.sum()):.3f} %; excluded pixels "
          f"{int(excluded.sum())} = {100 * share:.3f} % of hit pixels; points the fp32 reference puts in another bucket "
          f"{s['moved']}; other pixels with another winner {wrong}; winners equal to float64 overall "
          f"{100 * float((got == want).mean()):.5f} %")
    assert share <= EXCLUDED_MAX
    assert wrong == 0
    for p in np.nonzero(excluded & (got != want))[0]:
        assert got[p] == -1 or int(got[p]) in near[p], p
    for img, c in zip(images, s["layers"]):
        assert np.array_equal(_np(img), dr.gather_image(got.reshape(H, W), c, white))       # bit-equal to the gather, or background
    assert torch.equal(index, index2) and all(torch.equal(a, b) for a, b in zip(images, again))


# ---- 3. splat edge cases ---------------------------------------------------------------------------------------------------

IDENTITY = [[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]        # p = (x, y, z, 1): px = (x + 1) / 2 * W
W_IS_Z = [[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]]          # p = (x, y, 0, z): a perspective division by z


def test_splat_edge_cases():
    from trase_amd.display import splat_points
    dev = _dev()
    W, H = 64, 48
    cam = _cam(IDENTITY, W, H)
    # N = 0
    img, index = splat_points(torch.zeros(0, 3, device=dev), cam, return_index=True)
    assert not bool(img.any()) and bool((index == -1).all()) and tuple(img.shape) == (3, H, W)
    img = splat_points(torch.zeros(0, 3, device=dev), cam, [None, torch.zeros(0, 3, device=dev)], white_background=True)
    assert len(img) == 2 and all(bool((i == 1).all()) for i in img)
    # no point in the image
    out = torch.tensor([[2.0, 0, 0], [0, -3.0, 0], [float("nan"), 0, 0], [float("inf"), 0, 0]], device=dev)
    assert bool((_check_exact(out, cam) == -1).all())
    # all points in one pixel: the highest index wins
    same = torch.zeros(1000, 3, device=dev)
    col = torch.rand(1000, 3, device=dev)
    want = _check_exact(same, cam, [col])
    assert int((want >= 0).sum()) == 1 and want[H // 2, W // 2] == 999
    # points exactly on the borders px = 0 and px = W (and py = 0, py = H) land nowhere; one step inside they do
    x = torch.tensor([-1.0, 1.0, -1.0 + 1.0 / W, 1.0 - 1.0 / W, 0.25, 0.25], device=dev)
    y = torch.tensor([0.25, 0.25, 0.25, 0.25, -1.0, 1.0], device=dev)
    border = torch.stack([x, y, torch.zeros_like(x)], 1)
    want = _check_exact(border, cam, white_background=True)
    assert sorted(want[want >= 0].tolist()) == [2, 3] and want[30, 0] == 2 and want[30, W - 1] == 3
    # w < 0 with the flipped projection inside the image lands; w = 0 does not
    persp = _cam(W_IS_Z, W, H)
    pts = torch.tensor([[0.5, 0.5, -2.0], [0.5, 0.5, 2.0], [0.5, 0.5, 0.0], [0.0, 0.0, 0.0], [-1.0, 0.5, -2.0]], device=dev)
    want = _check_exact(pts, persp, [torch.rand(5, 3, device=dev)])
    assert sorted(want[want >= 0].tolist()) == [0, 1, 4] and want[18, 24] == 0 and want[30, 40] == 1
    # a non-contiguous view, a mask, L = 4
    g = torch.Generator().manual_seed(4)
    wide = (torch.rand(5000, 5, generator=g) * 2.2 - 1.1).to(dev)
    view = wide[:, 1:4]
    assert not view.is_contiguous()
    cols = [torch.rand(5000, 3, generator=g).to(dev) for _ in range(3)]
    mask = (torch.rand(5000, generator=g) < 0.5).to(dev)
    _check_exact(view, cam, [cols[0], None, cols[1], cols[2]], mask=mask)
    _check_exact(view, cam, (cols[0],), white_background=True)
    assert torch.equal(wide[:, 1:4], view)
    # argument errors
    with pytest.raises(ValueError, match="1 to 4 colour layers"):
        splat_points(view, cam, [None] * 5)
    with pytest.raises(ValueError, match="1 to 4 colour layers"):
        splat_points(view, cam, [])
    with pytest.raises(ValueError, match=r"points must be \(N, 3\)"):
        splat_points(wide, cam)
    with pytest.raises(ValueError, match="colors must be"):
        splat_points(view, cam, cols[0][:-1])
    with pytest.raises(ValueError, match="mask entries"):
        splat_points(view, cam, mask=mask[:-1])
    with pytest.raises(RuntimeError, match="GPU only"):
        splat_points(view.cpu(), cam)
    with pytest.raises(RuntimeError, match="GPU only"):
        splat_points(view, cam, [cols[0].cpu()])
    with pytest.raises(RuntimeError, match="GPU only"):
        splat_points(view, cam, mask=mask.cpu())


# ---- 4. PCA colours ----------------------------------------------------------------------------------------------------------

def cluster_features(n, d, seed=3):
    """Features around 12 cluster centres with a per-dimension scale decaying by 0.8: a clear spectrum."""
    g = np.random.default_rng(seed)
    scale = 2.0 * 0.8 ** np.arange(d)
    centres = g.standard_normal((12, d)) * scale
    label = g.integers(0, 12, n)
    return (centres[label] + 0.15 * g.standard_normal((n, d)) * scale).astype(np.float32)


def reference_colors_fp32(x):
    """render.py:52-59 restated with torch in fp32 on the CPU."""
    x = torch.from_numpy(x)
    X_center = x - torch.mean(x, axis=0)
    q, r = torch.linalg.qr(X_center)
    U, s, Vt = torch.linalg.svd(r, full_matrices=False)
    pca_result = torch.matmul(q, torch.matmul(U[:, :3], torch.diag(s[:3])))
    return ((pca_result - pca_result.min()) / (pca_result.max() - pca_result.min())).numpy()


def _check_pca(what, feats):
    from trase_amd.display import feature_colors
    X = torch.from_numpy(feats).to(_dev())
    colors, (axes, mean) = feature_colors(X, return_basis=True)
    again = feature_colors(X)
    o = dr.pca_colors(feats)
    D = feats.shape[-1]
    k = min(3, D)
    ref = reference_colors_fp32(feats.reshape(len(feats), D))
    ref_bar = float(np.abs(dr.align_colors(ref, o["raw"][:, :k]) - o["colors"][:, :k]).max())
    ours = _np(colors).astype(np.float64)
    err = float(np.abs(ours - o["colors"]).max())
    cos = np.abs((axes[:k] * o["axes"][:k]).sum(axis=1))
    ev = o["eigenvalues"]
    gaps = ((ev[:k] - ev[1:k + 1]) / ev[:k]) if D > k else ((ev[:k - 1] - ev[1:k]) / ev[:k - 1])
    print(f"{what}: relative eigenvalue gaps {np.round(gaps, 3).tolist()}; reference fp32 QR/SVD bar {ref_bar:.3e}, ours off float64 "
          f"by {err:.3e}; axes 1 - |cos| {float((1 - cos).max()):.3e}; mean off by {float(np.abs(mean - o['mean']).max()):.3e}")
    assert bool((gaps >= EIGEN_GAP_MIN).all())
    assert err <= ref_bar
    assert float(cos.min()) >= 1 - 1e-6
    lead = axes[np.arange(k), np.abs(axes[:k]).argmax(axis=1)]
    assert bool((lead > 0).all()) and not axes[k:].any()                # the sign rule; missing axes are zero
    assert torch.equal(colors, again)
    assert float(colors.min()) == 0.0 and float(colors.max()) == 1.0
    return colors


def test_pca_full_size_against_float64():
    _check_pca("N 300k, D 32", cluster_features(300_000, 32))


@pytest.mark.parametrize("D", [1, 3, 64])
def test_pca_other_widths(D):
    _check_pca(f"N 5000, D {D}", cluster_features(5000, D))


def test_pca_input_forms_constant_features_and_errors():
    from trase_amd.display import feature_colors
    dev = _dev()
    feats = torch.from_numpy(cluster_features(3000, 32)).to(dev)
    before = feats.clone()
    base = feature_colors(feats)
    assert torch.equal(feature_colors(feats.unsqueeze(1)), base) and torch.equal(feats, before)
    wide = torch.cat([feats, feats], 1)
    assert torch.equal(feature_colors(wide[:, :32]), base)              # a non-contiguous view
    # constant features: every centred row is zero, max == min, and the reference's 0 / 0 is NaN
    const = torch.tensor([0.5, -1.25, 2.0, 0.0], device=dev).repeat(4096, 1)
    assert bool(torch.isnan(feature_colors(const)).all())
    with pytest.raises(ValueError, match="n_components"):
        feature_colors(feats, 4)
    with pytest.raises(ValueError, match="D <= 64"):
        feature_colors(torch.zeros(10, 65, device=dev))
    with pytest.raises(ValueError, match="N >= 2"):
        feature_colors(feats[:1])
    with pytest.raises(ValueError, match=r"\(N, D\)"):
        feature_colors(torch.zeros(10, 2, 8, device=dev))


# ---- 5. nearest centre ---------------------------------------------------------------------------------------------------------

def _assign_scene(K):
    from trase_amd.synthetic import make_scene
    feats = make_scene(N_FULL, feat_dim=32, seed=0).gaussian_features.reshape(N_FULL, 32)
    normed = torch.nn.functional.normalize(feats, dim=-1, p=2)
    g = torch.Generator().manual_seed(K)
    rows = torch.randperm(N_FULL, generator=g)[:K]
    centres = torch.nn.functional.normalize(normed[rows] + 0.05 * torch.randn(K, 32, generator=g), dim=-1, p=2)
    return feats, normed, centres


@pytest.mark.parametrize("K", [64, 4096])
def test_assignment_full_size_against_float64(K):
    from trase_amd.segment import assign_clusters
    feats, normed, centres = _assign_scene(K)
    dev = _dev()
    ids, scores = assign_clusters(feats.to(dev), centres.to(dev), return_scores=True)
    again = assign_clusters(feats.to(dev), centres.to(dev))
    got = ids.cpu()
    f64 = feats.double()
    n64 = f64 / f64.norm(dim=-1, keepdim=True)
    c64 = centres.double()
    ref_bar, best, second, arg, mine, ref_differs = 0.0, [], [], [], [], 0
    for lo in range(0, N_FULL, 20_000):                                     # N x K float64 scores, in row chunks
        s64 = n64[lo:lo + 20_000] @ c64.T
        s32 = torch.einsum("nc,bc->bn", centres, normed[lo:lo + 20_000])    # gui.py:288
        ref_bar = max(ref_bar, float((s32.double() - s64).abs().max()))
        top = s64.max(dim=1)
        best.append(top.values)
        arg.append(top.indices)
        mine.append(s64.gather(1, got[lo:lo + 20_000, None])[:, 0])
        ref_differs += int((s32.argmax(dim=1) != top.indices).sum())
        second.append(s64.scatter_(1, top.indices[:, None], -float("inf")).max(dim=1).values)     # -inf at K = 1: decided
    best, second, arg, mine = torch.cat(best), torch.cat(second), torch.cat(arg), torch.cat(mine)
    decided = (best - second) > 2 * ref_bar
    undecided_share = 1.0 - float(decided.double().mean())
    wrong = int((got[decided] != arg[decided]).sum())
    excess = float((best - mine).max())
    score_err = float((scores.cpu().double() - mine).abs().max())
    print(f"K {K}: reference fp32 einsum bar {ref_bar:.3e}; undecided rows {undecided_share:.2e}; decided rows with another id "
          f"{wrong}; largest score deficit {excess:.3e}; our winning scores off float64 by {score_err:.3e}; the fp32 reference "
          f"disagrees with float64 on {ref_differs} rows; ids equal to float64 overall {100 * float((got == arg).double().mean()):.5f} %")
    assert undecided_share <= UNDECIDED_MAX
    assert wrong == 0
    assert excess <= 2 * ref_bar
    assert torch.equal(ids, again)


def test_assignment_ties_zero_rows_limits_and_downstream():
    from trase_amd.segment import assign_clusters, lift_votes, segment_mask
    z, cam, t = _fixture()
    dev = _dev()
    ids = assign_clusters(t["features"], t["centres"])
    doubled = torch.cat([t["centres"], t["centres"]])
    assert torch.equal(assign_clusters(t["features"], doubled), ids)                    # exact ties go to the lowest k
    flipped = torch.cat([t["centres"].flip(0), t["centres"]])
    want = torch.minimum(11 - ids, 12 + ids)
    assert torch.equal(assign_clusters(t["features"], flipped), want)
    feats = t["features"].clone()
    feats[5] = 0
    got, scores = assign_clusters(feats, t["centres"], return_scores=True)
    assert int(got[5]) == 0 and float(scores[5]) == 0.0 and torch.equal(got[6:], ids[6:])   # a zero row gives id 0
    one = assign_clusters(t["features"], t["centres"][:1])
    assert one.dtype == torch.int64 and not bool(one.any())                             # K = 1
    assert assign_clusters(t["features"][:0], t["centres"]).numel() == 0
    for D in (1, 5, 8, 24, 64):                                                         # every register width, odd sizes
        g = torch.Generator().manual_seed(D)
        f, c = torch.randn(777, D, generator=g), torch.randn(300, D, generator=g)
        assert np.array_equal(_np(assign_clusters(f.to(dev), c.to(dev))), dr.assign(f, c)[0])
    with pytest.raises(ValueError, match="K <= 4096"):
        assign_clusters(t["features"], torch.zeros(4097, 32, device=dev))
    with pytest.raises(ValueError, match="centres must be"):
        assign_clusters(t["features"], t["centres"][:, :16])
    with pytest.raises(RuntimeError, match="GPU only"):
        assign_clusters(t["features"].cpu(), t["centres"])
    # the ids pass unchanged into segment_mask and lift_votes
    m = segment_mask(t["features"], ids, [int(ids[0])], 0.5)
    assert m.dtype == torch.bool and bool(m.any()) and bool((ids[m] == ids[0]).all())
    H, W = cam.image_height, cam.image_width
    prompt = torch.zeros(H, W, dtype=torch.bool, device=dev)
    prompt[10:40, 20:70] = True
    votes = lift_votes(torch.full((H, W), 3.0, device=dev), prompt, cam, t["points"], ids, num_clusters=12)
    assert votes.numel() == 12 and int(votes.sum()) == int(prompt.sum())


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------

def test_feature_colours_into_the_renderer_and_the_splat():
    from gaussian_renderer import render
    from trase_amd.display import feature_colors, splat_points
    from trase_amd.synthetic import SynthGaussianModel, SynthPipe, make_scene, orbit_camera
    dev = _dev()
    n, W, H = 3000, 160, 96
    scene = make_scene(n, feat_dim=32, seed=6, scale_mult=0.9)
    scene.gaussian_features = torch.from_numpy(cluster_features(n, 32)).reshape(n, 1, 32)
    pc = SynthGaussianModel(scene.to(dev), requires_grad=False)
    cam = orbit_camera(W, H, angle=0.2).to(dev)
    colors = feature_colors(pc.get_gaussian_features)
    assert tuple(colors.shape) == (n, 3) and float(colors.min()) == 0.0 and float(colors.max()) == 1.0
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        img = render(cam, pc, SynthPipe(), bg, 0.0, 0.0, 0.0, override_color=colors)["render"]
        want = render(cam, pc, SynthPipe(), bg, 0.0, 0.0, 0.0, override_color=colors.clone().contiguous())["render"]
    assert torch.equal(img, want) and float(img.max()) > 0.1
    dots, pca = splat_points(pc.get_xyz, cam, [None, colors])
    hit = dots[0] > 0
    assert int(hit.sum()) > n // 3 and bool((pca[:, ~hit] == 0).all())
