"""The trajectory view and the frame finish on the GPU (trase_amd.trajectory; the kernels of trase_amd/csrc/trajectory.hip)
against the numpy restatement of tests/trajectory_reference.py, the reference's own sampler sequences of
tests/golden/trajectory.npz, and torch's expressions on the device.

* sampler: every sequence is compared bit for bit (the int64 rows) with the numpy float32 rule on ordinary fp32 clouds;
  one constructed cloud has a sequence that a fused multiply-add in the distance would change.
* overlay: the winner map and the overlay are compared exactly with the numpy rule.
* present: the resize against ``F.interpolate`` on the device within ``8 * 2^-24 * max|v|`` -- the eight roundings an
  FMA-contracted evaluation of ``h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)`` and of the source index can differ in --
  exact for equal sizes; depth mode against the torch expression at the same bound; every blend exactly against the same
  fp32 expression in torch.  The figures are printed before they are asserted.

Measured on one MI355X: torch's kernel evaluates the source index with the product fused into the subtraction,
``fma(scale, dst + 0.5, -0.5)``.  An evaluation that rounds the product first is 2.9e-6 off ``F.interpolate`` at 48 x 64 ->
80 x 100 (bound 6.2e-7; depth mode 1.5e-6 against 4.8e-7) -- the weights move by an ulp of the source coordinate -- and
1.8e-7 off at -> 31 x 17, so the kernel fuses that product too."""
import os
import types

import numpy as np
import pytest
import torch

from tests import trajectory_reference as tr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "trajectory.npz")
RESIZE_BOUND = 8 * 2.0 ** -24


def _dev():
    return torch.device("cuda", 0)


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. sampler --------------------------------------------------------------------------------------------------------------

_fps_cache = {}


def _cloud(N):
    """An anisotropic fp32 normal cloud, its start row and the numpy sequence of the largest sample count asked of it."""
    if N not in _fps_cache:
        g = np.random.default_rng(N)
        points = (g.standard_normal((N, 3)) * np.array([1.0, 0.6, 0.3])).astype(np.float32)
        start = int(g.integers(0, N))
        longest = N if N <= 257 else 512 if N == 300_000 else 64
        _fps_cache[N] = (points, start, tr.fps(points, longest, start))
    return _fps_cache[N]


@pytest.mark.parametrize("N", [1, 255, 256, 257, 65_537, 300_000])
def test_sampler_sequences_equal_the_numpy_rule(N):
    from trase_amd.trajectory import farthest_point_sample
    points, start, want = _cloud(N)
    dev_points = torch.from_numpy(points).to(_dev())
    before = dev_points.clone()
    for npoint in sorted({1, 64, len(want)}):
        got = farthest_point_sample(dev_points, npoint, start=start)
        again = farthest_point_sample(dev_points.unsqueeze(0), npoint, start=start)          # (1, N, 3); reproducible
        assert got.dtype == torch.int64 and tuple(got.shape) == (npoint,)
        ref = want[:npoint] if npoint <= len(want) else tr.fps(points, npoint, start)        # N < 64: the rows repeat
        assert np.array_equal(_np(got), ref), (N, npoint)
        assert torch.equal(got, again)
    assert torch.equal(dev_points, before)


@pytest.mark.parametrize("N", [257, 65_537])
def test_sampler_masks(N):
    from trase_amd.trajectory import farthest_point_sample
    points, _, _ = _cloud(N)
    dev_points = torch.from_numpy(points).to(_dev())
    second = np.arange(N) % 2 == 1
    got = farthest_point_sample(dev_points, 64, mask=torch.from_numpy(second).to(_dev()), start=N - 2)
    assert np.array_equal(_np(got), tr.fps(points, 64, N - 2, mask=second)) and bool(second[_np(got)].all())
    single = np.arange(N) == N // 3
    got = farthest_point_sample(dev_points, 5, mask=torch.from_numpy(single).to(_dev()), start=N // 3)
    assert _np(got).tolist() == [N // 3] * 5
    got = farthest_point_sample(dev_points, 5, mask=torch.from_numpy(single).to(_dev()))     # the draw over one candidate
    assert _np(got).tolist() == [N // 3] * 5
    with pytest.raises(ValueError, match="masked row"):
        farthest_point_sample(dev_points, 4, mask=torch.from_numpy(second).to(_dev()), start=0)
    with pytest.raises(ValueError, match="no candidate"):
        farthest_point_sample(dev_points, 4, mask=torch.zeros(N, dtype=torch.bool, device=_dev()))
    with pytest.raises(ValueError, match="not a row"):
        farthest_point_sample(dev_points, 4, start=N)
    with pytest.raises(ValueError, match="npoint"):
        farthest_point_sample(dev_points, 0, start=0)
    with pytest.raises(ValueError, match="mask entries"):
        farthest_point_sample(dev_points, 4, mask=torch.ones(N - 1, dtype=torch.bool, device=_dev()))
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        farthest_point_sample(dev_points[:, :2], 4)


def test_sampler_repeats_once_every_distance_is_zero():
    from trase_amd.trajectory import farthest_point_sample
    g = np.random.default_rng(5)
    distinct = g.standard_normal((40, 3)).astype(np.float32)
    points = distinct[g.integers(0, 40, 700)]                           # 700 rows, 40 distinct points: more than one block
    assert len(np.unique(points, axis=0)) == 40
    dev_points = torch.from_numpy(points).to(_dev())
    got = _np(farthest_point_sample(dev_points, 64, start=123))
    assert np.array_equal(got, tr.fps(points, 64, 123))
    assert len(np.unique(got[:40])) == 40 and got[40:].tolist() == [0] * 24           # then the lowest candidate row repeats
    mask = np.arange(700) >= 9
    got = _np(farthest_point_sample(dev_points, 64, start=123, mask=torch.from_numpy(mask).to(_dev())))
    assert np.array_equal(got, tr.fps(points, 64, 123, mask=mask)) and got[40:].tolist() == [9] * 24


def test_sampler_rounds_every_product_and_sum():
    """A cloud on which a fused multiply-add changes the sequence: rows 1 = (b, a, 0) and 2 = (a, b, 0) are equally far from
    row 0 = the origin when every product and sum is rounded, rn(rn(a^2) + rn(b^2)) either way, so the lower row 1 is the
    second sample; an evaluation that fuses the second product into the sum, rn(rn(x^2) + y^2), puts row 2 farther."""
    from trase_amd.trajectory import farthest_point_sample
    g = np.random.default_rng(0)
    for _ in range(1000):
        a, b = g.uniform(0.5, 2.0, 2).astype(np.float32)
        fused1 = np.float32(np.float64(b * b) + np.float64(a) * np.float64(a))        # row 1, (dx, dy) = (b, a)
        fused2 = np.float32(np.float64(a * a) + np.float64(b) * np.float64(b))        # row 2
        if fused2 > fused1:
            break
    assert fused2 > fused1 and a * a + b * b == b * b + a * a
    points = np.array([[0, 0, 0], [b, a, 0], [a, b, 0]], dtype=np.float32)
    assert tr.fps(points, 2, 0).tolist() == [0, 1]
    assert _np(farthest_point_sample(torch.from_numpy(points).to(_dev()), 2, start=0)).tolist() == [0, 1]


def test_sampler_reference_sequences_and_default_draw():
    from trase_amd.trajectory import farthest_point_sample
    z = np.load(GOLD)
    for c in range(int(z["count"])):
        points, rows, seed = z[f"points{c}"], z[f"rows{c}"], int(z[f"seed{c}"])
        mask = torch.from_numpy(z[f"mask{c}"]).to(_dev()) if z[f"mask{c}"].size else None
        dev_points = torch.from_numpy(points).to(_dev())
        got = farthest_point_sample(dev_points, len(rows), mask=mask, start=int(rows[0]))
        assert np.array_equal(_np(got), rows), c
        torch.manual_seed(seed)                                          # the reference's own torch.randint draw
        drawn = farthest_point_sample(dev_points, len(rows), mask=mask)
        assert int(drawn[0]) == int(rows[0]) and np.array_equal(_np(drawn), rows), c


# ---- 2. overlay ----------------------------------------------------------------------------------------------------------------

def _cam(W, H, **kw):
    from trase_amd.synthetic import orbit_camera
    return orbit_camera(W, H, **kw).to(_dev())


def _walks(S, G, seed, extent=1.2, step=0.08):
    """S samples of G random walks: fp32 (S, G, 3)."""
    g = np.random.default_rng(seed)
    first = g.uniform(-extent, extent, (1, G, 3))
    return np.concatenate([first, first + np.cumsum(g.standard_normal((S - 1, G, 3)) * step, axis=0)]).astype(np.float32)


def _check_overlay(coords, cam, colors=None):
    from trase_amd.trajectory import draw_trajectories, jet_colors
    dev_coords = torch.from_numpy(coords).to(_dev())
    before = dev_coords.clone()
    img, index = draw_trajectories(dev_coords, cam, None if colors is None else torch.from_numpy(colors).to(_dev()), return_index=True)
    again = draw_trajectories(dev_coords, cam, None if colors is None else colors)           # a host table is accepted too
    want = tr.winner_map(coords, cam)
    assert index.dtype == torch.int32 and np.array_equal(_np(index).astype(np.int64), want)
    table = jet_colors(coords.shape[1]) if colors is None else colors
    assert img.dtype == torch.float32 and img.is_contiguous() and np.array_equal(_np(img), tr.overlay_image(want, table))
    assert torch.equal(img, again) and torch.equal(dev_coords.view(torch.int32), before.view(torch.int32))       # (NaN inputs: bits)
    return want


@pytest.mark.parametrize("W,H,G,S", [(64, 48, 1, 1), (64, 48, 7, 2), (67, 35, 7, 32), (67, 35, 512, 2), (64, 48, 512, 1),
                                     (1920, 1080, 512, 32)])
def test_overlay_equals_the_numpy_rule(W, H, G, S):
    cam = _cam(W, H, angle=0.3, radius=3.0)
    want = _check_overlay(_walks(S, G, seed=W + G + S), cam)
    hit = int((want >= 0).sum())
    print(f"{W} x {H}, G {G}, S {S}: {hit} overlay pixels, {len(np.unique(want[want >= 0]))} trajectories visible")
    assert hit >= 1 and (G == 1 or len(np.unique(want[want >= 0])) > 1)


def test_overlay_behind_the_camera_nan_and_user_colours():
    W, H, G, S = 67, 35, 7, 32
    cam = _cam(W, H, angle=0.2, radius=1.0)                             # the camera inside the cloud
    coords = _walks(S, G, seed=11, extent=1.6, step=0.25)
    full = tr.camera_fields(cam)[0]
    w = np.concatenate([coords.astype(np.float64), np.ones((S, G, 1))], -1) @ full[:, 3]
    _, _, ok = tr.pixels(coords, full, W, H)
    behind = (w < 0) & ok
    assert int(behind.sum()) >= 10 and int((w > 0).sum()) >= 10         # samples on both sides of the camera plane
    crossing = int((ok[:-1] & ok[1:] & ((w[:-1] < 0) != (w[1:] < 0))).sum())
    assert crossing >= 3                                                # segments that cross it are drawn all the same
    g = np.random.default_rng(2)
    colors = g.uniform(0, 1, (G, 3)).astype(np.float32)
    _check_overlay(coords, cam, colors)
    # NaN, infinite and far-away samples break their polylines
    broken = coords.copy()
    broken[3, 2] = np.nan
    broken[10, 4, 1] = np.inf
    eye = _np(cam.camera_center).astype(np.float64)
    fwd = -eye / np.linalg.norm(eye)
    side = np.cross(fwd, [0.0, 1.0, 0.0])
    broken[20, 5] = eye + side / np.linalg.norm(side) + 1e-5 * fwd      # 1e-5 in front of the camera plane, one unit aside:
    w_near = float(np.append(broken[20, 5].astype(np.float64), 1.0) @ full[:, 3])      # finite, far beyond 2^20 pixels
    assert 0 < abs(w_near) < 1e-4 and not tr.pixels(broken, full, W, H)[2][20, 5]
    broken[:, 6] = np.nan                                               # a trajectory that draws nothing
    want = _check_overlay(broken, cam, colors)
    assert not bool((want == 6).any())
    # ends far outside a large image: only the in-image range is visited
    wide = _cam(1920, 1080, angle=0.0, radius=3.0)
    eye = _np(wide.camera_center).astype(np.float64)
    side = g.uniform(-40, 40, (7, 3))
    side -= np.outer(side @ eye, eye) / (eye @ eye)                     # in the plane half a unit in front of the camera
    far = np.stack([g.uniform(-1, 1, (7, 3)), eye * (1 - 0.5 / np.linalg.norm(eye)) + side]).astype(np.float32)
    ix, iy, ok = tr.pixels(far, tr.camera_fields(wide)[0], 1920, 1080)
    assert bool(ok.all()) and int((np.abs(ix[1]) > 20_000).sum()) >= 4 and int((np.abs(iy[1]) > 20_000).sum()) >= 4
    _check_overlay(far, wide)


def test_overlay_ring_wraps():
    from trase_amd.trajectory import TrajectoryOverlay, jet_colors
    W, H, G, samp = 64, 48, 7, 4
    cam = _cam(W, H, angle=0.1, radius=3.0)
    g = np.random.default_rng(8)
    N = 900
    model = g.uniform(-1.2, 1.2, (N, 3)).astype(np.float32)
    opacity = g.uniform(0, 1, (N, 1)).astype(np.float32)
    mask = g.uniform(size=N) < 0.7
    view = TrajectoryOverlay(gs_num=G, samp_num=samp)
    rows = view.select(torch.from_numpy(model).to(_dev()), torch.from_numpy(opacity).to(_dev()), torch.from_numpy(mask).to(_dev()),
                       start=int(np.nonzero(mask & (opacity[:, 0] > 0.1))[0][5]))
    cand = mask & (opacity[:, 0] > np.float32(0.1))
    assert rows.dtype == torch.int64 and np.array_equal(_np(rows), tr.fps(model, G, int(rows[0]), mask=cand))
    frames = []
    for k in range(samp + 3):                                           # the ring wraps
        frame = (model + g.standard_normal((N, 3)) * 0.05 * (k + 1)).astype(np.float32)
        frames.append(frame[_np(rows)])
        img, index = view.update(torch.from_numpy(frame).to(_dev()), cam, return_index=True)
        held = np.stack(frames[-samp:])
        assert np.array_equal(_np(view.coords()), held), k
        want = tr.winner_map(held, cam)
        assert np.array_equal(_np(index).astype(np.int64), want), k
        assert np.array_equal(_np(img), tr.overlay_image(want, jet_colors(G))), k
    assert view.count == samp
    view.reset()
    out = torch.full((H, W, 4), 7.0, device=_dev())
    img, index = view.update(torch.from_numpy(frame).to(_dev()), cam, out=out, return_index=True)
    assert img is out and np.array_equal(_np(index).astype(np.int64), tr.winner_map(frames[-1][None], cam))
    assert int((index >= 0).sum()) <= G
    # the default draw of select() is the sampler's: torch.manual_seed reproduces it
    torch.manual_seed(3)
    a = view.select(torch.from_numpy(model).to(_dev()), torch.from_numpy(opacity).to(_dev()))
    torch.manual_seed(3)
    b = view.select(torch.from_numpy(model).to(_dev()), torch.from_numpy(opacity).to(_dev()))
    assert torch.equal(a, b) and bool((opacity[_np(a), 0] > 0.1).all())


# ---- 3. present ----------------------------------------------------------------------------------------------------------------

def _torch_finish(image, size):
    """gui.py:1085-1096 with torch on the device."""
    b = torch.nn.functional.interpolate(image.unsqueeze(0), size=size, mode="bilinear", align_corners=False).squeeze(0)
    return b.permute(1, 2, 0).contiguous().clamp(0, 1).contiguous()


def _image(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(3, h, w, generator=g) * 1.6 - 0.3).to(_dev())   # some values below 0 and above 1: the clamp acts


@pytest.mark.parametrize("size", [(80, 100), (31, 17), (48, 64)])
def test_present_resize_against_interpolate(size):
    from trase_amd.trajectory import present_frame
    image = _image(48, 64, seed=size[0])
    before = image.clone()
    got = present_frame(image, size=size)
    want = _torch_finish(image, size)
    bound = RESIZE_BOUND * float(image.abs().max())
    err = float((got - want).abs().max())
    print(f"48 x 64 -> {size[0]} x {size[1]}: max |ours - F.interpolate| {err:.3e}, bound {bound:.3e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == size + (3,) and got.is_contiguous()
    if size == (48, 64):
        assert torch.equal(got, want) and torch.equal(present_frame(image), got)             # equal sizes: exact
        inside = torch.rand(3, 48, 64, device=_dev())
        assert torch.equal(present_frame(inside), inside.permute(1, 2, 0))                  # values in [0, 1]: the input, bit for bit
    else:
        assert err <= bound
    assert float(got.min()) == 0.0 and float(got.max()) == 1.0
    assert torch.equal(image, before)


@pytest.mark.parametrize("size", [(80, 100), (48, 64)])
def test_present_depth_mode(size):
    from trase_amd.trajectory import present_frame
    g = torch.Generator().manual_seed(9)
    depth = (torch.rand(1, 48, 64, generator=g) * 7.5 + 0.2).to(_dev())
    before = depth.clone()
    got = present_frame(depth, size=size, depth=True)
    b = depth.repeat(3, 1, 1)
    b = (b - b.min()) / (b.max() - b.min() + 1e-20)                     # gui.py:1082-1083
    want = _torch_finish(b, size)
    err = float((got - want).abs().max())
    print(f"depth 48 x 64 -> {size[0]} x {size[1]}: max |ours - torch| {err:.3e}, bound {RESIZE_BOUND:.3e}")
    assert err <= RESIZE_BOUND * float(b.abs().max())
    assert torch.equal(got[..., 0], got[..., 1]) and torch.equal(got[..., 0], got[..., 2])
    if size == (48, 64):
        assert float(got.min()) == 0.0 and float(got.max()) == 1.0
    assert torch.equal(depth, before)
    flat = torch.full((1, 8, 8), 2.5, device=_dev())                    # max == min: 0 / 1e-20
    assert not bool(present_frame(flat, depth=True).any())


@pytest.mark.parametrize("size", [(80, 100), (48, 64)])
def test_present_blends_are_exact(size):
    from trase_amd.trajectory import draw_trajectories, present_frame
    H, W = size
    image = _image(48, 64, seed=21)
    g = torch.Generator().manual_seed(22)
    control = torch.zeros(H, W, 3)
    control[10:20, 12:22] += torch.tensor([1.0, 0.0, 0.0])              # gui.py:1149: red squares, summed where they overlap
    control[15:25, 17:27] += torch.tensor([1.0, 0.0, 0.0])
    control = control.to(_dev())
    cam = _cam(W, H, angle=0.3, radius=3.0)
    overlay = draw_trajectories(torch.from_numpy(_walks(8, 40, seed=4)).to(_dev()), cam)
    assert int((overlay[..., 3] > 0).sum()) > 50
    soft = torch.rand(H, W, 4, generator=g).to(_dev())                  # a fractional alpha: both products round
    tint = torch.rand(H, W, 3, generator=g).to(_dev())
    inputs = [image, control, overlay, soft, tint]
    before = [t.clone() for t in inputs]
    base = present_frame(image, size=size)

    def torch_blend(b, control=None, overlay=None, tint=None, weight=0.3):
        if control is not None:
            b = b * (control.sum(-1, keepdim=True) == 0) + control      # gui.py:1109-1111
        if overlay is not None:
            b = b * (1 - overlay[..., 3:]) + overlay[..., :3] * overlay[..., 3:]          # gui.py:1118
        if tint is not None:
            b = b + weight * tint                                       # gui.py:1122
        return b

    for kw in (dict(control_overlay=control), dict(overlay=overlay), dict(overlay=soft), dict(tint=tint),
               dict(tint=tint, tint_weight=0.45), dict(control_overlay=control, overlay=soft, tint=tint)):
        got = present_frame(image, size=size, **kw)
        want = torch_blend(base, kw.get("control_overlay"), kw.get("overlay"), kw.get("tint"), kw.get("tint_weight", 0.3))
        assert torch.equal(got, want), sorted(kw)
    assert float(present_frame(image, size=size, tint=tint).max()) > 1.0                # not clamped afterwards
    out = torch.empty(H, W, 3, device=_dev())
    assert present_frame(image, size=size, overlay=soft, out=out) is out and torch.equal(out, torch_blend(base, overlay=soft))
    assert all(torch.equal(a, b) for a, b in zip(inputs, before))
    with pytest.raises(ValueError, match="overlay must be"):
        present_frame(image, size=size, overlay=soft[:-1])
    with pytest.raises(ValueError, match="image must be"):
        present_frame(image, size=size, depth=True)
    with pytest.raises(ValueError, match="out must be"):
        present_frame(image, size=size, out=torch.empty(W, H, 3, device=_dev()))
    with pytest.raises(RuntimeError, match="GPU only"):
        present_frame(image, size=size, tint=tint.cpu())
