"""CPU checks of the trajectory restatement (tests/trajectory_reference.py): the sampler rule against the sequences the
reference's own farthest_point_sample produced (tests/golden/trajectory.npz, written by tests/golden/make_trajectory.py), the
jet table against matplotlib's recorded values, the line rule against a brute-force per-pixel statement of the same
definition, and what the new entry points do without a GPU (limits, null pointers, refusal of CPU tensors)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests import trajectory_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "trajectory.npz")
INVALID = -1                    # TRASE_ERR_INVALID


def clouds():
    z = np.load(GOLD)
    for c in range(int(z["count"])):
        mask = z[f"mask{c}"]
        yield c, z[f"points{c}"], (mask if mask.size else None), z[f"rows{c}"], int(z[f"seed{c}"])


def test_sampler_rule_reproduces_the_reference_sequences():
    z = np.load(GOLD)
    assert int(z["count"]) == 4 and int(z["npoint"]) == 64
    sizes = []
    for c, points, mask, rows, _ in clouds():
        # the fixture's premise: coordinates are multiples of 1/256 in [-2, 2], so every fp32 distance is exact
        k = points.astype(np.float64) * 256
        assert np.array_equal(k, np.round(k)) and float(np.abs(points).max()) <= 2.0
        got = tr.fps(points, len(rows), int(rows[0]), mask=mask)
        assert np.array_equal(got, rows), c
        assert len(np.unique(rows)) == len(rows)
        if mask is not None:
            assert bool(mask[rows].all()) and not bool(mask.all())
        sizes.append(len(points))
    assert sizes == [65, 257, 1000, 5000]


def test_sampler_rule_ties_repeats_and_masks():
    # equal distances go to the lowest row: the four corners of a square, start at corner 0 -> the far corner, then 1 before 2
    square = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float32)
    assert tr.fps(square, 4, 0).tolist() == [0, 3, 1, 2]
    # more samples than distinct points: once every distance is 0 the lowest candidate row repeats
    dup = np.repeat(square[:3], 2, axis=0)                      # rows 0,1 | 2,3 | 4,5 pairwise equal
    assert tr.fps(dup, 6, 3).tolist() == [3, 4, 0, 0, 0, 0]
    mask = np.array([False, True, True, True, True, True])
    assert tr.fps(dup, 6, 3, mask=mask).tolist() == [3, 4, 1, 1, 1, 1]
    assert tr.fps(dup, 3, 5, mask=np.arange(6) == 5).tolist() == [5, 5, 5]       # a single candidate


def test_jet_table_equals_matplotlib():
    from trase_amd.trajectory import jet_colors
    z = np.load(GOLD)
    for n in (1, 2, 7, 512):
        got = jet_colors(n)
        assert got.dtype == np.float32 and got.shape == (n, 3)
        assert np.array_equal(got, (z[f"jet{n}"] / 255).astype(np.float32)), n
        assert np.array_equal((got.astype(np.float64) * 255).round().astype(np.int32), z[f"jet{n}"])


def brute_force_line(ax, ay, bx, by, W, H):
    """The line rule stated per pixel: (x, y) is drawn iff x lies between the ends on the major axis and y is the rule's
    minor coordinate at x (roles swapped for a steep segment).  Every pixel of the image is asked."""
    dx, dy = abs(bx - ax), abs(by - ay)
    img = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            if dx >= dy:
                if not min(ax, bx) <= x <= max(ax, bx):
                    continue
                want = ay if dx == 0 else ay + (1 if by > ay else -1) * ((2 * abs(x - ax) * dy + dx) // (2 * dx))
                img[y, x] = y == want
            else:
                if not min(ay, by) <= y <= max(ay, by):
                    continue
                want = ax + (1 if bx > ax else -1) * ((2 * abs(y - ay) * dx + dy) // (2 * dy))
                img[y, x] = x == want
    return img


SEGMENTS = [
    (3, 5, 20, 5), (20, 5, 3, 5),                       # horizontal, reversed
    (7, 2, 7, 15), (7, 15, 7, 2),                       # vertical, reversed
    (2, 2, 14, 14), (14, 14, 2, 2), (2, 14, 14, 2),     # diagonals
    (1, 1, 22, 9), (22, 9, 1, 1), (1, 9, 22, 1),        # shallow
    (4, 0, 9, 16), (9, 16, 4, 0), (9, 0, 4, 16),        # steep
    (5, 5, 5, 5),                                       # a == b: one pixel
    (-8, 3, 30, 12), (10, -7, 13, 25), (-5, -5, 40, 30),                        # both ends outside, crossing
    (-100_000, 4, 100_000, 9), (6, -100_000, 11, 100_000),                      # ends 10^5 pixels outside
    (-100_000, -70_000, 100_000, 70_030), (100_000, 8, -100_000, 12),
    (-100_000, 3, -50_000, 8), (30, 40, 50, 90),                                # wholly outside
    (0, 0, 23, 16), (23, 16, 0, 0),                                             # the corners
]


@pytest.mark.parametrize("seg", SEGMENTS)
def test_line_rule_against_the_per_pixel_statement(seg):
    W, H = 24, 17
    ax, ay, bx, by = seg
    x, y = tr.line_pixels(ax, ay, bx, by, W, H)
    assert x.dtype == np.int64 and len(x) <= max(W, H)                  # only the in-image range of the major axis is visited
    img = np.zeros((H, W), dtype=bool)
    img[y, x] = True
    assert int(img.sum()) == len(x)                                     # no pixel twice
    assert np.array_equal(img, brute_force_line(ax, ay, bx, by, W, H))
    for px, py in ((ax, ay), (bx, by)):                                 # both end points are drawn if they are in the image
        if 0 <= px < W and 0 <= py < H:
            assert img[py, px]


def _cam(matrix, W, H):
    return types.SimpleNamespace(full_proj_transform=np.asarray(matrix, dtype=np.float32), image_width=W, image_height=H)


IDENTITY = [[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]        # px = (x + 1) / 2 * W


def test_overlay_rule_truncation_breaks_and_priority():
    W, H = 32, 16
    cam = _cam(IDENTITY, W, H)
    to_world = lambda px, py: [2 * px / W - 1, 2 * py / H - 1, 0.0]           # noqa: E731
    # truncation toward zero: -0.5 -> 0 (astype(int32)), not floor's -1
    ix, iy, ok = tr.pixels(np.array([to_world(-0.5, 3.75), to_world(5.25, -0.75)], dtype=np.float32), np.asarray(IDENTITY, dtype=np.float64), W, H)
    assert ix.tolist() == [0, 5] and iy.tolist() == [3, 0] and bool(ok.all())
    # two crossing trajectories: the higher index wins the crossing; one sample draws one pixel
    a = [to_world(2.5, 8.5), to_world(20.5, 8.5)]
    b = [to_world(10.5, 2.5), to_world(10.5, 14.5)]
    coords = np.array([[a[0], b[0]], [a[1], b[1]]], dtype=np.float32)          # (S = 2, G = 2, 3)
    win = tr.winner_map(coords, cam)
    assert win[8, 10] == 1 and win[8, 9] == 0 and win[8, 2] == 0 and win[8, 20] == 0 and win[2, 10] == 1 and win[14, 10] == 1
    assert int((win == 0).sum()) == 18 and int((win == 1).sum()) == 13
    one = tr.winner_map(coords[:1], cam)
    assert int((one >= 0).sum()) == 2 and one[8, 2] == 0 and one[2, 10] == 1
    assert int((tr.winner_map(coords[:0], cam) >= 0).sum()) == 0
    # a broken sample removes both adjacent segments; an isolated sample between two breaks draws nothing
    nan = [np.nan, 0.0, 0.0]
    far = to_world(float(1 << 20), 4.5)
    track = np.array([[to_world(1.5, 1.5)], [to_world(6.5, 1.5)], [nan], [to_world(9.5, 9.5)], [far], [to_world(3.5, 12.5)],
                      [to_world(8.5, 12.5)]], dtype=np.float32)
    win = tr.winner_map(track, cam)
    assert sorted(zip(*np.nonzero(win >= 0))) == [(1, x) for x in range(1, 7)] + [(12, x) for x in range(3, 9)]
    img = tr.overlay_image(win, np.array([[0.25, 0.5, 0.75]], dtype=np.float32))
    assert img.shape == (H, W, 4) and img[1, 3].tolist() == [0.25, 0.5, 0.75, 1.0] and not img[0].any()
    # w = 0 and w < 0: no w > 0 test; a division by zero is a break
    persp = _cam([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]], W, H)        # p = (x, y, 0, z)
    pts = np.array([[[0.5, 0.5, -2.0]], [[0.5, 0.5, 2.0]], [[0.5, 0.5, 0.0]]], dtype=np.float32)
    ix, iy, ok = tr.pixels(pts, np.asarray(persp.full_proj_transform, dtype=np.float64), W, H)
    assert ok.reshape(-1).tolist() == [True, True, False] and ix.reshape(-1)[:2].tolist() == [12, 20]


def test_new_entry_points_refuse_bad_sizes_and_null_pointers_without_gpu():
    from trase_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(256)           # a non-null pointer that is never dereferenced: every call below returns before the GPU
    proj = (C.c_double * 16)(*([0.0] * 16))
    fps = lib.trase_fps_sample
    assert fps(one, 0, None, 0, None, 1, one, one, one, 0, None) == INVALID
    assert b"1 <= N < 2^31" in lib.trase_last_error()
    assert fps(one, 10, None, 0, None, 0, one, one, one, 0, None) == INVALID
    assert fps(one, 10, None, 0, None, 65537, one, one, one, 0, None) == INVALID
    assert fps(one, 10, None, 10, None, 4, one, one, one, 0, None) == INVALID
    assert fps(one, 10, None, -1, None, 4, one, one, one, 0, None) == INVALID
    for args in ((None, 10, None, 0, None, 4, one, one, one), (one, 10, None, 0, None, 4, None, one, one),
                 (one, 10, None, 0, None, 4, one, None, one), (one, 10, None, 0, None, 4, one, one, None)):
        assert fps(*args, 0, None) == INVALID and b"null pointer" in lib.trase_last_error()
    app = lib.trase_trajectory_append
    assert app(one, 10, one, 0, one, 0, None) == INVALID
    assert app(one, 10, one, 65537, one, 0, None) == INVALID
    assert app(one, -1, one, 4, one, 0, None) == INVALID
    assert app(None, 10, one, 4, one, 0, None) == INVALID and app(one, 10, None, 4, one, 0, None) == INVALID
    assert app(one, 10, one, 4, None, 0, None) == INVALID and b"null pointer" in lib.trase_last_error()
    draw = lib.trase_trajectory_draw
    good = dict(coords=one, S=4, G=8, first=0, cap=4, proj=C.byref(proj), W=64, H=48, colors=one, overlay=one, winner=one)
    order = ("coords", "S", "G", "first", "cap", "proj", "W", "H", "colors", "overlay", "winner")
    for change in (dict(S=-1), dict(S=5), dict(cap=1025, S=1025), dict(G=0), dict(G=65537), dict(first=4), dict(first=-1), dict(W=0),
                   dict(H=0), dict(W=65536, H=32768), dict(proj=None), dict(winner=None), dict(coords=None), dict(colors=None)):
        a = dict(good, **change)
        assert draw(*[a[k] for k in order], 0, None) == INVALID, change
    pres = lib.trase_present_frame
    for h, w, H, W in ((0, 8, 8, 8), (8, 0, 8, 8), (8, 8, 0, 8), (8, 8, 8, 0), (65536, 32768, 8, 8), (8, 8, 65536, 32768)):
        assert pres(one, h, w, 0, H, W, None, None, None, 0.3, one, None, 0, None) == INVALID
    assert b"h * w < 2^31" in lib.trase_last_error()
    assert pres(None, 8, 8, 0, 8, 8, None, None, None, 0.3, one, None, 0, None) == INVALID
    assert pres(one, 8, 8, 0, 8, 8, None, None, None, 0.3, None, None, 0, None) == INVALID
    assert pres(one, 8, 8, 1, 8, 8, None, None, None, 0.3, one, None, 0, None) == INVALID       # depth mode needs minmax
    assert not [n for n, _, _ in _lib.SYMBOLS if n.endswith("_sizes") and ("fps" in n or "traj" in n or "present" in n)]


def test_entry_points_reject_cpu_tensors_and_bad_arguments():
    from trase_amd.trajectory import TrajectoryOverlay, draw_trajectories, farthest_point_sample, present_frame
    cam = _cam(IDENTITY, 32, 16)
    with pytest.raises(RuntimeError, match="GPU only"):
        farthest_point_sample(torch.zeros(10, 3), 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        draw_trajectories(torch.zeros(2, 4, 3), cam)
    with pytest.raises(RuntimeError, match="GPU only"):
        present_frame(torch.zeros(3, 8, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        TrajectoryOverlay(4, 2).select(torch.zeros(10, 3))
    with pytest.raises(RuntimeError, match="select"):
        TrajectoryOverlay(4, 2).update(torch.zeros(10, 3), cam)
    with pytest.raises(ValueError, match="gs_num"):
        TrajectoryOverlay(0, 2)
    with pytest.raises(ValueError, match="samp_num"):
        TrajectoryOverlay(4, 1025)
