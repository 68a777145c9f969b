"""ByteFrame at the camera's resolution without a GPU: the numpy restatement of Pillow's bicubic resize
(``tests/resize_reference.py``) -- its scalar and its vectorised table builder against each other, the int32 premise of the
accumulator, the images against ``PIL.Image.resize`` itself where PIL imports and against the frames the reference's own
statements produced (tests/golden/frame_resize.npz) -- then the host side: ``camera_resolution`` against the sizes the reference's
``loadCam`` statements computed, the restated tile choice against the edges the GPU plan must meet, and every refusal of the two C
entry points and of the Python arguments.  No device is touched: every refused call returns before it selects one."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import frames_reference as fr
from tests import resize_reference as rr

INVALID = -1                          # TRASE_ERR_INVALID (include/trase_rast.h)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_resize.npz")
BACKGROUNDS = {"bg0": (0.0, 0.0, 0.0), "bg1": (1.0, 1.0, 1.0), "bgc": (0.2, 0.5, 0.7)}

# ((H, W) -> (H', W')) of the comparison with Pillow
PIL_CASES = [((35, 67), (17, 33)), ((35, 67), (13, 20)), ((11, 10), (32, 32)), ((270, 480), (135, 240)), ((100, 203), (100, 101)),
             ((77, 50), (31, 50)), ((64, 64), (1, 1)), ((9, 9), (64, 3)), ((1014, 1352), (600, 800)), ((40, 40), (41, 39))]
CONTENTS = ["random", "checker", "white"]


def _content(size, kind):
    H, W = size
    if kind == "random":
        return np.random.default_rng(H * 31 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((H, W, 3), 255, dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    board = (((yy // 8 + xx // 8) & 1) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([board, 255 - board, board], axis=-1))


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
def test_the_plan_holds_the_scales_it_must():
    scales = {i / o for i, o in rr.PLAN}
    for s in (10 / 32, 0.5, 2.0, 4.0, 8.0, 16.0, 1.69):
        assert s in scales, s
    assert any(0.95 < s < 1.0 for s in scales) and any(1.0 < s < 1.05 for s in scales)
    assert any(o == 1 and i > 1 for i, o in rr.PLAN) and any(i == 1 and o > 1 for i, o in rr.PLAN)
    assert all(i <= rr.MAX_SHRINK * o for i, o in rr.PLAN)


@pytest.mark.parametrize("pair", rr.PLAN, ids=str)
def test_scalar_and_vectorised_tables_agree_and_fit_int32(pair):
    in_size, out_size = pair
    cs, bs = rr.axis_tables_scalar(in_size, out_size)
    cv, bv = rr.axis_tables(in_size, out_size)
    assert cs.shape == cv.shape == (out_size, rr.ksize_for(in_size, out_size)) and np.array_equal(cs, cv) and np.array_equal(bs, bv)
    assert (bv[:, 0] >= 0).all() and (bv[:, 1] >= 1).all() and (bv[:, 0] + bv[:, 1] <= in_size).all() and (bv[:, 1] <= cv.shape[1]).all()
    assert (np.diff(bv[:, 0]) >= 0).all() and (np.diff(bv[:, 0] + bv[:, 1]) >= 0).all()       # a tile's span: first to last index
    assert cv.shape[1] <= 65
    # the accumulator: 2^21 + sum coeff * byte stays inside int32 whatever the bytes are
    assert 255 * rr.abs_coeff_sum(cv) + (1 << 21) < 1 << 31
    assert (np.abs(cv.astype(np.int64).sum(axis=1) - (1 << 22)) <= cv.shape[1]).all()           # the rows sum to one, up to rounding


# ---- the images ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("src,dst", PIL_CASES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in PIL_CASES])
def test_restatement_is_pillow_byte_for_byte(src, dst, kind):
    Image = pytest.importorskip("PIL.Image")
    hwc = _content(src, kind)
    want = np.array(Image.fromarray(hwc, "RGB").resize((dst[1], dst[0])))
    got = rr.resize(hwc, (dst[1], dst[0]))
    assert got.dtype == np.uint8 and got.shape == dst + (3,) and np.array_equal(got, want)


def test_the_checkerboard_reaches_both_clamps():
    """The bicubic overshoot of a 0 / 255 board leaves [0, 255] on both sides before the clamp, in each pass"""
    hwc = _content((35, 67), "checker")
    for axis, out_size in ((1, 33), (0, 17), (1, 134)):
        coeffs, bounds = rr.axis_tables(hwc.shape[axis], out_size)
        src = np.moveaxis(hwc, axis, 0).astype(np.int64)
        acc = np.full((out_size,) + src.shape[1:], 1 << 21, dtype=np.int64)
        for j in range(coeffs.shape[1]):
            acc += coeffs[:, j].astype(np.int64)[:, None, None] * src[np.minimum(bounds[:, 0] + j, src.shape[0] - 1)]
        assert (acc >> 22).min() < 0 and (acc >> 22).max() > 255
    out = rr.resize(hwc, (33, 17))
    assert out.min() == 0 and out.max() == 255


def test_an_unchanged_axis_is_skipped():
    hwc = _content((40, 40), "random")
    assert np.array_equal(rr.resize(hwc, (40, 40)), hwc)
    assert np.array_equal(rr.resize(hwc, (20, 40)), rr._pass(hwc, 20, 1))
    assert np.array_equal(rr.resize(hwc, (40, 20)), rr._pass(hwc, 20, 0))
    assert np.array_equal(rr.resize(hwc, (20, 20)), rr._pass(rr._pass(hwc, 20, 1), 20, 0))     # horizontal first, into bytes
    assert not np.array_equal(rr.resize(hwc, (20, 20)), rr._pass(rr._pass(hwc, 20, 0), 20, 1))


@pytest.mark.parametrize("bg", sorted(BACKGROUNDS))
def test_golden_frames_are_the_restatement(bg):
    z = np.load(GOLDEN)
    rgba = z["rgba"]
    assert rgba.shape == (67, 35, 4) and (rgba[..., 3] == 255).all()
    rgb = fr.composite(rgba, BACKGROUNDS[bg])
    assert np.array_equal(rgb, rgba[..., :3])                                      # opaque: every background gives the colours
    for W, H in ((17, 33), (13, 20), (70, 134)):
        frame = z[f"frame_{bg}_{W}x{H}"]
        assert frame.dtype == np.float32 and frame.shape == (3, H, W)
        got = rr.resize(rgb, (W, H))
        assert np.array_equal(fr.to_float(got).transpose(2, 0, 1), frame)
        assert got.min() == 0 and got.max() == 255


# ---- camera_resolution --------------------------------------------------------------------------------------------------------------
def test_camera_resolution_is_loadcams():
    from trase_amd.frames import camera_resolution
    z = np.load(GOLDEN)
    cams, scales, sizes = z["cameras"], z["camera_scales"], z["camera_sizes"]
    assert len(cams) == len(scales) == len(sizes) >= 20
    seen = set()
    for (w, h, r), s, (W, H) in zip(cams.tolist(), scales.tolist(), sizes.tolist()):
        assert camera_resolution(w, h, r, s) == (W, H) == rr.camera_resolution(w, h, r, s), (w, h, r, s)
        if (w, h, s) == (2704, 2028, 1.0):
            seen.add(r)
    assert seen == {-1, 1, 2, 4, 8, 800}
    assert camera_resolution(2704, 2028) == (1600, 1200) and camera_resolution(1352, 1014) == (1352, 1014)
    # widths whose quotient ends in .5: Python's round goes to the even neighbour
    assert camera_resolution(1001, 751, 2) == (500, 376) and camera_resolution(1003, 753, 2) == (502, 376)
    assert any(r in (2, 4, 8) and 2 * (w % r) == r for (w, h, r) in cams.tolist())


# ---- the tile choice ----------------------------------------------------------------------------------------------------------------
def test_tile_choice_and_the_edges_of_the_gpu_plan():
    from tests import test_gpu_frame_resize as g
    # the span bound behind INTER_ROWS: at a shrink of exactly 16 four rows still fit, and 64 columns fit the stage
    for out in (4, 5, 64, 100):
        assert rr.tile_span(16 * out, out, 4) <= 3 * 16 + 66 <= rr.INTER_ROWS
        assert rr.tile_span(16 * out, out, rr.TILE_W) <= 63 * 16 + 66 <= rr.STAGE_PIXELS
    picked = {}
    for (sH, sW), (H, W) in g.SIZES + [g.FULL]:
        assert sH <= rr.MAX_SHRINK * H and sW <= rr.MAX_SHRINK * W
        th = rr.tile_height(sH, H)
        picked.setdefault(th, []).append((H, W))
    assert sorted(picked) == sorted(rr.TILE_HEIGHTS)
    for th, sizes in picked.items():
        heights, widths = {h for h, _ in sizes}, {w for _, w in sizes}
        # more than one tile, and an extent below, at and above a multiple of the tile, in both directions
        assert any(h % th == th - 1 for h in heights), th
        assert any(h >= th and h % th == 0 for h in heights), th
        assert any(h > th and h % th == 1 for h in heights), th
        assert {63, 64, 65} <= widths, th
    widths = {W for _, (_, W) in g.SIZES}
    assert {15, 16, 17, 31, 32, 33, 127, 128, 129} <= widths
    sizes = set(g.SIZES)
    for case in (((1, 1), (1, 1)), ((1, 1), (3, 5)), ((35, 67), (17, 33)), ((35, 67), (13, 20)), ((11, 10), (32, 32))):
        assert case in sizes
    assert any(s[0] == d[0] and s[1] != d[1] for s, d in sizes) and any(s[1] == d[1] and s[0] != d[0] for s, d in sizes)
    for f in (2, 4, 8, 16):
        assert any(s[0] == f * d[0] and s[1] == f * d[1] for s, d in sizes), f
    assert g.FULL == ((2028, 2704), (1200, 1600))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
_store = np.zeros(4096, dtype=np.uint8)
_BASE = (_store.ctypes.data + 15) // 16 * 16          # a 16-byte aligned host address: nothing dereferences it in a refused call
_P = _BASE + 1024
PLANAR = 1                                            # TRASE_FRAME_PLANAR

RESIZE_ARGS = [("src", _P), ("src_H", 10), ("src_W", 34), ("src_layout", 4), ("src_pitch", 0), ("background", None), ("planes", _BASE),
               ("H", 5), ("W", 17), ("pitch", 32), ("device", 0), ("stream", None)]
TABLE_ARGS = [("in", 35), ("out", 17), ("coeffs", _P), ("bounds", _P), ("device", 0), ("stream", None)]


def _call(name, template, over):
    from trase_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, name)
    assert len(template) == len(fn.argtypes)
    rc = fn(*[over.get(k, v) for k, v in template])
    return rc, lib.trase_last_error().decode()


def test_frame_resize_refuses_bad_arguments():
    bg = (C.c_float * 3)(0.0, 0.5, 1.0)
    cases = [("null src", {"src": None}), ("null planes", {"planes": None}),
             ("layout 0", {"src_layout": 0}), ("layout 2", {"src_layout": 2}), ("layout 5", {"src_layout": 5}),
             ("a background with 3 channels", {"src_layout": 3, "background": bg}),
             ("a background with planes", {"src_layout": PLANAR, "src_pitch": 48, "background": bg}),
             ("src_H = 0", {"src_H": 0}), ("src_W = 0", {"src_W": 0}), ("src_H < 0", {"src_H": -2}),
             ("planar pitch below src_W", {"src_layout": PLANAR, "src_pitch": 32}), ("planar pitch 0", {"src_layout": PLANAR}),
             ("H = 0", {"H": 0}), ("W = 0", {"W": 0}), ("H < 0", {"H": -3}),
             ("pitch below W", {"pitch": 16}), ("pitch no multiple of 16", {"pitch": 24}), ("pitch = W", {"pitch": 17}), ("pitch = 0", {"pitch": 0}),
             ("misaligned planes", {"planes": _BASE + 4}), ("misaligned planes by one", {"planes": _BASE + 1}),
             ("rows shrink by more than 16", {"src_H": 81}), ("columns shrink by more than 16", {"src_W": 273}),
             ("both shrink by more than 16", {"src_H": 1000, "src_W": 1000})]
    for what, over in cases:
        rc, msg = _call("trase_frame_resize", RESIZE_ARGS, over)
        assert rc == INVALID, f"{what}: returned {rc}, {msg!r}"
        assert "trase_frame_resize:" in msg, f"{what}: the message {msg!r} does not name the function"
    rc, msg = _call("trase_frame_resize", RESIZE_ARGS, {"src_H": 81})
    assert "at most 16" in msg


def test_resize_tables_entry_refuses_bad_arguments():
    for what, over in (("null coeffs", {"coeffs": None}), ("null bounds", {"bounds": None}), ("in = 0", {"in": 0}), ("out = 0", {"out": 0}),
                       ("in < 0", {"in": -1}), ("a shrink above 16", {"in": 273})):
        rc, msg = _call("trase_selftest_resize_tables", TABLE_ARGS, over)
        assert rc == INVALID, f"{what}: returned {rc}, {msg!r}"
        assert "trase_selftest_resize_tables:" in msg


def test_python_arguments_are_refused_before_a_device_is_asked_for():
    from trase_amd.frames import ByteFrame, resize_tables
    rgba = np.zeros((33, 40, 4), dtype=np.uint8)
    for bad in ((0, 5), (5, 0), (-1, 5), (5,), (1, 2, 3), 7, "ab", (None, 3)):
        with pytest.raises(ValueError, match="resolution"):
            ByteFrame.from_array(rgba, device="cpu", resolution=bad)
        with pytest.raises(ValueError, match="resolution"):
            ByteFrame.from_rgba(rgba, (0.0, 0.0, 0.0), device="cpu", resolution=bad)
    for resolution in ((40, 2), (2, 33), (2, 2)):
        with pytest.raises(ValueError, match="at most 16"):
            ByteFrame.from_array(rgba, device="cpu", resolution=resolution)
        with pytest.raises(ValueError, match="at most 16"):
            ByteFrame.from_rgba(rgba, (0.0, 0.0, 0.0), device="cpu", resolution=resolution)
    with pytest.raises(ValueError, match="4"):
        ByteFrame.from_rgba(rgba[..., :3], (0.0, 0.0, 0.0), device="cpu", resolution=(20, 17))
    with pytest.raises(RuntimeError, match="GPU only"):                              # a valid request: only then is a device asked for
        ByteFrame.from_array(rgba, device="cpu", resolution=(20, 17))
    with pytest.raises(RuntimeError, match="GPU only"):
        ByteFrame.from_rgba(rgba, (0.0, 0.0, 0.0), device="cpu", resolution=(3, 3))
    host = ByteFrame(torch.from_numpy(fr.planes(rgba)), 33, 40)
    with pytest.raises(RuntimeError, match="GPU only"):
        host.resized((20, 17))
    for bad, why in (((0, 1), "at least 1"), ((1, 0), "at least 1"), ((33, 2), "at most 16")):
        with pytest.raises(ValueError, match=why):
            resize_tables(bad[0], bad[1], "cuda")
    with pytest.raises(RuntimeError, match="GPU only"):
        resize_tables(35, 17, "cpu")


def test_the_new_entry_points_are_declared_and_bound():
    from trase_amd import _lib
    bound = {n for n, _, _ in _lib.SYMBOLS}
    assert {"trase_frame_resize", "trase_selftest_resize_tables"} <= bound
    lib = _lib.load()
    assert hasattr(lib, "trase_frame_resize") and hasattr(lib, "trase_selftest_resize_tables")
    assert _lib.FRAME_PLANAR == PLANAR
