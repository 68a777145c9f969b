"""ByteFrame at the camera's resolution (trase_amd.frames: ``resolution=``, ``resized``, ``resize_tables``; frame_resize_kernel in
trase_amd/csrc/frames.hip): Pillow's 8-bit bicubic resize, both passes in one launch.

Nothing here uses a tolerance: every frame is compared byte for byte with the numpy restatement (tests/resize_reference.py,
itself compared with ``PIL.Image.resize`` and with the reference's own frames without a GPU), every table entry with the
restatement's tables.

Sizes: the smallest at which each mechanism can go wrong -- one pixel; an enlargement from one pixel; both axes, each axis alone;
exact halves to sixteenths; output widths around the 16-byte pitch and the dword tails; output widths around the 64-column tile
and output heights around every tile height (32, 16, 8, 4), each at a vertical scale at which the host picks that height
(tests/test_resize_reference.py asserts the plan meets these edges); 2028 x 2704 -> 1200 x 1600 once."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import frames_reference as fr
from tests import resize_reference as rr

pytestmark = pytest.mark.gpu

BACKGROUNDS = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.2, 0.5, 0.7)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_resize.npz")

# ((source H, W), (frame H, W))
BASIC = [((1, 1), (1, 1)), ((1, 1), (3, 5)), ((35, 67), (17, 33)), ((35, 67), (13, 20)), ((11, 10), (32, 32)),
         ((100, 203), (100, 101)), ((77, 50), (31, 50))]
FRACTIONS = [((64, 96), (32, 48)), ((64, 96), (16, 24)), ((64, 96), (8, 12)), ((64, 96), (4, 6)), ((64, 96), (64, 6)), ((64, 96), (4, 96))]
PITCH = [((20, 40), (10, w)) for w in (15, 16, 17, 31, 32, 33)]
# heights one below, at and one above a multiple of the tile height, widths 63 / 64 / 65 and 127 / 128 / 129, at vertical scales
# 2, 6, 10 and 16: the host picks 32, 16, 8 and 4 rows there
TILE_EDGES = [((2 * h, int(w * s)), (h, w)) for h, w, s in ((31, 63, 1.69), (32, 64, 2), (33, 65, 0.5), (65, 129, 1.0))] + \
             [((6 * h, int(w * s)), (h, w)) for h, w, s in ((47, 63, 2), (48, 64, 0.7), (49, 65, 3), (33, 127, 1.69))] + \
             [((10 * h, int(w * s)), (h, w)) for h, w, s in ((23, 63, 4), (24, 64, 1.3), (25, 65, 1.0), (17, 128, 2))] + \
             [((16 * h, int(w * s)), (h, w)) for h, w, s in ((11, 63, 16), (12, 64, 8), (13, 65, 16), (10, 129, 1.1))]
SIZES = BASIC + FRACTIONS + PITCH + TILE_EDGES
FULL = ((2028, 2704), (1200, 1600))

_sources = {}


def _source(size):
    """(H, W, 4) uint8: random colours and alphas, a 0 / 255 checkerboard patch (the overshoot reaches both clamps) and a
    constant-255 patch -- built once per size, never modified"""
    if size not in _sources:
        H, W = size
        g = np.random.default_rng(H * 4099 + W)
        rgba = g.integers(0, 256, (H, W, 4), dtype=np.uint8)
        yy, xx = np.mgrid[0:H, 0:W]
        board = (((yy // 8 + xx // 8) & 1) * 255).astype(np.uint8)
        rgba[: H // 2, : W // 2, :3] = board[: H // 2, : W // 2, None]
        rgba[H // 2:, : W // 3, :3] = 255
        _sources[size] = rgba
    return _sources[size]


def _behind_ff(array):
    """The array's bytes on the device with 0xFF in front of and behind them (64 bytes each side, the copy 16-byte aligned)"""
    flat = torch.from_numpy(np.ascontiguousarray(array)).reshape(-1)
    buf = torch.full((flat.numel() + 128,), 0xFF, dtype=torch.uint8, device="cuda")
    buf[64:64 + flat.numel()] = flat.cuda()
    return buf[64:64 + flat.numel()].view(array.shape)


def _want_planes(rgb, dst):
    return torch.from_numpy(fr.planes(rr.resize(rgb, (dst[1], dst[0]))))


def _ids(cases):
    return [f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in cases]


# ---- tables -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [p for p in rr.PLAN if p[0] <= rr.MAX_SHRINK * p[1]], ids=str)
def test_tables_are_the_restatements(pair):
    from trase_amd.frames import resize_tables
    coeffs, bounds = resize_tables(pair[0], pair[1], "cuda")
    want_c, want_b = rr.axis_tables(*pair)
    assert coeffs.dtype == torch.int32 and tuple(coeffs.shape) == want_c.shape and tuple(bounds.shape) == want_b.shape
    assert np.array_equal(bounds.cpu().numpy(), want_b)
    assert np.array_equal(coeffs.cpu().numpy(), want_c)


# ---- every size, every loader -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", SIZES, ids=_ids(SIZES))
def test_resized_frame_is_the_restatement_from_every_source(src, dst):
    from trase_amd.frames import ByteFrame
    rgba = _source(src)
    rgb = np.ascontiguousarray(rgba[..., :3])
    res = (dst[1], dst[0])
    want = _want_planes(rgb, dst).cuda()
    # (H, W, 3) and (H, W, 4) with the alpha dropped; host arrays, host tensors and device tensors with 0xFF around them
    for hwc in (rgb, rgba):
        for source in (hwc, torch.from_numpy(hwc), _behind_ff(hwc)):
            frame = ByteFrame.from_array(source, device="cuda", resolution=res)
            assert frame.shape == (3,) + dst and frame.pitch == fr.pitch_for(dst[1]) and frame.data.is_cuda
            assert torch.equal(frame.data, want), "from_array differs from the restatement (or the padding is not 0)"
    # a source whose first byte is off the dword boundary: the 4-channel loader reads bytes there
    odd = torch.full((rgba.size + 131,), 0xFF, dtype=torch.uint8, device="cuda")
    odd[65:65 + rgba.size] = torch.from_numpy(rgba).reshape(-1).cuda()
    assert torch.equal(ByteFrame.from_array(odd[65:65 + rgba.size].view(rgba.shape), resolution=res).data, want)
    # the composite over three backgrounds, random alpha
    for bg in BACKGROUNDS:
        want_bg = _want_planes(fr.composite(rgba, bg), dst).cuda()
        for source in (rgba, _behind_ff(rgba)):
            got = ByteFrame.from_rgba(source, torch.tensor(bg), device="cuda", resolution=res)
            assert got.shape == (3,) + dst and torch.equal(got.data, want_bg), f"from_rgba over {bg} differs from the restatement"
    # the planes of a resident frame
    resident = ByteFrame.from_array(rgb, device="cuda")
    again = resident.resized(res)
    assert again.shape == (3,) + dst and torch.equal(again.data, want)
    assert torch.equal(resident.resized(res).data, again.data)                      # two runs, identical bits
    assert torch.equal(ByteFrame.from_array(rgb, device="cuda", resolution=res).data, again.data)


@pytest.mark.parametrize("src,dst", SIZES, ids=_ids(SIZES))
def test_nothing_is_written_behind_the_planes(src, dst):
    """The C entry point on the caller's buffers: 0xCD in front of and behind the planes stays, the row padding is written as 0,
    from an interleaved source with 0xFF around it and from planes whose padding and surroundings hold 0xFF"""
    from trase_amd import _lib
    lib = _lib.load()
    rgb = np.ascontiguousarray(_source(src)[..., :3])
    (sH, sW), (H, W) = src, dst
    pitch = fr.pitch_for(W)
    want = _want_planes(rgb, dst).cuda()
    planar = torch.from_numpy(fr.planes(rgb, fill=0xFF)).numpy()
    for source, layout, src_pitch in ((_behind_ff(rgb), 3, 0), (_behind_ff(planar), _lib.FRAME_PLANAR, fr.pitch_for(sW))):
        buf = torch.full((3 * H * pitch + 512,), 0xCD, dtype=torch.uint8, device="cuda")
        out = buf[256:256 + 3 * H * pitch]
        assert out.data_ptr() % 16 == 0
        rc = lib.trase_frame_resize(_lib.ptr(source), sH, sW, layout, src_pitch, None, _lib.ptr(out), H, W, pitch, 0, None)
        assert rc == 0, lib.trase_last_error().decode()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
        assert bool((buf[:256] == 0xCD).all()) and bool((buf[256 + 3 * H * pitch:] == 0xCD).all())


def test_full_size_once():
    from trase_amd.frames import ByteFrame
    src, dst = FULL
    g = np.random.default_rng(7)
    rgba = g.integers(0, 256, src + (4,), dtype=np.uint8)
    rgba[:700, :900, :3] = ((np.add.outer(np.arange(700) // 2, np.arange(900) // 2) & 1) * 255).astype(np.uint8)[..., None]
    bg = BACKGROUNDS[2]
    want = _want_planes(fr.composite(rgba, bg), dst).cuda()
    got = ByteFrame.from_rgba(rgba, bg, device="cuda", resolution=(dst[1], dst[0]))
    assert got.shape == (3,) + dst and torch.equal(got.data, want)


# ---- consistency with the existing paths --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (35, 67), (40, 64)], ids=str)
def test_the_source_size_and_none_keep_the_packed_bits(size):
    from trase_amd.frames import ByteFrame
    rgba = _source(size)
    H, W = size
    want = torch.from_numpy(fr.planes(rgba)).cuda()
    for resolution in (None, (W, H)):
        for source in (rgba, np.ascontiguousarray(rgba[..., :3]), torch.from_numpy(rgba).cuda()):
            assert torch.equal(ByteFrame.from_array(source, device="cuda", resolution=resolution).data, want)
        for bg in BACKGROUNDS:
            today = ByteFrame.from_rgba(rgba, bg, device="cuda")
            assert torch.equal(today.data, torch.from_numpy(fr.planes(fr.composite(rgba, bg))).cuda())
            assert torch.equal(ByteFrame.from_rgba(rgba, bg, device="cuda", resolution=resolution).data, today.data)
    frame = ByteFrame.from_array(rgba, device="cuda")
    assert torch.equal(frame.resized((W, H)).data, want) and frame.resized((W, H)).data.data_ptr() != frame.data.data_ptr()


def test_the_loss_on_a_resized_frame_is_the_loss_on_its_float_frame():
    from trase_amd.frames import ByteFrame
    from trase_amd.losses import photometric_loss
    frame = ByteFrame.from_array(_source((77, 130)), device="cuda", resolution=(65, 33))
    gt = frame.to_float()
    assert gt.shape == (3, 33, 65)
    img = torch.rand(gt.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    results = []
    for target in (frame, gt):
        x = img.clone().requires_grad_(True)
        loss, l1, ss = photometric_loss(x, target, 0.2, with_parts=True)
        loss.backward()
        results.append((loss.detach(), l1, ss, x.grad))
    for a, b in zip(*results):
        assert torch.equal(a, b)


# ---- the fixture: the reference's own frames ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg", ["bg0", "bg1", "bgc"])
def test_golden_frames_bit_for_bit(bg):
    from trase_amd.frames import ByteFrame
    z = np.load(GOLDEN)
    background = {"bg0": BACKGROUNDS[0], "bg1": BACKGROUNDS[1], "bgc": BACKGROUNDS[2]}[bg]
    for W, H in ((17, 33), (13, 20), (70, 134)):
        want = torch.from_numpy(z[f"frame_{bg}_{W}x{H}"]).cuda()
        got = ByteFrame.from_rgba(z["rgba"], background, device="cuda", resolution=(W, H)).to_float()
        assert got.shape == want.shape and torch.equal(got, want)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_a_shrink_above_sixteen_is_refused_without_a_launch():
    from trase_amd import _lib
    from trase_amd.frames import ByteFrame, resize_tables
    lib = _lib.load()
    rgb = torch.zeros((33, 40, 3), dtype=torch.uint8, device="cuda")
    for resolution in ((40, 2), (2, 33), (2, 2)):                      # 33 rows -> 2, 40 columns -> 2
        with pytest.raises(ValueError, match="at most 16"):
            ByteFrame.from_array(rgb, resolution=resolution)
    frame = ByteFrame.from_array(rgb)
    with pytest.raises(ValueError, match="at most 16"):
        frame.resized((2, 33))
    with pytest.raises(ValueError, match="at most 16"):
        resize_tables(33, 2, "cuda")
    out = torch.full((3 * 2 * 48 + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    rc = lib.trase_frame_resize(_lib.ptr(rgb), 33, 40, 3, 0, None, _lib.ptr(out), 2, 40, 48, 0, None)
    assert rc == -1 and b"at most 16" in lib.trase_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0xCD).all())                                    # nothing ran
    assert ByteFrame.from_array(rgb, resolution=(3, 3)).shape == (3, 3, 3)        # 33 -> 3 and 40 -> 3 are within the limit
