"""The 8-bit ground-truth frame without a GPU: the numpy statements of ``tests/frames_reference.py`` against the reference's
expressions (the composite on every (value, alpha) pair, the fixture the reference's own PILtoTorch produced, the black-mask
tap rule against ``F.interpolate`` on the CPU), the host side of ``trase_amd.frames.ByteFrame``, and the argument refusals of
the seven C entry points.  No device is touched: every refused call returns before it selects one."""
import os

import numpy as np
import pytest
import torch

from tests import frames_reference as fr

INVALID, WORKSPACE = -1, -3          # TRASE_ERR_INVALID, TRASE_ERR_WORKSPACE (include/trase_rast.h)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames.npz")
BACKGROUNDS = {"black": (0.0, 0.0, 0.0), "white": (1.0, 1.0, 1.0), "colour": (0.2, 0.5, 0.7)}


def table_image():
    """256 x 256 RGBA: row = value (in all three channels), column = alpha"""
    v, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return np.stack([v, v, v, a], axis=-1)


# ---- the composite rule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg", sorted(BACKGROUNDS))
def test_composite_rule_on_every_value_alpha_pair(bg):
    rgba = table_image()
    background = np.array(BACKGROUNDS[bg], dtype=np.float32)
    norm = rgba / 255.0                                                            # the expressions of train.py:222-226
    over = norm[:, :, :3] * norm[:, :, 3:4] + background * (1 - norm[:, :, 3:4])
    assert over.dtype == np.float64
    want = np.array(over * 255.0, dtype=np.byte).view(np.uint8)
    got = fr.composite(rgba, background)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(got[:, 255], rgba[:, 255, :3])                           # an opaque pixel keeps its value
    # a rounding implementation cannot pass: rint differs from trunc on a large part of the table
    rounded = np.rint(over * 255.0).astype(np.int64).astype(np.uint8)
    assert int((rounded != want).any(axis=-1).sum()) > 20000


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg", ["bg0", "bg1"])
def test_golden_frame_is_the_exact_quotient(bg):
    z = np.load(GOLDEN)
    as_bytes, frame = z[f"bytes_{bg}"], z[f"frame_{bg}"]
    assert as_bytes.dtype == np.uint8 and as_bytes.shape == (67, 35, 4) and frame.dtype == np.float32 and frame.shape == (4, 67, 35)
    got = fr.to_float(as_bytes).transpose(2, 0, 1)
    assert got.dtype == np.float32 and np.array_equal(got, frame)
    assert np.array_equal(fr.composite(z["rgba"], [float(bg[-1])] * 3), as_bytes[..., :3])
    # the black and opaque patch is black over both backgrounds, a pixel that is zero in two channels only is not
    assert fr.black_mask(as_bytes[..., :3].transpose(2, 0, 1))[10:40, 5:20].all()
    assert not fr.black_mask(as_bytes[..., :3].transpose(2, 0, 1))[3, 30]


def test_multiplying_by_the_reciprocal_is_not_the_quotient():
    b = np.arange(256, dtype=np.float32)
    assert int((b * np.float32(1.0 / 255.0) != b / np.float32(255.0)).sum()) == 126
    assert np.array_equal(fr.to_float(np.arange(256, dtype=np.uint8)), (torch.arange(256, dtype=torch.uint8) / 255.0).numpy())


# ---- the black-mask tap rule ------------------------------------------------------------------------------------------------------
def _patchy(H, W, seed):
    g = np.random.default_rng(seed)
    chw = g.integers(0, 256, (3, H, W), dtype=np.uint8)
    black = g.random((H, W)) < 0.55
    black[: H // 2, : W // 3] = True
    chw[:, black] = 0
    two = g.random((H, W)) < 0.2            # zero in two channels only: not black
    chw[0][two] = 0
    chw[1][two] = 0
    chw[2][two] = np.maximum(chw[2][two], 1)
    return chw


@pytest.mark.parametrize("src,dst", [((66, 34), (33, 17)), ((67, 35), (20, 13)), ((10, 11), (32, 32)), ((66, 34), (66, 34)),
                                     ((10, 11), (10, 11)), ((1, 1), (1, 1)), ((1, 1), (3, 2))])
def test_black_mask_tap_rule_is_the_resized_sum(src, dst):
    chw = _patchy(*src, seed=src[0] * 100 + dst[1])
    gt = torch.from_numpy(chw) / 255.0
    resized = torch.nn.functional.interpolate(gt.unsqueeze(0), dst, mode="bilinear").squeeze(0)
    want = (torch.sum(resized, dim=0) == 0).numpy()
    got = fr.black_mask(chw, dst)
    assert got.shape == dst and np.array_equal(got, want)
    assert 0 < int(want.sum()) < want.size or src == (1, 1)
    if src == dst:
        assert np.array_equal(got, fr.black_mask(chw)) and np.array_equal(got, (torch.sum(gt, dim=0) == 0).numpy())


# ---- the host side of ByteFrame ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,pitch", [(1, 16), (15, 16), (16, 16), (17, 32), (35, 48), (1920, 1920), (21857, 21872)])
def test_pitch_is_the_smallest_multiple_of_16(W, pitch):
    from trase_amd.frames import ByteFrame
    assert ByteFrame.pitch_for(W) == pitch == fr.pitch_for(W)


def test_host_array_hands_over_the_bytes_unpermuted():
    from trase_amd.frames import ByteFrame
    g = np.random.default_rng(0)
    for ch in (3, 4):
        hwc = g.integers(0, 256, (5, 7, ch), dtype=np.uint8)
        for source in (hwc, torch.from_numpy(hwc.copy()), np.asfortranarray(hwc), hwc[::-1]):
            src, H, W, c = ByteFrame.host_array(source)
            assert (H, W, c) == (5, 7, ch) and src.dtype == torch.uint8 and src.is_contiguous()
            assert np.array_equal(src.numpy(), np.asarray(source))
        src, *_ = ByteFrame.host_array(hwc)
        assert src.data_ptr() == hwc.ctypes.data                                   # a contiguous array is not copied on the host
    for bad in (hwc.astype(np.int8), hwc.astype(np.float32), hwc[..., :2], hwc[0], np.zeros((0, 4, 3), np.uint8), [[1, 2, 3]]):
        with pytest.raises(ValueError):
            ByteFrame.host_array(bad)
    with pytest.raises(RuntimeError, match="GPU only"):
        ByteFrame.from_array(hwc, device="cpu")
    with pytest.raises(ValueError, match="4"):
        ByteFrame.from_rgba(hwc[..., :3], (0.0, 0.0, 0.0), device="cpu")
    with pytest.raises(ValueError, match="three"):
        ByteFrame.from_rgba(hwc, (0.0, 0.0), device="cpu")


def test_byteframe_refuses_unusable_buffers():
    from trase_amd.frames import ByteFrame
    H, W = 5, 17                                   # pitch 32: 480 bytes
    f = ByteFrame(torch.from_numpy(fr.planes(np.zeros((H, W, 3), np.uint8))), H, W)
    assert f.shape == (3, H, W) and f.pitch == 32 and f.nbytes == 480 and f.dim() == 3
    for data, why in ((torch.zeros(479, dtype=torch.uint8), "480"), (torch.zeros(3 * H * W, dtype=torch.uint8), "480"),
                      (torch.zeros(480, dtype=torch.int8), "uint8"), (torch.zeros(960, dtype=torch.uint8)[::2], "contiguous"),
                      (torch.zeros(496, dtype=torch.uint8)[4:484], "16-byte boundary"), (torch.zeros(3, H, 32, dtype=torch.uint8), "1-d")):
        with pytest.raises(ValueError, match=why):
            ByteFrame(data, H, W)
    with pytest.raises(ValueError):
        ByteFrame(torch.zeros(480, dtype=torch.uint8), 0, W)


def test_from_float_checks_that_the_image_is_bytes():
    from trase_amd.frames import ByteFrame
    exact = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (3, 6, 9), dtype=np.uint8)) / 255.0
    with pytest.raises(RuntimeError, match="GPU only"):          # the check passes; only then is a device asked for
        ByteFrame.from_float(exact)
    off = exact.clone()
    off[1, 2, 3] = 0.3
    with pytest.raises(ValueError, match="1 values are not exactly k / 255"):
        ByteFrame.from_float(off)
    recip = torch.arange(256, dtype=torch.float32).reshape(1, 16, 16).repeat(3, 1, 1) * (1.0 / 255.0)
    with pytest.raises(ValueError, match="378 values"):           # 3 x 126: multiplying by 1 / 255 is not the frame
        ByteFrame.from_float(recip)
    with pytest.raises(RuntimeError, match="GPU only"):
        ByteFrame.from_float(off, check=False)
    with pytest.raises(ValueError):
        ByteFrame.from_float(exact[:2])


def test_mask_black_needs_a_byteframe():
    from trase_amd import losses
    img, gt = torch.zeros(3, 4, 4), torch.zeros(3, 4, 4)
    with pytest.raises(TypeError, match="ByteFrame"):
        losses.photometric_loss(img, gt, 0.2, mask_black=True)
    with pytest.raises(TypeError, match="ByteFrame"):
        losses.l1_ssim(img, gt, mask_black=True)
    with pytest.raises(RuntimeError, match="GPU only"):           # without the flag: the tensor path's own refusal, unchanged
        losses.photometric_loss(img, gt, 0.2)


# ---- argument refusals of the C entry points ----------------------------------------------------------------------------------------
_H, _W, _PITCH = 5, 17, 32
_store = np.zeros(4096, dtype=np.uint8)
_BASE = (_store.ctypes.data + 15) // 16 * 16          # a 16-byte aligned host address: nothing dereferences it in a refused call
_P = _BASE + 1024                                     # any other non-null pointer
_WS = 1 << 20


def _loss_args(photometric, backward):
    args = [("img", _P), ("planes", _BASE), ("H", _H), ("W", _W), ("pitch", _PITCH), ("flags", 0)]
    if photometric:
        args.append(("lambda_dssim", 0.2))
    args += [("g", _P), ("ws", _P), ("ws_bytes", _WS), ("d_img", _P)] if backward else [("out", _P), ("ws", _P), ("ws_bytes", _WS)]
    return args + [("device", 0), ("stream", None)]


ENTRY_POINTS = {
    "trase_frame_pack": [("hwc", _P), ("H", _H), ("W", _W), ("channels", 4), ("background", None), ("planes", _BASE), ("pitch", _PITCH),
                         ("device", 0), ("stream", None)],
    "trase_frame_unpack": [("planes", _BASE), ("H", _H), ("W", _W), ("pitch", _PITCH), ("chw", _P), ("device", 0), ("stream", None)],
    "trase_frame_black_mask": [("planes", _BASE), ("H", _H), ("W", _W), ("pitch", _PITCH), ("h", 3), ("w", 4), ("mask", _P), ("device", 0),
                               ("stream", None)],
    "trase_loss_l1_ssim_forward_u8": _loss_args(False, False),
    "trase_loss_l1_ssim_backward_u8": _loss_args(False, True),
    "trase_loss_photometric_forward_u8": _loss_args(True, False),
    "trase_loss_photometric_backward_u8": _loss_args(True, True),
}
_POINTERS = {"hwc", "planes", "chw", "mask", "img", "g", "ws", "d_img", "out"}


def _refusals(name):
    """(description, argument overrides, return code) of every call the entry point must refuse"""
    import ctypes as C
    names = [k for k, _ in ENTRY_POINTS[name]]
    cases = [(f"null {k}", {k: None}, INVALID) for k in names if k in _POINTERS]
    cases += [("H = 0", {"H": 0}, INVALID), ("W = 0", {"W": 0}, INVALID), ("H < 0", {"H": -3}, INVALID),
              ("pitch below W", {"pitch": 16}, INVALID), ("pitch no multiple of 16", {"pitch": 24}, INVALID),
              ("pitch = W", {"pitch": _W}, INVALID), ("pitch = 0", {"pitch": 0}, INVALID),
              ("misaligned planes", {"planes": _BASE + 4}, INVALID), ("misaligned planes by one", {"planes": _BASE + 1}, INVALID)]
    if name == "trase_frame_pack":
        bg = (C.c_float * 3)(0.0, 0.5, 1.0)
        cases += [("2 channels", {"channels": 2}, INVALID), ("5 channels", {"channels": 5}, INVALID), ("0 channels", {"channels": 0}, INVALID),
                  ("a background with 3 channels", {"channels": 3, "background": bg}, INVALID)]
    if name == "trase_frame_black_mask":
        cases += [("h = 0", {"h": 0}, INVALID), ("w = 0", {"w": 0}, INVALID)]
    if "ws_bytes" in names:
        import ctypes
        from trase_amd import _lib
        need = ctypes.c_size_t()
        assert _lib.load().trase_loss_sizes(3, _H, _W, ctypes.byref(need)) == 0
        cases += [("workspace one byte short", {"ws_bytes": need.value - 1}, WORKSPACE), ("workspace of 0 bytes", {"ws_bytes": 0}, WORKSPACE),
                  ("unknown flag", {"flags": 2}, INVALID)]
    if "lambda_dssim" in names and "out" in names:
        cases.append(("lambda above 1", {"lambda_dssim": 1.5}, INVALID))
    return cases


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_points_refuse_bad_arguments(name):
    from trase_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, name)
    assert len(ENTRY_POINTS[name]) == len(fn.argtypes)
    seen = 0
    for what, over, code in _refusals(name):
        args = [over.get(k, v) for k, v in ENTRY_POINTS[name]]
        rc = fn(*args)
        msg = lib.trase_last_error().decode()
        assert rc == code, f"{name} ({what}): returned {rc}, {msg!r}"
        assert name + ":" in msg, f"{name} ({what}): the message {msg!r} does not name the function"
        seen += 1
    assert seen >= 11


def test_there_are_seven_entry_points_and_all_are_bound():
    from trase_amd import _lib
    bound = {n for n, _, _ in _lib.SYMBOLS}
    assert len(ENTRY_POINTS) == 7 and set(ENTRY_POINTS) <= bound
