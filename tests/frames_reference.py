"""TEST INFRASTRUCTURE ONLY -- the 8-bit ground-truth frame (``trase_amd.frames.ByteFrame``) restated in numpy:

* ``composite``: the RGBA-over-background rule of train.py:221-228 as ONE statement per channel,
  ``trunc(((v / 255.0) * (a / 255.0) + bg * (1 - a / 255.0)) * 255.0)`` in float64, the fp32 background promoted to double, the
  result modulo 256 (numpy's conversion to ``np.byte`` truncates toward zero and keeps the low eight bits).
* ``to_float``: ``float32(b) / float32(255)``, the value ``torch.from_numpy(bytes) / 255.0`` gives (PILtoTorch).
* ``planes``: the planar buffer -- three planes of H rows, ``pitch`` bytes apart, ``pitch`` the smallest multiple of 16 >= W.
* ``black_mask``: ``r | g | b == 0``; at another size, the tap rule: a destination pixel is black exactly when every bilinear tap
  of non-zero weight (ATen's taps, ``feature_resample_reference.axis_table``) is black.
"""
import numpy as np

from tests.feature_resample_reference import axis_table


def composite(rgba, bg):
    """(H, W, 4) uint8, three background values -> (H, W, 3) uint8."""
    rgba = np.asarray(rgba)
    assert rgba.dtype == np.uint8 and rgba.shape[-1] == 4
    bg = np.asarray(bg, dtype=np.float32).astype(np.float64).reshape(3)
    v = rgba[..., :3].astype(np.float64) / 255.0
    a = rgba[..., 3:4].astype(np.float64) / 255.0
    arr = v * a + bg * (1.0 - a)
    return (np.trunc(arr * 255.0).astype(np.int64) & 255).astype(np.uint8)


def to_float(b):
    return np.asarray(b).astype(np.float32) / np.float32(255.0)


def pitch_for(W):
    return (W + 15) // 16 * 16


def planes(hwc, fill=0):
    """(H, W, 3 | 4) uint8 -> the 1-d planar buffer (a fourth channel is dropped; the padding holds ``fill``)."""
    hwc = np.asarray(hwc)
    H, W = hwc.shape[:2]
    out = np.full((3, H, pitch_for(W)), fill, dtype=np.uint8)
    out[:, :, :W] = hwc[..., :3].transpose(2, 0, 1)
    return out.reshape(-1)


def black_mask(chw, size=None):
    """(3, H, W) uint8 -> (h, w) bool."""
    chw = np.asarray(chw)
    black = (chw[0] | chw[1] | chw[2]) == 0
    if size is None:
        return black
    h, w = size
    y0, y1, hl0, hl1 = axis_table(chw.shape[1], h)
    x0, x1, wl0, wl1 = axis_table(chw.shape[2], w)
    out = np.ones((h, w), dtype=bool)
    for ys, hl in ((y0, hl0), (y1, hl1)):
        for xs, wl in ((x0, wl0), (x1, wl1)):
            used = (hl != 0)[:, None] & (wl != 0)[None, :]
            out &= ~used | black[ys[:, None], xs[None, :]]
    return out
