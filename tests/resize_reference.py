"""TEST INFRASTRUCTURE ONLY -- Pillow's 8-bit bicubic resize (``Image.resize(size)`` of a mode "RGB" image: default filter
BICUBIC, no ``box``, no ``reducing_gap``) restated in numpy, and the host restatement of the kernel's tile choice.

Per axis, for input size ``in`` and output size ``out``: ``scale = in / out``, ``filterscale = max(scale, 1)``,
``support = 2 * filterscale``, ``ksize = int(ceil(support)) * 2 + 1``, ``ss = 1 / filterscale``; per output index ``xx``:
``center = (xx + 0.5) * scale``, ``xmin = max(int(center - support + 0.5), 0)``, ``xmax = min(int(center + support + 0.5), in)``,
``n = xmax - xmin``, ``w[x] = bicubic(((x + xmin) - center + 0.5) * ss)``, ``ww`` their sum IN TAP ORDER, ``k[x] = w[x] / ww``, the
integer coefficient ``int(k * 2^22 -+ 0.5)`` (toward zero).  One pass is
``clamp(((1 << 21) + sum coeff[x] * byte[xmin + x]) >> 22, 0, 255)``; the horizontal pass runs first, into bytes; an axis whose
size does not change is skipped.  Everything is float64 / integer arithmetic, each operation rounded on its own.

``axis_tables_scalar`` is the statement above one value at a time (Python floats are C doubles); ``axis_tables`` is the same
sequence of operations on arrays and is what the image functions use."""
import math

import numpy as np

PRECISION_BITS = 22
MAX_SHRINK = 16                       # what the kernel supports per axis: in <= 16 * out (ksize <= 65)

# (in, out): the scales 1 / 3.2, 1 / 2, just below and above 1, 1.69, 2, 4, 8 and exactly 16, out = 1, in = 1, and the odd sizes of
# the image cases
PLAN = [(10, 32), (16, 32), (40, 41), (40, 39), (2704, 1600), (2028, 1200), (1352, 800), (270, 135), (480, 240), (64, 16), (64, 8),
        (64, 4), (1600, 100), (16, 1), (9, 1), (1, 1), (1, 3), (1, 5), (35, 17), (67, 33), (35, 13), (67, 20), (11, 32), (203, 101),
        (77, 31), (9, 64), (9, 3), (1014, 600), (33, 32), (31, 32), (100, 7), (37, 37)]


def ksize_for(in_size, out_size):
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    return int(math.ceil(2.0 * filterscale)) * 2 + 1


def _bicubic(t):
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def axis_tables_scalar(in_size, out_size):
    """-> (coeffs (out, ksize) int32, zero beyond n; bounds (out, 2) int32 of (xmin, n))"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    coeffs = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [_bicubic(((x + xmin) - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            k = w[x] / ww if ww != 0.0 else w[x]
            coeffs[xx, x] = int(k * 4194304.0 - 0.5) if k < 0 else int(k * 4194304.0 + 0.5)
        bounds[xx] = (xmin, n)
    return coeffs, bounds


def axis_tables(in_size, out_size):
    """The same operations on arrays: one output index per row, the taps added to ``ww`` one column at a time, in tap order."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    a = -0.5
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    t = np.abs(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    near = ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    far = (((t - 5) * t + 8) * t - 4) * a
    w = np.where(t < 1.0, near, np.where(t < 2.0, far, 0.0))
    w = np.where(x < n[:, None], w, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for j in range(ksize):                       # in tap order (the taps beyond n add +0.0, which changes nothing: ww is never -0.0)
        ww = ww + w[:, j]
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(ww[:, None] != 0.0, w / ww[:, None], w)
    q = np.where(k < 0, np.trunc(k * 4194304.0 - 0.5), np.trunc(k * 4194304.0 + 0.5))
    coeffs = np.where(x < n[:, None], q, 0.0).astype(np.int32)
    return coeffs, np.stack([xmin, n], axis=1).astype(np.int32)


def abs_coeff_sum(coeffs):
    return int(np.abs(coeffs.astype(np.int64)).sum(axis=1).max())


def _pass(img, out_size, axis):
    """One pass along ``axis`` (0 or 1) of an (H, W, C) uint8 array."""
    coeffs, bounds = axis_tables(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)                        # (in, other, C)
    acc = np.full((out_size,) + src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for j in range(coeffs.shape[1]):
        idx = np.minimum(bounds[:, 0].astype(np.int64) + j, src.shape[0] - 1)       # (beyond n the coefficient is 0)
        acc += coeffs[:, j].astype(np.int64)[:, None, None] * src[idx]
    assert np.abs(acc).max() < 2 ** 31
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize(hwc, resolution):
    """(H, W, 3) uint8, resolution = (W', H') as PILtoTorch takes it -> (H', W', 3) uint8, the bytes of
    ``np.array(Image.fromarray(hwc, "RGB").resize(resolution))``."""
    hwc = np.asarray(hwc)
    assert hwc.dtype == np.uint8 and hwc.ndim == 3 and hwc.shape[2] == 3
    W, H = int(resolution[0]), int(resolution[1])
    out = hwc
    if W != hwc.shape[1]:
        out = _pass(out, W, 1)
    if H != hwc.shape[0]:
        out = _pass(out, H, 0)
    return np.ascontiguousarray(out)


def camera_resolution(orig_w, orig_h, resolution=-1, resolution_scale=1.0):
    """(W, H) of utils/camera_utils.py:30-48, restated"""
    if resolution in [1, 2, 4, 8]:
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


# ---- the kernel's tile choice, restated (trase_amd/csrc/frames.hip: resize_plan) ------------------------------------------------
TILE_W = 64
TILE_HEIGHTS = (32, 16, 8, 4)
INTER_ROWS = 128                      # rows of horizontally resampled bytes a workgroup keeps
STAGE_PIXELS = 3072                   # source pixels staged per batch of rows


def tile_span(in_size, out_size, tile):
    """The largest number of source indices the taps of one tile of ``tile`` outputs span (``tile`` itself where the axis is
    skipped)."""
    if in_size == out_size:
        return min(tile, out_size)
    _, b = axis_tables(in_size, out_size)
    lo = b[::tile, 0].astype(np.int64)
    last = np.minimum(np.arange(0, out_size, tile) + tile, out_size) - 1
    hi = (b[last, 0] + b[last, 1]).astype(np.int64)
    return int((hi - lo).max())


def tile_height(in_h, out_h):
    """The largest tile height whose span of source rows fits INTER_ROWS"""
    for th in TILE_HEIGHTS:
        if tile_span(in_h, out_h, th) <= INTER_ROWS:
            return th
    raise AssertionError("no tile height fits: the shrink is above 16")
