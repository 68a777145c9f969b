"""numpy restatement of the two launches around ``render_layers``' rasterizer pass (trase_amd/layers.py,
trase_amd/csrc/layers.hip), in this repository's own words: test infrastructure, CPU only.

Pack: L tables of (P, 3) fp32 become one (P, 32) fp32 block, row i = [t0[i], t1[i], ..., 0 ... 0].
Finish: ``plane[3l + c] = fma(T, bg[c], plane[3l + c])`` for l < L, one rounding.  numpy has no fused multiply-add, so the rule
is stated for the backgrounds where the product is exact: ``bg[c]`` 0 or 1 (black, white).  There ``T * bg`` is +0 or T itself
and the fused operation is a single fp32 addition (which leaves every plane value but -0.0 as it is when ``bg`` is 0).
The 8-bit frames are ``to8b`` of tests/evaluate_reference.py, transposed to (H, W, 3)."""
from __future__ import annotations

import numpy as np

from tests.evaluate_reference import to8b

FEATURE_CHANNELS = 32
MAX_LAYERS = 10


def pack(tables) -> np.ndarray:
    """-> (P, 32) fp32: the tables side by side, the remaining columns +0.0."""
    tables = [np.asarray(t, dtype=np.float32) for t in tables]
    assert 1 <= len(tables) <= MAX_LAYERS
    P = tables[0].shape[0]
    out = np.zeros((P, FEATURE_CHANNELS), dtype=np.float32)
    for l, t in enumerate(tables):
        assert t.shape == (P, 3)
        out[:, 3 * l:3 * l + 3] = t
    return out


def finish(planes, final_T, bg, L: int) -> np.ndarray:
    """-> the (n >= 3L, H, W) planes after the background step; planes >= 3L are returned as they came."""
    planes = np.array(planes, dtype=np.float32, copy=True)
    T = np.asarray(final_T, dtype=np.float32)
    assert np.isfinite(T).all()
    for l in range(L):
        for c in range(3):
            b = np.float32(bg[c])
            if b != 0 and b != 1:
                raise ValueError("the restatement covers bg in {0, 1}: the product T * bg must be exact")
            planes[3 * l + c] = ((T * b).astype(np.float32) + planes[3 * l + c]).astype(np.float32)
    return planes


def frames_u8(x) -> np.ndarray:
    """(3, H, W) fp32 -> (H, W, 3) uint8 (render.py:106)."""
    return np.ascontiguousarray(to8b(x).transpose(1, 2, 0))
