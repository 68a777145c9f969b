"""numpy restatement of the segment output and its scores (trase_amd/evaluate.py, trase_amd/csrc/evaluate.hip), in this
repository's own words: test infrastructure, CPU only.

Output of a selection (render.py:344-366): the all-ones render on black is ``alpha = 1 - T_final``; the predicted mask is
``alpha >= threshold`` (a NaN is outside); the cut-out is the image inside the mask and 0 -- 1 on a white background --
outside; ``to8b`` turns both into (H, W, 3) bytes.  Scores (metrics_segmentation.py:33-48, :118-150): counts of the mask
pair, and the squared error of the image pair after both went through ``save_image``'s quantiser.

The two quantisers work on fp32 values with every intermediate rounded to fp32.  They are written here through exact
float64 products (a 24-bit significand times 255 is exact in float64) rounded once to fp32, which is what one fp32
multiplication gives."""
from __future__ import annotations

import math

import numpy as np

RECORD_WORDS = 8
INTER, UNION, EQUAL, PIXELS, SSE, VALUES, _RESERVED, SSIM = range(RECORD_WORDS)


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def to8b(x):
    """render.py:106 for fp32 input: bytes of trunc(fp32(255 * clip(x, 0, 1))); a NaN gives 0."""
    x = _f32(x).astype(np.float64)
    c = np.where(x > 0.0, np.where(x < 1.0, x, 1.0), 0.0)              # a NaN fails x > 0
    return np.floor((255.0 * c).astype(np.float32).astype(np.float64)).astype(np.uint8)


def save8b(x):
    """torchvision's save_image for fp32 input: bytes of trunc(clamp(fp32(fp32(x * 255) + 0.5), 0, 255)); a NaN gives 0."""
    x = _f32(x).astype(np.float64)
    prod = (x * 255.0).astype(np.float32).astype(np.float64)           # exact product, one rounding
    v = (prod + 0.5).astype(np.float32).astype(np.float64)             # exact sum of two fp32 values, one rounding
    return np.where(v > 0.0, np.where(v < 255.0, np.floor(v), 255.0), 0.0).astype(np.uint8)


def segment_output(image, final_T, threshold=0.5, white_background=False):
    """-> dict(object (3,H,W) fp32, pred_mask (H,W) bool, alpha (H,W) fp32, object_u8, pred_mask_u8 (H,W,3) uint8)."""
    image, T = _f32(image), _f32(final_T)
    alpha = (np.float32(1.0) - T).astype(np.float32)
    with np.errstate(invalid="ignore"):
        inside = alpha >= np.float32(threshold)
    obj = np.where(inside[None], image, np.float32(1.0 if white_background else 0.0)).astype(np.float32)
    return dict(object=obj, pred_mask=inside, alpha=alpha, object_u8=np.ascontiguousarray(to8b(obj).transpose(1, 2, 0)),
                pred_mask_u8=np.repeat((inside.astype(np.uint8) * 255)[:, :, None], 3, axis=2))


def gt_bytes(gt_object):
    """The ground-truth object image as (3,H,W) bytes: uint8 input as stored ((3,H,W) or (H,W,3)), fp32 through save8b."""
    g = np.asarray(gt_object)
    if g.dtype == np.uint8:
        return g.transpose(2, 0, 1) if (g.shape[2] == 3 and g.shape[0] != 3) else g
    return save8b(g)


def frame_record(pred_mask=None, gt_mask=None, obj=None, gt_object=None, quantize=True):
    """-> (int64[8] record, float64 unquantised squared error or None) of one frame."""
    rec = np.zeros(RECORD_WORDS, dtype=np.int64)
    sse_float = None
    if gt_mask is not None:
        p, g = np.asarray(pred_mask) != 0, np.asarray(gt_mask) != 0
        rec[INTER], rec[UNION] = np.count_nonzero(p & g), np.count_nonzero(p | g)
        rec[EQUAL], rec[PIXELS] = np.count_nonzero(p == g), p.size
    if gt_object is not None:
        obj = _f32(obj)
        rec[VALUES] = obj.size
        g = np.asarray(gt_object)
        if quantize:
            d = save8b(obj).astype(np.int64) - gt_bytes(g).astype(np.int64)
            rec[SSE] = int((d * d).sum())
        else:
            gf = g.astype(np.float64) if g.dtype != np.uint8 else (gt_bytes(g).astype(np.float32) / np.float32(255.0)).astype(np.float64)
            d = obj.astype(np.float64) - gf
            sse_float = float(np.sum(d * d))
    return rec, sse_float


def compared_pair(obj, gt_object):
    """The quantised pair as the reference reads it back from the files: (3,H,W) fp32, byte / 255."""
    return ((save8b(obj).astype(np.float32) / np.float32(255.0)).astype(np.float32),
            (gt_bytes(gt_object).astype(np.float32) / np.float32(255.0)).astype(np.float32))


def scores(rec, sse_float=None):
    """-> (IoU, accuracy, PSNR in dB) of one record, float64; None where the record holds no such pair."""
    iou = acc = psnr = None
    if rec[PIXELS] > 0:
        iou = 0.0 if rec[UNION] == 0 else int(rec[INTER]) / int(rec[UNION])
        acc = int(rec[EQUAL]) / int(rec[PIXELS])
    if rec[VALUES] > 0:
        mse = (int(rec[SSE]) / (255.0 * 255.0) if sse_float is None else sse_float) / int(rec[VALUES])
        psnr = math.inf if mse == 0.0 else -10.0 * math.log10(mse)
    return iou, acc, psnr
