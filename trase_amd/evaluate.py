"""Segment output and scoring on the device (trase_amd/csrc/evaluate.hip): what the reference writes for a selection and the
scores it publishes from those files.

``render_segment`` is render.py:344-366 (repeated at :380-395; gui.py's ``render_set``): the reference rasterises the selection
with ``override_color = ones`` on black, binarises at 0.5, takes ``mean(axis=0).bool()``, rasterises the selection again
for its RGB, blanks the outside and turns both images into 8-bit frames on the host.  An all-ones render on black is
``sum(alpha_i T_i) = 1 - T_final``, which the compositing kernels already hold per pixel, so here it is ONE fused
``render(mask=)`` forward (run with its transmittance kept) and ONE launch that reads the image planes and ``final_T``.

``FrameScores`` collects what metrics_segmentation.py:33-48 and :118-150 compute from the written files -- IoU and pixel
accuracy of the predicted mask, PSNR and SSIM of the cut-out against the benchmark's object image -- in a small device
buffer, one record per frame, read back ONCE by ``result()``.  ``segment_scores`` / ``image_scores`` score images a caller
already has with the same kernel.  With ``FrameScores(..., lpips=net)`` (an ``LPIPSVGG``, trase_amd/lpips.py) the frame's
LPIPS (``lpips(render, gt, net_type='vgg')``, metrics_segmentation.py:118-165) goes into the same record.

Deliberate deviations: the mask comes from ``1 - T_final`` and not from a second render; a ground-truth
mask is "non-zero = object"; a NaN pixel is outside the mask and 0 in the 8-bit frames.

Only CUDA tensors are accepted: there is no CPU path."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .rasterizer import _stream
from .segment import _device_index

RECORD_WORDS = 8            # TRASE_EVAL_RECORD_WORDS
PARTIAL_SLOTS = 2048        # TRASE_EVAL_MAX_BLOCKS
# words of a frame's record
INTER, UNION, EQUAL, PIXELS, SSE, VALUES, LPIPS, SSIM = range(RECORD_WORDS)
GT_NONE, GT_F32_CHW, GT_U8_CHW, GT_U8_HWC = range(4)


def scores_from_records(records, sse_float=None, *, quantize: bool = True, ssim: bool = True, lpips: bool = False) -> dict:
    """The scores of metrics_segmentation.py from (n, 8) int64 records (host), in float64.

    Per frame: ``IOU = inter / union`` (0 when the union is empty, ``compute_iou``), ``ACC = equal / pixels``
    (``compute_acc``), ``PSNR = 20 log10(1 / sqrt(mse))`` over all 3 H W values (``utils/image_utils.psnr``; ``inf`` for
    identical images) with ``mse = sse / 255^2 / values`` for the quantised pair or ``sse_float / values`` (``sse_float``: one
    float64 per frame) for the unquantised one, ``SSIM`` = the float64 stored in the record.  A frame that recorded no mask
    pair (no image pair) has ``None`` in the mask (image) lists; the means run over the frames that have the score and
    are ``None`` when no frame has it.  Returns ``{"IOU", "ACC", "PSNR_frames", "SSIM_frames": per-frame lists; "mIOU",
    "mACC", "PSNR", "SSIM": means}``; with ``lpips`` also ``"LPIPS_frames"`` and ``"LPIPS"``, the float64 stored in word 6."""
    rec = np.ascontiguousarray(np.asarray(records, dtype=np.int64).reshape(-1, RECORD_WORDS))
    ssim_f64 = rec.view(np.float64)[:, SSIM]
    iou, acc, psnr, ssims = [], [], [], []
    for i, r in enumerate(rec):
        has_mask, has_image = r[PIXELS] > 0, r[VALUES] > 0
        iou.append(None if not has_mask else float(r[INTER]) / float(r[UNION]) if r[UNION] != 0 else 0.0)
        acc.append(None if not has_mask else float(r[EQUAL]) / float(r[PIXELS]))
        if has_image:
            mse = float(r[SSE]) / 65025.0 / float(r[VALUES]) if quantize else float(sse_float[i]) / float(r[VALUES])
            psnr.append(20.0 * math.log10(1.0 / math.sqrt(mse)) if mse > 0.0 else (math.inf if mse == 0.0 else math.nan))
        else:
            psnr.append(None)
        ssims.append(float(ssim_f64[i]) if (has_image and ssim) else None)

    def mean(xs):
        xs = [x for x in xs if x is not None]
        return float(np.mean(np.asarray(xs, dtype=np.float64))) if xs else None

    out = {"IOU": iou, "ACC": acc, "PSNR_frames": psnr, "SSIM_frames": ssims,
           "mIOU": mean(iou), "mACC": mean(acc), "PSNR": mean(psnr), "SSIM": mean(ssims)}
    if lpips:
        lpips_f64 = rec.view(np.float64)[:, LPIPS]
        frames = [float(lpips_f64[i]) if r[VALUES] > 0 else None for i, r in enumerate(rec)]
        out["LPIPS_frames"], out["LPIPS"] = frames, mean(frames)
    return out


class FrameScores:
    """``capacity`` score records on ``device``, zeroed once; ``render_segment`` / ``segment_scores`` / ``image_scores`` add
    a frame's counts to row ``frame``.  A row takes one mask pair and one image pair: the counts ADD, so write a slot once
    (``reset()`` zeroes everything).  ``quantize`` (default): the image pair is compared as the 8-bit files the reference
    reads back, ``floor(255 x + 0.5)`` clamped to 0..255, and the squared error is an exact integer; ``quantize=False``
    compares the fp32 values, summed in float64 per workgroup and combined in workgroup order.  ``ssim=False`` skips the SSIM
    launch.  ``lpips`` (an ``LPIPSVGG``): the frame's LPIPS of the pair SSIM sees (quantised unless ``quantize=False``) goes
    into word 6 of the record as a device float64, without a synchronisation; ``result()`` then also returns
    ``"LPIPS_frames"`` and ``"LPIPS"``.  With ``lpips=None`` records, keys and launches are what they are without it.
    Everything recorded is bitwise reproducible.

    ``result()`` makes ONE device-to-host copy and returns ``{"IOU", "ACC", "PSNR_frames", "SSIM_frames": per-frame
    lists; "mIOU", "mACC", "PSNR", "SSIM": means in float64}`` (``scores_from_records``)."""

    def __init__(self, capacity: int, *, device, quantize: bool = True, ssim: bool = True, lpips=None):
        if int(capacity) < 1:
            raise ValueError("FrameScores: capacity must be at least 1")
        self.capacity, self.quantize, self.ssim = int(capacity), bool(quantize), bool(ssim)
        self.device = torch.device(device)
        # one allocation, one read-back: a row = the record, then (unquantised only) the per-workgroup float64 sums
        words = RECORD_WORDS + (0 if self.quantize else PARTIAL_SLOTS)
        self.buffer = torch.zeros(self.capacity, words, dtype=torch.int64, device=self.device)
        self._ssim = self.buffer.view(torch.float64)[:, SSIM]
        self.lpips = lpips
        self._lpips = self.buffer.view(torch.float64)[:, LPIPS]

    @property
    def records(self) -> torch.Tensor:
        """The (capacity, 8) int64 records (a view of the buffer)."""
        return self.buffer[:, :RECORD_WORDS]

    def reset(self) -> None:
        self.buffer.zero_()

    def _row(self, frame):
        frame = 0 if frame is None else int(frame)
        if not 0 <= frame < self.capacity:
            raise IndexError(f"FrameScores: frame {frame} outside 0..{self.capacity - 1}")
        base = self.buffer.data_ptr() + frame * self.buffer.shape[1] * 8
        return frame, base, (None if self.quantize else base + RECORD_WORDS * 8)

    def result(self) -> dict:
        host = self.buffer.cpu().numpy()                 # the one read-back
        sse_float = None
        if not self.quantize:
            parts = host[:, RECORD_WORDS:].view(np.float64)
            sse_float = np.zeros(self.capacity, dtype=np.float64)
            for b in range(PARTIAL_SLOTS):               # workgroup order
                sse_float += parts[:, b]
        return scores_from_records(host[:, :RECORD_WORDS], sse_float, quantize=self.quantize, ssim=self.ssim,
                                   lpips=self.lpips is not None)


def _cuda(t, what, dev=None):
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise RuntimeError(f"trase_amd.evaluate runs on the GPU only (there is no CPU path): {what}")
    if dev is not None and t.device != dev:
        raise ValueError(f"{what} is on {t.device}, expected {dev}")
    return t


def _mask_bytes(t, what, H, W, dev):
    _cuda(t, what, dev)
    if t.dtype not in (torch.bool, torch.uint8) or tuple(t.shape) != (H, W):
        raise ValueError(f"{what} must be a bool or uint8 tensor of shape ({H}, {W}), got {t.dtype} {tuple(t.shape)}")
    return t.contiguous().view(torch.uint8)


def _gt_object(t, H, W, dev):
    _cuda(t, "gt_object", dev)
    if t.dtype == torch.float32 and tuple(t.shape) == (3, H, W):
        return t.contiguous(), GT_F32_CHW
    if t.dtype == torch.uint8 and tuple(t.shape) == (3, H, W):
        return t.contiguous(), GT_U8_CHW
    if t.dtype == torch.uint8 and tuple(t.shape) == (H, W, 3):
        return t.contiguous(), GT_U8_HWC
    raise ValueError(f"gt_object must be (3, {H}, {W}) fp32 or uint8, or ({H}, {W}, 3) uint8, got {t.dtype} {tuple(t.shape)}")


def _evaluate(dev, H, W, *, image=None, img_ws=None, final_T=None, pred_in=None, outputs=False, frames_u8=False,
              white_background=False, threshold=0.5, scores=None, frame=None, gt_mask=None, gt_object=None) -> dict:
    """One ``trase_evaluate_frame`` launch (and the SSIM launches when an image pair is scored); no synchronisation."""
    lib = _lib.load()
    if (gt_mask is not None or gt_object is not None) and scores is None:
        raise ValueError("a ground truth needs a FrameScores to record into (scores=)")
    if scores is not None and scores.device != dev:
        raise ValueError(f"the FrameScores lives on {scores.device}, the frame on {dev}")
    f = _lib.EvalFrame()
    f.W, f.H, f.threshold, f.outside = W, H, float(threshold), 1.0 if white_background else 0.0
    keep = [image, img_ws, final_T, pred_in]
    f.image, f.final_T, f.pred_in = _lib.ptr(image), _lib.ptr(final_T), _lib.ptr(pred_in)
    out = {}
    has_T = img_ws is not None or final_T is not None
    if outputs:
        if image is not None:
            out["object"] = torch.empty(3, H, W, device=dev)
            f.object = _lib.ptr(out["object"])
        out["pred_mask"] = torch.empty(H, W, dtype=torch.bool, device=dev)
        f.pred_mask = _lib.ptr(out["pred_mask"])
        if has_T:
            out["alpha"] = torch.empty(H, W, device=dev)
            f.alpha = _lib.ptr(out["alpha"])
        if frames_u8:
            out["pred_mask_u8"] = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
            f.pred_mask_u8 = _lib.ptr(out["pred_mask_u8"])
            if image is not None:
                out["object_u8"] = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
                f.object_u8 = _lib.ptr(out["object_u8"])
    pair = None
    if scores is not None and (gt_mask is not None or gt_object is not None):
        frame, rec, parts = scores._row(frame)
        f.record, f.partials, f.quantize = rec, parts, int(scores.quantize)
        if gt_mask is not None:
            gt_mask = _mask_bytes(gt_mask, "gt_mask", H, W, dev)
            f.gt_mask = _lib.ptr(gt_mask)
        if gt_object is not None:
            if image is None:
                raise ValueError("gt_object needs an image to compare with")
            gt_object, f.gt_object_kind = _gt_object(gt_object, H, W, dev)
            f.gt_object = _lib.ptr(gt_object)
            if scores.ssim or scores.lpips is not None:
                pair = torch.empty(2, 3, H, W, device=dev)
                f.pair_object, f.pair_gt = _lib.ptr(pair[0]), _lib.ptr(pair[1])
        keep += [gt_mask, gt_object]
    ws = None
    if img_ws is not None:
        ws = _lib.RastWorkspace()
        ws.img, ws.img_bytes = _lib.ptr(img_ws), img_ws.numel()
    _lib.check(lib.trase_evaluate_frame(C.byref(f), C.byref(ws) if ws is not None else None, _device_index(dev), _stream(dev)),
               "trase_evaluate_frame")
    if pair is not None and scores.ssim:
        from .losses import ssim as _ssim
        with torch.no_grad():
            scores._ssim[frame].copy_(_ssim(pair[0], pair[1]))      # a device scalar into the record: nothing synchronises
    if pair is not None and scores.lpips is not None:
        from .lpips import total_of
        with torch.no_grad():
            scores._lpips[frame].copy_(total_of(scores.lpips.to(dev).layers_device(pair[0], pair[1])))
    return out


def render_segment(viewpoint_camera, pc, pipe, bg_color, d_xyz, d_rotation, d_scaling, is_6dof=False, *, mask,
                   white_background=False, threshold=0.5, frames_u8=False, scores=None, frame=None, gt_mask=None,
                   gt_object=None) -> dict:
    """The reference's output for a selection (render.py:344-366) from one rasterizer pass.

    ``mask`` (N,) bool selects the Gaussians, as in ``render(mask=)``.  Returns
      ``object``     (3,H,W) fp32: the ``render(mask=)`` image inside the predicted mask, exactly 0.0 -- 1.0 with
                     ``white_background`` -- outside it;
      ``pred_mask``  (H,W) bool: ``alpha >= threshold``;
      ``alpha``      (H,W) fp32: ``1 - T_final``, what an all-ones render on black composites;
      with ``frames_u8`` also ``object_u8`` and ``pred_mask_u8``, (H,W,3) uint8: ``to8b(x).transpose(1,2,0)``.
    With ``gt_mask`` ((H,W) bool or uint8, non-zero = object) and / or ``gt_object`` ((3,H,W) fp32 in [0,1], or uint8 as
    (3,H,W) or (H,W,3)) the same pass adds the frame's record to row ``frame`` of ``scores`` (a ``FrameScores``).

    One fused forward plus one launch (plus the SSIM launches when an image pair is scored).  Nothing here synchronises;
    the forward itself reads the pair count back unless the sync-free capacity policy is on (``rasterizer.set_sync``).
    Arguments the fused forward does not take (``renderer._fusable``) are refused."""
    from .renderer import render
    if mask is None:
        raise ValueError("render_segment needs the selection (mask=)")
    H, W = int(viewpoint_camera.image_height), int(viewpoint_camera.image_width)
    hold: dict = {}
    with torch.no_grad():
        image = render(viewpoint_camera, pc, pipe, bg_color, d_xyz, d_rotation, d_scaling, is_6dof, mask=mask,
                       _keep_img=hold)["render"]
    return _evaluate(image.device, H, W, image=image, img_ws=hold["img"], outputs=True, frames_u8=frames_u8,
                     white_background=white_background, threshold=threshold, scores=scores, frame=frame, gt_mask=gt_mask,
                     gt_object=gt_object)


def segment_frame(image, final_T, *, white_background=False, threshold=0.5, frames_u8=False, scores=None, frame=None,
                  gt_mask=None, gt_object=None) -> dict:
    """``render_segment``'s launch on a caller's own ``image`` (3,H,W) fp32 and per-pixel transmittance ``final_T`` (H,W)
    fp32: the same dict, the same scoring, no rasterizer."""
    _cuda(image, "image")
    _cuda(final_T, "final_T", image.device)
    if image.dtype != torch.float32 or image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"image must be (3, H, W) fp32, got {image.dtype} {tuple(image.shape)}")
    H, W = int(image.shape[1]), int(image.shape[2])
    if final_T.dtype != torch.float32 or tuple(final_T.shape) != (H, W):
        raise ValueError(f"final_T must be ({H}, {W}) fp32, got {final_T.dtype} {tuple(final_T.shape)}")
    return _evaluate(image.device, H, W, image=image.detach().contiguous(), final_T=final_T.detach().contiguous(), outputs=True,
                     frames_u8=frames_u8, white_background=white_background, threshold=threshold, scores=scores, frame=frame,
                     gt_mask=gt_mask, gt_object=gt_object)


def segment_scores(pred_mask, gt_mask, scores: FrameScores, frame=None) -> None:
    """Adds intersection, union, equal pixels and pixel count of two (H,W) masks (bool or uint8, non-zero = object) to row
    ``frame`` of ``scores`` -- the kernel of ``render_segment`` with the render inputs absent."""
    _cuda(pred_mask, "pred_mask")
    H, W = (int(v) for v in pred_mask.shape[-2:])
    pred = _mask_bytes(pred_mask, "pred_mask", H, W, pred_mask.device)
    _evaluate(pred.device, H, W, pred_in=pred, scores=scores, frame=frame, gt_mask=gt_mask)


def image_scores(image, gt, scores: FrameScores, frame=None) -> None:
    """Adds the squared error (and SSIM) of ``image`` ((3,H,W) fp32) against ``gt`` ((3,H,W) fp32 in [0,1], or uint8 as
    (3,H,W) or (H,W,3)) to row ``frame`` of ``scores`` -- the kernel of ``render_segment`` with the render inputs absent."""
    _cuda(image, "image")
    if image.dtype != torch.float32 or image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"image must be (3, H, W) fp32, got {image.dtype} {tuple(image.shape)}")
    H, W = int(image.shape[1]), int(image.shape[2])
    _evaluate(image.device, H, W, image=image.detach().contiguous(), scores=scores, frame=frame, gt_object=gt)
