"""A view's ground truth as bytes on the device.

Every ground-truth frame of the reference is the image of a byte array: ``PILtoTorch`` (utils/general_utils.py:22-28) is
``torch.from_numpy(np.array(pil_image)) / 255.0``, so each pixel is exactly ``float32(b) / float32(255)``.  The reference keeps
that as fp32 on the device (scene/cameras.py:60, 24.9 MB per 1080p frame) or, with ``load_image_on_the_fly``, rebuilds it on
the host in every iteration (train.py:220-230).  ``ByteFrame`` keeps the bytes (6.2 MB), planar so that the loss kernels read
one plane per channel; ``trase_amd.losses`` accepts it wherever it accepts the fp32 tensor and returns bitwise the same
results, and ``black_mask`` gives ``--mask_black_bg`` its mask (train.py:231-234, :253-269) without the fp32 frame.  With
``resolution=(W, H)`` the frame is ``pil_image.resize(resolution)`` of the bytes -- Pillow's default bicubic filter, bit for bit,
in the launch that writes the planes -- which is what ``PILtoTorch`` does before it takes them."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .rasterizer import _stream


MAX_SHRINK = 16          # trase_frame_resize: each axis shrinks by at most this (in <= 16 * out)


def _dev_index(dev) -> int:
    return dev.index if dev.index is not None else torch.cuda.current_device()


def camera_resolution(orig_w, orig_h, resolution=-1, resolution_scale=1.0):
    """The ``(W, H)`` that ``loadCam`` (utils/camera_utils.py:30-48) hands to ``PILtoTorch``: ``round`` of the quotient for
    ``--resolution`` 1 / 2 / 4 / 8; for -1 the source's own size, or 1600 pixels wide for a wider source; otherwise
    ``resolution`` pixels wide; both of the latter through ``int()``."""
    if resolution in [1, 2, 4, 8]:
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


@torch.no_grad()
def resize_tables(in_size, out_size, device):
    """The coefficient rows the resize kernel computes for one axis, by its own device function: ``(coeffs, bounds)``, int32
    tensors of (out, ksize) -- zero beyond n -- and (out, 2) = (xmin, n)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resize_tables: sizes must be at least 1 (got {in_size} -> {out_size})")
    if in_size > MAX_SHRINK * out_size:
        raise ValueError(f"resize_tables: an axis may shrink by at most {MAX_SHRINK} (got {in_size} -> {out_size})")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("trase_amd.frames runs on the GPU only (there is no CPU path)")
    ksize = int(math.ceil(2.0 * max(in_size / out_size, 1.0))) * 2 + 1
    coeffs = torch.empty((out_size, ksize), dtype=torch.int32, device=dev)
    bounds = torch.empty((out_size, 2), dtype=torch.int32, device=dev)
    dev = coeffs.device
    lib = _lib.load()
    _lib.check(lib.trase_selftest_resize_tables(in_size, out_size, _lib.ptr(coeffs), _lib.ptr(bounds), _dev_index(dev), _stream(dev)),
               "trase_selftest_resize_tables")
    return coeffs, bounds


class ByteFrame:
    """``data``: a contiguous 1-d uint8 tensor of ``3 * H * pitch`` bytes whose storage starts on a 16-byte boundary -- the
    planes r, g, b, each of H rows ``pitch`` bytes apart, ``pitch`` the smallest multiple of 16 that is at least W.  What the row
    padding holds is ignored by every consumer."""

    def __init__(self, data: torch.Tensor, H: int, W: int):
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f"ByteFrame: H, W must be >= 1 (got {H}, {W})")
        if not torch.is_tensor(data) or data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
            raise ValueError("ByteFrame: data must be a contiguous 1-d uint8 tensor")
        pitch = ByteFrame.pitch_for(W)
        if data.numel() != 3 * H * pitch:
            raise ValueError(f"ByteFrame: data holds {data.numel()} bytes; a {H} x {W} frame is 3 * {H} * {pitch} = {3 * H * pitch}")
        if data.data_ptr() % 16:
            raise ValueError("ByteFrame: data must start on a 16-byte boundary")
        self.data, self.H, self.W, self.pitch = data, H, W, pitch

    @staticmethod
    def pitch_for(W: int) -> int:
        """Bytes from row to row: the smallest multiple of 16 that is at least W."""
        return (int(W) + 15) // 16 * 16

    @property
    def shape(self):
        return (3, self.H, self.W)

    @property
    def device(self):
        return self.data.device

    @property
    def nbytes(self) -> int:
        return self.data.numel()

    @property
    def _version(self):          # what the l1_loss / ssim pair cache of trase_amd.losses compares
        return self.data._version

    def dim(self) -> int:
        return 3

    def _gpu(self):
        if self.data.device.type != "cuda":
            raise RuntimeError("trase_amd.frames runs on the GPU only (there is no CPU path)")
        return self

    # ---- construction ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def host_array(hwc):
        """(source, H, W, channels) of an (H, W, 3 | 4) uint8 numpy array or tensor -- ``np.array(pil_image)`` -- as the one
        contiguous uint8 tensor that is uploaded as it is (never permuted on the host); a device tensor stays where it is."""
        if isinstance(hwc, np.ndarray):
            if hwc.dtype != np.uint8:
                raise ValueError(f"ByteFrame: the image must be uint8 (got {hwc.dtype})")
            src = torch.from_numpy(np.ascontiguousarray(hwc))
        elif torch.is_tensor(hwc):
            if hwc.dtype != torch.uint8:
                raise ValueError(f"ByteFrame: the image must be uint8 (got {hwc.dtype})")
            src = hwc.detach().contiguous()
        else:
            raise ValueError(f"ByteFrame: cannot read an image from {type(hwc).__name__}")
        if src.dim() != 3 or src.shape[2] not in (3, 4) or src.shape[0] < 1 or src.shape[1] < 1:
            raise ValueError(f"ByteFrame: the image must be (H, W, 3) or (H, W, 4) (got {tuple(src.shape)})")
        return src, int(src.shape[0]), int(src.shape[1]), int(src.shape[2])

    @staticmethod
    def _resolution(resolution, who):
        """``(W, H)`` as two ints at least 1, or None"""
        if resolution is None:
            return None
        try:
            W, H = resolution
            W, H = int(W), int(H)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: resolution must be (W, H) (got {resolution!r})") from None
        if W < 1 or H < 1:
            raise ValueError(f"{who}: resolution must be at least 1 x 1 (got {W} x {H})")
        return W, H

    @staticmethod
    def _check_shrink(who, sH, sW, H, W):
        if sH > MAX_SHRINK * H or sW > MAX_SHRINK * W:
            raise ValueError(f"{who}: an axis may shrink by at most {MAX_SHRINK} (got {sW} x {sH} -> {W} x {H})")

    @staticmethod
    @torch.no_grad()
    def _pack(hwc, background, device, resolution=None) -> "ByteFrame":
        who = "ByteFrame.from_array" if background is None else "ByteFrame.from_rgba"
        src, sH, sW, ch = ByteFrame.host_array(hwc)
        bg = None
        if background is not None:
            if ch != 4:
                raise ValueError("ByteFrame.from_rgba: the composite needs an (H, W, 4) image")
            b = background.detach().cpu() if torch.is_tensor(background) else torch.as_tensor(np.asarray(background))
            b = b.to(torch.float32).reshape(-1)
            if b.numel() != 3:
                raise ValueError(f"ByteFrame.from_rgba: the background must hold three values (got {b.numel()})")
            bg = (C.c_float * 3)(*b.tolist())
        W, H = ByteFrame._resolution(resolution, who) or (sW, sH)
        ByteFrame._check_shrink(who, sH, sW, H, W)
        dev = torch.device(device) if device is not None else src.device
        if dev.type != "cuda":
            raise RuntimeError("trase_amd.frames runs on the GPU only (there is no CPU path)")
        src = src.to(dev)                                             # the one upload (nothing for a device source)
        dev = src.device
        pitch = ByteFrame.pitch_for(W)
        data = torch.empty(3 * H * pitch, dtype=torch.uint8, device=dev)
        lib = _lib.load()
        if (H, W) == (sH, sW):
            _lib.check(lib.trase_frame_pack(_lib.ptr(src), H, W, ch, bg, _lib.ptr(data), pitch, _dev_index(dev), _stream(dev)),
                       "trase_frame_pack")
        else:
            _lib.check(lib.trase_frame_resize(_lib.ptr(src), sH, sW, ch, 0, bg, _lib.ptr(data), H, W, pitch, _dev_index(dev),
                                              _stream(dev)), "trase_frame_resize")
        return ByteFrame(data, H, W)

    @staticmethod
    def from_array(hwc, device=None, *, resolution=None) -> "ByteFrame":
        """``np.array(pil_image)``, (H, W, 3) or (H, W, 4) uint8 on the host or the device: one upload of the bytes as they are
        and one launch that writes the planes.  A fourth channel is dropped (utils/camera_utils.py:51).  ``device``: where the
        frame lives (default: the source's device).  ``resolution``: ``(W, H)``, the argument of ``PILtoTorch`` -- the frame is
        ``pil_image.resize(resolution)`` of the RGB bytes (Pillow's default bicubic filter, bit for bit), formed by that one
        launch; ``None`` or the source's own size packs the bytes as they are."""
        return ByteFrame._pack(hwc, None, device, resolution)

    @staticmethod
    def from_rgba(rgba, background, device=None, *, resolution=None) -> "ByteFrame":
        """The on-the-fly frame of train.py:221-228 from ``np.array(image.convert("RGBA"))``: per channel the byte
        ``trunc(((v / 255.0) * (a / 255.0) + bg * (1 - a / 255.0)) * 255.0)``, evaluated on the device in float64 exactly as numpy
        evaluates it (``background``: three values, taken as float32 like the reference's tensor).  ``resolution``: ``(W, H)`` of
        train.py:229 -- the composite is resized as an RGB image (what the reference does where every alpha is 255)."""
        if background is None:
            raise ValueError("ByteFrame.from_rgba: a background is required (use from_array to drop the alpha)")
        return ByteFrame._pack(rgba, background, device, resolution)

    @torch.no_grad()
    def resized(self, resolution) -> "ByteFrame":
        """A new frame at ``resolution = (W, H)`` from this resident one (the coarser levels of ``resolution_scales``): Pillow's
        bicubic resize of its bytes, one launch."""
        dev = self._gpu().data.device
        W, H = ByteFrame._resolution(resolution, "ByteFrame.resized") or (self.W, self.H)
        ByteFrame._check_shrink("ByteFrame.resized", self.H, self.W, H, W)
        pitch = ByteFrame.pitch_for(W)
        data = torch.empty(3 * H * pitch, dtype=torch.uint8, device=dev)
        lib = _lib.load()
        _lib.check(lib.trase_frame_resize(_lib.ptr(self.data), self.H, self.W, _lib.FRAME_PLANAR, self.pitch, None, _lib.ptr(data), H, W,
                                          pitch, _dev_index(dev), _stream(dev)), "trase_frame_resize")
        return ByteFrame(data, H, W)

    @staticmethod
    @torch.no_grad()
    def from_float(chw: torch.Tensor, check: bool = True) -> "ByteFrame":
        """From a (3, H, W) ``original_image``: the bytes ``rint(v * 255)``.  ``check``: one comparison of the frame those bytes
        give against the input; ``ValueError`` if any pixel is not exactly a ``k / 255`` (the frame would not be the input)."""
        if not torch.is_tensor(chw) or chw.dim() != 3 or chw.shape[0] != 3 or chw.shape[1] < 1 or chw.shape[2] < 1:
            raise ValueError("ByteFrame.from_float: expected a (3, H, W) tensor")
        v = chw.detach().to(torch.float32)
        q = torch.clamp(torch.round(v * 255.0), 0.0, 255.0)           # torch.round is rint: half to even
        _, H, W = v.shape
        pitch = ByteFrame.pitch_for(W)
        if v.device.type == "cuda":
            data = torch.zeros(3 * H * pitch, dtype=torch.uint8, device=v.device)
            data.view(3, H, pitch)[:, :, :W] = q.to(torch.uint8)
            frame = ByteFrame(data, H, W)
            back = frame.to_float() if check else None
        else:
            # (on the host torch's division is the IEEE quotient; on the device it multiplies by the reciprocal, so the
            # comparison there goes through to_float's kernel)
            frame, back = None, (q / 255.0 if check else None)
        if check and not torch.equal(back, v):
            raise ValueError(f"ByteFrame.from_float: {int((back != v).sum())} values are not exactly k / 255 for a byte k; the bytes "
                             "would not reproduce this image (check=False rounds them)")
        if frame is None:
            raise RuntimeError("trase_amd.frames runs on the GPU only (there is no CPU path)")
        return frame

    # ---- consumers ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def to_float(self) -> torch.Tensor:
        """The (3, H, W) fp32 frame, bit for bit the reference's ``original_image``: every value the fp32 quotient ``b / 255``."""
        dev = self._gpu().data.device
        out = torch.empty(self.shape, dtype=torch.float32, device=dev)
        lib = _lib.load()
        _lib.check(lib.trase_frame_unpack(_lib.ptr(self.data), self.H, self.W, self.pitch, _lib.ptr(out), _dev_index(dev), _stream(dev)),
                   "trase_frame_unpack")
        return out

    @torch.no_grad()
    def black_mask(self, size=None) -> torch.Tensor:
        """(H, W) bool, ``torch.sum(gt_image, dim=0) == 0`` (train.py:232): the pixels that are 0 in all three planes.  With
        ``size=(h, w)``: the mask at SAM-mask resolution as train.py:267-268 forms it (bilinear resize, then the same test): a
        pixel is black exactly when every tap of non-zero weight is.  One launch; the result is what
        ``get_sample_pixel_and_mask(..., exclude=)`` takes."""
        dev = self._gpu().data.device
        h, w = (self.H, self.W) if size is None else (int(size[0]), int(size[1]))
        if h < 1 or w < 1:
            raise ValueError(f"ByteFrame.black_mask: size must be at least 1 x 1 (got {h} x {w})")
        out = torch.empty((h, w), dtype=torch.uint8, device=dev)
        lib = _lib.load()
        _lib.check(lib.trase_frame_black_mask(_lib.ptr(self.data), self.H, self.W, self.pitch, h, w, _lib.ptr(out), _dev_index(dev),
                                              _stream(dev)), "trase_frame_black_mask")
        return out.view(torch.bool)
