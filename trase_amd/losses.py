"""Photometric loss heads of the training loop on the GPU as two HIP kernels:
``l1_loss`` (utils/loss_utils.py:30-31) and ``ssim`` (utils/loss_utils.py:56-86), combined at train.py:235-238 as
``(1 - lambda) * Ll1 + lambda * (1 - ssim(image, gt))``.

``l1_ssim(img, gt)`` returns both scalars from ONE forward kernel (separable 11-tap window from LDS tiles instead
of the reference's five depthwise 11x11 convolutions) and back-propagates both with ONE backward kernel.
``ssim(img1, img2)`` and ``l1_loss(x, gt)`` keep the reference signatures; when they are called on the same pair of
tensors (as train.py does) the second call reuses the first call's fused result.

The ground truth may also be a ``trase_amd.frames.ByteFrame`` (the frame as bytes): the same kernel bodies read the planes and
convert with the exact division, so every result is bitwise that of the fp32 tensor ``frame.to_float()``."""
from __future__ import annotations

import ctypes as C
import weakref

import torch

from . import _lib
from .frames import ByteFrame
from .rasterizer import _bytes, _stream

MASK_BLACK = 1          # include/trase_rast.h TRASE_FRAME_MASK_BLACK


def _gt_operand(gt, mask_black=False):
    """(the tensor the kernels read, None | (pitch, flags)) of a ground truth given as a tensor or as a ByteFrame"""
    if isinstance(gt, ByteFrame):
        return gt.data, (gt.pitch, MASK_BLACK if mask_black else 0)
    return gt, None


class _L1SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, gt, u8=None):
        # u8: None = gt is the (C,H,W) tensor; (pitch, flags) = gt is a ByteFrame's planes
        lib = _lib.load()
        dev = img.device
        x = img.detach().float().contiguous()
        y = gt.detach().float().contiguous() if u8 is None else gt
        c, h, w = x.shape
        nbytes = C.c_size_t()
        _lib.check(lib.trase_loss_sizes(c, h, w, C.byref(nbytes)), "trase_loss_sizes")
        ws = _bytes(nbytes.value, dev)
        out2 = torch.empty(2, device=dev)
        d = dev.index if dev.index is not None else torch.cuda.current_device()
        if u8 is None:
            _lib.check(lib.trase_loss_l1_ssim_forward(_lib.ptr(x), _lib.ptr(y), c, h, w, _lib.ptr(out2), _lib.ptr(ws), ws.numel(),
                                                      d, _stream(dev)), "trase_loss_l1_ssim_forward")
        else:
            _lib.check(lib.trase_loss_l1_ssim_forward_u8(_lib.ptr(x), _lib.ptr(y), h, w, u8[0], u8[1], _lib.ptr(out2), _lib.ptr(ws),
                                                         ws.numel(), d, _stream(dev)), "trase_loss_l1_ssim_forward_u8")
        ctx.save_for_backward(x, y, ws)
        ctx.u8 = u8
        return out2[0], out2[1]

    @staticmethod
    def backward(ctx, g_l1, g_ssim):
        lib = _lib.load()
        x, y, ws = ctx.saved_tensors
        # the shared evaluation cached by _fused() has served its iteration: drop it, so that it neither keeps the saved
        # images / derivative maps alive until the next call nor hands out outputs whose graph has been freed
        _last["img"] = _last["gt"] = _last["val"] = None
        dev = x.device
        c, h, w = x.shape
        z = torch.zeros((), device=dev)
        g2 = torch.stack([g_l1 if g_l1 is not None else z, g_ssim if g_ssim is not None else z]).float().contiguous()
        d_img = torch.empty_like(x)
        d = dev.index if dev.index is not None else torch.cuda.current_device()
        if ctx.u8 is None:
            _lib.check(lib.trase_loss_l1_ssim_backward(_lib.ptr(x), _lib.ptr(y), c, h, w, _lib.ptr(g2), _lib.ptr(ws), ws.numel(),
                                                       _lib.ptr(d_img), d, _stream(dev)), "trase_loss_l1_ssim_backward")
        else:
            _lib.check(lib.trase_loss_l1_ssim_backward_u8(_lib.ptr(x), _lib.ptr(y), h, w, ctx.u8[0], ctx.u8[1], _lib.ptr(g2), _lib.ptr(ws),
                                                          ws.numel(), _lib.ptr(d_img), d, _stream(dev)), "trase_loss_l1_ssim_backward_u8")
        return d_img, None, None


class _Photometric(torch.autograd.Function):
    """One scalar out, one cotangent in: the combination of train.py:235-238 inside the two loss launches."""

    @staticmethod
    def forward(ctx, img, gt, lambda_dssim, u8=None):
        lib = _lib.load()
        dev = img.device
        x = img.detach().float().contiguous()
        y = gt.detach().float().contiguous() if u8 is None else gt          # u8: see _L1SSIM.forward
        c, h, w = x.shape
        nbytes = C.c_size_t()
        _lib.check(lib.trase_loss_sizes(c, h, w, C.byref(nbytes)), "trase_loss_sizes")
        ws = _bytes(nbytes.value, dev)
        out3 = torch.empty(3, device=dev)
        d = dev.index if dev.index is not None else torch.cuda.current_device()
        if u8 is None:
            _lib.check(lib.trase_loss_photometric_forward(_lib.ptr(x), _lib.ptr(y), c, h, w, float(lambda_dssim), _lib.ptr(out3),
                                                          _lib.ptr(ws), ws.numel(), d, _stream(dev)), "trase_loss_photometric_forward")
        else:
            _lib.check(lib.trase_loss_photometric_forward_u8(_lib.ptr(x), _lib.ptr(y), h, w, u8[0], u8[1], float(lambda_dssim),
                                                             _lib.ptr(out3), _lib.ptr(ws), ws.numel(), d, _stream(dev)),
                       "trase_loss_photometric_forward_u8")
        ctx.save_for_backward(x, y, ws)
        ctx.u8 = u8
        ctx.lam = float(lambda_dssim)
        ctx.mark_non_differentiable(out3)
        return out3[2], out3

    @staticmethod
    def backward(ctx, g, _g_parts):
        lib = _lib.load()
        x, y, ws = ctx.saved_tensors
        dev = x.device
        c, h, w = x.shape
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.float().contiguous()
        d_img = torch.empty_like(x)
        d = dev.index if dev.index is not None else torch.cuda.current_device()
        if ctx.u8 is None:
            _lib.check(lib.trase_loss_photometric_backward(_lib.ptr(x), _lib.ptr(y), c, h, w, ctx.lam, _lib.ptr(g), _lib.ptr(ws), ws.numel(),
                                                           _lib.ptr(d_img), d, _stream(dev)), "trase_loss_photometric_backward")
        else:
            _lib.check(lib.trase_loss_photometric_backward_u8(_lib.ptr(x), _lib.ptr(y), h, w, ctx.u8[0], ctx.u8[1], ctx.lam, _lib.ptr(g),
                                                              _lib.ptr(ws), ws.numel(), _lib.ptr(d_img), d, _stream(dev)),
                       "trase_loss_photometric_backward_u8")
        return d_img, None, None, None


def photometric_loss(img: torch.Tensor, gt, lambda_dssim: float = 0.2, with_parts: bool = False, *, mask_black: bool = False):
    """``(1 - lambda_dssim) * l1_loss(img, gt) + lambda_dssim * (1 - ssim(img, gt))`` (train.py:235-238) as ONE autograd node: the
    scalar composition happens inside the loss kernels (forward: in the reduction kernel; backward: the cotangent is scaled
    in the SSIM backward kernel), so the ~10 one-element kernels PyTorch launches for the reference's two lines are gone.
    with_parts: also return the detached (l1, ssim) scalars (train.py logs Ll1, :303).
    gt: the (3,H,W) tensor or a ByteFrame.  mask_black (ByteFrame only): train.py:231-234 fused -- where the frame's pixel is black
    the rendered value counts as 0, in the window too, and receives no gradient (a non-finite rendered value there is ignored,
    where the reference's ``image * 0`` gives NaN)."""
    _check(img, gt, mask_black)
    y, u8 = _gt_operand(gt, mask_black)
    loss, parts = _Photometric.apply(img, y, lambda_dssim, u8)
    return (loss, parts[0], parts[1]) if with_parts else loss


def _check(img, gt, mask_black=False):
    if mask_black and not isinstance(gt, ByteFrame):
        raise TypeError("mask_black=True needs the ground truth as a trase_amd.frames.ByteFrame (ByteFrame.from_float(gt) makes one)")
    if img.device.type != "cuda":
        raise RuntimeError("trase_amd.losses runs on the GPU only (there is no CPU path)")
    if img.dim() != 3 or tuple(img.shape) != tuple(gt.shape):
        raise ValueError(f"expected two (C,H,W) images of equal shape, got {tuple(img.shape)} and {tuple(gt.shape)}")
    if isinstance(gt, ByteFrame) and gt.device != img.device:
        raise ValueError(f"the ByteFrame is on {gt.device}, the image on {img.device}")


def l1_ssim(img: torch.Tensor, gt, *, mask_black: bool = False):
    """(mean |img - gt|, mean SSIM(img, gt)) -- one fused forward, one fused backward (gradient w.r.t. img only,
    the reference's gt is a constant).  gt: the tensor or a ByteFrame; mask_black as in photometric_loss."""
    _check(img, gt, mask_black)
    return _L1SSIM.apply(img, *_gt_operand(gt, mask_black))


_last = {"img": None, "gt": None, "ver": None, "val": None}


def _fused(img, gt):
    """One fused evaluation shared by l1_loss(x, gt) and ssim(x, gt) when train.py calls them back to back on the same
    tensors.  The cache holds WEAK references to the inputs and compares object identity + version counters: a new tensor
    that happens to reuse a freed tensor's id() can never hit it.  The cached outputs are released by the backward (a
    logging call after loss.backward() re-evaluates instead of returning outputs of a freed graph)."""
    ri, rg = _last["img"], _last["gt"]
    ver = (img._version, gt._version, torch.is_grad_enabled(), img.requires_grad)
    if ri is None or ri() is not img or rg() is not gt or _last["ver"] != ver:
        _last["val"] = l1_ssim(img, gt)
        _last["img"], _last["gt"], _last["ver"] = weakref.ref(img), weakref.ref(gt), ver
    return _last["val"]


def l1_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """utils/loss_utils.py:30-31."""
    return _fused(network_output, gt)[0]


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """utils/loss_utils.py:56-86 for the configuration the training scripts use (window 11, size_average)."""
    if window_size != 11 or not size_average:
        raise NotImplementedError("trase_amd.losses.ssim: only window_size=11, size_average=True is compiled in")
    return _fused(img1, img2)[1]


# ---- contrastive pixel-pair losses (utils/loss_utils.py:275-406) --------------------------------------------------------
PAIR_POSITIVE, PAIR_NEGATIVE, PAIR_SOFT, PAIR_ALL, PAIR_HARD = 0, 1, 0, 2, 4      # include/trase_rast.h TRASE_PAIR_*


class _PixelPair(torch.autograd.Function):
    @staticmethod
    def forward(ctx, C_F, Cm, weights, th, kind):
        lib = _lib.load()
        dev = C_F.device
        S = C_F.shape[0]
        cf = C_F.detach().float().contiguous()
        cm = Cm.detach().float().contiguous()
        wt = None if weights is None else weights.detach().float().contiguous()
        nbytes = C.c_size_t()
        _lib.check(lib.trase_contrastive_sizes(S, C.byref(nbytes)), "trase_contrastive_sizes")
        ws = _bytes(nbytes.value, dev)
        out2 = torch.empty(2, device=dev)
        d = dev.index if dev.index is not None else torch.cuda.current_device()
        _lib.check(lib.trase_contrastive_forward(_lib.ptr(cm), _lib.ptr(cf), _lib.ptr(wt), S, float(th), int(kind),
                                                 _lib.ptr(out2), _lib.ptr(ws), ws.numel(), d, _stream(dev)),
                   "trase_contrastive_forward")
        ctx.save_for_backward(cf, cm, ws, out2, *(() if wt is None else (wt,)))
        ctx.kind, ctx.th = int(kind), float(th)
        return out2[0]

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        cf, cm, ws, out2, *rest = ctx.saved_tensors
        wt = rest[0] if rest else None
        dev = cf.device
        S = cf.shape[0]
        d_cf = torch.empty_like(cf)
        gg = g.reshape(1).float().contiguous()
        d = dev.index if dev.index is not None else torch.cuda.current_device()
        _lib.check(lib.trase_contrastive_backward(_lib.ptr(cm), _lib.ptr(cf), _lib.ptr(wt), S, ctx.th, ctx.kind,
                                                  _lib.ptr(out2), _lib.ptr(gg), _lib.ptr(ws), ws.numel(), _lib.ptr(d_cf), d,
                                                  _stream(dev)),
                   "trase_contrastive_backward")
        return d_cf, None, None, None, None


def _pixel_pair(C_mat, C_F, th, weights, kind):
    if C_F.device.type != "cuda":
        raise RuntimeError("trase_amd.losses runs on the GPU only (there is no CPU path)")
    if C_F.dim() != 2 or C_F.shape[0] != C_F.shape[1] or C_mat.shape != C_F.shape or (weights is not None and weights.shape != C_F.shape):
        raise ValueError("expected square C, C_F (and weights) of equal shape")
    return _PixelPair.apply(C_F, C_mat, weights, th, kind)


def pixel_mask_correspondence_loss_soft_hard_positive(C, C_F, positive_th=0.75, weights=None, verbose=False, log_tb=False,
                                                      tb_writer=None, iteration=None):
    """utils/loss_utils.py:304-327 (``positive_pixel_pair_loss['soft']``).  Differences: no host synchronisation, so
    the "[WARNING] no positive sample found" print is gone and an empty selection yields a zero TENSOR."""
    return _pixel_pair(C, C_F, positive_th, weights, PAIR_POSITIVE | PAIR_SOFT)


def pixel_mask_correspondence_loss_soft_negative(C, C_F, negative_th=0.5, weights=None, verbose=False, log_tb=False,
                                                 tb_writer=None, iteration=None):
    """utils/loss_utils.py:329-349 (``negative_pixel_pair_loss['soft']``)."""
    return _pixel_pair(C, C_F, negative_th, weights, PAIR_NEGATIVE | PAIR_SOFT)


def pixel_mask_correspondence_loss_positive(C, C_F, positive_th=0.75, weights=None, verbose=False, log_tb=False,
                                            tb_writer=None, iteration=None):
    """utils/loss_utils.py:275-288 (``positive_pixel_pair_loss['all']``; the threshold is unused there as here).  With
    no positive pair at all the reference divides 0 by 0 (nan); this returns 0."""
    return _pixel_pair(C, C_F, positive_th, weights, PAIR_POSITIVE | PAIR_ALL)


def pixel_mask_correspondence_loss_negative(C, C_F, negative_th=0.5, weights=None, verbose=False, log_tb=False,
                                            tb_writer=None, iteration=None):
    """utils/loss_utils.py:290-302 (``negative_pixel_pair_loss['all']``)."""
    return _pixel_pair(C, C_F, negative_th, weights, PAIR_NEGATIVE | PAIR_ALL)


def pixel_mask_correspondence_loss_hard_positive(C, C_F, positive_th=0.75, weights=None, verbose=False, log_tb=False,
                                                 tb_writer=None, iteration=None):
    """utils/loss_utils.py:351-372 (``positive_pixel_pair_loss['hard']``): mean of -w * C_F over the strictly upper
    triangle pairs with C == 1 and C_F < th, without the nonzero() index list (and its host synchronisation)."""
    return _pixel_pair(C, C_F, positive_th, weights, PAIR_POSITIVE | PAIR_HARD)


def pixel_mask_correspondence_loss_hard_negative(C, C_F, negative_th=0.5, weights=None, verbose=False, log_tb=False,
                                                 tb_writer=None, iteration=None):
    """utils/loss_utils.py:374-394 (``negative_pixel_pair_loss['hard']``)."""
    return _pixel_pair(C, C_F, negative_th, weights, PAIR_NEGATIVE | PAIR_HARD)


# the reference's mode tables, utils/loss_utils.py:396-406 (train.py:290-291 indexes them with opt.contrastive_mode)
positive_pixel_pair_loss = {
    "hard": pixel_mask_correspondence_loss_hard_positive,
    "all": pixel_mask_correspondence_loss_positive,
    "soft": pixel_mask_correspondence_loss_soft_hard_positive,
}
negative_pixel_pair_loss = {
    "hard": pixel_mask_correspondence_loss_hard_negative,
    "all": pixel_mask_correspondence_loss_negative,
    "soft": pixel_mask_correspondence_loss_soft_negative,
}


# ---- NNFM style loss (utils/loss_utils.py:223-228) -----------------------------------------------------------------------
class _NNFM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat1, feats2):
        lib = _lib.load()
        dev = feat1.device
        f1 = feat1.detach().float().contiguous()
        f2 = feats2.detach().float().contiguous()
        c, n1, n2 = f1.shape[0], f1.shape[1], f2.shape[1]
        nbytes = C.c_size_t()
        _lib.check(lib.trase_nnfm_sizes(c, n1, n2, C.byref(nbytes)), "trase_nnfm_sizes")
        ws = _bytes(nbytes.value, dev)
        loss = torch.empty(1, device=dev)
        d = dev.index if dev.index is not None else torch.cuda.current_device()
        _lib.check(lib.trase_nnfm_forward(_lib.ptr(f1), _lib.ptr(f2), c, n1, n2, _lib.ptr(loss), _lib.ptr(ws), ws.numel(), d,
                                          _stream(dev)), "trase_nnfm_forward")
        ctx.save_for_backward(f1, f2, ws)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        f1, f2, ws = ctx.saved_tensors
        dev = f1.device
        c, n1, n2 = f1.shape[0], f1.shape[1], f2.shape[1]
        g1 = g.detach().float().reshape(1).contiguous()
        d_f1 = torch.empty_like(f1)
        d = dev.index if dev.index is not None else torch.cuda.current_device()
        _lib.check(lib.trase_nnfm_backward(_lib.ptr(f1), _lib.ptr(f2), c, n1, n2, _lib.ptr(g1), _lib.ptr(ws), ws.numel(),
                                           _lib.ptr(d_f1), d, _stream(dev)), "trase_nnfm_backward")
        return d_f1, None


def loss_nnfm_style(feat1: torch.Tensor, feats2: torch.Tensor) -> torch.Tensor:
    """utils/loss_utils.py:223-228: feat1 (C, N1) rendered-frame features, feats2 (C, N2) style features ->
    mean_i min_j (1 - cosine).  Gradient w.r.t. feat1 only (the reference's style features carry no graph to the scene)."""
    if feat1.device.type != "cuda":
        raise RuntimeError("trase_amd.losses runs on the GPU only (there is no CPU path)")
    if feat1.dim() != 2 or feats2.dim() != 2 or feat1.shape[0] != feats2.shape[0]:
        raise ValueError(f"expected (C, N1) and (C, N2) feature matrices, got {tuple(feat1.shape)} and {tuple(feats2.shape)}")
    if feats2.requires_grad:
        # At the reference call site (train_style_transfer_nnfm.py:202) the style features come out of a VGG whose weights
        # were never frozen (style_transfer/fx.py only calls .eval()), so they DO require grad -- but no optimizer holds the
        # VGG weights: that branch of the graph is dead.  Cut it here instead of refusing the call.
        global _NNFM_WARNED
        if not _NNFM_WARNED:
            import warnings
            warnings.warn("loss_nnfm_style: the style features require grad; no gradient is produced for them "
                          "(the reference never consumes it) -- detaching")
            _NNFM_WARNED = True
        feats2 = feats2.detach()
    return _NNFM.apply(feat1, feats2)


_NNFM_WARNED = False


# ---- image-space losses and style statistics (utils/loss_utils.py:33-44, :230-272; csrc/style.hip) ---------------------------------
PIXEL_MASKED_L1, PIXEL_WEIGHTED_L1, PIXEL_L2 = 0, 1, 2                       # include/trase_rast.h TRASE_PIXEL_*
AUX_NONE, AUX_U8, AUX_F32, AUX_F32_FULL = 0, 1, 2, 3                         # TRASE_PIXEL_AUX_*
STYLE_MAX_C = 512
_CONST_WARNED = set()


def _constant(t, who, what):
    """A ground truth, mask, weight or style / content target takes no gradient: one that requires grad is detached, with one
    warning per function (as loss_nnfm_style does for its style features)."""
    if torch.is_tensor(t) and t.requires_grad:
        if who not in _CONST_WARNED:
            import warnings
            warnings.warn(f"{who}: the {what} requires grad; no gradient is produced for it -- detaching")
            _CONST_WARNED.add(who)
        return t.detach()
    return t


def _dev_index(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


class _PixelLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gt, pitch, aux, aux_kind, kind, chw):
        lib = _lib.load()
        dev = x.device
        xc = x.detach().float().contiguous()
        y = gt if pitch else gt.detach().float().contiguous()
        nbytes = C.c_size_t()
        _lib.check(lib.trase_pixel_loss_ws_bytes(C.byref(nbytes)), "trase_pixel_loss_ws_bytes")
        ws = _bytes(nbytes.value, dev)
        out = torch.empty(1, device=dev)
        _lib.check(lib.trase_pixel_loss_forward(_lib.ptr(xc), _lib.ptr(y), pitch, chw[0], chw[1], chw[2], kind, _lib.ptr(aux), aux_kind,
                                                _lib.ptr(out), _lib.ptr(ws), ws.numel(), _dev_index(dev), _stream(dev)),
                   "trase_pixel_loss_forward")
        ctx.save_for_backward(xc, y, ws, *(() if aux is None else (aux,)))
        ctx.args = (pitch, aux_kind, kind, chw)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        xc, y, ws, *rest = ctx.saved_tensors
        aux = rest[0] if rest else None
        pitch, aux_kind, kind, chw = ctx.args
        dev = xc.device
        g1 = g.detach().float().reshape(1).contiguous()
        d_x = torch.empty_like(xc)
        _lib.check(lib.trase_pixel_loss_backward(_lib.ptr(xc), _lib.ptr(y), pitch, chw[0], chw[1], chw[2], kind, _lib.ptr(aux), aux_kind,
                                                 _lib.ptr(g1), _lib.ptr(ws), ws.numel(), _lib.ptr(d_x), _dev_index(dev), _stream(dev)),
                   "trase_pixel_loss_backward")
        return d_x, None, None, None, None, None, None


_GPU_ONLY = "trase_amd.losses runs on the GPU only (there is no CPU path)"


def _pixel_operands(who, network_output, gt):
    """(what the kernels read as ground truth, its pitch: 0 = an fp32 tensor).  Shapes are checked before the device."""
    if not torch.is_tensor(network_output) or network_output.dim() != 3 or not (torch.is_tensor(gt) or isinstance(gt, ByteFrame)) \
            or tuple(network_output.shape) != tuple(gt.shape) or network_output.numel() < 1:
        raise ValueError(f"{who}: expected two (C,H,W) images of equal shape, got "
                         f"{tuple(network_output.shape) if torch.is_tensor(network_output) else type(network_output).__name__} and "
                         f"{tuple(gt.shape) if hasattr(gt, 'shape') else type(gt).__name__}")
    if network_output.numel() >= 2 ** 31:
        raise ValueError(f"{who}: fewer than 2^31 elements are supported")
    if network_output.device.type != "cuda":
        raise RuntimeError(_GPU_ONLY)
    if gt.device != network_output.device:
        raise ValueError(f"{who}: the ground truth is on {gt.device}, the image on {network_output.device}")
    if isinstance(gt, ByteFrame):
        return gt.data, gt.pitch
    return _constant(gt, who, "ground truth"), 0


def masked_l1_loss(network_output: torch.Tensor, gt, mask: torch.Tensor) -> torch.Tensor:
    """utils/loss_utils.py:33-37: ``sum(|x - gt| * m) / (C * sum(m))``, mask (H, W) bool, uint8 or float (the value of a uint8 mask
    counts, as ``mask.float()`` does); gt a tensor or a ByteFrame.  An all-zero mask gives 0 with a zero gradient (the reference
    divides 0 by 0)."""
    if not torch.is_tensor(mask) or mask.dim() != 2 or not torch.is_tensor(network_output) or tuple(mask.shape) != tuple(network_output.shape[1:]):
        raise ValueError(f"masked_l1_loss: expected an (H, W) mask for a {tuple(network_output.shape)} image, got "
                         f"{tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__}")
    if not (mask.dtype in (torch.bool, torch.uint8) or mask.dtype.is_floating_point):
        raise TypeError(f"masked_l1_loss: the mask must be bool, uint8 or float (got {mask.dtype})")
    y, pitch = _pixel_operands("masked_l1_loss", network_output, gt)
    if mask.device != network_output.device:
        raise ValueError(f"masked_l1_loss: the mask is on {mask.device}, the image on {network_output.device}")
    mask = _constant(mask, "masked_l1_loss", "mask")
    if mask.dtype == torch.bool:
        aux, kind = mask.contiguous().view(torch.uint8), AUX_U8
    elif mask.dtype == torch.uint8:
        aux, kind = mask.contiguous(), AUX_U8
    else:
        aux, kind = mask.float().contiguous(), AUX_F32
    return _PixelLoss.apply(network_output, y, pitch, aux, kind, PIXEL_MASKED_L1, tuple(network_output.shape))


def weighted_l1_loss(network_output: torch.Tensor, gt, weight: torch.Tensor) -> torch.Tensor:
    """utils/loss_utils.py:39-41: ``mean(|x - gt| * w)``, weight (H, W), (1, H, W) or (C, H, W)."""
    if not torch.is_tensor(network_output) or network_output.dim() != 3:
        raise ValueError("weighted_l1_loss: expected a (C,H,W) image")
    c, h, w = network_output.shape
    if not torch.is_tensor(weight) or tuple(weight.shape) not in ((h, w), (1, h, w), (c, h, w)):
        raise ValueError(f"weighted_l1_loss: expected an (H, W), (1, H, W) or (C, H, W) weight for a {(c, h, w)} image, got "
                         f"{tuple(weight.shape) if torch.is_tensor(weight) else type(weight).__name__}")
    if not weight.dtype.is_floating_point:
        raise TypeError(f"weighted_l1_loss: the weight must be float (got {weight.dtype})")
    y, pitch = _pixel_operands("weighted_l1_loss", network_output, gt)
    if weight.device != network_output.device:
        raise ValueError(f"weighted_l1_loss: the weight is on {weight.device}, the image on {network_output.device}")
    weight = _constant(weight, "weighted_l1_loss", "weight")
    kind = AUX_F32_FULL if weight.dim() == 3 and weight.shape[0] == c and c > 1 else AUX_F32
    return _PixelLoss.apply(network_output, y, pitch, weight.float().contiguous(), kind, PIXEL_WEIGHTED_L1, (c, h, w))


def l2_loss(network_output: torch.Tensor, gt) -> torch.Tensor:
    """utils/loss_utils.py:43-44: ``mean((x - gt)^2)`` of an image and its ground truth (a tensor or a ByteFrame), or of any two
    fp32 tensors of equal shape (fewer than 2^31 elements)."""
    if isinstance(gt, ByteFrame):
        y, pitch = _pixel_operands("l2_loss", network_output, gt)
        return _PixelLoss.apply(network_output, y, pitch, None, AUX_NONE, PIXEL_L2, tuple(network_output.shape))
    if not torch.is_tensor(network_output) or not torch.is_tensor(gt) or tuple(gt.shape) != tuple(network_output.shape) \
            or network_output.numel() < 1:
        raise ValueError(f"l2_loss: expected two non-empty tensors of equal shape, got "
                         f"{tuple(network_output.shape) if torch.is_tensor(network_output) else type(network_output).__name__} and "
                         f"{tuple(gt.shape) if torch.is_tensor(gt) else type(gt).__name__}")
    if network_output.numel() >= 2 ** 31:
        raise ValueError("l2_loss: fewer than 2^31 elements are supported")
    if network_output.device.type != "cuda":
        raise RuntimeError(_GPU_ONLY)
    if gt.device != network_output.device:
        raise ValueError(f"l2_loss: the second tensor is on {gt.device}, the first on {network_output.device}")
    gt = _constant(gt, "l2_loss", "second tensor")
    return _PixelLoss.apply(network_output, gt, 0, None, AUX_NONE, PIXEL_L2, (1, 1, network_output.numel()))


def cal_mse_content_loss(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """utils/loss_utils.py:271-272: the l2 kernel on two feature tensors (bitwise the content term of style_statistics_loss)."""
    return l2_loss(x, y)


def _features_2d(t, who):
    """(C, n) view of a (1, C, h, w) or (C, n) feature tensor"""
    if not torch.is_tensor(t) or not ((t.dim() == 4 and t.shape[0] == 1) or t.dim() == 2):
        raise ValueError(f"{who}: expected (1, C, h, w) or (C, n) features, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    c = t.shape[1] if t.dim() == 4 else t.shape[0]
    n = t.numel() // c if c else 0
    if not 1 <= c <= STYLE_MAX_C or n < 1 or n >= 2 ** 31:
        raise ValueError(f"{who}: need 1 <= C <= {STYLE_MAX_C} channels and 1 <= n < 2^31 positions, got {tuple(t.shape)}")
    if t.device.type != "cuda":
        raise RuntimeError(_GPU_ONLY)
    return t.reshape(c, n) if t.dim() == 4 else t


def _style_ws(c, n, dev):
    nbytes = C.c_size_t()
    _lib.check(_lib.load().trase_style_ws_bytes(c, n, C.byref(nbytes)), "trase_style_ws_bytes")
    return _bytes(nbytes.value, dev)


def _grad_gemm(D, a, b, cc, x, y, g):
    """trase_style_grad_gemm: g * (2 D x + a + b * x + cc * (x - y)), every part optional"""
    dev = x.device
    dx = torch.empty_like(x)
    g1 = None if g is None else g.detach().float().reshape(1).contiguous()
    _lib.check(_lib.load().trase_style_grad_gemm(_lib.ptr(D), _lib.ptr(a), _lib.ptr(b), float(cc), _lib.ptr(x), _lib.ptr(y), x.shape[0],
                                                 x.shape[1], _lib.ptr(g1), _lib.ptr(dx), _dev_index(dev), _stream(dev)),
               "trase_style_grad_gemm")
    return dx


class _Gram(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f):
        x = f.detach().float().contiguous()
        dev = x.device
        c, n = x.shape
        ws = _style_ws(c, n, dev)
        G = torch.empty(c, c, device=dev)
        _lib.check(_lib.load().trase_gram_matrix(_lib.ptr(x), c, n, _lib.ptr(G), _lib.ptr(ws), ws.numel(), _dev_index(dev), _stream(dev)),
                   "trase_gram_matrix")
        ctx.save_for_backward(x)
        return G

    @staticmethod
    def backward(ctx, gG):
        (x,) = ctx.saved_tensors
        D = (0.5 * (gG + gG.t())).float().contiguous()            # d / dx of <gG, x x^T> = (gG + gG^T) x = 2 D x
        return _grad_gemm(D, None, None, 0.0, x, None, None)


class _MeanStd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, eps):
        x = f.detach().float().contiguous()
        dev = x.device
        c, n = x.shape
        ws = _style_ws(c, n, dev)
        mean, std = torch.empty(c, device=dev), torch.empty(c, device=dev)
        _lib.check(_lib.load().trase_mean_std(_lib.ptr(x), c, n, float(eps), _lib.ptr(mean), _lib.ptr(std), _lib.ptr(ws), ws.numel(),
                                              _dev_index(dev), _stream(dev)), "trase_mean_std")
        ctx.save_for_backward(x, mean, std)
        ctx.eps = float(eps)
        return mean, std

    @staticmethod
    def backward(ctx, g_mean, g_std):
        x, mean, std = ctx.saved_tensors
        n = x.shape[1]
        z = torch.zeros_like(mean)
        g_mean = z if g_mean is None else g_mean.float()
        g_std = z if g_std is None else g_std.float()
        sd = std - ctx.eps
        b = torch.where(sd > 0, g_std / ((n - 1) * sd), z)        # a channel of zero variance takes no gradient from the std
        a = g_mean / n - b * mean
        return _grad_gemm(None, a.contiguous(), b.contiguous(), 0.0, x, None, None), None


def gram_matrix(tensor: torch.Tensor) -> torch.Tensor:
    """utils/loss_utils.py:240-249: (1, C, h, w) or (C, n) features -> the (C, C) fp32 matrix ``X X^T`` on the exact-fp32 matrix
    instruction: fp32 chains of 1024 positions, the chain results added in float64 in order and rounded once.  Symmetric bit for
    bit; two calls give the same bits."""
    return _Gram.apply(_features_2d(tensor, "gram_matrix"))


def calc_mean_std(x: torch.Tensor, eps: float = 1e-8):
    """utils/loss_utils.py:230-238: (mean, std), each (1, C, 1); std is the unbiased standard deviation with eps added in fp32.
    Two passes in float64 (the sum, then the squared deviations from the float64 mean)."""
    f = _features_2d(x, "calc_mean_std")
    if f.shape[1] < 2:
        raise ValueError("calc_mean_std: the unbiased standard deviation needs n >= 2 positions")
    mean, std = _MeanStd.apply(f, eps)
    return mean.reshape(1, -1, 1), std.reshape(1, -1, 1)


class StyleTargets:
    """What style_statistics_loss compares a feature map with: the style map's Gram matrix (C, C), channel means and standard
    deviations (C,), and optionally a content map (C, n) of the rendered features' size.  Built once per style image."""

    def __init__(self, gram=None, mean=None, std=None, content=None):
        self.gram, self.mean, self.std, self.content = gram, mean, std, content

    @staticmethod
    def from_features(style_feats: torch.Tensor, content_feats: torch.Tensor = None) -> "StyleTargets":
        with torch.no_grad():
            f = _features_2d(style_feats, "StyleTargets.from_features").detach()
            gram = gram_matrix(f)
            mean = std = None
            if f.shape[1] >= 2:
                mean, std = (t.reshape(-1).contiguous() for t in calc_mean_std(f))
            content = None
            if content_feats is not None:
                content = _features_2d(content_feats, "StyleTargets.from_features").detach().float().contiguous()
        return StyleTargets(gram, mean, std, content)


class _StyleNode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, gram, mean, std, content, gw, aw, cw):
        x = f.detach().float().contiguous()
        dev = x.device
        c, n = x.shape
        ws = _style_ws(c, n, dev)
        out4 = torch.empty(4, device=dev)
        saved = torch.empty(c * c + 2 * c, device=dev)
        _lib.check(_lib.load().trase_style_node_forward(_lib.ptr(x), c, n, _lib.ptr(gram), _lib.ptr(mean), _lib.ptr(std), _lib.ptr(content),
                                                        gw, aw, cw, _lib.ptr(out4), _lib.ptr(saved), _lib.ptr(ws), ws.numel(),
                                                        _dev_index(dev), _stream(dev)), "trase_style_node_forward")
        ctx.save_for_backward(x, saved, *(() if content is None else (content,)))
        ctx.weights = (gw, aw, cw)
        ctx.mark_non_differentiable(out4)
        return out4[0], out4

    @staticmethod
    def backward(ctx, g, _g_parts):
        x, saved, *rest = ctx.saved_tensors
        gw, aw, cw = ctx.weights
        c, n = x.shape
        D = saved[:c * c] if gw != 0.0 else None
        a = saved[c * c:c * c + c] if aw != 0.0 else None
        b = saved[c * c + c:] if aw != 0.0 else None
        y = rest[0] if cw != 0.0 else None
        return _grad_gemm(D, a, b, 2.0 * cw / (float(c) * float(n)), x, y, g), None, None, None, None, None, None, None


def style_statistics_loss(feats: torch.Tensor, targets: StyleTargets, *, gram_weight: float = 0.0, adain_weight: float = 0.0,
                          content_weight: float = 0.0, with_parts: bool = False):
    """``gram_weight * mean((G - G_s)^2) / (C h w) + adain_weight * (mse(mean, mean_s) + mse(std, std_s)) + content_weight *
    mse(feats, content)`` of (1, C, h, w) or (C, n) features as ONE autograd node: a statistics pass, the Gram launches and one
    reduction forward (no read-back), one GEMM-shaped launch backward.  A term whose weight is 0 costs nothing and needs no
    target.  with_parts: also the detached weighted (gram, adain, content) terms.  A channel of zero variance takes no gradient
    from the std term (the reference's torch.std gives 0 / 0 there)."""
    if not isinstance(targets, StyleTargets):
        raise TypeError("style_statistics_loss: targets must be a StyleTargets (StyleTargets.from_features(style_feats) makes one)")
    gw, aw, cw = float(gram_weight), float(adain_weight), float(content_weight)
    if gw == 0.0 and aw == 0.0 and cw == 0.0:
        raise ValueError("style_statistics_loss: every weight is 0")
    f = _features_2d(feats, "style_statistics_loss")
    c, n = f.shape
    gram = mean = std = content = None
    if gw != 0.0:
        if targets.gram is None or tuple(targets.gram.shape) != (c, c):
            raise ValueError(f"style_statistics_loss: the Gram term needs a ({c}, {c}) style Gram matrix")
        gram = _constant(targets.gram, "style_statistics_loss", "style target").float().contiguous()
    if aw != 0.0:
        if n < 2:
            raise ValueError("style_statistics_loss: the AdaIN term needs n >= 2 positions")
        if targets.mean is None or targets.std is None or targets.mean.numel() != c or targets.std.numel() != c:
            raise ValueError(f"style_statistics_loss: the AdaIN term needs the style mean and std of {c} channels")
        mean = _constant(targets.mean, "style_statistics_loss", "style target").float().reshape(-1).contiguous()
        std = _constant(targets.std, "style_statistics_loss", "style target").float().reshape(-1).contiguous()
    if cw != 0.0:
        if targets.content is None or targets.content.numel() != c * n:
            raise ValueError(f"style_statistics_loss: the content term needs a content map of the features' size ({c}, {n})")
        if c * n >= 2 ** 31:
            raise ValueError("style_statistics_loss: the content term supports fewer than 2^31 elements")
        content = _constant(targets.content, "style_statistics_loss", "content target").float().reshape(c, n).contiguous()
    for t in (gram, mean, std, content):
        if t is not None and t.device != f.device:
            raise ValueError(f"style_statistics_loss: a target is on {t.device}, the features on {f.device}")
    loss, parts = _StyleNode.apply(f, gram, mean, std, content, gw, aw, cw)
    return (loss, parts[1], parts[2], parts[3]) if with_parts else loss


def cal_adain_style_loss(x: torch.Tensor, y) -> torch.Tensor:
    """utils/loss_utils.py:251-262; y: the style features, or the ``(mean, std)`` pair of calc_mean_std computed once."""
    if isinstance(y, (tuple, list)):
        if len(y) != 2:
            raise ValueError("cal_adain_style_loss: y is a feature tensor or a (mean, std) pair")
        t = StyleTargets(mean=y[0], std=y[1])
    else:
        with torch.no_grad():
            m, s = calc_mean_std(_constant(y, "cal_adain_style_loss", "style features"))
        t = StyleTargets(mean=m, std=s)
    return style_statistics_loss(x, t, adain_weight=1.0)


def cal_style_loss(target: torch.Tensor, style: torch.Tensor, weight) -> torch.Tensor:
    """utils/loss_utils.py:264-269: ``weight * mean((G_t - G_s)^2) / (C h w)`` with the target's dimensions; style: features of any
    spatial size, or a (C, C) Gram matrix computed once."""
    f = _features_2d(target, "cal_style_loss")
    if torch.is_tensor(style) and style.dim() == 2 and tuple(style.shape) == (f.shape[0], f.shape[0]):
        gram = style
    else:
        with torch.no_grad():
            gram = gram_matrix(_constant(style, "cal_style_loss", "style features"))
    return style_statistics_loss(target, StyleTargets(gram=gram), gram_weight=float(weight))


# the two k-NN graph losses of utils/loss_utils.py (:132-152, :179-221) live in trase_amd/neighbors.py
from .neighbors import loss_reg_3d_feature, loss_rigid_body_motion_reg_loss, polar_rotation, rigid_fit  # noqa: E402,F401
# the two dense-search losses (:154-175, :89-130) and their search too
from .neighbors import dense_topk, loss_cls_3d, loss_feature3d  # noqa: E402,F401
