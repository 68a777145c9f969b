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


# the two k-NN graph losses of utils/loss_utils.py (:132-152, :179-221) live in trase_amd/neighbors.py
from .neighbors import loss_reg_3d_feature, loss_rigid_body_motion_reg_loss, polar_rotation, rigid_fit  # noqa: E402,F401
# the two dense-search losses (:154-175, :89-130) and their search too
from .neighbors import dense_topk, loss_cls_3d, loss_feature3d  # noqa: E402,F401
