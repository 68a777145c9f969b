"""The FEATURE-state loss head of train.py:251-296 without any S x S matrix.

The reference builds, per iteration, ``C_matrix`` (utils/feature_utils.py:40-49), ``C_F_matrix`` (:51-57) and
``pixel_weights`` (:28-38, through an N x H x W int64 temporary), all S x S with S ~ 5000, feeds them to the two pair
losses (utils/loss_utils.py:275-406) and indexes them again for the two logged similarities (train.py:295-296): about
10 ms of PyTorch around a 1.6 ms rasterizer.  Every entry of those matrices is a function of per-pixel factors, so the
kernels of ``csrc/pairhead.hip`` evaluate them on the fly:

    cover, sizes   = mask_stats(sam_masks)                                     # one pass over the masks
    sampled_pixel, sampled_mask = get_sample_pixel_and_mask(sam_masks, 5000, 50, cover_count=cover)
    loss_pos, loss_neg, pos_sim, neg_sim = contrastive_head(rendered_features, sam_masks, sampled_pixel, sampled_mask,
                                                            mode="soft", positive_th=0.75, negative_th=0.5,
                                                            mask_size=sizes)
    loss = loss_pos + loss_neg + opt.rfn * feature_norm_reg(full_res_rendered_features)

``rendered_features`` is the (32, Hr, Wr) feature image as rendered.  When the masks have another size (every
``--downsample_mask`` recipe: a half or a quarter, not always an integral ratio) the head takes each sampled pixel's column as
the four bilinear taps train.py:283-284's ``interpolate`` would blend -- the resized map is never formed -- and the backward
writes the full-resolution gradient in one dense pass without atomics; ``with_norm_reg=True`` then is the reference's
composition: norm at render resolution, pairs at mask resolution.  There is no CPU path.

Wherever ``sam_masks`` is accepted it may be a ``PackedMasks``: the view's masks as the bit stream the reference saves
(extract_masks.py:91-99), resident on the device at an eighth of the bool bytes and read in place (``csrc/maskbits.hip``) --
train.py:245-249's per-iteration ``np.array(bitarray.tolist())`` + ``.cuda()`` becomes, once per view,

    sam_masks = PackedMasks.from_saved(torch.load(path), "cuda")

and every result is bitwise what the bool tensor gives.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .rasterizer import _bytes, _stream

_MODES = {"soft": 0, "all": 1, "hard": 2}


def _dev_index(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _pad16(nbytes: int) -> int:
    return (nbytes + 15) // 16 * 16


_BITREV = None      # 256-entry table: a byte with its bits reversed (a little-endian bitarray's byte -> the stream's)


class PackedMasks:
    """N x H x W bool masks as ``numpy.packbits(masks.reshape(-1))``: stream bit i is bit ``7 - (i & 7)`` of byte ``i >> 3``, mask n
    starts at stream bit ``n * H * W``, only the last byte is padded.  ``bits`` is a contiguous uint8 tensor whose storage starts
    on a 16-byte boundary and whose length is a multiple of 16, at least ``ceil(N * H * W / 8)``; what it holds behind bit
    ``N * H * W`` is never looked at."""
    __slots__ = ("bits", "N", "H", "W")

    def __init__(self, bits: torch.Tensor, N: int, H: int, W: int):
        N, H, W = int(N), int(H), int(W)
        if N < 1 or H < 1 or W < 1:
            raise ValueError(f"PackedMasks: N, H, W must be >= 1 (got {N}, {H}, {W})")
        if not torch.is_tensor(bits) or bits.dtype != torch.uint8 or bits.dim() != 1 or not bits.is_contiguous():
            raise ValueError("PackedMasks: bits must be a contiguous 1-d uint8 tensor")
        need = (N * H * W + 7) // 8
        if bits.numel() % 16 or bits.numel() < need:
            raise ValueError(f"PackedMasks: bits holds {bits.numel()} bytes; need a multiple of 16, at least {need}")
        if bits.data_ptr() % 16:
            raise ValueError("PackedMasks: bits must start on a 16-byte boundary")
        self.bits, self.N, self.H, self.W = bits, N, H, W

    @property
    def shape(self):
        return (self.N, self.H, self.W)

    @property
    def device(self):
        return self.bits.device

    def _gpu(self):
        if self.bits.device.type != "cuda":
            raise RuntimeError("trase_amd.feature_head runs on the GPU only (there is no CPU path)")
        return self

    @staticmethod
    @torch.no_grad()
    def from_bool(masks: torch.Tensor) -> "PackedMasks":
        """Pack an (N, H, W) bool or byte tensor (any non-zero value is set) on the device."""
        if masks.device.type != "cuda":
            raise RuntimeError("trase_amd.feature_head runs on the GPU only (there is no CPU path)")
        if masks.dim() != 3 or masks.dtype not in (torch.bool, torch.uint8, torch.int8):
            raise ValueError("masks must be [N, H, W] bool or byte")
        m = masks.contiguous().view(torch.uint8)
        N, H, W = m.shape
        dev = m.device
        bits = torch.empty(_pad16((N * H * W + 7) // 8), dtype=torch.uint8, device=dev)
        lib = _lib.load()
        _lib.check(lib.trase_pack_masks(_lib.ptr(m), N, H * W, _lib.ptr(bits), bits.numel(), _dev_index(dev), _stream(dev)),
                   "trase_pack_masks")
        return PackedMasks(bits, N, H, W)

    @torch.no_grad()
    def to_bool(self) -> torch.Tensor:
        """The (N, H, W) bool tensor, unpacked on the device."""
        dev = self._gpu().bits.device
        out = torch.empty(self.shape, dtype=torch.uint8, device=dev)
        lib = _lib.load()
        _lib.check(lib.trase_unpack_masks(_lib.ptr(self.bits), self.bits.numel(), self.N, self.H * self.W, _lib.ptr(out), _dev_index(dev),
                                          _stream(dev)), "trase_unpack_masks")
        return out.view(torch.bool)

    @staticmethod
    def host_stream(obj):
        """(padded uint8 numpy buffer, N, H, W) of the reference's saved dict ``{'masks', 'N', 'H', 'W'}``: ``'masks'`` is ``bytes``,
        a uint8 array or tensor, or anything with ``.tobytes()`` (a ``bitarray``; a ``.endian()`` of ``'little'`` is bit-reversed per
        byte through a 256-entry table).  One copy into the zero-padded buffer; never a list of bools."""
        import numpy as np
        global _BITREV
        N, H, W = int(obj["N"]), int(obj["H"]), int(obj["W"])
        if N < 1 or H < 1 or W < 1:
            raise ValueError(f"PackedMasks: N, H, W must be >= 1 (got {N}, {H}, {W})")
        need = (N * H * W + 7) // 8
        raw = obj["masks"]
        little = False
        if torch.is_tensor(raw):
            if raw.dtype != torch.uint8:
                raise ValueError("PackedMasks: a tensor of stream bytes must be uint8")
            src = raw.detach().cpu().contiguous().reshape(-1).numpy()
        elif isinstance(raw, np.ndarray):
            if raw.dtype != np.uint8:
                raise ValueError("PackedMasks: an array of stream bytes must be uint8")
            src = raw.reshape(-1)
        elif isinstance(raw, (bytes, bytearray, memoryview)):
            src = np.frombuffer(raw, dtype=np.uint8)
        elif hasattr(raw, "tobytes"):
            little = hasattr(raw, "endian") and raw.endian() == "little"
            src = np.frombuffer(raw.tobytes(), dtype=np.uint8)
        else:
            raise ValueError(f"PackedMasks: cannot read a mask stream from {type(raw).__name__}")
        if src.size < need:
            raise ValueError(f"PackedMasks: {src.size} stream bytes for {N} x {H} x {W} masks (need {need})")
        buf = np.zeros(_pad16(need), dtype=np.uint8)
        if little:
            if _BITREV is None:
                _BITREV = np.array([int(f"{i:08b}"[::-1], 2) for i in range(256)], dtype=np.uint8)
            np.take(_BITREV, src[:need], out=buf[:need])
        else:
            buf[:need] = src[:need]
        return buf, N, H, W

    @staticmethod
    def from_saved(obj, device="cuda") -> "PackedMasks":
        """The reference's saved masks (extract_masks.py:91-99) on ``device``: one host copy (host_stream), one upload."""
        buf, N, H, W = PackedMasks.host_stream(obj)
        return PackedMasks(torch.from_numpy(buf).to(device), N, H, W)


def _masks_u8(sam_masks: torch.Tensor) -> torch.Tensor:
    if sam_masks.device.type != "cuda":
        raise RuntimeError("trase_amd.feature_head runs on the GPU only (there is no CPU path)")
    if sam_masks.dim() != 3:
        raise ValueError("sam_masks must be [N, H, W]")
    m = sam_masks if sam_masks.dtype == torch.bool else (sam_masks != 0)
    return m.contiguous().view(torch.uint8)


@torch.no_grad()
def mask_stats(sam_masks):
    """(cover_count [H, W] int32, mask_size [N] int32): ``sam_masks.sum(dim=0)`` and ``sam_masks.sum(-1).sum(-1)``
    (utils/feature_utils.py:23, :30) in one pass over the masks (a tensor or a PackedMasks)."""
    packed = isinstance(sam_masks, PackedMasks)
    m = sam_masks._gpu() if packed else _masks_u8(sam_masks)
    N, H, W = m.shape
    dev = m.device
    cover = torch.empty((H, W), dtype=torch.int32, device=dev)
    size = torch.empty((N,), dtype=torch.int32, device=dev)
    lib = _lib.load()
    name = "trase_mask_stats_bits" if packed else "trase_mask_stats"
    masks = (_lib.ptr(m.bits), m.bits.numel()) if packed else (_lib.ptr(m),)
    _lib.check(getattr(lib, name)(*masks, N, H * W, _lib.ptr(cover), _lib.ptr(size), _dev_index(dev), _stream(dev)), name)
    return cover, size


@torch.no_grad()
def get_sample_pixel_and_mask(sam_masks, num_sampled_pixels, num_sampled_masks, cover_count=None, rng="cpu", exclude=None):
    """utils/feature_utils.py:17-26, the non-mask region taken from ``mask_stats`` instead of an int64 N x H x W
    reduction.  ``rng="cpu"`` (default) makes the same draws as the reference -- ``torch.rand`` on the CPU generator, in
    the same order, then copied to the GPU -- which costs ~3.4 ms at 1080p (2 M scalar Mersenne-Twister draws + an 8 MB
    copy); ``rng="cuda"`` draws the same Bernoulli fields from torch's CUDA generator (~0.03 ms).
    ``exclude``: an (H, W) bool tensor of pixels to leave out of the draw (``black_mask`` of train.py:253-269's
    ``mask_black_bg``), removed here -- before the count tag is attached -- so that the head stays on its sync-free path; the tag
    keeps the draw's target count, which is an upper estimate for buffer sizing only."""
    if rng not in ("cpu", "cuda"):
        raise ValueError("rng must be 'cpu' or 'cuda'")
    if exclude is not None and tuple(exclude.shape) != tuple(sam_masks.shape[-2:]):
        raise ValueError(f"exclude must be [{sam_masks.shape[-2]}, {sam_masks.shape[-1]}] (got {list(exclude.shape)})")
    if cover_count is None:
        cover_count, _ = mask_stats(sam_masks)
    dev = sam_masks.device
    where = dev if rng == "cuda" else "cpu"
    mask_sample_rate = num_sampled_masks / (sam_masks.shape[0])
    sampled_mask = torch.rand(sam_masks.shape[0], device=where).to(dev) < mask_sample_rate
    pixel_sample_rate = num_sampled_pixels / (sam_masks.shape[-1] * sam_masks.shape[-2])
    sampled_pixel = torch.rand(sam_masks.shape[-2], sam_masks.shape[-1], device=where).to(dev) < pixel_sample_rate
    sampled_pixel = torch.logical_and(sampled_pixel, cover_count != 0)
    if exclude is not None:
        sampled_pixel = torch.logical_and(sampled_pixel, torch.logical_not((exclude != 0).to(dev)))
    # (how many pixels the draw aims at: lets contrastive_head size its buffers without reading the count back from the device)
    # tied to THIS tensor's contents: (target count, number of pixels of the draw, version counter) -- an in-place edit afterwards
    # (`sampled_pixel |= ...`) bumps the version and contrastive_head falls back to counting
    sampled_pixel._trase_expected_count = (int(num_sampled_pixels), int(sampled_pixel.numel()), int(sampled_pixel._version))
    return sampled_pixel, sampled_mask


_COUNT_CHECKS: list = []      # (event, pinned int32[2] copy of the device count, capacity) of sync-free compactions not yet verified
_COUNT_FREE: list = []        # verified (pinned buffer, event) pairs, reused (no pinned allocation / event creation per iteration)


def _poll_count_checks(block: bool = False):
    """A compaction whose true count (count[1]) exceeded the buffer it was given dropped its highest pixels: reported here, by a
    LATER call of the head (or check_sampled_counts()), without making any call wait for the device."""
    keep = []
    for ev, pin, cap in _COUNT_CHECKS:
        if block:
            ev.synchronize()
        if block or ev.query():
            if len(_COUNT_FREE) < 8:
                _COUNT_FREE.append((pin, ev))
            if int(pin[1]) > cap:
                _COUNT_CHECKS[:] = []
                raise RuntimeError(f"trase_amd.feature_head: a sync-free contrastive_head call sampled {int(pin[1])} pixels but its index "
                                   f"buffer held {cap}: the highest pixels of that draw were dropped from its losses.  Pass a boolean "
                                   f"mask that does not come from get_sample_pixel_and_mask (counted on the host) for such draws.")
        else:
            keep.append((ev, pin, cap))
    _COUNT_CHECKS[:] = keep


def check_sampled_counts():
    """Blocking: verify every sync-free contrastive_head call issued so far (see _poll_count_checks)."""
    _poll_count_checks(block=True)


def _featnorm_forward(lib, f):
    """out2 = [(1 - mean norm) ** 2, mean norm] of the contiguous float32 (F, ...) image ``f`` (train.py:281-282)"""
    dev = f.device
    F = f.shape[0]
    HW = f.numel() // F
    nbytes = C.c_size_t()
    _lib.check(lib.trase_featnorm_sizes(HW, C.byref(nbytes)), "trase_featnorm_sizes")
    ws = _bytes(nbytes.value, dev)
    out2 = torch.empty(2, device=dev)
    _lib.check(lib.trase_featnorm_forward(_lib.ptr(f), F, HW, _lib.ptr(out2), _lib.ptr(ws), ws.numel(), _dev_index(dev), _stream(dev)),
               "trase_featnorm_forward")
    return out2


# (packed masks, resized) -> the forward's entry point
_FORWARD = {(False, False): "trase_pairhead_forward_n", (True, False): "trase_pairhead_forward_bits",
            (False, True): "trase_pairhead_forward_resized", (True, True): "trase_pairhead_forward_bits_resized"}


class _PairHead(torch.autograd.Function):
    """``resized``: the features have another size than the masks (or are to be treated so): the sampled columns are bilinear taps of
    the (32, Hr, Wr) image, and the backward writes every element of its gradient once (taps and, with_reg, the regulariser's term in
    one pass).  Otherwise the columns are read in place and the backward scatters them into the image."""

    @staticmethod
    def forward(ctx, feats, masks_u8, sampled_mask_u8, n_sampled, mask_size, pix, mode, pth, nth, use_w, with_reg, s_dev=None, resized=False):
        # s_dev: int32[2] on the device, s_dev[0] = number of valid entries of `pix` (trase_compact_pixels); None: all of them
        lib = _lib.load()
        dev = feats.device
        F, Hr, Wr = feats.shape
        N, h, w = masks_u8.shape
        S = pix.numel()
        f = feats.detach().float().contiguous()
        geom = (Hr, Wr, h, w) if resized else (Hr * Wr,)
        nbytes = C.c_size_t()
        if resized:
            _lib.check(lib.trase_pairhead_sizes_resized(S, *geom, C.byref(nbytes)), "trase_pairhead_sizes_resized")
        else:
            _lib.check(lib.trase_pairhead_sizes(S, C.byref(nbytes)), "trase_pairhead_sizes")
        ws = _bytes(nbytes.value, dev)
        out8 = torch.empty(8, device=dev)
        packed = isinstance(masks_u8, PackedMasks)      # the stream in place of the bool bytes: same workspace, same backward
        masks = (_lib.ptr(masks_u8.bits), masks_u8.bits.numel()) if packed else (_lib.ptr(masks_u8),)
        name = _FORWARD[packed, resized]
        _lib.check(getattr(lib, name)(_lib.ptr(f), F, *geom, *masks, N, _lib.ptr(sampled_mask_u8), int(n_sampled), _lib.ptr(mask_size),
                                      _lib.ptr(pix), S, _lib.ptr(s_dev), int(mode), float(pth), float(nth), int(use_w), _lib.ptr(out8),
                                      _lib.ptr(ws), ws.numel(), _dev_index(dev), _stream(dev)),
                   "trase_pairhead_forward" if name == "trase_pairhead_forward_n" else name)
        ctx.s_dev = s_dev
        sims = out8[4:6].clone()
        ctx.mark_non_differentiable(sims)
        ctx.cfg = (F, Hr, Wr, geom, S, int(mode), float(pth), float(nth), int(use_w), bool(with_reg), bool(resized))
        if not with_reg:
            ctx.save_for_backward(ws, out8, pix)
            return out8[0], out8[2], sims
        # the regulariser of train.py:280-282 on the image as rendered (before any resize)
        out2 = _featnorm_forward(lib, f)
        ctx.save_for_backward(ws, out8, pix, f, out2)
        return out8[0], out8[2], sims, out2[0]

    @staticmethod
    def backward(ctx, g_pos, g_neg, _g_sims, g_reg=None):
        lib = _lib.load()
        F, Hr, Wr, geom, S, mode, pth, nth, use_w, with_reg, resized = ctx.cfg
        ws, out8, pix = ctx.saved_tensors[:3]
        dev = ws.device
        d, st = _dev_index(dev), _stream(dev)
        g2 = torch.stack([g_pos.reshape(()), g_neg.reshape(())]).float().contiguous()
        d_feats = torch.empty((F, Hr, Wr), device=dev)
        f = out2 = gg = None
        if with_reg:
            f, out2 = ctx.saved_tensors[3:]
            gg = g_reg.reshape(1).float().contiguous()
        if resized:         # one dense pass: the taps and, given its three pointers, the regulariser's term
            _lib.check(lib.trase_pairhead_backward_resized(F, *geom, _lib.ptr(pix), S, _lib.ptr(ctx.s_dev), mode, pth, nth, use_w, _lib.ptr(out8),
                                                           _lib.ptr(g2), _lib.ptr(ws), ws.numel(), _lib.ptr(f), _lib.ptr(out2), _lib.ptr(gg),
                                                           _lib.ptr(d_feats), d, st), "trase_pairhead_backward_resized")
            return (d_feats,) + (None,) * 12
        # the regulariser's dense gradient is written first and the S sampled columns are added into it (no zero-fill, no separate
        # accumulation pass)
        if with_reg:
            _lib.check(lib.trase_featnorm_backward(_lib.ptr(f), F, *geom, _lib.ptr(out2), _lib.ptr(gg), _lib.ptr(d_feats), d, st),
                       "trase_featnorm_backward")
        _lib.check(lib.trase_pairhead_backward_n(F, *geom, _lib.ptr(pix), S, _lib.ptr(ctx.s_dev), mode, pth, nth, use_w, _lib.ptr(out8),
                                                 _lib.ptr(g2), _lib.ptr(ws), ws.numel(), 1 if with_reg else 0, _lib.ptr(d_feats), d, st),
                   "trase_pairhead_backward")
        return (d_feats,) + (None,) * 12


@torch.no_grad()
def resized_columns(rendered_features, size, sampled_pixel):
    """``F.interpolate(rendered_features[None], size, mode="bilinear")[0][:, sampled_pixel].T`` as (S, 32) float32 without the
    resized map: the un-normalised columns the head derives its similarities from, in boolean-index order (one synchronisation,
    for S).  With ``size`` equal to the features' own it is plain indexing, as ``interpolate`` copies then."""
    if rendered_features.device.type != "cuda":
        raise RuntimeError("trase_amd.feature_head runs on the GPU only (there is no CPU path)")
    h, w = int(size[0]), int(size[1])
    if rendered_features.dim() != 3 or rendered_features.shape[0] != 32:
        raise ValueError("rendered_features must be (32, Hr, Wr)")
    if tuple(sampled_pixel.shape) != (h, w):
        raise ValueError(f"sampled_pixel must be [{h}, {w}]")
    dev = rendered_features.device
    sp = (sampled_pixel != 0).to(dev)
    F, Hr, Wr = rendered_features.shape
    if (Hr, Wr) == (h, w):
        return rendered_features[:, sp].T.float().contiguous()
    pix = torch.nonzero(sp.reshape(-1)).reshape(-1).to(torch.int32)
    out = torch.empty((pix.numel(), F), device=dev)
    if pix.numel() == 0:
        return out
    f = rendered_features.float().contiguous()
    lib = _lib.load()
    _lib.check(lib.trase_pairhead_columns_resized(_lib.ptr(f), F, Hr, Wr, h, w, _lib.ptr(pix), pix.numel(), _lib.ptr(out),
                                                  _dev_index(dev), _stream(dev)), "trase_pairhead_columns_resized")
    return out


def contrastive_head(rendered_features, sam_masks, sampled_pixel, sampled_mask, mode="soft", positive_th=0.75, negative_th=0.5,
                     use_weights=True, mask_size=None, with_norm_reg=False):
    """(loss_pos, loss_neg, pos_similarity, neg_similarity[, norm_reg]) of train.py:272-296:
    ``positive_pixel_pair_loss[mode](C, C_F, positive_th, weights)``, ``negative_pixel_pair_loss[mode](...)``,
    ``C_F[C == 1].mean()``, ``C_F[C == 0].mean()`` for the matrices the reference derives from ``sam_masks``,
    ``sampled_pixel``, ``sampled_mask`` and the (32, H, W) features.  No synchronisation when ``sampled_pixel`` comes from
    ``get_sample_pixel_and_mask`` (it carries the draw's target count: the indices are compacted and counted on the device); one --
    the number of sampled pixels -- for any other boolean mask (the reference synchronises at every boolean index).
    ``rendered_features`` is (32, Hr, Wr); where (Hr, Wr) is not the masks' (H, W) the sampled columns are those of train.py:284's
    bilinear ``interpolate`` to (H, W), taken as four taps each.  ``with_norm_reg=True`` also returns the regulariser
    ``(1 - rendered_features.norm(dim=0).mean()) ** 2`` (train.py:280-282) of the image as rendered, and shares one dense
    gradient pass with the pair losses.  ``sam_masks`` is the (N, H, W) tensor or a PackedMasks (bitwise the same results)."""
    if mode not in _MODES:
        raise ValueError(f"contrastive mode {mode!r} (expected one of {sorted(_MODES)})")
    m = sam_masks._gpu() if isinstance(sam_masks, PackedMasks) else _masks_u8(sam_masks)
    N, H, W = m.shape
    if rendered_features.dim() != 3 or rendered_features.shape[0] != 32 or min(rendered_features.shape[1:]) < 1:
        raise ValueError("rendered_features must be (32, Hr, Wr)")
    resized = tuple(rendered_features.shape[1:]) != (H, W)
    if rendered_features.device != m.device:
        raise ValueError("rendered_features and sam_masks live on different devices")
    if tuple(sampled_pixel.shape) != (H, W) or sampled_mask.numel() != N:
        raise ValueError("sampled_pixel must be [H, W] and sampled_mask [N]")
    dev = m.device
    if mask_size is None:
        _, mask_size = mask_stats(sam_masks)
    sm = (sampled_mask != 0).to(dev).contiguous().view(torch.uint8)
    n_sampled = N if N <= 256 else int(sm.sum())
    if n_sampled > 256:
        raise ValueError(f"{n_sampled} sampled masks (the membership bit sets hold 256)")
    expected = getattr(sampled_pixel, "_trase_expected_count", None)
    if expected is not None:
        # only while the tensor still IS the draw the count describes (same number of pixels, not edited in place since)
        expected = expected[0] if (isinstance(expected, tuple) and expected[1] == H * W
                                   and expected[2] == sampled_pixel._version) else None
    s_dev = None
    if expected is not None and sampled_pixel.dtype == torch.bool:
        if not torch.cuda.is_current_stream_capturing():
            _poll_count_checks()
        # no read-back (round 5): the indices are compacted on the device into a buffer sized for the draw's target plus eight
        # standard deviations of the binomial count; every kernel of the head takes the count from the device.  (A draw that
        # overflowed the buffer -- probability ~ 1e-15 -- would drop its highest pixels; count[1] keeps the true number.)
        cap = int(expected + 8.0 * expected ** 0.5 + 64)
        lib = _lib.load()
        flags = sampled_pixel.contiguous().view(torch.uint8)
        pix = torch.empty(cap, dtype=torch.int32, device=dev)
        s_dev = torch.empty(2, dtype=torch.int32, device=dev)
        nb = C.c_size_t()
        _lib.check(lib.trase_compact_pixels_sizes(H * W, C.byref(nb)), "trase_compact_pixels_sizes")
        cws = _bytes(nb.value, dev)
        _lib.check(lib.trase_compact_pixels(_lib.ptr(flags), H * W, _lib.ptr(pix), cap, _lib.ptr(s_dev), _lib.ptr(cws), cws.numel(),
                                            _dev_index(dev), _stream(dev)), "trase_compact_pixels")
        if len(_COUNT_CHECKS) < 64 and not torch.cuda.is_current_stream_capturing():   # the true count is looked at later, off the critical path
            pin, ev = _COUNT_FREE.pop() if _COUNT_FREE else (torch.empty(2, dtype=torch.int32, pin_memory=True), torch.cuda.Event())
            pin.copy_(s_dev, non_blocking=True)
            ev.record(torch.cuda.current_stream(dev))
            _COUNT_CHECKS.append((ev, pin, cap))
    else:
        pix = torch.nonzero(sampled_pixel.reshape(-1)).reshape(-1).to(torch.int32)       # ascending = boolean-index order (synchronises)
        if pix.numel() == 0:
            z = rendered_features.sum() * 0.0
            nan = torch.full((), float("nan"), device=dev)
            return (z, z, nan, nan, feature_norm_reg(rendered_features)) if with_norm_reg else (z, z, nan, nan)
    res = _PairHead.apply(rendered_features, m, sm, n_sampled, mask_size.contiguous(), pix, _MODES[mode], positive_th, negative_th,
                          1 if use_weights else 0, bool(with_norm_reg), s_dev, resized)
    lp, ln, sims = res[:3]
    return (lp, ln, sims[0], sims[1], res[3]) if with_norm_reg else (lp, ln, sims[0], sims[1])


class _FeatNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats):
        f = feats.detach().float().contiguous()
        out2 = _featnorm_forward(_lib.load(), f)
        ctx.save_for_backward(f, out2)
        return out2[0]

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        f, out2 = ctx.saved_tensors
        dev = f.device
        F = f.shape[0]
        d = torch.empty_like(f)
        gg = g.reshape(1).float().contiguous()
        _lib.check(lib.trase_featnorm_backward(_lib.ptr(f), F, f.numel() // F, _lib.ptr(out2), _lib.ptr(gg), _lib.ptr(d), _dev_index(dev),
                                               _stream(dev)), "trase_featnorm_backward")
        return d


def feature_norm_reg(rendered_features: torch.Tensor) -> torch.Tensor:
    """``(1 - rendered_features.norm(dim=0, p=2).mean()) ** 2`` (train.py:281-282): one reduction pass forward, one
    dense pass backward."""
    if rendered_features.device.type != "cuda":
        raise RuntimeError("trase_amd.feature_head runs on the GPU only (there is no CPU path)")
    if rendered_features.dim() != 3:
        raise ValueError("rendered_features must be (C, H, W)")
    return _FeatNorm.apply(rendered_features)
