"""VGG16 on the GPU, written down once: the thirteen-layer table (``NET_*``), the seeded draw, ``weight_pairs``, the
normalisation constants' arrays and the device / pack bookkeeping (``_Packed``) below serve this module's extractor and the
LPIPS metric of ``trase_amd.lpips``.

The style-transfer loop's feature extractor (style_transfer/fx.py; train_style_transfer_nnfm.py:141-215) on the GPU:
VGG16's 3x3 convolutions up to conv4_1 as HIP kernels (csrc/vgg.hip), forward and gradient to the image.

``VGG16Features(weights, key)`` packs the weights once; ``net(image)`` returns the PRE-ReLU output of convolution ``key`` as
``(1, C, h, w)`` fp32, the network being cut there.  Arithmetic: conv1_1 and its image gradient in fp32, every other product as
bf16x3 (hi + lo bf16 operands, three matrix-core products into an fp32 accumulator).  The weights are constants: the backward
produces the gradient to the image only, from 1 bit per convolution output and 4 bits per pooled unit kept by the forward."""
from __future__ import annotations

import ctypes as C
import math
import warnings

import torch

from . import _lib
from .rasterizer import _bytes, _stream

# the network's thirteen convolutions (csrc/vgg.hip: vg_chan, vg_shift, vg_pooled)
NET_KEYS = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1",
            "conv5_2", "conv5_3")
NET_FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)   # torchvision's vgg16().features positions of the convolutions
NET_CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)   # in front of layer 1, behind layers 1 .. 13
NET_POOL_AFTER = (2, 4, 7, 10)                          # MaxPool2d(2, 2) follows these layers (1-based)
CUT_MAX = 8                                             # the extractor cuts behind conv1_1 .. conv4_1
KEYS = NET_KEYS[:CUT_MAX]
FEATURE_INDEX = NET_FEATURE_INDEX[:CUT_MAX]
CHANNELS = NET_CHANNELS[:CUT_MAX + 1]                   # channels in front of layer 1, behind layers 1 .. 8
POOL_AFTER = tuple(p for p in NET_POOL_AFTER if p < CUT_MAX)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def key_layers(key: str) -> int:
    """number of convolutions of the network cut at ``key``"""
    if key not in KEYS:
        raise NotImplementedError(f"VGG16Features: key {key!r} is not supported; supported keys: {', '.join(KEYS)} "
                                  "(the pre-ReLU output of that convolution)")
    return KEYS.index(key) + 1


def pools_before(layer: int) -> int:
    """pools in front of 1-based ``layer``"""
    return sum(1 for p in POOL_AFTER if p < layer)


def random_pairs(g, layers: int, device):
    """the first ``layers`` layers drawn from generator ``g``, layer by layer (weight, then bias): std = sqrt(2 / (9 Cin)), biases
    0.05 * randn"""
    out = []
    for l in range(1, layers + 1):
        cin, cout = NET_CHANNELS[l - 1], NET_CHANNELS[l]
        w = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        b = 0.05 * torch.randn(cout, generator=g)
        out.append((w.to(device), b.to(device)))
    return out


def vgg16_random_weights(seed: int, key: str = "conv4_1", device="cpu"):
    """He-scaled seeded weights of the layers up to ``key`` (``random_pairs``); [(w, b), ...]"""
    return random_pairs(torch.Generator().manual_seed(int(seed)), key_layers(key), device)


def weight_pairs(weights, layers: int, who: str = "VGG16Features", exact: bool = False):
    """[(w, b)] * layers out of a torchvision state dict (``features.N.weight`` or bare ``N.weight``) or a list of pairs; a longer
    list is cut to ``layers``, or with ``exact`` refused; ``who`` speaks in the messages"""
    if isinstance(weights, dict):
        pairs = []
        for idx in NET_FEATURE_INDEX[:layers]:
            for prefix in (f"features.{idx}.", f"{idx}."):
                if prefix + "weight" in weights:
                    pairs.append((weights[prefix + "weight"], weights[prefix + "bias"]))
                    break
            else:
                raise KeyError(f"{who}: the state dict has neither features.{idx}.weight nor {idx}.weight")
    else:
        pairs = [tuple(p) for p in weights]
        if len(pairs) < layers or (exact and len(pairs) != layers):
            raise ValueError(f"{who}: {layers} (weight, bias) pairs are needed, got {len(pairs)}")
        pairs = pairs[:layers]
    for l, (w, b) in enumerate(pairs, start=1):
        want = (NET_CHANNELS[l], NET_CHANNELS[l - 1], 3, 3), (NET_CHANNELS[l],)
        if (tuple(w.shape), tuple(b.shape)) != want:
            raise ValueError(f"{who}: layer {NET_KEYS[l - 1]} expects weight {want[0]} and bias {want[1]}, got {tuple(w.shape)} and "
                             f"{tuple(b.shape)}")
    return pairs


def norm_arrays(mean, std):
    """(mean, 1 / std) as the ``float[3]`` arguments of the forward entries; the reciprocal in fp32: what the kernels multiply by"""
    m = torch.tensor(mean, dtype=torch.float32)
    inv = 1.0 / torch.tensor(std, dtype=torch.float32)
    return (C.c_float * 3)(*m.tolist()), (C.c_float * 3)(*inv.tolist())


def sizes(layers: int, H: int, W: int):
    """(pack_bytes, ws_forward_bytes, ws_backward_bytes, saved_bytes, C, h, w) of trase_vgg_ws_bytes"""
    lib = _lib.load()
    sz = [C.c_size_t() for _ in range(4)]
    dims = [C.c_int32() for _ in range(3)]
    _lib.check(lib.trase_vgg_ws_bytes(layers, H, W, *[C.byref(v) for v in sz], *[C.byref(v) for v in dims]), "trase_vgg_ws_bytes")
    return tuple(v.value for v in sz) + tuple(v.value for v in dims)


def _device_index(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _indexed(device):
    """``torch.device(device)`` with the current index filled in for a bare "cuda": tensors always carry one"""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def check_image(t, who: str):
    if not ((t.dim() == 3 and t.shape[0] == 3) or (t.dim() == 4 and tuple(t.shape[:2]) == (1, 3))):
        raise ValueError(f"{who}: expected a (3, H, W) or (1, 3, H, W) image, got {tuple(t.shape)}")


class _Packed:
    """Device and pack bookkeeping of a network whose weights are packed once.  A subclass sets ``MODULE`` (for the messages) and
    ``self._pairs``, and gives ``_pack_bytes()``, ``_tensors()`` (the groups of tensors the C pack takes: weights, biases, ...)
    and ``_pack(lib, arrays, device_index, stream)`` (the C call on arrays of their device pointers)."""

    def _gpu_only(self):
        return RuntimeError(f"{self.MODULE} runs on the GPU only (there is no CPU path)")

    def _place(self, device):
        """the end of ``__init__``: the device asked for, else the weights' if they are on one; packs when there is one"""
        self.pack = None
        self.device = _indexed(device) if device is not None else None
        if self.device is None and self._pairs[0][0].device.type == "cuda":
            self.device = self._pairs[0][0].device
        if self.device is not None:
            self.repack()

    def to(self, device):
        device = _indexed(device)
        if device.type != "cuda":
            raise self._gpu_only()
        if self.device != device or self.pack is None:
            self.device = device
            self.repack()
        return self

    def repack(self):
        """pack the weights as they are now (after the caller changed them in place)"""
        lib = _lib.load()
        dev = self.device
        if dev is None or dev.type != "cuda":
            raise self._gpu_only()
        staged = [[t.detach().to(dev, torch.float32).contiguous() for t in group] for group in self._tensors()]
        pack_bytes = self._pack_bytes()
        if self.pack is None or self.pack.numel() != pack_bytes or self.pack.device != dev:
            self.pack = _bytes(pack_bytes, dev)
        arrays = [(C.c_void_p * len(group))(*[t.data_ptr() for t in group]) for group in staged]
        self._pack(lib, arrays, _device_index(dev), _stream(dev))
        torch.cuda.current_stream(dev).synchronize()        # the staged copies may be temporaries
        return self


class _VGG(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, net, keep):
        lib = _lib.load()
        dev = image.device
        x = image.detach().float().contiguous()
        H, W = int(x.shape[-2]), int(x.shape[-1])
        _, ws_fwd, _, saved_bytes, c, h, w = sizes(net.layers, H, W)
        ws = _bytes(ws_fwd, dev)
        saved = _bytes(saved_bytes, dev) if keep and saved_bytes else None
        out = torch.empty(1, c, h, w, device=dev)
        _lib.check(lib.trase_vgg_forward(net.layers, _lib.ptr(net.pack), net.pack.numel(), _lib.ptr(x), H, W, net._mean, net._inv_std,
                                         _lib.ptr(out), _lib.ptr(saved), saved_bytes if saved is not None else 0, _lib.ptr(ws),
                                         ws.numel(), _device_index(dev), _stream(dev)), "trase_vgg_forward")
        if keep:
            ctx.net, ctx.hw, ctx.in_shape = net, (H, W), tuple(image.shape)
            ctx.save_for_backward(*([saved] if saved is not None else []))
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        net, (H, W) = ctx.net, ctx.hw
        saved = ctx.saved_tensors[0] if ctx.saved_tensors else None
        dev = g.device
        _, _, ws_bwd, saved_bytes, _, _, _ = sizes(net.layers, H, W)
        go = g.detach().float().contiguous()
        ws = _bytes(ws_bwd, dev)
        d_img = torch.empty(3, H, W, device=dev)
        _lib.check(lib.trase_vgg_backward(net.layers, _lib.ptr(net.pack), net.pack.numel(), _lib.ptr(go), H, W, net._inv_std,
                                          _lib.ptr(saved), saved_bytes if saved is not None else 0, _lib.ptr(d_img), _lib.ptr(ws),
                                          ws.numel(), _device_index(dev), _stream(dev)), "trase_vgg_backward")
        return d_img.reshape(ctx.in_shape), None, None


_WEIGHTS_WARNED = False


class VGG16Features(_Packed):
    """VGG16 ``features`` cut at ``key``: ``net(image)`` -> ``(1, C, h, w)`` fp32, the pre-ReLU output of that convolution.

    ``weights``: a state dict with torchvision's names (``features.{0,2,5,7,10,12,14,17}.{weight,bias}`` or the bare ``features``
    spelling) or a list of ``(w, b)`` pairs; only the layers up to ``key`` are needed.  They are packed at construction --
    call ``repack()`` after changing them.  The weights are constants here (weights that require grad are detached, with one
    warning): the only gradient is the one to the image."""

    MODULE = "trase_amd.vgg"

    def __init__(self, weights, key: str = "conv4_1", *, normalize: bool = True, mean=MEAN, std=STD, device=None):
        global _WEIGHTS_WARNED
        self.key = key
        self.layers = key_layers(key)
        pairs = weight_pairs(weights, self.layers)
        if any(w.requires_grad or b.requires_grad for w, b in pairs) and not _WEIGHTS_WARNED:
            warnings.warn("VGG16Features: the weights require grad; they are constants here and no gradient is produced for them "
                          "(no optimizer of the reference holds them) -- detaching")
            _WEIGHTS_WARNED = True
        self._pairs = pairs
        self.normalize = bool(normalize)
        self._mean, self._inv_std = norm_arrays(mean, std) if self.normalize else (None, None)
        self._place(device)

    def _pack_bytes(self):
        return sizes(self.layers, 8, 8)[0]

    def _tensors(self):
        return [w for w, _ in self._pairs], [b for _, b in self._pairs]

    def _pack(self, lib, arrays, device_index, stream):
        _lib.check(lib.trase_vgg_pack(self.layers, *arrays, _lib.ptr(self.pack), self.pack.numel(), device_index, stream), "trase_vgg_pack")

    def out_shape(self, H: int, W: int):
        p = pools_before(self.layers)
        return (1, CHANNELS[self.layers], H >> p, W >> p)

    def __call__(self, image: torch.Tensor) -> torch.Tensor:
        if image.device.type != "cuda":
            raise self._gpu_only()
        check_image(image, "VGG16Features")
        if self.pack is None or self.device != image.device:
            self.to(image.device)
        # under no_grad, or for an image that needs no gradient, nothing is kept
        return _VGG.apply(image, self, bool(torch.is_grad_enabled() and image.requires_grad))
