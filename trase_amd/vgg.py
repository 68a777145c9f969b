"""The style-transfer loop's feature extractor (style_transfer/fx.py; train_style_transfer_nnfm.py:141-215) on the GPU:
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

KEYS = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1")
FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17)            # torchvision's vgg16().features positions of the eight convolutions
CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512)    # channels in front of layer 1, behind layers 1 .. 8
POOL_AFTER = (2, 4, 7)                                  # MaxPool2d(2, 2) follows these layers (1-based)
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


def vgg16_random_weights(seed: int, key: str = "conv4_1", device="cpu"):
    """He-scaled seeded weights of the layers up to ``key``: std = sqrt(2 / (9 Cin)), biases 0.05 * randn; [(w, b), ...]"""
    g = torch.Generator().manual_seed(int(seed))
    out = []
    for l in range(1, key_layers(key) + 1):
        cin, cout = CHANNELS[l - 1], CHANNELS[l]
        w = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        b = 0.05 * torch.randn(cout, generator=g)
        out.append((w.to(device), b.to(device)))
    return out


def weight_pairs(weights, layers: int):
    """[(w, b)] * layers out of a torchvision state dict (``features.N.weight`` or bare ``N.weight``) or a list of pairs"""
    if isinstance(weights, dict):
        pairs = []
        for idx in FEATURE_INDEX[:layers]:
            for prefix in (f"features.{idx}.", f"{idx}."):
                if prefix + "weight" in weights:
                    pairs.append((weights[prefix + "weight"], weights[prefix + "bias"]))
                    break
            else:
                raise KeyError(f"VGG16Features: the state dict has neither features.{idx}.weight nor {idx}.weight")
    else:
        pairs = [tuple(p) for p in weights]
        if len(pairs) < layers:
            raise ValueError(f"VGG16Features: {layers} (weight, bias) pairs are needed, got {len(pairs)}")
        pairs = pairs[:layers]
    for l, (w, b) in enumerate(pairs, start=1):
        if tuple(w.shape) != (CHANNELS[l], CHANNELS[l - 1], 3, 3) or tuple(b.shape) != (CHANNELS[l],):
            raise ValueError(f"VGG16Features: layer {KEYS[l - 1]} expects weight {(CHANNELS[l], CHANNELS[l - 1], 3, 3)} and bias "
                             f"{(CHANNELS[l],)}, got {tuple(w.shape)} and {tuple(b.shape)}")
    return pairs


def sizes(layers: int, H: int, W: int):
    """(pack_bytes, ws_forward_bytes, ws_backward_bytes, saved_bytes, C, h, w) of trase_vgg_ws_bytes"""
    lib = _lib.load()
    sz = [C.c_size_t() for _ in range(4)]
    dims = [C.c_int32() for _ in range(3)]
    _lib.check(lib.trase_vgg_ws_bytes(layers, H, W, *[C.byref(v) for v in sz], *[C.byref(v) for v in dims]), "trase_vgg_ws_bytes")
    return tuple(v.value for v in sz) + tuple(v.value for v in dims)


def _device_index(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


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


class VGG16Features:
    """VGG16 ``features`` cut at ``key``: ``net(image)`` -> ``(1, C, h, w)`` fp32, the pre-ReLU output of that convolution.

    ``weights``: a state dict with torchvision's names (``features.{0,2,5,7,10,12,14,17}.{weight,bias}`` or the bare ``features``
    spelling) or a list of ``(w, b)`` pairs; only the layers up to ``key`` are needed.  They are packed at construction --
    call ``repack()`` after changing them.  The weights are constants here (weights that require grad are detached, with one
    warning): the only gradient is the one to the image."""

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
        if self.normalize:
            m = torch.tensor(mean, dtype=torch.float32)
            inv = 1.0 / torch.tensor(std, dtype=torch.float32)            # fp32 reciprocal: what the kernels multiply by
            self._mean = (C.c_float * 3)(*m.tolist())
            self._inv_std = (C.c_float * 3)(*inv.tolist())
        else:
            self._mean = self._inv_std = None
        self.pack = None
        self.device = torch.device(device) if device is not None else None
        if self.device is None and pairs[0][0].device.type == "cuda":
            self.device = pairs[0][0].device
        if self.device is not None:
            self.repack()

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("trase_amd.vgg runs on the GPU only (there is no CPU path)")
        if self.device != device or self.pack is None:
            self.device = device
            self.repack()
        return self

    def repack(self):
        """pack the weights as they are now (after the caller changed them in place)"""
        lib = _lib.load()
        dev = self.device
        if dev is None or dev.type != "cuda":
            raise RuntimeError("trase_amd.vgg runs on the GPU only (there is no CPU path)")
        ws = [w.detach().to(dev, torch.float32).contiguous() for w, _ in self._pairs]
        bs = [b.detach().to(dev, torch.float32).contiguous() for _, b in self._pairs]
        pack_bytes = sizes(self.layers, 8, 8)[0]
        if self.pack is None or self.pack.numel() != pack_bytes or self.pack.device != dev:
            self.pack = _bytes(pack_bytes, dev)
        wp = (C.c_void_p * self.layers)(*[t.data_ptr() for t in ws])
        bp = (C.c_void_p * self.layers)(*[t.data_ptr() for t in bs])
        _lib.check(lib.trase_vgg_pack(self.layers, wp, bp, _lib.ptr(self.pack), self.pack.numel(), _device_index(dev), _stream(dev)),
                   "trase_vgg_pack")
        torch.cuda.current_stream(dev).synchronize()        # ws / bs may be temporaries
        return self

    def out_shape(self, H: int, W: int):
        p = pools_before(self.layers)
        return (1, CHANNELS[self.layers], H >> p, W >> p)

    def __call__(self, image: torch.Tensor) -> torch.Tensor:
        if image.device.type != "cuda":
            raise RuntimeError("trase_amd.vgg runs on the GPU only (there is no CPU path)")
        if not ((image.dim() == 3 and image.shape[0] == 3) or (image.dim() == 4 and tuple(image.shape[:2]) == (1, 3))):
            raise ValueError(f"VGG16Features: expected a (3, H, W) or (1, 3, H, W) image, got {tuple(image.shape)}")
        if self.pack is None or self.device != image.device:
            self.to(image.device)
        # under no_grad, or for an image that needs no gradient, nothing is kept
        return _VGG.apply(image, self, bool(torch.is_grad_enabled() and image.requires_grad))
