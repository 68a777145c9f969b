"""LPIPS with the VGG16 backbone (lpipsPyTorch ``lpips(x, y, net_type='vgg')``; metrics_segmentation.py:118-165) on the GPU,
forward only: the thirteen convolutions up to relu5_3 with the kernels of ``trase_amd.vgg`` and a distance head in float64
(csrc/vgg.hip: trase_lpips_ws_bytes / _pack / _forward / _head).

``LPIPSVGG(vgg_weights, lin_weights)`` packs once; ``net(x, y)`` returns ``(1, 1, 1, 1)`` fp32 as the reference does: per tap
relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 the spatial mean of ``sum_c lin_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2``,
summed over the five taps in float64 and rounded once.  The images go in as the caller has them (``[0, 1]`` in the reference's
metric script); ``z = (x - mean) * (1 / std)`` with the LPIPS constants is fused into conv1_1.  Everything is bitwise
reproducible, ``net(x, y)`` and ``net(y, x)`` are the same bits and ``net(x, x)`` is exactly 0.

There is no backward: the reference uses LPIPS as a metric under ``no_grad`` only."""
from __future__ import annotations

import ctypes as C
import functools

import torch

from . import _lib, vgg
from .rasterizer import _bytes, _stream
from .vgg import _device_index

KEYS, FEATURE_INDEX, CHANNELS, POOL_AFTER = vgg.NET_KEYS, vgg.NET_FEATURE_INDEX, vgg.NET_CHANNELS, vgg.NET_POOL_AFTER    # all thirteen layers
TAP_LAYERS = (2, 4, 7, 10, 13)                                     # relu1_2 relu2_2 relu3_3 relu4_3 relu5_3 (modules 4 9 16 23 30)
TAP_NAMES = ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3")
TAP_CHANNELS = tuple(CHANNELS[l] for l in TAP_LAYERS)
MEAN = (-.030, -.088, -.188)                                       # networks.py:41-44
STD = (.458, .448, .450)
LAYERS = len(KEYS)


def lpips_random_weights(seed: int, device="cpu"):
    """(pairs, lins): the 13 layers He-scaled as in ``vgg16_random_weights`` (std = sqrt(2 / (9 Cin)), biases 0.05 * randn) and
    five non-negative ``lin`` vectors of 64, 128, 256, 512, 512 elements; drawn on the CPU generator, so it needs no GPU"""
    g = torch.Generator().manual_seed(int(seed))
    pairs = vgg.random_pairs(g, LAYERS, device)
    lins = [(torch.rand(c, generator=g) * (2.0 / c)).to(device) for c in TAP_CHANNELS]
    return pairs, lins


# [(w, b)] * 13 out of a torchvision state dict (``features.N.weight`` or bare ``N.weight``) or a list of exactly 13 pairs
weight_pairs = functools.partial(vgg.weight_pairs, layers=LAYERS, who="LPIPSVGG", exact=True)


def lin_vectors(lin_weights):
    """five flat ``lin`` vectors out of the published file's dict (``lin{k}.model.1.weight``), the reference's renamed one
    (``{k}.1.weight``), or five tensors of C elements in any shape"""
    if isinstance(lin_weights, dict):
        lins = []
        for k in range(5):
            for key in (f"lin{k}.model.1.weight", f"{k}.1.weight"):
                if key in lin_weights:
                    lins.append(lin_weights[key])
                    break
            else:
                raise KeyError(f"LPIPSVGG: the linear weights have neither lin{k}.model.1.weight nor {k}.1.weight")
    else:
        lins = list(lin_weights)
        if len(lins) != 5:
            raise ValueError(f"LPIPSVGG: five lin vectors are needed, got {len(lins)}")
    for k, (v, c) in enumerate(zip(lins, TAP_CHANNELS)):
        if v.numel() != c:
            raise ValueError(f"LPIPSVGG: lin{k} expects {c} elements, got {tuple(v.shape)}")
    return [v.reshape(-1) for v in lins]


def sizes(H: int, W: int):
    """(pack_bytes, ws_bytes, map_floats) of trase_lpips_ws_bytes"""
    lib = _lib.load()
    sz = [C.c_size_t() for _ in range(3)]
    _lib.check(lib.trase_lpips_ws_bytes(H, W, *[C.byref(v) for v in sz]), "trase_lpips_ws_bytes")
    return tuple(v.value for v in sz)


def tap_shapes(H: int, W: int):
    """[(C_l, h_l, w_l)] of the five taps"""
    return [(c, H >> l, W >> l) for l, c in enumerate(TAP_CHANNELS)]


def head_ws_bytes(C_: int, hw: int) -> int:
    """workspace of trase_lpips_head: the two inputs' hi and lo planes and the map, each rounded up to 256 bytes, and 256
    float64 partial sums of the mean"""
    r = lambda n: (n + 255) // 256 * 256
    return 4 * r(2 * C_ * hw) + r(4 * hw) + 2048


def total_of(layers):
    """the float64 sum of the five layer values in layer order (a device scalar; a library reduction fixes no order)"""
    return (((layers[0] + layers[1]) + layers[2]) + layers[3]) + layers[4]


class LPIPSVGG(vgg._Packed):
    """LPIPS (VGG16, version 0.1), forward only.  ``vgg_weights``: torchvision's state dict (``features.N.weight`` or bare
    ``N.weight``, N in 0 2 5 7 10 12 14 17 19 21 24 26 28) or 13 ``(w, b)`` pairs; ``lin_weights``: see ``lin_vectors``.  Packed at
    construction when a device is known -- call ``repack()`` after changing the weights.

    ``net(x, y)`` -> ``(1, 1, 1, 1)`` fp32.  With ``return_layers`` / ``return_maps`` / ``return_taps`` a tuple: the value, then
    the ``(5,)`` float64 layer values, the five ``(h_l, w_l)`` fp32 maps, ``(taps_x, taps_y)`` as five ``(C_l, h_l, w_l)`` fp32
    tensors each, in that order, those asked for.  Nothing synchronises."""

    MODULE = "trase_amd.lpips"

    def __init__(self, vgg_weights, lin_weights, *, device=None):
        self._pairs = weight_pairs(vgg_weights)
        self._lins = lin_vectors(lin_weights)
        self._mean, self._inv_std = vgg.norm_arrays(MEAN, STD)
        self.packs = 0                                                  # how often the weights were packed
        self._place(device)

    def _pack_bytes(self):
        return sizes(16, 16)[0]

    def _tensors(self):
        return [w for w, _ in self._pairs], [b for _, b in self._pairs], self._lins

    def _pack(self, lib, arrays, device_index, stream):
        _lib.check(lib.trase_lpips_pack(*arrays, _lib.ptr(self.pack), self.pack.numel(), device_index, stream), "trase_lpips_pack")
        self.packs += 1

    def layers_device(self, x, y, *, maps=None, taps=None):
        """the launch sequence: -> (5,) float64 device tensor of the layer values; ``maps`` / ``taps`` = (taps_x, taps_y): flat fp32
        buffers to fill (``sizes`` / ``tap_shapes``)"""
        lib = _lib.load()
        dev = x.device
        H, W = int(x.shape[-2]), int(x.shape[-1])
        _, ws_bytes, _ = sizes(H, W)
        ws = _bytes(ws_bytes, dev)
        out = torch.empty(5, dtype=torch.float64, device=dev)
        tx, ty = taps if taps is not None else (None, None)
        _lib.check(lib.trase_lpips_forward(_lib.ptr(self.pack), self.pack.numel(), _lib.ptr(x), _lib.ptr(y), H, W, self._mean,
                                           self._inv_std, _lib.ptr(out), _lib.ptr(maps), _lib.ptr(tx), _lib.ptr(ty), _lib.ptr(ws),
                                           ws.numel(), _device_index(dev), _stream(dev)), "trase_lpips_forward")
        return out

    def __call__(self, x, y, *, return_layers=False, return_maps=False, return_taps=False):
        for t in (x, y):
            if not torch.is_tensor(t) or t.device.type != "cuda":
                raise self._gpu_only()
            if t.dim() == 4 and t.shape[0] > 1:
                raise ValueError(f"LPIPSVGG: batches above 1 are not supported, got {tuple(t.shape)}")
            vgg.check_image(t, "LPIPSVGG")
            if t.dtype != torch.float32:
                raise ValueError(f"LPIPSVGG: the images must be fp32, got {t.dtype}")
            if t.requires_grad:
                raise NotImplementedError("LPIPSVGG: the metric is forward only (there is no backward); detach the input or call "
                                          "under torch.no_grad()")
        if tuple(x.shape[-2:]) != tuple(y.shape[-2:]) or x.device != y.device:
            raise ValueError(f"LPIPSVGG: the images differ in shape or device: {tuple(x.shape)} and {tuple(y.shape)}")
        if self.pack is None or self.device != x.device:
            self.to(x.device)
        with torch.no_grad():
            dev = x.device
            xs, ys = x.detach().reshape(3, *x.shape[-2:]).contiguous(), y.detach().reshape(3, *y.shape[-2:]).contiguous()
            H, W = int(xs.shape[1]), int(xs.shape[2])
            shapes = tap_shapes(H, W)
            maps = torch.empty(sum(h * w for _, h, w in shapes), device=dev) if return_maps else None
            taps = None
            if return_taps:
                n = sum(c * h * w for c, h, w in shapes)
                taps = (torch.empty(n, device=dev), torch.empty(n, device=dev))
            layers = self.layers_device(xs, ys, maps=maps, taps=taps)
            value = total_of(layers).to(torch.float32).reshape(1, 1, 1, 1)
            out = [value]
            if return_layers:
                out.append(layers)
            if return_maps:
                ms, o = [], 0
                for _, h, w in shapes:
                    ms.append(maps[o:o + h * w].view(h, w))
                    o += h * w
                out.append(ms)
            if return_taps:
                both = []
                for t in taps:
                    ts, o = [], 0
                    for c, h, w in shapes:
                        ts.append(t[o:o + c * h * w].view(c, h, w))
                        o += c * h * w
                    both.append(ts)
                out.append(tuple(both))
        return out[0] if len(out) == 1 else tuple(out)


def lpips_head(a, b, lin, *, return_map=False):
    """The distance head alone: ``a``, ``b`` fp32 CUDA tensors ``(C, ...)`` of equal shape (C in 64, 128, 256, 512), ``lin`` C
    weights -> the layer value, a 0-d float64 device tensor (with ``return_map`` also the ``(...)`` fp32 map).  The inputs are
    split into hi + lo bf16 planes first, so the head sees ``hi + lo`` of them."""
    lib = _lib.load()
    for t in (a, b, lin):
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise RuntimeError("trase_amd.lpips runs on the GPU only (there is no CPU path)")
    if a.shape != b.shape or a.dim() < 2 or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(f"lpips_head: expected two fp32 (C, ...) tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    c = int(a.shape[0])
    if lin.numel() != c:
        raise ValueError(f"lpips_head: lin must have {c} elements, got {tuple(lin.shape)}")
    dev = a.device
    with torch.no_grad():
        a2, b2 = a.detach().reshape(c, -1).contiguous(), b.detach().reshape(c, -1).contiguous()
        l2 = lin.detach().to(torch.float32).reshape(-1).contiguous()
        hw = int(a2.shape[1])
        ws = _bytes(head_ws_bytes(c, hw), dev)
        out = torch.empty(1, dtype=torch.float64, device=dev)
        m = torch.empty(a.shape[1:], device=dev) if return_map else None
        _lib.check(lib.trase_lpips_head(_lib.ptr(a2), _lib.ptr(b2), _lib.ptr(l2), c, hw, _lib.ptr(out), _lib.ptr(m), _lib.ptr(ws),
                                        ws.numel(), _device_index(dev), _stream(dev)), "trase_lpips_head")
    return (out[0], m) if return_map else out[0]
