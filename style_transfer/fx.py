"""``VGG16FeatureExtractor`` of the reference's style_transfer/fx.py on the HIP convolutions of trase_amd.vgg.

What the style-transfer script uses is provided: ONE key out of conv1_1 .. conv4_1 (the pre-ReLU output of that convolution,
the network cut there), ``.normalize``, ``forward(x, detach=False) -> {key: (1, C, h, w)}`` which normalises inside,
``.cuda()`` / ``.eval()`` / ``.to()``.

The weights never come from torchvision and nothing is downloaded: pass a state dict (torchvision's names) or a list of
``(w, b)`` pairs as ``weights``, or name a ``torch.load``-able state dict in the environment variable TRASE_VGG16_WEIGHTS.
The weights are constants (no gradient is produced for them)."""
import os
import re

import torch

from trase_amd.vgg import KEYS, MEAN, STD, VGG16Features, key_layers, weight_pairs

__all__ = ["VGGFeatureExtractor", "VGG16FeatureExtractor", "VGG19FeatureExtractor"]

WEIGHTS_ENV = "TRASE_VGG16_WEIGHTS"
_SUPPORTED = "supported: one key out of " + ", ".join(KEYS) + " on VGG16"


class _Normalize(torch.nn.Module):
    """(x - mean) / std per channel of a (..., 3, H, W) tensor: transforms.Normalize as a plain differentiable torch op"""

    def __init__(self, mean, std):
        super().__init__()
        self.register_buffer("mean", torch.tensor(mean, dtype=torch.float32).view(3, 1, 1), persistent=False)
        self.register_buffer("std", torch.tensor(std, dtype=torch.float32).view(3, 1, 1), persistent=False)

    def forward(self, x):
        return (x - self.mean.to(x.device)) / self.std.to(x.device)


def _check_keys(keys):
    if isinstance(keys, str):
        keys = [keys]
    keys = list(keys)
    if len(keys) != 1:
        raise NotImplementedError(f"style_transfer shim: {len(keys)} keys requested; one key per extractor is provided ({_SUPPORTED})")
    key = keys[0]
    m = re.match(r"^(conv|relu)([1-5])(?:_([1-4]))?$", key)
    if not m:
        raise ValueError(f'"{key}" is an invalid identifier')
    op, block, layer = m.groups()
    if op == "relu":
        raise NotImplementedError(f"style_transfer shim: relu keys such as {key!r} are not provided ({_SUPPORTED})")
    if layer is None:
        raise NotImplementedError(f"style_transfer shim: block keys such as {key!r} (every layer of a block) are not provided ({_SUPPORTED})")
    if key not in KEYS:
        raise NotImplementedError(f"style_transfer shim: {key!r} lies behind conv4_1, where the provided network ends ({_SUPPORTED})")
    return key


class VGGFeatureExtractor(torch.nn.Module):
    def __init__(self, keys, weights=None):
        super().__init__()
        key = _check_keys(keys)
        self.keys = [(key, [key])]
        self.key = key
        if weights is None:
            path = os.environ.get(WEIGHTS_ENV)
            if not path:
                raise RuntimeError(f"style_transfer shim: no VGG16 weights; pass weights= (a state dict or (w, b) pairs) or set "
                                   f"{WEIGHTS_ENV} to a torch.load-able state dict (this package never downloads any)")
            weights = torch.load(path, map_location="cpu")
        for l, (w, b) in enumerate(weight_pairs(weights, key_layers(key)), start=1):
            self.register_buffer(f"w{l}", w.detach().float().clone(), persistent=False)
            self.register_buffer(f"b{l}", b.detach().float().clone(), persistent=False)
        self.normalize = _Normalize(MEAN, STD)
        self._net = None

    def _features(self, device):
        if self._net is None or self._net.device != device:
            pairs = [(getattr(self, f"w{l}"), getattr(self, f"b{l}")) for l in range(1, key_layers(self.key) + 1)]
            self._net = VGG16Features(pairs, self.key, normalize=True, mean=MEAN, std=STD, device=device)
        return self._net

    def forward(self, x, detach: bool = False) -> dict:
        if x.dim() == 3:
            x = x.unsqueeze(0)
        assert x.dim() == 4  # NCHW
        out = self._features(x.device)(x.detach() if detach else x)       # normalises inside (fused into conv1_1)
        return {self.key: out.detach() if detach else out}


class VGG16FeatureExtractor(VGGFeatureExtractor):
    pass


class VGG19FeatureExtractor(VGGFeatureExtractor):
    def __init__(self, keys, weights=None):
        raise NotImplementedError(f"style_transfer shim: VGG19 is not provided ({_SUPPORTED})")
