"""Writes tests/golden/lpips.npz: the reference's own LPIPS ``forward`` (lpipsPyTorch/modules/lpips.py) on seeded weights.

    python tests/golden/make_lpips.py <root of the reference checkout>

The reference's constructors fetch weights (torchvision's VGG16, torch.hub for the linear layers); none of them runs here.  The
first statements below make fetching impossible, and the module is put together by hand: a ``BaseNet`` whose ``layers`` is an
``nn.Sequential`` of torchvision's VGG16 topology filled from ``lpips_random_weights(seed)``, a ``LinLayers`` filled from the
seeded vectors, and an ``LPIPS`` object made without its ``__init__``.  ``forward`` is then the reference's.

The fixture holds two image pairs with values k / 255, the seed, the reference's result in fp32 and float64 (total and per
layer), and per weight tensor its float64 sum and sum of squares.  It holds no weights."""
import sys
import types

import torch


def _no_download(*a, **k):
    raise RuntimeError("make_lpips.py: nothing may be downloaded")


torch.hub.load_state_dict_from_url = _no_download
_tv = types.ModuleType("torchvision")
_tv.models = types.ModuleType("torchvision.models")
sys.modules["torchvision"], sys.modules["torchvision.models"] = _tv, _tv.models

import importlib.util  # noqa: E402
import os  # noqa: E402

import numpy as np  # noqa: E402
import torch.nn as nn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import lpips_reference as L  # noqa: E402
from trase_amd.lpips import lpips_random_weights  # noqa: E402

SEED = 20
SIZES = ((35, 67), (16, 16))
VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


def load_reference(root):
    """the reference's lpipsPyTorch package by path (this repository has a package of the same name)"""
    pkg = os.path.join(root, "lpipsPyTorch")
    spec = importlib.util.spec_from_file_location("lpipsPyTorch", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["lpipsPyTorch"] = mod
    spec.loader.exec_module(mod)
    from lpipsPyTorch.modules import lpips as ref_lpips, networks as ref_networks
    return ref_lpips, ref_networks


def build(ref_lpips, ref_networks, pairs, lins):
    class SeededVGG16(ref_networks.BaseNet):
        def __init__(self):
            super().__init__()
            mods, cin, it = [], 3, iter(pairs)
            for v in VGG16_CFG:
                if v == "M":
                    mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
                    continue
                conv = nn.Conv2d(cin, v, kernel_size=3, padding=1)
                w, b = next(it)
                with torch.no_grad():
                    conv.weight.copy_(w)
                    conv.bias.copy_(b)
                mods += [conv, nn.ReLU(inplace=True)]
                cin = v
            self.layers = nn.Sequential(*mods)
            self.target_layers = [4, 9, 16, 23, 30]
            self.n_channels_list = [64, 128, 256, 512, 512]
            self.set_requires_grad(False)

    net = SeededVGG16()
    lin = ref_networks.LinLayers(net.n_channels_list)
    with torch.no_grad():
        for seq, v in zip(lin, lins):
            seq[1].weight.copy_(v.view(1, -1, 1, 1))
    model = ref_lpips.LPIPS.__new__(ref_lpips.LPIPS)
    nn.Module.__init__(model)
    model.net, model.lin = net, lin
    return model.eval()


def per_layer(model, x, y):
    """the statements of LPIPS.forward up to the per-layer means"""
    feat_x, feat_y = model.net(x), model.net(y)
    diff = [(fx - fy) ** 2 for fx, fy in zip(feat_x, feat_y)]
    return torch.cat([l(d).mean((2, 3), True) for d, l in zip(diff, model.lin)], 0).reshape(-1)


def main(root):
    ref_lpips, ref_networks = load_reference(root)
    pairs, lins = lpips_random_weights(SEED)
    out = {"seed": np.int64(SEED), "checksums": L.checksums(pairs, lins).numpy()}
    for i, (H, W) in enumerate(SIZES):
        g = torch.Generator().manual_seed(1000 + i)
        x = torch.randint(0, 256, (3, H, W), generator=g).float() / 255.0
        y = torch.randint(0, 256, (3, H, W), generator=g).float() / 255.0
        out[f"x{i}"], out[f"y{i}"] = x.numpy(), y.numpy()
        with torch.no_grad():
            for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
                model = build(ref_lpips, ref_networks, pairs, lins).to(dt)
                total = model(x[None].to(dt), y[None].to(dt))
                assert tuple(total.shape) == (1, 1, 1, 1)
                out[f"total_{name}_{i}"] = total.reshape(()).numpy()
                out[f"layers_{name}_{i}"] = per_layer(model, x[None].to(dt), y[None].to(dt)).numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lpips.npz")
    np.savez(path, **out)
    print("wrote", path, {k: (v.shape, v.dtype) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
