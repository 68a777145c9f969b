"""``lpips(x, y, net_type, version)`` and ``LPIPS(net_type, version)`` of the reference's lpipsPyTorch on the HIP kernels of
trase_amd.lpips.

Only ``net_type='vgg'``, ``version='0.1'`` is provided -- what metrics_segmentation.py calls; ``'alex'`` (the signature's default)
and ``'squeeze'`` raise ``NotImplementedError``.  Nothing is ever downloaded and torchvision is not needed: the VGG16 weights
come from the ``torch.load``-able state dict TRASE_VGG16_WEIGHTS names (all of ``vgg16().features``), the linear weights from the
one TRASE_LPIPS_VGG_WEIGHTS names (the published ``vgg.pth``), or both from the ``weights=`` / ``lin_weights=`` keywords.

The packed network is cached per (files, device): the function form does not rebuild it per call as the reference does.
Forward only, batch 1, CUDA tensors only."""
import os

import torch

from trase_amd.lpips import LPIPSVGG

__all__ = ["lpips", "LPIPS"]

VGG_ENV = "TRASE_VGG16_WEIGHTS"
LIN_ENV = "TRASE_LPIPS_VGG_WEIGHTS"
_SUPPORTED = "supported: net_type='vgg', version='0.1'"
_CACHE: dict = {}


def _check(net_type, version):
    if version not in ("0.1",):
        raise NotImplementedError(f"lpipsPyTorch shim: version {version!r} is not provided ({_SUPPORTED})")
    if net_type in ("alex", "squeeze"):
        raise NotImplementedError(f"lpipsPyTorch shim: net_type {net_type!r} is not provided ({_SUPPORTED})")
    if net_type != "vgg":
        raise NotImplementedError(f"choose net_type from [alex, squeeze, vgg]; {_SUPPORTED}")


def _sources(weights, lin_weights):
    """(vgg source, lin source): a keyword's object or an environment variable's path; RuntimeError when one is missing"""
    vgg = weights if weights is not None else os.environ.get(VGG_ENV)
    lin = lin_weights if lin_weights is not None else os.environ.get(LIN_ENV)
    if not vgg or not lin:
        raise RuntimeError(f"lpipsPyTorch shim: no weights; set {VGG_ENV} (a torch.load-able state dict of vgg16().features) and "
                           f"{LIN_ENV} (the published linear weights, vgg.pth), or pass weights= and lin_weights= (this package never "
                           "downloads any)")
    return vgg, lin


def _network(vgg, lin, device):
    """the packed network of (sources, device); file sources are cached by (path, modification time)"""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = None
    if isinstance(vgg, (str, os.PathLike)) and isinstance(lin, (str, os.PathLike)):
        vgg, lin = os.fspath(vgg), os.fspath(lin)
        key = (vgg, os.path.getmtime(vgg), lin, os.path.getmtime(lin), str(device))
        if key in _CACHE:
            return _CACHE[key]
    if isinstance(vgg, (str, os.PathLike)):
        vgg = torch.load(vgg, map_location="cpu")
    if isinstance(lin, (str, os.PathLike)):
        lin = torch.load(lin, map_location="cpu")
    net = LPIPSVGG(vgg, lin, device=device)
    if key is not None:
        _CACHE[key] = net
    return net


class LPIPS(torch.nn.Module):
    r"""Learned Perceptual Image Patch Similarity, the reference's criterion: ``LPIPS('vgg')(x, y) -> (1, 1, 1, 1)``."""

    def __init__(self, net_type: str = 'alex', version: str = '0.1', *, weights=None, lin_weights=None):
        super().__init__()
        _check(net_type, version)
        self._vgg, self._lin = _sources(weights, lin_weights)
        self._net = None

    def forward(self, x: torch.Tensor, y: torch.Tensor):
        if self._net is None or self._net.device != x.device:
            self._net = _network(self._vgg, self._lin, x.device)
        return self._net(x, y)


def lpips(x: torch.Tensor, y: torch.Tensor, net_type: str = 'alex', version: str = '0.1', *, weights=None, lin_weights=None):
    r"""LPIPS of two images ``(3, H, W)`` or ``(1, 3, H, W)``, as the reference's function; the network is built once."""
    _check(net_type, version)
    vgg, lin = _sources(weights, lin_weights)
    return _network(vgg, lin, x.device)(x, y)
