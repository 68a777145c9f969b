"""Plain torch restatement of the photometric loss (trase_amd/losses.py, trase_amd/csrc/loss.hip), parameterised by the
working dtype: test infrastructure, CPU only.

``l1`` is utils/loss_utils.py:30-31, ``ssim`` is utils/loss_utils.py:46-86 in its own formulation -- five depthwise 11x11
``conv2d`` with zero padding 5, C1 = 0.01^2, C2 = 0.03^2, the mean of the map -- and ``photometric`` is the combination
of train.py:235-238.  Gradients come from autograd.

The window is built as the reference builds it: Python floats -> float32 -> divided by its float32 sum.  Only then is it
promoted to the working dtype and multiplied out to 11x11, so a float64 evaluation differs from the kernel (which applies
the same eleven float32 taps separably) in arithmetic alone, never in the window; at float32 the outer product is the
reference's own ``_1D_window.mm(_1D_window.t())``."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

WINDOW, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window_1d() -> torch.Tensor:
    """utils/loss_utils.py:46-48: eleven float32 taps."""
    g = torch.tensor([math.exp(-(x - WINDOW // 2) ** 2 / float(2 * SIGMA ** 2)) for x in range(WINDOW)], dtype=torch.float32)
    return g / g.sum()


def window_2d(channels: int, dtype=torch.float64) -> torch.Tensor:
    g = window_1d().to(dtype).unsqueeze(1)
    return g.mm(g.t()).unsqueeze(0).unsqueeze(0).expand(channels, 1, WINDOW, WINDOW).contiguous()


def l1(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return (x - y).abs().mean()


def ssim_map(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """(C,H,W) x (C,H,W) -> the (C,H,W) SSIM map, in the dtype of x."""
    c = x.shape[0]
    win = window_2d(c, x.dtype)
    conv = lambda t: F.conv2d(t.unsqueeze(0), win, padding=WINDOW // 2, groups=c).squeeze(0)
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(x * x) - mu1_sq, conv(y * y) - mu2_sq, conv(x * y) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def ssim(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return ssim_map(x, y).mean()


def photometric(x: torch.Tensor, y: torch.Tensor, lambda_dssim: float = 0.2) -> torch.Tensor:
    """train.py:235-238."""
    return (1.0 - lambda_dssim) * l1(x, y) + lambda_dssim * (1.0 - ssim(x, y))


def evaluate(img, gt, dtype=torch.float64):
    """One evaluation at ``dtype`` of the (C,H,W) pair (any float tensors or arrays): -> (l1, ssim, d l1 / d img,
    d ssim / d img), the two scalars as Python floats and the two gradients as float64 tensors.  The gradient for any
    pair of cotangents is ``g_l1 * d_l1 + g_ssim * d_ssim`` (both heads are linear in their cotangent)."""
    x = torch.as_tensor(img).detach().cpu().to(dtype).clone().requires_grad_(True)
    y = torch.as_tensor(gt).detach().cpu().to(dtype)
    a, s = l1(x, y), ssim(x, y)
    d_l1, = torch.autograd.grad(a, x)
    d_ss, = torch.autograd.grad(s, x)
    return float(a.detach()), float(s.detach()), d_l1.double(), d_ss.double()
