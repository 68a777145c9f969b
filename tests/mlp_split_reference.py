"""Emulation of the split-bf16 deformation MLP (trase_amd/csrc/mlp_split.hip, ``precision="bf16x3"``) on top of
tests/mlp_reference.py.

Every matrix operand -- the encoding, every weight matrix, every post-ReLU activation, the head inputs -- is rounded to fp32
and carried as ``hi + lo`` with ``hi = bf16(v)``, ``lo = bf16(v - hi)`` (both round-to-nearest-even).  A product is
``hi.hi + hi.lo + lo.hi`` (``lo.lo`` is dropped); the three partial products of a layer go into ONE accumulation, in fp32
(``accumulate="fp32"``, what the matrix cores do) or in float64 (``accumulate="fp64"``: the arithmetic's own error without
the accumulation's).  Biases are added in fp32.  Everything outside the matrix products (the encoding's sines, the timenet of
is_blender, the is_6dof transform) is evaluated in float64 as in ``mlp_reference.forward``.

A plain module (no HIP library, no conftest): float64 tensors in, float64 tensors out, on whatever device they live on.
"""
from __future__ import annotations

from typing import Mapping, Tuple

import torch

from tests import mlp_reference as R

F32 = torch.float32


def split(v: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(hi, lo): two fp32 tensors holding bf16 values with hi + lo = fp32(v) up to 2^-16 relative."""
    v = v.to(F32)
    hi = v.to(torch.bfloat16).to(F32)
    lo = (v - hi).to(torch.bfloat16).to(F32)
    return hi, lo


def linear(a: torch.Tensor, w: torch.Tensor, b: torch.Tensor, accumulate: str = "fp32") -> torch.Tensor:
    """a @ w.T + b with split operands: one accumulation over the 3 K partial products; fp32 result."""
    ah, al = split(a)
    wh, wl = split(w)
    lhs, rhs = torch.cat([al, ah, ah], -1), torch.cat([wh, wl, wh], -1)         # lo.hi + hi.lo + hi.hi
    if accumulate == "fp64":
        return ((lhs.double() @ rhs.double().T).to(F32) + b.to(F32))
    if accumulate != "fp32":
        raise ValueError("accumulate must be 'fp32' or 'fp64'")
    return lhs @ rhs.T + b.to(F32)


def forward(p: Mapping[str, torch.Tensor], x: torch.Tensor, t: torch.Tensor, is_blender: bool = False, is_6dof: bool = False,
            accumulate: str = "fp32"):
    """(d_xyz, d_rotation, d_scaling) in float64 for float64 parameters ``p`` (reference names); same contract as
    ``mlp_reference.forward``."""
    n = x.shape[0]
    x = x.to(R.F64)
    t = t.to(R.F64).reshape(n, 1)
    if is_blender:
        h = torch.relu(R.embed(t[0:1], 6) @ p["timenet.0.weight"].T + p["timenet.0.bias"])
        temb = (h @ p["timenet.2.weight"].T + p["timenet.2.bias"]).expand(n, -1)
    else:
        temb = R.embed(t, 10)
    e = torch.cat([R.embed(x, 10), temb], -1).to(F32)
    h = e
    for i in range(8):
        h = torch.relu(linear(h, p[f"linear.{i}.weight"], p[f"linear.{i}.bias"], accumulate))
        if i == 4:
            h = torch.cat([e, h], -1)

    def head(name):
        return linear(h, p[name + ".weight"], p[name + ".bias"], accumulate).to(R.F64)
    rot, scale = head("gaussian_rotation"), head("gaussian_scaling")
    if is_6dof:
        w, v = head("branch_w"), head("branch_v")
        theta = torch.linalg.vector_norm(w, dim=-1, keepdim=True)
        return R.se3_exp(w / theta + 1e-5, v / theta + 1e-5, theta), rot, scale
    return head("gaussian_warp"), rot, scale

