"""Float64 reference of the deformation MLP (utils/time_utils.py:60-131 ``DeformNetwork``), evaluated the way the HIP
kernels of trase_amd/csrc/mlp.hip round it.

* ``bf16=True``: the encoding, every weight matrix and every post-ReLU activation are rounded to bf16 -- the operands the
  matrix cores see -- while products, sums, biases (fp32 parameters, exact in float64) and the heads stay in float64.
  The rounding is straight-through (``v + (round(v) - v).detach()``), so autograd yields the gradient of exactly that
  computation, as ``_bf16_evaluated_net`` of tests/test_gpu_parity.py does in fp32.
* ``bf16=False``: the plain float64 network (tests/test_mlp_reference.py pins it to the fixtures of the imported reference).

A plain module (no HIP library, no conftest): it runs on whatever device its tensors live on, the CPU for the fixture test
and the GPU for the full-size form tests (tests/test_gpu_mlp_forms.py), in row chunks so that a million rows with autograd
stay within a few GB.  The is_6dof transform is restated from Modern Robotics eq. 3.51 / 3.88 here rather than imported
from trase_amd.deform, so that the fixture test also vouches for it.
"""
from __future__ import annotations

from typing import Dict, Mapping, Optional, Sequence, Tuple

import torch

F64 = torch.float64
HIDDEN = tuple(f"linear.{i}.{s}" for i in range(8) for s in ("weight", "bias"))
TIMENET = ("timenet.0.weight", "timenet.0.bias", "timenet.2.weight", "timenet.2.bias")
CHUNK = 1 << 17


def param_keys(is_blender: bool = False, is_6dof: bool = False) -> Tuple[str, ...]:
    heads = ("branch_w", "branch_v") if is_6dof else ("gaussian_warp",)
    heads += ("gaussian_rotation", "gaussian_scaling")
    return (TIMENET if is_blender else ()) + HIDDEN + tuple(f"{h}.{s}" for h in heads for s in ("weight", "bias"))


def _round(v: torch.Tensor, on: bool) -> torch.Tensor:
    if not on:
        return v
    return v + (v.to(torch.bfloat16).to(v.dtype) - v).detach()


def embed(v: torch.Tensor, nf: int) -> torch.Tensor:
    """get_embedder(nf): v, then per frequency 2^f: sin(v 2^f), cos(v 2^f) (every input column of one function together)."""
    out = [v]
    for f in range(nf):
        a = v * float(2 ** f)
        out += [torch.sin(a), torch.cos(a)]
    return torch.cat(out, -1)


def _skew(w: torch.Tensor) -> torch.Tensor:
    z = torch.zeros_like(w[:, 0])
    return torch.stack([z, -w[:, 2], w[:, 1], w[:, 2], z, -w[:, 0], -w[:, 1], w[:, 0], z], -1).reshape(-1, 3, 3)


def se3_exp(w: torch.Tensor, v: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
    """(N,4,4) homogeneous transform of screw axis (w, v) and magnitude theta (N,1): R = I + sin W + (1 - cos) W^2,
    p = (theta I + (1 - cos) W + (theta - sin) W^2) v."""
    W = _skew(w)
    W2 = W @ W
    th = theta.reshape(-1, 1, 1)
    eye = torch.eye(3, dtype=w.dtype, device=w.device)
    R = eye + torch.sin(th) * W + (1 - torch.cos(th)) * W2
    p = (th * eye + (1 - torch.cos(th)) * W + (th - torch.sin(th)) * W2) @ v.unsqueeze(-1)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=w.dtype, device=w.device).expand(w.shape[0], 1, 4)
    return torch.cat([torch.cat([R, p], -1), bottom], 1)


def to_f64(params: Mapping[str, torch.Tensor], device=None, requires_grad: bool = False) -> Dict[str, torch.Tensor]:
    return {k: v.detach().to(device or v.device, F64).clone().requires_grad_(requires_grad) for k, v in params.items()}


def forward(p: Mapping[str, torch.Tensor], x: torch.Tensor, t: torch.Tensor, is_blender: bool = False, is_6dof: bool = False,
            bf16: bool = True, skip_encoding: bool = True):
    """(d_xyz, d_rotation, d_scaling) in float64 for float64 parameters ``p`` (reference names).  ``t`` is (N,1), any
    stride.  is_blender: the timenet output of the FIRST row's time is the 30 shared time columns (the kernels' contract).
    ``skip_encoding=False`` drops the encoding columns of the skip layer (a mutation for the tests' bars)."""
    n = x.shape[0]
    x = x.to(F64)
    t = t.to(F64).reshape(n, 1)
    if is_blender:
        h = torch.relu(embed(t[0:1], 6) @ p["timenet.0.weight"].T + p["timenet.0.bias"])
        temb = (h @ p["timenet.2.weight"].T + p["timenet.2.bias"]).expand(n, -1)
    else:
        temb = embed(t, 10)
    e = _round(torch.cat([embed(x, 10), temb], -1), bf16)
    h = e
    for i in range(8):
        w = p[f"linear.{i}.weight"]
        if i == 5 and not skip_encoding:
            w = torch.cat([torch.zeros_like(w[:, :e.shape[1]]), w[:, e.shape[1]:]], 1)
        h = _round(torch.relu(h @ _round(w, bf16).T + p[f"linear.{i}.bias"]), bf16)
        if i == 4:
            h = torch.cat([e, h], -1)

    def head(name):
        return h @ _round(p[name + ".weight"], bf16).T + p[name + ".bias"]
    rot, scale = head("gaussian_rotation"), head("gaussian_scaling")
    if is_6dof:
        w, v = head("branch_w"), head("branch_v")
        theta = torch.linalg.vector_norm(w, dim=-1, keepdim=True)
        return se3_exp(w / theta + 1e-5, v / theta + 1e-5, theta), rot, scale
    return head("gaussian_warp"), rot, scale


def evaluate(params: Mapping[str, torch.Tensor], x: torch.Tensor, t: torch.Tensor, cot: Optional[Sequence[torch.Tensor]] = None,
             is_blender: bool = False, is_6dof: bool = False, bf16: bool = True, skip_encoding: bool = True,
             chunk: int = CHUNK):
    """Outputs (float64) of ``forward`` over all rows, evaluated in row chunks on x's device; with cotangents ``cot`` also the
    float64 gradient of sum(out * cot) for every parameter (the row sums of the chunks added).  Returns (outs, grads|None)."""
    p = to_f64(params, x.device, requires_grad=cot is not None)
    n = x.shape[0]
    t = t.reshape(n, 1)
    outs = []
    for s in range(0, n, chunk):
        sl = slice(s, min(n, s + chunk))
        with torch.set_grad_enabled(cot is not None):
            o = forward(p, x[sl], t[sl], is_blender, is_6dof, bf16, skip_encoding)
            if cot is not None:
                torch.autograd.backward(o, [c[sl].to(F64) for c in cot])
        outs.append([v.detach() for v in o])
    out = tuple(torch.cat([o[j] for o in outs], 0) for j in range(3))
    grads = {k: v.grad if v.grad is not None else torch.zeros_like(v) for k, v in p.items()} if cot is not None else None
    return out, grads
