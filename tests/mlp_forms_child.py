"""Runs the fused deformation MLP over the cases of tests/test_gpu_mlp_forms.py and writes what the kernels produced to an .npz.

    python -m tests.mlp_forms_child OUT.npz infer|train|both

"infer" runs the inference entry point (register-chained kernel), "train" the training pair (block forward + backward) under
every row order of the case.  The test calls ``run`` in its own process; the command line writes the same .npz from a
library of the caller's choosing (TRASE_RAST_LIB), so the results of two builds can be compared bit for bit.  Inputs and
parameters are rebuilt from fixed seeds on the CPU (``case_inputs``, ``make_params``), so every process sees bit-identical
data.  Every case runs twice; the second run's bit-equality is recorded.  Not a test module (no ``test_`` prefix)."""
from __future__ import annotations

import sys
import zlib
from typing import Dict, NamedTuple, Tuple

import numpy as np
import torch

SCENE = 40.0          # |x| of the scene-sized slab (Gaussian centres are not rescaled before DeformNetwork)


class Case(NamedTuple):
    name: str
    variant: str          # "default" | "blender" | "6dof"
    n: int
    tkind: str            # "expand" (stride-0, as train.py builds it) | "rows" (contiguous, distinct per row)
    orders: Tuple[str, ...]   # training row orders; () = inference only


def cases():
    out = []
    tails = [256 * 3 + r for r in (1, 31, 33, 64, 65, 200)]      # every wave position of the last RC workgroup
    for n in [255, 256, 257, 511, 4096, 20_011, 300_000] + tails:
        for tk in ("expand", "rows"):
            orders = ("morton", "none") if n in (20_011, 300_000) else ("morton",)
            out.append(Case(f"default-{n}-{tk}", "default", n, tk, orders))
    out.append(Case("default-1000000-expand", "default", 1_000_000, "expand", ("morton",)))
    for n in (20_011, 300_000):
        out.append(Case(f"blender-{n}-expand", "blender", n, "expand", ("morton",)))
        for tk in ("expand", "rows"):
            out.append(Case(f"6dof-{n}-{tk}", "6dof", n, tk, ("morton",)))
    return out


def make_params(variant: str) -> Dict[str, torch.Tensor]:
    """fp32 CPU parameters of a randomly initialised reference-shaped network (fixed seed per variant)."""
    from trase_amd.synthetic import SynthDeformNetwork
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed({"default": 11, "blender": 12, "6dof": 13}[variant])
        net = SynthDeformNetwork(is_blender=variant == "blender", is_6dof=variant == "6dof")
    return {k: v.detach().clone() for k, v in net.named_parameters()}


def scene_rows(n: int) -> slice:
    """Rows at scene-sized coordinates: a slab in the middle of the index range (one eighth of the rows)."""
    return slice(n // 2, n // 2 + max(1, n // 8))


def case_inputs(c: Case):
    """CPU tensors: x (n,3), t (n,1) [stride 0 for "expand"], cotangents (3 tensors; (n,4,4) first for 6dof), dead-row mask.
    x is uniform in [-1.3, 1.3] except the scene slab, uniform in [-SCENE, SCENE]; the cotangents are zero on the rows with
    |x_1| > 0.9 outside that slab (what culled Gaussians send back), so the backward skips whole tiles under the Morton order."""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    n = c.n
    x = (torch.rand(n, 3, generator=g) * 2 - 1) * 1.3
    sl = scene_rows(n)
    x[sl] = (torch.rand(x[sl].shape, generator=g) * 2 - 1) * SCENE
    if c.tkind == "expand":
        t = torch.rand(1, 1, generator=g).expand(n, -1)
    else:
        t = torch.rand(n, 1, generator=g)
    scene = torch.zeros(n, dtype=torch.bool)
    scene[sl] = True
    dead = (x[:, 1].abs() > 0.9) & ~scene
    shapes = ((4, 4), (4,), (3,)) if c.variant == "6dof" else ((3,), (4,), (3,))
    cot = [torch.randn((n,) + s, generator=g) * (~dead).reshape((n,) + (1,) * len(s)) for s in shapes]
    return x, t, cot, dead, scene


def _to_dev(x, t):
    x = x.cuda()
    t = t[0:1].cuda().expand(x.shape[0], -1) if t.stride(0) == 0 else t.cuda()
    return x, t


def run(out_path: str, mode: str = "both") -> None:
    """Evaluate every case with the library's current form; mode "infer" / "train" / "both" picks the entry points."""
    from trase_amd import deform
    res: Dict[str, np.ndarray] = {}
    params = {v: {k: p.cuda() for k, p in make_params(v).items()} for v in ("default", "blender", "6dof")}
    try:
        for c in cases():
            x, t, cot, _, _ = case_inputs(c)
            x, t = _to_dev(x, t)
            P = params[c.variant]
            kw = dict(is_blender=c.variant == "blender", is_6dof=c.variant == "6dof")
            if mode in ("infer", "both"):
                runs = []
                for _ in range(2):
                    with torch.no_grad():
                        runs.append([o.cpu().numpy() for o in deform.deform_forward(P, x, t, **kw)])
                for j in range(3):
                    res[f"{c.name}|infer|{j}"] = runs[0][j]
                res[f"{c.name}|infer|repro"] = np.array(all(np.array_equal(a, b) for a, b in zip(*runs)))
            if mode in ("train", "both"):
                cd = [v.cuda() for v in cot]
                for order in c.orders:
                    deform.set_row_order(order)
                    runs = []
                    for _ in range(2):
                        leaf = {k: v.clone().requires_grad_(True) for k, v in P.items()}
                        out = deform.deform_forward(leaf, x, t, **kw)
                        torch.autograd.backward(out, cd)
                        runs.append(([o.detach().cpu().numpy() for o in out],
                                     {k: v.grad.cpu().numpy() for k, v in leaf.items()}))
                    tag = f"{c.name}|train-{order}"
                    for j in range(3):
                        res[f"{tag}|{j}"] = runs[0][0][j]
                    for k, g in runs[0][1].items():
                        res[f"{tag}|grad|{k}"] = g
                    same = all(np.array_equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
                    same = same and all(np.array_equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
                    res[f"{tag}|repro"] = np.array(same)
            torch.cuda.synchronize()
    finally:
        deform.set_row_order("morton")
    np.savez(out_path, **res)


if __name__ == "__main__":
    run(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "both")
