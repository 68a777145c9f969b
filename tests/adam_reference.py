"""float64 restatement of the single-tensor Adam update, exactly as the header of trase_amd/csrc/optim.hip states it:

    m <- lerp(m, g, 1 - b1);  v <- b2 v + (1 - b2) g g;  p <- p - (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)

with bc1 = 1 - b1^step, bc2 = 1 - b2^step formed in double.  Every tensor carries its own learning rate and its own step
counter (torch.optim.Adam's per-parameter state, scene/gaussian_model.py:253-300).  Test infrastructure, CPU only."""
from __future__ import annotations

import torch


def adam_update(p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-15):
    """One update of one tensor.  ``step`` is the 1-based count of this update.  -> new (p, m, v), float64; the inputs
    are left unchanged."""
    if step < 1:
        raise ValueError("step counts from 1")
    p, g, m, v = (torch.as_tensor(t).detach().cpu().double() for t in (p, g, m, v))
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = v.sqrt() / (bc2 ** 0.5) + eps
    return p - (lr / bc1) * (m / denom), m, v


class Adam64:
    """A list of tensors stepped like an optimiser with one group per tensor: ``lrs[i]`` may be edited between steps, a
    gradient of None leaves the tensor, its moments and its counter alone."""

    def __init__(self, params, lrs, betas=(0.9, 0.999), eps=1e-15):
        self.p = [torch.as_tensor(t).detach().cpu().double().clone() for t in params]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.steps = [0] * len(self.p)
        self.lrs = [float(x) for x in lrs]
        self.betas, self.eps = betas, eps
        assert len(self.lrs) == len(self.p)

    def seed(self, i, step, exp_avg, exp_avg_sq):
        """Pre-set the state of tensor i (a resumed checkpoint)."""
        self.steps[i] = int(step)
        self.m[i] = torch.as_tensor(exp_avg).detach().cpu().double().clone()
        self.v[i] = torch.as_tensor(exp_avg_sq).detach().cpu().double().clone()

    def step(self, grads):
        assert len(grads) == len(self.p)
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.steps[i] += 1
            self.p[i], self.m[i], self.v[i] = adam_update(self.p[i], g, self.m[i], self.v[i], self.lrs[i], self.steps[i],
                                                          self.betas[0], self.betas[1], self.eps)
