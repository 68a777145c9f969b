"""tests/adam_reference.py against torch.optim.Adam(..., eps=1e-15, foreach=False) run in float64 on the CPU: per-tensor
learning rates that change between steps, a tensor without a gradient in one step, a pre-seeded state at step 29 999, an
empty tensor, gradients from 1e2 down to 1e-20 and exact zeros.  No GPU."""
import pytest
import torch

from tests.adam_reference import Adam64, adam_update

# both sides are float64 and differ in the order of a handful of operations (torch folds lr / bc1 into addcdiv's scalar
# and divides sqrt(v) by sqrt(bc2) as we do): a few ulps of 2^-53, compared at 1e-13 of each quantity's scale
REL = 1e-13


def _close(got, want, what):
    scale = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= REL * scale, (what, err, scale)


def _torch_adam(params, lrs):
    return torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(params, lrs)], lr=0.0, eps=1e-15, foreach=False)


def test_matches_torch_adam_in_float64_over_steps():
    g = torch.Generator().manual_seed(0)
    sizes = [1, 5, 0, 1025, 37]
    lrs = [1.6e-4, 2.5e-3, 1e-3, 5e-2, 1e-2]
    init = [torch.randn(n, generator=g, dtype=torch.float64) for n in sizes]
    tp = [t.clone().requires_grad_(True) for t in init]
    opt, ref = _torch_adam(tp, lrs), Adam64(init, lrs)
    for it in range(6):
        grads = []
        for k, t in enumerate(tp):
            gk = torch.randn(t.shape, generator=g, dtype=torch.float64) * 10.0 ** (2 - 5 * k)
            if it >= 2:
                gk[::3] = 0.0
            grads.append(None if (it == 3 and k == 1) else gk)
            t.grad = None if grads[-1] is None else gk.clone()
        opt.step(); ref.step(grads)
        opt.param_groups[0]["lr"] *= 0.97; ref.lrs[0] *= 0.97
    for k, t in enumerate(tp):
        st = opt.state[t]
        assert int(st["step"]) == ref.steps[k] == (5 if k == 1 else 6)
        _close(ref.p[k], t.detach(), ("p", k)); _close(ref.m[k], st["exp_avg"], ("m", k)); _close(ref.v[k], st["exp_avg_sq"], ("v", k))


@pytest.mark.parametrize("step0", [0, 29_999])
def test_bias_corrections_at_the_first_and_a_late_step(step0):
    g = torch.Generator().manual_seed(step0 + 1)
    p0 = torch.randn(64, generator=g, dtype=torch.float64)
    m0 = 0.1 * torch.randn(64, generator=g, dtype=torch.float64) if step0 else torch.zeros(64, dtype=torch.float64)
    v0 = 0.01 * torch.rand(64, generator=g, dtype=torch.float64) if step0 else torch.zeros(64, dtype=torch.float64)
    gr = torch.randn(64, generator=g, dtype=torch.float64)
    t = p0.clone().requires_grad_(True)
    opt = _torch_adam([t], [1e-2])
    if step0:
        opt.state[t] = {"step": torch.tensor(float(step0)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    t.grad = gr.clone()
    opt.step()
    p1, m1, v1 = adam_update(p0, gr, m0, v0, 1e-2, step0 + 1)
    _close(p1, t.detach(), "p"); _close(m1, opt.state[t]["exp_avg"], "m"); _close(v1, opt.state[t]["exp_avg_sq"], "v")
    if not step0:                      # step 1 from an empty state moves every element by lr * sign(g) (eps is 1e-15)
        assert float(((p0 - p1) - 1e-2 * gr.sign()).abs().max()) < 1e-12


def test_zero_gradient_leaves_an_unseen_row_bit_identical():
    p0 = torch.randn(9, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    ref = Adam64([p0], [1e-2])
    for _ in range(3):
        ref.step([torch.zeros(9, dtype=torch.float64)])
    assert torch.equal(ref.p[0], p0) and not ref.m[0].any() and not ref.v[0].any() and ref.steps == [3]
    with pytest.raises(ValueError):
        adam_update(p0, p0, p0, p0, 1e-2, 0)
