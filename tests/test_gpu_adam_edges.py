"""The fused Adam step (trase_amd/csrc/optim.hip: adam_kernel behind trase_amd.optim.FusedAdam) against the float64
restatement of tests/adam_reference.py: tensor sizes around the 1024-element block and the 4-element vector, an empty tensor
in the table, more tensors than one launch takes, pointers that are not 16-byte aligned, the bias corrections at step 1 and
step 30 000, gradients from 1e2 down to where g^2 underflows in float32, and the bookkeeping of partial steps.

Tolerance: none is fixed in advance.  Every case also runs torch.optim.Adam(..., eps=1e-15, foreach=False) in float32 on
the CPU on the same inputs and measures ITS distance to float64 per tensor (max-abs) for the parameter and both moments.
The kernel's bar, per tensor and quantity, is

    MARGIN * (float32 torch.optim.Adam's error)  +  FLOOR_ULPS * (2^-23 * max|float64 value| + 2^-149)

MARGIN = 4: the kernel states the same update in the same order of operations as torch's single-tensor path, except that it
rounds lr, 1 - b1^t and sqrt(1 - b2^t) to float32 separately where torch folds lr / bc1 in double (two more roundings on the
step, one on the denominator).  FLOOR_ULPS = 4 ulps of the tensor's scale stay when torch's error happens to vanish; 2^-149
is the spacing of float32 subnormals, the ulp of exp_avg_sq at gradients of 1e-20.  `guard=None` throughout.  No number
below is derived from the kernel's output.

Measured (largest error over the case's tensors as a fraction of each tensor's scale; `f32` is float32 torch.optim.Adam on
the CPU, `hip` the kernel on an MI355X; every test prints its figures as
`ADAMEDGE <case> p: f32=... hip=... m: ... v: ...` after its comparisons; margin 4 throughout):

    case                         p f32    p hip     m f32    m hip     v f32    v hip     margin
    sizes-forward-five_steps     1.2e-07  1.2e-07   3.1e-07  3.1e-07   2.1e-07  2.0e-07   4
    sizes-forward-step_one       4.0e-08  4.0e-08   6.5e-08  6.5e-08   1.4e-07  1.4e-07   4
    sizes-forward-step_30000     3.6e-08  3.6e-08   6.3e-08  6.3e-08   1.0e-07  5.9e-08   4
    sizes-reversed-five_steps    1.3e-07  1.3e-07   8.8e-08  8.8e-08   1.7e-07  1.5e-07   4
    sizes-reversed-step_one      4.6e-08  4.6e-08   6.8e-08  6.8e-08   9.9e-08  9.9e-08   4
    sizes-reversed-step_30000    1.1e-07  1.1e-07   6.5e-08  6.5e-08   1.0e-07  6.4e-08   4
    chunks-19                    9.9e-08  9.9e-08   1.1e-07  1.1e-07   1.6e-07  1.3e-07   4
    chunks-16                    1.1e-07  1.1e-07   1.6e-07  1.6e-07   1.4e-07  1.6e-07   4
    grad-none                    9.1e-08  9.1e-08   7.5e-08  7.5e-08   1.1e-07  1.1e-07   4
    misaligned-p-1               7.1e-08  7.1e-08   7.3e-08  7.3e-08   1.1e-07  1.6e-07   4
    misaligned-p-2               8.8e-08  8.8e-08   7.1e-08  7.1e-08   1.2e-07  1.1e-07   4
    misaligned-p-3               6.5e-08  6.5e-08   1.1e-07  1.1e-07   1.1e-07  1.2e-07   4
    misaligned-g-1               7.1e-08  7.1e-08   7.3e-08  7.3e-08   1.1e-07  1.6e-07   4
    misaligned-g-2               8.8e-08  8.8e-08   7.1e-08  7.1e-08   1.2e-07  1.1e-07   4
    misaligned-g-3               6.5e-08  6.5e-08   1.1e-07  1.1e-07   1.1e-07  1.2e-07   4
    misaligned-both-1            7.6e-08  7.6e-08   6.7e-08  6.7e-08   1.1e-07  9.8e-08   4
    misaligned-both-2            9.5e-08  9.5e-08   7.9e-08  7.9e-08   1.2e-07  1.4e-07   4
    misaligned-both-3            7.7e-08  7.7e-08   6.3e-08  6.3e-08   9.3e-08  9.8e-08   4
    regimes-five_steps           1.1e-07  1.1e-07   8.2e-08  8.2e-08   2.1e-03  2.1e-03   4
    regimes-step_30000           1.0e-07  1.0e-07   7.3e-08  7.3e-08   2.1e-03  2.1e-03   4
"""
import pytest
import torch

from tests.adam_reference import Adam64

pytestmark = pytest.mark.gpu

MARGIN = 4.0
FLOOR_ULPS = 4.0
ULP = 2.0 ** -23
SUBNORMAL = 2.0 ** -149
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2051, 0, 7, 4096]
GRAD_SCALES = [1e2, 1.0, 1e-6, 1e-12, 1e-20]
LATE = 29_999


def _lrs(n):
    return [(1.6e-4, 2.5e-3, 1.25e-4, 5e-2, 5e-3, 1e-3, 1e-2)[k % 7] for k in range(n)]


def _groups(params, lrs):
    return [{"params": [p], "lr": lr, "name": str(k)} for k, (p, lr) in enumerate(zip(params, lrs))]


def _seed_state(opt, p, step0, m, v):
    opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": m, "exp_avg_sq": v}


def _run(init, lrs, grads, preseed=None, place=None, place_grad=None):
    """init: float32 CPU tensors; grads[it][k]: a float32 CPU tensor or None; preseed: (step0, [m], [v]) or None.
    -> (float64 reference, float32 CPU optimiser and its parameters, FusedAdam and its parameters).  The learning rate of
    tensor 0 decays after every step (update_learning_rate, train.py:388-389)."""
    from trase_amd.optim import FusedAdam
    dev = torch.device("cuda", 0)
    place = place or (lambda t, k: t.clone().to(dev))
    place_grad = place_grad or (lambda t, k: t.to(dev))
    ref = Adam64(init, lrs)
    cp = [t.clone().requires_grad_(True) for t in init]
    gp = [place(t, k).detach().requires_grad_(True) for k, t in enumerate(init)]
    copt = torch.optim.Adam(_groups(cp, lrs), lr=0.0, eps=1e-15, foreach=False)
    gopt = FusedAdam(_groups(gp, lrs), lr=0.0, eps=1e-15)
    if preseed is not None:
        step0, ms, vs = preseed
        for k in range(len(init)):
            ref.seed(k, step0, ms[k], vs[k])
            _seed_state(copt, cp[k], step0, ms[k].clone(), vs[k].clone())
            _seed_state(gopt, gp[k], step0, ms[k].to(dev), vs[k].to(dev))
    for step_grads in grads:
        for k, g in enumerate(step_grads):
            cp[k].grad = None if g is None else g.clone()
            gp[k].grad = None if g is None else place_grad(g, k)
        ref.step(step_grads); copt.step(); gopt.step(guard=None)
        ref.lrs[0] *= 0.97; copt.param_groups[0]["lr"] *= 0.97; gopt.param_groups[0]["lr"] *= 0.97
    torch.cuda.synchronize()
    return ref, copt, cp, gopt, gp


def _compare(name, init, ref, copt, cp, gopt, gp):
    worst = {q: [0.0, 0.0] for q in "pmv"}
    for k in range(len(init)):
        if ref.steps[k] == 0:                              # never received a gradient: untouched, and no state was made
            assert torch.equal(gp[k].detach().cpu(), init[k]) and len(gopt.state[gp[k]]) == 0, (name, k)
            continue
        sc, sg = copt.state[cp[k]], gopt.state[gp[k]]
        assert int(sg["step"]) == int(sc["step"]) == ref.steps[k], (name, k)
        assert sg["step"].device.type == "cpu" and set(sg.keys()) == {"step", "exp_avg", "exp_avg_sq"}
        for q, want, c32, got in (("p", ref.p[k], cp[k], gp[k]), ("m", ref.m[k], sc["exp_avg"], sg["exp_avg"]),
                                  ("v", ref.v[k], sc["exp_avg_sq"], sg["exp_avg_sq"])):
            got = got.detach().cpu().double()
            assert got.shape == want.shape and bool(torch.isfinite(got).all()), (name, k, q)
            if want.numel() == 0:
                continue
            scale = float(want.abs().max())
            err32 = float((c32.detach().double() - want).abs().max())
            diff = (got - want).abs()
            err = float(diff.max())
            bar = MARGIN * err32 + FLOOR_ULPS * (ULP * scale + SUBNORMAL)
            unit = max(scale, SUBNORMAL)
            worst[q] = [max(worst[q][0], err32 / unit), max(worst[q][1], err / unit)]
            i = int(diff.argmax())
            assert err <= bar, (f"{name}: tensor {k} ({want.numel()} elements) {q}[{i}]: kernel {float(got[i])!r}, float64 "
                                f"{float(want[i])!r}: off by {err:.3e}, bar {bar:.3e} = {MARGIN} x {err32:.3e} + "
                                f"{FLOOR_ULPS} ulp of {scale:.3e}")
    print(f"ADAMEDGE {name} " + " ".join(f"{q}: f32={worst[q][0]:.2e} hip={worst[q][1]:.2e}" for q in "pmv"))


def _inputs(sizes, n_steps, seed, grad_scale=None):
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(n, generator=g) for n in sizes]
    scale = grad_scale or (lambda k: 10.0 ** (k % 3 - 2))
    grads = [[torch.randn(n, generator=g) * scale(k) for k, n in enumerate(sizes)] for _ in range(n_steps)]
    return g, init, grads


def _late_state(g, sizes):
    return (LATE, [0.1 * torch.randn(n, generator=g) for n in sizes], [0.01 * torch.rand(n, generator=g) + 1e-6 for n in sizes])


@pytest.mark.parametrize("mode", ["five_steps", "step_one", "step_30000"])
@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_sizes_around_the_block_and_the_vector(order, mode):
    """One-block tensors next to each other, block-exact sizes and an empty tensor in the middle of first_block[]; five
    steps from an empty state, step 1 alone, and one step resumed at 29 999 with moments in place."""
    sizes = SIZES if order == "forward" else SIZES[::-1]
    g, init, grads = _inputs(sizes, 5 if mode == "five_steps" else 1, seed=len(mode) + len(order))
    preseed = _late_state(g, sizes) if mode == "step_30000" else None
    out = _run(init, _lrs(len(sizes)), grads, preseed)
    _compare(f"sizes-{order}-{mode}", init, *out)
    ref, gopt, gp = out[0], out[3], out[4]
    k0 = sizes.index(0)
    assert gp[k0].numel() == 0 and int(gopt.state[gp[k0]]["step"]) == ref.steps[k0]
    if mode == "step_one":            # bias corrections at t = 1: every element moves by lr * sign(g), whatever |g|
        for k, n in enumerate(sizes):
            moved = (init[k].double() - gp[k].detach().cpu().double())
            want = _lrs(len(sizes))[k] * grads[0][k].double().sign()
            assert n == 0 or float((moved - want).abs().max()) <= 4 * ULP * float(init[k].abs().max()) + 1e-5 * _lrs(len(sizes))[k], k


@pytest.mark.parametrize("with_grad", [19, 16])
def test_more_tensors_than_one_launch_takes(with_grad):
    """FusedAdam.step hands the kernel 16 tensors at a time: 19 with a gradient (16 + 3), and 19 of which exactly 16 have one
    -- the other three keep their values and get no state."""
    sizes = [5, 1, 37, 1024, 3, 260, 2, 1025, 9, 64, 7, 4, 129, 33, 6, 1000, 11, 8, 515]
    assert len(sizes) == 19
    _, init, grads = _inputs(sizes, 3, seed=with_grad)
    without = {} if with_grad == 19 else {2, 9, 17}
    grads = [[None if k in without else gk for k, gk in enumerate(step)] for step in grads]
    assert sum(gk is not None for gk in grads[0]) == with_grad
    out = _run(init, _lrs(19), grads)
    _compare(f"chunks-{with_grad}", init, *out)


def test_a_parameter_without_gradient_keeps_values_moments_and_counter():
    sizes = [1025, 7, 300]
    _, init, grads = _inputs(sizes, 4, seed=3)
    grads[2][1] = None
    grads[2][2] = None
    grads[3][2] = None
    ref, copt, cp, gopt, gp = _run(init, _lrs(3), grads[:2])
    before = [(p.detach().clone(), gopt.state[p]["exp_avg"].clone(), gopt.state[p]["exp_avg_sq"].clone()) for p in gp]
    dev = gp[0].device
    for step in grads[2:]:
        for k, gk in enumerate(step):
            gp[k].grad = None if gk is None else gk.to(dev)
            cp[k].grad = None if gk is None else gk.clone()
        ref.step(step); copt.step(); gopt.step(guard=None)
    assert [int(gopt.state[p]["step"]) for p in gp] == ref.steps == [4, 3, 2]
    for k in (2,):                                       # skipped twice: bit-identical to the state after two steps
        for a, b in zip(before[k], (gp[k].detach(), gopt.state[gp[k]]["exp_avg"], gopt.state[gp[k]]["exp_avg_sq"])):
            assert torch.equal(a, b)
    assert not torch.equal(before[0][0], gp[0].detach()) and not torch.equal(before[1][0], gp[1].detach())
    _compare("grad-none", init, ref, copt, cp, gopt, gp)


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("which", ["p", "g", "both"])
def test_pointers_that_are_not_16_byte_aligned(which, offset):
    """Parameters and / or gradients as contiguous 1-D slices of a larger buffer that start 4, 8 or 12 bytes past a 16-byte
    boundary (a gradient that is a view into a flat all-reduce bucket): the same bar as the aligned run, and the elements of
    the backing buffer around the slice keep their bits."""
    dev = torch.device("cuda", 0)
    sizes = [5, 1027]
    g, init, grads = _inputs(sizes, 3, seed=10 * offset + len(which))
    pad = 8
    fill = lambda n: torch.randn(n + 2 * pad, generator=g)
    pbuf = [fill(n).to(dev) for n in sizes]
    gbuf = [[fill(n).to(dev) for n in sizes] for _ in grads]
    pbuf0 = [b.clone() for b in pbuf]
    gbuf0 = [[b.clone() for b in bs] for bs in gbuf]
    step_no = [0]

    def place(t, k):
        if which == "g":
            return t.to(dev)
        view = pbuf[k][offset:offset + t.numel()]
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4 * offset
        return view

    def place_grad(t, k):
        if which == "p":
            return t.to(dev)
        view = gbuf[step_no[0] // len(sizes)][k][offset:offset + t.numel()]
        step_no[0] += 1
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4 * offset
        return view

    out = _run(init, _lrs(2), grads, place=place, place_grad=place_grad)
    _compare(f"misaligned-{which}-{offset}", init, *out)
    gp = out[4]
    for k, n in enumerate(sizes):
        if which != "g":
            assert gp[k].data_ptr() == pbuf[k].data_ptr() + 4 * offset                 # the kernel wrote through the slice
            assert torch.equal(pbuf[k][:offset], pbuf0[k][:offset]) and torch.equal(pbuf[k][offset + n:], pbuf0[k][offset + n:])
            assert torch.equal(pbuf[k][offset:offset + n], gp[k].detach())
        if which != "p":
            for it in range(len(grads)):
                assert torch.equal(gbuf[it][k][:offset], gbuf0[it][k][:offset])
                assert torch.equal(gbuf[it][k][offset + n:], gbuf0[it][k][offset + n:])
                assert torch.equal(gbuf[it][k][offset:offset + n], grads[it][k].to(dev))   # gradients are read only


@pytest.mark.parametrize("mode", ["five_steps", "step_30000"])
def test_gradient_regimes_down_to_underflow_and_exact_zeros(mode):
    """One tensor per gradient scale 1e2 ... 1e-20 (g^2 underflows in float32 at the last).  Of every three elements the first
    never receives a gradient -- it keeps its bits and both moments stay exactly 0, the reference's unseen Gaussians
    (0 / (0 + 1e-15)) -- the second receives one at the first step and zeros afterwards, the third at every step."""
    n = 1029
    sizes = [n] * len(GRAD_SCALES)
    g, init, grads = _inputs(sizes, 5, seed=7, grad_scale=lambda k: GRAD_SCALES[k])
    idx = torch.arange(n)
    for it, step in enumerate(grads):
        for gk in step:
            gk[idx % 3 == 0] = 0.0
            if it > 0:
                gk[idx % 3 == 1] = 0.0
    preseed = None
    if mode == "step_30000":          # resumed: the unseen elements come with zero moments, the others with history
        step0, ms, vs = _late_state(g, sizes)
        for k in range(len(sizes)):
            ms[k] *= GRAD_SCALES[k]; vs[k] *= GRAD_SCALES[k] ** 2
            ms[k][idx % 3 == 0] = 0.0; vs[k][idx % 3 == 0] = 0.0
        preseed = (step0, ms, vs)
    out = _run(init, _lrs(len(sizes)), grads, preseed)
    _compare(f"regimes-{mode}", init, *out)
    gopt, gp = out[3], out[4]
    unseen = (idx % 3 == 0)
    for k in range(len(sizes)):
        st = gopt.state[gp[k]]
        assert torch.equal(gp[k].detach().cpu()[unseen], init[k][unseen]), GRAD_SCALES[k]
        assert not st["exp_avg"].cpu()[unseen].any() and not st["exp_avg_sq"].cpu()[unseen].any(), GRAD_SCALES[k]
        assert not torch.equal(gp[k].detach().cpu()[~unseen], init[k][~unseen])


def test_two_partial_steps_equal_one_whole_step_bit_for_bit():
    """step(only=A) followed by step(only=B) against one step() over A u B, twice over (so the second round starts from
    moments the first one made); a parameter outside both stays out."""
    from trase_amd.optim import FusedAdam
    dev = torch.device("cuda", 0)
    sizes = [1, 1023, 1024, 1025, 0, 7, 2051, 5]
    _, init, grads = _inputs(sizes, 2, seed=11)
    lrs = _lrs(len(sizes))
    pa = [t.clone().to(dev).requires_grad_(True) for t in init]
    pb = [t.clone().to(dev).requires_grad_(True) for t in init]
    oa, ob = FusedAdam(_groups(pa, lrs), lr=0.0, eps=1e-15), FusedAdam(_groups(pb, lrs), lr=0.0, eps=1e-15)
    first, second, out = [0, 2, 5, 6], [1, 3, 4], 7
    for step in grads:
        for k, gk in enumerate(step):
            pa[k].grad = gk.to(dev); pb[k].grad = gk.to(dev)
        oa.step(guard=None, only=[pa[k] for k in first])
        oa.step(guard=None, only=[pa[k] for k in second])
        ob.step(guard=None, only=[pb[k] for k in first + second])
    for k in range(len(sizes)):
        if k == out:
            assert torch.equal(pa[k].detach().cpu(), init[k]) and len(oa.state[pa[k]]) == 0 and len(ob.state[pb[k]]) == 0
            continue
        sa, sb = oa.state[pa[k]], ob.state[pb[k]]
        assert int(sa["step"]) == int(sb["step"]) == 2
        assert torch.equal(pa[k], pb[k]) and torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
        assert sizes[k] == 0 or not torch.equal(pa[k].detach().cpu(), init[k])
    # and a whole step() equals them both
    pc = [t.clone().to(dev).requires_grad_(True) for t in init]
    oc = FusedAdam(_groups(pc, lrs), lr=0.0, eps=1e-15)
    for step in grads:
        for k, gk in enumerate(step):
            pc[k].grad = None if k == out else gk.to(dev)
        oc.step(guard=None)
    for k in range(len(sizes)):
        assert torch.equal(pa[k], pc[k]), k
