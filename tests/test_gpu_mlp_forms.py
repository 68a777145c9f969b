"""Both kernel forms of the deformation MLP (trase_amd/csrc/mlp.hip) at full size against the float64 reference of
tests/mlp_reference.py (bf16 operands, float64 arithmetic):
  inference  register-chained kernel, two 32-row groups per wave (mlp_fwd_rc_kernel)
  training   block kernel (mlp_fwd_train_kernel_blk, FULL and tail workgroups) + the backward kernels
tests/mlp_forms_child.py runs them over the cases and writes outputs and gradients to an .npz; this module builds the
reference and asserts.

Cases (tests/mlp_forms_child.py:cases): 255 .. 300 000 rows, the tails 256 k + r of every wave position of the last RC
workgroup, 1 000 000 training rows; time as a stride-0 expand and as distinct per-row values; is_blender and is_6dof at
20 011 and 300 000 rows; one eighth of the rows at scene-sized coordinates (|x| up to 40); a dead slab of zero cotangents;
Morton and index row order.  Every bar below is checked separately on the unit-cube rows and on the scene rows.
"""
import os

import numpy as np
import pytest
import torch

from tests import mlp_forms_child as child
from tests import mlp_reference as R

pytestmark = pytest.mark.gpu

# Outputs against the bf16 float64 reference, per row group (elementwise of the group's output scale, relative L2 per output).
# The 2e-3 elementwise bar of the 20 011-row test (test_gpu_parity.py) does not hold at full size for either form: an
# activation whose fp32 sum lands within accumulation noise of a bf16 rounding boundary rounds to the neighbouring bf16 value
# (0.4 % of it), which moves an output by ~2e-3 of its scale; with 300 k rows x 2048 activations such rows always exist.  The
# two forms differ from EACH OTHER by as much (below); the mutated references of the last test miss by 0.25 (rows swapped), 0.63
# (time of the next row) and 5.9 (skip encoding dropped) of scale.
# Measured worst on MI355X: unit rows 4.71e-3 of scale (blender, 300 000) / rel L2 4.55e-4; scene rows 4.66e-3 / rel L2 8.95e-4
# (32 scene rows of 257).  Before the encoding's argument reduction (mlp.hip pe_rev) the unit rows' rel L2 was 7.7e-4 and the
# scene rows' 3.7e-3: __sinf lost up to 1e-3 rad at |x 2^9| = 2e4 rad, a quarter of a bf16 ulp of the encoding.
OUT_ABS = 1e-5
OUT_BARS = {"unit": (1e-2, 1.5e-3), "scene": (1e-2, 3e-3)}       # group -> (elementwise of scale, relative L2)
# Training forward against the inference forward, of max(scale, 1): the unit rows keep the bar of the suite's training-vs-inference
# check (test_gpu_parity.py, 4e-4; measured worst 2.70e-4, 6dof 300 000).  Scene-sized rows feed |x| up to 40 into the
# network, so their activations are large against their outputs and one bf16 flip moves an output further: measured worst
# 1.17e-3 (1 000 000 rows).
FORM_TOLS = {"unit": 4e-4, "scene": 2.5e-3}
# parameter gradients against the bf16 float64 reference, the bars of test_deform_mlp_training_step_matches_bf16_evaluated_autograd
# (measured worst: rel L2 1.80e-2, linear.0.weight at 769 rows; elementwise 4.95e-2 of scale at 769 rows)
GRAD_REL_L2, GRAD_ELEM = 5e-2, 1e-1


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """NpzFile of the inference and training outputs and gradients of every case."""
    if os.environ.get("TRASE_MLP_ROW_ORDER", "morton") != "morton":
        pytest.fail("the test process must run the default Morton row order; found TRASE_MLP_ROW_ORDER in the environment")
    path = str(tmp_path_factory.mktemp("mlp_forms") / "default.npz")
    child.run(path, "both")
    return np.load(path)


@pytest.fixture(scope="module")
def refs():
    """case name -> (3 float64 reference outputs, float64 parameter gradients for the case's cotangents), on the GPU."""
    cache = {}

    def get(c):
        if c.name not in cache:
            x, t, cot, _, _ = child.case_inputs(c)
            P = child.make_params(c.variant)
            cache[c.name] = R.evaluate(P, x.cuda(), t.cuda(), [v.cuda() for v in cot], c.variant == "blender",
                                       c.variant == "6dof")
        return cache[c.name]
    return get


def _groups(c):
    _, _, _, _, scene = child.case_inputs(c)
    return (("unit", ~scene), ("scene", scene))


def compare_outputs(got, ref, groups):
    """Per row group the worst (max error / scale, relative L2) over the three outputs, and the list of misses."""
    worst, miss = {}, []
    for gname, rows in groups:
        rows = rows.cuda()
        if not bool(rows.any()):
            continue
        we, wr = 0.0, 0.0
        for j, (g, r) in enumerate(zip(got, ref)):
            r = r[rows].reshape(int(rows.sum()), -1)
            dd = torch.as_tensor(g).cuda()[rows].reshape(r.shape).double() - r
            scale, err = float(r.abs().max()), float(dd.abs().max())
            rel = float(dd.norm() / r.norm())
            we, wr = max(we, err / scale), max(wr, rel)
            elem, rel_l2 = OUT_BARS[gname]
            if not (err < elem * scale + OUT_ABS and rel < rel_l2):
                miss.append(f"{gname} output {j}: max {err:.3e} vs scale {scale:.3e}, rel L2 {rel:.3e}")
        worst[gname] = (we, wr)
    return worst, miss


def _fmt(worst):
    return "  ".join(f"{g}: max {e:.2e} of scale, rel L2 {r:.2e}" for g, (e, r) in worst.items())


def _outputs(res, tag):
    return [res[f"{tag}|{j}"] for j in range(3)]


def test_inference_and_training_forwards_match_float64_reference(results, refs):
    """The inference outputs and the training forward's outputs (every row order), every case, against the bf16 float64
    reference."""
    misses = []
    for c in child.cases():
        ref, _ = refs(c)
        groups = _groups(c)
        for tag in [f"{c.name}|infer"] + [f"{c.name}|train-{o}" for o in c.orders]:
            worst, miss = compare_outputs(_outputs(results, tag), ref, groups)
            print(f"[measured] {tag:36s} vs float64 ref  {_fmt(worst)}")
            misses += [f"{tag}: {m}" for m in miss]
    assert not misses, "\n".join(misses)


def test_forms_agree_with_default_inference(results):
    """The training forward (every row order) against the inference forward, every case."""
    misses = []
    for c in child.cases():
        base = _outputs(results, f"{c.name}|infer")
        groups = _groups(c)
        for tag in [f"{c.name}|train-{o}" for o in c.orders]:
            worst = {}
            for gname, rows in groups:
                if not bool(rows.any()):
                    continue
                worst[gname] = 0.0
                for j, (a, b) in enumerate(zip(_outputs(results, tag), base)):
                    a, b = a[rows.numpy()], b[rows.numpy()]
                    d, scale = float(np.abs(a - b).max()), max(float(np.abs(b).max()), 1.0)
                    worst[gname] = max(worst[gname], d / scale)
                    if d > FORM_TOLS[gname] * scale:
                        misses.append(f"{tag} {gname} output {j}: {d:.3e} vs inference (scale {scale:.3e})")
            print(f"[measured] {tag:36s} vs inference  "
                  + "  ".join(f"{g}: {v:.2e}" for g, v in worst.items()) + " of max(scale, 1)")
    assert not misses, "\n".join(misses)


def test_training_gradients_match_float64_reference(results, refs):
    """Every case and row order, every parameter gradient against the float64 reference's (straight-through bf16
    rounding; dead slab of zero cotangents included)."""
    misses = []
    for c in child.cases():
        _, want = refs(c)
        for o in c.orders:
            tag = f"{c.name}|train-{o}"
            wr, we, wk = 0.0, 0.0, ""
            for k, w in want.items():
                g = torch.as_tensor(results[f"{tag}|grad|{k}"]).cuda().double()
                scale = float(w.abs().max())
                if scale == 0.0:
                    if float(g.abs().max()) != 0.0:
                        misses.append(f"{tag} grad {k}: nonzero where the reference is zero")
                    continue
                err, rel = float((g - w).abs().max()), float((g - w).norm() / w.norm())
                if rel > wr:
                    wk = k
                wr, we = max(wr, rel), max(we, err / scale)
                if not (rel < GRAD_REL_L2 and err < GRAD_ELEM * scale + 1e-6):
                    misses.append(f"{tag} grad {k}: rel L2 {rel:.3e}, max {err:.3e} vs scale {scale:.3e}")
            print(f"[measured] {tag:36s} grads vs float64 ref: worst rel L2 {wr:.2e} ({wk}), worst max {we:.2e} of scale")
    assert not misses, "\n".join(misses)


def test_forms_are_bit_reproducible(results):
    """Every case, run twice, gives bit-identical outputs (and gradients)."""
    bad = [k for k in results.files if k.endswith("|repro") and not bool(results[k])]
    assert not bad, bad


def test_bars_reject_mutated_references(results, refs):
    """The output comparison must fail against three wrong references of the default inference at 20 011 rows, per-row
    time: two adjacent rows swapped in the last full 256-row workgroup, every row's time taken from the next row, and the
    skip layer's encoding columns dropped."""
    c = next(c for c in child.cases() if c.name == "default-20011-rows")
    got = _outputs(results, f"{c.name}|infer")
    ref, _ = refs(c)
    groups = _groups(c)
    worst, miss = compare_outputs(got, ref, groups)
    print(f"[measured] unmutated reference: {_fmt(worst)}")
    assert not miss, miss
    x, t, _, _, scene = child.case_inputs(c)
    P = child.make_params(c.variant)
    i = 256 * (c.n // 256) - 2
    assert not bool(scene[i]) and not bool(scene[i + 1])
    swapped = tuple(r.clone() for r in ref)
    for r in swapped:
        r[[i, i + 1]] = r[[i + 1, i]]
    shifted, _ = R.evaluate(P, x.cuda(), torch.roll(t, -1, 0).cuda())
    no_skip, _ = R.evaluate(P, x.cuda(), t.cuda(), skip_encoding=False)
    accepted = []
    for name, mut in (("rows swapped", swapped), ("time of the next row", shifted), ("skip encoding dropped", no_skip)):
        worst, miss = compare_outputs(got, mut, groups)
        print(f"[measured] mutation '{name}': {_fmt(worst)} -> {len(miss)} misses")
        if not miss:
            accepted.append(name)
    assert not accepted, f"the output bars accept the mutated references {accepted}"
