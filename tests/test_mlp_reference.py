"""The float64 reference of tests/mlp_reference.py IS the reference network: with bf16 rounding off it reproduces the fixtures
captured from the imported reference's DeformNetwork (tests/golden/deform_mlp*.npz, fp32) for all three variants -- outputs and,
where the fixture holds them, every parameter gradient.  So a bug in the reference cannot hide a bug in a kernel that the
full-size form tests (tests/test_gpu_mlp_forms.py) compare against it.  CPU only."""
import os

import numpy as np
import pytest
import torch

from tests import mlp_reference as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
# fp32 accumulation distance of the fixtures to float64 (measured: outputs 6.8e-7 of scale, is_blender d_scaling; gradients
# 8.4e-7 of scale, is_blender) -- the bf16-rounded network sits 3.0e-3 .. 4.5e-3 of scale away, three orders above
OUT_TOL, GRAD_TOL = 2e-6, 3e-6


@pytest.mark.parametrize("name,is_blender,is_6dof", [("deform_mlp", False, False), ("deform_mlp_blender", True, False),
                                                     ("deform_mlp_6dof", False, True)])
def test_float64_reference_reproduces_golden(name, is_blender, is_6dof):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    params = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w_")}
    assert set(params) == set(R.param_keys(is_blender, is_6dof))
    x, t = torch.from_numpy(d["x"]), torch.from_numpy(d["t"])
    cot = [torch.from_numpy(d[k]) for k in ("gx", "gr", "gs")] if "gx" in d.files else None
    out, grads = R.evaluate(params, x, t, cot, is_blender, is_6dof, bf16=False)
    out_bf, _ = R.evaluate(params, x, t, None, is_blender, is_6dof, bf16=True)
    for key, got, got_bf in zip(("d_xyz", "d_rotation", "d_scaling"), out, out_bf):
        want = d[key].astype(np.float64)
        scale = np.abs(want).max()
        err = np.abs(got.numpy() - want).max()
        print(f"[measured] {name} {key}: float64 reference vs fixture {err / scale:.2e} of scale (bar {OUT_TOL})")
        assert got.shape == want.shape and err <= OUT_TOL * scale, f"{key}: {err:.3e} vs scale {scale:.3e}"
        # the rounding switch does something: the bf16 network is far outside the fp32 bar
        assert np.abs(got_bf.numpy() - want).max() > 100 * OUT_TOL * scale, key
    if cot is None:
        return
    for k, g in grads.items():
        want = d["grad_" + k].astype(np.float64)
        scale = np.abs(want).max()
        err = np.abs(g.numpy() - want).max()
        assert g.shape == want.shape and err <= GRAD_TOL * scale, f"grad {k}: {err:.3e} vs scale {scale:.3e}"


def test_float64_reference_chunking_and_time_layout():
    """Row chunks give the same outputs and gradients as one chunk; a stride-0 time equals the contiguous copy."""
    d = np.load(os.path.join(GOLDEN, "deform_mlp.npz"))
    params = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w_")}
    x = torch.from_numpy(d["x"])
    t0 = torch.tensor([[0.37]]).expand(x.shape[0], -1)
    cot = [torch.from_numpy(d[k]) for k in ("gx", "gr", "gs")]
    a, ga = R.evaluate(params, x, t0, cot, chunk=1 << 17)
    b, gb = R.evaluate(params, x, t0.contiguous(), cot, chunk=17)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for k in ga:
        assert float((ga[k] - gb[k]).abs().max()) <= 1e-12 * float(ga[k].abs().max()), k
