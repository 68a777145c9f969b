"""tests/photometric_reference.py against the imported reference's own numbers (tests/golden/losses.npz: l1_loss, ssim, the
train.py:235-238 combination and its autograd gradient, captured in fp32), and its float64 evaluation against its float32
one.  No GPU."""
import os

import numpy as np
import torch

from tests import photometric_reference as pr

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses.npz"))


def _total_and_grad(dtype):
    x = torch.from_numpy(G["a"]).to(dtype).requires_grad_(True)
    y = torch.from_numpy(G["b"]).to(dtype)
    total = pr.photometric(x, y, 0.2)
    total.backward()
    return float(total.detach()), x.grad.double()


def test_window_is_the_reference_window():
    g = pr.window_1d()
    assert g.dtype == torch.float32 and g.shape == (11,) and torch.equal(g, g.flip(0))
    assert abs(float(g.double().sum()) - 1.0) < 11 * 2.0 ** -24
    w32, w64 = pr.window_2d(3, torch.float32), pr.window_2d(3, torch.float64)
    assert w32.shape == w64.shape == (3, 1, 11, 11)
    # float64: the exact products of the float32 taps (24 x 24 bits fit), float32: each product rounded once
    assert torch.equal(w64[0, 0], g.double()[:, None] * g.double()[None, :])
    assert torch.equal(w32, w64.float())


def test_float32_reference_reproduces_the_fixture():
    """The fixture's existing tolerances (tests/test_gpu_parity.py): 1e-5 absolute on the scalars, 1e-5 of the gradient's
    scale."""
    a, b = torch.from_numpy(G["a"]), torch.from_numpy(G["b"])
    assert abs(float(pr.l1(a, b)) - float(G["l1"])) < 1e-5
    assert abs(float(pr.ssim(a, b)) - float(G["ssim"])) < 1e-5
    total, grad = _total_and_grad(torch.float32)
    assert abs(total - float(G["total"])) < 1e-5
    want = torch.from_numpy(G["grad_a"]).double()
    assert float((grad - want).abs().max()) < 1e-5 * float(want.abs().max())
    # evaluate() hands out the same numbers in parts
    l1, ss, d_l1, d_ss = pr.evaluate(a, b, torch.float32)
    assert abs(l1 - float(G["l1"])) < 1e-5 and abs(ss - float(G["ssim"])) < 1e-5
    assert float((0.8 * d_l1 - 0.2 * d_ss - want).abs().max()) < 1e-5 * float(want.abs().max())


def test_float64_agrees_with_float32_on_the_fixture():
    """On a random image the fp32 composition carries a few roundings of 121-term sums: 1e-6 on the scalars, 1e-5 of the
    gradient's scale is ten times what it needs, and a float64 evaluation that differed in the window, the padding or the
    constants would be off by far more."""
    t32, g32 = _total_and_grad(torch.float32)
    t64, g64 = _total_and_grad(torch.float64)
    assert abs(t32 - t64) < 1e-6
    assert float((g32 - g64).abs().max()) < 1e-5 * float(g64.abs().max())
    assert abs(t64 - float(G["total"])) < 1e-6
    a, b = torch.from_numpy(G["a"]), torch.from_numpy(G["b"])
    l1_32, ss_32, dl_32, ds_32 = pr.evaluate(a, b, torch.float32)
    l1_64, ss_64, dl_64, ds_64 = pr.evaluate(a, b, torch.float64)
    assert abs(l1_32 - l1_64) < 1e-6 and abs(ss_32 - ss_64) < 1e-6
    assert float((dl_32 - dl_64).abs().max()) <= 2.0 ** -23 * float(dl_64.abs().max())    # sign(x - y) / N, rounded once
    assert float((ds_32 - ds_64).abs().max()) < 1e-5 * float(ds_64.abs().max())


def test_identical_images_have_ssim_one_and_no_gradient_in_float64():
    x = torch.rand(2, 13, 9, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    l1, ss, d_l1, d_ss = pr.evaluate(x, x.clone(), torch.float64)
    assert l1 == 0.0 and abs(ss - 1.0) < 1e-14
    assert float(d_l1.abs().max()) == 0.0 and float(d_ss.abs().max()) < 1e-12
