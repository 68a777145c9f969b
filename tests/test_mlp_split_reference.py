"""The split-bf16 arithmetic of ``precision="bf16x3"`` (tests/mlp_split_reference.py) is what it claims to be, and the two C
entry points behind it refuse what they must -- all without a GPU: the refusals come before any device is touched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import mlp_reference as R
from tests import mlp_split_reference as S

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
INVALID = -1            # TRASE_ERR_INVALID


@pytest.mark.parametrize("name,is_blender,is_6dof", [("deform_mlp", False, False), ("deform_mlp_blender", True, False),
                                                     ("deform_mlp_6dof", False, True)])
def test_split_emulation_is_64x_closer_than_bf16(name, is_blender, is_6dof):
    """A condition, not a measurement: hi + lo carries 16 mantissa bits against 8, the reference arithmetic alone gives
    450-700x on the default fixture."""
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    p = R.to_f64({k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w_")})
    x, t = torch.from_numpy(d["x"]), torch.from_numpy(d["t"])
    with torch.no_grad():
        want = R.forward(p, x, t, is_blender, is_6dof, bf16=False)
        bf = R.forward(p, x, t, is_blender, is_6dof, bf16=True)
        for accumulate in ("fp32", "fp64"):
            sp = S.forward(p, x, t, is_blender, is_6dof, accumulate)
            for key, w, b, s in zip(("d_xyz", "d_rotation", "d_scaling"), want, bf, sp):
                e_bf, e_sp = float((b - w).abs().max()), float((s - w).abs().max())
                print(f"[measured] {name} {key} ({accumulate} accumulate): split {e_sp:.2e}, bf16 {e_bf:.2e}, ratio {e_bf / e_sp:.0f}")
                assert s.dtype == torch.float64 and s.shape == w.shape
                assert 64 * e_sp <= e_bf, (key, accumulate, e_sp, e_bf)


def test_split_halves_are_bf16_and_sum_to_sixteen_bits():
    v = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * 3
    hi, lo = S.split(v)
    for h in (hi, lo):
        assert torch.equal(h, h.to(torch.bfloat16).to(torch.float32))
    # bf16 has 8 significant bits: hi is within half an ulp (2^-8 relative), lo = bf16(v - hi) within 2^-8 of |v - hi| <= 2^-8 |v|,
    # plus the fp32 rounding of v itself
    assert float(((hi.double() - v).abs() / v.abs()).max()) <= 2.0 ** -8
    assert float(((hi.double() + lo.double() - v).abs() / v.abs()).max()) <= 2.0 ** -16 + 2.0 ** -24


def _weights(lib_mod, **over):
    w = lib_mod.MlpWeights()
    w.D, w.W, w.xyz_multires, w.t_multires = 8, 256, 10, 10
    w.is_blender = w.is_6dof = w.variant = 0
    fake = 0x1000                      # never dereferenced: every call below is refused before the device is touched
    for i in range(8):
        w.weight[i], w.bias[i] = fake, fake
    w.w_warp = w.b_warp = w.w_rotation = w.b_rotation = w.w_scaling = w.b_scaling = fake
    for k, v in over.items():
        setattr(w, k, v)
    return w


def _call(lib, w, n=8, ws_bytes=None, x=0x1000, t=0x1000, dx=0x1000, dr=0x1000, ds=0x1000, ws=0x1000, t_stride=1):
    if ws_bytes is None:
        b = C.c_size_t()
        assert lib.trase_mlp_split_ws_bytes(C.byref(b)) == 0
        ws_bytes = b.value
    wp = C.byref(w) if w is not None else None
    return lib.trase_mlp_forward_split(wp, x, t, t_stride, n, dx, dr, ds, ws, ws_bytes, 0, None)


def test_split_entry_points_refuse_before_touching_a_device():
    from trase_amd import _lib
    lib = _lib.load()
    assert lib.trase_mlp_split_ws_bytes(None) == INVALID and "null" in _lib.last_error()
    b = C.c_size_t()
    assert lib.trase_mlp_split_ws_bytes(C.byref(b)) == 0
    # the hi and lo streams of all 126 K-steps of weights: 2 x 126 x 256 x 16 bf16
    assert b.value >= 2 * 126 * 256 * 16 * 2
    good = _weights(_lib)
    assert _call(lib, None) == INVALID and "null weights" in _lib.last_error()
    for null in ("x", "t", "dx", "dr", "ds"):
        assert _call(lib, good, **{null: None}) == INVALID, null
        assert "null pointer" in _lib.last_error(), null
    assert _call(lib, _weights(_lib, w_rotation=None)) == INVALID and "null head" in _lib.last_error()
    w = _weights(_lib)
    w.bias[3] = None
    assert _call(lib, w) == INVALID and "null layer 3" in _lib.last_error()
    assert _call(lib, good, n=-1) == INVALID and "bad arguments" in _lib.last_error()
    assert _call(lib, good, ws_bytes=b.value - 1) == INVALID and "workspace too small" in _lib.last_error()
    assert _call(lib, good, ws=None) == INVALID and "workspace too small" in _lib.last_error()
    for over in (dict(D=7), dict(W=128), dict(xyz_multires=6), dict(t_multires=6), dict(is_blender=1), dict(is_6dof=1)):
        assert _call(lib, _weights(_lib, **over)) == INVALID, over      # (is_blender needs t_multires 6)
        assert "is compiled in" in _lib.last_error(), over
    assert _call(lib, _weights(_lib, variant=1)) == INVALID and "variant" in _lib.last_error()
    assert _call(lib, _weights(_lib, is_blender=1, t_multires=6), t_stride=1) == INVALID and "t_stride" in _lib.last_error()
    # N == 0: nothing to do, nothing launched (there is no device here to launch on), null data pointers are fine
    assert _call(lib, good, n=0, x=None, t=None, dx=None, dr=None, ds=None, ws=None, ws_bytes=0) == 0


def test_precision_is_validated_before_the_device():
    from trase_amd.deform import DeformNetworkHIP, deform_forward
    from trase_amd.synthetic import SynthDeformNetwork
    x, t = torch.zeros(4, 3), torch.zeros(4, 1)           # CPU tensors: the device check would raise RuntimeError
    with pytest.raises(ValueError, match="precision"):
        deform_forward({}, x, t, precision="fp32")
    with pytest.raises(ValueError, match="precision"):
        DeformNetworkHIP(SynthDeformNetwork(), precision="bf16x2")
    assert DeformNetworkHIP(SynthDeformNetwork()).precision == "bf16"
    assert DeformNetworkHIP(SynthDeformNetwork(), precision="bf16x3").precision == "bf16x3"
    with pytest.raises(RuntimeError, match="GPU only"):
        deform_forward({}, x, t, precision="bf16x3")
