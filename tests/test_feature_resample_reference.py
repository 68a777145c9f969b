"""CPU checks of the resize restatement the resized FEATURE-state head is tested against (tests/feature_resample_reference.py):
the float64 blend from ATen's fp32 coordinates against CPU ``F.interpolate``, the gather-form adjoint (the form of the HIP
backward) against autograd's scatter form, and what the new entry points refuse before they touch a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import feature_resample_reference as fr

RESIZE_BOUND = 8 * 2.0 ** -24                       # of max|v|: the bar of tests/test_gpu_trajectory.py
INVALID = -1                                        # TRASE_ERR_INVALID
# (render Hr, Wr) -> (masks h, w): --downsample_mask 4 of an odd frame, a non-integral half, masks larger than the render, both axes
# shrinking by different ratios, an exact half, equal sizes, a tiny frame
SHAPES = [((1014, 1352), (253, 338)), ((67, 35), (33, 17)), ((48, 64), (80, 100)), ((48, 64), (31, 17)), ((270, 480), (135, 240)),
          ((35, 67), (35, 67)), ((5, 7), (3, 2))]
_ids = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SHAPES]


@pytest.mark.parametrize("src,dst", SHAPES, ids=_ids)
def test_restatement_equals_cpu_interpolate(src, dst):
    g = torch.Generator().manual_seed(src[0] * 7 + dst[1])
    f = torch.randn(3, *src, generator=g)
    want = torch.nn.functional.interpolate(f[None], size=dst, mode="bilinear", align_corners=False)[0].double()
    scale = float(f.abs().max())
    err = float((fr.resample64(f, dst) - want).abs().max()) / scale
    loose = float((fr.resample64(f, dst, fused=False) - want).abs().max()) / scale
    print(f"{src} -> {dst}: fused {err:.3e}, unfused {loose:.3e}, bound {RESIZE_BOUND:.3e}")
    assert err <= RESIZE_BOUND
    if src == dst:
        assert err == 0.0
    if (src, dst) == ((48, 64), (80, 100)):
        assert loose > RESIZE_BOUND                 # a product rounded before the subtraction is told apart here


@pytest.mark.parametrize("src,dst", SHAPES, ids=_ids)
def test_gather_adjoint_equals_autograd(src, dst):
    """Every destination sampled, and a 5 % sample: upsampling gives a source pixel more than four contributors, and where
    the masks are at least as large as the render the last row and column are clamped (both taps on one pixel)."""
    gen = torch.Generator().manual_seed(dst[0] * 13 + src[1])
    ch = 2
    for rate in (1.0, 0.05):
        sampled = torch.rand(*dst, generator=gen) < rate
        if not bool(sampled.any()):
            sampled[dst[0] - 1, dst[1] - 1] = True
        cot = torch.randn(ch, *dst, generator=gen, dtype=torch.float64) * sampled
        f = torch.zeros(ch, *src, dtype=torch.float64, requires_grad=True)
        (fr.resample64(f, dst) * cot).sum().backward()
        got = fr.adjoint_gather(cot.numpy(), src, sampled.numpy())
        assert float(np.abs(got - f.grad.numpy()).max()) <= 1e-12 * max(1.0, float(f.grad.abs().max()))
    first, count = fr.first_count(src[0], dst[0])
    assert int(count.sum()) == dst[0] and int(first[0]) == 0
    if dst[0] > src[0]:
        assert int(count.max()) >= 2                                        # more than four contributors per source pixel
    if dst[0] >= src[0] and dst != src:
        i0, i1, _, l1 = fr.axis_table(src[0], dst[0])
        assert i0[-1] == i1[-1] == src[0] - 1 and l1[-1] > 0                # the clamped edge carries both weights


def test_new_entry_points_refuse_bad_arguments_without_gpu():
    from trase_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(256)           # a non-null pointer that is never dereferenced: every call below returns before the GPU
    nb = C.c_size_t()
    sizes = lib.trase_pairhead_sizes_resized
    assert sizes(5000, 1080, 1920, 270, 480, C.byref(nb)) == 0
    plain = C.c_size_t()
    assert lib.trase_pairhead_sizes(5000, C.byref(plain)) == 0
    extra = 5000 * 32 * 4 + 270 * 480 * 4 + 2 * (1080 + 1920) * 4            # v, the slot map, the four tables
    assert plain.value + extra <= nb.value <= plain.value + extra + 6 * 256   # each array starts on a 256-byte boundary
    assert sizes(5000, 1080, 1920, 270, 480, None) == INVALID and b"null pointer" in lib.trase_last_error()
    for bad in ((0, 8, 8, 4, 4), (5, 0, 8, 4, 4), (5, 8, 0, 4, 4), (5, 8, 8, 0, 4), (5, 8, 8, 4, 0), (5, -3, 8, 4, 4),
                (5, 65536, 32768, 4, 4), (5, 8, 8, 65536, 32768)):
        assert sizes(*bad, C.byref(nb)) == INVALID, bad
    assert b"2^31" in lib.trase_last_error()

    fwd = lib.trase_pairhead_forward_resized
    good = dict(feats=one, F=32, Hr=8, Wr=12, h=4, w=6, masks=one, N=3, sampled=one, ns=3, size=one, pix=one, S=5, S_dev=None, mode=0,
                pth=0.75, nth=0.5, use_w=1, out8=one, ws=one, ws_bytes=1 << 30)
    order = tuple(good)
    for change in (dict(feats=None), dict(masks=None), dict(sampled=None), dict(size=None), dict(pix=None), dict(out8=None),
                   dict(F=16), dict(F=0), dict(Hr=0), dict(Wr=0), dict(h=0), dict(w=0), dict(S=0), dict(N=0), dict(N=8193), dict(mode=3),
                   dict(ns=257), dict(Hr=65536, Wr=32768), dict(h=65536, w=32768)):
        a = dict(good, **change)
        assert fwd(*[a[k] for k in order], 0, None) == INVALID, change
    assert fwd(*[dict(good, feats=None)[k] for k in order], 0, None) == INVALID and b"null pointer" in lib.trase_last_error()
    assert fwd(*[dict(good, F=16)[k] for k in order], 0, None) == INVALID and b"16 feature channels" in lib.trase_last_error()

    bwd = lib.trase_pairhead_backward_resized
    good = dict(F=32, Hr=8, Wr=12, h=4, w=6, pix=one, S=5, S_dev=None, mode=0, pth=0.75, nth=0.5, use_w=1, out8=one, g2=one, ws=one,
                ws_bytes=1 << 30, feats=None, out2=None, g_reg=None, d=one)
    order = tuple(good)
    for change in (dict(pix=None), dict(out8=None), dict(g2=None), dict(d=None), dict(F=31), dict(Hr=0), dict(Wr=-1), dict(h=0),
                   dict(w=0), dict(S=0), dict(mode=-1), dict(Hr=65536, Wr=32768),
                   dict(feats=one), dict(feats=one, out2=one), dict(g_reg=one)):          # the regulariser's inputs come together
        a = dict(good, **change)
        assert bwd(*[a[k] for k in order], 0, None) == INVALID, change
    assert b"together" in lib.trase_last_error()

    cols = lib.trase_pairhead_columns_resized
    for args in ((None, 32, 8, 12, 4, 6, one, 5, one), (one, 32, 8, 12, 4, 6, None, 5, one), (one, 32, 8, 12, 4, 6, one, 5, None),
                 (one, 8, 8, 12, 4, 6, one, 5, one), (one, 32, 0, 12, 4, 6, one, 5, one), (one, 32, 8, 12, 4, 0, one, 5, one),
                 (one, 32, 8, 12, 4, 6, one, 0, one)):
        assert cols(*args, 0, None) == INVALID, args


def test_python_entry_points_refuse_cpu_tensors_and_bad_shapes():
    from trase_amd.feature_head import contrastive_head, resized_columns
    with pytest.raises(RuntimeError, match="GPU only"):
        resized_columns(torch.zeros(32, 8, 12), (4, 6), torch.ones(4, 6, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="GPU only"):
        contrastive_head(torch.zeros(32, 8, 12), torch.ones(3, 4, 6, dtype=torch.bool), torch.ones(4, 6, dtype=torch.bool),
                         torch.ones(3, dtype=torch.bool))
