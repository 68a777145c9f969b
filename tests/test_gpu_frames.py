"""The GAUSSIAN-state loss on 8-bit ground truth (trase_amd.frames.ByteFrame; trase_amd/csrc/frames.hip and the GtBytes
instantiations of the loss kernels in loss.hip).

Nothing here uses a tolerance.  The planes hold the uploaded bytes; ``to_float`` is the reference's
``torch.from_numpy(bytes) / 255.0``; the composite is compared byte for byte with the numpy statement
(tests/frames_reference.py, itself checked against the reference's expressions without a GPU); the loss on bytes runs the
float kernels' bodies on the same values and is compared with ``torch.equal`` -- loss, both parts and the gradient -- against
the float entry points on ``frame.to_float()``; ``mask_black`` against the float head on the reference's blend, differentiated
through the blend by autograd.

Sizes (H x W): the smallest at which each mechanism can go wrong -- one pixel; sizes below, at and just above the 32 x 32 tile
and off the 16-byte pitch; 96 x 960 (270 blocks: the masked rows of the reduction's unroll); 1 x 21857 (2052 blocks: the
reduction's second trip); 1080 x 1920 once.  Scenes are built once per (size, content) and shared."""
import os

import numpy as np
import pytest
import torch

from tests import frames_reference as fr

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 7), (10, 11), (32, 32), (64, 31), (33, 65), (40, 40), (96, 960), (1, 21857)]
FULL = (1080, 1920)
KINDS = ["random", "black", "patches", "two_zero", "identical"]
RESIZES = [((66, 34), (33, 17)), ((67, 35), (20, 13)), ((10, 11), (32, 32)), ((66, 34), (66, 34)), ((10, 11), (10, 11))]
BACKGROUNDS = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.2, 0.5, 0.7)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames.npz")

_scenes = {}


def _bytes_for(size, kind):
    """(H, W, 3) uint8"""
    H, W = size
    g = np.random.default_rng(H * 1009 + W * 7 + KINDS.index(kind))
    hwc = g.integers(1 if kind != "random" else 0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "black":
        hwc[:] = 0
    elif kind in ("patches", "identical"):
        # black rectangles across the 32-pixel tile edges, reaching into the neighbouring tiles' 5-pixel halo, and at the borders
        for y0 in (0, 28, H - 2):
            for x0 in (0, 27, 61, W - 4):
                hwc[max(y0, 0):max(y0, 0) + 9, max(x0, 0):max(x0, 0) + 11] = 0
    elif kind == "two_zero":
        hwc[..., 0] = 0
        hwc[..., 1] = 0                              # zero in two channels, at least 1 in the third: not black
        hwc[H // 2:, W // 2:, 2] = 0                 # ... and a quadrant that is
        hwc[0, 0] = (0, 0, 0)
    return hwc


def _scene(size, kind):
    """(hwc bytes, ByteFrame, its fp32 frame, the rendered image) -- built once, never modified"""
    from trase_amd.frames import ByteFrame
    key = (size, kind)
    if key not in _scenes:
        hwc = _bytes_for(size, kind)
        frame = ByteFrame.from_array(hwc, device="cuda")
        gt = frame.to_float()
        if kind == "identical":
            img = gt.clone()
        else:
            g = torch.Generator(device="cuda").manual_seed(size[0] * 31 + size[1])
            img = torch.rand(gt.shape, device="cuda", generator=g)
        _scenes[key] = (hwc, frame, gt, img)
    return _scenes[key]


def _photometric(img, gt, **kw):
    from trase_amd.losses import photometric_loss
    x = img.clone().requires_grad_(True)
    loss, l1, ss = photometric_loss(x, gt, 0.2, with_parts=True, **kw)
    loss.backward()
    return loss.detach(), l1, ss, x.grad


def _l1_ssim(img, gt, cot, **kw):
    from trase_amd.losses import l1_ssim
    x = img.clone().requires_grad_(True)
    l1, ss = l1_ssim(x, gt, **kw)
    (cot[0] * l1 + cot[1] * ss).backward()
    return l1.detach(), ss.detach(), x.grad


def _assert_equal(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a, b), f"{what}: output {i} differs"
    assert len(got) == len(want)


def _cases():
    return [pytest.param(s, k, id=f"{s[0]}x{s[1]}-{k}") for s in SIZES for k in KINDS] + [pytest.param(FULL, "patches", id="1080x1920-patches")]


# ---- pack / unpack -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES + [FULL], ids=str)
def test_pack_and_unpack_are_the_bytes_and_their_quotient(size):
    from trase_amd.frames import ByteFrame
    H, W = size
    rgb = _bytes_for(size, "random")
    rgba = np.concatenate([rgb, np.random.default_rng(5).integers(0, 256, (H, W, 1), dtype=np.uint8)], axis=2)
    want = (torch.from_numpy(rgb).permute(2, 0, 1) / 255.0).cuda()
    want_planes = torch.from_numpy(fr.planes(rgb)).cuda()
    for hwc in (rgb, rgba):
        for source in (hwc, torch.from_numpy(hwc), torch.from_numpy(hwc).cuda()):
            frame = ByteFrame.from_array(source, device="cuda")
            assert frame.shape == (3, H, W) and frame.pitch == fr.pitch_for(W) and frame.data.is_cuda
            assert torch.equal(frame.data, want_planes)                       # the padding is written as 0
            got = frame.to_float()
            assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got, want)
    back = ByteFrame.from_float(want)
    assert torch.equal(back.data, want_planes)
    with pytest.raises(ValueError, match="k / 255"):
        ByteFrame.from_float(want * 0.999 + 0.0001)


def test_every_byte_value_is_the_exact_quotient():
    from trase_amd.frames import ByteFrame
    b = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    got = ByteFrame.from_array(b, device="cuda").to_float()
    assert torch.equal(got.cpu(), torch.from_numpy(fr.to_float(b).transpose(2, 0, 1).copy()))


# ---- the composite -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg", BACKGROUNDS, ids=str)
def test_from_rgba_is_the_numpy_composite(bg):
    from trase_amd.frames import ByteFrame
    from tests.test_frames_reference import table_image
    for rgba in (table_image(), np.load(GOLDEN)["rgba"]):
        want = torch.from_numpy(fr.planes(fr.composite(rgba, bg)))
        for background in (torch.tensor(bg, dtype=torch.float32, device="cuda"), np.array(bg, dtype=np.float32), bg):
            frame = ByteFrame.from_rgba(rgba, background, device="cuda")
            assert torch.equal(frame.data.cpu(), want)
        assert torch.equal(ByteFrame.from_rgba(torch.from_numpy(rgba).cuda(), bg).data.cpu(), want)


@pytest.mark.parametrize("bg", ["bg0", "bg1"])
def test_golden_frame_through_the_device(bg):
    from trase_amd.frames import ByteFrame
    z = np.load(GOLDEN)
    frame = ByteFrame.from_rgba(z["rgba"], [float(bg[-1])] * 3, device="cuda")
    assert torch.equal(frame.to_float().cpu(), torch.from_numpy(z[f"frame_{bg}"][:3]))
    assert torch.equal(ByteFrame.from_array(z[f"bytes_{bg}"], device="cuda").data, frame.data)


# ---- the loss on bytes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,kind", _cases())
def test_loss_on_bytes_is_the_loss_on_floats(size, kind):
    _, frame, gt, img = _scene(size, kind)
    want = _photometric(img, gt)
    got = _photometric(img, frame)
    assert torch.isfinite(want[0]) and torch.isfinite(want[3]).all()
    if kind == "identical":
        assert float(want[1]) == 0.0
    _assert_equal(got, want, "photometric_loss")
    _assert_equal(_photometric(img, frame), got, "photometric_loss, second call")
    for cot in ((0.8, -0.2), (0.0, 1.0)):
        _assert_equal(_l1_ssim(img, frame, cot), _l1_ssim(img, gt, cot), f"l1_ssim {cot}")


@pytest.mark.parametrize("size,kind", _cases())
def test_mask_black_is_the_reference_blend(size, kind):
    from trase_amd.losses import l1_ssim, photometric_loss
    _, frame, gt, img = _scene(size, kind)
    bm = (torch.sum(gt, dim=0) == 0).float()                                   # train.py:232-233
    if kind in ("black", "patches", "two_zero"):
        assert float(bm.sum()) > 0
    if kind == "two_zero":
        assert float(bm.sum()) < bm.numel() or size == (1, 1)

    x = img.clone().requires_grad_(True)
    loss, l1, ss = photometric_loss(x * (1 - bm) + gt * bm, gt, 0.2, with_parts=True)      # train.py:234-238 on the float head
    loss.backward()
    want = (loss.detach(), l1, ss, x.grad)
    got = _photometric(img, frame, mask_black=True)
    _assert_equal(got, want, "photometric_loss(mask_black=True)")
    assert not got[3][:, bm.bool()].any()
    _assert_equal(_photometric(img, frame, mask_black=True), got, "mask_black, second call")

    x = img.clone().requires_grad_(True)
    l1, ss = l1_ssim(x * (1 - bm) + gt * bm, gt)
    (0.8 * l1 - 0.2 * ss).backward()
    _assert_equal(_l1_ssim(img, frame, (0.8, -0.2), mask_black=True), (l1.detach(), ss.detach(), x.grad), "l1_ssim(mask_black=True)")


def test_mask_black_ignores_a_non_finite_render_at_a_black_pixel():
    _, frame, gt, img = _scene((33, 65), "patches")
    bad = img.clone()
    black = torch.sum(gt, dim=0) == 0
    bad[:, black] = float("nan")
    bad[0, 30, 29] = float("inf")                                                # (28..36, 27..37 is black)
    assert bool(black[30, 29])
    _assert_equal(_photometric(bad, frame, mask_black=True), _photometric(img, frame, mask_black=True), "non-finite under the mask")


# ---- the padding is never looked at ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(5, 7), (10, 11), (64, 31), (33, 65), (1, 21857)], ids=str)
def test_padding_and_what_follows_the_buffer_are_ignored(size):
    from trase_amd.frames import ByteFrame
    H, W = size
    hwc, frame, gt, img = _scene(size, "patches")
    n = frame.nbytes
    store = torch.full((n + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    assert store.data_ptr() % 16 == 0
    store[:n] = torch.from_numpy(fr.planes(hwc, fill=0xFF)).cuda()
    dirty = ByteFrame(store[:n], H, W)
    assert frame.pitch > W and int((dirty.data != frame.data).sum()) == 3 * H * (frame.pitch - W)
    assert torch.equal(dirty.to_float(), gt)
    assert torch.equal(dirty.black_mask(), frame.black_mask())
    small = (max(1, H // 2), max(1, (W + 1) // 3))
    assert torch.equal(dirty.black_mask(small), frame.black_mask(small))
    for kw in ({}, {"mask_black": True}):
        _assert_equal(_photometric(img, dirty, **kw), _photometric(img, frame, **kw), f"dirty padding {kw}")
    assert bool((store[n:] == 0xFF).all())


# ---- black_mask ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", RESIZES, ids=str)
def test_black_mask_is_the_torch_expression(src, dst):
    from trase_amd.frames import ByteFrame
    from tests.test_frames_reference import _patchy
    chw = _patchy(*src, seed=src[0] * 100 + dst[1])
    frame = ByteFrame.from_array(np.ascontiguousarray(chw.transpose(1, 2, 0)), device="cuda")
    gt = frame.to_float()
    full = frame.black_mask()
    assert full.dtype == torch.bool and torch.equal(full, torch.sum(gt, dim=0) == 0)
    resized = torch.nn.functional.interpolate(gt.unsqueeze(0), dst, mode="bilinear").squeeze(0)      # train.py:267
    want = torch.sum(resized, dim=0) == 0
    got = frame.black_mask(dst)
    assert got.shape == dst and got.dtype == torch.bool and torch.equal(got, want)
    assert torch.equal(got.cpu(), torch.from_numpy(fr.black_mask(chw, dst)))
    assert 0 < int(want.sum()) < want.numel()


@pytest.mark.parametrize("size,kind", [pytest.param(s, k, id=f"{s[0]}x{s[1]}-{k}") for s in SIZES for k in ("patches", "two_zero", "black")] +
                         [pytest.param(FULL, "patches", id="1080x1920-patches")])
def test_black_mask_at_frame_size(size, kind):
    _, frame, gt, _ = _scene(size, kind)
    assert torch.equal(frame.black_mask(), torch.sum(gt, dim=0) == 0)


def test_black_mask_keeps_the_draw_sync_free(monkeypatch):
    from trase_amd import feature_head as fh
    from trase_amd.frames import ByteFrame
    from tests.test_frames_reference import _patchy
    src, (h, w) = (67, 35), (20, 13)
    frame = ByteFrame.from_array(np.ascontiguousarray(_patchy(*src, seed=3).transpose(1, 2, 0)), device="cuda")
    exclude = frame.black_mask((h, w))
    g = torch.Generator(device="cuda").manual_seed(2)
    masks = torch.rand((6, h, w), device="cuda", generator=g) < 0.4
    masks[0] = True
    packed = fh.PackedMasks.from_bool(masks)
    cover, _ = fh.mask_stats(packed)
    torch.manual_seed(5)
    sp0, sm0 = fh.get_sample_pixel_and_mask(packed, 60, 4, cover_count=cover)
    torch.manual_seed(5)

    def no_host_count(*a, **k):
        raise AssertionError("the draw counted its pixels on the host")
    with monkeypatch.context() as mp:
        mp.setattr(torch, "nonzero", no_host_count)
        sp1, sm1 = fh.get_sample_pixel_and_mask(packed, 60, 4, cover_count=cover, exclude=exclude)
    assert torch.equal(sp1, sp0 & ~exclude) and torch.equal(sm1, sm0)
    assert int(sp0.sum()) > int(sp1.sum()) >= 1
    assert sp1._trase_expected_count == (60, h * w, sp1._version)          # the tag survives: the head stays on its sync-free path


# ---- reproducibility and the l1_loss / ssim pair ---------------------------------------------------------------------------------------------
def test_l1_loss_then_ssim_evaluate_the_fused_pair_once(monkeypatch):
    from trase_amd import losses
    _, frame, gt, img = _scene((33, 65), "patches")
    want = _l1_ssim(img, gt, (0.8, -0.2))                                        # (before the counter is installed)
    calls = []
    real = losses.l1_ssim

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(losses, "l1_ssim", counting)
    x = img.clone().requires_grad_(True)
    l1 = losses.l1_loss(x, frame)
    ss = losses.ssim(x, frame)
    assert len(calls) == 1
    (0.8 * l1 - 0.2 * ss).backward()
    _assert_equal((l1.detach(), ss.detach(), x.grad), want, "l1_loss + ssim on a ByteFrame")
    losses.l1_loss(x, frame)                                                    # after the backward the pair is evaluated afresh
    assert len(calls) == 2


def test_the_scenes_were_not_modified():
    for (size, kind), (hwc, frame, gt, img) in _scenes.items():
        assert np.array_equal(hwc, _bytes_for(size, kind))
        assert torch.equal(frame.data.cpu(), torch.from_numpy(fr.planes(hwc)))
