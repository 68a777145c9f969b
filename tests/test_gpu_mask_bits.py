"""The FEATURE-state head on bit-packed SAM masks (trase_amd.feature_head.PackedMasks; trase_amd/csrc/maskbits.hip and the BITS
instantiations of ph_gather_kernel in pairhead.hip).

Everything is tolerance-free.  The stream is ``numpy.packbits(masks.reshape(-1))``; cover counts and mask sizes are integers and
are compared exactly with torch's sums and with the bool-byte kernel; the head is fed the same memberships and runs the same
arithmetic behind them, so its outputs and gradient are compared BITWISE with the bool call (NaN equal to NaN).

Shapes are the smallest at which each mechanism can break: every dimension 1; masks that start in the middle of a byte; an
H * W (561, 2345) that gives every mask another shift, a partial last window and a tail that is no multiple of 4; shift 0
throughout; mask counts around the counter planes' 2^8 step and a cover count above 255; and the workload size once.
Scenes are built once per shape and shared."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = [(1, 1, 1), (3, 3, 2), (14, 17, 33), (14, 35, 67), (9, 16, 24), (255, 5, 13), (256, 5, 13), (257, 5, 13), (300, 7, 9)]
WORKLOAD = (100, 540, 960)
# features (Hr, Wr) on masks (h, w): equal size twice, then the two resized geometries
HEAD_GEOM = [((17, 33), (17, 33)), ((32, 48), (32, 48)), ((67, 35), (33, 17)), ((64, 96), (32, 48))]

_scenes, _heads = {}, {}


def _masks(shape):
    """(masks (N, H, W) bool on the GPU, its numpy.packbits stream): rectangles as in tests/test_gpu_feature_resized.py::_scene,
    plus -- where N allows -- an all-ones mask, an empty mask and a mask whose only set pixel is the last one."""
    if shape not in _scenes:
        N, H, W = shape
        g = torch.Generator(device="cuda").manual_seed(N * 7919 + H * 131 + W)
        yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
        cy, cx = torch.randint(0, H, (N,), device="cuda", generator=g), torch.randint(0, W, (N,), device="cuda", generator=g)
        ry = torch.randint(max(1, H // 10), max(2, H // 3), (N,), device="cuda", generator=g)
        rx = torch.randint(max(1, W // 10), max(2, W // 3), (N,), device="cuda", generator=g)
        m = ((yy[None] - cy[:, None, None]).abs() <= ry[:, None, None]) & ((xx[None] - cx[:, None, None]).abs() <= rx[:, None, None])
        if N >= 3:
            m[N // 2] = True
            m[N - 2] = False
            m[N - 1] = False
            m[N - 1, H - 1, W - 1] = True
        if shape == (300, 7, 9):
            m[:, 3, 4] = True                    # one pixel under all 300 masks: a count above 255
        _scenes[shape] = (m, np.packbits(m.reshape(-1).cpu().numpy()))
    return _scenes[shape]


def _pad16(n):
    return (n + 15) // 16 * 16


def _same(a, b):
    """bitwise, NaN equal to NaN"""
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))


# ---- pack / unpack ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL + [WORKLOAD], ids=str)
def test_round_trip_is_numpy_packbits(shape):
    from trase_amd.feature_head import PackedMasks
    m, stream = _masks(shape)
    keep = m.clone()
    pm = PackedMasks.from_bool(m)
    assert pm.shape == shape and pm.bits.numel() == _pad16(stream.size)
    got = pm.bits.cpu().numpy()
    assert np.array_equal(got[:stream.size], stream)
    assert not got[stream.size:].any()
    back = pm.to_bool()
    assert back.dtype == torch.bool and torch.equal(back, m)
    assert set(back.view(torch.uint8).unique().tolist()) <= {0, 1}
    # any non-zero byte is set: 2 and 255 in a byte tensor
    as_bytes = torch.where(m, torch.where((torch.arange(m.numel(), device="cuda") % 3 == 0).view(m.shape), 2, 255), 0).to(torch.uint8)
    assert torch.equal(PackedMasks.from_bool(as_bytes).bits, pm.bits)
    # the host route gives the same tensor
    saved = PackedMasks.from_saved({"masks": stream, "N": shape[0], "H": shape[1], "W": shape[2]}, "cuda")
    assert torch.equal(saved.bits, pm.bits) and torch.equal(saved.to_bool(), m)
    assert torch.equal(m, keep)


# ---- cover counts and mask sizes -------------------------------------------------------------------------------------------------
def _dirty_variants(shape, stream):
    """the stream with every bit behind N * H * W set: in the last byte and the padding; and the same as a view into a longer
    allocation that goes on with 0xFF"""
    from trase_amd.feature_head import PackedMasks
    N, H, W = shape
    total = N * H * W
    host = np.full(_pad16(stream.size), 0xFF, np.uint8)
    host[:stream.size] = stream
    if total % 8:
        host[stream.size - 1] |= 0xFF >> (total % 8)
    dirty = PackedMasks(torch.from_numpy(host).cuda(), N, H, W)
    long = torch.full((host.size + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    long[:stream.size] = torch.from_numpy(stream).cuda()
    if total % 8:
        long[stream.size - 1] |= 0xFF >> (total % 8)
    return dirty, PackedMasks(long[:host.size], N, H, W)


@pytest.mark.parametrize("shape", SMALL + [WORKLOAD], ids=str)
def test_stats_equal_the_bool_kernel_and_torch(shape):
    from trase_amd.feature_head import PackedMasks, mask_stats
    m, stream = _masks(shape)
    N, H, W = shape
    want_cover = m.sum(0).to(torch.int32)
    want_size = m.flatten(1).sum(1).to(torch.int32)
    if shape == (300, 7, 9):
        assert int(want_cover.max()) == 300
    cover_b, size_b = mask_stats(m)
    clean = PackedMasks.from_saved({"masks": stream, "N": N, "H": H, "W": W}, "cuda")
    dirty, view = _dirty_variants(shape, stream)
    for name, pm in (("clean", clean), ("padding 0xFF", dirty), ("0xFF behind the buffer", view)):
        before = pm.bits.clone()
        cover, size = mask_stats(pm)
        assert cover.dtype == torch.int32 and size.dtype == torch.int32 and cover.shape == (H, W) and size.shape == (N,)
        bad = (cover != want_cover).nonzero()
        assert bad.numel() == 0, f"{name}: {bad.shape[0]} cover counts differ, first at {bad[0].tolist()}: {int(cover[tuple(bad[0])])} != {int(want_cover[tuple(bad[0])])}"
        assert torch.equal(size, want_size), f"{name}: sizes differ at masks {(size != want_size).nonzero().flatten().tolist()[:8]}"
        assert torch.equal(cover, cover_b) and torch.equal(size, size_b), name
        cover2, size2 = mask_stats(pm)
        assert torch.equal(cover2, cover) and torch.equal(size2, size), name
        assert torch.equal(pm.bits, before), name


# ---- the head ----------------------------------------------------------------------------------------------------------------------
def _head_scene(src, dst):
    """(features (32, Hr, Wr), masks (14, h, w) bool, PackedMasks, sampled_pixel, sampled_mask)"""
    key = (src, dst)
    if key not in _heads:
        from trase_amd.feature_head import PackedMasks
        (Hr, Wr), (h, w) = src, dst
        m, stream = _masks((14, h, w))
        g = torch.Generator(device="cuda").manual_seed(Hr * 1000 + w)
        sm = torch.rand(14, device="cuda", generator=g) < 0.5
        sm[1] = True
        sm[13] = True                            # the mask of the last pixel alone is sampled
        base = torch.randn(14, 32, device="cuda", generator=g)
        big = torch.nn.functional.interpolate(m.float()[None], size=(Hr, Wr), mode="nearest")[0]
        feat = (big.permute(1, 2, 0) @ base).permute(2, 0, 1) * 0.5 + 0.8 * torch.randn(32, Hr, Wr, device="cuda", generator=g)
        sp = torch.rand(h, w, device="cuda", generator=g) < min(400, h * w // 3) / (h * w)
        sp[h - 1, w - 1] = True                  # the last pixel: the last bit of every mask
        assert int(sp.sum()) >= 2
        pm = PackedMasks.from_saved({"masks": stream, "N": 14, "H": h, "W": w}, "cuda")
        _heads[key] = (feat, m, pm, sp, sm)
    return _heads[key]


def _run(feat, masks, sp, sm, mode, **kw):
    """(loss_pos, loss_neg, pos_similarity, neg_similarity[, reg], gradient of loss_pos + 0.5 loss_neg [+ 0.3 reg])"""
    from trase_amd.feature_head import contrastive_head
    f = feat.clone().requires_grad_(True)
    out = contrastive_head(f, masks, sp, sm, mode, 0.75, 0.5, **kw)
    loss = out[0] + 0.5 * out[1] + (0.3 * out[4] if len(out) == 5 else 0.0)
    grad, = torch.autograd.grad(loss, f)
    return tuple(o.detach() for o in out) + (grad,)


def _assert_bitwise(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert _same(a, b), f"{what}: output {i} differs ({a.flatten()[:4].tolist()} != {b.flatten()[:4].tolist()})"


@pytest.mark.parametrize("mode", ["soft", "all", "hard"])
@pytest.mark.parametrize("src,dst", HEAD_GEOM, ids=lambda v: "x".join(map(str, v)))
def test_head_on_packed_masks_is_bitwise_the_bool_head(src, dst, mode):
    from trase_amd.feature_head import check_sampled_counts, get_sample_pixel_and_mask
    feat, m, pm, sp, sm = _head_scene(src, dst)
    keep = [t.clone() for t in (feat, m, pm.bits, sp, sm)]
    for reg in (False, True):
        want = _run(feat, m, sp, sm, mode, with_norm_reg=reg)
        assert len(want) == (6 if reg else 5)
        assert torch.isfinite(want[0]) and torch.isfinite(want[1])
        assert mode == "hard" or float(want[-1].abs().sum()) > 0          # (a 'hard' selection may be empty; the others are not)
        got = _run(feat, pm, sp, sm, mode, with_norm_reg=reg)
        _assert_bitwise(got, want, f"{mode} reg={reg}")
        _assert_bitwise(_run(feat, pm, sp, sm, mode, with_norm_reg=reg), got, f"{mode} reg={reg} second call")
    # a draw made FROM the packed masks, on the sync-free path (the tensor carries the draw's count tag)
    torch.manual_seed(11)
    dsp, dsm = get_sample_pixel_and_mask(pm, 200, 7)
    torch.manual_seed(11)
    bsp, bsm = get_sample_pixel_and_mask(m, 200, 7)
    assert torch.equal(dsp, bsp) and torch.equal(dsm, bsm)
    assert dsp._trase_expected_count == (200, dsp.numel(), dsp._version)
    dsm[1] = True
    _assert_bitwise(_run(feat, pm, dsp, dsm, mode, with_norm_reg=True), _run(feat, m, dsp, dsm, mode, with_norm_reg=True), f"{mode} sync-free")
    check_sampled_counts()
    for t, k in zip((feat, m, pm.bits, sp, sm), keep):
        assert torch.equal(t, k)


def test_exclude_keeps_the_draw_sync_free(monkeypatch):
    from trase_amd import feature_head as fh
    src, dst = (67, 35), (33, 17)
    feat, m, pm, _, _ = _head_scene(src, dst)
    h, w = dst
    exclude = torch.zeros(h, w, dtype=torch.bool, device="cuda")
    exclude[:, : w // 2] = True
    cover, sizes = fh.mask_stats(pm)
    torch.manual_seed(5)
    sp0, sm0 = fh.get_sample_pixel_and_mask(pm, 200, 7, cover_count=cover)
    torch.manual_seed(5)
    sp1, sm1 = fh.get_sample_pixel_and_mask(pm, 200, 7, cover_count=cover, exclude=exclude)
    assert torch.equal(sp1, sp0 & ~exclude) and torch.equal(sm1, sm0)
    assert int(sp0.sum()) > int(sp1.sum()) >= 2
    assert sp1._trase_expected_count == (200, h * w, sp1._version)          # the tag survives: target count, this tensor, unedited
    sm1[1] = True

    def no_host_count(*a, **k):
        raise AssertionError("the head fell back to counting the sampled pixels on the host")
    f = feat.clone().requires_grad_(True)
    with monkeypatch.context() as mp:
        mp.setattr(torch, "nonzero", no_host_count)
        out = fh.contrastive_head(f, pm, sp1, sm1, "soft", 0.75, 0.5, mask_size=sizes, with_norm_reg=True)
    grad, = torch.autograd.grad(out[0] + 0.5 * out[1] + 0.3 * out[4], f)
    got = tuple(o.detach() for o in out) + (grad,)
    _assert_bitwise(got, _run(feat, m, sp1, sm1, "soft", with_norm_reg=True), "exclude")
    fh.check_sampled_counts()
