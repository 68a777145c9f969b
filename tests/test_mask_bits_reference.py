"""The packed SAM-mask stream without a GPU: the host side of ``trase_amd.feature_head.PackedMasks`` against ``numpy.packbits``
(the independent statement of the reference's format, extract_masks.py:91-99), the argument refusals of every C entry point
that takes a stream, and the ``exclude=`` shape check of the sampler.  No device is touched: every refused call returns before
it selects one."""
import ctypes as C

import numpy as np
import pytest
import torch

INVALID = -1          # TRASE_ERR_INVALID (include/trase_rast.h)


class _SavedBits:
    """Stands in for the ``bitarray`` of the reference's saved dict: ``tobytes()`` and ``endian()`` only."""

    def __init__(self, flags, endian):
        self._bytes = np.packbits(np.asarray(flags, dtype=np.uint8).reshape(-1), bitorder=endian).tobytes()
        self._endian = endian

    def tobytes(self):
        return self._bytes

    def endian(self):
        return self._endian

    def tolist(self):
        raise AssertionError("the stream must never become a Python list")


def _flags(N, H, W, seed):
    rng = np.random.default_rng(seed)
    m = rng.random((N, H, W)) < 0.4
    m[0] = True
    m[-1] = False
    m[-1, -1, -1] = True          # the last stream bit
    return m


# 18 bits; 14 * 561 = 7854 bits (not a multiple of 8); 32 bits (a whole number of bytes); 16 * 8 * 8 = one whole padded buffer
SHAPES = [(3, 3, 2), (14, 17, 33), (2, 4, 4), (16, 8, 8), (1, 1, 1)]


@pytest.mark.parametrize("endian", ["big", "little"])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_stream_is_numpy_packbits(shape, endian):
    from trase_amd.feature_head import PackedMasks
    N, H, W = shape
    m = _flags(N, H, W, seed=N * 100 + W)
    want = np.packbits(m.reshape(-1))
    buf, n, h, w = PackedMasks.host_stream({"masks": _SavedBits(m, endian), "N": N, "H": H, "W": W})
    assert (n, h, w) == shape
    assert buf.dtype == np.uint8 and buf.ndim == 1
    assert buf.size % 16 == 0 and buf.size >= want.size and buf.size - want.size < 16
    assert np.array_equal(buf[:want.size], want)
    assert not buf[want.size:].any()


def test_host_stream_takes_bytes_arrays_and_tensors():
    from trase_amd.feature_head import PackedMasks
    N, H, W = 5, 7, 9
    m = _flags(N, H, W, seed=3)
    want = np.packbits(m.reshape(-1))
    for raw in (want.tobytes(), bytearray(want.tobytes()), want, torch.from_numpy(want.copy()),
                np.concatenate([want, np.full(5, 0xFF, np.uint8)])):          # a longer stream: only ceil(N H W / 8) bytes are taken
        buf, *_ = PackedMasks.host_stream({"masks": raw, "N": N, "H": H, "W": W})
        assert np.array_equal(buf[:want.size], want) and not buf[want.size:].any() and buf.size % 16 == 0
    with pytest.raises(ValueError, match="stream bytes"):
        PackedMasks.host_stream({"masks": want.tobytes()[:-1], "N": N, "H": H, "W": W})
    with pytest.raises(ValueError):
        PackedMasks.host_stream({"masks": [True, False], "N": 1, "H": 1, "W": 2})


def test_from_saved_builds_the_padded_tensor_on_the_host_device():
    from trase_amd.feature_head import PackedMasks
    N, H, W = 3, 3, 2
    m = _flags(N, H, W, seed=1)
    pm = PackedMasks.from_saved({"masks": _SavedBits(m, "little"), "N": N, "H": H, "W": W}, device="cpu")
    assert pm.shape == (N, H, W) and (pm.N, pm.H, pm.W) == (N, H, W)
    assert pm.bits.dtype == torch.uint8 and pm.bits.numel() == 16
    assert np.array_equal(pm.bits.numpy()[:3], np.packbits(m.reshape(-1))) and not pm.bits.numpy()[3:].any()


def test_packed_masks_refuses_unusable_buffers():
    from trase_amd.feature_head import PackedMasks
    ok = torch.zeros(32, dtype=torch.uint8)
    PackedMasks(ok, 2, 8, 16)
    for bits, why in ((torch.zeros(24, dtype=torch.uint8), "multiple of 16"), (torch.zeros(16, dtype=torch.uint8), "multiple of 16"),
                      (torch.zeros(32, dtype=torch.int32), "uint8"), (torch.zeros(64, dtype=torch.uint8)[::2], "contiguous"),
                      (torch.zeros(48, dtype=torch.uint8)[1:33], "16-byte boundary")):
        with pytest.raises(ValueError, match=why):          # 2 x 8 x 16 bits need 32 bytes
            PackedMasks(bits, 2, 8, 16)
    with pytest.raises(ValueError):
        PackedMasks(ok, 0, 8, 16)


# ---- argument refusals of the C entry points ---------------------------------------------------------------------------------
_N, _HW = 14, 561                      # 7854 bits -> 982 bytes -> a 992-byte buffer
_BYTES = 992
_store = np.zeros(_BYTES + 64, dtype=np.uint8)
_BASE = (_store.ctypes.data + 15) // 16 * 16          # a 16-byte aligned host address: nothing dereferences it in a refused call
_P = _BASE + 16                                       # any other non-null pointer


def _head_args(resized):
    geom = [("F", 32), ("Hr", 34), ("Wr", 66), ("h", 17), ("w", 33)] if resized else [("F", 32), ("HW", _HW)]
    return ([("feats", _P)] + geom +
            [("bits", _BASE), ("bits_bytes", _BYTES), ("N", _N), ("sampled_mask", _P), ("n_sampled", _N), ("mask_size", _P), ("pix", _P),
             ("S", 10), ("S_dev", None), ("mode", 0), ("pth", 0.75), ("nth", 0.5), ("use_w", 1), ("out8", _P), ("ws", _P),
             ("ws_bytes", 1 << 30), ("device", 0), ("stream", None)])


ENTRY_POINTS = {
    "trase_mask_stats_bits": [("bits", _BASE), ("bits_bytes", _BYTES), ("N", _N), ("HW", _HW), ("cover", _P), ("size", _P), ("device", 0),
                              ("stream", None)],
    "trase_pack_masks": [("masks", _P), ("N", _N), ("HW", _HW), ("bits", _BASE), ("bits_bytes", _BYTES), ("device", 0), ("stream", None)],
    "trase_unpack_masks": [("bits", _BASE), ("bits_bytes", _BYTES), ("N", _N), ("HW", _HW), ("masks", _P), ("device", 0), ("stream", None)],
    "trase_pairhead_forward_bits": _head_args(False),
    "trase_pairhead_forward_bits_resized": _head_args(True),
}
_POINTERS = {"bits", "cover", "size", "masks", "feats", "sampled_mask", "mask_size", "pix", "out8"}


def _refusals(name):
    """(description, argument overrides) of every call the entry point must refuse"""
    names = [k for k, _ in ENTRY_POINTS[name]]
    cases = [(f"null {k}", {k: None}) for k in names if k in _POINTERS]
    cases += [("misaligned stream", {"bits": _BASE + 4}), ("misaligned stream by one", {"bits": _BASE + 1}),
              ("bits_bytes too short", {"bits_bytes": 976}),          # a multiple of 16 below ceil(7854 / 8) = 982
              ("bits_bytes no multiple of 16", {"bits_bytes": 984}),  # >= 982 but 984 % 16 == 8
              ("bits_bytes zero", {"bits_bytes": 0}), ("N = 0", {"N": 0}), ("N = 8193", {"N": 8193, "bits_bytes": 1 << 20})]
    if "HW" in names:
        cases.append(("HW = 0", {"HW": 0}))
    else:
        cases += [("h = 0", {"h": 0}), ("w = 0", {"w": 0})]
    return cases


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_points_refuse_bad_arguments(name):
    from trase_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, name)
    assert len(ENTRY_POINTS[name]) == len(fn.argtypes)
    seen = 0
    for what, over in _refusals(name):
        args = [over.get(k, v) for k, v in ENTRY_POINTS[name]]
        rc = fn(*args)
        msg = lib.trase_last_error().decode()
        assert rc == INVALID, f"{name} ({what}): returned {rc}, {msg!r}"
        assert name + ":" in msg, f"{name} ({what}): the message {msg!r} does not name the function"
        seen += 1
    assert seen >= 9


def test_no_new_function_is_a_sizes_function():
    assert not [n for n in ENTRY_POINTS if n.endswith("_sizes")]


# ---- the sampler's exclude= -----------------------------------------------------------------------------------------------------
def test_exclude_shape_mismatch_raises():
    from trase_amd.feature_head import PackedMasks, get_sample_pixel_and_mask
    masks = torch.zeros(3, 4, 5, dtype=torch.bool)
    cover = torch.ones(4, 5, dtype=torch.int32)
    for bad in (torch.zeros(5, 4, dtype=torch.bool), torch.zeros(20, dtype=torch.bool), torch.zeros(1, 4, 5, dtype=torch.bool)):
        with pytest.raises(ValueError, match="exclude"):
            get_sample_pixel_and_mask(masks, 10, 2, cover_count=cover, exclude=bad)
    packed = PackedMasks(torch.zeros(16, dtype=torch.uint8), 3, 4, 5)
    with pytest.raises(ValueError, match="exclude"):
        get_sample_pixel_and_mask(packed, 10, 2, cover_count=cover, exclude=torch.zeros(5, 4, dtype=torch.bool))
