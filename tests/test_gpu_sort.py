"""The radix sort, the tile ranges and the zero fill of trase_amd/csrc/binning.hip, called directly through their test entry
points (trase_selftest_sort / _tile_ranges / _zero_bytes) and compared exactly with numpy (tests/sort_reference.py).  Integer
algorithms: every comparison is array_equal, no tolerance anywhere.

Sort cases (tests/sort_reference.py: SIZES x CONFIGS x FAMILIES x modes_for): the sizes either side of a wave round (64), a wave
segment (512), a workgroup tile (2048) and the short sort's limit (32768), a count far below the capacity, an empty sort; 8-bit
and 9-bit digits with full and partial last digits and bits outside the field; iota and caller-supplied values; the input in
either ping-pong buffer; the default histogram count and one histogram (which sends a multi-pass sort of any size down the
three-launch passes).  Every case asserts which of the two paths ran."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import sort_child as child
from tests import sort_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the sort ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap", R.SIZES, ids=[f"n{n}-cap{cap}" for n, cap in R.SIZES])
def test_sort_equals_stable_reference(n, cap):
    tally = child.run_size(n, cap)
    print(f"cases per (path, digit bits) at n={n} cap={cap}:", dict(tally))
    paths = {p for p, _ in tally}
    assert paths == ({"three-launch"} if R.rs_blocks(cap) > R.RS_SMALL_NB else {"short", "three-launch"})
    assert {db for _, db in tally} == {8, 9}


def test_scan_long_branch():
    """More than 8192 workgroups: every thread of radix_scan_kernel owns more than 32 of them (its serial branch)."""
    from trase_amd.rasterizer import selftest_sort
    n = 8193 * 2048 - 7
    assert (R.rs_blocks(n) + 255) // 256 > 32
    rng = np.random.default_rng(8193)
    keys = R._runs(rng, n, lambda m: rng.integers(0, 256, size=m, dtype=np.uint64)).astype(np.uint32)
    order = np.argsort(keys.astype(np.uint8), kind="stable")
    want_k, want_v = child.dev_words(keys[order]), child.dev_words(order.astype(np.uint32))
    dk = child.dev_words(keys)
    for _ in range(2):                                      # the second run: bit-identical, being equal to the same reference
        ko, vo, out_idx, _, short = selftest_sort(dk, None, n, 0, 8, 8, 0, 0)
        assert out_idx == 1 and not short
        assert torch.equal(ko, want_k), "sorted keys"
        assert torch.equal(vo, want_v), "sorted values (tie order)"


# (n, cap, digit_bits, bit_lo, bit_hi, hist_copies, short)
WATCH = [(1000, 1500, 9, 0, 27, 0, True), (1000, 1500, 9, 0, 27, 1, False), (1000, 1500, 8, 0, 32, 0, True),
         (2049, 2100, 8, 0, 8, 0, True), (40000, 41000, 9, 0, 27, 0, False), (40000, 41000, 8, 0, 32, 0, False)]


@pytest.mark.parametrize("n,cap,db,lo,hi,hc,short", WATCH)
def test_saturated_key_watch(n, cap, db, lo, hi, hc, short):
    """Bit value 2 of the flag word exactly when a key below n equals flag_key -- the whole key, as the first pass sees it."""
    flag_key = 0x07FFFFFE                                   # the depth sort's saturated key
    rng = np.random.default_rng(n + db)
    base = R.make_keys("uniform", cap, rng, lo, hi, db)
    base[base == flag_key] ^= 1
    # keys that agree with flag_key in every digit but the first: nothing for a later pass to find
    near = np.uint32(flag_key ^ 1)
    base[rng.integers(0, cap, size=cap // 7)] = near
    base[n - 2], base[n] = near, near

    def run(at, start):
        keys = base.copy()
        for i in at:
            keys[i] = flag_key
        flag, _ = child.check_sort(keys, None, n, db, lo, hi, start, hc, short, flag_key=flag_key, what=f"watch at {at}")
        return flag

    assert run([], 0) == 0, "no key equals flag_key"
    assert run([0], 1) == 2, "first item"
    assert run([n - 1], 0) == 2, "last live item"
    assert run([n], 1) == 0, "the item AT n is not part of the sort"
    assert run([n, cap - 1], 0) == 0
    assert run([n // 2, n - 1, n], 1) == 2
    # without a flag word the sort does not watch
    flag, _ = child.check_sort(base, None, n, db, lo, hi, 0, hc, short, what="no watch")
    assert flag == 0


def test_three_launch_passes_when_short_sorts_are_switched_off():
    """TRASE_SORT_SMALL=0 is read once per process: a fresh child repeats the sizes up to 32768 and must find the three-launch
    passes everywhere, with the same results."""
    env = dict(os.environ, TRASE_SORT_SMALL="0")
    p = subprocess.run([sys.executable, "-m", "tests.sort_child", "three-launch"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert p.stdout.strip().splitlines()[-1].startswith("ok {")
    print(p.stdout.strip().splitlines()[-1])


# ---- tile ranges -----------------------------------------------------------------------------------------------------------
FILL = 0x7B7B7B7B
GUARD = 8               # pairs behind ranges[T] that nothing may touch


def _key_sets(n, rng):
    """name -> (n sorted keys, T)"""
    i = np.arange(n, dtype=np.int64)
    out = {"distinct": (3 * i + 1, 3 * n + 2), "one-run": (np.full(n, 7, dtype=np.int64), 16)}
    for d in (-1, 0, 1):                                    # runs end at, one before and one after multiples of 8 (so of 4) and of 1024
        edge = ((i - d) % 8 == 0) | ((i - d) % 1024 == 0)
        edge[:1] = False
        k = np.cumsum(edge)
        out[f"runs{d:+d}"] = (k, int(k.max(initial=0)) + 2)
    d4 = ((i % 4 == 0) & (i // 4 % 3 == 0)) | ((i % 4 == 1) & (i // 4 % 3 == 1)) | ((i % 4 == 3) & (i // 4 % 3 == 2))
    d4[:1] = False
    k = np.cumsum(d4)                                       # and at every multiple of 4 in turn: at, after, before
    out["runs4"] = (k, int(k.max(initial=0)) + 2)
    T = 1 << 18
    out["sparse"] = (np.sort(rng.choice(T, size=n, replace=False)).astype(np.int64), T)      # T far above the keys present
    return out


def _ranges_case(keys, n, cap, T, clear, prefill=FILL):
    """Runs the aligned and the one-word-offset form; returns [(ranges incl. guard, dbg)] and the key words as laid out."""
    from trase_amd.rasterizer import selftest_tile_ranges
    words = np.empty(cap, dtype=np.uint32)
    words[:n] = keys
    words[n:] = keys[n - 1] if n else 0                     # behind n: the last key again, so a read past n hides a run's end
    res = []
    for off in (0, 1):
        buf = np.full(cap + 8, words[0] if n else 0, dtype=np.uint32)       # before the list: the first key again
        buf[off + 4:off + 4 + cap] = words
        dbuf = child.dev_words(buf)
        view = dbuf[4 + off:4 + off + cap]
        assert (view.data_ptr() % 16 == 0) == (off == 0)
        ranges = torch.full((T + GUARD, 2), prefill, dtype=torch.int32, device="cuda")
        dbg = selftest_tile_ranges(view, n, cap, ranges, T, clear)
        res.append((child.host_words(ranges).reshape(-1, 2), dbg))
    return res


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 1024, 1025, 4097])
@pytest.mark.parametrize("clear", [True, False])
def test_tile_ranges_equal_reference(n, clear):
    rng = np.random.default_rng(n)
    caps = [max(4, (n + 3) // 4 * 4)] + ([4100] if n == 1023 else [])       # n far below the capacity the grid is sized for, too
    for name, (keys, T) in _key_sets(n, rng).items():
        for cap in caps:
            before = np.full((T + GUARD, 2), FILL, dtype=np.uint32)
            if clear:
                before[:T] = 0
            want = R.tile_ranges_reference(keys.astype(np.uint32), n, before)
            if not clear:                                   # absent entries keep the prefilled words
                absent = np.setdiff1d(np.arange(T), keys)
                assert np.all(want[absent] == FILL) and (n == 0 or np.all(want[keys] != FILL))
            (r0, dbg0), (r1, dbg1) = _ranges_case(keys, n, cap, T, clear)
            assert np.array_equal(r0, want), f"{name} cap {cap} aligned: {child.first_diff(r0.ravel(), want.ravel())}"
            assert np.array_equal(r1, want), f"{name} cap {cap} offset by one word: {child.first_diff(r1.ravel(), want.ravel())}"
            assert dbg0[0] == 0 and dbg1[0] == 0


@pytest.mark.parametrize("n", [1, 4, 5, 1025])
def test_tile_ranges_out_of_range_key(n):
    """One key >= T (the last of the sorted list): reported, clamped into T - 1, nothing behind ranges[T] written."""
    T = 2 * n + 3
    keys = 2 * np.arange(n, dtype=np.int64)                 # T - 1 itself is not among them
    keys[n - 1] = T + 5
    cap = (n + 3) // 4 * 4
    before = np.full((T + GUARD, 2), FILL, dtype=np.uint32)
    before[:T] = 0
    want = R.tile_ranges_reference(keys[:n - 1].astype(np.uint32), n - 1, before)
    want[T - 1] = (n - 1, n)
    for r, dbg in _ranges_case(keys, n, cap, T, True):
        assert dbg == [1, n - 1, T + 5]
        assert np.array_equal(r[T:], before[T:]), "guard words behind ranges[T]"
        assert np.array_equal(r, want), child.first_diff(r.ravel(), want.ravel())


# ---- zero fill ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [0, 1, 15, 16, 17, 31, 4096 + 5, (1 << 20) + 3])
def test_zero_bytes_exact_extent(nbytes):
    from trase_amd.rasterizer import selftest_zero_bytes
    lead = 32                                               # bytes in front of the pointer, also at offset 0
    buf = torch.empty(lead + 16 + nbytes + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    for off in range(16):
        buf.fill_(0xA5)
        p = lead + off
        selftest_zero_bytes(buf, p, nbytes)
        assert bool((buf[:p] == 0xA5).all()), f"offset {off}: a byte before the range was written"
        assert bool((buf[p:p + nbytes] == 0).all()), f"offset {off}: a byte of the range was not cleared"
        assert bool((buf[p + nbytes:] == 0xA5).all()), f"offset {off}: a byte behind the range was written"
