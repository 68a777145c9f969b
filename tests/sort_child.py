"""Drives the radix sort's test entry point (trase_selftest_sort) over the cases of tests/sort_reference.py and compares every
result buffer, whole, with the numpy reference.  tests/test_gpu_sort.py imports ``check_sort`` / ``run_size``; the command line

    python -m tests.sort_child three-launch

repeats the sizes up to 32768 items for the 8-bit one-pass and the 9-bit three-pass configuration and requires the three-launch
passes everywhere: the test starts it in a process of its own with TRASE_SORT_SMALL=0, which the library reads once.  Not a
test module (no ``test_`` prefix)."""
from __future__ import annotations

import sys
import zlib
from collections import Counter
from typing import Optional

import numpy as np
import torch

from tests import sort_reference as R

SENTINEL = 0xDEADBEEF


def dev_words(a: np.ndarray) -> torch.Tensor:
    """uint32 words on the device (an int32 tensor holding the same bits)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def host_words(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def first_diff(got: np.ndarray, want: np.ndarray) -> str:
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return "equal"
    i = int(bad[0])
    return f"{bad.size} words differ, first at {i}: got {int(got[i]):#x} want {int(want[i]):#x}"


def check_sort(keys: np.ndarray, vals: Optional[np.ndarray], n: int, digit_bits: int, bit_lo: int, bit_hi: int, start: int,
               hist_copies: int, expect_short: Optional[bool], ref=None, flag_key: Optional[int] = None, what: str = ""):
    """One case: sort twice, require the expected path and result buffer index, the first n entries equal to the reference, the
    rest of both result buffers as they were before the sort, and the second run bit-identical.  keys / vals: `cap` words on the
    host (vals None = iota).  ref: (keys_out, vals_out) of R.sort_reference when the caller shares it between modes.  Returns
    (flag word, short)."""
    from trase_amd.rasterizer import selftest_sort
    cap = keys.shape[0]
    m = min(n, cap)
    dk, dv = dev_words(keys), (None if vals is None else dev_words(vals))
    runs = []
    for _ in range(2):
        ko, vo, out_idx, flag, short = selftest_sort(dk, dv, n, bit_lo, bit_hi, digit_bits, hist_copies, start, flag_key, SENTINEL)
        runs.append((host_words(ko), host_words(vo), out_idx, flag, short))
    ko, vo, out_idx, flag, short = runs[0]
    tag = f"{what} n={n} cap={cap} digit_bits={digit_bits} bits=[{bit_lo},{bit_hi}) {'iota' if vals is None else 'vals'} start={start} " \
          f"hist_copies={hist_copies} short={short}"
    if expect_short is not None:
        assert short == expect_short, f"{tag}: expected the {'short' if expect_short else 'three-launch'} path"
    passes = R.radix_passes(bit_lo, bit_hi, digit_bits)
    assert out_idx == start ^ (passes & 1), f"{tag}: out_idx {out_idx}"
    rk, rv = ref if ref is not None else R.sort_reference(keys, vals, m, bit_lo, bit_hi)
    # what the result buffers held before the sort: the input when the sort ends where it began, else the sentinel
    if out_idx == start:
        want_k = keys.copy()
        want_v = np.full(cap, SENTINEL, dtype=np.uint32) if vals is None else vals.copy()
    else:
        want_k = np.full(cap, SENTINEL, dtype=np.uint32)
        want_v = np.full(cap, SENTINEL, dtype=np.uint32)
    want_k[:m], want_v[:m] = rk, rv
    assert np.array_equal(ko[:m], want_k[:m]), f"{tag}: sorted keys: {first_diff(ko[:m], want_k[:m])}"
    assert np.array_equal(vo[:m], want_v[:m]), f"{tag}: sorted values (tie order): {first_diff(vo[:m], want_v[:m])}"
    assert np.array_equal(ko[m:], want_k[m:]), f"{tag}: keys written at or beyond n: {first_diff(ko[m:], want_k[m:])}"
    assert np.array_equal(vo[m:], want_v[m:]), f"{tag}: values written at or beyond n: {first_diff(vo[m:], want_v[m:])}"
    k2, v2, o2, f2, s2 = runs[1]
    assert np.array_equal(k2, ko) and np.array_equal(v2, vo) and (o2, f2, s2) == (out_idx, flag, short), f"{tag}: second run differs"
    return flag, short


def run_size(n: int, cap: int, configs=None, small_off: bool = False) -> Counter:
    """Every family, configuration and planned mode at one size; returns the number of cases per (path, digit_bits)."""
    tally: Counter = Counter()
    vals = R.make_vals(cap, np.random.default_rng(cap))            # one set of caller-supplied values per size
    for ci, (db, lo, hi) in enumerate(R.CONFIGS):
        if configs is not None and (db, lo, hi) not in configs:
            continue
        for fi, fam in enumerate(R.FAMILIES):
            rng = np.random.default_rng(zlib.crc32(f"{fam}-{n}-{cap}-{db}-{lo}-{hi}".encode()))
            keys = R.make_keys(fam, cap, rng, lo, hi, db)
            order = R.sort_order(keys, n, lo, hi)
            ref_iota = (keys[:n][order], order.astype(np.uint32))
            ref_vals = (keys[:n][order], vals[:n][order])
            for mode in R.modes_for(fi, ci, n):
                want_short = R.sort_is_short(cap, mode.hist_copies, lo, hi, db, small_off)
                _, short = check_sort(keys, None if mode.iota else vals, n, db, lo, hi, mode.start, mode.hist_copies, want_short,
                                      ref=ref_iota if mode.iota else ref_vals, what=fam)
                tally[("short" if short else "three-launch", db)] += 1
    return tally


def main(argv) -> int:
    assert argv[1:] == ["three-launch"], __doc__
    total: Counter = Counter()
    for n, cap in R.SIZES:
        if cap <= 32768:
            total += run_size(n, cap, configs=[(8, 0, 8), (9, 0, 27)], small_off=True)
    assert total and all(path == "three-launch" for path, _ in total), total
    print("ok", dict(total))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
