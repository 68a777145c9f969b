"""The numpy references of tests/sort_reference.py against brute force on tiny inputs, the sort's workgroup arithmetic either
side of its thresholds, and the coverage the case plan of tests/test_gpu_sort.py claims.  No GPU."""
import itertools
import os
import re

import numpy as np

from tests import sort_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute_order(keys, n, lo, hi):
    """Selection by (field, position): no sort routine involved."""
    f = [(int(k) >> lo) & ((1 << (hi - lo)) - 1) for k in keys[:n]]
    left, out = list(range(n)), []
    while left:
        best = left[0]
        for i in left[1:]:
            if f[i] < f[best]:
                best = i
        out.append(best)
        left.remove(best)
    return np.array(out, dtype=np.int64)


def test_sort_reference_against_brute_force():
    rng = np.random.default_rng(1)
    for n, cap in ((0, 3), (1, 1), (2, 2), (7, 9), (40, 40)):
        for lo, hi in ((0, 2), (0, 8), (3, 5), (4, 26), (0, 32), (31, 32)):
            for trial in range(4):
                keys = rng.integers(0, 1 << 32, size=cap, dtype=np.uint64).astype(np.uint32)
                if trial & 1:                                  # many ties in the field, everything else at random
                    keys = (keys & np.uint32(0xFFFFFFFF ^ (((1 << (hi - lo)) - 1) << lo))) | \
                           (rng.integers(0, 2, size=cap, dtype=np.uint64) << np.uint64(lo)).astype(np.uint32)
                vals = R.make_vals(cap, rng)
                want = _brute_order(keys, n, lo, hi)
                assert np.array_equal(R.sort_order(keys, n, lo, hi), want)
                k, v = R.sort_reference(keys, vals, n, lo, hi)
                assert np.array_equal(k, keys[:n][want]) and np.array_equal(v, vals[:n][want])
                k, v = R.sort_reference(keys, None, n, lo, hi)
                assert np.array_equal(v, want.astype(np.uint32)) and v.dtype == np.uint32


def test_digit_by_digit_order_is_the_one_shot_order():
    """Per-pass stability is exactly what the one-shot order needs: LSD passes with a stable sort per digit reproduce it, with
    full and partial last digits, for every configuration and family of the GPU test."""
    for db, lo, hi in R.CONFIGS + [(8, 0, 2), (9, 3, 32), (8, 31, 32)]:
        for fam in R.FAMILIES:
            for n in (0, 1, 2, 65, 700, 5000):
                keys = R.make_keys(fam, n + 3, np.random.default_rng(n), lo, hi, db)
                assert keys.dtype == np.uint32 and keys.shape == (n + 3,)
                assert np.array_equal(R.lsd_order(keys, n, lo, hi, db), R.sort_order(keys, n, lo, hi)), (db, lo, hi, fam, n)


def test_an_unstable_pass_breaks_the_order():
    """The converse: one pass that reverses its ties gives another order, so the kernels cannot get away with less."""
    keys = np.array([0x101, 0x201, 0x102, 0x202, 0x101], dtype=np.uint32)
    order = np.array(sorted(range(5), key=lambda i: (int(keys[i]) & 0xFF, -i)))            # low digit, ties in DESCENDING position
    order = order[np.argsort((keys[order] >> 8) & 0xFF, kind="stable")]
    assert not np.array_equal(order, R.sort_order(keys, 5, 0, 16))


def test_key_families_have_what_they_promise():
    rng = np.random.default_rng(5)
    for db, lo, hi in R.CONFIGS:
        W, nd = hi - lo, 1 << db
        for count in (64, 513, 2049, 40000):
            f = {fam: R.field(R.make_keys(fam, count, rng, lo, hi, db), lo, hi) for fam in R.FAMILIES}
            assert len(np.unique(f["equal"])) == 1
            assert np.all(np.diff(f["ascending"].astype(np.int64)) >= 0) and np.all(np.diff(f["descending"].astype(np.int64)) <= 0)
            assert len(np.unique(f["alternate"])) == 2 and np.all(f["alternate"][:-1] != f["alternate"][1:])
            a, b = np.unique(f["alternate"])
            for shift in range(0, W, db):                       # the two values differ in every digit
                m = (1 << min(db, W - shift)) - 1
                assert (int(a) >> shift) & m != (int(b) >> shift) & m
            for shift in range(0, W, db):
                m = (1 << min(db, W - shift)) - 1
                d = (f["extremes"] >> np.uint64(shift)) & np.uint64(m)
                assert set(np.unique(d)) == {0, m} and (m == nd - 1 or shift + db > W)
            for fam in R.TIE_FAMILIES:                          # ties: fewer distinct fields than items
                assert len(np.unique(f[fam])) < count, fam
            outside = 0xFFFFFFFF ^ (((1 << W) - 1) << lo)
            for fam in ("ascending", "descending", "alternate", "extremes"):
                assert not np.any(R.make_keys(fam, count, rng, lo, hi, db) & np.uint32(outside))
            if outside:
                o = R.make_keys("outside", count, rng, lo, hi, db) & np.uint32(outside)
                assert len(np.unique(o)) > min(count, 1 << bin(outside).count("1")) // 4
        runs = R.make_keys("runs", 400000, rng, lo, hi, db)
        edges = np.flatnonzero(np.diff(runs.astype(np.int64)) != 0) + 1
        lens = np.diff(np.concatenate(([0], edges)))
        assert lens.min() >= 1 and lens.max() <= 200 and lens.max() > 150
        assert len(set(edges % 64)) == 64                       # run ends at every phase of a wave round


def _brute_ranges(keys, n, ranges):
    out = ranges.copy()
    for t in set(int(k) for k in keys[:n]):
        idx = [i for i in range(n) if int(keys[i]) == t]
        out[t] = (idx[0], idx[-1] + 1)
    return out


def test_tile_ranges_reference_against_brute_force():
    rng = np.random.default_rng(2)
    for n, cap in ((0, 4), (1, 4), (3, 4), (5, 8), (30, 32), (30, 40)):
        for T in (1, 2, 7, 50):
            keys = np.sort(rng.integers(0, T, size=cap)).astype(np.uint32)
            before = rng.integers(100, 200, size=(T + 2, 2)).astype(np.uint32)
            got = R.tile_ranges_reference(keys, n, before)
            assert np.array_equal(got, _brute_ranges(keys, n, before))
            absent = np.setdiff1d(np.arange(T + 2), keys[:n])
            assert np.array_equal(got[absent], before[absent])


def test_workgroup_arithmetic_either_side_of_the_thresholds():
    assert [R.rs_blocks(n) for n in (0, 1, 2047, 2048, 2049, 4096, 4097)] == [0, 1, 1, 1, 2, 2, 3]
    assert [R.rs_blocks(n) for n in (32767, 32768, 32769)] == [16, 16, 17]
    assert [R.rs_hist_copies(nb) for nb in (0, 1, 16, 17, 8193)] == [4, 4, 4, 1, 1]
    assert R.rs_blocks(8193 * 2048 - 7) == 8193 and (8193 + 255) // 256 == 33 and (8192 + 255) // 256 == 32   # radix_scan_kernel's `per`
    assert [R.radix_passes(lo, hi, db) for db, lo, hi in R.CONFIGS] == [1, 2, 4, 3, 3, 3, 1]
    # short: at most 16 workgroups AND a histogram per pass AND not switched off
    assert R.sort_is_short(32768, 0, 0, 32, 8) and not R.sort_is_short(32769, 0, 0, 32, 8)
    assert R.sort_is_short(32768, 0, 0, 27, 9) and not R.sort_is_short(32768, 1, 0, 27, 9) and not R.sort_is_short(32768, 2, 0, 27, 9)
    assert R.sort_is_short(32768, 3, 0, 27, 9) and R.sort_is_short(2048, 1, 0, 8, 8) and R.sort_is_short(1, 1, 0, 9, 9)
    assert not R.sort_is_short(32769, 4, 0, 8, 8) and not R.sort_is_short(40000, 0, 0, 8, 8)
    assert not R.sort_is_short(2048, 0, 0, 8, 8, small_off=True)
    assert not R.sort_is_short(32768, 0, 0, 40, 8)              # five passes: more than the default layout's four histograms


def test_constants_are_the_ones_in_common_h():
    src = open(os.path.join(ROOT, "trase_amd", "csrc", "common.h")).read()

    def const(name):
        return int(re.search(r"constexpr int (?:[A-Z_]+ = [^,;]+, )*%s = (\d+)" % name, src).group(1))
    assert const("RS_THREADS") * int(re.search(r"#define TRASE_RS_ITEMS (\d+)", src).group(1)) == R.RS_TILE
    assert const("RS_SMALL_NB") == R.RS_SMALL_NB and const("RS_SMALL_COPIES") == R.RS_SMALL_COPIES
    assert const("RS_MAX_PASSES") == R.RS_MAX_PASSES
    assert "return nb <= RS_SMALL_NB ? RS_SMALL_COPIES : 1;" in src and "return (int)((n + RS_TILE - 1) / RS_TILE);" in src


def test_case_plan_covers_every_mode_at_every_size_with_ties():
    """At every size, every configuration meets every (values, start, hist_copies) mode with a family that has ties, and both
    paths wherever the size allows both (above 16 workgroups there is no short sort; a one-pass sort of at most 16 is always short)."""
    tie = {R.FAMILIES.index(f) for f in R.TIE_FAMILIES}
    for n, cap in R.SIZES:
        for ci, (db, lo, hi) in enumerate(R.CONFIGS):
            seen = {m for fi in tie for m in R.modes_for(fi, ci, n)}
            assert seen == set(R.MODES), (n, cap, db, lo, hi)
            paths = {R.sort_is_short(cap, m.hist_copies, lo, hi, db) for m in seen}
            possible = {False} if R.rs_blocks(cap) > R.RS_SMALL_NB else ({True} if R.radix_passes(lo, hi, db) == 1 else {True, False})
            assert paths == possible, (n, cap, db, lo, hi)
        for fi in range(len(R.FAMILIES)):
            assert all(R.modes_for(fi, ci, n) for ci in range(len(R.CONFIGS)))
    for fi, _ in enumerate(R.FAMILIES):                         # below the largest size every family meets every mode somewhere
        assert {m for ci in range(len(R.CONFIGS)) for m in R.modes_for(fi, ci, 2048)} == set(R.MODES)
    assert len(set(itertools.chain(R.SIZES))) == 16
