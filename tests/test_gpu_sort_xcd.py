"""The three-launch radix passes visit their tiles through a map of the workgroup index over the LIVE tile count
(rs_tile in trase_amd/csrc/binning.hip: every XCD takes a contiguous eighth of the live tiles).  The map must be a bijection on
[0, live tiles) for every remainder of the live count modulo 8, also when the grid (sized by capacity) has dead workgroups behind
the live ones.  A tile the map misses leaves its slice unsorted, a tile visited twice overwrites another's: either shows as a
mismatch with the stable numpy order (tests/sort_reference.py), compared exactly through tests/sort_child.check_sort, which also
requires everything at or beyond n untouched and a second run bit-identical.

Sizes: live tile counts 17 .. 25 (every remainder modulo 8 just above the short sort's 16 tiles), each with its last tile holding
one item, all but one and all 2048; capacities n, n + 3 * 2048 + 5 and 2 n + 7; the pair sort's 8-bit two-pass configuration and
the depth sort's 9-bit three-pass one; caller-supplied and iota values."""
import zlib

import numpy as np
import pytest

from tests import sort_child as child
from tests import sort_reference as R

pytestmark = pytest.mark.gpu

CONFIGS = [(8, 0, 13), (9, 0, 27)]
FAMILIES = ("uniform", "runs")          # every tile's content differs; "runs": ties that cross tiles (the stable order)


def sizes(k):
    return [k * R.RS_TILE - 1, k * R.RS_TILE, (k - 1) * R.RS_TILE + 1]


def caps(n):
    return [n, n + 3 * R.RS_TILE + 5, 2 * n + 7]


@pytest.mark.parametrize("k", range(17, 26))
def test_mapped_tiles_sort_exactly(k):
    cases = 0
    for n in sizes(k):
        assert R.rs_blocks(n) == k
        for cap in caps(n):
            assert cap >= n and R.rs_blocks(cap) > R.RS_SMALL_NB
            vals = R.make_vals(cap, np.random.default_rng(cap))
            for db, lo, hi in CONFIGS:
                for fam in FAMILIES:
                    rng = np.random.default_rng(zlib.crc32(f"xcd-{fam}-{n}-{cap}-{db}".encode()))
                    keys = R.make_keys(fam, cap, rng, lo, hi, db)
                    order = R.sort_order(keys, n, lo, hi)
                    for v in (vals, None):
                        ref = (keys[:n][order], order.astype(np.uint32) if v is None else v[:n][order])
                        _, short = child.check_sort(keys, v, n, db, lo, hi, 0, 0, False, ref=ref, what=f"{fam} k={k}")
                        assert not short
                        cases += 1
    assert cases == 3 * 3 * len(CONFIGS) * len(FAMILIES) * 2


def test_live_count_far_below_the_grid():
    """n_ptr far below the capacity: 17 live tiles in a grid of 200, and the empty sort in the same grid."""
    cap = 200 * R.RS_TILE
    vals = R.make_vals(cap, np.random.default_rng(cap))
    for n in (16 * R.RS_TILE + 1, 0):
        for db, lo, hi in CONFIGS:
            keys = R.make_keys("uniform", cap, np.random.default_rng(n + db), lo, hi, db)
            for v in (vals, None):
                child.check_sort(keys, v, n, db, lo, hi, 0, 0, False, what="sparse grid")
