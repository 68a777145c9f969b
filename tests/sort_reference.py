"""numpy references of the integer primitives in trase_amd/csrc/binning.hip -- the stable LSD radix sort on a bit field, the
tile ranges of a sorted key list -- the sort's workgroup arithmetic restated from common.h, and the key families and case
plan that tests/test_gpu_sort.py and tests/sort_child.py run.  No GPU, no torch.  Not a test module (no ``test_`` prefix)."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import numpy as np

# common.h
RS_TILE = 2048            # items per workgroup (256 threads x 8)
RS_SEG = 512              # contiguous items per wave
RS_SMALL_NB = 16          # the short sort: at most this many workgroups ...
RS_SMALL_COPIES = 4       # ... and this many histograms in the default layout
RS_MAX_PASSES = 8


def rs_blocks(n: int) -> int:
    return (n + RS_TILE - 1) // RS_TILE


def rs_hist_copies(nb: int) -> int:
    return RS_SMALL_COPIES if nb <= RS_SMALL_NB else 1


def radix_passes(bit_lo: int, bit_hi: int, digit_bits: int) -> int:
    return (bit_hi - bit_lo + digit_bits - 1) // digit_bits


def sort_is_short(cap: int, hist_copies: int, bit_lo: int, bit_hi: int, digit_bits: int, small_off: bool = False) -> bool:
    """radix_sort_is_short for a sort laid out for `cap` items (hist_copies 0 = the layout's default rule)."""
    nb = rs_blocks(cap)
    copies = hist_copies if hist_copies else rs_hist_copies(nb)
    return nb <= RS_SMALL_NB and copies >= radix_passes(bit_lo, bit_hi, digit_bits) and not small_off


# ---- the sort ------------------------------------------------------------------------------------------------------------
def field(keys: np.ndarray, bit_lo: int, bit_hi: int) -> np.ndarray:
    """The sorted-on bit field of uint32 keys, in the narrowest unsigned type that holds it (numpy's stable sort of 8- and 16-bit
    integers is a counting sort)."""
    W = bit_hi - bit_lo
    f = (keys.astype(np.uint32) >> np.uint32(bit_lo)) & np.uint32((1 << W) - 1)
    return f.astype(np.uint8 if W <= 8 else np.uint16) if W <= 16 else f


def sort_order(keys: np.ndarray, n: int, bit_lo: int, bit_hi: int) -> np.ndarray:
    """Input positions of the first n keys in output order: ascending bit field, ties in ascending input position."""
    return np.argsort(field(keys[:n], bit_lo, bit_hi), kind="stable")


def sort_reference(keys: np.ndarray, vals: Optional[np.ndarray], n: int, bit_lo: int, bit_hi: int) -> Tuple[np.ndarray, np.ndarray]:
    """(keys_out, vals_out) of the first n items; vals None = iota values (the input positions)."""
    order = sort_order(keys, n, bit_lo, bit_hi)
    return keys[:n][order], (order.astype(np.uint32) if vals is None else vals[:n][order])


def lsd_order(keys: np.ndarray, n: int, bit_lo: int, bit_hi: int, digit_bits: int) -> np.ndarray:
    """The same order digit by digit, least significant first, every pass a stable sort on its digit alone (the last digit may
    be partial): what the kernels do.  Equal to sort_order only because every pass is stable."""
    order = np.arange(n, dtype=np.int64)
    k = keys[:n].astype(np.uint64)
    for shift in range(bit_lo, bit_hi, digit_bits):
        nbits = min(digit_bits, bit_hi - shift)
        d = (k[order] >> np.uint64(shift)) & np.uint64((1 << nbits) - 1)
        order = order[np.argsort(d, kind="stable")]
    return order


# ---- tile ranges -----------------------------------------------------------------------------------------------------------
def tile_ranges_reference(keys: np.ndarray, n: int, ranges: np.ndarray) -> np.ndarray:
    """ranges: (>= T, 2) as they were before the launch (after the clear, when there is one).  Returns a copy in which every key
    present among the first n (sorted) keys has [first index, last index + 1); absent entries are left as they were."""
    out = ranges.copy()
    k = keys[:n].astype(np.int64)
    if n == 0:
        return out
    first = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
    last = np.flatnonzero(np.concatenate((k[1:] != k[:-1], [True])))
    out[k[first], 0] = first
    out[k[last], 1] = last + 1
    return out


# ---- key families ------------------------------------------------------------------------------------------------------------
FAMILIES = ("uniform", "equal", "ascending", "descending", "alternate", "runs", "extremes", "outside")
TIE_FAMILIES = ("equal", "alternate", "runs", "extremes", "outside")      # many equal bit fields at every size above 2


def _runs(rng: np.random.Generator, count: int, draw) -> np.ndarray:
    """`count` items in runs of 1 to 200 equal values drawn by draw(number of runs): they cross wave rounds (64), wave segments
    (512) and workgroup tiles (2048) at every phase."""
    m = count // 50 + 2                                   # mean run length 100.5: more than enough runs
    lens = rng.integers(1, 201, size=m)
    return np.repeat(draw(m), lens)[:count]


def make_keys(family: str, count: int, rng: np.random.Generator, bit_lo: int, bit_hi: int, digit_bits: int) -> np.ndarray:
    """`count` uint32 keys of one family for a sort on [bit_lo, bit_hi) in digit_bits-bit digits."""
    W = bit_hi - bit_lo
    fmask = (1 << W) - 1
    outside = np.uint64(0xFFFFFFFF ^ (fmask << bit_lo))
    i = np.arange(count, dtype=np.uint64)

    def place(f):                                         # a bit field into the key, nothing outside it
        return ((f.astype(np.uint64) & np.uint64(fmask)) << np.uint64(bit_lo)).astype(np.uint32)

    def rand32(m):
        return rng.integers(0, 1 << 32, size=m, dtype=np.uint64)

    if family == "uniform":
        return rand32(count).astype(np.uint32)
    if family == "equal":
        return np.full(count, 0x5A5A5A5A, dtype=np.uint32)
    if family in ("ascending", "descending"):
        f = (i << np.uint64(W)) // np.uint64(max(count, 1))         # ascending over the whole field, ties when count > 2^W
        return place(f if family == "ascending" else f[::-1])
    if family == "alternate":                             # two values that differ in every digit, lane by lane
        a, b = 0x55555555 & fmask, 0xAAAAAAAA & fmask
        return place(np.where(i & np.uint64(1), np.uint64(b), np.uint64(a)))
    if family == "runs":
        return _runs(rng, count, rand32).astype(np.uint32)
    if family == "extremes":                              # every digit 0 or all ones (digit ND - 1; the partial last one: its own top)
        f = np.zeros(count, dtype=np.uint64)
        for shift in range(0, W, digit_bits):
            nbits = min(digit_bits, W - shift)
            f |= np.where(rng.integers(0, 2, size=count).astype(bool), np.uint64(((1 << nbits) - 1) << shift), np.uint64(0))
        return place(f)
    if family == "outside":                               # few distinct fields in runs; the bits outside the field at random
        alphabet = rand32(37) & np.uint64(fmask)
        f = _runs(rng, count, lambda m: alphabet[rng.integers(0, 37, size=m)])
        return (place(f).astype(np.uint64) | (rand32(count) & outside)).astype(np.uint32)
    raise ValueError(family)


def make_vals(count: int, rng: np.random.Generator) -> np.ndarray:
    """Caller-supplied values: all distinct, in no order (an odd multiplier is a bijection of the 32-bit words)."""
    return ((rng.permutation(count).astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# ---- the case plan -----------------------------------------------------------------------------------------------------------
SIZES = [(0, 4096), (1, 1), (63, 63), (64, 64), (65, 65), (511, 511), (512, 512), (513, 513), (2047, 2047), (2048, 2048),
         (2049, 2049), (32768, 32768), (32769, 32769), (5, 32768), (33000, 40000), (256 * 2048 + 1, 256 * 2048 + 1)]     # (n, cap)
CONFIGS = [(8, 0, 8), (8, 0, 13), (8, 0, 32), (8, 4, 26), (9, 0, 27), (9, 0, 20), (9, 0, 9)]       # (digit_bits, bit_lo, bit_hi)


class Mode(NamedTuple):
    iota: bool
    start: int
    hist_copies: int


MODES = [Mode(io, st, hc) for io in (True, False) for st in (0, 1) for hc in (0, 1)]


def modes_for(family_index: int, config_index: int, n: int) -> List[Mode]:
    """The pruned cross product.  The two tie families made of runs ("runs", "outside"; below the largest size) meet all eight
    (values, start, hist_copies) modes under every configuration; every other family meets two of them, rotating with the family
    and the configuration so that each mode is met by each family somewhere.  At the largest size only "runs" meets all eight."""
    fam = FAMILIES[family_index]
    if fam == "runs" or (fam == "outside" and n <= 40000):
        return list(MODES)
    r = (3 * family_index + config_index) % 8
    return [MODES[r], MODES[(r + 5) % 8]] if n <= 40000 else [MODES[r]]
