"""Generates pairhead_argument_errors.json: the (return code, trase_last_error() text) of the eleven entry points of the
FEATURE-state pair head (csrc/pairhead.hip) for a table of bad calls -- one defect at a time, plus two-defect calls that pin
which check answers first.  tests/test_pairhead_argument_errors.py asserts that the library under test refuses the same calls
with the same code and the same message, so regenerate it only from a commit whose answers are known to be right (the table
was recorded from the commit before the head's entry points were put on one forward and one backward).

    python tests/golden/make_pairhead_argument_errors.py     (TRASE_RAST_LIB=<path> selects another build of the library)

The calls need no GPU and never reach one: every pointer is a fake, suitably aligned non-null address that nobody dereferences,
and the device index (DEVICE) does not exist, so that a call the argument checks accept ends in hipSetDevice, in front of its
first launch (TRASE_ERR_HIP).  The generator asserts exactly that of every entry's unedited good call (0 for the two *_sizes
calls) and that every edited call is a refusal by the checks.

A case is {"entry", "label", "ops", "rc", "msg"}; ``ops`` edit the good call of GOOD[entry]: ["null", "feats"] passes a null
pointer for that argument, ["set", "F", 16] stores a value, ["add", "ws_bytes", -1] adds to one."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from trase_amd import _lib  # noqa: E402

DEVICE = 1 << 20            # no such device
REFUSED = (-1, -2, -3)      # TRASE_ERR_INVALID, _UNSUPPORTED, _WORKSPACE
ERR_HIP = -4
S, N, F = 10, 14, 32
HR, WR, H, W = 34, 66, 17, 33
HW = H * W                  # 14 masks of 561 pixels: 7854 bits -> 982 bytes -> a 992-byte stream
BITS_BYTES = 992
BIG = (65536, 32768)        # a plane of 2^31 pixels


def _fake(n):
    return 0x10000 + 256 * n        # fake device addresses: distinct, 256-aligned, never dereferenced


_GEOM = [("Hr", HR), ("Wr", WR), ("h", H), ("w", W)]
_TAIL = [("mode", 0), ("pth", 0.75), ("nth", 0.5), ("use_w", 1)]
_END = [("device", DEVICE), ("stream", None)]


def _forward(resized, packed, s_dev=True):
    a = [("feats", _fake(0)), ("F", F)] + (_GEOM if resized else [("HW", HW)])
    a += [("bits", _fake(1)), ("bits_bytes", BITS_BYTES)] if packed else [("masks", _fake(1))]
    a += [("N", N), ("sampled_mask", _fake(2)), ("n_sampled", N), ("mask_size", _fake(3)), ("pix", _fake(4)), ("S", S)]
    a += [("S_dev", None)] if s_dev else []              # optional: null means "all S entries of pix"
    return a + _TAIL + [("out8", _fake(5)), ("ws", _fake(6)), ("ws_bytes", None)] + _END


def _backward(s_dev=True):
    a = [("F", F), ("HW", HW), ("pix", _fake(4)), ("S", S)] + ([("S_dev", None)] if s_dev else [])
    return a + _TAIL + [("out8", _fake(5)), ("g2", _fake(7)), ("ws", _fake(6)), ("ws_bytes", None), ("accumulate", 0), ("d_feats", _fake(8))] + _END


# the good call of every entry point, in its argument order (include/trase_rast.h); ws_bytes = None: what the matching *_sizes
# call returns; "out" of the two *_sizes calls is a real size_t
GOOD = {
    "trase_pairhead_sizes": [("S", S), ("out", "size_t")],
    "trase_pairhead_sizes_resized": [("S", S)] + _GEOM + [("out", "size_t")],
    "trase_pairhead_forward": _forward(False, False, s_dev=False),
    "trase_pairhead_forward_n": _forward(False, False),
    "trase_pairhead_forward_bits": _forward(False, True),
    "trase_pairhead_forward_resized": _forward(True, False),
    "trase_pairhead_forward_bits_resized": _forward(True, True),
    "trase_pairhead_backward": _backward(s_dev=False),
    "trase_pairhead_backward_n": _backward(),
    "trase_pairhead_backward_resized": ([("F", F)] + _GEOM + [("pix", _fake(4)), ("S", S), ("S_dev", None)] + _TAIL +
                                        [("out8", _fake(5)), ("g2", _fake(7)), ("ws", _fake(6)), ("ws_bytes", None), ("feats", _fake(0)),
                                         ("out2", _fake(9)), ("g_reg", _fake(10)), ("d_feats", _fake(8))] + _END),
    "trase_pairhead_columns_resized": [("feats", _fake(0)), ("F", F)] + _GEOM + [("pix", _fake(4)), ("S", S), ("columns", _fake(11))] + _END,
}
ENTRIES = list(GOOD)
FORWARD = [e for e in ENTRIES if "_forward" in e]
RESIZED = [e for e in ENTRIES if e.endswith("_resized")]
REG = ("feats", "out2", "g_reg")        # trase_pairhead_backward_resized: all three or none
_SCALARS = {"F", "HW", "Hr", "Wr", "h", "w", "bits_bytes", "N", "n_sampled", "S", "mode", "pth", "nth", "use_w", "ws_bytes", "accumulate", "device"}


def _ws_bytes(lib, resized):
    nb = C.c_size_t()
    rc = lib.trase_pairhead_sizes_resized(S, HR, WR, H, W, C.byref(nb)) if resized else lib.trase_pairhead_sizes(S, C.byref(nb))
    assert rc == 0 and nb.value > 0
    return nb.value


def call(lib, entry, ops):
    """-> (rc, message) of `entry` called with the good call edited by `ops`"""
    args = dict(GOOD[entry])
    if "ws_bytes" in args:
        args["ws_bytes"] = _ws_bytes(lib, entry in RESIZED)
    out = C.c_size_t()
    if "out" in args:
        args["out"] = C.byref(out)
    for op, name, *val in ops:
        assert name in args, (entry, name)
        args[name] = None if op == "null" else val[0] if op == "set" else args[name] + val[0]
    rc = int(getattr(lib, entry)(*args.values()))
    return rc, lib.trase_last_error().decode()


def _pointers(entry):
    optional = ("S_dev", "stream") + (REG if entry == "trase_pairhead_backward_resized" else ())
    return [k for k, _ in GOOD[entry] if k not in optional and k not in _SCALARS]


def _single(entry):
    """one defect at a time"""
    names = [k for k, _ in GOOD[entry]]
    d = [("null " + k, [["null", k]]) for k in _pointers(entry)]
    d += [("S = 0", [["set", "S", 0]])]
    if "N" in names:
        d += [("N = 0", [["set", "N", 0]]), ("N = 8193", [["set", "N", 8193]])]
    if "HW" in names:
        d += [("HW = 0", [["set", "HW", 0]])]
    if "Hr" in names:
        d += [(k + " = 0", [["set", k, 0]]) for k in ("Hr", "Wr", "h", "w")]
        d += [("Hr * Wr = 2^31", [["set", "Hr", BIG[0]], ["set", "Wr", BIG[1]]]), ("h * w = 2^31", [["set", "h", BIG[0]], ["set", "w", BIG[1]]])]
    if "mode" in names:
        d += [("mode = -1", [["set", "mode", -1]]), ("mode = 3", [["set", "mode", 3]])]
    if "F" in names:
        d += [("F = 16", [["set", "F", 16]])]
    if "n_sampled" in names:
        d += [("n_sampled_masks = -1", [["set", "n_sampled", -1]]), ("n_sampled_masks = 257", [["set", "n_sampled", 257]])]
    if "ws_bytes" in names:
        d += [("workspace one byte short", [["add", "ws_bytes", -1]])]
    if "bits" in names:
        d += [("stream misaligned by 1", [["add", "bits", 1]]), ("stream misaligned by 4", [["add", "bits", 4]]),
              ("bits_bytes too short", [["set", "bits_bytes", 976]]),            # a multiple of 16 below ceil(7854 / 8) = 982
              ("bits_bytes no multiple of 16", [["set", "bits_bytes", 984]]),    # >= 982, but 984 % 16 == 8
              ("bits_bytes = 0", [["set", "bits_bytes", 0]])]
        if "HW" in names:
            d += [("HW = 2^31", [["set", "HW", 1 << 31]])]
    if entry == "trase_pairhead_backward_resized":       # every proper subset of the regulariser's three but the empty one, which is a good call
        for keep in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):
            d += [("regulariser: only " + " + ".join(REG[i] for i in keep), [["null", REG[i]] for i in range(3) if i not in keep])]
    return d


def _double(entry):
    """two defects: which check answers first"""
    names = [k for k, _ in GOOD[entry]]
    short = ["add", "ws_bytes", -1]
    f16 = ["set", "F", 16]
    d = []
    if entry in FORWARD:
        d += [("null feats + F = 16", [["null", "feats"], f16]), ("N = 0 + F = 16", [["set", "N", 0], f16]),
              ("F = 16 + workspace one byte short", [f16, short]), ("F = 16 + null workspace", [f16, ["null", "ws"]]),
              ("n_sampled_masks = 257 + workspace one byte short", [["set", "n_sampled", 257], short]),
              ("F = 16 + n_sampled_masks = 257", [f16, ["set", "n_sampled", 257]]), ("mode = 3 + F = 16", [["set", "mode", 3], f16]),
              ("null out8 + N = 8193", [["null", "out8"], ["set", "N", 8193]])]
        if "bits" in names:
            d += [("stream misaligned by 4 + F = 16", [["add", "bits", 4], f16]), ("bits_bytes too short + F = 16", [["set", "bits_bytes", 976], f16]),
                  ("stream misaligned by 4 + N = 0", [["add", "bits", 4], ["set", "N", 0]]),
                  ("stream misaligned by 4 + mode = 3", [["add", "bits", 4], ["set", "mode", 3]]),
                  ("bits_bytes = 0 + n_sampled_masks = 257", [["set", "bits_bytes", 0], ["set", "n_sampled", 257]]),
                  ("bits_bytes = 0 + workspace one byte short", [["set", "bits_bytes", 0], short]),
                  ("null bits + S = 0", [["null", "bits"], ["set", "S", 0]])]
    elif "_backward" in entry:
        d += [("null pix + F = 16", [["null", "pix"], f16]), ("F = 16 + workspace one byte short", [f16, short]),
              ("mode = 3 + F = 16", [["set", "mode", 3], f16]), ("mode = 3 + workspace one byte short", [["set", "mode", 3], short]),
              ("S = 0 + null workspace", [["set", "S", 0], ["null", "ws"]])]
    if entry in RESIZED:
        first = _pointers(entry)[0]
        d += [(f"null {first} + S = 0", [["null", first], ["set", "S", 0]]),
              ("S = 0 + Hr * Wr = 2^31", [["set", "S", 0], ["set", "Hr", BIG[0]], ["set", "Wr", BIG[1]]])]
        if "mode" in names:
            d += [("S = 0 + mode = 3", [["set", "S", 0], ["set", "mode", 3]]),
                  ("h * w = 2^31 + mode = 3", [["set", "h", BIG[0]], ["set", "w", BIG[1]], ["set", "mode", 3]])]
        if "F" in names:
            d += [("S = 0 + F = 16", [["set", "S", 0], f16])]
    if entry == "trase_pairhead_backward_resized":
        d += [("regulariser: only feats + S = 0", [["null", "out2"], ["null", "g_reg"], ["set", "S", 0]]),
              ("null g2 + regulariser: only out2", [["null", "g2"], ["null", "feats"], ["null", "g_reg"]]),
              ("regulariser: only g_reg + F = 16", [["null", "feats"], ["null", "out2"], f16])]
    return d


def cases():
    """[(entry, label, ops)]: every bad call of the table"""
    return [(entry, label, ops) for entry in ENTRIES for label, ops in _single(entry) + _double(entry)]


def check_good_calls(lib):
    """every unedited call gets past the argument checks: 0 from the *_sizes calls, hipSetDevice's error from the others"""
    for entry in ENTRIES:
        rc, msg = call(lib, entry, [])
        assert rc == (0 if "_sizes" in entry else ERR_HIP), f"{entry}: the good call returned {rc} ({msg!r})"
    rc, msg = call(lib, "trase_pairhead_backward_resized", [["null", k] for k in REG])         # without the regulariser
    assert rc == ERR_HIP, f"trase_pairhead_backward_resized without the regulariser returned {rc} ({msg!r})"


def build_table(lib):
    check_good_calls(lib)
    rows = []
    for entry, label, ops in cases():
        rc, msg = call(lib, entry, ops)
        assert rc in REFUSED and msg, f"{entry} / {label}: rc {rc} ({msg!r}) -- every case of the table is a refusal by the argument checks"
        rows.append({"entry": entry, "label": label, "ops": ops, "rc": rc, "msg": msg})
    return rows


def main():
    out = os.path.join(HERE, "pairhead_argument_errors.json")
    rows = build_table(_lib.load())
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("wrote", out, os.path.getsize(out), "bytes,", len(rows), "cases")


if __name__ == "__main__":
    main()
