"""Generates vgg_argument_errors.json: the (return code, trase_last_error() text) of the eight entry points of csrc/vgg.hip --
the VGG16 feature extractor's trase_vgg_ws_bytes / _pack / _forward / _backward and LPIPS's trase_lpips_ws_bytes / _pack /
_forward / _head -- for a table of bad calls: one defect at a time, plus two-defect calls that pin which check answers first.
tests/test_vgg_argument_errors.py asserts that the library under test refuses the same calls with the same code and the same
message, so regenerate it only from a commit whose answers are known to be right (the table was recorded from the commit before
the two families were put on one network table, one pack description and one set of checks).

    python tests/golden/make_vgg_argument_errors.py     (TRASE_RAST_LIB=<path> selects another build of the library)

The calls need no GPU and never reach one: every device pointer is a fake, suitably aligned non-null address that nobody
dereferences, and the device index (DEVICE) does not exist, so that a call the argument checks accept ends in hipSetDevice, in
front of its first launch (TRASE_ERR_HIP).  The arrays of pointers that the pack entries read on the host (weights, biases, lin)
are real arrays of such fakes.  The generator asserts exactly that of every entry's unedited good call (0 for the two *_ws_bytes
calls) and that every edited call is a refusal by the checks.

A case is {"entry", "label", "ops", "rc", "msg"}; ``ops`` edit the good call of GOOD[entry]: ["null", "pack"] passes a null
pointer for that argument, ["set", "layers", 9] stores a value, ["add", "ws_bytes", -1] adds to one (a number or an address),
["null_item", "weights", 3] clears one entry of a pointer array."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from trase_amd import _lib  # noqa: E402

DEVICE = 1 << 20            # no such device
REFUSED = (-1, -3)          # TRASE_ERR_INVALID, TRASE_ERR_WORKSPACE
ERR_HIP = -4
LAYERS, H, W = 8, 67, 35    # the extractor's good call: the deepest cut, an odd image
MIN_VGG, MIN_LPIPS = 8, 16  # smallest side: three pools in front of conv4_1, four in front of conv5_1
HEAD_C, HEAD_HW = 128, 77
BIG = (4096, 8192)          # H * W = 2^25


def _fake(n):
    return 0x10000 + 256 * n        # fake device addresses: distinct, 256-aligned, never dereferenced


_END = [("device", DEVICE), ("stream", None)]
# the good call of every entry point, in its argument order (include/trase_rast.h).  "size_t" / "int32": a real output object;
# ("fakes", n): a host array of n fake addresses; "norm": three real floats; None for a byte count: what the *_ws_bytes call returns
GOOD = {
    "trase_vgg_ws_bytes": [("layers", LAYERS), ("H", H), ("W", W), ("pack_bytes", "size_t"), ("ws_forward_bytes", "size_t"),
                           ("ws_backward_bytes", "size_t"), ("saved_bytes", "size_t"), ("C", "int32"), ("h", "int32"), ("w", "int32")],
    "trase_vgg_pack": [("layers", LAYERS), ("weights", ("fakes", LAYERS)), ("biases", ("fakes", LAYERS)), ("pack", _fake(0)),
                       ("pack_bytes", None)] + _END,
    "trase_vgg_forward": [("layers", LAYERS), ("pack", _fake(0)), ("pack_bytes", None), ("image", _fake(1)), ("H", H), ("W", W),
                          ("mean", "norm"), ("inv_std", "norm"), ("out", _fake(2)), ("saved", _fake(3)), ("saved_bytes", None),
                          ("ws", _fake(4)), ("ws_bytes", None)] + _END,
    "trase_vgg_backward": [("layers", LAYERS), ("pack", _fake(0)), ("pack_bytes", None), ("d_out", _fake(2)), ("H", H), ("W", W),
                           ("inv_std", "norm"), ("saved", _fake(3)), ("saved_bytes", None), ("d_image", _fake(1)), ("ws", _fake(4)),
                           ("ws_bytes", None)] + _END,
    "trase_lpips_ws_bytes": [("H", H), ("W", W), ("pack_bytes", "size_t"), ("ws_bytes", "size_t"), ("map_floats", "size_t")],
    "trase_lpips_pack": [("weights", ("fakes", 13)), ("biases", ("fakes", 13)), ("lin", ("fakes", 5)), ("pack", _fake(0)),
                         ("pack_bytes", None)] + _END,
    "trase_lpips_forward": [("pack", _fake(0)), ("pack_bytes", None), ("x", _fake(1)), ("y", _fake(2)), ("H", H), ("W", W), ("mean", "norm"),
                            ("inv_std", "norm"), ("out_layers", _fake(3)), ("maps", _fake(5)), ("taps_x", _fake(6)), ("taps_y", _fake(7)),
                            ("ws", _fake(4)), ("ws_bytes", None)] + _END,
    "trase_lpips_head": [("a", _fake(1)), ("b", _fake(2)), ("lin", _fake(8)), ("C", HEAD_C), ("hw", HEAD_HW), ("out_layer", _fake(3)),
                         ("map", _fake(5)), ("ws", _fake(4)), ("ws_bytes", None)] + _END,
}
ENTRIES = list(GOOD)
VGG = [e for e in ENTRIES if e.startswith("trase_vgg")]
SIZES = ("trase_vgg_ws_bytes", "trase_lpips_ws_bytes")
# what a good call may leave null (include/trase_rast.h); every other pointer is required
OPTIONAL = {"trase_vgg_forward": ("mean", "inv_std", "saved"), "trase_vgg_backward": ("inv_std",),
            "trase_lpips_forward": ("mean", "inv_std", "maps", "taps_x", "taps_y"), "trase_lpips_head": ("map",)}
ALIGN16 = ("pack", "saved", "ws")
ALIGN8 = ("out_layers", "out_layer")
ALIGN4 = ("x", "y", "maps", "taps_x", "taps_y", "a", "b", "lin", "map")


def _sizes(lib, entry, layers):
    """{byte-count argument: value} of the good call, from the family's *_ws_bytes function"""
    if entry == "trase_lpips_head":
        from trase_amd.lpips import head_ws_bytes
        return {"ws_bytes": head_ws_bytes(HEAD_C, HEAD_HW)}
    sz = [C.c_size_t() for _ in range(4)]
    dims = [C.c_int32() for _ in range(3)]
    if entry in VGG:
        rc = lib.trase_vgg_ws_bytes(layers, H, W, *[C.byref(v) for v in sz], *[C.byref(v) for v in dims])
        names = ("pack_bytes", "ws_forward", "ws_backward", "saved_bytes")
    else:
        rc = lib.trase_lpips_ws_bytes(H, W, *[C.byref(v) for v in sz[:3]])
        names = ("pack_bytes", "ws_bytes", "map_floats")
    assert rc == 0 and sz[0].value > 0
    out = dict(zip(names, (v.value for v in sz)))
    if entry in VGG:
        out["ws_bytes"] = out["ws_backward" if entry.endswith("backward") else "ws_forward"]
    return out


def call(lib, entry, ops):
    """-> (rc, message) of `entry` called with the good call edited by `ops`"""
    args = dict(GOOD[entry])
    sizes = {} if entry in SIZES else _sizes(lib, entry, LAYERS)
    keep = []                                               # the host objects of this call
    for k, v in list(args.items()):
        if v is None and k.endswith("_bytes"):
            args[k] = sizes[k]
        elif v == "size_t" or v == "int32":
            keep.append(C.c_size_t() if v == "size_t" else C.c_int32())
            args[k] = C.byref(keep[-1])
        elif v == "norm":
            args[k] = (C.c_float * 3)(0.5, 0.25, 2.0)
        elif isinstance(v, tuple):
            args[k] = (C.c_void_p * v[1])(*[_fake(16 + i) for i in range(v[1])])
    for op, name, *val in ops:
        assert name in args, (entry, name)
        if op == "null":
            args[name] = None
        elif op == "set":
            args[name] = val[0]
        elif op == "add":
            args[name] = args[name] + val[0]
        else:
            assert op == "null_item"
            args[name][val[0]] = None
    rc = int(getattr(lib, entry)(*args.values()))
    return rc, lib.trase_last_error().decode()


def _pointers(entry, required=True):
    names = [k for k, v in GOOD[entry] if isinstance(v, (str, tuple)) or (isinstance(v, int) and v >= _fake(0) and k != "device")]
    return [k for k in names if (k not in OPTIONAL.get(entry, ())) == required]


def _single(entry):
    """one defect at a time"""
    names = [k for k, _ in GOOD[entry]]
    small = MIN_VGG if entry in VGG else MIN_LPIPS
    d = [("null " + k, [["null", k]]) for k in _pointers(entry)]
    for k in names:
        if isinstance(dict(GOOD[entry])[k], tuple):         # lin of the pack entry is an array, of the head a vector
            continue
        if k in ALIGN16:
            d += [(f"{k} misaligned by {o}", [["add", k, o]]) for o in (4, 8)]
        if k in ALIGN8:
            d += [(f"{k} misaligned by 4", [["add", k, 4]])]
        if k in ALIGN4:
            d += [(f"{k} misaligned by 2", [["add", k, 2]])]
    if entry not in SIZES:
        d += [(k + " one short", [["add", k, -1]]) for k in names if k.endswith("_bytes")]
    if "layers" in names:
        d += [("layers = 0", [["set", "layers", 0]]), ("layers = 9", [["set", "layers", 9]])]
    if "H" in names:
        d += [(f"H = {small - 1}", [["set", "H", small - 1]]), (f"W = {small - 1}", [["set", "W", small - 1]]),
              ("H * W = 2^25", [["set", "H", BIG[0]], ["set", "W", BIG[1]]])]
    if "mean" in names:
        d += [("mean without inv_std", [["null", "inv_std"]]), ("inv_std without mean", [["null", "mean"]])]
    if "taps_x" in names:
        d += [("taps_x without taps_y", [["null", "taps_y"]]), ("taps_y without taps_x", [["null", "taps_x"]])]
    if "weights" in names:
        last = dict(GOOD[entry])["weights"][1] - 1
        d += [("null weights[3]", [["null_item", "weights", 3]]), (f"null biases[{last}]", [["null_item", "biases", last]]),
              ("null weights[0] and biases[1]", [["null_item", "weights", 0], ["null_item", "biases", 1]])]
        if entry == "trase_lpips_pack":
            d += [("null lin[0]", [["null_item", "lin", 0]]), ("null lin[4]", [["null_item", "lin", 4]])]
    if entry == "trase_lpips_head":
        d += [(f"C = {c}", [["set", "C", c]]) for c in (0, 32, 96, 1024)]
        d += [("hw = 0", [["set", "hw", 0]]), ("C * hw = 2^31", [["set", "C", 512], ["set", "hw", 1 << 22]])]
    return d


def _double(entry):
    """two defects: which check answers first"""
    names = [k for k, _ in GOOD[entry]]
    small = MIN_VGG if entry in VGG else MIN_LPIPS
    low = ["set", "H", small - 1]
    off, short_pack, short_ws, short_saved = ["add", "pack", 8], ["add", "pack_bytes", -1], ["add", "ws_bytes", -1], ["add", "saved_bytes", -1]
    d = []
    if entry in SIZES:
        first = _pointers(entry)[0]
        d += [(f"H = {small - 1} + null {first}", [low, ["null", first]])]
        if entry in VGG:
            d += [("layers = 9 + H = 7", [["set", "layers", 9], low]), ("layers = 0 + null C", [["set", "layers", 0], ["null", "C"]])]
    elif entry.endswith("_pack"):
        d += [("null weights + pack misaligned by 8", [["null", "weights"], off]), ("null biases[2] + pack misaligned by 8", [["null_item", "biases", 2], off]),
              ("pack misaligned by 8 + pack_bytes one short", [off, short_pack])]
        if entry in VGG:
            d += [("layers = 9 + null weights", [["set", "layers", 9], ["null", "weights"]])]
        else:
            d += [("null weights[12] + null lin[0]", [["null_item", "weights", 12], ["null_item", "lin", 0]]),
                  ("null lin[1] + pack misaligned by 8", [["null_item", "lin", 1], off])]
    elif entry == "trase_lpips_head":
        d += [("C = 96 + null a", [["set", "C", 96], ["null", "a"]]), ("null b + ws misaligned by 8", [["null", "b"], ["add", "ws", 8]]),
              ("ws misaligned by 8 + out_layer misaligned by 4", [["add", "ws", 8], ["add", "out_layer", 4]]),
              ("map misaligned by 2 + ws_bytes one short", [["add", "map", 2], short_ws]),
              ("ws misaligned by 8 + ws_bytes one short", [["add", "ws", 8], short_ws])]
    else:                                                   # the forward and backward entries
        first = [k for k in _pointers(entry) if k != "pack"][0]
        d += [(f"H = {small - 1} + null pack", [low, ["null", "pack"]]), (f"null {first} + pack misaligned by 8", [["null", first], off]),
              ("pack misaligned by 8 + pack_bytes one short", [off, short_pack]), ("pack_bytes one short + ws_bytes one short", [short_pack, short_ws])]
        if "layers" in names:
            d += [("layers = 9 + H = 7", [["set", "layers", 9], low]), ("ws_bytes one short + saved_bytes one short", [short_ws, short_saved]),
                  ("saved misaligned by 8 + saved_bytes one short", [["add", "saved", 8], short_saved])]
        if "mean" in names:
            d += [(f"null {first} + mean without inv_std", [["null", first], ["null", "inv_std"]]),
                  ("mean without inv_std + ws misaligned by 8", [["null", "inv_std"], ["add", "ws", 8]])]
        if "taps_x" in names:
            d += [("mean without inv_std + taps_x without taps_y", [["null", "inv_std"], ["null", "taps_y"]]),
                  ("taps_x without taps_y + pack misaligned by 8", [["null", "taps_y"], off]),
                  ("ws misaligned by 8 + out_layers misaligned by 4", [["add", "ws", 8], ["add", "out_layers", 4]]),
                  ("x misaligned by 2 + pack_bytes one short", [["add", "x", 2], short_pack])]
    return d


def cases():
    """[(entry, label, ops)]: every bad call of the table"""
    return [(entry, label, ops) for entry in ENTRIES for label, ops in _single(entry) + _double(entry)]


def check_good_calls(lib):
    """every unedited call gets past the argument checks: 0 from the *_ws_bytes calls, hipSetDevice's error from the others,
    also with everything optional left out"""
    for entry in ENTRIES:
        for ops in ([], [["null", k] for k in _pointers(entry, required=False)]):
            if entry == "trase_vgg_forward" and ops:
                ops = ops + [["set", "saved_bytes", 0]]
            rc, msg = call(lib, entry, ops)
            assert rc == (0 if entry in SIZES else ERR_HIP), f"{entry} {ops}: the good call returned {rc} ({msg!r})"


def build_table(lib):
    check_good_calls(lib)
    rows = []
    for entry, label, ops in cases():
        rc, msg = call(lib, entry, ops)
        assert rc in REFUSED and msg, f"{entry} / {label}: rc {rc} ({msg!r}) -- every case of the table is a refusal by the argument checks"
        rows.append({"entry": entry, "label": label, "ops": ops, "rc": rc, "msg": msg})
    return rows


def main():
    out = os.path.join(HERE, "vgg_argument_errors.json")
    rows = build_table(_lib.load())
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("wrote", out, os.path.getsize(out), "bytes,", len(rows), "cases")


if __name__ == "__main__":
    main()
