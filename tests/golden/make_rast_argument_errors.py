"""Generates rast_argument_errors.json: the (return code, trase_last_error() text) of every rasterizer entry point for a
table of bad calls, one defect at a time.  tests/test_rast_argument_errors.py asserts that the library under test refuses
the same calls with the same code and the same message, so regenerate it only from a commit whose answers are known to be
right (the table was recorded from the commit before the two entry-point families were put on one stage sequence).

    python tests/golden/make_rast_argument_errors.py     (TRASE_RAST_LIB=<path> selects another build of the library;
                                                          TRASE_RAST_LIB_AB=1 lets an older build load that lacks an
                                                          entry point; the rows of such an entry are kept as recorded)

The calls need no GPU and never reach one: every record is full of fake non-null pointers that nobody dereferences, every
call is refused by the argument checks, and should one ever pass them, the device index of the records (DEVICE) does not
exist, so that the call ends in hipSetDevice (TRASE_ERR_HIP, which the generator and the test both reject).  ``debug = 1``
keeps the launch-graph cache (and its miss counter) out of the picture.

A case is {"entry", "label", "ops", "rc", "msg"}; ``ops`` edit the good call: ["null", "s"] passes a null pointer for that
argument, ["set", "in.P", -1] stores a field, ["add", "ws.geom_bytes", -1] adds to one.  Arguments: s settings, in / raw
the input record, out, ws, gr; the pair entry has s0 raw0 out0 ws0 s1 raw1 out1 ws1 and the scalars pair_ws, pair_bytes;
the ranged backward has p_begin, p_end; trase_rast_bin_layout has capacity, T, off."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from trase_amd import _lib  # noqa: E402

DEVICE = 1 << 20            # no such device
P, W, H, F, CAP = 100, 64, 48, 32, 5000
FORWARD_ONLY = 0x800000     # TRASE_VARIANT_FORWARD_ONLY
FAKE = 0x10000              # fake device addresses: distinct, 256-aligned, never dereferenced
REFUSED = (-1, -2, -3)      # TRASE_ERR_INVALID, _UNSUPPORTED, _WORKSPACE

COOKED = ["trase_rast_preprocess", "trase_rast_render", "trase_rast_forward", "trase_rast_backward"]
RAW_FWD = ["trase_rast_preprocess_raw", "trase_rast_render_raw", "trase_rast_forward_raw"]
RAW_BWD = ["trase_rast_backward_raw", "trase_rast_backward_raw_compose", "trase_rast_backward_raw_gaussians"]
RAW = RAW_FWD + RAW_BWD
# entries that look at the geom and pre workspaces only before they launch: stage 1 needs no others, and the one-call forwards
# meet a stage-2 defect (bin / img / tmp, capacity, an output map) only after their stage 1 is in the stream
STAGE1 = ["trase_rast_preprocess", "trase_rast_preprocess_raw", "trase_rast_forward", "trase_rast_forward_raw"]
BACKWARD = ["trase_rast_backward"] + RAW_BWD


def _fake(n):
    return FAKE + 256 * n


def _fill(obj, first):
    """every pointer field of a record <- a fake address"""
    k = first
    for name, t in obj._fields_:
        if t is C.c_void_p:
            setattr(obj, name, _fake(k))
            k += 1
    return obj


def _workspace(lib, p, backward):
    sz = _lib.RastSizes()
    assert lib.trase_rast_sizes(p, W, H, F, CAP, C.byref(sz)) == 0
    ws = _fill(_lib.RastWorkspace(), 100)
    ws.geom_bytes, ws.bin_bytes, ws.img_bytes, ws.pre_bytes = sz.geom_bytes, sz.bin_bytes, sz.img_bytes, sz.pre_bytes
    ws.tmp_bytes = sz.bwd_tmp_bytes if backward else sz.tmp_bytes        # exactly what the entry asks for
    ws.capacity = CAP
    return ws


def _settings():
    s = _fill(_lib.RastSettings(), 0)
    s.image_height, s.image_width, s.tanfovx, s.tanfovy, s.scale_modifier = H, W, 0.5, 0.5, 1.0
    s.sh_degree, s.debug, s.device = 3, 1, DEVICE
    return s


def good_call(lib, entry):
    """-> {argument name: ctypes record or scalar} of a call the argument checks accept, in the entry's argument order"""
    if entry == "trase_rast_bin_layout":
        return {"capacity": CAP, "T": 48, "off": (C.c_int64 * 3)()}
    backward = entry in BACKWARD
    if entry in COOKED:
        rec = _fill(_lib.RastInputs(), 10)
        rec.P, rec.M, rec.F = P, 16, F
        rec.colors_precomp = rec.cov3D_precomp = None         # SH colours, scale / rotation
        args = {"s": _settings(), "in": rec, "out": _fill(_lib.RastOutputs(), 30), "ws": _workspace(lib, P, backward)}
        if backward:
            args["gr"] = _fill(_lib.RastGrads(), 40)
        return args

    def raw():
        r = _fill(_lib.RastRawInputs(), 10)
        r.P, r.F, r.norm_features = P, F, 1
        r.colors_precomp = r.mask = r.d_xyz_se3 = None
        return r
    if entry == "trase_rast_forward_raw_pair":
        nbytes = C.c_size_t()
        assert lib.trase_rast_pair_sizes(P, C.byref(nbytes)) == 0
        args = {}
        for v in "01":
            args.update({"s" + v: _settings(), "raw" + v: raw(), "out" + v: _fill(_lib.RastOutputs(), 30), "ws" + v: _workspace(lib, P, False)})
        args.update({"pair_ws": _fake(200), "pair_bytes": nbytes.value})
        return args
    args = {"s": _settings(), "raw": raw()}
    if entry != "trase_rast_zero_live_rows":
        args["out"] = _fill(_lib.RastOutputs(), 30)
    args["ws"] = _workspace(lib, P, backward)
    if backward or entry == "trase_rast_zero_live_rows":
        args["gr"] = _fill(_lib.RastRawGrads(), 40)
    if entry == "trase_rast_backward_raw_gaussians":
        args.update({"p_begin": 0, "p_end": P})
    return args


def call(lib, entry, ops):
    """-> (rc, message) of `entry` called with the good call edited by `ops`"""
    args = good_call(lib, entry)
    for op, where, *val in ops:
        name, _, field = where.partition(".")
        if op == "null":
            args[name] = None
        elif field:
            setattr(args[name], field, val[0] if op == "set" else getattr(args[name], field) + val[0])
        else:
            args[name] = val[0] if op == "set" else args[name] + val[0]
    actual = [C.byref(v) if isinstance(v, (C.Structure, C.Array)) else v for v in args.values()]
    if entry != "trase_rast_bin_layout":
        actual.append(None)                                   # the stream
    rc = int(getattr(lib, entry)(*actual))
    return rc, lib.trase_last_error().decode()


def _record_defects(rec, cooked):
    """defects of the settings and the input record that every entry point taking both refuses"""
    d = [("null settings", [["null", "s"]]), ("null record", [["null", rec]]),
         ("P < 0", [["set", rec + ".P", -1]]), ("W = 0", [["set", "s.image_width", 0]]), ("H = 0", [["set", "s.image_height", 0]]),
         ("F = 8", [["set", rec + ".F", 8]]),
         ("sh_degree 4, P = 1", [["set", "s.sh_degree", 4], ["set", rec + ".P", 1]]),
         ("sh_degree -1", [["set", "s.sh_degree", -1]]),
         # P = 0: the operator path returns from its checks before it looks at the degree, the raw path after -- the null
         # workspace behind it makes the former a refusal too (and keeps the call off the device)
         ("sh_degree 4, P = 0, null workspace", [["set", "s.sh_degree", 4], ["set", rec + ".P", 0], ["null", "ws"]])]
    d += [("no " + cam, [["set", "s." + cam, None]]) for cam in ("bg", "viewmatrix", "projmatrix", "campos")]
    if cooked:
        d += [("SH and colours", [["set", "in.colors_precomp", _fake(90)]]), ("neither SH nor colours", [["set", "in.shs", None]]),
              ("scale without rotation", [["set", "in.rotations", None]]), ("rotation without scale", [["set", "in.scales", None]]),
              ("covariance beside scale / rotation", [["set", "in.cov3D_precomp", _fake(91)]]),
              ("no covariance, scale or rotation", [["set", "in.scales", None], ["set", "in.rotations", None]]),
              ("no means3D", [["set", "in.means3D", None]]), ("no opacities", [["set", "in.opacities", None]]),
              ("M = 3 at degree 1", [["set", "in.M", 3], ["set", "s.sh_degree", 1]]), ("M = 17", [["set", "in.M", 17]]),
              ("F > 0 without feature rows", [["set", "in.sh_objs", None]])]
    else:
        d += [("no " + f, [["set", "raw." + f, None]]) for f in ("xyz", "opacity", "scaling", "rotation", "features_dc", "features_rest")]
        d += [("colors_precomp with sh_dir_undeformed", [["set", "raw.colors_precomp", _fake(90)], ["set", "raw.sh_dir_undeformed", 1]]),
              ("d_xyz_se3 with d_xyz", [["set", "raw.d_xyz_se3", _fake(91)]]),
              ("F > 0 without gaussian_features", [["set", "raw.gaussian_features", None]]),
              ("F > 0 without featn", [["set", "raw.featn", None]])]
    return d


def _workspace_defects(entry, ws="ws"):
    parts = ["geom", "pre"] + ([] if entry in STAGE1 or entry == "trase_rast_forward_raw_pair" else ["bin", "img", "tmp"])
    d = [("null workspace", [["null", ws]])]
    for p in parts:
        d += [(f"{p} one byte short", [["add", f"{ws}.{p}_bytes", -1]]), (f"{p} null", [["set", f"{ws}.{p}", None]])]
    if "bin" in parts:
        d += [("capacity 0", [["set", ws + ".capacity", 0]]), ("capacity beyond 32 bits", [["set", ws + ".capacity", 0xfffffff1]])]
    return d


def cases():
    """[(entry, label, ops)]: every bad call of the table"""
    t = []
    for entry in COOKED + RAW:
        cooked = entry in COOKED
        d = _record_defects("in" if cooked else "raw", cooked) + _workspace_defects(entry)
        d += [("null outputs", [["null", "out"]]), ("no radii", [["set", "out.radii", None]])]
        if entry in ("trase_rast_render", "trase_rast_render_raw"):
            d += [("no image", [["set", "out.image", None]]), ("no depth", [["set", "out.depth", None]]), ("F > 0 without feats output", [["set", "out.feats", None]])]
        if entry in BACKWARD:
            d += [("null grads", [["null", "gr"]])]
        if entry in RAW_BWD:
            d += [("backward of a FORWARD_ONLY forward", [["set", "s.variant", FORWARD_ONLY]])]
        if entry == "trase_rast_backward_raw_gaussians":
            d += [("misaligned range start", [["set", "p_begin", 32]]), ("reversed range", [["set", "p_begin", 64], ["set", "p_end", 0]]),
                  ("negative range start", [["set", "p_begin", -64]]), ("range end beyond P", [["set", "p_end", P + 28]]),
                  ("misaligned range end", [["set", "p_end", 32]])]
        t += [(entry, label, ops) for label, ops in d]
    z = "trase_rast_zero_live_rows"
    t += [(z, "null " + a, [["null", a]]) for a in ("s", "raw", "ws", "gr")]
    t += [(z, f"{p} one byte short", [["add", f"ws.{p}_bytes", -1]]) for p in ("geom", "pre")]
    t += [(z, f"{p} null", [["set", "ws." + p, None]]) for p in ("geom", "pre")]
    pair = "trase_rast_forward_raw_pair"
    for v in "01":
        def of_view(where):              # "ws.geom" -> "ws0.geom"
            name, dot, field = where.partition(".")
            return name + v + dot + field
        t += [(pair, f"view {v}: {label}", [[op, of_view(w), *val] for op, w, *val in ops])
              for label, ops in _record_defects("raw", False) + _workspace_defects(pair)]
        t += [(pair, f"view {v}: null outputs", [["null", "out" + v]]), (pair, f"view {v}: no radii", [["set", f"out{v}.radii", None]]),
              (pair, f"view {v}: a tile-row strip", [["set", f"s{v}.tile_row_end", 1]])]
    t += [(pair, "unequal P", [["set", "raw1.P", P - 1]]), (pair, "two devices", [["set", "s1.device", DEVICE + 1]]),
          (pair, "pair workspace one byte short", [["add", "pair_bytes", -1]]), (pair, "pair workspace null", [["set", "pair_ws", None]])]
    b = "trase_rast_bin_layout"
    t += [(b, "capacity 0", [["set", "capacity", 0]]), (b, "capacity beyond 32 bits", [["set", "capacity", 0xfffffff1]]),
          (b, "T = 0", [["set", "T", 0]]), (b, "null offsets", [["null", "off"]])]
    return t


def build_table(lib, keep=()):
    rows = []
    for entry, label, ops in cases():
        if not hasattr(lib, entry):
            rows += [r for r in keep if (r["entry"], r["label"]) == (entry, label)]
            continue
        rc, msg = call(lib, entry, ops)
        assert rc in REFUSED and msg, f"{entry} / {label}: rc {rc} ({msg!r}) -- every case of the table is a refusal by the argument checks"
        rows.append({"entry": entry, "label": label, "ops": ops, "rc": rc, "msg": msg})
    return rows


def main():
    out = os.path.join(HERE, "rast_argument_errors.json")
    keep = json.load(open(out)) if os.path.exists(out) else []
    rows = build_table(_lib.load(), keep)
    assert len(rows) == len(cases()), "an entry point is missing from this build and from the recorded table"
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("wrote", out, os.path.getsize(out), "bytes,", len(rows), "cases")


if __name__ == "__main__":
    main()
