"""The per-row arithmetic of the compose kernel (trase_amd/csrc/compose_math.h) compiled for the host: against the float64
restatement within the forward-error bounds, the zero-angle quirk bit for bit, and the guard on out-of-range rows."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import compose_reference as cr
from tests.test_compose_reference import _inside, edit_of, fixture, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("xyz", "scaling", "rotation", "opacity", "features_dc", "features_rest", "gaussian_features")


@pytest.fixture(scope="module")
def sim():
    out = os.path.join(tempfile.gettempdir(), f"libtrase_compose_hostsim_{os.getpid()}.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "hostsim", "compose_hostsim.cpp")])
    lib = C.CDLL(out)
    lib.hs_compose_part.restype = None
    return lib


def run(lib, mdl, rows=None, d=(None, None, None), edit=None):
    """edit: the record of trase_amd.edit.rigid_edit (what the kernel is given), or None."""
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    arrs = [c(mdl[k]) if mdl[k] is not None else None for k in KEYS]
    n = mdl["n"] if "n" in mdl else arrs[0].shape[0]
    F = mdl["F"] if "F" in mdl else arrs[6].shape[-1]
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    m = n if rows is None else rows.shape[0]
    d = [c(x) for x in d]
    mode = 0 if edit is None else (1 if edit.zero_angles else 2)
    R = c(edit.R.reshape(-1) if edit is not None else np.zeros(9))
    q = c(edit.q if edit is not None else np.zeros(4))
    t = c(edit.offset if edit is not None else np.zeros(3))
    s = float(edit.scale_factor) if edit is not None else 1.0
    new = lambda *shape: np.full(shape, np.nan, dtype=np.float32)
    out = dict(means=new(m, 3), scales=new(m, 3), rots=new(m, 4), opac=new(m, 1), shs=new(m, 16, 3), objs=new(m, 1, F))
    lib.hs_compose_part(C.c_int(n), C.c_int(m), C.c_int(F), *[p(a) for a in arrs], p(rows), p(d[0]), p(d[1]), p(d[2]),
                        C.c_int(mode), C.c_float(s), p(R), p(q), p(t), *[p(out[k]) for k in ("means", "scales", "rots", "opac", "shs", "objs")])
    return out


def _record(z, tag="edit"):
    from trase_amd.edit import rigid_edit
    if tag == "zero":
        return rigid_edit(float(z["zero_scale"]), (0.0, 0.0, 0.0), z["zero_offset"].tolist())
    return rigid_edit(float(z["edit_scale"]), [float(a) for a in z["edit_angles"]], z["edit_offset"].tolist())


def test_host_build_lies_inside_the_bounds(sim):
    z = fixture()
    d = (z["d_xyz"], z["d_rotation"], z["d_scaling"])
    rows = np.nonzero(z["mask"])[0]
    for tag, mdl, kw, args in (
            ("plain", model(z, "bg"), {}, {}),
            ("masked edit", model(z, "dyn"), dict(d_xyz=d[0], d_rotation=d[1], d_scaling=d[2], rows=rows, edit=edit_of(z)),
             dict(rows=rows, d=d, edit=_record(z))),
            ("zero angles", model(z, "dyn"), dict(d_xyz=d[0], d_rotation=d[1], d_scaling=d[2], edit=edit_of(z, "zero")),
             dict(d=d, edit=_record(z, "zero")))):
        x, b = cr.compose_part(model=mdl, **kw)
        got = run(sim, mdl, **args)
        for k in ("means", "scales", "rots", "opac"):           # 8, 4, 16, 4 roundings: the table in compose_reference.py
            _inside(f"{tag} {k}", got[k], x[k], b[k])
        assert np.array_equal(got["shs"], x["shs"]) and np.array_equal(got["objs"], x["objs"])
    # ... and next to the reference's own fp32 composite
    got = run(sim, model(z, "dyn"), rows=rows, d=d, edit=_record(z))
    n_bg = z["bg_xyz"].shape[0]
    assert float(np.abs(got["means"] - z["masked_means"][n_bg:]).max()) < 2e-6


def test_zero_angles_leave_the_quaternion_unrenormalised_bit_for_bit(sim):
    z = fixture()
    d = (z["d_xyz"], z["d_rotation"], z["d_scaling"])
    plain = run(sim, model(z, "dyn"), d=d)                                  # normalize(q) + d_rotation, no edit
    zero = run(sim, model(z, "dyn"), d=d, edit=_record(z, "zero"))
    assert np.array_equal(zero["rots"].view(np.uint32), plain["rots"].view(np.uint32))
    assert float(np.abs(np.linalg.norm(zero["rots"].astype(np.float64), axis=1) - 1).max()) > 1e-3
    full = run(sim, model(z, "dyn"), d=d, edit=_record(z))
    assert float(np.abs(np.linalg.norm(full["rots"].astype(np.float64), axis=1) - 1).max()) < 1e-6
    assert np.array_equal(zero["scales"], plain["scales"] * np.float32(z["zero_scale"]))


def test_out_of_range_rows_give_null_gaussians_without_touching_the_source(sim):
    z = fixture()
    mdl = model(z, "dyn")
    n = mdl["xyz"].shape[0]
    rows = np.array([0, -1, 5, n, n - 1, n + 7, -(2 ** 40), 2 ** 40], dtype=np.int64)
    got = run(sim, mdl, rows=rows, d=(z["d_xyz"], z["d_rotation"], z["d_scaling"]), edit=_record(z))
    bad = np.array([False, True, False, True, False, True, True, True])
    for k, a in got.items():
        assert not np.isnan(a).any(), k
        assert float(np.abs(a[bad]).max()) == 0.0, f"{k}: an out-of-range row is not all zeros"
    assert float(got["opac"][~bad].min()) > 0 and float(got["scales"][~bad].min()) > 0
    good = run(sim, mdl, rows=rows[~bad], d=(z["d_xyz"], z["d_rotation"], z["d_scaling"]), edit=_record(z))
    for k in got:
        assert np.array_equal(got[k][~bad], good[k])
    # no source at all (every pointer NULL, n = 0): all rows are out of range and nothing may be dereferenced
    null = dict({k: None for k in KEYS}, n=0, F=8)
    got = run(sim, null, rows=np.array([0, 1, -1], dtype=np.int64))
    assert all(float(np.abs(a).max()) == 0.0 for a in got.values())
