"""Every workspace size the library reports, and the offsets of trase_rast_geom_layout, equal the recorded table
(tests/golden/workspace_sizes.json, written by tests/golden/make_workspace_sizes.py from the commit before the layouts moved
into one function per workspace; the rows of trase_vgg_ws_bytes and trase_lpips_ws_bytes from the commit before the two VGG16
families were put on one network table) integer for integer, and bad arguments keep their error returns.  No GPU needed: the
sizes functions are host arithmetic."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_workspace_sizes as mws  # noqa: E402

TABLE = json.load(open(os.path.join(HERE, "golden", "workspace_sizes.json")))


@pytest.fixture(scope="module")
def lib():
    from trase_amd import _lib
    return _lib.load()


def test_table_covers_every_sizes_function():
    from trase_amd import _lib
    declared = sorted(n for n, _, _ in _lib.SYMBOLS
                      if n.endswith("_sizes") or n in ("trase_rast_geom_layout", "trase_vgg_ws_bytes", "trase_lpips_ws_bytes"))
    assert mws.declared() == declared
    assert sorted(TABLE) == declared
    assert sorted(mws.cases()) == declared
    for name, rows in mws.cases().items():          # the recorded cases are the generator's, none dropped
        assert [c["args"] for c in TABLE[name] if not c.get("null_out")] == rows, name


@pytest.mark.parametrize("name", sorted(TABLE))
def test_sizes_equal_the_recorded_table(lib, name):
    ok = bad = 0
    for case in TABLE[name]:
        rc, out = mws.call(lib, name, case["args"], null_out=case.get("null_out", False))
        assert (rc, out) == (case["rc"], case["out"]), f"{name}{tuple(case['args'])}: got rc {rc} {out}, recorded rc {case['rc']} {case['out']}"
        ok += rc == 0
        bad += rc != 0
    assert ok >= 1 and bad >= 1, f"{name}: the table holds {ok} accepted and {bad} refused calls"


def test_bad_arguments_keep_their_error_codes(lib):
    invalid, unsupported = -1, -2          # TRASE_ERR_INVALID, TRASE_ERR_UNSUPPORTED (include/trase_rast.h)
    for name, rows in TABLE.items():
        for case in rows:
            assert case["rc"] in (0, invalid, unsupported) and (case["rc"] == 0 or case["out"] == []), (name, case)
            if case.get("null_out"):
                assert case["rc"] == invalid, name
    assert mws.call(lib, "trase_rast_sizes", [-1, 640, 360, 32, 1]) == (invalid, [])
    assert b"bad arguments" in lib.trase_last_error()
    assert mws.call(lib, "trase_nnfm_sizes", [32, 10, 10]) == (unsupported, [])          # channel count not compiled in
    assert mws.call(lib, "trase_nnfm_sizes", [64, 0, 10]) == (invalid, [])               # empty feature map
    assert mws.call(lib, "trase_hdbscan_sizes", [65537, 32, 5]) == (invalid, [])
    assert b"2 <= n <= 65536" in lib.trase_last_error()
