"""Every rasterizer entry point refuses a bad call before it touches the device, with the return code and the
trase_last_error() text recorded in tests/golden/rast_argument_errors.json (written by
tests/golden/make_rast_argument_errors.py from the commit before the operator-level and the fused entry points were put on
one stage sequence; trase_rast_bin_layout, which that commit lacks, from the commit that added it).  No GPU needed: the
records hold fake pointers that nobody dereferences and name a device that does not exist."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_rast_argument_errors as mae  # noqa: E402

TABLE = json.load(open(os.path.join(HERE, "golden", "rast_argument_errors.json")))
ENTRIES = sorted({r["entry"] for r in TABLE})


@pytest.fixture(scope="module")
def lib():
    from trase_amd import _lib
    return _lib.load()


def test_table_holds_the_generators_cases_and_only_refusals():
    assert [(r["entry"], r["label"], r["ops"]) for r in TABLE] == [(e, label, json.loads(json.dumps(ops))) for e, label, ops in mae.cases()]
    assert ENTRIES == sorted(mae.COOKED + mae.RAW + ["trase_rast_zero_live_rows", "trase_rast_forward_raw_pair", "trase_rast_bin_layout"])
    for r in TABLE:      # a case the recorded commit accepted (or let through to the device) would be a mistake in the table
        assert r["rc"] in mae.REFUSED and r["msg"], r


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_calls_keep_code_and_message(lib, entry):
    rows = [r for r in TABLE if r["entry"] == entry]
    assert len(rows) >= 4
    for r in rows:
        got = mae.call(lib, entry, r["ops"])
        assert got == (r["rc"], r["msg"]), f"{entry} / {r['label']}: got {got}, recorded {(r['rc'], r['msg'])}"


def test_the_two_paths_test_the_sh_degree_in_their_own_order(lib):
    """An empty scene with sh_degree 4 and a null workspace: the operator path returns from its record checks before it looks at
    the degree and refuses the workspace, the fused path refuses the degree."""
    ops = [["set", "s.sh_degree", 4], ["set", "in.P", 0], ["null", "ws"]]
    assert mae.call(lib, "trase_rast_preprocess", ops) == (-3, "null workspace")
    assert mae.call(lib, "trase_rast_render", ops) == (-3, "null workspace")
    ops[1][1] = "raw.P"
    for entry in ("trase_rast_preprocess_raw", "trase_rast_render_raw", "trase_rast_backward_raw_compose"):
        assert mae.call(lib, entry, ops) == (-1, "sh_degree 4 outside 0..3")


def test_an_empty_scene_needs_no_feature_rows(lib):
    """P = 0, F = 32 and a null featn -- what render() hands over for an empty scene, whose tensors carry null pointers -- is
    no defect of trase_rast_render_raw (it used to answer -1 "featn required"; the operator path never asked for feature rows
    of an empty scene): the checks go on to the workspace, here a null one.  The one-call trase_rast_forward_raw reaches that
    check behind its stage 1, on the device: tests/test_gpu_parity.py::test_empty_scene_through_both_doors[render-one-call-32]."""
    ops = [["set", "raw.P", 0], ["set", "raw.featn", None], ["set", "raw.gaussian_features", None]]
    assert mae.call(lib, "trase_rast_render_raw", ops + [["null", "ws"]]) == (-3, "null workspace")
    assert mae.call(lib, "trase_rast_render_raw", ops + [["set", "out.image", None]]) == (-1, "null output")
    # with Gaussians the rows stay required
    assert mae.call(lib, "trase_rast_render_raw", [["set", "raw.featn", None]]) == (-1, "raw inputs: gaussian_features/featn required when F > 0")
