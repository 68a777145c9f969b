"""Every entry point of csrc/vgg.hip -- the VGG16 extractor's and LPIPS's -- refuses a bad call before it touches the device,
with the return code and the trase_last_error() text recorded in tests/golden/vgg_argument_errors.json (written by
tests/golden/make_vgg_argument_errors.py from the commit before the two families were put on one network table, one pack
description and one set of checks).  No GPU needed: the calls hold fake pointers that nobody dereferences and name a device that
does not exist."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_vgg_argument_errors as mae  # noqa: E402

TABLE = json.load(open(os.path.join(HERE, "golden", "vgg_argument_errors.json")))


@pytest.fixture(scope="module")
def lib():
    from trase_amd import _lib
    return _lib.load()


def test_table_holds_the_generators_cases_and_only_refusals():
    assert [(r["entry"], r["label"], r["ops"]) for r in TABLE] == [(e, label, json.loads(json.dumps(ops))) for e, label, ops in mae.cases()]
    assert len({(r["entry"], r["label"]) for r in TABLE}) == len(TABLE)
    assert sorted({r["entry"] for r in TABLE}) == sorted(mae.ENTRIES) and len(mae.ENTRIES) == 8
    for r in TABLE:      # a case the recorded commit accepted (or let through to the device) would be a mistake in the table
        assert r["rc"] in mae.REFUSED and r["msg"].startswith(r["entry"] + ": "), r


def test_good_calls_pass_the_checks_and_end_in_hipSetDevice(lib):
    """0 from the two *_ws_bytes calls; from every other entry the error of hipSetDevice on a device that does not exist, which
    every entry point calls in front of its first launch -- that is what keeps a call of the table off the GPU should it ever
    get past the checks.  Also with every optional pointer null."""
    mae.check_good_calls(lib)


@pytest.mark.parametrize("entry", mae.ENTRIES)
def test_bad_calls_keep_code_and_message(lib, entry):
    rows = [r for r in TABLE if r["entry"] == entry]
    assert len(rows) >= 7
    for r in rows:
        got = mae.call(lib, entry, r["ops"])
        assert got == (r["rc"], r["msg"]), f"{entry} / {r['label']}: got {got}, recorded {(r['rc'], r['msg'])}"
