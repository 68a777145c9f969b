"""The profiler report's keys and per-key counts (what bench.py and profiles/bench_*.py read) for one fixed sequence of calls
equal the table recorded in tests/golden/profile_scopes.json (written by tests/golden/make_profile_scopes.py from the commit
before the launch sites were put on TRASE_LAUNCH / TRASE_LAUNCHES): no scope renamed, merged, split, added or dropped."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_profile_scopes as mps  # noqa: E402

pytestmark = pytest.mark.gpu


def test_profile_scopes_match_the_recorded_table():
    want = json.load(open(os.path.join(HERE, "golden", "profile_scopes.json")))
    got = mps.collect()
    assert got == want, {k: (got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)}
