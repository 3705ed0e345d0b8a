"""No GPU: the host decisions of the 3x3 Winograd launchers (csrc/conv_plan.hpp and the plans built on it) against the table recorded
from the commit before they shared a plan (tests/golden/wino_plan.json, tests/golden/make_golden_wino_plan.py), and the agreement of
eligibility and launcher on what is structurally refused."""
import ctypes
import json
import os

import pytest

import wino_plan_cases as cases
from rpg_ramnet_amd import _hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino_plan.json")


@pytest.fixture(scope="module")
def tables():
    with open(GOLDEN) as f:
        want = json.load(f)
    return want, cases.table(_hip.lib())


def test_grid_is_the_recorded_one(tables):
    want, got = tables
    assert want["axes"] == got["axes"] and want["rows"] == got["rows"] == len(want["variant"]) > 3000


@pytest.mark.parametrize("what", ["variant", "split_ok", "splitk_floats"])
def test_host_decisions_equal_the_parent_row_by_row(tables, what):
    want, got = tables
    bad = [(i, row, w, g) for i, (row, w, g) in enumerate(zip(cases.grid(), want[what], got[what])) if w != g]
    assert not bad, "%d of %d rows differ, first: %r" % (len(bad), want["rows"], bad[:5])
    assert any(want[what]) and not all(want[what])              # the grid reaches both answers


def test_violation_rows_equal_the_parent(tables):
    want, got = tables
    assert [list(v) for v in got["violations"]] == want["violations"]
    assert all(f0[:2] == [0, 0] and f1[:2] == [0, 0] for _, f0, f1 in want["violations"])


@pytest.mark.parametrize("name,make", cases.VIOLATIONS, ids=[n for n, _ in cases.VIOLATIONS])
def test_launcher_refuses_what_eligibility_refuses(name, make):
    """A descriptor ramnet_conv_wino_variant(d, 1) turns down on structural grounds is refused by the F(2x4,3x3) launchers with 10001
    before any HIP call (null stream, no device) — and asking does not touch ramnet_last_error()."""
    L = _hip.lib()
    assert L.ramnet_conv_launch(None, None) == 10001
    before = L.ramnet_last_error()
    d = make()
    assert L.ramnet_conv_wino_variant(ctypes.byref(d), 1) == 0 and L.ramnet_conv_wino_split_ok(ctypes.byref(d), 1) == 0
    assert L.ramnet_last_error() == before
    for algo in (_hip.ALGO_WINOGRAD_2X4, _hip.ALGO_WINOGRAD_2X4_SPLIT):
        d = make()
        d.algo = algo
        assert L.ramnet_conv_launch(ctypes.byref(d), None) == 10001 and b"bad argument" in L.ramnet_last_error(), algo
    assert L.ramnet_last_error() != before
