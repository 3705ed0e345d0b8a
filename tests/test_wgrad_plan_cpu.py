"""No GPU: the host decisions of the backward-weights launchers (the split plan of csrc/conv_plan.hpp) against the table recorded from the
commit before they shared it (tests/golden/wgrad_plan.json, tests/golden/make_golden_wgrad_plan.py), the structural refusals of the three
3x3 families, and the Python restatement of the rule (tests/wgrad_plan_cases.py) against the values it was written down with."""
import ctypes
import itertools
import json
import os

import pytest

import wgrad_plan_cases as cases
from rpg_ramnet_amd import _hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plan.json")


@pytest.fixture(scope="module")
def tables():
    with open(GOLDEN) as f:
        want = json.load(f)
    return want, cases.table(_hip.lib())


def test_grid_is_the_recorded_one(tables):
    want, got = tables
    assert want["axes"] == got["axes"] and want["rows"] == got["rows"] == len(want["slabs"]) > 5000
    assert os.path.getsize(GOLDEN) <= 31 * 1024


def test_slab_answers_equal_the_parent_row_by_row(tables):
    want, got = tables
    bad = [(i, row, w, g) for i, (row, w, g) in enumerate(zip(cases.grid(), want["slabs"], got["slabs"])) if w != g]
    assert not bad, "%d of %d rows differ, first: %r" % (len(bad), want["rows"], bad[:5])
    assert got["channel_only"] == want["channel_only"]
    seen = set(want["slabs"])                                   # the grid reaches 0, 1, the cap and values between
    assert {0, 1, cases.SLAB_CAP} <= seen and any(1 < v < cases.SLAB_CAP for v in seen)
    for algo in cases.ALGOS:                                    # ... and every algorithm answers something
        assert any(w > 0 for row, w in zip(cases.grid(), want["slabs"]) if row[0] == algo), algo


def test_descriptor_query_of_the_3x3_families_is_the_channel_only_one(tables):
    """ramnet_wgrad_slabs of a WINOGRAD / WINOGRAD_2X4 / DIRECT_SPLIT descriptor = ramnet_wgrad_*_slabs(logical Cin, Cout)"""
    want, _ = tables
    L = _hip.lib()
    n = 0
    for (algo, mode, C0, Cout, *_), w in zip(cases.grid(), want["slabs"]):
        if algo in cases.CHANNEL_ONLY:
            assert w == getattr(L, cases.CHANNEL_ONLY[algo])(cases.logical_cin(mode, C0), Cout), (algo, mode, C0, Cout)
            n += 1
    assert n == 3 * 5 * 81


def test_refusal_codes_equal_the_parent(tables):
    want, got = tables
    assert got["violations"] == want["violations"] and len(want["violations"]) == len(cases.VIOLATIONS) >= 30
    assert all(rc == 10001 for _, rc in want["violations"])


@pytest.mark.parametrize("name,fam,make", cases.VIOLATIONS, ids=[n for n, _, _ in cases.VIOLATIONS])
def test_launcher_refuses_a_single_violation(name, fam, make):
    """one structural condition broken, nothing else: RAMNET_E_BADARG with a message, before any HIP call (null stream, no device)"""
    L = _hip.lib()
    assert L.ramnet_conv_launch(None, None) == 10001            # (last error = something else)
    before = L.ramnet_last_error()
    d = make()
    assert L.ramnet_wgrad_launch(ctypes.byref(d), None) == 10001
    assert b"bad argument" in L.ramnet_last_error() and L.ramnet_last_error() != before


@pytest.mark.parametrize("fam,opts,shape,want", cases.EXPECTED + cases.EXPECTED_DSPLIT,
                         ids=["%s-%s-%s" % (f, "x".join(map(str, s)), "-".join("%s%s" % kv for kv in o.items()) or "default")
                              for f, o, s, _ in cases.EXPECTED + cases.EXPECTED_DSPLIT])
def test_restatement_gives_the_written_values(fam, opts, shape, want):
    p = cases.plan(fam, *shape, **opts)
    assert {k: p[k] for k in want} == want, p


def test_restated_cap_is_the_librarys_query():
    L = _hip.lib()
    for fam, (algo, _, _) in cases.FAMILIES.items():
        for ci, co in itertools.product(cases.CH, cases.CH):
            assert cases.cap(fam, ci, co) == getattr(L, cases.CHANNEL_ONLY[algo])(ci, co), (fam, ci, co)
