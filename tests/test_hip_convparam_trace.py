"""GPU: the library launches behind ConvParam — packs, weight-gradient layouts, slab joins, unpacks — against the recorded sequence
of tests/golden/convparam_trace.json (written by tests/golden/make_golden_convparam_trace.py at the commit whose behaviour is kept):
names, integer / float arguments, null-ness of pointers and the descriptors' algo / Cout / dw_slabs / head_cin, for two passes with an
in-place parameter update between them, under every switch setting that selects another layout."""
import json
import os
from collections import Counter

import pytest

import convparam_trace_cases as cases
from util import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "convparam_trace.json")) as f:
        return cases.decode(json.load(f))


@pytest.mark.parametrize("net,setting", cases.CASES)
def test_launch_trace(golden, net, setting):
    want = golden["%s/%s" % (net, setting)]
    got = cases.run_case(net, setting)
    for i in (0, 1):
        for j, (g, w) in enumerate(zip(got[i], want[i])):
            assert g == w, "pass %d, call %d" % (i + 1, j)
        assert len(got[i]) == len(want[i]), "pass %d" % (i + 1)
    # the update bumped every trained parameter's version: the second pass re-runs packs of the first — once each, none twice; fewer
    # where a parameter did not change (frozen) or a cached descriptor no longer asks for the pack that its first build went through
    first, second = (Counter(r for r in p if cases.pack_kind(r) is not None) for p in got)
    assert second and not second - first


def test_the_workload_reaches_every_pack_and_layout(golden):
    """The fixture itself: a pack kind or a layout that falls out of these small networks would go unchecked above."""
    assert set(golden) == {"%s/%s" % c for c in cases.CASES}
    flat = [r for passes in golden.values() for p in passes for r in p]
    assert {cases.pack_kind(r) for r in flat} - {None} == cases.PACK_KINDS
    algos = {cases.wgrad_algo(r) for r in flat}
    for kind, algo in cases.LAYOUT_ALGOS.items():
        assert algo in algos, kind
    # deterministic mode: the direct (0), head (2) and both fold launches (3: F(2x2,4x4), 7: F(2x3,4x4)) own slabs as well
    det = [r for s in cases.DETERMINISTIC for net in cases.NETS for p in golden["%s/%s" % (net, s)] for r in p]
    for algo in (0, 2, 3, 7):
        assert any(cases.wgrad_algo(r) == algo and cases.wgrad_slabs(r) > 0 for r in det), algo
    # the frozen weight's unpack launch is gone from the fold, nothing else changes in the first pass
    frozen, trained = Counter(golden["gru/frozen_weight"][0]), Counter(golden["gru/defaults"][0])
    gone = list((trained - frozen).elements())
    assert not frozen - trained and len(gone) == 1 and gone[0].startswith("ramnet_unpack_wgrad"), gone
