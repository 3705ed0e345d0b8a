"""GPU: a training pass gives the same loss and gradients whatever the process did before it — other batch sizes and map sizes, a tour
of the switches, an aborted pass, forward-only work, frozen layers, an optimizer step, every manner of writing or replacing a weight, a
device round trip, a deep copy, a second model, graph captures, a user stream, activation checkpointing — and leaves the state between
passes as a fresh model's: workspaces and split-reduction counters zero, nothing dirty or queued, packs those of the live parameters.
Probe, reference, rows and invariants: tests/history_cases.py.  Bits in deterministic mode (the bench schedule, and the same with the
F(2x4,3x3) / F(2x3,4x4) kernels forced); the bench schedule once more in the default mode, at the project's run-to-run bound."""
import pytest

import history_cases as hc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wiring,setting,det", [(w, s, d) for w in hc.HISTORY_WIRINGS for s, d in hc.MODES],
                         ids=lambda v: {True: "det", False: "default"}.get(v, v))
def test_the_settings_reach_their_kernels(wiring, setting, det):
    """the reference pass, by its trace: S1 a head backward-weights launch and a fold launch; S2 an F(2x4,3x3) backward-weights launch
    with slabs, a multi-segment launch, a forward F(2x4,3x3) launch and F(2x3,4x4) (history_cases.reached: which of them a wiring has)"""
    case = hc.Case(wiring, setting, det)
    with hc.schedule(setting, det):
        calls = case.reference()[2]
    got = hc.reached(wiring, setting, calls)
    print(wiring, setting, det, got)
    assert all(got.values()), got


@pytest.mark.parametrize("setting,det", hc.MODES, ids=lambda v: {True: "det", False: "default"}.get(v, v))
def test_the_deferred_queue_gives_the_gradients_of_one_launch_per_update(setting, det):
    hc.check_deferral(setting, det)


@pytest.mark.parametrize("case", hc.CASES, ids=hc.case_id)
def test_history(case):
    hc.run_row(*case)
