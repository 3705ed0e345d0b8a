"""GPU: the launches that keep state between calls, held to their own stream (profiles/stream_tests_notes.md).

tests/stream_cases.py lists the state and the rows; tests/stream_worker.py runs every row in ONE fresh child process (library scratch is
keyed by the raw stream handle, and "first use on this stream" holds only in a process that has not touched the stream) and prints a JSON
line per row; this file starts it once per session and holds every row to its line.  Row kinds:

first_use    the default stream is held busy by a calibrated delay, the call is made on a fresh stream and that stream alone is
             synchronised; values by the entry point's own launch-test rule, bits equal to the same call on the default stream; a
             package-workspace row must be conclusive (the delay was still running when the synchronise returned), a library-scratch
             row reports it (the library's own hipMalloc may order the device)
second_use   the same call again on that stream: the same bits, every ticket word of the stream's workspace zero
two_streams  two streams, different data, four rounds issued alternately behind one delay with no host synchronisation: every result has
             the bits of its solo result
table_owner  structural (the device is synchronised between the steps): every launch that reads a pointer table reads one that was
             filled on its own stream
capture      captured on a side stream and replayed twice with refilled inputs: the eager bits (atomic forms: the existing rule), and
             no cache entry made or taken while capturing"""
import json
import os
import subprocess
import sys

import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER_CAP = 300          # seconds: a cap against a hang, not an expectation (the notes give the time it takes)


@pytest.fixture(scope="module")
def lines():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stream_worker.py")], capture_output=True, text=True, timeout=WORKER_CAP,
                       cwd=ROOT, env=dict(os.environ))
    out = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    print(r.stdout[-6000:])
    print(r.stderr[-3000:], file=sys.stderr)
    return dict(code=r.returncode, out=out, rows={l["row"]: l for l in out if "row" in l}, stderr=r.stderr[-3000:])


def test_the_worker_ran_every_row(lines):
    fatal = [l for l in lines["out"] if "fatal" in l or "baseline_failed" in l]
    assert not fatal, fatal[0]
    assert lines["code"] == 0, (lines["code"], lines["stderr"])
    assert [l for l in lines["out"] if "done" in l], "the worker did not finish"
    cal = [l["calibration"] for l in lines["out"] if "calibration" in l][0]
    assert 20.0 <= cal["delay_ms"] <= 500.0 and cal["delay_ms"] >= min(20.0 * cal["slowest_undelayed_ms"], 500.0), cal
    assert list(lines["rows"]) == [sc.row_id(r) for r in sc.ROWS]


@pytest.mark.parametrize("row", sc.ROWS, ids=sc.row_id)
def test_stream_row(lines, row):
    line = lines["rows"].get(sc.row_id(row))
    assert line is not None, "the worker stopped before this row: %s" % ([l for l in lines["out"] if "fatal" in l or "baseline_failed" in l] or lines["stderr"])
    print(line)
    assert line["ok"], line["why"]
    if row[1] == "first_use":
        assert isinstance(line["conclusive"], bool)
        if not sc.SURFACES[row[0]]["library"]:
            assert line["conclusive"], "the delay had ended: the row shows nothing"
