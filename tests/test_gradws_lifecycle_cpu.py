"""No GPU: the life of ConvParam's weight-gradient workspaces over two passes of a layer — stamped layout, sizes, the launch's dw_slabs,
the slab joins and unpacks asked of the library, what is zeroed for the next pass — against tests/golden/gradws_lifecycle.json, recorded
by tests/golden/make_golden_gradws_lifecycle.py at the commit whose behaviour is kept (CPU tensors, launches recorded and not run)."""
import json
import os

import pytest

import make_golden_gradws_lifecycle as gen
from util import GOLDEN


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "gradws_lifecycle.json")) as f:
        return json.load(f)


def test_the_fixture_has_every_row(golden):
    assert set(golden) == set(gen.ROWS) and len(gen.ROWS) == 4 * 9 + 2 + 4
    # what the recorded commit did on the 64 -> 64 5x5 decoder layer in deterministic mode: the bias joins over the 64 slabs reserved for
    # whichever form the launch takes although the one-launch form owns 32; the direct parity launches join class by class
    calls = golden["fold24_64_k5/det1/auto"][0]["calls"]
    assert calls[:2] == ["ramnet_reduce_slabs|fold24+0,32,409600", "ramnet_reduce_slabs|bias+0,64,64"]
    assert calls[2].startswith("ramnet_fold_unpack_wgrad|") and calls[2].endswith("64,64,64") and len(calls) == 3
    calls = golden["fold_direct_64_k5/det1/auto"][0]["calls"]
    assert calls[:5] == ["ramnet_reduce_slabs|fold_direct+%d,64,65536" % (c * 64 * 65536) for c in range(4)] + ["ramnet_reduce_slabs|bias+0,64,64"]
    first = golden["k3_64_plain/det1/auto"][0]
    assert (first["layout"], first["det_slabs"], first["numel"]["main"]) == (["direct", 192], 64, 18874368)


@pytest.mark.parametrize("row", sorted(gen.ROWS))
def test_lifecycle(golden, row):
    got = json.loads(json.dumps(gen.run_row(row)))
    want = golden[row]
    assert len(got) == len(want) == 2
    for i, (g, w) in enumerate(zip(got, want)):
        for key in ("layout", "det_slabs", "head_cin", "dw_slabs", "algo", "numel", "calls", "zero_runs"):
            assert g[key] == w[key], "pass %d: %s" % (i + 1, key)
        for name, runs in g["zero_runs"].items():       # what was zeroed is one prefix per group of slabs
            n = g["numel"][name]
            assert all(start == j * (n // len(runs)) for j, (start, _) in enumerate(runs)), name
            assert len({length for _, length in runs}) <= 1, name
    assert got[0]["numel"] == got[1]["numel"]           # (the second pass reuses what the first allocated)
