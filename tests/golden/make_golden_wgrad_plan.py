#!/usr/bin/env python3
"""tests/golden/wgrad_plan.json: what the host side of the backward-weights launchers decides — ramnet_wgrad_slabs over the descriptor grid
of tests/wgrad_plan_cases.py, the three channel-only slab queries, and the return code of every structurally refused launch — recorded
from the library of the commit BEFORE the launchers shared one split plan (csrc/conv_plan.hpp).  The table is the reference of
tests/test_wgrad_plan_cpu.py, so it must never be regenerated from the code under test: build the parent commit's library elsewhere and run

    RAMNET_HIP_LIB=/path/to/parent/librpg_ramnet_hip.so python tests/golden/make_golden_wgrad_plan.py

No GPU is needed: the queries are host-only and the refused launches return before any HIP call."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import wgrad_plan_cases as cases  # noqa: E402
from rpg_ramnet_amd import _hip  # noqa: E402


def main():
    if not os.environ.get("RAMNET_HIP_LIB"):
        sys.exit("set RAMNET_HIP_LIB to the parent commit's library: the table is a reference, not a snapshot of the tree")
    t = cases.table(_hip.lib())
    with open(os.path.join(HERE, "wgrad_plan.json"), "w") as f:
        json.dump(t, f, separators=(",", ":"))
        f.write("\n")
    s = t["slabs"]
    print("%d rows: %d answer 0, %d answer 1, %d the cap %d, %d between or above; %d violation rows" % (
        t["rows"], s.count(0), s.count(1), s.count(cases.SLAB_CAP), cases.SLAB_CAP, sum(1 for v in s if v > 1 and v != cases.SLAB_CAP),
        len(t["violations"])))


if __name__ == "__main__":
    main()
