#!/usr/bin/env python3
"""tests/golden/wino_plan.json: what the host side of the 3x3 Winograd launchers decides — ramnet_conv_wino_variant,
ramnet_conv_wino_split_ok and ramnet_conv_splitk_floats — over the descriptor grid of tests/wino_plan_cases.py, recorded from the library
of the commit BEFORE the launchers were put on one shared plan (csrc/conv_plan.hpp).  The table is the reference of
tests/test_wino_plan_cpu.py, so it must never be regenerated from the code under test: build the parent commit's library elsewhere and run

    RAMNET_HIP_LIB=/path/to/parent/librpg_ramnet_hip.so python tests/golden/make_golden_wino_plan.py

No GPU is needed: the three entry points are host-only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import wino_plan_cases as cases  # noqa: E402
from rpg_ramnet_amd import _hip  # noqa: E402


def main():
    if not os.environ.get("RAMNET_HIP_LIB"):
        sys.exit("set RAMNET_HIP_LIB to the parent commit's library: the table is a reference, not a snapshot of the tree")
    t = cases.table(_hip.lib())
    with open(os.path.join(HERE, "wino_plan.json"), "w") as f:
        json.dump(t, f, separators=(",", ":"))
        f.write("\n")
    print("%d rows (%d variant, %d split_ok, %d with a split workspace), %d violation rows" % (
        t["rows"], sum(t["variant"]), sum(t["split_ok"]), sum(1 for v in t["splitk_floats"] if v), len(t["violations"])))


if __name__ == "__main__":
    main()
