#!/usr/bin/env python3
"""tests/golden/train_metrics.npz: the REFERENCE's own training metrics (RAM_Net/model/metric.py: mse, abs_rel_diff, squ_rel_diff,
rms_linear, scale_invariant_error, mean_error, median_error — what LSTMTrainer._eval_metrics calls) on seeded (prediction, target)
pairs.  Small pairs are stored with their inputs; of the full-size pairs (8 x 1 x 256 x 344, 2 x 1 x 260 x 346) only the recipe
(tests/train_metrics_restatement.seeded_pair arguments) and the outputs are stored.  Imports the reference (build container only).
Prints, per metric, the largest relative difference between the reference (float32 sums) and the float64 restatement of the tests:
the measured float32 summation noise that tests/test_train_metrics_cpu.py takes its bound from.
    python tests/golden/make_golden_train_metrics.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
import train_metrics_restatement as R  # noqa: E402


def main():
    metric = import_reference()[3]
    out, worst = {}, {k: 0.0 for k in R.NAMES}
    for tag, rec in list(R.SMALL_CASES.items()) + list(R.FULL_CASES.items()):
        p, t = R.seeded_pair(*rec)
        seed, shape, nan_frac, parity, quantised = rec
        out["%s.recipe" % tag] = np.array([seed, *shape, nan_frac, -1 if parity is None else parity, int(quantised)], np.float64)
        if tag in R.SMALL_CASES:
            out["%s.pred" % tag], out["%s.target" % tag] = p, t
        mine = R.restate(p, t)
        out["%s.n" % tag] = np.int64(mine["n"])
        for k in R.NAMES:
            with np.errstate(all="ignore"):
                v = getattr(metric, k)(p.copy(), t.copy())
            out["%s.%s" % (tag, k)] = np.float64(v)
            out["%s.%s.dtype" % (tag, k)] = np.array(str(np.asarray(v).dtype))
            rel = abs(float(v) - float(mine[k])) / abs(float(mine[k])) if mine[k] else abs(float(v))
            worst[k] = max(worst[k], rel)
            if k == "median_error":
                assert np.float32(v) == np.float32(mine[k]), (tag, v, mine[k])
        print(tag, "n", mine["n"], {k: float(out["%s.%s" % (tag, k)]) for k in ("mse", "abs_rel_diff", "median_error")})
    print("largest |reference - float64 restatement| / |restatement| per metric:")
    for k in R.NAMES:
        print("  %-22s %.3e" % (k, worst[k]))
    np.savez_compressed(os.path.join(HERE, "train_metrics.npz"), **out)
    print("train_metrics.npz", os.path.getsize(os.path.join(HERE, "train_metrics.npz")), "bytes")


if __name__ == "__main__":
    main()
