#!/usr/bin/env python3
"""tests/golden/eval_table.npz: every cell of the REFERENCE's evaluation table (evaluation.py:359-390) on seeded 37 x 53 maps — all
pixels, the six depth cut-offs, and the same seven variants under an event mask — as ITS functions compute them: prepare_depth_data,
then add_to_metrics(0, {}, target, prediction, mask, prefix="_") once per file and variant.  The mask is an argument of add_to_metrics;
that is how the event-masked cells are obtained: the reference's own `__main__` raises KeyError on the `event_masked_*` keys (they are
missing from its metrics_keywords), so its command line cannot produce them.

Two groups (tests/eval_table_restatement.py GROUPS): "sim" (clip 80, reg 3.70378; a NaN-free file, one with 20 % NaN targets, one whose
predictions saturate at both clip bounds so that the medians sit in runs of ties, one whose targets all lie beyond 30 m with an all-zero
event mask) and "mvsec" (clip 1000, reg 5.70378; three files, one of them with an all-ones mask).  The other masks are ~30 % dense.
The assertions at the end are made on the reference's output alone."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
import eval_table_restatement as R  # noqa: E402


def inputs(rng, group, i):
    shape = (R.H, R.W)
    t = rng.random(shape).astype(np.float32)
    p = np.clip(t + 0.08 * rng.standard_normal(shape), 0, 1).astype(np.float32)
    mask = rng.random(shape) < 0.3
    if group == "sim":
        if i == 1:
            t[rng.random(shape) < 0.2] = np.nan
        elif i == 2:                                     # most predictions far outside [0, 1]: clipped to clip / exp(-reg) * clip
            far = rng.random(shape) < 0.8
            p = np.where(far, np.where(t > 0.3, np.float32(1.25), np.float32(-0.5)), p).astype(np.float32)
            mask = np.ones(shape, bool)
        elif i == 3:                                     # beyond 30 m: y > 1 + ln(30 / 80) / reg = 0.735
            t = (0.75 + 0.25 * t).astype(np.float32)
            p = np.clip(t + 0.08 * rng.standard_normal(shape), 0, 1).astype(np.float32)
            t[rng.random(shape) < 0.1] = np.nan
            mask = np.zeros(shape, bool)
    else:
        if i == 0:
            mask = np.ones(shape, bool)
        elif i == 1:
            t[rng.random(shape) < 0.3] = np.nan
        elif i == 2:                                     # beyond 10 m, NaN-free: y > 1 + ln(10 / 1000) / reg = 0.193
            t = (0.2 + 0.8 * t).astype(np.float32)
            p = np.clip(t + 0.08 * rng.standard_normal(shape), 0, 1).astype(np.float32)
    return t, p, mask


def main():
    _, _, _, _, _, _, ev = import_reference()
    rng = np.random.default_rng(41)
    out, cells, counts, tie_ok = {}, [], [], False
    for group, (clip, reg, nfiles) in R.GROUPS.items():
        for i in range(nfiles):
            t_in, p_in, mask = inputs(rng, group, i)
            t, p = ev.prepare_depth_data(t_in.copy(), p_in.copy(), clip, reg_factor=reg)
            vs = R.variants(t, mask, R.CUTOFFS)
            c = np.empty((len(vs), len(R.KEYS)))
            for v, inside in enumerate(vs):
                with np.errstate(all="ignore"), warnings.catch_warnings():
                    warnings.simplefilter("ignore")              # (means of empty slices: the NaN cells)
                    m = ev.add_to_metrics(0, {}, t, p, inside, prefix="_")
                c[v] = [np.float64(m["_" + k]) for k in R.KEYS]
            n_mask = np.array([int(inside.sum()) for inside in vs])
            tag = "%s%d" % (group, i)
            out[tag + ".target_in"], out[tag + ".pred_in"] = t_in, p_in
            out[tag + ".mask"] = np.packbits(mask.ravel())
            out[tag + ".cells"], out[tag + ".n_mask"] = c, n_mask
            cells.append(c), counts.append(n_mask)
            if tag == "sim2":                             # a median strictly inside a run of equal values
                for x in (t, p):
                    s = np.sort(x.ravel())
                    k = s.size
                    tie_ok |= bool(s[(k - 1) // 2 - 1] == s[k // 2 + 1])
            print(tag, "abs_rel", c[:, 0].round(4).tolist(), "median_diff", c[:, 6].round(4).tolist(), "n_mask", n_mask.tolist())
    cells, counts = np.concatenate(cells), np.concatenate(counts)
    nan_frac = float(np.isnan(cells[:, 0]).mean())
    finite_med = np.isfinite(cells[:, 6])
    print("cells %d, NaN abs_rel_diff %.1f %%, finite median_diff %.1f %%" % (len(cells), 100 * nan_frac, 100 * finite_med.mean()))
    assert 0.02 <= nan_frac <= 0.25, nan_frac
    assert finite_med.mean() >= 1.0 / 3.0
    assert (counts[finite_med] % 2 == 1).any() and (counts[finite_med] % 2 == 0).any()
    assert tie_ok
    # the edge cases the table has to reproduce are in: an empty mask (ten NaN), a mask of NaN targets only (thresholds 0.0, the rest NaN)
    assert any(n == 0 and np.isnan(c).all() for c, n in zip(cells, counts))
    assert any(n > 0 and (c[7:] == 0).all() and np.isnan(c[:7]).all() for c, n in zip(cells, counts))
    path = os.path.join(HERE, "eval_table.npz")
    np.savez_compressed(path, **out)
    print("eval_table.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
