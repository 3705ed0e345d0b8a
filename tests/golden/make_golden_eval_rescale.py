#!/usr/bin/env python3
"""tests/golden/eval_rescale.npz: the REFERENCE's evaluation table with --rescale and with --down_scale_factor, as ITS functions compute
it: prepare_depth_data(target, prediction, clip, down_scale_factor, reg_factor), then add_to_metrics(0, {}, target, prediction, mask,
prefix="_", rescale=...) once per file and variant (all pixels, the six cut-offs, the same under the event mask).

Files (tests/eval_rescale_restatement.py golden_files):
  sim0..3, mvsec0..2   the seeded 37 x 53 inputs and masks of tests/golden/eval_table.npz, read from it: rescaled cells;
  flat0                every prediction beyond the clip: the clipped prediction is constant, zero spread;
  down0, down1         --down_scale_factor 0.5 / 0.7: 37 x 53 targets with 20 % NaN, predictions and masks at floor(37 s) x floor(53 s);
                       plain and rescaled cells.
A cell on which the reference RAISES is stored as NaN with raised = 1: an empty variant (np.min of an empty array: ValueError) and a variant
in which a side has zero spread (0 / 0 makes it NaN and model/metric.py's masked division fails to broadcast).  The assertions at the end are
made on the reference's output alone."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
import eval_table_restatement as R  # noqa: E402
import eval_rescale_restatement as RS  # noqa: E402


def cells_of(ev, t, p, mask, rescale):
    vs = R.variants(t, mask, R.CUTOFFS)
    c, raised = np.full((len(vs), len(R.KEYS)), np.nan), np.zeros(len(vs), np.uint8)
    for v, inside in enumerate(vs):
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                m = ev.add_to_metrics(0, {}, t, p, inside, prefix="_", rescale=rescale)
                c[v] = [np.float64(m["_" + k]) for k in R.KEYS]
            except (ValueError, IndexError) as e:
                raised[v] = 1
                print("    variant %d raised %s: %s" % (v, type(e).__name__, str(e)[:80]))
    return c, raised, np.array([int(inside.sum()) for inside in vs])


def main():
    _, _, _, _, _, _, ev = import_reference()
    old = np.load(os.path.join(HERE, "eval_table.npz"))
    out, all_cells, all_raised = {}, [], []
    files = [(g, clip, reg, t_in, p_in, mask) for g, clip, reg, t_in, p_in, mask, _, _ in R.golden_files(old)]
    tags = ["%s%d" % (g, i) for g, (_, _, n) in R.GROUPS.items() for i in range(n)]
    rng = np.random.default_rng(43)
    t = rng.random((R.H, R.W)).astype(np.float32)
    files.append(("flat", 80.0, 3.70378, t, np.full((R.H, R.W), 1.5, np.float32), rng.random((R.H, R.W)) < 0.3))
    tags.append("flat0")
    for tag, (_, clip, reg, t_in, p_in, mask) in zip(tags, files):
        tm, pm = ev.prepare_depth_data(t_in.copy(), p_in.copy(), clip, reg_factor=reg)
        print(tag)
        c, raised, n_mask = cells_of(ev, tm, pm, mask, True)
        out[tag + ".target_in"], out[tag + ".pred_in"], out[tag + ".mask"] = t_in, p_in, np.packbits(mask.ravel())
        out[tag + ".cells_rescale"], out[tag + ".raised_rescale"], out[tag + ".n_mask"] = c, raised, n_mask
        all_cells.append(c), all_raised.append(raised)
        if tag == "flat0":
            assert raised[n_mask > 0].all()                  # zero spread: the reference raises on every variant that holds a pixel
    for tag, s in RS.DOWN.items():
        small = (int(np.floor(R.H * s)), int(np.floor(R.W * s)))
        t_in = rng.random((R.H, R.W)).astype(np.float32)
        t_in[rng.random((R.H, R.W)) < 0.2] = np.nan
        p_in = np.clip(rng.random(small) + 0.08 * rng.standard_normal(small), 0, 1).astype(np.float32)
        mask = rng.random(small) < 0.3
        tm, pm = ev.prepare_depth_data(t_in.copy(), p_in.copy(), RS.DOWN_CLIP, down_scale_factor=s, reg_factor=RS.DOWN_REG)
        assert tm.shape == small == pm.shape and tm.dtype == np.float32, (tm.shape, small, tm.dtype)
        print(tag, small, "NaN targets after the resize %.0f %%" % (100 * np.isnan(tm).mean()))
        out[tag + ".target_in"], out[tag + ".pred_in"], out[tag + ".mask"] = t_in, p_in, np.packbits(mask.ravel())
        plain, raised_plain, n_mask = cells_of(ev, tm, pm, mask, False)
        assert not raised_plain.any() and np.isfinite(plain[:, 0]).sum() >= 10
        c, raised, _ = cells_of(ev, tm, pm, mask, True)
        out[tag + ".cells_plain"], out[tag + ".cells_rescale"], out[tag + ".raised_rescale"], out[tag + ".n_mask"] = plain, c, raised, n_mask
    cells, raised = np.concatenate(all_cells), np.concatenate(all_raised).astype(bool)
    finite = np.isfinite(cells[:, 0])
    print("rescaled cells %d: raised %d, finite abs_rel_diff %d, NaN %d" % (len(cells), raised.sum(), finite.sum(), (~finite & ~raised).sum()))
    assert finite.sum() >= 40 and raised.any() and (~finite & ~raised).any()
    assert (cells[~finite & ~raised][:, 7:] == 0).all()      # a NaN target inside: thresholds 0, NaN elsewhere
    assert np.nanmax(cells[finite][:, 6]) < 1e-4             # the medians are aligned: median_diff is rounding
    path = os.path.join(HERE, "eval_rescale.npz")
    np.savez_compressed(path, **out)
    print("eval_rescale.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
