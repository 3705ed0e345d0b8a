"""Float64 restatement of the rows of ramnet_eval_table (include/ramnet_hip.h) for the tests, and the layout of tests/golden/eval_table.npz
that they share with tests/golden/make_golden_eval_table.py.

The rows are filled from float32 METRIC-depth maps (target, clipped prediction): the counts, the sums of depth_metrics_kernel's terms —
each term formed in float64 from the float32 depths, the terms added in float64 by numpy — and the float32 medians, found on the sorted
values independently of np.median.  So the restatement differs from the HIP table by the order of a float64 sum, and from the reference's
add_to_metrics by the reference's own float32 arithmetic."""
import numpy as np

KEYS = ("abs_rel_diff", "squ_rel_diff", "RMS_linear", "RMS_log", "SILog", "mean_depth_error", "median_diff", "threshold_delta_1.25",
        "threshold_delta_1.25^2", "threshold_delta_1.25^3")
CUTOFFS = (10, 20, 30, 80, 250, 500)
GROUPS = {"sim": (80.0, 3.70378, 4), "mvsec": (1000.0, 5.70378, 3)}          # group -> clip_distance, reg_factor, files
H, W = 37, 53
ROW = 16
EPS = 1e-5


def metric_depth_numpy(y, clip, reg, clamp=False):
    """prepare_depth_data (evaluation.py:74-96) on float32 arrays, as numpy performs it."""
    y = np.asarray(y, np.float32)
    d = np.exp(np.float32(reg) * (y - np.float32(1.0))) * np.float32(clip)
    if clamp:
        d = np.clip(d, np.float32(np.exp(np.float32(-reg)) * np.float32(clip)), np.float32(clip))
    return d.astype(np.float32)


def median_f32(x):
    """np.median's rule on float32 values without np.median: the middle of the sorted values, (a + b) * 0.5f for an even count."""
    s = np.sort(np.asarray(x, np.float32).ravel())
    k = s.size
    return s[k // 2] if k % 2 else np.float32((s[k // 2 - 1] + s[k // 2]) * np.float32(0.5))


def variants(t, mask, cutoffs):
    """Boolean 'inside' maps in the order of a table row: all pixels, each cut-off (np.nan_to_num(t) < cutoff), then the same under mask."""
    t0 = np.nan_to_num(t)
    base = [np.ones(t.shape, bool)] + [t0 < np.float32(c) for c in cutoffs]
    return base if mask is None else base + [b & (np.asarray(mask) != 0) for b in base]


def restate_rows(t, p, mask=None, cutoffs=CUTOFFS):
    """t / p: float32 metric target (NaN = no ground truth) / clipped metric prediction of one file -> [V, 16] float64 rows."""
    t, p = np.asarray(t, np.float32), np.asarray(p, np.float32)
    rows = []
    for inside in variants(t, mask, cutoffs):
        row = np.zeros(ROW)
        tv, pv = t[inside], p[inside]
        ok = ~np.isnan(tv)
        t64, p64 = tv[ok].astype(np.float64), pv[ok].astype(np.float64)
        d, ld = t64 - p64, np.log(t64 + EPS) - np.log(p64 + EPS)
        r = np.maximum(t64 / (p64 + EPS), p64 / (t64 + EPS))
        row[0], row[1] = tv.size, t64.size
        row[2], row[3], row[4] = np.sum(np.abs(d) / (t64 + 1e-6)), np.sum(d * d / (t64 * t64 + 1e-6)), np.sum(d * d)
        row[5], row[6], row[7] = np.sum(ld * ld), np.sum(np.abs(ld)), np.sum(np.abs(d))
        row[8], row[9], row[10] = np.sum(r <= 1.25), np.sum(r <= 1.5625), np.sum(r <= 1.953125)
        if tv.size and ok.all():
            row[11], row[12] = median_f32(tv), median_f32(pv)
        else:
            row[11] = row[12] = np.nan
        rows.append(row)
    return np.stack(rows)


def golden_files(z):
    """[(group, clip, reg, target_in, pred_in, mask, cells [V, 10], n_mask [V])] of eval_table.npz; V = 14: with masks."""
    out = []
    for group, (clip, reg, nfiles) in GROUPS.items():
        for i in range(nfiles):
            tag = "%s%d" % (group, i)
            mask = np.unpackbits(z[tag + ".mask"])[:H * W].reshape(H, W).astype(bool)
            out.append((group, clip, reg, z[tag + ".target_in"], z[tag + ".pred_in"], mask, z[tag + ".cells"], z[tag + ".n_mask"]))
    return out


def check_cells(got, want, tag, rtol=1e-4, atol=2e-5):
    """got / want: [..., 10] table entries.  NaN exactly where the reference has NaN, the rest at the bound of the existing per-pair table test."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN positions differ\n%s\n%s" % (tag, np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=str(tag))
