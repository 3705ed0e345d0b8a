"""Float64 restatement of the rows of a RESCALED evaluation table (ramnet_eval_table_ex with RAMNET_EVAL_RESCALE, include/ramnet_hip.h) and of
the target resize of --down_scale_factor, for the tests, and the layout of tests/golden/eval_rescale.npz that they share with
tests/golden/make_golden_eval_rescale.py.

rescale_by_the_median (evaluation.py:99-154) followed by add_to_metrics, per (file, variant), in double on the float32 metric depths:

    med_x = the float32 median (sorted middle, (a + b) * 0.5f for an even count)      std_x = sqrt(mean((x - mean(x))^2))
    T_x(v) = (v - med_x) / std_x + |(min_x - med_x) / std_x|
    m_x = T_x(middle value), (T_x(a) + T_x(b)) * 0.5 for an even count;   md = |m_t - m_p|
    m_t < m_p: t' = T_t(t) + md, p' = T_p(p);   otherwise t' = T_t(t), p' = T_p(p) + md

The medians come from a sort, never from np.median; minimum and median of a transformed map are the transforms of the minimum and of the
middle values because T_x is monotone.  A variant that holds a NaN target, or nothing, has NaN sums and medians and zero threshold counts;
zero spread is left to IEEE arithmetic (0 / 0)."""
import numpy as np

import eval_table_restatement as R

DOWN = {"down0": 0.5, "down1": 0.7}          # the files of the down-scaled group of eval_rescale.npz -> down_scale_factor
DOWN_CLIP, DOWN_REG = 80.0, 3.70378


def _middle(x):
    s = np.sort(np.asarray(x, np.float32).ravel())
    k = s.size
    return s[(k - 1) // 2], s[k // 2]


def transform_constants(x):
    """x: float32 values of one side -> (med, std, off, m) in float64."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    a, b = _middle(x)
    med = np.float64(a if x64.size % 2 else np.float32((a + b) * np.float32(0.5)))
    mean = np.sum(x64) / x64.size
    std = np.sqrt(np.sum((x64 - mean) ** 2) / x64.size)
    with np.errstate(all="ignore"):
        off = np.abs((np.min(x64) - med) / std)
        ta, tb = (np.float64(a) - med) / std + off, (np.float64(b) - med) / std + off
    return med, std, off, (ta if x64.size % 2 else (ta + tb) * 0.5)


def rescale_pair(tv, pv):
    """tv / pv: float32 metric target / clipped prediction of the pixels inside (NaN-free, not empty) -> (t', p', median t', median p')."""
    mt, st, ot, m_t = transform_constants(tv)
    mp, sp, op, m_p = transform_constants(pv)
    with np.errstate(all="ignore"):
        t2 = (tv.astype(np.float64) - mt) / st + ot
        p2 = (pv.astype(np.float64) - mp) / sp + op
        md = np.abs(m_t - m_p)
        if m_t < m_p:
            return t2 + md, p2, m_t + md, m_p
        return t2, p2 + md, m_t, m_p + md


def restate_rescaled_rows(t, p, mask=None, cutoffs=R.CUTOFFS):
    """t / p: float32 metric target (NaN = no ground truth) / clipped metric prediction of one file -> [V, 16] float64 rows."""
    t, p = np.asarray(t, np.float32), np.asarray(p, np.float32)
    rows = []
    for inside in R.variants(t, mask, cutoffs):
        row = np.zeros(R.ROW)
        tv, pv = t[inside], p[inside]
        ok = ~np.isnan(tv)
        row[0], row[1] = tv.size, ok.sum()
        if tv.size == 0 or not ok.all():
            row[2:8] = np.nan
            row[11:13] = np.nan
        else:
            t2, p2, row[11], row[12] = rescale_pair(tv, pv)
            with np.errstate(all="ignore"):
                d, ld = t2 - p2, np.log(t2 + R.EPS) - np.log(p2 + R.EPS)
                r = np.fmax(t2 / (p2 + R.EPS), p2 / (t2 + R.EPS))
                row[2], row[3], row[4] = np.sum(np.abs(d) / (t2 + 1e-6)), np.sum(d * d / (t2 * t2 + 1e-6)), np.sum(d * d)
                row[5], row[6], row[7] = np.sum(ld * ld), np.sum(np.abs(ld)), np.sum(np.abs(d))
                row[8], row[9], row[10] = np.sum(r <= 1.25), np.sum(r <= 1.5625), np.sum(r <= 1.953125)
        rows.append(row)
    return np.stack(rows)


def resize_bilinear(x, s):
    """F.interpolate(x[None, None], scale_factor=s, mode='bilinear') at its defaults, restated in float64 numpy: align_corners=False,
    source coordinate max((dst + 0.5) / s - 0.5, 0) from the given factor; a NaN tap makes the output NaN, at weight zero too."""
    x = np.asarray(x, np.float64)
    Hh, Ww = x.shape
    Ho, Wo = int(np.floor(Hh * s)), int(np.floor(Ww * s))
    sy = np.maximum((np.arange(Ho) + 0.5) * (1.0 / s) - 0.5, 0.0)
    sx = np.maximum((np.arange(Wo) + 0.5) * (1.0 / s) - 0.5, 0.0)
    y0, x0 = np.minimum(sy.astype(np.int64), Hh - 1), np.minimum(sx.astype(np.int64), Ww - 1)
    y1, x1 = y0 + (y0 < Hh - 1), x0 + (x0 < Ww - 1)
    ly, lx = (sy - y0)[:, None], (sx - x0)[None, :]
    with np.errstate(invalid="ignore"):
        top = (1.0 - lx) * x[y0][:, x0] + lx * x[y0][:, x1]
        bot = (1.0 - lx) * x[y1][:, x0] + lx * x[y1][:, x1]
        return (1.0 - ly) * top + ly * bot


def _unpack(bits, shape):
    return np.unpackbits(bits)[:shape[0] * shape[1]].reshape(shape).astype(bool)


def golden_files(z):
    """[(tag, clip, reg, down_scale_factor, target_in, pred_in, mask, cells {rescale: [V, 10]}, raised {rescale: [V] bool}, n_mask [V])] of
    eval_rescale.npz.  The same-size files hold rescaled cells only (the plain ones are eval_table.npz); the down-scaled ones hold both."""
    out = []
    tags = [("%s%d" % (g, i), clip, reg, 1.0) for g, (clip, reg, n) in R.GROUPS.items() for i in range(n)]
    tags += [("flat0", 80.0, 3.70378, 1.0)] + [(tag, DOWN_CLIP, DOWN_REG, s) for tag, s in DOWN.items()]
    for tag, clip, reg, s in tags:
        p_in = z[tag + ".pred_in"]
        cells = {True: z[tag + ".cells_rescale"]}
        raised = {True: z[tag + ".raised_rescale"].astype(bool)}
        if s < 1.0:
            cells[False], raised[False] = z[tag + ".cells_plain"], np.zeros(len(cells[True]), bool)
        out.append((tag, clip, reg, s, z[tag + ".target_in"], p_in, _unpack(z[tag + ".mask"], p_in.shape), cells, raised, z[tag + ".n_mask"]))
    return out


def rows_to_cells(rows, has_mask=True, cutoffs=R.CUTOFFS):
    """[V, 16] rows of one file -> [V, 10] table entries through the package's host part (the file's own cells: a table of one file)."""
    from rpg_ramnet_amd import metrics as M
    res = M.finish_eval_rows(np.asarray(rows)[None], cutoffs, has_mask, skip_empty=False)
    return np.array([[res[pre + k] for k in R.KEYS] for pre in M.eval_variant_prefixes(cutoffs, has_mask)])


ABS_REL = R.KEYS.index("abs_rel_diff")
# rtol of the abs_rel_diff column against the reference's rescaled cells: 4 x the worst ratio measured over the whole fixture on the CPU
# (profiles/eval_rescale_notes.md; the rescaled target's minimum is exactly 0 and its neighbours are divided by about 1e-6, so the
# reference's float32 rounding of the target shows there).  Measured 1.050e-3, so 4.2e-3.
ABS_REL_RTOL = 4.2e-3


def check_rescaled_cells(got, want, raised, tag):
    """got / want [V, 10], raised [V]: the cells the reference computed at R.check_cells' bounds (abs_rel_diff at ABS_REL_RTOL), NaN exactly
    where it has NaN; the cells it raised on are the table's own definition: threshold entries 0 or NaN, NaN elsewhere."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    keep = ~np.asarray(raised, bool)
    other = [k for k in range(len(R.KEYS)) if k != ABS_REL]
    R.check_cells(got[keep][:, other], want[keep][:, other], tag)
    assert np.array_equal(np.isnan(got[keep, ABS_REL]), np.isnan(want[keep, ABS_REL])), tag
    np.testing.assert_allclose(got[keep, ABS_REL], want[keep, ABS_REL], rtol=ABS_REL_RTOL, atol=2e-5, err_msg=str(tag))
    bad = got[~keep]
    assert np.isnan(bad[:, :7]).all() and (np.isnan(bad[:, 7:]) | (bad[:, 7:] == 0)).all(), (tag, bad)


def resize_largest_tap(x, s):
    """The largest of the four taps of every output pixel of resize_bilinear(x, s) (NaN taps ignored): the scale of its rounding error."""
    x = np.asarray(x, np.float64)
    Hh, Ww = x.shape
    Ho, Wo = int(np.floor(Hh * s)), int(np.floor(Ww * s))
    sy = np.maximum((np.arange(Ho) + 0.5) * (1.0 / s) - 0.5, 0.0)
    sx = np.maximum((np.arange(Wo) + 0.5) * (1.0 / s) - 0.5, 0.0)
    y0, x0 = np.minimum(sy.astype(np.int64), Hh - 1), np.minimum(sx.astype(np.int64), Ww - 1)
    y1, x1 = y0 + (y0 < Hh - 1), x0 + (x0 < Ww - 1)
    a = np.nan_to_num(np.abs(x))
    return np.max(np.stack([a[y0][:, x0], a[y0][:, x1], a[y1][:, x0], a[y1][:, x1]]), axis=0)
