"""GPU: the five launches of csrc/metrics.hip alone through the C ABI and tests/guarded.py — ramnet_batch_metrics, ramnet_eval_table, ramnet_eval_table_ex,
ramnet_metric_depth, ramnet_resize_metric_target — against the float64 statements of tests/metric_launch_cases.py, per cell.

Every map sits between FINITE poison guards (3e38 / 2.5e38: one guard element read as a pixel breaks a count, a sum and the median; a NaN
would read as "no ground truth" and vanish), every mask between 0xA5 bytes (non-zero: "inside"), every output between sentinels, every
pointer table in a frozen guarded buffer, and the workspace has exactly the stated size, 256-byte aligned between guards, its tickets zero
and everything behind them 0xC3.  Every call runs twice on the same, then dirty, workspace: the same bytes, the tickets zero again.

Rules (profiles/metric_launch_tests_notes.md section 1): counts exact; medians bit for bit as float32; sums within (n - 1) 2^-53 sum|term| of
the statement's own terms (+ the log terms' LOG_ULPS); non-finite cells as the statement has them."""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_table_restatement as R
import guarded as G
import metric_launch_cases as K
from guarded import BADARG, In, Out, call

pytestmark = pytest.mark.gpu

F32 = np.float32
F64 = torch.float64
WORST = {}          # rule -> largest error / bound seen (printed by the last test)


def lib():
    from rpg_ramnet_amd import _hip
    return _hip.lib()


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def fmap(x, fill, skew=0):
    return In(T(np.asarray(x, F32).reshape(1, -1)), fill=float(fill), skew=skew)


def bmask(m, skew=0):
    return In(T(np.asarray(m, np.uint8).reshape(1, -1)), fill=G.SENT_BYTE, dtype=torch.uint8, skew=skew)


def note(rule, err, bound):
    ok = bound > 0
    if ok.any():
        WORST[rule] = max(WORST.get(rule, 0.0), float(np.max(err[ok] / bound[ok])))


def f32_bits_equal(got, want):
    """a widened float32, and the statement's float32 bit for bit (a NaN: any NaN)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    g32, w32 = got.astype(F32), want.astype(F32)
    return (np.array_equal(np.isnan(got), nan) and np.array_equal(g32[~nan].view(np.uint32), w32[~nan].view(np.uint32))
            and np.array_equal(g32[~nan].astype(np.float64), got[~nan]))


def metric_depth(y, clamp, clip=K.CLIP, reg=K.REG, skew=0):
    """ramnet_metric_depth through the guarded call -> float32 array of y's shape"""
    y = np.asarray(y, F32)
    out = Out(1, y.size, skew=(skew + 1) % 4 if skew else 0)
    call("ramnet_metric_depth", fmap(y, K.POISON_P, skew), y.size, clip, reg, clamp, out)
    return out.value().numpy().reshape(y.shape)


# ================================================================================================ ramnet_batch_metrics
def run_bm(pairs, skew=0):
    """pairs: [(p, t)], each [N][npix] -> out [G][10]; two calls on one workspace of exactly the stated size."""
    Gn = len(pairs)
    N, npix = pairs[0][0].shape
    pin = [fmap(p, K.POISON_P, skew) for p, _ in pairs]
    tin = [fmap(t, K.POISON_T, (skew + g + 1) % 4 if skew else 0) for g, (_, t) in enumerate(pairs)]
    nbytes = lib().ramnet_batch_metrics_workspace(Gn, N, npix)
    assert nbytes == K.bm_workspace_bytes(Gn, N, npix)
    ws = G.workspace(nbytes, K.TICKET_BYTES)
    ptab, ttab = G.pointer_table(pin, through_kernel=True, tail=1), G.pointer_table(tin)
    outs = []
    for _ in range(2):
        out = Out(Gn, 10, dtype=F64)
        call("ramnet_batch_metrics", ptab, ttab, Gn, N, npix, ws, out)
        assert G.tickets_zero(ws), "ramnet_batch_metrics left a ticket behind"
        outs.append(out.value().numpy())
    assert outs[0].tobytes() == outs[1].tobytes(), "a second call on the dirty workspace gives other bytes"
    assert not (outs[0] == G.SENT).any() and len(pin) == len(tin) == Gn                                  # (the inputs live until here)
    return outs[0]


def check_bm(got, p, t, tag):
    want, bound = K.bm_statement(p, t)
    assert got[0] == want[0] and got[1] == want[1] and got[9] == 0, (tag, "counts", got, want)
    assert f32_bits_equal(got[8], want[8]), (tag, "median", float(got[8]), float(want[8]))
    assert K.same_class(got[2:8], want[2:8]), (tag, "non-finite cells", got, want)
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)                                                # (inf - inf in the non-finite cells, compared above)
    note("batch_metrics sums", err[fin], bound[fin])
    assert np.all(err[fin] <= bound[fin]), (tag, "sums", (err / np.maximum(bound, 1e-300))[fin].tolist(), got, want)


@pytest.mark.parametrize("N,npix", list(K.BM_STAGE_ROWS))
def test_batch_metrics_stage_chunks(N, npix):
    """P = N rows staged 64 at a time: one full chunk, a second, a ragged third; a sample of the last chunk without a valid target"""
    s = K.BM_STAGE_ROWS[(N, npix)]
    for nan_sample in (s, None):
        pairs = [K.bm_pair(100 * N + g, N, npix, nan_sample=nan_sample) for g in range(2)]
        for skew in (1, 2, 3):
            got = run_bm(pairs, skew)
            for g, (p, t) in enumerate(pairs):
                check_bm(got[g], p, t, "stage N=%d npix=%d nan=%s skew=%d g=%d" % (N, npix, nan_sample, skew, g))
                assert np.isnan(got[g, 2]) == (nan_sample is not None)


@pytest.mark.parametrize("N,npix", list(K.BM_PLAN_ROWS))
def test_batch_metrics_plan_boundaries(N, npix):
    Ws, P = K.BM_PLAN_ROWS[(N, npix)]
    assert (lib().ramnet_batch_metrics_workspace(1, N, npix) - K.TICKET_BYTES) // K.BM_SLAB_BYTES == P
    p, t = K.bm_pair(7 * N + npix, N, npix, nan_frac=0.2)
    want = K.bm_statement(p, t)
    for skew in (1, 2, 3):
        got = run_bm([(p, t)], skew)
        check_bm(got[0], p, t, "plan N=%d npix=%d Ws=%d skew=%d" % (N, npix, Ws, skew))
    assert want[0][0] < N * npix


@pytest.mark.parametrize("shape", list(K.BM_RANK_SHAPES))
def test_batch_metrics_rank_parting(shape):
    """the two middle ranks part in pass 1, 2, 3 or never; one call for all rows of a shape (G = 6 pairs)"""
    names = list(K.BM_RANK_ROWS)
    pairs = [K.bm_rank_pair(n, shape) for n in names]
    for skew in (0, 1):
        got = run_bm(pairs, skew)
        for g, n in enumerate(names):
            check_bm(got[g], *pairs[g], "rank %s %s skew=%d" % (n, shape, skew))
    vals = K.BM_RANK_ROWS["pass3"][0]
    if not K.BM_RANK_SHAPES[shape][2]:
        assert got[names.index("pass3"), 8] == float(F32((F32(vals[2]) + F32(vals[3])) * F32(0.5))) and got[names.index("pass1"), 8] == 0.375


@pytest.mark.parametrize("shape", [(1, 6), (2, 3)])
def test_batch_metrics_key_extremes(shape):
    """+0, a denormal, FLT_MAX / 2 beside its neighbour and +inf as the middle elements: bins 0 and 2040 of the first histogram"""
    names = list(K.BM_EXTREME_ROWS)
    pairs = [(p.reshape(shape), t.reshape(shape)) for p, t in K.BM_EXTREME_ROWS.values()]
    got = run_bm(pairs, 2)
    for g, n in enumerate(names):
        check_bm(got[g], *pairs[g], "extreme %s %s" % (n, shape))
        assert got[g, 0] == got[g, 1] == 6
    assert got[names.index("zero"), 8] == 0 and np.isposinf(got[names.index("inf"), 8]) and 0 < got[names.index("denormal"), 8] < 1.2e-38


def refused(name, *args, also=()):
    call(name, *args, rc=BADARG)
    for b in also:
        b._host = None
        b.check(name, untouched=True)


def test_batch_metrics_argument_checks():
    L = lib()
    N, npix = 2, 5
    p, t = K.bm_pair(1, N, npix)
    pin, tin = fmap(p, K.POISON_P), fmap(t, K.POISON_T)
    ptab, ttab = G.pointer_table([pin]), G.pointer_table([tin])
    ws = G.workspace(L.ramnet_batch_metrics_workspace(1, N, npix), K.TICKET_BYTES)
    out = Out(1, 10, dtype=F64)
    both = (ws, out)
    name = "ramnet_batch_metrics"
    refused(name, None, ttab, 1, N, npix, ws, out)
    refused(name, ptab, None, 1, N, npix, ws, out)
    refused(name, ptab, ttab, 1, N, npix, None, out, also=both)
    refused(name, ptab, ttab, 1, N, npix, ws, None, also=both)
    refused(name, ptab, ttab, 1, N, npix, ws.ptr + 128, out, also=both)          # workspace off 256 bytes
    refused(name, ptab, ttab, 1, N, npix, ws, out.ptr + 4, also=both)            # out off 8 bytes
    refused(name, ptab, ttab, 1, 2, 1 << 30, ws, out)                            # N npix = 2^31
    refused(name, ptab, ttab, 65536, N, npix, ws, out)
    refused(name, ptab, ttab, 1, 65536, npix, ws, out)
    refused(name, ptab, ttab, 1, 0, npix, ws, out)
    refused(name, ptab, ttab, 1, N, 0, ws, out)
    refused(name, ptab, ttab, -1, N, npix, ws, out)
    call(name, ptab, ttab, 0, N, npix, ws, out)                                   # G = 0: nothing to do
    for b in both:
        b._host = None
        b.check(name, untouched=True)
    assert L.ramnet_batch_metrics_workspace(1, 2, 1 << 30) == 0 and L.ramnet_batch_metrics_workspace(65536, N, npix) == 0
    assert L.ramnet_batch_metrics_workspace(1, 65536, npix) == 0 and L.ramnet_batch_metrics_workspace(1, N, 0) == 0
    got = run_bm([(p, t)])                                                       # and the valid call on the same arguments
    check_bm(got[0], p, t, "after the refusals")


# ================================================================================================ evaluation table
def run_et(ps, ts, ms, cutoffs, flags, skew=0, clip=K.CLIP, reg=K.REG):
    """One table of G maps -> [G, V, 16]; flags = 0: ramnet_eval_table, then ramnet_eval_table_ex on the dirty workspace; else _ex twice.
    ms: None, or a list with None entries (NULL in the table)."""
    Gn, npix, has_mask, ncut = len(ps), int(np.asarray(ps[0]).size), ms is not None, len(cutoffs)
    V = (1 + ncut) * (2 if has_mask else 1)
    pin = [fmap(p, K.POISON_P, skew) for p in ps]
    tin = [fmap(t, K.POISON_T, (skew + g + 1) % 4 if skew else 0) for g, t in enumerate(ts)]
    mtab, min_ = None, []
    if has_mask:
        min_ = [0 if m is None else bmask(m, (skew + g) % 4 if skew else 0) for g, m in enumerate(ms)]       # (a NULL entry: all inside)
        mtab = G.pointer_table(min_, through_kernel=True)
    ptab, ttab = G.pointer_table(pin), G.pointer_table(tin, tail=2)
    L = lib()
    nbytes = L.ramnet_eval_table_ex_workspace(Gn, npix, ncut, int(has_mask), flags)
    assert nbytes == K.et_workspace_bytes(Gn, npix, ncut, has_mask, flags)
    assert flags & K.RESCALE or nbytes == L.ramnet_eval_table_workspace(Gn, npix, ncut, int(has_mask))
    ws = G.workspace(nbytes, K.TICKET_BYTES)
    cut = (C.c_float * max(ncut, 1))(*[float(c) for c in cutoffs])
    outs = []
    for rep in range(2):
        out = Out(Gn * V, 16, dtype=F64)
        if flags == 0 and rep == 0:
            call("ramnet_eval_table", ptab, ttab, mtab, Gn, npix, clip, reg, cut, ncut, ws, out)
        else:
            call("ramnet_eval_table_ex", ptab, ttab, mtab, Gn, npix, clip, reg, cut, ncut, flags, ws, out)
        assert G.tickets_zero(ws), "the table left a ticket behind"
        outs.append(out.value().numpy())
    assert outs[0].tobytes() == outs[1].tobytes(), "a second call on the dirty workspace gives other bytes"
    assert not (outs[0] == G.SENT).any() and len(pin) == len(tin) == Gn and len(min_) in (0, Gn)      # (the inputs live until here)
    return outs[0].reshape(Gn, V, 16)


def et_inputs(ps, ts, flags, clip=K.CLIP, reg=K.REG):
    """the float32 metric maps the statement is fed: ramnet_metric_depth's own (test_table_converts_with_the_bits_of_metric_depth ties the
    table kernels to it)"""
    def convert(xs, clamp):                                                     # (one launch for all maps)
        xs = [np.asarray(x, F32) for x in xs]
        flat = metric_depth(np.concatenate([x.ravel() for x in xs]), clamp, clip, reg)
        return [a.reshape(x.shape) for a, x in zip(np.split(flat, np.cumsum([x.size for x in xs])[:-1]), xs)]
    return [np.asarray(t, F32) for t in ts] if flags & K.TARGET_METRIC else convert(ts, 0), convert(ps, 1)


def check_et(got, tm, pm, mask, cutoffs, flags, tag):
    want, bound = K.et_statement(tm.ravel(), pm.ravel(), None if mask is None else np.asarray(mask).ravel(), cutoffs, flags)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    exact = [0, 1, 8, 9, 10, 13, 14, 15]
    assert np.array_equal(got[:, exact], want[:, exact]), (tag, "counts", got[:, exact].tolist(), want[:, exact].tolist())
    assert K.same_class(got[:, 2:8], want[:, 2:8]) and K.same_class(got[:, 11:13], want[:, 11:13]), (tag, "non-finite cells", got.tolist(), want.tolist())
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)                                                # (inf - inf in the non-finite cells, compared above)
    for rule, cols in (("sums", [2, 3, 4, 7]), ("log sums", [5, 6])):
        f = fin[:, cols]
        note("eval_table%s %s" % (" rescaled" if flags & K.RESCALE else "", rule), err[:, cols][f], bound[:, cols][f])
        assert np.all(err[:, cols][f] <= bound[:, cols][f]), (tag, rule, np.max(err[:, cols][f] / np.maximum(bound[:, cols][f], 1e-300)))
    if flags & K.RESCALE:
        f = fin[:, 11:13]
        assert np.all(err[:, 11:13][f] <= bound[:, 11:13][f]), (tag, "medians of the transformed maps")
    else:
        assert f32_bits_equal(got[:, 11:13], want[:, 11:13]), (tag, "medians", got[:, 11:13].tolist(), want[:, 11:13].tolist())


def run_and_check(ps, ts, ms, cutoffs, flags, skew, tag):
    """ts: normalised log depth; under TARGET_METRIC the table is given ramnet_metric_depth's float32 metric depths of them"""
    tm, pm = et_inputs(ps, ts, 0)
    got = run_et(ps, tm if flags & K.TARGET_METRIC else ts, ms, cutoffs, flags, skew)
    for g in range(len(ps)):
        check_et(got[g], tm[g], pm[g], None if ms is None else K.et_mask(ms[g], np.asarray(ps[g]).shape), cutoffs, flags,
                 "%s flags=%d skew=%d g=%d" % (tag, flags, skew, g))
    return got


def test_log_ulps_measured_through_the_kernel():
    """one-pixel maps: column 6 is a single |log(t + 1e-5) - log(p + 1e-5)| of the device's double log; against numpy's, in units of
    2^-53 (|log(t + 1e-5)| + |log(p + 1e-5)|)"""
    worst = 0.0
    for seed in range(4):
        rng = np.random.default_rng(seed)
        tm = np.exp(rng.uniform(np.log(0.01), np.log(80.0), 4096)).astype(F32)
        pn = K.norm_of(np.clip(tm.astype(np.float64) * rng.uniform(0.5, 2.0, 4096), 2.0, 80.0))
        pm = metric_depth(pn, 1)
        got = run_et([pn[i:i + 1] for i in range(4096)], [tm[i:i + 1] for i in range(4096)], None, (), K.TARGET_METRIC, skew=seed)[:, 0]
        assert np.array_equal(got[:, 11].astype(F32), tm) and np.array_equal(got[:, 12].astype(F32), pm)
        lt, lp = np.log(tm.astype(np.float64) + R.EPS), np.log(pm.astype(np.float64) + R.EPS)
        unit = K.U53 * (np.abs(lt) + np.abs(lp))
        worst = max(worst, float(np.max(np.abs(got[:, 6] - np.abs(lt - lp)) / unit)))
        print("seed %d: device log against numpy %.3f units at most so far; column 5: %.3f of its bound" % (seed, worst, float(np.max(
            np.abs(got[:, 5] - (lt - lp) ** 2) / (2 * np.abs(lt - lp) * K.LOG_ULPS * unit + (K.LOG_ULPS * unit) ** 2 + K.U53 * (lt - lp) ** 2)))))
        assert np.all(np.abs(got[:, 5] - (lt - lp) ** 2) <= 2 * np.abs(lt - lp) * K.LOG_ULPS * unit + (K.LOG_ULPS * unit) ** 2 + K.U53 * (lt - lp) ** 2)
    print("device log against numpy: %.3f x 2^-53 (|log t| + |log p|) at most over 16384 pixels; LOG_ULPS = %.1f" % (worst, K.LOG_ULPS))
    WORST["LOG_ULPS measured"] = worst
    assert worst + 1.0 <= K.LOG_ULPS, worst


@pytest.mark.parametrize("tag", list(K.ET_CAP_ROWS))
@pytest.mark.parametrize("flags", [0, K.RESCALE])
def test_eval_table_workgroup_cap(tag, flags):
    """32 workgroups per cell: the first size at the cap and one beyond it with a ragged tail; rescaled: the row stage full (32 x 16 doubles)"""
    npix = K.ET_CAP_ROWS[tag]
    assert K.et_plan(npix, 1, True) == (4, 32)
    ps, ts, ms = K.et_pairs(npix % 1000, 1, (1, npix), nan_frac=0.1)
    tm, pm = et_inputs(ps, ts, 0)
    for skew in (1, 2, 3):
        got = run_et(ps, ts, ms, (20.0,), flags, skew)
        if skew == 1:
            check_et(got[0], tm[0], pm[0], ms[0], (20.0,), flags, "%s flags=%d" % (tag, flags))
            first = got
        assert got.tobytes() == first.tobytes()
    assert np.isnan(got[0, :2, 11]).all() and np.isfinite(got[0, 2:, 2:13]).all() and got[0, 0, 0] == npix > got[0, 0, 1]


@pytest.mark.parametrize("flags", K.FLAG_SETS)
@pytest.mark.parametrize("shape", [(3, 5), (37, 53)])
def test_eval_table_eight_cutoffs_with_masks(shape, flags):
    ps, ts, ms = K.et_pairs(shape[0] + flags, 2, shape, nan_frac=0.1)
    ts[1] = np.where(np.isnan(ts[1]), F32(0.5), ts[1])                          # pair 1 keeps finite medians in every variant
    got = run_and_check(ps, ts, ms, K.CUT8, flags, 1 + flags % 3, "ncut8 %dx%d" % shape)
    assert got.shape == (2, 18, 16)


@pytest.mark.parametrize("flags", [0, K.RESCALE | K.TARGET_METRIC])
def test_eval_table_5400_cells(flags):
    """G = 300, V = 18: tickets and states far from index 0"""
    ps, ts, ms = K.et_pairs(300 + flags, 300, (3, 5), nan_frac=0.05)
    ms[7] = None
    got = run_and_check(ps, ts, ms, K.CUT8, flags, 3, "G300")
    assert got.shape == (300, 18, 16) and np.isfinite(got[:, :, 11]).sum() > 1000


def test_table_converts_with_the_bits_of_metric_depth():
    """4096 one-pixel maps: column 11 is the metric target, column 12 the clamped metric prediction of the pixel"""
    y = K.conversion_values()
    maps = [y[i:i + 1] for i in range(y.size)]
    got = run_et(maps, maps, None, (), 0, skew=1)[:, 0]
    for col, clamp in ((11, 0), (12, 1)):
        want = metric_depth(y, clamp, skew=2)
        assert np.array_equal(got[:, col].astype(F32).view(np.uint32), want.view(np.uint32)), "column %d is not ramnet_metric_depth(clamp=%d)" % (col, clamp)
        assert np.array_equal(got[:, col].astype(F32).astype(np.float64), got[:, col])
    lo = F32(np.exp(F32(-K.REG)) * F32(K.CLIP))
    assert got[:, 12].max() == K.CLIP and abs(got[:, 12].min() - lo) <= 1e-6 * lo and got[:, 11].max() > 400 and (got[:, 0] == 1).all()


def test_eval_table_cutoff_is_strict_and_a_nan_target_is_inside():
    cut = (10.0, 30.0)
    tm = K.cutoff_targets(cut)
    rng = np.random.default_rng(5)
    ps = [rng.random(tm.size).astype(F32) for _ in range(2)]
    ts = [tm, tm[::-1].copy()]
    pm = [metric_depth(p, 1) for p in ps]
    for flags in (K.TARGET_METRIC, K.TARGET_METRIC | K.RESCALE):
        got = run_et(ps, ts, [np.ones(tm.size, np.uint8), None], cut, flags, skew=2)
        for g in range(2):
            check_et(got[g], ts[g], pm[g], np.ones(tm.size, np.uint8), cut, flags, "cutoff g=%d flags=%d" % (g, flags))
            assert got[g, 0, 0] == tm.size and got[g, 1, 0] == 3 and got[g, 1, 1] == 2        # 1, nextafter(10, 0) and the NaN: 10 itself is outside
            assert got[g, 2, 0] == 6 and got[g, 2, 1] == 5 and np.array_equal(got[g, 3:, :2], got[g, :3, :2])
    # a NaN-free sibling: the medians show the strictness too
    t2 = np.array([10.0, np.nextafter(F32(10), F32(0)), 5.0, np.nextafter(F32(10), F32(99)), 30.0, np.nextafter(F32(30), F32(0))], F32)
    got = run_et([ps[0][:6]], [t2], None, cut, K.TARGET_METRIC, skew=3)
    check_et(got[0], t2, pm[0][:6], None, cut, K.TARGET_METRIC, "cutoff medians")
    assert got[0, 1, 0] == 2 and got[0, 1, 11] == float(F32((F32(5) + np.nextafter(F32(10), F32(0))) * F32(0.5))) and got[0, 2, 0] == 5


@pytest.mark.parametrize("npix", [1, 2, 3, 5, 6, 7, 15, 1031])
def test_eval_table_mask_bytes(npix):
    """mask bytes 0, 1, 2, 128, 255; an all-zero mask; a NULL entry beside non-NULL ones; the byte-quad load and its tail, masks skewed by 1..3 bytes"""
    rng = np.random.default_rng(npix)
    ps, ts, _ = K.et_pairs(npix, 4, (1, npix))
    ms = [np.array([0, 1, 2, 128, 255], np.uint8)[rng.integers(0, 5, npix)], None, np.zeros(npix, np.uint8),
          np.array([2, 128, 255, 0], np.uint8)[np.arange(npix) % 4]]
    for flags, skew in ((0, 1), (K.RESCALE, 2), (K.TARGET_METRIC, 3)):
        got = run_and_check(ps, ts, ms, (20.0,), flags, skew, "mask bytes npix=%d" % npix)
        assert (got[2, 2:, :2] == 0).all() and np.isnan(got[2, 2:, 11:13]).all() and got[1, 2:].tobytes() == got[1, :2].tobytes()
        assert got[3, 2, 0] == np.count_nonzero(ms[3]) and got[0, 2, 0] == np.count_nonzero(ms[0])


@pytest.mark.parametrize("name", list(K.ET_STREAM_ROWS))
def test_eval_table_streams_part_independently(name):
    tm, pn, pass_t, pass_p = K.ET_STREAM_ROWS[name]
    pm = metric_depth(pn, 1)
    assert K.parting_pass(tm) == pass_t and K.parting_pass(pm) == pass_p
    for n in (6, 5):
        for flags in (K.TARGET_METRIC, K.TARGET_METRIC | K.RESCALE):
            got = run_et([pn[:n], pn[:n][::-1].copy()], [tm[:n], tm[:n][::-1].copy()], None, (), flags, skew=n - 4)
            check_et(got[0], tm[:n], pm[:n], None, (), flags, "%s n=%d flags=%d" % (name, n, flags))
            check_et(got[1], tm[:n][::-1], pm[:n][::-1], None, (), flags, "%s reversed n=%d flags=%d" % (name, n, flags))


def test_eval_table_zero_metric_target():
    """TARGET_METRIC: metric targets are >= 0 and the caller owes that (include/ramnet_hip.h); +0 is the smallest key"""
    tm = np.array([0.0, 0.0, 0.0, 5.0, 0.0, 7.0], F32)
    pn = np.array([0.2, 0.5, 0.7, 0.4, 0.9, 0.3], F32)
    pm = metric_depth(pn, 1)
    for n in (6, 5):
        got = run_et([pn[:n]], [tm[:n]], None, (1.0,), K.TARGET_METRIC, skew=1)
        check_et(got[0], tm[:n], pm[:n], None, (1.0,), K.TARGET_METRIC, "zero target n=%d" % n)
        assert got[0, 0, 11] == 0 and got[0, 1, 0] == 4 and np.isfinite(got[0, :, 2:8]).all()


def test_eval_table_argument_checks():
    L = lib()
    npix, ncut = 15, 2
    ps, ts, ms = K.et_pairs(3, 1, (3, 5))
    ins = [fmap(ps[0], K.POISON_P), fmap(ts[0], K.POISON_T), bmask(ms[0])]
    ptab, ttab, mtab = [G.pointer_table([b]) for b in ins]
    ws = G.workspace(L.ramnet_eval_table_ex_workspace(1, npix, ncut, 1, 3), K.TICKET_BYTES)
    out = Out(6, 16, dtype=F64)
    both = (ws, out)
    cut = (C.c_float * 2)(10.0, 30.0)

    def ex(pred=ptab, target=ttab, mask=mtab, Gn=1, n=npix, clip=K.CLIP, cutoffs=cut, nc=ncut, flags=0, w=ws, o=out):
        refused("ramnet_eval_table_ex", pred, target, mask, Gn, n, clip, K.REG, cutoffs, nc, flags, w, o, also=both)
        if flags == 0:
            refused("ramnet_eval_table", pred, target, mask, Gn, n, clip, K.REG, cutoffs, nc, w, o, also=both)

    ex(pred=None), ex(target=None), ex(w=None), ex(o=None), ex(cutoffs=None)
    ex(w=ws.ptr + 128), ex(o=out.ptr + 4)
    ex(Gn=0), ex(Gn=65536), ex(Gn=-1), ex(n=0), ex(n=1 << 32)
    ex(nc=9), ex(nc=-1)
    for bad in ((10.0, 10.0), (30.0, 10.0), (0.0, 5.0), (-1.0, 5.0), (float("nan"), 5.0)):
        ex(cutoffs=(C.c_float * 2)(*bad))
    ex(flags=4), ex(flags=8), ex(flags=7), ex(flags=-1)
    ex(clip=0.0), ex(clip=-1.0)
    # more cells than tickets: 3641 x 18 = 65538 > 65536 (every table entry is the one valid map: nothing is launched)
    big = [G.pointer_table([tab.value()[0, 0].item()] * 3641) for tab in (ptab, ttab, mtab)]
    ex(pred=big[0], target=big[1], mask=big[2], Gn=3641, cutoffs=(C.c_float * 8)(*K.CUT8), nc=8)
    assert L.ramnet_eval_table_workspace(3641, npix, 8, 1) == 0 and L.ramnet_eval_table_ex_workspace(1, npix, 2, 1, 4) == 0
    assert L.ramnet_eval_table_workspace(1, npix, 9, 1) == 0 and L.ramnet_eval_table_workspace(1, 0, 2, 1) == 0 and L.ramnet_eval_table_workspace(65536, npix, 0, 0) == 0
    got = run_and_check(ps, ts, ms, (10.0, 30.0), 3, 0, "after the refusals")
    assert got.shape == (1, 6, 16)


# ================================================================================================ resize and metric depth
@pytest.mark.parametrize("H,W,s", K.RESIZE_ROWS)
def test_resize_metric_target(H, W, s):
    Ho, Wo = int(np.floor(H * s)), int(np.floor(W * s))
    rng = np.random.default_rng(H * 100 + W)
    ts = rng.random((3, H, W)).astype(F32)
    ts[1][rng.random((H, W)) < 0.2] = np.nan
    ts[2, H // 2, W // 2] = np.nan
    tin = [fmap(ts[g], K.POISON_T, skew=g + 1) for g in range(3)]
    ttab = G.pointer_table(tin, through_kernel=True)
    if Ho == 0 or Wo == 0:
        out = Out(3, 4)
        call("ramnet_resize_metric_target", ttab, 3, H, W, s, K.CLIP, K.REG, out, rc=BADARG)
        return
    out = Out(3, Ho * Wo)                                                       # exactly G H' W' floats
    call("ramnet_resize_metric_target", ttab, 3, H, W, s, K.CLIP, K.REG, out)
    got = out.value().numpy().reshape(3, Ho, Wo)
    for g in range(3):
        md = metric_depth(ts[g], 0, skew=3 - g)
        want = K.resize_statement(md, s)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got[g]), nan), (H, W, s, g)
        assert np.array_equal(got[g][~nan].view(np.uint32), want[~nan].view(np.uint32)), (H, W, s, g, float(np.max(np.abs(got[g][~nan] - want[~nan]))))
        if s == 1.0:
            assert g > 0 or np.array_equal(got[g].view(np.uint32), md.view(np.uint32))          # the NaN-free map: ramnet_metric_depth itself
            assert nan.sum() >= np.isnan(ts[g]).sum() and (g != 2 or nan.sum() == 4)             # a NaN tap at weight zero still makes the output NaN
    assert np.isfinite(got[0]).all()


def test_resize_and_metric_depth_argument_checks():
    ts = np.random.default_rng(1).random((1, 4, 6)).astype(F32)
    tin = fmap(ts[0], K.POISON_T)
    ttab = G.pointer_table([tin])
    out = Out(1, 24)
    name = "ramnet_resize_metric_target"
    refused(name, None, 1, 4, 6, 0.5, K.CLIP, K.REG, out)
    refused(name, ttab, 1, 4, 6, 0.5, K.CLIP, K.REG, None, also=(out,))
    for s in (1.0000001, 2.0, 0.0, -0.5, float("nan"), 0.2):                    # 0.2: floor(4 x 0.2) = 0
        refused(name, ttab, 1, 4, 6, s, K.CLIP, K.REG, out)
    refused(name, ttab, 0, 4, 6, 0.5, K.CLIP, K.REG, out)
    refused(name, ttab, 65536, 4, 6, 0.5, K.CLIP, K.REG, out)
    refused(name, ttab, 1, 0, 6, 0.5, K.CLIP, K.REG, out)
    refused(name, ttab, 1, 4, 6, 0.5, 0.0, K.REG, out)
    y = fmap(ts[0], K.POISON_P)
    refused("ramnet_metric_depth", None, 24, K.CLIP, K.REG, 0, out)
    refused("ramnet_metric_depth", y, 24, K.CLIP, K.REG, 0, None, also=(out,))
    refused("ramnet_metric_depth", y, 0, K.CLIP, K.REG, 0, out)
    refused("ramnet_metric_depth", y, 24, 0.0, K.REG, 0, out)
    refused("ramnet_metric_depth", y, 24, -1.0, K.REG, 1, out)


@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 777])
def test_metric_depth_guarded(n):
    """one element, either side of a workgroup, and beyond the first trip of the 4096 x 256 grid; against float64 exp at 1e-6 relative"""
    rng = np.random.default_rng(n)
    y = rng.uniform(-0.5, 1.5, n).astype(F32)
    y[5::97] = np.nan
    reg64, lo = float(F32(K.REG)), np.exp(-float(F32(K.REG))) * K.CLIP
    for clamp, skew in ((0, 1), (1, 2), (1, 3)):
        got = metric_depth(y, clamp, skew=skew)
        want = np.exp(reg64 * (y.astype(np.float64) - 1.0)) * K.CLIP
        if clamp:
            want = np.clip(want, lo, K.CLIP)
        nan = np.isnan(y)
        assert np.array_equal(np.isnan(got), nan)
        err = np.abs(got.astype(np.float64) - want)[~nan]
        note("metric_depth", err, 1e-6 * want[~nan])
        assert np.all(err <= 1e-6 * want[~nan]), (n, clamp, float(np.max(err / want[~nan])))
        assert n < 255 or not clamp or (got[~nan].max() == K.CLIP and got[~nan].min() >= F32(lo) * (1 - 1e-6))


def test_zz_report_largest_error_over_bound():
    for k in sorted(WORST):
        print("largest error / bound, %s: %.4f" % (k, WORST[k]))
