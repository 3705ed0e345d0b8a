"""The rows of tests/test_hip_metric_launch.py (the launches of csrc/metrics.hip through tests/guarded.py), their float64 statements
with per-cell bounds, and the launch plans restated from include/ramnet_hip.h.  tests/test_metric_launch_cases_cpu.py asserts without a
GPU that every row reaches the branch its name says (profiles/metric_launch_tests_notes.md).

The statements are train_metrics_restatement.restate, eval_table_restatement.restate_rows and eval_rescale_restatement; this file adds
the bounds: kernel and statement add the same float64 terms in another order, so a sum differs by at most (n - 1) 2^-53 sum|term|."""
import numpy as np

import eval_rescale_restatement as RS
import eval_table_restatement as R
import train_metrics_restatement as TM

F32 = np.float32
U53 = 2.0 ** -53
POISON_P, POISON_T = F32(3e38), F32(2.5e38)       # finite guards of the prediction / target maps: a NaN guard would read as "no ground truth"
CLIP, REG = 80.0, 3.70378
TICKET_BYTES = 262144
BM_SPAN, BM_STAGE, BM_MAX_PER_PAIR, BM_SLAB_BYTES = 8192, 64, 32, 16384
ET_SPAN, ET_MAX_PER_MAP, ET_SLAB_BYTES, ET_MAX_CELLS = 16384, 32, 16384, TICKET_BYTES // 4
RESCALE, TARGET_METRIC = 1, 2
# Device double log against numpy's, in units of 2^-53 (|log(t + 1e-5)| + |log(p + 1e-5)|) of one |ld| term: measured on the MI355X through
# column 6 of 16384 one-pixel maps (test_log_ulps_measured_through_the_kernel; notes section 2) 2.240 at most, plus 1 of margin (numpy's
# log is itself only faithful).  The measured value exceeds 2: an ulp of a log is up to two of these units, and the term holds two logs
# and a subtraction.
LOG_ULPS = 3.25
REL_RESCALED = 1e-10        # sums of a RESCALED row: tests/test_hip_eval_rescale.py's rule (the terms themselves move with the order of the
#                             sums behind mean and std; 2.2e-14 measured, profiles/eval_rescale_notes.md)


def bits(x):
    return np.asarray(x, F32).view(np.uint32)


def from_bits(b):
    return np.asarray(b, np.uint32).view(F32)


def r256(x):
    return (x + 255) & ~255


# ------------------------------------------------------------------------------------------------ plans
def bm_plan(N, npix):
    """(Ws, P) of ramnet_batch_metrics: Ws = min(ceil(npix / 8192), floor(32 / N) for N < 32, else 1)."""
    ws = min(-(-npix // BM_SPAN), 1 if N >= BM_MAX_PER_PAIR else BM_MAX_PER_PAIR // N)
    ws = max(ws, 1)
    return ws, N * ws


def bm_workspace_bytes(G, N, npix):
    P = bm_plan(N, npix)[1]
    return TICKET_BYTES + r256(G * 32) + r256(G * P * 64) + G * P * BM_SLAB_BYTES


def et_plan(npix, ncut, has_mask):
    """(V, Ws) of the evaluation table."""
    return (1 + ncut) * (2 if has_mask else 1), min(-(-npix // ET_SPAN), ET_MAX_PER_MAP)


def et_workspace_bytes(G, npix, ncut, has_mask, flags=0):
    V, Ws = et_plan(npix, ncut, has_mask)
    cells, rs = G * V, bool(flags & RESCALE)
    return TICKET_BYTES + r256(cells * 48) + r256(cells * Ws * (16 if rs else 12) * 8) + cells * Ws * ET_SLAB_BYTES + (cells * 64 if rs else 0)


def parting_pass(values):
    """The pass in which the two middle ranks of the non-NaN values part: 1 (bits 30..20), 2 (19..10), 3 (9..0), 0 never (equal, or odd)."""
    b = np.sort(bits(values)[~np.isnan(np.asarray(values, F32))] & np.uint32(0x7fffffff))
    n = b.size
    lo, hi = int(b[(n - 1) // 2]), int(b[n // 2])
    return 1 if lo >> 20 != hi >> 20 else 2 if lo >> 10 != hi >> 10 else 3 if lo != hi else 0


# ------------------------------------------------------------------------------------------------ ramnet_batch_metrics: statement + bound
def bm_statement(p, t):
    """p / t [N][npix] float32 -> (row [10], bound [10]) of out[g]: 0 n, 1 n_target, 2 mse, 3 abs_rel, 4 squ_rel, 5 rms, 6 SI, 7 mean, 8 median.
    Every term is non-negative, so sum|term| = n x mean; the division by n and the statement's own division add 2^-53 each:
    (n + 1) 2^-53 mean.  rms: half of that of mean d^2 plus the two roots' roundings; SI: mean d^2 - (mean d)^2 carried through; mse: a
    sample's (n_s + 1) 2^-53, the N quotients added and divided once more.  A non-finite statement has bound 0: compared as it is."""
    N, npix = p.shape
    r = TM.restate(p.reshape(N, 1, 1, npix), t.reshape(N, 1, 1, npix))
    n = r["n"]
    row = np.array([n, r["n_target"], r["mse"], r["abs_rel_diff"], r["squ_rel_diff"], r["rms_linear"], r["scale_invariant_error"],
                    r["mean_error"], r["median_error"], 0.0])
    b = np.zeros(10)
    with np.errstate(all="ignore"):
        m1, m2 = r["mean_error"], r["mean_d2"]
        k = (n + 1) * U53
        b[2] = (npix + N + 2) * U53 * abs(r["mse"])
        b[3], b[4], b[7] = k * abs(row[3]), k * abs(row[4]), k * abs(m1)
        b[5] = (0.5 * k + 2 * U53) * abs(row[5])
        b[6] = k * m2 + 2 * k * m1 * m1 + 2 * U53 * (m2 + m1 * m1)
    b[~np.isfinite(row)] = 0.0
    return row, np.nan_to_num(b, nan=0.0, posinf=0.0)


def bm_pair(seed, N, npix, nan_sample=None, nan_frac=0.1):
    """(p, t) [N][npix]: a tenth of the targets NaN, every sample keeps a valid target except `nan_sample`, which has none."""
    rng = np.random.default_rng(seed)
    t = (rng.random((N, npix), dtype=F32) * F32(0.9) + F32(0.05)).astype(F32)
    p = np.clip(t + F32(0.05) * rng.standard_normal((N, npix), dtype=F32), 0, 1).astype(F32)
    t[rng.random((N, npix)) < nan_frac] = np.nan
    t[:, 0] = np.where(np.isnan(t[:, 0]), F32(0.5), t[:, 0])
    if nan_sample is not None:
        t[nan_sample] = np.nan
    return p, t


# (N, npix) -> the sample of the second chunk of staged rows without a valid target (P = 64: one full chunk, its last row)
BM_STAGE_ROWS = {(64, 5): 63, (65, 5): 64, (70, 7): 66, (128, 4): 100, (130, 3): 129}
# (N, npix) -> (Ws, P)
BM_PLAN_ROWS = {(16, 8193): (2, 32), (17, 8193): (1, 17), (32, 9): (1, 32), (33, 9): (1, 33), (5, 3 * 8192 + 5): (4, 20),
                (1, 32 * 8192 + 3): (32, 32)}

_Q = F32(0.25)
_Q2, _Q3 = from_bits(bits(_Q) | np.uint32(1 << 10)), from_bits(bits(_Q) + np.uint32(1))
# name -> (the six d of an even count, sorted; the pass in which ranks 2 and 3 part).  p = 0, so d = t exactly.
BM_RANK_ROWS = {
    "pass1": ([0.01, 0.02, _Q, 0.5, 1.0, 2.0], 1),
    "pass2": ([0.01, 0.02, _Q, _Q2, 1.0, 2.0], 2),
    "pass3": ([0.01, 0.02, _Q, _Q3, 1.0, 2.0], 3),
    "ties_inside": ([0.01, _Q, _Q, _Q, _Q, 2.0], 0),
    "ties_first": ([0.01, 0.02, _Q, _Q, _Q, 2.0], 0),            # rank 2 is rank 0 of the run
    "ties_last": ([0.01, _Q, _Q, _Q, 1.0, 2.0], 0),              # rank 3 is the last of the run
}
# shape tag -> (N, npix, odd).  n = 6: the sorted values at positions ORDER, so ranks 2 and 3 sit at elements 1 and 4: with N = 2 in different
# samples = different workgroups.  Odd siblings: a seventh, largest value (n = 7, one rank), with N = 2 an eighth element whose target is NaN.
BM_RANK_SHAPES = {"n6": (1, 6, False), "n7": (1, 7, True), "n6_two_wg": (2, 3, False), "n7_two_wg": (2, 4, True)}
ORDER = (5, 2, 0, 4, 3, 1)


def bm_rank_pair(name, shape):
    vals, _ = BM_RANK_ROWS[name]
    N, npix, odd = BM_RANK_SHAPES[shape]
    t = np.array([vals[i] for i in ORDER], F32)
    if odd:
        t = np.concatenate([t[:3], [F32(4.0)], t[3:]]).astype(F32)     # (N = 2: rank 2 stays in sample 0, rank 3 moves to sample 1)
    if t.size < N * npix:
        t = np.concatenate([t, [F32(np.nan)]]).astype(F32)
    assert t.size == N * npix
    return np.zeros((N, npix), F32), t.reshape(N, npix)


_M = F32(np.finfo(np.float32).max)
_H = F32(_M / F32(2))
_INF = F32(np.inf)
# name -> (p, t) of six pixels whose middle ranks are the key extremes of the histogram
BM_EXTREME_ROWS = {
    "zero": (np.array([0.3, 0.7, 0, 0.2, 0.9, 0], F32), np.array([0.3, 0.7, 1, 0.2, 0.9, 2], F32)),                     # d = +0 (p = t) four times
    "denormal": (np.zeros(6, F32), np.array([1e-40, 2.0, 0, 1e-42, 1.0, 2e-40], F32)),
    "fltmax_half": (np.zeros(6, F32), np.array([_H, 0.2, _M, np.nextafter(_H, F32(0)), 0.1, _M], F32)),
    "inf": (np.array([0, _INF, 0, _INF, 0, _INF], F32), np.array([0.1, 5, 0.3, 6, 0.2, 7], F32)),                       # +inf is the upper middle element
}


def same_class(got, want):
    """non-finite cells: NaN where the statement has NaN, the same infinity where it has one"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = ~np.isfinite(want)
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[bad & ~np.isnan(want)], want[bad & ~np.isnan(want)])


# ------------------------------------------------------------------------------------------------ evaluation table: statement + bound
def et_mask(m, shape):
    return np.ones(shape, bool) if m is None else np.asarray(m) != 0


def et_statement(tm, pm, mask, cutoffs, flags, log_ulps=LOG_ULPS):
    """tm / pm: float32 metric target / clipped metric prediction of one map -> (rows [V, 16], bounds [V, 16]).  Columns 2..7 of a plain
    row: (n - 1) 2^-53 sum|term| of the statement's own terms, + per term 2 |ld| delta + delta^2 (column 5) and delta (column 6),
    delta = log_ulps 2^-53 (|log(t + 1e-5)| + |log(p + 1e-5)|).  A rescaled row: REL_RESCALED.  Everything else is exact (bound 0)."""
    tm, pm = np.asarray(tm, F32), np.asarray(pm, F32)
    m = None if mask is None else np.asarray(mask) != 0
    if flags & RESCALE:
        rows = RS.restate_rescaled_rows(tm, pm, m, cutoffs)
        b = np.zeros_like(rows)
        b[:, 2:8] = REL_RESCALED * np.abs(np.nan_to_num(rows[:, 2:8], nan=0.0, posinf=0.0, neginf=0.0))
        b[:, 11:13] = REL_RESCALED * np.abs(np.nan_to_num(rows[:, 11:13], nan=0.0, posinf=0.0, neginf=0.0))
        return rows, b
    rows = R.restate_rows(tm, pm, m, cutoffs)
    b = np.zeros_like(rows)
    for v, inside in enumerate(R.variants(tm, m, cutoffs)):
        tv, pv = tm[inside], pm[inside]
        ok = ~np.isnan(tv)
        t, p = tv[ok].astype(np.float64), pv[ok].astype(np.float64)
        n = t.size
        if n == 0:
            continue
        with np.errstate(all="ignore"):
            d, lt, lp = t - p, np.log(t + R.EPS), np.log(p + R.EPS)
            ld = lt - lp
            delta = log_ulps * U53 * (np.abs(lt) + np.abs(lp))
            terms = [np.abs(d) / (t + 1e-6), d * d / (t * t + 1e-6), d * d, ld * ld, np.abs(ld), np.abs(d)]
            for c, x in enumerate(terms):
                assert np.sum(x) == rows[v, 2 + c] or np.isnan(rows[v, 2 + c])          # the statement's own terms
                b[v, 2 + c] = (n - 1) * U53 * np.sum(np.abs(x))
            b[v, 5] += np.sum(2 * np.abs(ld) * delta + delta * delta)
            b[v, 6] += np.sum(delta)
    return rows, np.nan_to_num(b, nan=0.0, posinf=0.0)


def et_pairs(seed, G, shape, nan_frac=0.0, mask_frac=0.3, clear=True):
    """normalised log depth maps as tests/test_hip_eval_rescale.py draws them; clear: the masks keep clear of the NaN targets"""
    rng = np.random.default_rng(seed)
    ps, ts, ms = [], [], []
    for _ in range(G):
        t = rng.random(shape).astype(F32)
        p = (t + 0.1 * rng.standard_normal(shape)).astype(F32)
        if nan_frac:
            t[rng.random(shape) < nan_frac] = np.nan
        m = rng.random(shape) < mask_frac
        if clear:
            m &= ~np.isnan(t)
        ps.append(p), ts.append(t), ms.append(m.astype(np.uint8))
    return ps, ts, ms


ET_CAP_ROWS = {"first_at_cap": 31 * 16384 + 1, "beyond_cap": 32 * 16384 + 7}
CUT8 = (5.0, 10.0, 20.0, 30.0, 40.0, 50.0, 60.0, 70.0)
FLAG_SETS = (0, TARGET_METRIC, RESCALE, RESCALE | TARGET_METRIC)


def conversion_values():
    """4096 normalised log depths over [-0.5, 1.5]: 0, 1, and the two clamp bounds (y = 0: the lower, y = 1: the upper) from either side"""
    y = np.linspace(-0.5, 1.5, 4096).astype(F32)
    edge = [F32(0), F32(1)]
    for e in (F32(0), F32(1)):
        edge += [np.nextafter(e, F32(-9)), np.nextafter(e, F32(9)), e - F32(1e-6), e + F32(1e-6)]
    y[1:1 + len(edge)] = edge
    return y


def cutoff_targets(cutoffs):
    """metric targets at, just below and just above each cut-off, a NaN and two plain values"""
    out = [F32(1.0), F32(np.nan), F32(100.0)]
    for c in cutoffs:
        c = F32(c)
        out += [c, np.nextafter(c, F32(0)), np.nextafter(c, _INF)]
    return np.array(out, F32)


def norm_of(metric, clip=CLIP, reg=REG):
    """the normalised log depth whose metric depth is about `metric`"""
    return (1.0 + np.log(np.asarray(metric, np.float64) / clip) / reg).astype(F32)


# name -> (metric targets (TARGET_METRIC), normalised predictions, parting pass of the targets, of the predictions), even counts;
# the odd siblings drop the last pixel.  Predictions tie by the clamp: >= 1 gives clip, far below 0 gives the lower bound.
def _b(x, add):
    return from_bits(bits(F32(x)) + np.uint32(add))


ET_STREAM_ROWS = {
    "target_pass1_pred_never": (np.array([2, 30, 4, 8, 50, 60], F32), np.array([1.5, 1.0, 2.0, 1.2, 3.0, 1.1], F32), 1, 0),
    "target_never_pred_pass1": (np.full(6, 10.0, F32), norm_of([2, 30, 4, 8, 50, 60]), 0, 1),
    "both_pass2_other_prefixes": (np.array([2, 50, _b(8, 3 << 10), 8, 3, 60], F32), norm_of([20.0, 70, 20.01, 75, 5, 6]), 2, 2),
    "target_never_low_clamp_ties": (np.full(6, 10.0, F32), np.array([-5, -3, -9, -4, -6, -7], F32), 0, 0),
}

RESIZE_ROWS = ((10, 10, 0.3), (10, 30, 0.7), (100, 7, 0.29), (9, 9, 1.0 / 3.0), (5, 8, 1.0), (1, 9, 0.5), (2, 2, 0.5), (37, 53, 0.75))


def resize_statement(md, s):
    """the four-tap formula in float64 on float32 metric depths, rounded once"""
    with np.errstate(all="ignore"):
        return RS.resize_bilinear(np.asarray(md, F32), s).astype(F32)
