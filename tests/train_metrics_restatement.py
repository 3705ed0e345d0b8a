"""Float64 restatement of the training metrics (RAM_Net/model/metric.py:8-54) for the tests, and the seeded pairs they share with
tests/golden/make_golden_train_metrics.py.

Element arithmetic stays in float32 exactly as numpy performs it on float32 arrays (|t - p|, d / (t + 1e-6), d * d / (t * t + 1e-6));
only the SUMS are taken in float64.  So the restatement differs from the reference by the reference's own float32 summation error and
from the HIP reduction by the order of a float64 sum.  The median is found on the uint32 bit patterns of the non-NaN d (d >= +0: the
pattern orders like the value), independently of np.median."""
import numpy as np

NAMES = ("mse", "abs_rel_diff", "squ_rel_diff", "rms_linear", "scale_invariant_error", "mean_error", "median_error")
EPS = np.float32(1e-6)


def _mean64(x):
    return np.float64(np.sum(x.astype(np.float64))) / x.size if x.size else np.float64("nan")


def restate(pred, target):
    """dict: the seven metrics (float64; median_error the float32 value widened) + 'n', 'n_target' + 'mean_d2' (scale of the SI bound)."""
    p, t = np.ascontiguousarray(pred, np.float32), np.ascontiguousarray(target, np.float32)
    assert p.shape == t.shape and p.ndim == 4 and p.shape[1] == 1
    with np.errstate(all="ignore"):
        d = np.abs(t - p)
        vd, vt = ~np.isnan(d), ~np.isnan(t)
        dv, tv = d[vd], t[vd]
        d2 = dv * dv
        out = {"n": int(vd.sum()), "n_target": int(vt.sum())}
        mse = np.float64(0.0)
        for i in range(p.shape[0]):
            e = (p[i, 0] - t[i, 0])[vt[i, 0]]
            mse += _mean64(e * e)
        out["mse"] = mse / p.shape[0]
        out["abs_rel_diff"] = _mean64(dv / (tv + EPS))
        out["squ_rel_diff"] = _mean64(d2 / (tv * tv + EPS))
        m2, m1 = _mean64(d2), _mean64(dv)
        out["rms_linear"] = np.sqrt(m2)
        out["scale_invariant_error"] = m2 - m1 * m1
        out["mean_error"] = m1
        out["mean_d2"] = m2
        n = dv.size
        if n == 0:
            out["median_error"] = np.float64("nan")
        else:
            bits = np.sort(dv.view(np.uint32))
            a, b = bits[(n - 1) // 2:(n - 1) // 2 + 1].view(np.float32)[0], bits[n // 2:n // 2 + 1].view(np.float32)[0]
            out["median_error"] = np.float64(a if n % 2 else np.float32((a + b) * np.float32(0.5)))
    return out


def seeded_pair(seed, shape, nan_frac, parity=None, quantised=False):
    """(prediction, target) float32 N x 1 x H x W in [0, 1], a fraction of the targets NaN.  parity: force the count of valid pixels
    odd (1) or even (0).  quantised: |t - p| takes the 16 values k / 32, so the middle ranks sit inside runs of equal elements."""
    rng = np.random.default_rng(seed)
    if quantised:
        t = (0.25 + rng.integers(0, 16, size=shape) / 32.0).astype(np.float32)
        p = np.full(shape, 0.25, np.float32)
    else:
        t = (rng.random(shape, dtype=np.float32) * np.float32(0.9) + np.float32(0.05)).astype(np.float32)
        p = np.clip(t + np.float32(0.05) * rng.standard_normal(shape, dtype=np.float32), 0, 1).astype(np.float32)
    if nan_frac:
        t[rng.random(shape) < nan_frac] = np.nan
    if parity is not None and int((~np.isnan(t)).sum()) % 2 != parity:
        flat = t.reshape(-1)
        flat[np.flatnonzero(~np.isnan(flat))[0]] = np.nan
    return p, t


# tag -> (seed, shape, nan_frac, parity, quantised); the pairs of tests/golden/train_metrics.npz
SMALL_CASES = {
    "n1_odd": (31, (1, 1, 7, 9), 0.0, 1, False),
    "n3_even": (32, (3, 1, 10, 12), 0.0, 0, False),
    "n3_nan20_odd": (33, (3, 1, 10, 12), 0.2, 1, False),
    "n3_nan20_even": (34, (3, 1, 10, 12), 0.2, 0, False),
    "n1_nan90": (35, (1, 1, 16, 20), 0.9, None, False),
    "n3_nan90": (36, (3, 1, 12, 14), 0.9, None, False),
    "n3_ties_even": (37, (3, 1, 10, 12), 0.2, 0, True),
    "n1_ties_odd": (38, (1, 1, 9, 11), 0.0, 1, True),
    "n3_tail": (39, (3, 1, 7, 11), 0.2, None, False),          # N * npix = 231: not a multiple of 4
}
FULL_CASES = {
    "full_8x256x344_nan20": (101, (8, 1, 256, 344), 0.2, None, False),
    "full_2x260x346_nan20": (102, (2, 1, 260, 346), 0.2, None, False),
    "full_8x256x344": (103, (8, 1, 256, 344), 0.0, None, False),
}


def case_pair(tag):
    return seeded_pair(*{**SMALL_CASES, **FULL_CASES}[tag])
