"""Depth evaluation on device: metric depth from normalised log depth (RAM_Net/evaluation.py:74-96) and the error metrics
of `add_to_metrics` (evaluation.py:201-241, RAM_Net/model/metric.py:8-33) with the reference's key names, comparison
operators and epsilons; one fused HIP reduction per call (Abs-Rel is the accuracy half of the headline metric).  All ten rows of the
reference's table, NaN behaviour included: `RMS_log` and `median_diff` are plain `np.mean` / `np.median` over the masked pixels
(evaluation.py:214, 241), so ONE NaN target inside the mask makes them NaN, while the metric.py means skip it
(pinned by tests/golden/eval_metrics.npz, the reference's own `add_to_metrics` run on seeded maps).

The TRAINING metrics (model/metric.py:8-54 through LSTMTrainer._eval_metrics, lstm_trainer.py:100-106) are different functions, on the
normalised log-depth maps themselves: `batch_metrics` computes all of them for a whole list of (prediction, target) pairs in one HIP
reduction (exact median included) and leaves the table on the device; `eval_metrics` is the one-pair drop-in for `_eval_metrics`."""
import ctypes as C
import math

import torch

from . import _hip as H
from .ops import _p, _st


def depth_metrics(prediction, target, clip_distance, reg_factor, cutoff=float("inf")):
    """prediction / target: normalised log-depth tensors (any shape, same numel).  Pixels with metric target depth
    `nan_to_num(t) < cutoff` form the mask (evaluation.py:367); NaN targets are skipped by the means (metric.py) but stay in
    the denominator of the delta thresholds (`np.mean(ratio <= ...)`, evaluation.py:224-226)."""
    p = prediction.detach().float().contiguous()
    t = target.detach().to(p.device).float().contiguous()
    assert p.numel() == t.numel()
    out = torch.empty(11, device=p.device, dtype=torch.float64)
    H.check(H.lib().ramnet_depth_metrics(_p(p), _p(t), p.numel(), float(clip_distance), float(reg_factor),
                                         float(min(cutoff, 3.0e38)), _p(out), _st()), "ramnet_depth_metrics")
    n, nmask, ar, sr, se, l2, l1, ae, d1, d2, d3 = out.cpu().tolist()
    if n == 0:
        return {"n": 0}
    clean = n == nmask                        # no NaN target inside the mask
    return {"n": int(n), "abs_rel_diff": ar / n, "squ_rel_diff": sr / n, "RMS_linear": math.sqrt(se / n),
            "RMS_log": math.sqrt(l2 / n) if clean else float("nan"), "SILog": l2 / n - (l1 / n) ** 2, "mean_depth_error": ae / n,
            "median_diff": _median_diff(p, t, float(clip_distance), float(reg_factor), float(cutoff)) if clean else float("nan"),
            "threshold_delta_1.25": d1 / nmask, "threshold_delta_1.25^2": d2 / nmask, "threshold_delta_1.25^3": d3 / nmask}


def _median_diff(p, t, clip, reg, cutoff):
    """|median(target) - median(prediction)| of the masked metric depths (evaluation.py:241; np.median: the mean of the two middle
    values of an even count).  Called for NaN-free masks only; two device sorts — the table is filled once per evaluated frame."""
    tm = torch.exp(reg * (t.reshape(-1) - 1.0)) * clip
    pm = (torch.exp(reg * (p.reshape(-1) - 1.0)) * clip).clamp(math.exp(-reg) * clip, clip)
    keep = tm < cutoff
    med = []
    for v in (tm[keep], pm[keep]):
        s, k = torch.sort(v)[0], v.numel()
        med.append(0.5 * (s[(k - 1) // 2] + s[k // 2]))
    return float((med[0] - med[1]).abs())


# ------------------------------------------------------------------------------------------------ training metrics (model/metric.py)
TRAIN_METRICS = ("mse", "abs_rel_diff", "squ_rel_diff", "rms_linear", "scale_invariant_error", "mean_error", "median_error")
# columns of ramnet_batch_metrics' output row; "n" (non-NaN |t - p|) and "n_target" (non-NaN t) differ for a non-finite prediction
METRIC_COLUMNS = {"n": 0, "n_target": 1, "mse": 2, "abs_rel_diff": 3, "squ_rel_diff": 4, "rms_linear": 5, "scale_invariant_error": 6,
                  "mean_error": 7, "median_error": 8}
_ROW = 10
TICKET_BYTES = 262144   # RAMNET_BATCH_METRICS_TICKET_BYTES: the part of a workspace that has to be zero when it is allocated

_workspaces = {}        # (device index, raw stream) -> uint8 workspace of ramnet_batch_metrics (tickets zeroed once, at allocation)
_tables = {}            # (device index, pointers of the pairs) -> int64 [2][G] device table


def resolve_metrics(names):
    """config['metrics'] -> tuple of names, checked against TRAIN_METRICS (train.py:190 resolves them with getattr(module_metric, ...))."""
    out = []
    for m in names:
        if m == "structural_similarity":
            raise NotImplementedError("metric 'structural_similarity' (skimage.measure.compare_ssim) is not implemented")
        if m not in TRAIN_METRICS:
            raise KeyError("unknown metric %r; known: %s" % (m, ", ".join(TRAIN_METRICS)))
        out.append(m)
    return tuple(out)


def _columns(names):
    try:
        return [METRIC_COLUMNS[m] for m in names]
    except KeyError as e:
        raise KeyError("unknown metric column %s; known: %s" % (e, ", ".join(METRIC_COLUMNS)))


def _workspace(device, nbytes):
    key = (device.index, _st().value or 0)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, device=device, dtype=torch.uint8)
        ws[:TICKET_BYTES].zero_()
        _workspaces[key] = ws
    return ws


def _pointer_table(device, ps, ts):
    key = (device.index,) + tuple(ps) + tuple(ts)
    tab = _tables.get(key)
    if tab is None:
        if len(_tables) >= 256:
            _tables.clear()
        # pinned + non_blocking: a pageable upload would wait for the stream
        tab = torch.tensor([ps, ts], dtype=torch.int64).pin_memory().to(device, non_blocking=True)
        _tables[key] = tab
    return tab


def batch_metrics_table(preds, targets):
    """The full [G, 10] float64 table of ramnet_batch_metrics (include/ramnet_hip.h lists the columns) for G pairs of N x 1 x H x W maps, on the
    device of the predictions, enqueued on the current stream.  Nothing is read back: no synchronisation."""
    if len(preds) != len(targets):
        raise ValueError("batch_metrics: %d predictions, %d targets" % (len(preds), len(targets)))
    if not preds:
        raise ValueError("batch_metrics: no pairs")
    device = preds[0].device
    if device.type != "cuda":
        raise ValueError("batch_metrics: predictions must live on the GPU (no CPU fallback)")
    shape = tuple(preds[0].shape)
    if len(shape) != 4 or shape[1] != 1:
        raise ValueError("batch_metrics: maps are N x 1 x H x W, got %s" % (shape,))
    ps, ts, keep = [], [], []
    for p, t in zip(preds, targets):
        if tuple(p.shape) != shape or tuple(t.shape) != shape:
            raise ValueError("batch_metrics: every prediction and target must be %s, got %s / %s" % (shape, tuple(p.shape), tuple(t.shape)))
        p = p.detach().to(device=device, dtype=torch.float32).contiguous()
        t = t.detach().to(device=device, dtype=torch.float32, non_blocking=True).contiguous()
        keep.append((p, t))
        ps.append(p.data_ptr()), ts.append(t.data_ptr())
    G, N, npix = len(ps), shape[0], shape[2] * shape[3]
    with torch.cuda.device(device):
        L = H.lib()
        nbytes = L.ramnet_batch_metrics_workspace(G, N, npix)
        if nbytes == 0:
            raise ValueError("batch_metrics: unsupported sizes G=%d N=%d npix=%d" % (G, N, npix))
        ws = _workspace(device, nbytes)
        tab = _pointer_table(device, ps, ts)
        out = torch.empty((G, _ROW), device=device, dtype=torch.float64)
        H.check(L.ramnet_batch_metrics(_p(tab[0]), C.c_void_p(tab[1].data_ptr()), G, N, npix, C.c_void_p(ws.data_ptr()), C.c_void_p(out.data_ptr()), _st()),
                "ramnet_batch_metrics")
    return out


def batch_metrics(preds, targets, names=TRAIN_METRICS):
    """Training metrics of G (prediction, target) pairs -> torch.float64 [G, len(names)] ON THE DEVICE (current stream, no synchronisation).
    preds / targets: lists of N x 1 x H x W tensors (targets may live on the host: moved once); NaN in a target = no ground truth.
    names: TRAIN_METRICS entries (model/metric.py's function names) and / or the counts "n" / "n_target"."""
    cols = _columns(names)
    out = batch_metrics_table(preds, targets)
    if cols == list(range(cols[0], cols[0] + len(cols))):
        return out[:, cols[0]:cols[0] + len(cols)]
    return torch.stack([out[:, c] for c in cols], dim=1)


def eval_metrics(pred, target, names=TRAIN_METRICS):
    """LSTMTrainer._eval_metrics (lstm_trainer.py:100-106) for one pair: np.ndarray [len(names)] of float64, one read-back.  A prediction that
    is not finite where the target is valid raises ValueError (the reference's abs_rel_diff fails to broadcast there)."""
    cols = _columns(names)
    row = batch_metrics_table([pred], [target])[0].cpu().numpy()
    if row[0] != row[1]:
        raise ValueError("eval_metrics: %d valid targets but %d valid |target - prediction|: the prediction is not finite" % (row[1], row[0]))
    return row[cols]
