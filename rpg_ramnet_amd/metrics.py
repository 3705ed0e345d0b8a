"""Depth evaluation on device: metric depth from normalised log depth (RAM_Net/evaluation.py:74-96) and the error metrics
of `add_to_metrics` (evaluation.py:201-241, RAM_Net/model/metric.py:8-33) with the reference's key names, comparison
operators and epsilons; one fused HIP reduction per call (Abs-Rel is the accuracy half of the headline metric).  All ten rows of the
reference's table, NaN behaviour included: `RMS_log` and `median_diff` are plain `np.mean` / `np.median` over the masked pixels
(evaluation.py:214, 241), so ONE NaN target inside the mask makes them NaN, while the metric.py means skip it
(pinned by tests/golden/eval_metrics.npz, the reference's own `add_to_metrics` run on seeded maps).

The TRAINING metrics (model/metric.py:8-54 through LSTMTrainer._eval_metrics, lstm_trainer.py:100-106) are different functions, on the
normalised log-depth maps themselves: `batch_metrics` computes all of them for a whole list of (prediction, target) pairs in one HIP
reduction (exact median included) and leaves the table on the device; `eval_metrics` is the one-pair drop-in for `_eval_metrics`.

`EvalTable` is the batched form of the evaluation table: all ten rows for any number of files, every depth cut-off and the event-masked
half (evaluation.py:359-390) in three launches per batch, rows kept on the device, one read-back (`finish_eval_rows` is its host part).
`rescale=True` is evaluation.py's --rescale (rescale_by_the_median before the metrics, a fourth launch), `down_scale_factor` its
--down_scale_factor (the metric target resized on the device by `resize_metric_target`)."""
import ctypes as C
import math

import numpy as np
import torch

from . import _hip as H
from .ops import _p, _st


def depth_metrics(prediction, target, clip_distance, reg_factor, cutoff=float("inf")):
    """prediction / target: normalised log-depth tensors (any shape, same numel).  Pixels with metric target depth
    `nan_to_num(t) < cutoff` form the mask (evaluation.py:367); NaN targets are skipped by the means (metric.py) but stay in
    the denominator of the delta thresholds (`np.mean(ratio <= ...)`, evaluation.py:224-226)."""
    from . import ops
    ops.not_deterministic("metrics.depth_metrics (the batched tables, metrics.batch_metrics and EvalTable, are ordered)")
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
_tables = {}            # (device index, raw stream, pointers of the pairs) -> int64 [2][G] device table


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
    # (the stream is part of the key: the upload is ordered before its readers on the stream it was enqueued on and on no other)
    key = (device.index, _st().value or 0) + tuple(ps) + tuple(ts)
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


# ------------------------------------------------------------------------------------------------ evaluation table (evaluation.py:295-397)
EVAL_KEYS = ("abs_rel_diff", "squ_rel_diff", "RMS_linear", "RMS_log", "SILog", "mean_depth_error", "median_diff", "threshold_delta_1.25",
             "threshold_delta_1.25^2", "threshold_delta_1.25^3")
EVAL_CUTOFFS = (10, 20, 30, 80, 250, 500)       # depth_values of evaluation.py
EVAL_ROW = 16           # doubles of a row of ramnet_eval_table (include/ramnet_hip.h lists the columns)
EVAL_TICKET_BYTES = 262144   # RAMNET_EVAL_TABLE_TICKET_BYTES
EVAL_RESCALE, EVAL_TARGET_METRIC = 1, 2      # RAMNET_EVAL_RESCALE, RAMNET_EVAL_TARGET_METRIC: flags of ramnet_eval_table_ex

_eval_workspaces = {}   # (device index, raw stream) -> uint8 workspace of ramnet_eval_table (tickets zeroed once, at allocation)


def metric_depth(y, clip_distance, reg_factor, clamp=False):
    """Normalised log depth -> metric depth on the device, float32: exp(reg * (y - 1)) * clip, with clamp=True clipped to
    [exp(-reg) * clip, clip] (the prediction side of prepare_depth_data, evaluation.py:74-96).  NaN stays NaN.  The evaluation table
    converts with the same device function."""
    if y.device.type != "cuda":
        raise ValueError("metric_depth: the map must live on the GPU (no CPU fallback)")
    x = y.detach().to(torch.float32).contiguous()
    out = torch.empty_like(x)
    if x.numel():
        with torch.cuda.device(x.device):
            H.check(H.lib().ramnet_metric_depth(_p(x), x.numel(), float(clip_distance), float(reg_factor), int(bool(clamp)), _p(out), _st()),
                    "ramnet_metric_depth")
    return out


def _fill_table(device, ptrs, rows):
    """Device table [rows, len(ptrs) / rows] of int64 pointers, written by kernel argument on the current stream."""
    tab = torch.empty((rows, len(ptrs) // rows), device=device, dtype=torch.int64)
    host = (C.c_void_p * len(ptrs))(*ptrs)
    H.check(H.lib().ramnet_fill_pointer_table(C.c_void_p(tab.data_ptr()), host, len(ptrs), _st()), "ramnet_fill_pointer_table")
    return tab


def resized_shape(shape, scale_factor):
    """(H', W') of a map resized by F.interpolate(..., scale_factor=s): floor(H * s), floor(W * s)."""
    return int(math.floor(shape[-2] * float(scale_factor))), int(math.floor(shape[-1] * float(scale_factor)))


def resize_metric_target(targets, clip_distance, reg_factor, scale_factor):
    """The target side of prepare_depth_data with down_scale_factor < 1 (evaluation.py:87-94) on the device: targets = a list of H x W
    maps or a [G, 1, H, W] / [G, H, W] tensor of normalised log depth -> [G, H', W'] float32 METRIC depth, the bilinear interpolation of
    the metric depths with F.interpolate's default coordinates (align_corners=False, the given factor).  One launch for the G maps."""
    s = float(scale_factor)
    if not 0.0 < s <= 1.0:
        raise ValueError("resize_metric_target: scale_factor must be in (0, 1], got %r" % (scale_factor,))
    first = targets[0]
    device = first.device
    if device.type != "cuda":
        raise ValueError("resize_metric_target: the targets must live on the GPU (no CPU fallback)")
    with torch.cuda.device(device):
        ts = _eval_maps(targets, device, torch.float32, "targets")
        shape = tuple(ts[0].shape[-2:])
        if any(t is None or t.numel() != shape[0] * shape[1] or tuple(t.shape[-2:]) != shape for t in ts):
            raise ValueError("resize_metric_target: every target is one %s map" % (shape,))
        Ho, Wo = resized_shape(shape, s)
        if Ho < 1 or Wo < 1:
            raise ValueError("resize_metric_target: %s maps have no pixel left at scale_factor %r" % (shape, scale_factor))
        tab = _fill_table(device, [t.data_ptr() for t in ts], 1)
        out = torch.empty((len(ts), Ho, Wo), device=device, dtype=torch.float32)
        H.check(H.lib().ramnet_resize_metric_target(C.c_void_p(tab.data_ptr()), len(ts), shape[0], shape[1], s, float(clip_distance),
                                                    float(reg_factor), _p(out), _st()), "ramnet_resize_metric_target")
    return out


def eval_variant_prefixes(cutoffs, has_mask):
    """Key prefixes of the variants in the order of a table row: "", "10_", ..., then "event_masked_", "event_masked_10_", ..."""
    pre = [""] + ["%d_" % c for c in cutoffs]
    return pre + ["event_masked_" + p for p in pre] if has_mask else pre


def _eval_entries(rows):
    """[F, V, 16] rows -> ([F, V, 10] table entries in the order of EVAL_KEYS, as depth_metrics forms them, [F, V] n)."""
    r = np.asarray(rows, dtype=np.float64)
    nmask, n = r[..., 0], r[..., 1]
    with np.errstate(all="ignore"):
        clean = n == nmask
        msq = r[..., 5] / n
        med = np.abs(r[..., 11].astype(np.float32) - r[..., 12].astype(np.float32)).astype(np.float64)
        cols = [r[..., 2] / n, r[..., 3] / n, np.sqrt(r[..., 4] / n), np.where(clean, np.sqrt(msq), np.nan), msq - (r[..., 6] / n) ** 2,
                r[..., 7] / n, np.where(clean, med, np.nan), r[..., 8] / nmask, r[..., 9] / nmask, r[..., 10] / nmask]
    return np.stack(cols, axis=-1), n


def eval_file_counts(rows, skip_empty=True):
    """Files that count for each variant: [V].  skip_empty=True: those with a valid pixel inside the variant; False: all."""
    r = np.asarray(rows)
    return (r[..., 1] > 0).sum(axis=0) if skip_empty else np.full(r.shape[1], r.shape[0])


def finish_eval_rows(rows, cutoffs, has_mask, skip_empty=True):
    """Host part of the evaluation table, pure numpy: [F, V, 16] rows of ramnet_eval_table -> {"<variant prefix><metric>": mean over
    files, "files": F}.  Per file and variant the ten entries are formed as depth_metrics forms them; median_diff is
    abs(float32(median_t) - float32(median_p)); a variant without a pixel gives ten NaN, one with NaN targets only gives thresholds 0.0
    and the rest NaN (what the reference's add_to_metrics returns on such masks).
    skip_empty=True is evaluate_folders' rule: a file without a valid pixel in a variant does not count for that variant (a variant no
    file counts for has no keys).  skip_empty=False is the reference's sum / number of files, NaN propagating (evaluation.py:393)."""
    r = np.asarray(rows, dtype=np.float64)
    prefixes = eval_variant_prefixes(cutoffs, has_mask)
    if r.ndim != 3 or r.shape[1] != len(prefixes) or r.shape[2] != EVAL_ROW:
        raise ValueError("finish_eval_rows: rows are [F, %d, %d], got %s" % (len(prefixes), EVAL_ROW, r.shape))
    vals, n = _eval_entries(r)
    out = {}
    for v, pre in enumerate(prefixes):
        keep = n[:, v] > 0 if skip_empty else np.ones(r.shape[0], bool)
        if skip_empty and not keep.any():
            continue
        for k, name in enumerate(EVAL_KEYS):
            out[pre + name] = float(sum(vals[keep, v, k].tolist()) / int(keep.sum())) if keep.any() else float("nan")
    out["files"] = int(r.shape[0])
    return out


def _eval_maps(x, device, dtype, what):
    """list of maps or a [G, 1, H, W] / [G, H, W] tensor -> (list of contiguous tensors that own what the kernel reads, shape of a map)"""
    if torch.is_tensor(x):
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 3:
            raise ValueError("EvalTable.add: %s is a list of maps or a [G, 1, H, W] / [G, H, W] tensor, got %s" % (what, tuple(x.shape)))
        x = list(x.detach().to(device=device, dtype=dtype, non_blocking=True).contiguous())
        return x
    return [None if m is None else m.detach().to(device=device, dtype=dtype, non_blocking=True).contiguous() for m in x]


class EvalTable:
    """The reference's evaluation table (evaluation.py:295-397) for any number of (prediction, target) pairs of normalised log depth, on
    the device: all pixels, every depth cut-off, and the same under event masks when masks are given.  `add` launches
    ramnet_eval_table for its maps at once and appends their rows to a device-side table without a synchronisation; `result` reads the
    table back once and averages over the files on the host."""

    def __init__(self, clip_distance, reg_factor, cutoffs=EVAL_CUTOFFS, rescale=False, down_scale_factor=1.0):
        self.clip_distance, self.reg_factor = float(clip_distance), float(reg_factor)
        self.cutoffs = tuple(cutoffs)
        self.rescale, self.down_scale_factor = bool(rescale), float(down_scale_factor)
        if not 0.0 < self.down_scale_factor <= 1.0:
            raise ValueError("EvalTable: down_scale_factor must be in (0, 1], got %r" % (down_scale_factor,))
        if len(self.cutoffs) > 8 or any(not b > a for a, b in zip((0,) + self.cutoffs, self.cutoffs)):
            raise ValueError("EvalTable: at most 8 ascending positive cut-offs, got %r" % (self.cutoffs,))
        self._cut = (C.c_float * max(len(self.cutoffs), 1))(*[float(c) for c in self.cutoffs])
        self._chunks, self.has_mask = [], None

    def __len__(self):
        return sum(c.shape[0] for c in self._chunks)

    def add(self, preds, targets, masks=None):
        """preds / targets: lists of same-shape maps (targets may live on the host: moved once) or [G, 1, H, W] / [G, H, W] tensors;
        masks: the same of uint8 / bool (non-zero = inside the event mask; a list entry may be None: all inside).  Enqueued on the
        current stream for exactly these maps; no reference to them is kept (what had to be copied belongs to the stream-ordered allocator).
        down_scale_factor < 1: predictions (and masks) are H' x W' = floor(H s) x floor(W s), targets H x W; the metric targets are resized
        on the device first.  Returns the [G, V, 16] rows (device)."""
        has_mask = masks is not None
        if self.has_mask is None:
            self.has_mask = has_mask
        elif self.has_mask != has_mask:
            raise ValueError("EvalTable.add: every call of one table comes with masks, or none does")
        first = preds[0]
        device = first.device
        if device.type != "cuda":
            raise ValueError("EvalTable.add: predictions must live on the GPU (no CPU fallback)")
        with torch.cuda.device(device):
            ps, ts = _eval_maps(preds, device, torch.float32, "preds"), _eval_maps(targets, device, torch.float32, "targets")
            if has_mask:
                ms = [m if m is None or m.dtype == torch.uint8 else (m if m.dtype == torch.bool else m != 0).view(torch.uint8)
                      for m in _eval_maps(masks, device, None, "masks")]
            else:
                ms = []
            G = len(ps)
            if G == 0 or len(ts) != G or (has_mask and len(ms) != G):
                raise ValueError("EvalTable.add: %d predictions, %d targets, %s masks" % (G, len(ts), len(ms) if has_mask else "no"))
            npix = ps[0].numel()
            flags = EVAL_RESCALE if self.rescale else 0
            if self.down_scale_factor < 1.0:
                if any(p is None or t is None or t.dim() < 2 or p.dim() < 2 for p, t in zip(ps, ts)):
                    raise ValueError("EvalTable.add: a down-scaled table takes 2-D maps")
                small = tuple(ps[0].shape[-2:])
                for p, t in zip(ps, ts):
                    if tuple(p.shape[-2:]) != small or p.numel() != npix or resized_shape(t.shape, self.down_scale_factor) != small:
                        raise ValueError("EvalTable.add: predictions are %s, targets must resize to that by %r, got %s -> %s"
                                         % (small, self.down_scale_factor, tuple(t.shape), resized_shape(t.shape, self.down_scale_factor)))
                for m in ms:
                    if m is not None and (tuple(m.shape[-2:]) != small or m.numel() != npix):
                        raise ValueError("EvalTable.add: masks must have the size of the predictions, %s, got %s (resized event frames are not "
                                         "covered)" % (small, tuple(m.shape)))
                ts = list(resize_metric_target(ts, self.clip_distance, self.reg_factor, self.down_scale_factor))
                flags |= EVAL_TARGET_METRIC
            for p, t in zip(ps, ts):
                if p is None or t is None or p.numel() != npix or t.numel() != npix:
                    raise ValueError("EvalTable.add: every prediction and target holds %d pixels" % npix)
            for m in ms:
                if m is not None and (m.numel() != npix or m.dtype != torch.uint8):
                    raise ValueError("EvalTable.add: every mask holds %d uint8 / bool pixels" % npix)
            L = H.lib()
            nbytes = L.ramnet_eval_table_ex_workspace(G, npix, len(self.cutoffs), int(has_mask), flags) if flags else \
                L.ramnet_eval_table_workspace(G, npix, len(self.cutoffs), int(has_mask))
            if nbytes == 0:
                raise ValueError("EvalTable.add: unsupported sizes G=%d npix=%d cut-offs=%d" % (G, npix, len(self.cutoffs)))
            key = (device.index, _st().value or 0)
            ws = _eval_workspaces.get(key)
            if ws is None or ws.numel() < nbytes:
                ws = torch.empty(nbytes, device=device, dtype=torch.uint8)
                ws[:EVAL_TICKET_BYTES].zero_()
                _eval_workspaces[key] = ws
            ptrs = [p.data_ptr() for p in ps] + [t.data_ptr() for t in ts] + [0 if m is None else m.data_ptr() for m in ms]
            tab = torch.empty((3, G), device=device, dtype=torch.int64)
            host = (C.c_void_p * len(ptrs))(*ptrs)
            H.check(L.ramnet_fill_pointer_table(C.c_void_p(tab.data_ptr()), host, len(ptrs), _st()), "ramnet_fill_pointer_table")
            V = (1 + len(self.cutoffs)) * (2 if has_mask else 1)
            out = torch.empty((G, V, EVAL_ROW), device=device, dtype=torch.float64)
            if flags:
                H.check(L.ramnet_eval_table_ex(C.c_void_p(tab[0].data_ptr()), C.c_void_p(tab[1].data_ptr()),
                                               C.c_void_p(tab[2].data_ptr()) if has_mask else None, G, npix, self.clip_distance, self.reg_factor,
                                               self._cut, len(self.cutoffs), flags, C.c_void_p(ws.data_ptr()), C.c_void_p(out.data_ptr()), _st()),
                        "ramnet_eval_table_ex")
            else:
                H.check(L.ramnet_eval_table(C.c_void_p(tab[0].data_ptr()), C.c_void_p(tab[1].data_ptr()),
                                            C.c_void_p(tab[2].data_ptr()) if has_mask else None, G, npix, self.clip_distance, self.reg_factor,
                                            self._cut, len(self.cutoffs), C.c_void_p(ws.data_ptr()), C.c_void_p(out.data_ptr()), _st()),
                        "ramnet_eval_table")
        self._chunks.append(out)
        return out

    def rows(self):
        """[F, V, 16] float64 on the device: one row per added pair and variant, in the order they were added."""
        if not self._chunks:
            raise ValueError("EvalTable: nothing was added")
        if len(self._chunks) > 1:
            self._chunks = [torch.cat(self._chunks, dim=0)]
        return self._chunks[0]

    def result(self, skip_empty=True):
        """ONE read-back of the table, then finish_eval_rows."""
        return finish_eval_rows(self.rows().cpu().numpy(), self.cutoffs, bool(self.has_mask), skip_empty=skip_empty)
