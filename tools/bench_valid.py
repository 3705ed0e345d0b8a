"""Timing of the batched training metrics (csrc/metrics.hip) and of a validation epoch of trainer.SequenceTrainer next to what a user would
write without them.  One JSON line per measurement; record: profiles/epoch_metrics_notes.md.

    python tools/bench_valid.py [--rounds 5] [--only-metrics] [--only-epoch]

1. metrics.batch_metrics at G = 48, N = 8, 256 x 344, 20 % NaN targets (all (K + 1) L predictions of a B = 8, L = 8 step) against the same
   seven metrics from torch reductions and torch.sort medians on the device (no host copies), alternating in one process; device time
   from HIP events.  Bytes moved by the design = 3 passes x 8 B per element; share of the 8 TB/s the project quotes.
2. One validation epoch (B = 8, L = 8, K = 5, 256 x 344, 8 batches of the benchmark's synthetic recipe) with SequenceTrainer.valid_epoch
   (step_metrics on: every prediction of every package is measured, as the reference's forward_pass_sequence does) against the same
   forward with the reference's host pattern: .item() per loss entry and batch, .cpu().numpy() and numpy metrics per prediction (the
   host side's preview pass is left out, in its favour).  Sequences per second, alternating."""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rpg_ramnet_amd import metrics as M  # noqa: E402

PEAK = 8.0e12          # bytes / s the project quotes for the MI355X
NAMES = M.TRAIN_METRICS


def torch_metrics(p, t):
    """The seven metrics of one pair with torch on the device, nothing read back: masked sums, one sort for the median."""
    eps = 1e-6
    d = (t - p).abs()
    vd, vt = ~d.isnan(), ~t.isnan()
    n = vd.sum()
    zero = torch.zeros((), device=p.device)
    d0, t0 = torch.where(vd, d, zero), torch.where(vd, t, zero)
    m1, m2 = d0.double().sum() / n, (d0 * d0).double().sum() / n
    e = torch.where(vt, p - t, zero)
    mse = ((e * e).double().sum((1, 2, 3)) / vt.sum((1, 2, 3))).mean()
    s = torch.sort(d.reshape(-1))[0]                     # NaN sorts to the end
    med = 0.5 * (s.index_select(0, ((n - 1) // 2).reshape(1)) + s.index_select(0, (n // 2).reshape(1)))[0]       # (a tensor index: no read-back)
    return torch.stack([mse, (d0 / (t0 + eps)).double().sum() / n, (d0 * d0 / (t0 * t0 + eps)).double().sum() / n, m2.sqrt(), m2 - m1 * m1, m1,
                        med.double()])


def numpy_metrics(p, t):
    """The host pattern: float32 numpy on arrays copied from the device (the arithmetic of model/metric.py, masks computed once)."""
    with np.errstate(all="ignore"):
        d = np.abs(t - p)
        v = ~np.isnan(d)
        dv, tv = d[v], t[v]
        d2 = dv * dv
        mse = np.mean([np.mean((p[i] - t[i])[~np.isnan(t[i])] ** 2) for i in range(p.shape[0])])
        return np.array([mse, (dv / (tv + 1e-6)).mean(), (d2 / (tv * tv + 1e-6)).mean(), np.sqrt(d2.mean()), d2.mean() - dv.mean() ** 2, dv.mean(),
                         np.median(dv)], np.float64)


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def bench_metrics(args):
    dev = torch.device("cuda:0")
    G, N, Hh, W = 48, 8, 256, 344
    g = torch.Generator(device=dev).manual_seed(0)
    ps, ts = [], []
    for _ in range(G):
        t = torch.rand(N, 1, Hh, W, device=dev, generator=g) * 0.9 + 0.05
        p = (t + 0.05 * torch.randn(N, 1, Hh, W, device=dev, generator=g)).clamp(0, 1)
        t[torch.rand(N, 1, Hh, W, device=dev, generator=g) < 0.2] = float("nan")
        ps.append(p), ts.append(t)
    new = lambda: M.batch_metrics(ps, ts)                                    # noqa: E731
    old = lambda: torch.stack([torch_metrics(p, t) for p, t in zip(ps, ts)])  # noqa: E731
    for _ in range(2):
        a, b = new(), old()
    torch.cuda.synchronize()
    rel = float(((a - b).abs() / b.abs()).max())
    nbytes = 3 * 8 * G * N * Hh * W
    for r in range(args.rounds):
        ms_new, _ = device_ms(new)
        ms_old, _ = device_ms(old)
        print(json.dumps(dict(what="batch_metrics", round=r, G=G, N=N, H=Hh, W=W, ms_new=round(ms_new, 4), ms_torch=round(ms_old, 4),
                              ratio=round(ms_old / ms_new, 1), design_bytes=nbytes, share_of_peak=round(nbytes / (ms_new * 1e-3) / PEAK, 3),
                              max_rel_diff_to_torch=rel)), flush=True)


class ListLoader:
    """Batches that already live on the device, and their samples as the dataset the previews index."""

    def __init__(self, batches):
        self.batches = batches
        self.dataset = [[{k: v[b] for k, v in item.items()} for item in seq] for seq in batches for b in range(2)]

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def bench_epoch(args):
    import bench
    from rpg_ramnet_amd.model.model import ERGB2DepthRecurrent
    from rpg_ramnet_amd.trainer import SequenceTrainer, sequence_loss
    K, bins, B, L, Hh, W = 5, 5, 8, 8, 256, 344
    lc = ["image", "events4"]
    cfg = dict(bench.RELEASED, num_bins_events=bins, gpu=0, every_x_rgb_frame=K, baseline=False, loss_composition=lc)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        model = ERGB2DepthRecurrent(cfg)
    model = model.to(model.gpu)
    seqs = [bench.synth_sequence(model, B, L, Hh, W, K, bins, 20000, seed=100 + i) for i in range(2)]
    for seq in seqs:
        for item in seq:
            for k in range(K - 1):
                item["depth_events%d" % k] = item["depth_image"]
    loader = ListLoader([seqs[i % 2] for i in range(8)])
    config = {"metrics": list(NAMES), "loss": {"type": "scale_invariant_loss", "config": {"weight": 1.0, "n_lambda": 1.0}},
              "data_loader": {"train": {"every_x_rgb_frame": K}},
              "trainer": {"num_previews": 2, "num_val_previews": 2, "loss_composition": lc, "loss_weights": [1, 1]}}
    st = SequenceTrainer(config, model, loader, loader, step_metrics=True)
    plain = SequenceTrainer(config, model, loader, loader)

    def host_pattern():
        model.eval()
        losses, rows = {}, []
        with torch.no_grad():
            for sequence in loader:
                _, _, parts = sequence_loss(model, sequence, lc, [1, 1], parts=True)
                for k in ("loss", "L_si"):
                    losses.setdefault(k, []).append(parts[k].item())
                for l, key, p in parts["predictions"]:
                    rows.append(numpy_metrics(p.cpu().data.numpy(), sequence[l]["depth_" + key].cpu().data.numpy()))
        return {"val_loss": sum(losses["loss"]) / len(loader), "val_step_metrics": np.mean(rows, axis=0).tolist()}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    a, b = st.valid_epoch(), host_pattern()          # warm-up of both
    n_seq = len(loader) * B
    for r in range(args.rounds):
        s_new, a = wall(st.valid_epoch)
        s_old, b = wall(host_pattern)
        s_plain, _ = wall(plain.valid_epoch)
        print(json.dumps(dict(what="valid_epoch", round=r, batches=len(loader), B=B, L=L, seq_per_s_new=round(n_seq / s_new, 2),
                              seq_per_s_host_pattern=round(n_seq / s_old, 2), seq_per_s_new_without_step_metrics=round(n_seq / s_plain, 2),
                              ratio=round(s_old / s_new, 2), val_loss_new=a["val_loss"], val_loss_host=b["val_loss"],
                              max_rel_diff_step_metrics=float(np.max(np.abs(np.array(a["val_step_metrics"]) - b["val_step_metrics"])
                                                                     / np.abs(b["val_step_metrics"]))))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only-metrics", action="store_true")
    ap.add_argument("--only-epoch", action="store_true")
    args = ap.parse_args()
    if not args.only_epoch:
        bench_metrics(args)
    if not args.only_metrics:
        bench_epoch(args)


if __name__ == "__main__":
    main()
