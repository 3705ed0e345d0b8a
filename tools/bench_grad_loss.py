"""Timing of the batched multi-scale gradient loss (csrc/grad_loss.hip) next to the per-pair path, and of a training step of the released
recipe (SI loss + 0.25 x gradient loss) with the batched path off and on.  One JSON line per measurement; record:
profiles/grad_loss_batch_notes.md.

    python tools/bench_grad_loss.py [--rounds 5] [--only-loss] [--only-step] [--trace-only]

1. Forward + backward of the gradient loss of G = 16 and G = 20 pairs (B = 8, 256 x 344: the supervised maps of an L = 8 / L = 10 step), targets
   with block-shaped NaN regions covering about 20 %: ops.multi_scale_grad_loss_batch against G x ops.multi_scale_grad_loss, alternating in one
   process; device time from HIP events, library calls counted through _hip.set_tracer.  Bytes the algorithm has to move: 8 B per pixel
   forward (both maps once), 12 B per pixel backward (both maps and the gradient); halo re-reads are overhead.  Share of the 8 TB/s the
   project quotes.
2. One training step at B = 8, L = 8, K = 5, 256 x 344 through trainer.sequence_loss with grad_loss_weight = 0.25, option off / on alternating,
   in samples per second (wall clock around loss + backward, synchronised).
--trace-only: part 1's two paths a few times with no timing of its own — the run to put under `rocprofv3 --kernel-trace --stats`, which gives
the kernel-only time."""
import argparse
import contextlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rpg_ramnet_amd import _hip, ops  # noqa: E402

PEAK = 8.0e12          # bytes / s the project quotes for the MI355X


def block_nan_targets(G, B, Hh, W, dev, seed=0):
    """Pairs whose targets carry block-shaped NaN regions (sky / out-of-range blocks of a depth map): about 20 % of every sample."""
    g = torch.Generator(device=dev).manual_seed(seed)
    cpu = torch.Generator().manual_seed(seed)
    ps, ts = [], []
    for _ in range(G):
        t = torch.rand(B, 1, Hh, W, device=dev, generator=g) * 0.9 + 0.05
        p = (t + 0.05 * torch.randn(B, 1, Hh, W, device=dev, generator=g)).clamp(0, 1)
        for b in range(B):
            t[b, :, :Hh // 4, :W // 2] = float("nan")                                      # 12.5 %: a band at the top
            for _ in range(3):                                                              # + three 36 x 52 blocks off the 8-grid: <= 7.5 %
                y, x = int(torch.randint(Hh // 4, Hh - 36, (1,), generator=cpu)), int(torch.randint(0, W - 52, (1,), generator=cpu))
                t[b, :, y:y + 36, x:x + 52] = float("nan")
        ps.append(p), ts.append(t)
    return ps, ts


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def loss_paths(G, dev):
    B, Hh, W = 8, 256, 344
    ps, ts = block_nan_targets(G, B, Hh, W, dev)
    nan_share = float(torch.stack([t.isnan().float().mean() for t in ts]).mean())
    leaves = [p.clone().requires_grad_(True) for p in ps]

    def batched():
        for p in leaves:
            p.grad = None
        ops.multi_scale_grad_loss_batch(leaves, ts, with_sum=True)[1].backward()
        return leaves

    def per_pair():
        for p in leaves:
            p.grad = None
        torch.stack([ops.multi_scale_grad_loss(p, t) for p, t in zip(leaves, ts)]).sum().backward()
        return leaves

    return batched, per_pair, (G, B, Hh, W, nan_share)


def count_calls(fn):
    calls = []
    _hip.set_tracer(lambda name, f, a: (calls.append(name), f(*a))[1])
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _hip.set_tracer(None)
    return len(calls), sorted(set(calls))


def bench_loss(args):
    dev = torch.device("cuda:0")
    for G in (16, 20):
        batched, per_pair, (G, B, Hh, W, nan_share) = loss_paths(G, dev)
        for _ in range(2):
            a = [p.grad.clone() for p in batched()]
            b = [p.grad.clone() for p in per_pair()]
        torch.cuda.synchronize()
        diff = max(float((x - y).abs().max()) for x, y in zip(a, b)) / max(float(y.abs().max()) for y in b)
        n_new, names_new = count_calls(batched)
        n_old, _ = count_calls(per_pair)
        nbytes = (8 + 12) * G * B * Hh * W
        for r in range(args.rounds):
            ms_new, _ = device_ms(batched)
            ms_old, _ = device_ms(per_pair)
            print(json.dumps(dict(what="grad_loss_fwd_bwd", round=r, G=G, B=B, H=Hh, W=W, nan_share=round(nan_share, 3), ms_batched=round(ms_new, 4),
                                  ms_per_pair=round(ms_old, 4), ratio=round(ms_old / ms_new, 2), library_calls_batched=n_new,
                                  library_calls_per_pair=n_old, entry_points_batched=names_new, design_bytes=nbytes,
                                  share_of_peak=round(nbytes / (ms_new * 1e-3) / PEAK, 3), max_rel_grad_diff=diff)), flush=True)


def trace_only(args):
    dev = torch.device("cuda:0")
    batched, per_pair, _ = loss_paths(16, dev)
    for _ in range(args.rounds):
        batched()
        per_pair()
    torch.cuda.synchronize()
    print(json.dumps(dict(what="trace_only", G=16, repetitions=args.rounds)), flush=True)


def bench_step(args):
    import bench
    from rpg_ramnet_amd.model.model import ERGB2DepthRecurrent
    from rpg_ramnet_amd.trainer import sequence_loss
    K, bins, B, L, Hh, W = 5, 5, 8, 8, 256, 344
    lc = ["image", "events4"]
    cfg = dict(bench.RELEASED, num_bins_events=bins, gpu=0, every_x_rgb_frame=K, baseline=False, loss_composition=lc)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        model = ERGB2DepthRecurrent(cfg)
    model = model.to(model.gpu).train()
    seq = bench.synth_sequence(model, B, L, Hh, W, K, bins, 20000, seed=100)
    for item in seq:
        item["depth_events%d" % (K - 1)] = item["depth_image"]

    def step(on):
        ops.set_grad_loss_batched(on)
        try:
            model.zero_grad()
            total, _ = sequence_loss(model, seq, lc, [1, 1], grad_loss_weight=0.25)
            total.backward()
            return total.detach()
        finally:
            ops.set_grad_loss_batched(True)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for _ in range(2):
        step(False), step(True)
    n_on, _ = count_calls(lambda: step(True))
    n_off, _ = count_calls(lambda: step(False))
    for r in range(args.rounds):
        s_off, l_off = wall(lambda: step(False))
        s_on, l_on = wall(lambda: step(True))
        print(json.dumps(dict(what="train_step_grad_loss", round=r, B=B, L=L, K=K, H=Hh, W=W, samples_per_s_off=round(B / s_off, 2),
                              samples_per_s_on=round(B / s_on, 2), ratio=round(s_off / s_on, 4), library_calls_off=n_off, library_calls_on=n_on,
                              loss_off=float(l_off), loss_on=float(l_on))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only-loss", action="store_true")
    ap.add_argument("--only-step", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    if args.trace_only:
        return trace_only(args)
    if not args.only_step:
        bench_loss(args)
    if not args.only_loss:
        bench_step(args)


if __name__ == "__main__":
    main()
