"""Partial training (requires_grad = False honoured end to end): what a step costs when only part of the network trains.

  steps   the bench step (bench.py's workload: B = 8, L = 8, K = 5, 256 x 344, resident inputs, SI loss on [image, events4], fused Adam,
          backward-weights and decoders on their side streams, deferred cell launches) with every tensor trainable ("all") and with the
          freeze sets A (decoder only: resblocks, decoders, pred train) and B (one sensor branch: head_events, encoders_events,
          state_combination_events train).  One JSON line per set: per-step milliseconds (HIP events around each step, median / min / max
          over --steps after --warmup), samples/s, torch.cuda.max_memory_allocated of the timed steps, the last loss, and how many tensors
          hold a .grad afterwards.
  cells   the backward-data launches of a recurrent cell at the three state scales of that workload (C = 64 / 128 / 256 at 128 x 172 /
          64 x 86 / 32 x 43, batch 8), full width ([dx | dh], 2C output channels) against the state half (dh alone: C output channels
          into dxh[..., C:], the ConvGRU's stage B as its own launch), alternating, median of 5 windows each.

  pred    the prediction layer's backward at the bench step's supervised decode (2 segments of 8 x 256 x 344 pixels, 32 channels, ReLU
          mask of x applied): ramnet_pred_sigmoid_si_bwd (weight and bias sums joined through the forward's scratch) against the
          data-gradient-only ramnet_pred_sigmoid_si_dgrad, alternating; bytes = what the launch has to move (x, dx, y, target), share of
          the 8.0 TB/s HBM peak.

--root DIR imports bench.py and rpg_ramnet_amd from another checkout (A/B against a parent commit: the flags are set the same way by
name pattern; a tree that ignores them is the yardstick).  --tag names the tree in the output.

    python tools/bench_partial.py steps [--sets all,A,B] [--steps 10] [--warmup 3] [--root DIR] [--tag NAME] [--out FILE]
    python tools/bench_partial.py cells [--out FILE]
    python tools/bench_partial.py pred [--out FILE]
"""
import argparse
import contextlib
import fnmatch
import json
import os
import sys

import torch

P = "statenetphasedrecurrent."
SETS = {"all": None,
        "A": [P + "resblocks.*", P + "decoders.*", P + "pred.*"],
        "B": [P + "head_events.*", P + "encoders_events.*", P + "state_combination_events.*"]}
SCALES = [(64, 128, 172), (128, 64, 86), (256, 32, 43)]


def train_only(model, patterns):
    """By name pattern and p.requires_grad_ alone, so that it runs on a tree without trainer.freeze too."""
    n = 0
    for name, p in model.named_parameters():
        if patterns is not None and not any(fnmatch.fnmatchcase(name, pat) for pat in patterns):
            p.requires_grad_(False)
            n += 1
    return n


def steps(args, emit):
    import bench
    from rpg_ramnet_amd import ops
    from rpg_ramnet_amd.model.model import ERGB2DepthRecurrent
    from rpg_ramnet_amd.parallel import FlatGradReducer
    from rpg_ramnet_amd.trainer import sequence_loss
    ops.set_wgrad_overlap(True)
    ops.set_decoder_overlap(True)
    ops.set_wgrad_defer(2)
    K, bins, B, L, H, W = 5, 5, args.batch, args.seq_len, args.height, args.width
    cfg = dict(bench.RELEASED, num_bins_events=bins, gpu=0, every_x_rgb_frame=K, baseline=False, loss_composition=["image", "events4"])
    seq = None
    for name in args.sets.split(","):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(sys.stderr):
            model = ERGB2DepthRecurrent(cfg)
        model = model.to(model.gpu).train()
        if seq is None:
            seq = bench.synth_sequence(model, B, L, H, W, K, bins, args.events_per_grid, seed=1000)
        frozen = train_only(model, SETS[name])
        reducer = FlatGradReducer(model)
        opt = torch.optim.Adam(model.parameters(), lr=3e-4, weight_decay=0, fused=True)

        def step():
            reducer.zero()
            total, _ = sequence_loss(model, seq, cfg["loss_composition"], [1, 1])
            total.backward()
            reducer.all_reduce()
            reducer.wait()
            opt.step()
            return total

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        ev[0].record()
        for i in range(args.steps):
            total = step()
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps))
        med = ms[len(ms) // 2]
        emit(dict(what="step", tag=args.tag, set=name, frozen_tensors=frozen, B=B, L=L, K=K, H=H, W=W, steps=args.steps, warmup=args.warmup,
                  ms_median=round(med, 3), ms_min=round(ms[0], 3), ms_max=round(ms[-1], 3), samples_per_s=round(B * L * 1e3 / med, 2),
                  peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 3), loss=float(total),
                  tensors_with_grad=sum(p.grad is not None for p in model.parameters()),
                  tensors=sum(1 for _ in model.parameters())))
        reducer.close()
        del model, reducer, opt


def _window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def cells(args, emit):
    from rpg_ramnet_amd import _hip as Hh, ops
    dev = torch.device("cuda:0")
    L = Hh.lib()
    tapsd = ops.Taps.get("dgrad1", 3, 1)
    B = args.batch
    for Cc, H, W in SCALES:
        torch.manual_seed(Cc)
        mk = lambda co: ops.ConvParam([torch.nn.Parameter(torch.randn(co, 2 * Cc, 3, 3, device=dev) * 0.02)],  # noqa: E731
                                      [torch.nn.Parameter(torch.zeros(co, device=dev))])
        cp_o, cp_ur, cp_g = mk(Cc), mk(2 * Cc), mk(4 * Cc)
        npix = B * H * W
        dpo, h, dhd = (torch.randn(B, H, W, Cc, device=dev) for _ in range(3))
        ur, dpur = torch.rand(B, H, W, 2 * Cc, device=dev), torch.randn(B, H, W, 2 * Cc, device=dev)
        dpre = torch.randn(B, H, W, 4 * Cc, device=dev)
        dxh = torch.zeros(B, H, W, 2 * Cc, device=dev)
        p = ops._p

        def gru_full():
            if Cc % 64 == 0:
                ops.conv_launch(dpo, tapsd, cp_o.bwd(), dxh, 2 * Cc, epi=Hh.EPI_GRU_BWD, e0=ur, e1=h, o1=dpur)
            else:
                ops.conv_launch(dpo, tapsd, cp_o.bwd(), dxh, 2 * Cc)
                Hh.check(L.ramnet_gru_bwd_b(p(dxh), p(ur), p(h), p(dpur), p(dhd), npix, Cc, ops._st()), "gru_bwd_b")
            ops.conv_launch(dpur, tapsd, cp_ur.bwd(), dxh, 2 * Cc, beta=1.0)

        def gru_half():
            ops.conv_launch(dpo, tapsd, cp_o.state_half().bwd(), dxh, Cc, out_off=Cc)
            Hh.check(L.ramnet_gru_bwd_b(p(dxh), p(ur), p(h), p(dpur), p(dhd), npix, Cc, ops._st()), "gru_bwd_b")
            ops.conv_launch(dpur, tapsd, cp_ur.state_half().bwd(), dxh, Cc, out_off=Cc, beta=1.0)

        def lstm_full():
            ops.conv_launch(dpre, tapsd, cp_g.bwd(), dxh, 2 * Cc)

        def lstm_half():
            ops.conv_launch(dpre, tapsd, cp_g.state_half().bwd(), dxh, Cc, out_off=Cc)

        for cell, full, half in (("convgru", gru_full, gru_half), ("convlstm", lstm_full, lstm_half)):
            for fn in (full, half):
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            reps = max(5, int(2e4 / max(_window(full, 5), 1.0)))          # windows of ~20 ms
            tf, th = [], []
            for _ in range(5):                                            # alternating windows
                tf.append(_window(full, reps))
                th.append(_window(half, reps))
            f, hh = sorted(tf)[2], sorted(th)[2]
            emit(dict(what="cell_backward_data", cell=cell, C=Cc, H=H, W=W, B=B, us_full=round(f, 2), us_state_half=round(hh, 2),
                      us_full_windows=[round(t, 2) for t in tf], us_state_half_windows=[round(t, 2) for t in th], speedup=round(f / hh, 3)))


def pred(args, emit):
    import ctypes as C
    from rpg_ramnet_amd import _hip as Hh, ops
    dev = torch.device("cuda:0")
    L = Hh.lib()
    Cc, nseg, seg_pix = 32, 2, args.batch * args.height * args.width
    npix = nseg * seg_pix
    torch.manual_seed(0)
    x = torch.relu(torch.randn(npix, Cc, device=dev))
    w, b = torch.randn(Cc, device=dev) * 0.1, torch.zeros(1, device=dev)
    tg = torch.rand(npix, device=dev)
    y = torch.empty(npix, device=dev)
    arr = (C.c_void_p * nseg)(*[tg.data_ptr() + 4 * i * seg_pix for i in range(nseg)])
    scratch = torch.zeros(L.ramnet_pred_si_scratch_doubles(seg_pix, nseg), device=dev, dtype=torch.float64)
    stats = torch.empty(nseg, 4, device=dev, dtype=torch.float64)
    loss, gs = torch.empty(nseg, device=dev), torch.ones(nseg, device=dev)
    dx, dw, db = torch.empty(npix, Cc, device=dev), torch.zeros(Cc, device=dev), torch.zeros(1, device=dev)
    p = ops._p
    Hh.check(L.ramnet_pred_sigmoid_si_fwd(p(x), Cc, Cc, p(w), p(b), p(y), seg_pix, nseg, arr, 1.0, 1.0, p(scratch), p(stats), p(loss), ops._st()), "fwd")

    def full():
        Hh.check(L.ramnet_pred_sigmoid_si_bwd(p(x), Cc, Cc, p(w), p(y), None, seg_pix, nseg, arr, p(stats), p(gs), 1.0, 1.0, p(dx), Cc, p(dw), p(db),
                                              p(scratch), 1, ops._st()), "bwd")

    def dgrad():
        Hh.check(L.ramnet_pred_sigmoid_si_dgrad(p(x), Cc, Cc, p(w), p(y), None, seg_pix, nseg, arr, p(stats), p(gs), 1.0, 1.0, p(dx), Cc, 1,
                                                ops._st()), "dgrad")
    for fn in (full, dgrad):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    tf, td = [], []
    for _ in range(5):
        tf.append(_window(full, 200))
        td.append(_window(dgrad, 200))
    mb = npix * (2 * Cc + 2) * 4 / 1e6
    f, d = sorted(tf)[2], sorted(td)[2]
    emit(dict(what="pred_backward", npix=npix, C=Cc, nseg=nseg, mask_x=1, algorithmic_mb=round(mb, 1), us_full=round(f, 2), us_dgrad_only=round(d, 2),
              us_full_windows=[round(t, 2) for t in tf], us_dgrad_only_windows=[round(t, 2) for t in td],
              tb_s_full=round(mb / f, 3), tb_s_dgrad_only=round(mb / d, 3), hbm_frac_dgrad_only=round(mb / d / 8.0, 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["steps", "cells", "pred"])
    ap.add_argument("--sets", default="all,A,B")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq-len", type=int, default=8)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=344)
    ap.add_argument("--events-per-grid", type=int, default=200000)
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--tag", default="this")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    {"steps": steps, "cells": cells, "pred": pred}[args.what](args, emit)


if __name__ == "__main__":
    main()
