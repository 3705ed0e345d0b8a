#!/usr/bin/env python3
"""The cost of the deterministic mode (ops.set_deterministic) at the bench shape: the configs[1] training step — B = 8, L = 8, K = 5, 256 x 344,
SI loss on [image, events4], bench.py's schedule (backward-weights side stream, decoder stream, deferred cell launches), fused Adam,
resident inputs — in both modes in alternation in ONE process on one box; the extra device memory the mode keeps (slabs, bias slabs,
partial buffers), asserted below 1 GiB; and the slab forms of the backward-weights kernels against their atomic twins, each alone on an
idle chip at the shapes of that step.  Prints a table and one JSON line.
Usage (GPU box): python tools/bench_deterministic.py [--rounds 3] [--steps 3] [--batch 8] [--seq-len 8] [--no-kernels]"""
import argparse
import contextlib
import gc
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rpg_ramnet_amd import ops, _hip as H  # noqa: E402

GIB = 1 << 30


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def det_buffers():
    """bytes of what the mode alone allocates on the layers: slabs beyond the first of the fold workspaces, the direct parity slabs, the
    direct / head slabs beyond the default workspace, the bias slabs beyond one row, the partial buffers"""
    out = {"fold_slabs": 0, "fold_direct_slabs": 0, "direct_head_slabs": 0, "bias_slabs": 0, "partials": 0}
    for cp in [o for o in gc.get_objects() if isinstance(o, ops.ConvParam)]:
        ws = {name: r.t for name, r in cp.workspaces()}
        det = {name: ops._det_slabs(t) for name, t in ws.items()}       # (the stamp of the last pass; 0 on a workspace never asked for)
        for name in ("fold24", "fold23"):
            if det[name] > 1:
                out["fold_slabs"] += ws[name].numel() * 4 * (det[name] - 1) // det[name]
        if ws["fold_direct"] is not None:
            out["fold_direct_slabs"] += ws["fold_direct"].numel() * 4
        if det["main"] > 1:
            out["direct_head_slabs"] += (det["main"] - 1) * cp._slab_floats("direct") * 4
        if ws["bias"] is not None and ws["bias"].numel() > cp.Cout and (ws["fold_direct"] is not None or det["main"] + det["fold24"] + det["fold23"] > 0):
            out["bias_slabs"] += (ws["bias"].numel() - cp.Cout) * 4
        out["partials"] += sum(b.numel() * b.element_size() for b in cp._part.values())
    out["total"] = sum(out.values())
    return out


def step_times(a):
    import bench
    from rpg_ramnet_amd.model.model import ERGB2DepthRecurrent
    from rpg_ramnet_amd.trainer import sequence_loss
    K, bins = 5, 5
    ops.set_wgrad_overlap(True)
    ops.set_decoder_overlap(True)
    ops.set_wgrad_defer(2)
    cfg = dict(bench.RELEASED, num_bins_events=bins, gpu=0, every_x_rgb_frame=K, baseline=False, loss_composition=["image", "events4"])
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        model = ERGB2DepthRecurrent(cfg)
    model = model.to(model.gpu).train()
    seq = bench.synth_sequence(model, a.batch, a.seq_len, a.height, a.width, K, bins, a.events_per_grid, seed=1000)
    opt = torch.optim.Adam(model.parameters(), lr=3e-4, weight_decay=0, fused=True)

    def step():
        opt.zero_grad()
        total, _ = sequence_loss(model, seq, cfg["loss_composition"], [1, 1])
        total.backward()
        opt.step()
        return total

    times = {False: [], True: []}
    mem = {}
    for rnd in range(a.rounds):
        for det in (False, True):
            ops.set_deterministic(det)
            step()                                  # (the first step of a mode allocates its workspaces)
            torch.cuda.synchronize()
            if det not in mem:
                gc.collect()
                mem[det] = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            times[det].append((time.perf_counter() - t0) * 1e3 / a.steps)
            print("round %d  deterministic=%-5s  %.1f ms per step" % (rnd, det, times[det][-1]), flush=True)
    ops.set_deterministic(False)
    bufs = det_buffers()
    peak = torch.cuda.max_memory_allocated()
    return times, mem, bufs, peak


def kernel_pairs(a):
    """slab form against atomic form, one launch alone: the three decoders' backward-weights at the launch batch of a time step (B) and of a
    time-batched group (K B), and the head layers'"""
    dev = torch.device("cuda:0")
    rows = []
    Hb, Wb = a.height, a.width
    for (cin, cout, div) in ((256, 128, 8), (128, 64, 4), (64, 32, 2)):
        for batch in (a.batch, 5 * a.batch):
            Hh, Ww = Hb // div, Wb // div
            w = torch.nn.Parameter(torch.randn(cout, cin, 5, 5, device=dev) * 0.01)
            cp = ops.ConvParam([w], [torch.nn.Parameter(torch.zeros(cout, device=dev))])
            xpad = torch.randn(batch, Hh + 4, Ww + 4, cin, device=dev)
            dy, y = torch.randn(batch, 2 * Hh, 2 * Ww, cout, device=dev), torch.randn(batch, 2 * Hh, 2 * Ww, cout, device=dev)
            kind = "fold23" if ops._fold_wgrad_2x3(batch, Hh, Ww, cin, cout) else "fold24"
            t = {}
            for det in (False, True):
                ops.set_deterministic(det)
                bws = cp.grad_ws_fold()[3]
                ws = cp.grad_ws_fold24(kind)

                def launch():
                    ops.wgrad_launch(xpad, ops.Taps.get("fold", 4, 0, 0, 0), dy, ws, cout, gmask=y, dbias=bws, Ho=Hh, Wo=Ww,
                                     gview=(0, 0, 0, 0, 2 * Hh, 2 * Ww), wino24=ops._FOLD_LAYOUTS[kind][1])
                def launch_nobias():        # (the slab form's bias gradient is a kernel of its own: without it, the Winograd kernel alone)
                    ops.wgrad_launch(xpad, ops.Taps.get("fold", 4, 0, 0, 0), dy, ws, cout, gmask=y, Ho=Hh, Wo=Ww,
                                     gview=(0, 0, 0, 0, 2 * Hh, 2 * Ww), wino24=ops._FOLD_LAYOUTS[kind][1])
                t[det] = (timeit(launch, a.reps), H.lib().ramnet_last_kernel().decode(), ops._det_slabs(ws), timeit(launch_nobias, a.reps))
                cp.discard()
            ops.set_deterministic(False)
            rows.append(("decoder %d->%d B=%d %dx%d" % (cin, cout, batch, Hh, Ww), t))
            del cp, xpad, dy, y
    for cin, c0 in ((1, 4), (5, 8)):
        batch = 5 * a.batch
        w = torch.nn.Parameter(torch.randn(32, cin, 5, 5, device=dev) * 0.01)
        cp = ops.ConvParam([w], [torch.nn.Parameter(torch.zeros(32, device=dev))])
        x, dy = torch.randn(batch, Hb, Wb, c0, device=dev), torch.randn(batch, Hb, Wb, 32, device=dev)
        t = {}
        for det in (False, True):
            ops.set_deterministic(det)
            ws, bws = cp.grad_ws()

            def launch():
                ops.wgrad_launch(x, ops.Taps.get("conv", 5, 2), dy, ws, 32, gmask=dy, dbias=bws)
            t[det] = (timeit(launch, a.reps), H.lib().ramnet_last_kernel().decode(), ops._det_slabs(ws))
            cp.discard()
            cp._dirty = False
        ops.set_deterministic(False)
        rows.append(("head %d->32 B=%d %dx%d" % (cin, batch, Hb, Wb), t))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq-len", type=int, default=8)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=344)
    ap.add_argument("--events-per-grid", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    res = {"shape": "B=%d L=%d K=5 %dx%d" % (a.batch, a.seq_len, a.height, a.width)}
    if not a.no_step:
        times, mem, bufs, peak = step_times(a)
        for det in (False, True):
            ts = times[det]
            print("deterministic=%-5s  ms per step: %s  (min %.1f, median %.1f, max %.1f)" % (
                det, " ".join("%.1f" % t for t in ts), min(ts), sorted(ts)[len(ts) // 2], max(ts)))
        extra = mem[True] - mem[False]
        print("device memory held after a step: default %.3f GiB, deterministic %.3f GiB: + %.1f MiB;  peak %.2f GiB" % (
            mem[False] / GIB, mem[True] / GIB, extra / 2 ** 20, peak / GIB))
        print("the mode's own buffers on the layers (MiB): " + ", ".join("%s %.1f" % (k, v / 2 ** 20) for k, v in bufs.items()))
        assert max(extra, bufs["total"]) < GIB, "the deterministic mode's extra workspace passes 1 GiB at the bench shape"
        res.update(ms_default=times[False], ms_deterministic=times[True], extra_bytes_allocated=extra, det_buffers=bufs, peak_bytes=peak)
    if not a.no_kernels:
        rows = kernel_pairs(a)
        print("%-36s %10s %10s %7s %6s %22s  %s" % ("launch", "atomic ms", "slab ms", "ratio", "slabs", "no dbias: atomic, slab", "slab kernel"))
        for name, t in rows:
            nb = "%.3f, %.3f" % (t[False][3], t[True][3]) if len(t[True]) > 3 else "-"
            print("%-36s %10.3f %10.3f %7.2f %6d %22s  %s" % (name, t[False][0], t[True][0], t[True][0] / t[False][0], t[True][2], nb, t[True][1]))
        res["kernels"] = [dict(launch=n, atomic_ms=t[False][0], slab_ms=t[True][0], slabs=t[True][2], atomic_kernel=t[False][1], slab_kernel=t[True][1],
                               atomic_ms_no_dbias=t[False][3] if len(t[False]) > 3 else None, slab_ms_no_dbias=t[True][3] if len(t[True]) > 3 else None)
                          for n, t in rows]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
