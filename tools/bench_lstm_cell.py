"""Isolated ConvLSTM launches of the three state scales of the flagship workload (C = 64 / 128 / 256 at 128x172 / 64x86 / 32x43) over the
batch size: the cell launch (cat(x, h) * W, 2C -> 4C, cell epilogue) and the backward-data launch (4C -> 2C, LINEAR), F(2x2,3x3)
(ops.set_winograd_2x4("off")) against F(2x4,3x3) ("force"), through ops.conv_launch.  HIP-event time per launch: median of 3 windows of
>= 0.1 s after a warm-up.  One JSON line per (scale, direction, batch):

  us_2x2 / us_2x4   time per launch          gflop     algorithmic FLOP (2 * 9 * Cin * Cout per output pixel)
  tflops_*          gflop / time             useful_*  share of the executed MFMA products that land on real output pixels
                                                       (map area / area padded to the kernel's tiles; the F(2x4) kernel executes
                                                       3 products per output and channel pair, F(2x2) 4, direct 9)
  auto_2x4          ramnet_conv_wino_variant's choice without force, kernel_* = what the library reports

    python tools/bench_lstm_cell.py [--batches 1,2,4,8,16] [--fixed-reps N]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rpg_ramnet_amd import _hip as Hh, ops  # noqa: E402

SCALES = [(64, 128, 172), (128, 64, 86), (256, 32, 43)]


def _cdiv(a, b):
    return -(-a // b)


def _padded(H, W, shapes):
    return min(_cdiv(H, th) * th * _cdiv(W, tw) * tw for th, tw in shapes)


def _time(fn, target_s=0.1, windows=3, fixed=0):
    if fixed:                        # counter runs (rocprofv3 --pmc serialises dispatches): `fixed` launches, one window
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(fixed):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / fixed
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        fn()
    b.record()
    torch.cuda.synchronize()
    reps = max(10, int(target_s / max(a.elapsed_time(b) * 1e-3 / 10, 1e-6)))
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / reps)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--fixed-reps", type=int, default=0, help="exactly this many launches per case, no warm-up or calibration (counter runs)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = Hh.lib()
    taps, tapsd = ops.Taps.get("conv", 3, 1), ops.Taps.get("dgrad1", 3, 1)
    slower = []
    for Cc, H, W in SCALES:
        torch.manual_seed(Cc)
        w = torch.nn.Parameter(torch.randn(4 * Cc, 2 * Cc, 3, 3, device=dev) * 0.02)
        b = torch.nn.Parameter(torch.randn(4 * Cc, device=dev) * 0.1)
        cp = ops.ConvParam([w], [b], gates=4)
        for B in [int(v) for v in args.batches.split(",")]:
            x, h, c = (torch.randn(B, H, W, Cc, device=dev) for _ in range(3))
            hn, cn = torch.empty_like(x), torch.empty_like(x)
            gates = torch.empty(B, H, W, 4 * Cc, device=dev)
            dpre = torch.randn(B, H, W, 4 * Cc, device=dev)
            dxh = torch.empty(B, H, W, 2 * Cc, device=dev)
            launches = {
                "cell": lambda: ops.conv_launch(x, taps, cp.fwd(), hn, Cc, x1=h, in_mode=Hh.IN_CAT, C1=Cc, bias=cp.bias(), epi=Hh.EPI_LSTM,
                                                e1=c, o1=cn, o2=gates),
                "backward-data": lambda: ops.conv_launch(dpre, tapsd, cp.bwd(), dxh, 2 * Cc),
            }
            for direction, fn in launches.items():
                r = dict(C=Cc, H=H, W=W, B=B, direction=direction)
                flop = 2.0 * 9 * (2 * Cc) * (4 * Cc) * B * H * W
                r["gflop"] = round(flop / 1e9, 3)
                for mode, tag, shapes in (("off", "2x2", [(32, 4), (8, 16)]), ("force", "2x4", [(16, 16), (32, 8), (8, 32)])):
                    ops.set_winograd_2x4(mode)
                    try:
                        t = _time(fn, fixed=args.fixed_reps)
                        r["kernel_" + tag] = L.ramnet_last_kernel().decode()
                    finally:
                        ops.set_winograd_2x4("auto")
                    r["us_" + tag] = round(t, 2)
                    r["tflops_" + tag] = round(flop / t / 1e6, 1)
                    r["useful_" + tag] = round(H * W / _padded(H, W, shapes), 3)
                d = ops._conv_desc(x, taps, cp.fwd(), hn, Cc, x1=h, in_mode=Hh.IN_CAT, C1=Cc, bias=cp.bias(), epi=Hh.EPI_LSTM, e1=c, o1=cn,
                                   o2=gates) if direction == "cell" else ops._conv_desc(dpre, tapsd, cp.bwd(), dxh, 2 * Cc)
                r["auto_2x4"] = int(d.algo == Hh.ALGO_WINOGRAD_2X4)
                r["speedup"] = round(r["us_2x2"] / r["us_2x4"], 3)
                if r["auto_2x4"] and r["us_2x4"] > r["us_2x2"]:
                    slower.append((Cc, B, direction))
                print(json.dumps(r), flush=True)
    print(json.dumps({"auto_cases_slower_on_2x4": slower}))


if __name__ == "__main__":
    main()
