"""Isolated sweep of the folded decoders' backward-weights launch: F(2x2,4x4) (RAMNET_ALGO_WINOGRAD24) against F(2x3,4x4)
(RAMNET_ALGO_WINOGRAD24_2X3 on ramnet_wgrad_desc; csrc/conv_wgrad_wino24.hip) for the three decoder layers of the flagship workload over
the batch size, through raw descriptors (HIP-event time per launch, median of 5 windows of 10 launches; the two variants of a case are
timed alternately, window by window).  Prints one JSON line per (layer, batch) with ramnet_fold_wgrad_variant's "auto" answer, and the
cases where "auto" picked the slower variant.

    python tools/bench_fold23_wgrad.py [--batches 1,2,4,8,16,32]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rpg_ramnet_amd import _hip as Hh  # noqa: E402

DECODERS = [(256, 128, 32, 43), (128, 64, 64, 86), (64, 32, 128, 172)]     # (Cin, Cout, low-res H, W) at 256 x 344


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _window(L, d, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        L.ramnet_wgrad_launch(C.byref(d), None)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8,16,32")
    args = ap.parse_args()
    L = Hh.lib()
    dev = torch.device("cuda:0")
    rows = []
    for Cin, Cout, H, W in DECODERS:
        for B in [int(b) for b in args.batches.split(",")]:
            xpad = torch.relu(torch.randn(B, H + 4, W + 4, Cin, device=dev))
            g = torch.randn(B, 2 * H, 2 * W, Cout, device=dev)
            y = torch.relu(torch.randn(B, 2 * H, 2 * W, Cout, device=dev))          # the ReLU mask the decoders hand over
            dbias = torch.zeros(Cout, device=dev)
            descs = {}
            for tw, algo in ((2, Hh.ALGO_WINOGRAD24), (3, Hh.ALGO_WINOGRAD24_2X3)):
                ws = torch.zeros(4 * 5 * (tw + 3) * Cin * Cout, device=dev)
                d = Hh.WgradDesc()
                d.x0, d.ld0, d.C0, d.in_mode = _p(xpad), Cin, Cin, Hh.IN_PLAIN
                d.B, d.Hin, d.Win, d.stride, d.ntaps = B, H + 4, W + 4, 1, 16
                d.dout, d.gmask, d.ldg, d.ldgm = _p(g), _p(y), Cout, Cout
                d.Cout, d.Ho, d.Wo, d.HoG, d.WoG = Cout, H, W, 2 * H, 2 * W
                d.dw, d.dbias, d.algo = _p(ws), _p(dbias), algo
                descs[tw] = (d, ws)
            auto = L.ramnet_fold_wgrad_variant(C.byref(descs[2][0]), 0)
            ts = {2: [], 3: []}
            for tw in (2, 3):
                for _ in range(3):
                    assert L.ramnet_wgrad_launch(C.byref(descs[tw][0]), None) == 0, L.ramnet_last_error()
            for _ in range(5):
                for tw in (2, 3):
                    ts[tw].append(_window(L, descs[tw][0], 10))
            t22, t23 = sorted(ts[2])[2], sorted(ts[3])[2]
            flop23 = 2.0 * 30 * Cin * Cout * 4 * B * -(-H // 2) * -(-W // 3)          # executed by F(2x3): 30 positions per 2 x 3 tile and class
            r = dict(Cin=Cin, Cout=Cout, H=H, W=W, B=B, us_2x2=round(t22, 1), us_2x3=round(t23, 1), speedup=round(t22 / t23, 3),
                     min_2x2=round(min(ts[2]), 1), min_2x3=round(min(ts[3]), 1), tflops_exec_2x3=round(flop23 / t23 * 1e-6, 1),
                     auto_2x3=auto, auto_ok=bool((t23 < t22) if auto else True))
            rows.append(r)
            print(json.dumps(r), flush=True)
    print(json.dumps({"auto_picked_a_slower_launch": [(r["Cin"], r["B"]) for r in rows if not r["auto_ok"]]}))


if __name__ == "__main__":
    main()
