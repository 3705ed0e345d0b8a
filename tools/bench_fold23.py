"""Isolated sweep of the folded decoder launches: F(2x2,4x4) (RAMNET_ALGO_WINOGRAD24) against F(2x3,4x4) (RAMNET_ALGO_WINOGRAD24_2X3)
for the forward and backward-data launches of the three decoder layers of the flagship workload over the batch size, through raw
descriptors (HIP-event time per launch, median of 5 windows of 10 launches).  The F(2x2) forward runs with the split reduction the
library would pick.  Prints one JSON line per (layer, direction, batch) and the smallest launch size (2x3 workgroups) from which F(2x3)
is never slower; ramnet_fold_wino_variant's "auto" estimate (csrc/conv_wino24.hip) was checked against this sweep (auto_2x3 = its
choice for the launch).

    python tools/bench_fold23.py [--batches 1,2,4,8,16,32]
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


def _cdiv(a, b):
    return -(-a // b)


def _wgs23(d):
    """Workgroups of the F(2x3) launch of descriptor d (csrc/conv_wino24.hip: wino23_tile)."""
    dg = d.in_mode == Hh.IN_PARITY4
    pair = not dg and d.Cout == 32
    Wt = d.Wo + 1 if pair else d.Wo
    best = min((_cdiv(d.Ho, 64 // t) * _cdiv(Wt, 3 * t), t) for t in (4, 2, 16))
    nblk = d.Cout // 64 if (dg or not pair) else 1
    return best[0] * d.B * nblk * (1 if dg else 2 if pair else 4)


def _time(L, d, reps=10, windows=5):
    for _ in range(3):
        assert L.ramnet_conv_launch(C.byref(d), None) == 0, L.ramnet_last_error()
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            L.ramnet_conv_launch(C.byref(d), None)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / reps)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8,16,32")
    args = ap.parse_args()
    L = Hh.lib()
    dev = torch.device("cuda:0")
    rows = []
    for Cin, Cout, H, W in DECODERS:
        w = torch.randn(Cout, Cin, 5, 5, device=dev) * 0.05
        bias = torch.randn(Cout, device=dev) * 0.1
        packs = {}
        for name, n, fn in (("f22", L.ramnet_packed_weight_elems_fold_wino(Cout, Cin), L.ramnet_pack_weight_fold_wino),
                            ("d22", L.ramnet_packed_weight_elems_fold_wino(Cout, Cin), L.ramnet_pack_weight_fold_wino_dgrad),
                            ("f23", L.ramnet_packed_weight_elems_fold_wino2x3(Cout, Cin), L.ramnet_pack_weight_fold_wino2x3),
                            ("d23", L.ramnet_packed_weight_elems_fold_wino2x3(Cout, Cin), L.ramnet_pack_weight_fold_wino2x3_dgrad)):
            packs[name] = torch.empty(n, device=dev)
            assert fn(_p(w), _p(packs[name]), Cout, Cin, None) == 0
        for B in [int(b) for b in args.batches.split(",")]:
            xpad = torch.randn(B, H + 4, W + 4, Cin, device=dev)
            y = torch.empty(B, 2 * H, 2 * W, Cout, device=dev)
            g = torch.randn(B, 2 * H, 2 * W, Cout, device=dev)
            dx = torch.empty(B, H + 4, W + 4, Cin, device=dev)
            for direction in ("forward", "backward-data"):
                d = Hh.ConvDesc()
                if direction == "forward":
                    d.x0, d.ld0, d.C0, d.in_mode = _p(xpad), Cin, Cin, Hh.IN_PLAIN
                    d.B, d.Hin, d.Win, d.stride, d.ntaps = B, H + 4, W + 4, 1, 16
                    d.bias, d.Cout, d.Ho, d.Wo, d.HoF, d.WoF = _p(bias), Cout, H, W, 2 * H, 2 * W
                    d.epi, d.out, d.ldo = Hh.EPI_RELU, _p(y), Cout
                else:
                    d.x0, d.ld0, d.C0, d.in_mode = _p(g), Cout, Cout, Hh.IN_PARITY4
                    d.B, d.Hin, d.Win, d.stride, d.ntaps = B, 2 * H, 2 * W, 1, 16
                    d.Cout, d.Ho, d.Wo, d.HoF, d.WoF = Cin, H + 4, W + 4, H + 4, W + 4
                    d.epi, d.out, d.ldo = Hh.EPI_LINEAR, _p(dx), Cin
                d.osy, d.osx = 1, 1
                d.algo, d.w = Hh.ALGO_WINOGRAD24, _p(packs["f22" if direction == "forward" else "d22"])
                auto = L.ramnet_fold_wino_variant(C.byref(d), 0)
                ws = None
                n = L.ramnet_conv_splitk_floats(C.byref(d))
                if n:
                    ws = torch.zeros(n, device=dev)
                    d.splitk_ws, d.splitk_floats = _p(ws), n
                t22 = _time(L, d)
                d.splitk_ws, d.splitk_floats = None, 0
                d.algo, d.w = Hh.ALGO_WINOGRAD24_2X3, _p(packs["f23" if direction == "forward" else "d23"])
                t23 = _time(L, d)
                r = dict(Cin=Cin, Cout=Cout, H=H, W=W, B=B, direction=direction, split=bool(n), wgs23=_wgs23(d), us_2x2=round(t22, 2),
                         us_2x3=round(t23, 2), speedup=round(t22 / t23, 3), auto_2x3=auto)
                rows.append(r)
                print(json.dumps(r), flush=True)
    slower = [r["wgs23"] for r in rows if r["us_2x3"] > r["us_2x2"]]
    print(json.dumps({"largest_launch_where_2x3_is_slower_wgs23": max(slower) if slower else 0}))


if __name__ == "__main__":
    main()
