"""Isolated sweep of the F(2x3,4x4) decoder launches (RAMNET_ALGO_WINOGRAD24_2X3): the 8-wave workgroup (32 tiles, one per CU) against
the half workgroup (4 waves, 16 tiles, two per CU; ramnet_set_option("fold_half_wg")) for the forward (64 -> 32: the pair form) and
backward-data launches of the three decoder layers of the flagship workload over the batch size, through raw descriptors.  The two
variants alternate window by window (HIP-event time per launch, median of 5 windows of 10 launches each).  Prints one JSON line per
(layer, direction, batch) — auto_half = what ramnet_fold_halfwg_variant's "auto" rule picks for the launch — and a last line with the
launches where the rule picks a variant that measured slower.

    python tools/bench_fold23_halfwg.py [--batches 1,2,4,8,16,32] > profiles/fold23_halfwg_sweep.jsonl
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
        L.ramnet_conv_launch(C.byref(d), None)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def _time_pair(L, d, reps=10, windows=5):
    """Median window of each variant, the windows alternating 8-wave, half, 8-wave, ..."""
    ts = {0: [], 1: []}
    for mode in (0, 1):
        assert L.ramnet_set_option(b"fold_half_wg", mode) == 0
        for _ in range(3):
            assert L.ramnet_conv_launch(C.byref(d), None) == 0, L.ramnet_last_error()
    for _ in range(windows):
        for mode in (0, 1):
            L.ramnet_set_option(b"fold_half_wg", mode)
            ts[mode].append(_window(L, d, reps))
    return sorted(ts[0])[windows // 2], sorted(ts[1])[windows // 2]


def _wgs(L, d, half):
    r, c, n = C.c_int(), C.c_int(), C.c_long()
    assert L.ramnet_fold_halfwg_grid(C.byref(d), half, C.byref(r), C.byref(c), C.byref(n)) == 0
    return n.value, "%dx%d" % (r.value, c.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8,16,32")
    args = ap.parse_args()
    L = Hh.lib()
    dev = torch.device("cuda:0")
    old = L.ramnet_get_option(b"fold_half_wg")
    rows = []
    for Cin, Cout, H, W in DECODERS:
        w = torch.randn(Cout, Cin, 5, 5, device=dev) * 0.05
        bias = torch.randn(Cout, device=dev) * 0.1
        packs = {}
        for name, fn in (("f23", L.ramnet_pack_weight_fold_wino2x3), ("d23", L.ramnet_pack_weight_fold_wino2x3_dgrad)):
            packs[name] = torch.empty(L.ramnet_packed_weight_elems_fold_wino2x3(Cout, Cin), device=dev)
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
                d.algo, d.w = Hh.ALGO_WINOGRAD24_2X3, _p(packs["f23" if direction == "forward" else "d23"])
                L.ramnet_set_option(b"fold_half_wg", 2)
                auto = L.ramnet_fold_halfwg_variant(C.byref(d), 0)
                t8, t4 = _time_pair(L, d)
                (n32, blk32), (n16, blk16) = _wgs(L, d, 0), _wgs(L, d, 1)
                r = dict(Cin=Cin, Cout=Cout, H=H, W=W, B=B, direction=("pair" if direction == "forward" and Cout == 32 else direction),
                         wgs_8wave=n32, block_8wave=blk32, wgs_half=n16, block_half=blk16, us_8wave=round(t8, 2), us_half=round(t4, 2),
                         speedup=round(t8 / t4, 3), auto_half=auto)
                rows.append(r)
                print(json.dumps(r), flush=True)
    L.ramnet_set_option(b"fold_half_wg", old)
    wrong = [(r["Cin"], r["Cout"], r["B"], r["direction"]) for r in rows if r["auto_half"] and r["us_half"] > r["us_8wave"]]
    print(json.dumps({"auto_picks_half_where_it_measured_slower": wrong,
                      "half_faster": sum(r["us_half"] < r["us_8wave"] for r in rows), "launches": len(rows)}))


if __name__ == "__main__":
    main()
