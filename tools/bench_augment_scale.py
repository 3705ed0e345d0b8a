"""Isolated timing of the device augmentation with the datasets' scale_factor resize fused in (csrc/augment.hip: augment_scale_kernel) at the
training recipe's shapes, alternating with the two-step path that gives the same result without it: `augment.apply` followed by torch's
F.interpolate on the device (and, for the model's NHWC layout, the NCHW -> NHWC repack).  One JSON line per measurement; record:
profiles/augment_scale_notes.md.

    python tools/bench_augment_scale.py [--launches 100] [--rounds 3] [--window-ms 300]

Shapes: one B=8, L=8, K=5 step = 64 samples x (5 five-bin grids + 1 frame + 6 targets) at 260x346 with a 224x224 window and at 256x344 with
the whole image as window, scale_factor 0.5.  Bytes counted: the window read once + the reduced output written once."""
import argparse
import json
import os
import random
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rpg_ramnet_amd import augment as A  # noqa: E402
from rpg_ramnet_amd import data as D  # noqa: E402

PEAK = 8.0e12          # bytes / s the project quotes for the MI355X
S = 0.5
SHAPES = ((260, 346, 224, 224), (256, 344, 256, 344))
GROUPS = (("grids", 320, 5), ("frames", 64, 1), ("targets", 384, 1))


def _window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timed(fn, n, window_ms, warm=10):
    """ms per call over a window of at least n calls and about window_ms (a window of a few ms times the clock, not the kernel)"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    n = max(n, int(window_ms / max(_window(fn, 20) / 20, 1e-4)))
    return _window(fn, n) / n, n


def main(args):
    from rpg_ramnet_amd import ops
    dev = torch.device("cuda:0")
    for H, W, th, tw in SHAPES:
        transform = D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.0), D.RandomCrop([th, tw])])
        params = [A.draw(transform, 1000 + s, H, W, rng=random.Random()) for s in range(64)]
        table = A.ParamTable(params, H, W).to(dev)
        _, oh, ow = A.scaled_shape(th, tw, S)
        totals = {}
        for name, G, Cc in GROUPS:
            x = torch.randn(G, Cc, H, W, device=dev)
            pidx = (torch.arange(G, dtype=torch.int32) % 64).to(dev)
            cp = (Cc + 3) // 4 * 4
            full = torch.empty(G, Cc, th, tw, device=dev)
            n = G * Cc * oh * ow
            small = torch.empty(n + 4, device=dev)
            out = {"nchw": small[:n].view(G, Cc, oh, ow), "nchw_per_pixel": small[1:n + 1].view(G, Cc, oh, ow),     # (one float off 16 bytes)
                   "nhwc": torch.empty(G, oh, ow, cp, device=dev)}
            nbytes = 4 * G * Cc * (th * tw + oh * ow)

            def two_step(nhwc):
                A.apply(x, table, pidx=pidx, out=full)
                y = F.interpolate(full, scale_factor=S, mode="bilinear", align_corners=False, recompute_scale_factor=False)
                return ops.pack_input(y, dev) if nhwc else y

            runs = {"fused nchw": lambda: A.apply(x, table, pidx=pidx, out=out["nchw"], scale_factor=S),
                    "two-step nchw": lambda: two_step(False),
                    "fused nchw, per-pixel path": lambda: A.apply(x, table, pidx=pidx, out=out["nchw_per_pixel"], scale_factor=S),
                    "fused nhwc": lambda: A.apply(x, table, pidx=pidx, out=out["nhwc"], nhwc=True, scale_factor=S),
                    "two-step nhwc": lambda: two_step(True)}
            assert out["nchw"].data_ptr() % 16 == 0 and out["nchw_per_pixel"].data_ptr() % 16 == 4 and (Cc * oh * ow) % 4 == 0
            for r in range(args.rounds):                                  # alternating: every variant once per round
                for what, fn in runs.items():
                    ms, calls = timed(fn, args.launches, args.window_ms)
                    print(json.dumps(dict(path=what, round=r, group=name, G=G, C=Cc, image=[H, W], window=[th, tw], out=[oh, ow], calls=calls, ms=round(ms, 5),
                                          GBps=round(nbytes / ms / 1e6, 1), share_of_peak=round(nbytes / (ms * 1e-3) / PEAK, 3))), flush=True)
                    totals.setdefault(what, []).append(ms)
            del x, full, small, out
        per_step = {what: round(sum(min(ms[g * args.rounds:(g + 1) * args.rounds]) for g in range(len(GROUPS))), 4) for what, ms in totals.items()}
        print(json.dumps(dict(summary="one step's three groups, best round of each", image=[H, W], window=[th, tw], ms=per_step)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=300.0, help="least length of a timed window")
    main(ap.parse_args())
