"""Timing of the batched evaluation table (metrics.EvalTable, csrc/metrics.hip) next to the per-frame path it replaces.  One JSON line per
measurement; record: profiles/eval_table_notes.md.

    python tools/bench_eval_table.py [--rounds 5] [--frames 256] [--nan-frac 0.1] [--table-only]

256 seeded pairs of 260 x 346 resident on the device, the six default cut-offs.  --nan-frac of the targets are NaN: with any NaN inside a
variant its medians are NaN and the two selection passes return at once; --nan-frac 0 makes every variant select its medians.
(a) the per-frame path: seven metrics.depth_metrics calls per pair, as inference.evaluate_folders issues them (a launch, a read-back of
    eleven doubles and up to two sorts each);
(b) metrics.EvalTable.add in batches of 64, then one result().
(a) and (b) alternate --rounds times in one process; every timed window is wall time that ends in a device synchronise; ms per frame.
Then (b) alone with ~30 % dense event masks (14 variants).  --table-only runs (b) once without and once with masks and nothing else: the
run to put under rocprofv3 --kernel-trace --stats for the kernel times."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rpg_ramnet_amd import metrics as M  # noqa: E402

CLIP, REG, BATCH = 80.0, 3.70378, 64


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--nan-frac", type=float, default=0.1)
    ap.add_argument("--table-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    F, Hh, W = args.frames, 260, 346
    g = torch.Generator(device=dev).manual_seed(0)
    t = torch.rand(F, Hh, W, device=dev, generator=g)
    p = (t + 0.08 * torch.randn(F, Hh, W, device=dev, generator=g)).clamp(0, 1)
    if args.nan_frac > 0:
        t[torch.rand(F, Hh, W, device=dev, generator=g) < args.nan_frac] = float("nan")
    masks = torch.rand(F, Hh, W, device=dev, generator=g) < 0.3
    cuts = [float("inf")] + [float(c) for c in M.EVAL_CUTOFFS]

    def per_frame():
        out = []
        for f in range(F):
            out.append([M.depth_metrics(p[f], t[f], CLIP, REG, cutoff=c) for c in cuts])
        return out

    def table(ms=None):
        tab = M.EvalTable(CLIP, REG)
        for f0 in range(0, F, BATCH):
            tab.add(p[f0:f0 + BATCH], t[f0:f0 + BATCH], None if ms is None else ms[f0:f0 + BATCH])
        return tab.result()

    table(), table(masks)                                   # warm-up: workspace allocation, library load
    if args.table_only:
        for ms in (None, masks):
            ms_b, _ = wall_ms(lambda: table(ms))
            print(json.dumps(dict(what="table_only", masks=ms is not None, frames=F, nan_frac=args.nan_frac, ms_per_frame=round(ms_b / F, 5))), flush=True)
        return
    per_frame()
    for r in range(args.rounds):
        ms_a, a = wall_ms(per_frame)
        ms_b, b = wall_ms(table)
        old = sum(m["abs_rel_diff"] for m in (row[0] for row in a)) / F
        print(json.dumps(dict(what="eval_table", round=r, frames=F, H=Hh, W=W, nan_frac=args.nan_frac, cutoffs=len(M.EVAL_CUTOFFS), ms_per_frame_per_pair_path=round(ms_a / F, 4),
                              ms_per_frame_table=round(ms_b / F, 5), ratio=round(ms_a / ms_b, 1), abs_rel_diff_per_pair_path=old,
                              abs_rel_diff_table=b["abs_rel_diff"])), flush=True)
    for r in range(args.rounds):
        ms_b, b = wall_ms(lambda: table(masks))
        print(json.dumps(dict(what="eval_table_masks", round=r, frames=F, variants=14, nan_frac=args.nan_frac, ms_per_frame_table=round(ms_b / F, 5),
                              event_masked_abs_rel_diff=b["event_masked_abs_rel_diff"])), flush=True)


if __name__ == "__main__":
    main()
