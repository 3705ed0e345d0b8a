"""Timing of the batched evaluation table (metrics.EvalTable, csrc/metrics.hip) next to the per-frame path it replaces.  One JSON line per
measurement; record: profiles/eval_table_notes.md.

    python tools/bench_eval_table.py [--rounds 5] [--frames 256] [--nan-frac 0.1] [--table-only] [--rescale]

256 seeded pairs of 260 x 346 resident on the device, the six default cut-offs.  --nan-frac of the targets are NaN: with any NaN inside a
variant its medians are NaN and the two selection passes return at once; --nan-frac 0 makes every variant select its medians.
(a) the per-frame path: seven metrics.depth_metrics calls per pair, as inference.evaluate_folders issues them (a launch, a read-back of
    eleven doubles and up to two sorts each);
(b) metrics.EvalTable.add in batches of 64, then one result().
(a) and (b) alternate --rounds times in one process; every timed window is wall time that ends in a device synchronise; ms per frame.
Then (b) alone with ~30 % dense event masks (14 variants).  --table-only runs (b) once without and once with masks and nothing else: the
run to put under rocprofv3 --kernel-trace --stats for the kernel times.
--rescale (record: profiles/eval_rescale_notes.md): the plain and the rescaled table (EvalTable(rescale=True), four launches) alternate
--rounds times, without and with masks, next to (c) a torch-on-device restatement of rescale_by_the_median + the ten metrics per (file,
variant) on the first --torch-frames files, one read-back at the end.  Use --nan-frac 0: a NaN inside a variant ends its passes 2..4."""
import argparse
import json
import math
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
    ap.add_argument("--rescale", action="store_true")
    ap.add_argument("--torch-frames", type=int, default=32)
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

    def torch_rescaled(nf, ms=None):
        """rescale_by_the_median + add_to_metrics in float64 torch ops, per (file, variant); the entries stay on the device until the end."""
        out, eps = [], 1e-5
        lo = math.exp(-REG) * CLIP
        for f in range(nf):
            tm = (torch.exp(REG * (t[f] - 1.0)) * CLIP).double()
            pm = (torch.exp(REG * (p[f] - 1.0)) * CLIP).clamp(lo, CLIP).double()
            for half in ((None,) if ms is None else (None, ms[f])):
                for c in cuts:
                    keep = torch.nan_to_num(tm) < c
                    if half is not None:
                        keep = keep & half
                    xs = []
                    for x in (tm[keep], pm[keep]):
                        x = (x - x.median()) / x.std(unbiased=False)
                        xs.append(x + x.min().abs())
                    a, b = xs
                    ma, mb = a.median(), b.median()
                    md = (ma - mb).abs()
                    a, b = torch.where(ma < mb, a + md, a), torch.where(ma < mb, b, b + md)
                    d, ld = (a - b).abs(), torch.log(a + eps) - torch.log(b + eps)
                    r = torch.maximum(a / (b + eps), b / (a + eps))
                    out.append(torch.stack([(d / (a + 1e-6)).mean(), (d * d / (a * a + 1e-6)).mean(), (d * d).mean().sqrt(), (ld * ld).mean().sqrt(),
                                            (ld * ld).mean() - ld.mean() ** 2, d.mean(), (a.median() - b.median()).abs(), (r <= 1.25).double().mean(),
                                            (r <= 1.25 ** 2).double().mean(), (r <= 1.25 ** 3).double().mean()]))
        return torch.stack(out).cpu()

    def table(ms=None, rescale=False):
        tab = M.EvalTable(CLIP, REG, rescale=rescale)
        for f0 in range(0, F, BATCH):
            tab.add(p[f0:f0 + BATCH], t[f0:f0 + BATCH], None if ms is None else ms[f0:f0 + BATCH])
        return tab.result()

    table(), table(masks)                                   # warm-up: workspace allocation, library load
    if args.rescale:
        nf = min(F, args.torch_frames)
        table(None, True), table(masks, True), torch_rescaled(2, masks)
        for ms in (None, masks):
            for r in range(args.rounds):
                ms_p, a = wall_ms(lambda: table(ms))
                ms_r, b = wall_ms(lambda: table(ms, True))
                ms_t, c = wall_ms(lambda: torch_rescaled(nf, ms))
                print(json.dumps(dict(what="eval_rescale", masks=ms is not None, round=r, frames=F, H=Hh, W=W, nan_frac=args.nan_frac,
                                      ms_per_frame_plain=round(ms_p / F, 5), ms_per_frame_rescaled=round(ms_r / F, 5),
                                      rescaled_over_plain=round(ms_r / ms_p, 3), torch_frames=nf, ms_per_frame_torch=round(ms_t / nf, 4),
                                      torch_over_rescaled=round((ms_t / nf) / (ms_r / F), 1), abs_rel_diff_plain=a["abs_rel_diff"],
                                      abs_rel_diff_rescaled=b["abs_rel_diff"], abs_rel_diff_torch_first_files=float(c[::len(cuts) * (1 if ms is None else 2), 0].mean()))),
                      flush=True)
        return
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
