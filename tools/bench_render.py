"""Timing of the device renderer (rpg_ramnet_amd.render, csrc/render.hip) next to a host numpy / matplotlib statement of the same outputs.
One JSON line per measurement; record: profiles/render_notes.md.

    python tools/bench_render.py [--rounds 7] [--packages 50] [--kernels-only]

One data package of test.py at 260 x 346 and K = 5, resident on the device: 6 predictions and 6 targets (20 % NaN in the targets), 5 event
tensors of 5 channels and one frame, 6 (prediction, target) pairs for the scale.
(a) the device path: render.render_package (colour, grey, input previews, the scale riding in its first launch), ONE copy of the uint8
    buffer to the host and the copy of the six scales;
(b) the host path: the maps and inputs copied to the host as float32, then numpy and matplotlib do what test.py does up to cv2.imwrite's
    argument, rounded to uint8: make_colormap through a ScalarMappable, img * 255, the event / frame previews, the float32 scale.
(a) and (b) alternate --rounds times in one process, --packages packages per timed window; a window is wall time that ends in a device
synchronise; the outputs of both are compared once.  Writing the PNG files is the same work on both paths and is left out.
Then each entry point alone, --packages calls between two device events: microseconds per call and the bytes it has to move (computed
from the shapes below) per second, as a share of the HBM peak of 8 TB/s.  --kernels-only runs just that part: the run to put under
rocprofv3 --kernel-trace --stats for the time of each kernel."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rpg_ramnet_amd import render as R  # noqa: E402

CLIP, REG, K, H, W, CE = 1000.0, 5.70378, 5, 260, 346, 5
HBM_PEAK = 8.0e12


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def sat_u8(x):
    with np.errstate(invalid="ignore"):
        r = np.rint(x)
        return np.where(np.isnan(r), 0, np.clip(r, 0, 255)).astype(np.uint8)


def host_package(maps, inputs, kinds, pairs, mappable):
    """test.py:262-378 for one package from host float32 arrays."""
    color, grey, rgb, scale = [], [], [], []
    with np.errstate(all="ignore"):
        for m in maps:
            grey.append(sat_u8(m * 255.0))
            inv = np.nan_to_num(np.ones_like(m) * np.amax(m) - m, nan=1)
            q = np.nan_to_num(inv / np.amax(inv))
            color.append(sat_u8(mappable.to_rgba(q) * 255.0))
        for x, kind in zip(inputs, kinds):
            s = np.sum(x, axis=0)
            if kind == R.KIND_EVENTS:
                rgb.append(sat_u8(np.stack([np.where(s > 0.9, 1.0, 0.0), np.zeros_like(s), np.where(s <= -0.5, 1.0, 0.0)], axis=2) * 255.0))
            else:
                rgb.append(np.repeat(sat_u8(s * np.float32(255.0))[:, :, None], 3, axis=2))
        for p, t in pairs:
            pm = np.exp(REG * (p - np.ones(p.shape, dtype=np.float32))) * CLIP
            tm = np.exp(REG * (t - np.ones(t.shape, dtype=np.float32))) * CLIP
            scale.append(np.sum(pm * tm) / np.sum(pm * pm))
    return np.stack(color), np.stack(grey), np.stack(rgb), np.array(scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--packages", type=int, default=50)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    targets = [torch.rand(1, 1, H, W, device=dev, generator=g) for _ in range(K + 1)]
    preds = [(t + 0.08 * torch.randn(1, 1, H, W, device=dev, generator=g)).clamp(0, 1) for t in targets]
    for t in targets:
        t[torch.rand(1, 1, H, W, device=dev, generator=g) < 0.2] = float("nan")
    events = [torch.randn(1, CE, H, W, device=dev, generator=g) * 0.5 for _ in range(K)]
    frame = torch.rand(1, 1, H, W, device=dev, generator=g)
    inputs, kinds = events + [frame], [R.KIND_EVENTS] * K + [R.KIND_FRAME]
    clean = [torch.rand(1, 1, H, W, device=dev, generator=g) for _ in range(K + 1)]          # NaN-free targets for the scale
    mapper = R.ColorMapper(0.04, 0.83)
    maps = preds + targets
    npix, G, Gi = H * W, len(maps), len(inputs)

    def device_package():
        buf, _, _, _, s = R.render_package(maps, mapper, inputs, kinds, scale=(preds, clean, CLIP, REG))
        return buf.cpu().numpy(), s.cpu().numpy()

    def device_path():
        for _ in range(args.packages):
            out = device_package()
        return out

    # bytes each entry point has to move: maps read twice (statistics, map) and 5 bytes per pixel written; pairs read once; inputs read once
    bytes_depth = G * npix * (4 + 4 + 5)
    bytes_scale = (K + 1) * npix * 8
    bytes_inputs = npix * (4 * (K * CE + 1) + 3 * Gi)
    device_package()                                        # warm-up: library load, workspace, table upload
    if not args.kernels_only:
        import matplotlib as mpl
        import matplotlib.cm as cm
        mappable = cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=mapper.vmin, vmax=mapper.vmax), cmap="magma")

        def host_package_from_device():
            hm = [m[0, 0].cpu().numpy() for m in maps]
            hi = [x[0].cpu().numpy() for x in inputs]
            hp = [(p[0, 0].cpu().numpy(), t[0, 0].cpu().numpy()) for p, t in zip(preds, clean)]
            return host_package(hm, hi, kinds, hp, mappable)

        def host_path():
            for _ in range(args.packages):
                out = host_package_from_device()
            return out

        host_package_from_device()
        dev_ms, host_ms = [], []
        for r in range(args.rounds):
            ms_d, (buf, s) = wall_ms(device_path)
            ms_h, (hc, hg, hr, hs) = wall_ms(host_path)
            dev_ms.append(ms_d / args.packages), host_ms.append(ms_h / args.packages)
            color, grey, rgb = R.split_package(buf, G, Gi, (H, W))
            print(json.dumps(dict(what="render_package", round=r, packages=args.packages, H=H, W=W, K=K, ms_per_package_device=round(dev_ms[-1], 4),
                                  ms_per_package_host=round(host_ms[-1], 3), host_over_device=round(host_ms[-1] / dev_ms[-1], 1),
                                  same_colour=bool(np.array_equal(color, hc)), same_grey=bool(np.array_equal(grey, hg)),
                                  same_inputs=bool(np.array_equal(rgb, hr)), scale_rel_diff=float(np.max(np.abs(s / hs - 1))))), flush=True)
        print(json.dumps(dict(what="render_package_summary", rounds=args.rounds, ms_device_median=round(statistics.median(dev_ms), 4),
                              ms_device_min=round(min(dev_ms), 4), ms_device_max=round(max(dev_ms), 4), ms_host_median=round(statistics.median(host_ms), 3),
                              ms_host_min=round(min(host_ms), 3), ms_host_max=round(max(host_ms), 3))), flush=True)
    calls = max(args.packages, 200)
    for name, nbytes, fn in (("render_depth (statistics + map kernel)", bytes_depth, lambda: R.render_depth(maps, mapper)),
                             ("least_squares_scale (statistics kernel)", bytes_scale, lambda: R.least_squares_scale(preds, clean, CLIP, REG)),
                             ("render_inputs", bytes_inputs, lambda: R.render_inputs(inputs, kinds))):
        fn()
        us = [event_us(fn, calls) for _ in range(args.rounds)]
        med = statistics.median(us)
        print(json.dumps(dict(what="entry_point", name=name, calls=calls, bytes=nbytes, us_per_call_median=round(med, 2), us_per_call_min=round(min(us), 2),
                              us_per_call_max=round(max(us), 2), bytes_per_second=round(nbytes / (med * 1e-6), -6),
                              share_of_hbm_peak=round(nbytes / (med * 1e-6) / HBM_PEAK, 4),
                              note="call time between device events: pointer-table fill and host launch path included")), flush=True)


if __name__ == "__main__":
    main()
