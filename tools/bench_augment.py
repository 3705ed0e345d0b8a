"""Isolated timing of the device augmentation (csrc/augment.hip) at the training recipe's shapes, next to the NCHW -> NHWC repack on the same
tensors and to what the host path costs for the same batch.  One JSON line per measurement; record: profiles/augment_notes.md.

    python tools/bench_augment.py [--launches 200] [--no-host]

Shapes: one B=8, L=8, K=5 step = 64 samples x (5 five-bin grids + 1 frame + 6 targets) at 260x346, cropped to 224x224 and to 256x344."""
import argparse
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rpg_ramnet_amd import augment as A  # noqa: E402
from rpg_ramnet_amd import data as D  # noqa: E402

PEAK = 8.0e12          # bytes / s the project quotes for the MI355X
H, W = 260, 346
GROUPS = (("grids", 320, 5), ("frames", 64, 1), ("targets", 384, 1))


def timed(fn, n, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n          # ms per call


def device_side(args):
    from rpg_ramnet_amd import _hip, ops
    dev = torch.device("cuda:0")
    L = _hip.lib()
    for size in ((224, 224), (256, 344)):
        transform = D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.0), D.RandomCrop(list(size))])
        params = [A.draw(transform, 1000 + s, H, W, rng=random.Random()) for s in range(64)]
        table = A.ParamTable(params, H, W).to(dev)
        total_ms = 0.0
        for name, G, Cc in GROUPS:
            x = torch.randn(G, Cc, H, W, device=dev)
            pidx = (torch.arange(G, dtype=torch.int32) % 64).to(dev)
            for nhwc in (False, True):
                cp = (Cc + 3) // 4 * 4
                out = torch.empty((G, size[0], size[1], cp) if nhwc else (G, Cc, size[0], size[1]), device=dev)
                ms = timed(lambda: A.apply(x, table, pidx=pidx, out=out, nhwc=nhwc), args.launches)
                nbytes = 2 * 4 * G * Cc * size[0] * size[1]                      # algorithmic: the window read once, written once
                print(json.dumps(dict(kernel="augment", group=name, G=G, C=Cc, window=list(size), layout="nhwc" if nhwc else "nchw",
                                      ms=round(ms, 5), GBps=round(nbytes / ms / 1e6, 1), share_of_peak=round(nbytes / (ms * 1e-3) / PEAK, 3))))
                if not nhwc:
                    total_ms += ms
            crop = A.apply(x, table, pidx=pidx)
            dst = torch.empty(G, size[0], size[1], (Cc + 3) // 4 * 4, device=dev)
            ms = timed(lambda: _hip.check(L.ramnet_nchw_to_nhwc_pad(ops._p(crop), ops._p(dst), G, Cc, size[0], size[1], dst.shape[3], ops._st()),
                                          "repack"), args.launches)
            nbytes = 2 * 4 * G * Cc * size[0] * size[1]
            print(json.dumps(dict(kernel="nchw_to_nhwc_pad", group=name, G=G, C=Cc, window=list(size), ms=round(ms, 5),
                                  GBps=round(nbytes / ms / 1e6, 1), share_of_peak=round(nbytes / (ms * 1e-3) / PEAK, 3))))
            del x, out, crop, dst
        print(json.dumps(dict(summary="device launches per step", window=list(size), ms=round(total_ms, 4))))
    # upload of the untransformed step from pinned memory (overlaps the previous step in AugmentedLoader)
    host = torch.empty(64 * 32, H, W).pin_memory()
    devbuf = torch.empty_like(host, device=dev)
    ms = timed(lambda: devbuf.copy_(host, non_blocking=True), 10, warm=2)
    print(json.dumps(dict(summary="upload of one untransformed step", MB=round(host.numel() * 4 / 1e6, 1), ms=round(ms, 3),
                          GBps=round(host.numel() * 4 / ms / 1e6, 1))))


_sample = None


def _init():
    global _sample
    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(os.getpid())
    _sample = [torch.randn(5, H, W, generator=g) for _ in range(5)] + [torch.rand(1, H, W, generator=g) for _ in range(7)]


def _job(seed):
    transform = D.Compose([D.RandomRotationFlip(0.0, 0.5, 0.0), D.RandomCrop(224)])
    out = []
    for t in _sample:
        random.seed(seed)
        out.append(transform(t))
    return len(out)


def host_side(workers=16):
    """The host Compose over the 768 tensors of one step (64 samples x 12 tensors), `workers` processes of one thread each."""
    import torch.multiprocessing as mp
    with mp.get_context("spawn").Pool(workers, initializer=_init) as pool:
        pool.map(_job, range(64))                          # warm-up
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            pool.map(_job, range(64))
            times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(summary="host Compose over one step's 768 tensors", workers=workers, ms_min=round(min(times), 1),
                          ms_all=[round(t, 1) for t in times])))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-device", action="store_true")
    a = ap.parse_args()
    if not a.no_device:
        device_side(a)
    if not a.no_host:
        host_side()
