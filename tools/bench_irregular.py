#!/usr/bin/env python3
"""Batches of irregular packages (per-sample update masks) against the reference branch's strategy and the regular step.

Workload: B = 8, 256 x 344, sequences of L = 8 packages, Kmax = 8, seeded counts uniform in {1..8}; ConvGRU state, 5-bin grids, SI loss
on [image_last, events_last], Adam.  Reports ms per step and samples/s (B * L per step) for
  (a) the batched irregular training step (ERGB2DepthRecurrent.forward with num_events),
  (b) the same packages as a per-sample loop: B batch-1 sequences (what the reference's asynchronous_irregular_real_data branch does),
  (c) the regular training step at K = 8 (every sample 8 grids),
  (d) the no-grad forward of (a) and of (b).
Usage (GPU box): python tools/bench_irregular.py [--steps N] [--warmup W] [--only a,b,c,d] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rpg_ramnet_amd.model.model import ERGB2DepthRecurrent  # noqa: E402
from rpg_ramnet_amd.trainer import sequence_loss  # noqa: E402

B, H, W, L, KMAX, CE = 8, 256, 344, 8, 8, 5


def cfg(K, lc):
    return dict(num_bins_rgb=1, num_bins_events=CE, skip_type="sum", recurrent_block_type="conv", state_combination="convgru",
                num_encoders=3, base_num_channels=32, num_residual_blocks=2, use_upsample_conv=True, norm="none", gpu=0,
                every_x_rgb_frame=K, baseline=False, loss_composition=lc)


def make_seq(rng, dev, counts, regular):
    seq = []
    for cnt in counts:
        it = {"events%d" % k: torch.from_numpy(rng.standard_normal((B, CE, H, W)).astype(np.float32)).to(dev) for k in range(KMAX)}
        it["image"] = torch.from_numpy(rng.random((B, 1, H, W)).astype(np.float32)).to(dev)
        d = lambda: torch.from_numpy(rng.uniform(0.05, 1.0, (B, 1, H, W)).astype(np.float32)).to(dev)      # noqa: E731
        if regular:
            it["depth_image"], it["depth_events%d" % (KMAX - 1)] = d(), d()
        else:
            it["num_events"] = torch.tensor(cnt, dtype=torch.int64)
            it["depth_image_last"], it["depth_events_last"] = d(), d()
        seq.append(it)
    return seq


def per_sample(seq, b):
    out = []
    for it in seq:
        n = int(it["num_events"][b])
        one = {"events%d" % k: it["events%d" % k][b:b + 1] for k in range(max(n, 1))}
        one.update(num_events=torch.tensor([n]), image=it["image"][b:b + 1], depth_image_last=it["depth_image_last"][b:b + 1],
                   depth_events_last=it["depth_events_last"][b:b + 1])
        out.append(one)
    return out


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="a,b,c,d")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    which = set(a.only.split(","))
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    counts = [[int(c) for c in rng.integers(1, KMAX + 1, B)] for _ in range(L)]
    torch.manual_seed(0)
    lc = ["image_last", "events_last"]
    model = ERGB2DepthRecurrent(cfg(KMAX, lc)).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-5)
    seq = make_seq(rng, dev, counts, False)
    res = {"workload": "B=%d, %dx%d, L=%d, Kmax=%d, counts uniform in {1..%d} (seed 0), ConvGRU, SI loss on %s, Adam" % (B, H, W, L, KMAX, KMAX, lc),
           "counts": counts, "samples_per_step": B * L}

    def step_a():
        opt.zero_grad(set_to_none=True)
        total, _ = sequence_loss(model, seq, lc, [1, 1])
        total.backward()
        opt.step()

    def step_b():
        opt.zero_grad(set_to_none=True)
        for b in range(B):
            total, _ = sequence_loss(model, per_sample(seq, b), lc, [1, 1])
            (total / B).backward()
        opt.step()

    def fwd(items_list):
        with torch.no_grad():
            for items in items_list:
                prev = None
                for it in items:
                    _, s, _ = model(it, prev, None)
                    prev = s["image"]

    if "a" in which:
        res["a_batched_irregular_train"] = timed(step_a, a.steps, a.warmup)
    if "b" in which:
        res["b_per_sample_loop_train"] = timed(step_b, a.steps, a.warmup)
    if "d" in which:
        res["d_batched_irregular_forward"] = timed(lambda: fwd([seq]), a.steps, a.warmup)
        res["d_per_sample_loop_forward"] = timed(lambda: fwd([per_sample(seq, b) for b in range(B)]), a.steps, a.warmup)
    if "c" in which:
        lcr = ["image", "events%d" % (KMAX - 1)]
        reg = ERGB2DepthRecurrent(cfg(KMAX, lcr)).to(dev).train()
        reg.load_state_dict(model.state_dict())
        ropt = torch.optim.Adam(reg.parameters(), lr=1e-5)
        rseq = make_seq(rng, dev, counts, True)

        def step_c():
            ropt.zero_grad(set_to_none=True)
            total, _ = sequence_loss(reg, rseq, lcr, [1, 1])
            total.backward()
            ropt.step()
        res["c_regular_train_K8"] = timed(step_c, a.steps, a.warmup)
    for k in list(res):
        if k[:2] in ("a_", "b_", "c_", "d_"):
            res[k + "_samples_per_s"] = B * L / (res[k] / 1e3)
    if "a_batched_irregular_train" in res and "b_per_sample_loop_train" in res:
        res["a_speedup_over_b"] = res["b_per_sample_loop_train"] / res["a_batched_irregular_train"]
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
