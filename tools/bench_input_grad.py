"""Timings behind profiles/input_grad_notes.md: the head layer's backward-data kernel alone, next to the direct kernel's launch on the same
operands, and what asking for input gradients costs a step of the bench workload.  One JSON line per measurement; needs the GPU.

    python tools/bench_input_grad.py [--launches 50] [--rounds 5] [--steps 3] [--no-step]

Kernel part: ramnet_head_dgrad (what ConvAct.backward launches where the forward ran the head kernel) and the direct kernel's `dgrad1` launch
(what it launches with set_head_kernel(False)) on one set of operands, alternating, `rounds` times `launches` launches each; the spread of
the rounds is printed with the mean.  Shapes: 40 x 256 x 344 with 5 channels (the event head of a B=8, K=5 package) and 8 x 256 x 344 with
1 channel (its frame head), 32 feature maps, ReLU mask operand.  bytes = dy + mask + dx once each; flop_mfma = what the matrix units
execute (ramnet_head_dgrad: 16 x 32 pixel tiles x 800 reduction steps x 16 channel columns x 2).
Step part: B=8, L=8, K=5 at 256 x 344 (bench.py's workload on resident random tensors; forward, SI loss on [image, events4], BPTT backward,
no optimizer): the plain step, the step with requires_grad on every event grid and frame, and inference.input_gradients on the same
sequence, alternating; milliseconds, peak memory of each and the three losses."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rpg_ramnet_amd import _hip as Hh  # noqa: E402
from rpg_ramnet_amd import inference, ops  # noqa: E402

HBM_PEAK, MFMA_PEAK = 8.0e12, 157.3e12          # bytes / s, fp32 matrix FLOP / s (MI355X)


def timed(fn, n, warm=3):
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


def kernels(args):
    dev = torch.device("cuda:0")
    L = Hh.lib()
    for B, H, W, cin in ((40, 256, 344, 5), (8, 256, 344, 1)):
        g = torch.Generator(device="cpu").manual_seed(1)
        w = (torch.randn(32, cin, 5, 5, generator=g) * 0.1).to(dev)
        cp = ops.ConvParam([w], [torch.zeros(32, device=dev)])
        dy, y = torch.randn(B, H, W, 32, device=dev), torch.randn(B, H, W, 32, device=dev)
        ld = (cin + 3) // 4 * 4
        dx_head, dx_direct = torch.empty(B, H, W, ld, device=dev), torch.empty(B, H, W, ld, device=dev)

        def head():
            Hh.check(L.ramnet_head_dgrad(ops._p(dy), 32, ops._p(y), 32, ops._p(w), ops._p(dx_head), ld, B, H, W, cin, 32, ops._st()), "ramnet_head_dgrad")

        def direct():
            ops.conv_launch(dy, ops.Taps.get("dgrad1", 5, 2), cp.bwd(), dx_direct, ld, xm=y, in_mode=Hh.IN_RELUMASK)
        head()
        name_head = L.ramnet_last_kernel().decode()
        direct()
        name_direct = L.ramnet_last_kernel().decode()
        torch.cuda.synchronize()
        diff = float((dx_head - dx_direct).abs().max()) / max(float(dx_direct.abs().max()), 1e-30)
        ms = {"head": [], "direct": []}
        for _ in range(args.rounds):
            ms["head"].append(timed(head, args.launches))
            ms["direct"].append(timed(direct, args.launches))
        nbytes = 4.0 * B * H * W * (32 + 32 + ld)
        tiles = -(-W // 32) * -(-H // 16) * B
        flop = {"head": tiles * 512 * 800 * 16 * 2.0, "direct": None}
        for k, name in (("head", name_head), ("direct", name_direct)):
            m = statistics.mean(ms[k])
            rec = dict(kernel=name, launch=k, B=B, H=H, W=W, Cin=cin, Cout=32, ms_mean=round(m, 4), ms_min=round(min(ms[k]), 4), ms_max=round(max(ms[k]), 4),
                       rounds=args.rounds, launches=args.launches, bytes=nbytes, GBps=round(nbytes / m / 1e6, 1), share_of_hbm_peak=round(nbytes / (m * 1e-3) / HBM_PEAK, 3))
            if flop[k]:
                rec.update(flop_mfma=flop[k], TFLOPs=round(flop[k] / m / 1e9, 1), share_of_mfma_peak=round(flop[k] / (m * 1e-3) / MFMA_PEAK, 3),
                           flop_useful=2.0 * B * H * W * 800 * cin)
            print(json.dumps(rec), flush=True)
        print(json.dumps(dict(compare="head vs direct", B=B, Cin=cin, max_rel_difference=diff, head_over_direct=round(statistics.mean(ms["head"]) / statistics.mean(ms["direct"]), 3))),
              flush=True)


def step(args):
    from rpg_ramnet_amd.model.model import ERGB2DepthRecurrent
    from rpg_ramnet_amd.trainer import sequence_loss
    K, B, Ls, H, W = 5, 8, 8, 256, 344
    lc = ["image", "events4"]
    cfg = dict(num_bins_rgb=1, num_bins_events=5, skip_type="sum", recurrent_block_type="conv", state_combination="convgru", num_encoders=3,
               base_num_channels=32, num_residual_blocks=2, use_upsample_conv=True, norm="none", gpu=0, every_x_rgb_frame=K, baseline=False,
               loss_composition=lc)
    torch.manual_seed(0)
    model = ERGB2DepthRecurrent(cfg)
    model = model.to(model.gpu).train()
    g = torch.Generator(device="cpu").manual_seed(2)
    seq = []
    for _ in range(Ls):
        it = {"events%d" % k: torch.randn(B, 5, H, W, generator=g).to(model.gpu) for k in range(K)}
        it["image"] = torch.rand(B, 1, H, W, generator=g).to(model.gpu)
        for key in lc:
            it["depth_" + key] = torch.rand(B, 1, H, W, generator=g).to(model.gpu)
        seq.append(it)
    inputs = lambda it: [k for k in it if not k.startswith("depth_")]       # noqa: E731
    losses = {}

    def plain():
        model.zero_grad()
        total, _ = sequence_loss(model, seq, lc, [1, 1])
        total.backward()
        losses["plain"] = total.detach()

    def asking():
        model.zero_grad()
        s = [dict(it, **{k: it[k].detach().requires_grad_(True) for k in inputs(it)}) for it in seq]
        total, _ = sequence_loss(model, s, lc, [1, 1])
        total.backward()
        losses["requires_grad"] = total.detach()
        assert all(it[k].grad is not None for it in s for k in inputs(it))

    def frozen():
        total, _ = inference.input_gradients(model, seq, lc)
        losses["input_gradients"] = total

    variants = (("plain", plain), ("requires_grad", asking), ("input_gradients", frozen))
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    ms, mem = {k: [] for k, _ in variants}, {}
    for _ in range(args.steps):
        for k, fn in variants:
            torch.cuda.reset_peak_memory_stats()
            ms[k].append(timed(fn, 1, warm=0))
            mem[k] = torch.cuda.max_memory_allocated()
    for k, _ in variants:
        print(json.dumps(dict(step=k, B=B, L=Ls, K=K, H=H, W=W, ms_mean=round(statistics.mean(ms[k]), 2), ms_all=[round(v, 2) for v in ms[k]],
                              peak_memory_GB=round(mem[k] / 2 ** 30, 3), loss=float(losses[k]))), flush=True)
    print(json.dumps(dict(compare="step", added_ms=round(statistics.mean(ms["requires_grad"]) - statistics.mean(ms["plain"]), 2),
                          added_memory_GB=round((mem["requires_grad"] - mem["plain"]) / 2 ** 30, 3),
                          same_loss=bool(losses["plain"] == losses["requires_grad"]),
                          input_gradients_over_requires_grad=round(statistics.mean(ms["input_gradients"]) / statistics.mean(ms["requires_grad"]), 3))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_input_grad.py measures on the GPU"
    if not a.no_kernels:
        kernels(a)
    if not a.no_step:
        step(a)
