"""GPU: the deterministic mode at model level (rpg_ramnet_amd.ops.set_deterministic) under the bench schedule — backward-weights on the side
stream, decoders on their own stream, deferred multi-segment cell launches: repeated backward passes, optimizer trajectories and graph
replays give the same bits, `pred.conv2d.bias` included (the sum that tests/test_hip_model.py has to skip in its repeat comparisons); the
gradients stay within that file's bound between two summation orders of the default mode's; the input pipeline from raw events gives the
same tensors; operations without an ordered form raise RuntimeError in the mode and work outside it.

Seeded models of 32 base channels and 3 encoders (the decoders run the Winograd-domain backward-weights kernels, the heads the head
kernel), B = 2, L = 2 packages of K = 2 event grids, 5 bins, 32 x 48, SI loss on ["image", "events1"] plus the batched gradient loss, 20 %
NaN targets.  The NaN pixels are drawn outside a 24 x 24 corner of every target map (and more densely there, 20 % of the map in all): with
NaN spread over the whole map no 8 x 8 cell of the coarsest scale of the gradient loss is valid at this size and the loss VALUE is NaN in
either mode (the gradients stay finite), which would leave nothing to compare.  Every test sets the mode inside try / finally and restores
it, and the schedule switches to what they were."""
import numpy as np
import pytest
import torch

from history_cases import B, H, K, L, LC, W, WIRINGS, _backward, _cfg, _same, _seq, _targets_with_nan, bench_schedule  # noqa: F401
from util import assert_close, build_hip_model

# (the models, data and helpers of this file are shared with tests/test_hip_history.py: they live in tests/history_cases.py)
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wiring", sorted(WIRINGS))
def test_three_backward_passes_give_the_same_bits(wiring):
    arch, over, irregular = WIRINGS[wiring]
    lc = ["image_last", "events_last"] if irregular else LC
    cfg = _cfg(loss_composition=lc, **over)
    model = build_hip_model(arch, cfg).train()
    seq = _seq(model, 11, irregular)
    unet = arch == "ERGB2Depth"
    with bench_schedule(True):
        runs = [_backward(model, seq, lc, unet) for _ in range(3)]
    with bench_schedule(False):
        ref_loss, ref = _backward(model, seq, lc, unet)
    assert set(runs[0][1]) == set(ref) and any(k.endswith("pred.conv2d.bias") for k in ref)
    for loss, g in runs[1:]:
        assert _same(loss, runs[0][0]), "the loss differs between two passes"
        for k in g:
            assert _same(g[k], runs[0][1][k]), "%s differs between two passes" % k
    # against the default mode: the same partial sums joined in another order — the run-to-run bound of test_wgrad_side_stream_gradients
    # (tests/test_hip_model.py: 1e-5 above a floor of 1 % of the largest gradient)
    assert np.isfinite(float(ref_loss)) and np.isfinite(float(runs[0][0]))
    np.testing.assert_allclose(float(runs[0][0]), float(ref_loss), rtol=1e-5)
    gmax = max(float(v.abs().max()) for v in ref.values())
    for k in ref:
        if not k.endswith("pred.conv2d.bias"):      # (a sum of ~1e4 terms that cancels: its own summation-order noise in the default mode)
            assert_close(runs[0][1][k].cpu().numpy(), ref[k].cpu().numpy(), 1e-5, "deterministic vs default " + k, floor=1e-2 * gmax)


def _trajectory(det, steps=4):
    model = build_hip_model("ERGB2DepthRecurrent", _cfg(), seed=3).train()
    seq = _seq(model, 12)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    from rpg_ramnet_amd.trainer import sequence_loss
    with bench_schedule(det):
        for _ in range(steps):
            opt.zero_grad()
            total, _ = sequence_loss(model, seq, LC, [1, 1], grad_loss_weight=0.25)
            total.backward()
            opt.step()
        torch.cuda.synchronize()
    return {k: p.detach().clone() for k, p in model.named_parameters()}


def test_four_adam_steps_twice_give_the_same_weights():
    """the trajectory statement: over several steps Adam turns last-bit differences of a gradient into O(lr) moves of parameters, so equal
    weights after four steps need equal gradients in every step"""
    a, b = _trajectory(True), _trajectory(True)
    for k in a:
        assert _same(a[k], b[k]), k
    assert any(not torch.equal(a[k], p.detach()) for k, p in build_hip_model("ERGB2DepthRecurrent", _cfg(), seed=3).named_parameters())


def test_graph_replays_give_the_same_bits_and_the_mode_is_guarded():
    from rpg_ramnet_amd import ops
    from rpg_ramnet_amd.graph import GraphedTrainStep
    model = build_hip_model("ERGB2DepthRecurrent", _cfg()).train()
    seq = _seq(model, 13)
    with bench_schedule(True):
        g = GraphedTrainStep(model, seq, LC, [1, 1], grad_loss_weight=0.25)
        outs = []
        for _ in range(3):
            total, _ = g()
            torch.cuda.synchronize()
            outs.append((total.clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
        for total, grads in outs[1:]:
            assert _same(total, outs[0][0])
            for k in grads:
                assert _same(grads[k], outs[0][1][k]), k
        ops.set_deterministic(False)
        with pytest.raises(RuntimeError, match="set_deterministic"):
            g()
        ops.set_deterministic(True)
        g()
        torch.cuda.synchronize()


def test_input_pipeline_from_raw_events_gives_the_same_tensors():
    """raw events -> sorted voxeliser -> ordered normalisation statistics -> augment (one launch that normalises and transforms): three runs,
    the same bits; and the stand-alone normalisation of the same grids"""
    from rpg_ramnet_amd import augment, ops, voxel
    from rpg_ramnet_amd import data as D
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(14)
    bins, Hs, Ws, G = 5, 36, 52, 4
    lists = []
    for g in range(G):
        n = 0 if g == 2 else 3000 + 500 * g
        t = np.sort(rng.uniform(0.0, 1.0, n))
        lists.append(np.stack([t, rng.integers(0, Ws, n).astype(np.float64), rng.integers(0, Hs, n).astype(np.float64), rng.choice([-1.0, 1.0], n)], 1).reshape(n, 4))
    cat, off, mx = voxel.pack_event_lists(lists, dev)
    params = augment.ParamTable([augment.draw(D.Compose([D.RandomRotationFlip(20.0, 0.5, 0.5), D.RandomCrop((H, W))]), s, Hs, Ws)
                                 for s in range(G)], Hs, Ws).to(dev)
    with ops.switches(deterministic=True):
        runs = []
        for _ in range(3):
            out = augment.voxelize_augmented(cat, off, mx, bins, Ws, Hs, params)
            grids = voxel.events_to_voxel_grids(lists, bins, Ws, Hs, device=dev, normalize=True)
            one = voxel.normalize_nonzero(voxel.events_to_voxel_grid(lists[1], bins, Ws, Hs, device=dev))
            torch.cuda.synchronize()
            runs.append([t.clone() for t in (out if isinstance(out, (list, tuple)) else [out])] + [grids.clone(), one.clone()])
        for r in runs[1:]:
            for a, b in zip(r, runs[0]):
                assert torch.equal(a, b)
        assert torch.equal(runs[0][-1], runs[0][-2][1]), "one list through the sorted form == its grid in the batch"
        assert float(runs[0][-2][2].abs().max()) == 0.0 and float(runs[0][-2][0].abs().max()) > 0.0
    ref = voxel.events_to_voxel_grids(lists, bins, Ws, Hs, device=dev, normalize=True)           # the default mode: the same grids up to the fp64 sums' last bits
    assert_close(runs[0][-2].cpu().numpy(), ref.cpu().numpy(), 1e-6, "deterministic vs default grids")


def test_operations_without_an_ordered_form_raise_in_the_mode_and_work_outside_it():
    from rpg_ramnet_amd import metrics, ops, voxel
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(15)
    pred = torch.rand(2, 1, 16, 24, generator=g).to(dev)
    target = torch.rand(2, 1, 16, 24, generator=g).to(dev)
    ev = np.stack([np.linspace(0, 1, 50), np.arange(50) % 24, np.arange(50) % 16, np.ones(50)], 1)
    L_ = ops.H.lib()

    def unsorted():
        old = L_.ramnet_get_option(b"voxel_sorted")
        try:
            L_.ramnet_set_option(b"voxel_sorted", 0)
            return voxel.events_to_voxel_grids([ev, ev], 5, 24, 16, device=dev)
        finally:
            L_.ramnet_set_option(b"voxel_sorted", old)

    refused = {"mse_loss": lambda: ops.mse_loss(pred, target), "multi_scale_grad_loss": lambda: ops.multi_scale_grad_loss(pred, target),
               "depth_metrics": lambda: metrics.depth_metrics(pred, target, 80.0, 3.70378), "unsorted voxeliser": unsorted,
               "set_wgrad_slabs": lambda: ops.set_wgrad_slabs(False), "set_grad_loss_batched": lambda: ops.set_grad_loss_batched(False)}
    with ops.switches(wgrad_slabs=True, grad_loss_batched=True, deterministic=False):          # (the body's own changes are put back as well)
        for name, fn in refused.items():
            ops.set_deterministic(False)
            fn()                                    # works as before outside the mode
            ops.set_wgrad_slabs(True)
            ops.set_grad_loss_batched(True)
            ops.set_deterministic(True)
            with pytest.raises(RuntimeError, match="deterministic"):
                fn()
        # ordered in the mode, not refused: the stand-alone SI losses (their one-launch join has a fixed order outside a capture)
        # — on a map large enough for all 64 workgroups of its reduction, three calls, the same bits, and the float64 value
        big_p, big_t = torch.rand(4, 1, 256, 344, generator=g).to(dev), torch.rand(4, 1, 256, 344, generator=g).to(dev)
        a = [ops.scale_invariant_loss(big_p, big_t).detach().clone() for _ in range(3)]
        assert _same(a[1], a[0]) and _same(a[2], a[0])
        d64 = (big_p - big_t).double()
        np.testing.assert_allclose(float(a[0]), float((d64 ** 2).mean() - d64.mean() ** 2), rtol=1e-5)      # (weight 1, lambda 1: the defaults)
        # the contradicting settings refuse the switch itself
        ops.set_deterministic(False)
        for setter in (ops.set_wgrad_slabs, ops.set_grad_loss_batched):
            setter(False)
            with pytest.raises(RuntimeError):
                ops.set_deterministic(True)
            setter(True)
    torch.cuda.synchronize()


def test_the_fused_prediction_layer_refuses_its_atomic_fall_back_and_the_si_losses_refuse_a_capture():
    """PredSigmoidSI.backward joins through the forward's scratch; a change of the library option `pred_si_bwd_cap` in between leaves it the
    atomic form alone: refused in the mode, taken outside it.  scale_invariant_loss inside a stream capture has no library scratch for its
    fixed-order join: refused in the mode (by the operator, and by the library under its option `ordered_only`), taken outside it."""
    from rpg_ramnet_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(16)
    L_ = ops.H.lib()
    target = torch.rand(2, 1, 16, 24, generator=g).to(dev)

    def fused(change):
        x = torch.randn(2, 16, 24, 32, generator=g).to(dev).requires_grad_(True)
        w, b = torch.randn(1, 32, 1, 1, generator=g).to(dev).requires_grad_(True), torch.zeros(1, device=dev, requires_grad=True)
        old = L_.ramnet_get_option(b"pred_si_bwd_cap")
        try:
            _, loss = ops.PredSigmoidSI.apply(x, w, b, 1.0, 0.5, False, target)
            if change:
                L_.ramnet_set_option(b"pred_si_bwd_cap", old // 2)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            L_.ramnet_set_option(b"pred_si_bwd_cap", old)
        return w.grad

    pred = torch.rand(2, 1, 16, 24, generator=g).to(dev)
    with ops.switches(deterministic=False):
        assert bool(torch.isfinite(fused(True)).all())          # the atomic fall-back works outside the mode
        ops.set_deterministic(True)
        assert L_.ramnet_get_option(b"ordered_only") == 1
        assert bool(torch.isfinite(fused(False)).all())         # the join through the scratch: ordered, runs in the mode
        with pytest.raises(RuntimeError, match="deterministic"):
            fused(True)
        float(ops.scale_invariant_loss(pred, target))           # eager: the one-launch form, ordered
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with pytest.raises(RuntimeError, match="deterministic"):
            with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
                ops.scale_invariant_loss(pred, target)
        torch.cuda.synchronize()
        ops.set_deterministic(False)
        assert L_.ramnet_get_option(b"ordered_only") == 0
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = ops.scale_invariant_loss(pred, target)
        graph.replay()
        torch.cuda.synchronize()
        assert np.isfinite(float(out))
