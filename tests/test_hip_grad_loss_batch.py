"""GPU: the batched multi-scale gradient loss (csrc/grad_loss.hip; ops.multi_scale_grad_loss_batch, msg_local_stats,
multi_scale_grad_loss_from_stats) against the float64 oracle through torch autograd — tolerances of the per-pair test (loss rtol 2e-5,
gradient 1e-4 in max norm) — on targets whose NaN regions are BLOCKS, so that every scale keeps valid components and the comparison is never
NaN against NaN; bit reproducibility, the global-batch form, equivalence with the per-pair path and the trainer wiring."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import loss_ref
from util import assert_close, build_hip_model, ref_cfg

pytestmark = pytest.mark.gpu

NS = 4


def dev():
    return torch.device("cuda:0")


def make_pairs(G, B, H, W, nan, seed=0):
    """G pairs of float32 [B, 1, H, W] maps; nan: a corner rectangle [:H//3, :W//3] per sample and, where H >= 64, a 9 x 11 block at the
    centre (not aligned to 8)."""
    rng = np.random.default_rng(seed + 1000 * G + H * W)
    ps = [rng.random((B, 1, H, W)).astype(np.float32) for _ in range(G)]
    ts = [rng.random((B, 1, H, W)).astype(np.float32) for _ in range(G)]
    if nan:
        for t in ts:
            t[:, :, :H // 3, :W // 3] = np.nan
            if H >= 64:
                t[:, :, H // 2 - 4:H // 2 + 5, W // 2 - 5:W // 2 + 6] = np.nan
    return ps, ts


def oracle_pair(p, t, up=1.0, batch=None):
    """float64 oracle of one pair: (loss, d (up * loss) / d p, valid components per scale).  batch: the oracle's B factor (global-batch form)."""
    pc = torch.from_numpy(p).double().requires_grad_(True)
    tc = torch.from_numpy(t).double()
    l = loss_ref.multi_scale_grad_loss(pc, tc)
    if batch is not None:
        l = l * (batch / p.shape[0])
    (up * l).backward()
    d = (pc - tc).detach()
    counts = [int((~torch.isnan(loss_ref.spatial_gradient(F.avg_pool2d(d, 2 ** s, 2 ** s)))).sum()) for s in range(NS)]
    return float(l.detach()), pc.grad.numpy(), counts


CASES = [(3, 2, 77, 141, True), (2, 1, 72, 136, True), (2, 3, 35, 53, True), (1, 2, 20, 28, False), (1, 1, 16, 16, False)]


@functools.lru_cache(maxsize=None)
def reference(G, B, H, W, nan):
    """Inputs, weights, upstream gradients and the oracle's results of a case: computed once, shared, never modified."""
    ps, ts = make_pairs(G, B, H, W, nan)
    w = [1.0, 0.5, 2.0][:G]
    up = [1.5, -0.75, 2.5][:G]
    ref = [oracle_pair(p, t, up=u * wi) for p, t, u, wi in zip(ps, ts, up, w)]
    for a in ps + ts:
        a.setflags(write=False)
    return ps, ts, w, up, ref


def to_dev(arrs, grad=False):
    return [torch.from_numpy(np.array(a)).to(dev()).requires_grad_(grad) for a in arrs]


@pytest.mark.parametrize("G,B,H,W,nan", CASES)
def test_batched_loss_and_gradient_vs_oracle(G, B, H, W, nan):
    from rpg_ramnet_amd import ops
    ps, ts, w, up, ref = reference(G, B, H, W, nan)
    for l, _, counts in ref:                       # the comparison below is never NaN against NaN
        assert all(c >= 1 for c in counts) and np.isfinite(l), (counts, l)
    if nan:
        assert any(np.isnan(t).any() for t in ts)
    pg, tg = to_dev(ps, True), to_dev(ts)
    loss = ops.multi_scale_grad_loss_batch(pg, tg, weights=w)
    assert loss.shape == (G,) and loss.dtype == torch.float32
    (loss * torch.tensor(up, device=dev())).sum().backward()
    got = loss.detach().cpu().numpy()
    for g in range(G):
        print("pair %d: loss %.8g oracle %.8g" % (g, got[g], w[g] * ref[g][0]))
        np.testing.assert_allclose(got[g], w[g] * ref[g][0], rtol=2e-5)
        assert_close(pg[g].grad.cpu().numpy(), ref[g][1], 1e-4, "batched msg grad, pair %d" % g)
        if nan:
            assert float(pg[g].grad[torch.isnan(tg[g])].abs().max()) == 0.0          # pixels under a NaN target get 0
    # the sum output and its gradient path
    pg2 = to_dev(ps, True)
    loss2, total = ops.multi_scale_grad_loss_batch(pg2, tg, weights=w, with_sum=True)
    (3.0 * total).backward()
    np.testing.assert_allclose(float(total), sum(w[g] * ref[g][0] for g in range(G)), rtol=2e-5)
    for g in range(G):
        assert_close(pg2[g].grad.cpu().numpy(), ref[g][1] * (3.0 / up[g]), 1e-4, "gradient through the sum, pair %d" % g)


def test_a_pair_with_an_empty_scale_is_nan_and_leaves_the_others_alone():
    from rpg_ramnet_amd import ops
    ps, ts = make_pairs(3, 2, 20, 28, False, seed=7)
    ts[1] = ts[1].copy()
    ts[1][:, 0, 5, 12] = np.nan                    # column cell 1 of the 2 x 3 scale-3 map: every clamped Sobel window holds it
    ref = [oracle_pair(p, t) for p, t in zip(ps, ts)]
    assert ref[1][2][3] == 0 and all(c > 0 for c in ref[1][2][:3]) and np.isnan(ref[1][0]) and np.isfinite(ref[1][1]).all()
    pg, tg = to_dev(ps, True), to_dev(ts)
    loss = ops.multi_scale_grad_loss_batch(pg, tg)
    # (sum of the finite entries and the NaN one separately: an upstream gradient of 1 for every pair)
    loss.backward(torch.ones(3, device=dev()))
    got = loss.detach().cpu().numpy()
    assert np.isnan(got[1])
    for g in range(3):
        if g != 1:
            np.testing.assert_allclose(got[g], ref[g][0], rtol=2e-5)
        grad = pg[g].grad.cpu().numpy()
        assert np.isfinite(grad).all()
        assert_close(grad, ref[g][1], 1e-4, "empty scale: grad of pair %d" % g)


def test_bit_reproducible_across_calls_and_other_shapes_in_between():
    from rpg_ramnet_amd import ops
    ps, ts = make_pairs(4, 2, 77, 141, True, seed=3)
    other_p, other_t = make_pairs(2, 3, 35, 53, True, seed=4)
    tg, og_t = to_dev(ts), to_dev(other_t)
    up = torch.tensor([1.0, -2.0, 0.5, 3.0], device=dev())
    runs = []
    for rep in range(5):
        pg = to_dev(ps, True)
        stats = ops.msg_local_stats(pg, tg)
        loss = ops.multi_scale_grad_loss_batch(pg, tg, weights=[1.0, 0.5, 2.0, 1.0])
        (loss * up).sum().backward()
        runs.append((stats.clone(), loss.detach().clone(), [p.grad.clone() for p in pg]))
        if rep % 2 == 0:                           # another (G, shape) in between: workspace and table reuse
            og = to_dev(other_p, True)
            ops.multi_scale_grad_loss_batch(og, og_t).sum().backward()
    for st, l, gr in runs[1:]:
        assert torch.equal(st, runs[0][0]) and torch.equal(l, runs[0][1])
        assert all(torch.equal(a, b) for a, b in zip(gr, runs[0][2]))
    assert bool((runs[0][0][:, :, 1] > 0).all())


def test_global_batch_form_from_summed_shard_statistics():
    from rpg_ramnet_amd import ops
    ps, ts = make_pairs(1, 4, 35, 53, True, seed=9)
    ts[0] = ts[0].copy()
    ts[0][0, :, :20, :30] = np.nan                 # the shards have different valid counts
    p, t = ps[0], ts[0]
    l_ref, g_ref, counts = oracle_pair(p, t, up=1.0)
    assert all(c >= 1 for c in counts) and np.isfinite(l_ref)
    full = to_dev([p], True)
    l_full = ops.multi_scale_grad_loss_batch(full, to_dev([t]))
    l_full.sum().backward()
    halves = [(to_dev([p[:2]], True), to_dev([t[:2]])), (to_dev([p[2:]], True), to_dev([t[2:]]))]
    stats = sum(ops.msg_local_stats(a, b) for a, b in halves)
    assert torch.equal(stats[:, :, 1], ops.msg_local_stats(full, to_dev([t]))[:, :, 1])          # counts are integers: exact
    grads = []
    for i, (a, b) in enumerate(halves):
        batch = 4 if i == 0 else torch.tensor([4.0], device=dev(), dtype=torch.float64)       # host number / device scalar
        l = ops.multi_scale_grad_loss_from_stats(a, b, stats, batch, gain=1.0)
        np.testing.assert_allclose(float(l[0]), l_ref, rtol=2e-5)
        np.testing.assert_allclose(float(l[0]), float(l_full[0]), rtol=2e-5)
        l.sum().backward()
        grads.append(a[0].grad)
    cat = torch.cat(grads).cpu().numpy()
    assert_close(cat, g_ref, 1e-4, "from-stats gradient vs oracle")
    assert_close(cat, full[0].grad.cpu().numpy(), 1e-4, "from-stats gradient vs the full batch")
    # gain scales the backward alone
    a2 = to_dev([p[:2]], True)
    l2 = ops.multi_scale_grad_loss_from_stats(a2, halves[0][1], stats, 4, gain=2.0)
    l2.sum().backward()
    np.testing.assert_allclose(float(l2[0]), l_ref, rtol=2e-5)
    assert_close(a2[0].grad.cpu().numpy(), 2.0 * g_ref[:2], 1e-4, "gain")


@pytest.mark.parametrize("G,B,H,W", [(3, 2, 77, 141), (2, 3, 35, 53)])
def test_equals_the_per_pair_path(G, B, H, W):
    from rpg_ramnet_amd import ops
    ps, ts = make_pairs(G, B, H, W, False, seed=5)
    tg = to_dev(ts)
    pb, pp = to_dev(ps, True), to_dev(ps, True)
    loss = ops.multi_scale_grad_loss_batch(pb, tg)
    loss.sum().backward()
    for g in range(G):
        l = ops.multi_scale_grad_loss(pp[g], tg[g])
        l.backward()
        np.testing.assert_allclose(float(loss[g]), float(l), rtol=2e-5)
        assert_close(pb[g].grad.cpu().numpy(), pp[g].grad.cpu().numpy(), 1e-4, "batched vs per-pair grad %d" % g)


def test_rejects_bad_arguments_on_the_device():
    from rpg_ramnet_amd import ops, _hip
    a = torch.zeros(1, 1, 4, 16, device=dev())
    with pytest.raises(RuntimeError, match="bad argument"):          # H >> 3 == 0: no scale-3 map (as the per-pair entry refuses it)
        ops.multi_scale_grad_loss_batch([a], [a])
    with pytest.raises(ValueError, match="weights"):
        ops.multi_scale_grad_loss_batch([a], [a], weights=[1.0, 2.0])
    L = _hip.lib()
    assert L.ramnet_grad_loss_workspace(0, 1, 16, 16) == 0 and L.ramnet_grad_loss_workspace(2, 3, 65, 64) == 2 * 3 * 2 * 8 * 8


# ------------------------------------------------------------------------------------------------------------------ trainer wiring
def _model_and_sequence(L):
    from recipe import make_item
    K = 3
    lc = ["image", "events2"]
    cfg, _ = ref_cfg("net_seeded_ramnet.npz", every_x_rgb_frame=K, loss_composition=lc)
    model = build_hip_model("ERGB2DepthRecurrent", cfg).train()
    rng = np.random.default_rng(5)
    seq = [{k: v.to(model.gpu) for k, v in make_item(rng, 2, 32, 48, K, 5, 1, True, 0.0).items()} for _ in range(L)]
    return model, seq, lc


def _run(model, seq, lc, calls, **kw):
    from rpg_ramnet_amd.trainer import sequence_loss
    calls.clear()
    model.zero_grad()
    total, rep = sequence_loss(model, seq, lc, [1.0, 0.5], grad_loss_weight=0.25, **kw)
    total.backward()
    torch.cuda.synchronize()
    return float(total.detach()), float(rep), {k: p.grad.clone() for k, p in model.named_parameters()}, list(calls)


def _same(a, b, what):
    np.testing.assert_allclose(a[0], b[0], rtol=1e-6)
    np.testing.assert_allclose(a[1], b[1], rtol=1e-6)
    gmax = max(float(g.abs().max()) for g in b[2].values())
    for k, g in b[2].items():
        assert_close(a[2][k].cpu().numpy(), g.cpu().numpy(), 1e-5, "%s: grad %s" % (what, k), floor=gmax)


def test_sequence_loss_uses_one_batched_call_and_agrees_with_the_per_pair_path():
    from rpg_ramnet_amd import ops, _hip as Hh
    from rpg_ramnet_amd import graph
    calls = []
    Hh.set_tracer(lambda name, fn, args: (calls.append(name), fn(*args))[1])
    try:
        counts = {}
        for L in (1, 2):
            model, seq, lc = _model_and_sequence(L)
            on = _run(model, seq, lc, calls)
            assert not any(c.startswith("ramnet_msg_loss") for c in on[3])
            counts[L] = [sum(c == n for c in on[3]) for n in ("ramnet_grad_loss_stats", "ramnet_grad_loss_bwd")]
        assert counts[1] == counts[2] == [1, 1]                       # independent of L (and of the number of supervised maps)
        with ops.switches(grad_loss_batched=False):
            off = _run(model, seq, lc, calls)
        assert sum(c == "ramnet_msg_loss_fwd" for c in off[3]) == 2 * len(lc) and "ramnet_grad_loss_stats" not in off[3]
        _same(on, off, "batched vs per-pair")
        dp = _run(model, seq, lc, calls, dp_exact=True)                # a single process: world 1
        assert sum(c == "ramnet_grad_loss_stats" for c in dp[3]) == 1 and sum(c == "ramnet_grad_loss_from_stats" for c in dp[3]) == 1
        assert not any(c.startswith("ramnet_msg_loss") for c in dp[3])
        _same(dp, on, "dp_exact vs plain")
    finally:
        Hh.set_tracer(None)
    step = graph.GraphedTrainStep(model, seq, lc, [1.0, 0.5], grad_loss_weight=0.25)
    total, _ = step()
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(total), on[0], rtol=1e-6)
