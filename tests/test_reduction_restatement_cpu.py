"""CPU: anchors of tests/reduction_restatement.py, the float64 reference of tests/test_hip_reductions.py: against the oracle's losses
(oracle/loss_ref.py) and their autograd gradients, against the reference's own results in tests/golden/loss_metrics.npz and
loss_extra.npz, against torch's batch_norm / instance_norm (training and eval, running buffers included) and torch.matmul in float64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import loss_ref
from util import load_golden
import reduction_restatement as rr

F64 = torch.float64


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(F64)


def _close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert torch.equal(torch.isnan(a), torch.isnan(b))          # (a scale without a valid window: 0 / 0 on both sides)
    a, b = torch.nan_to_num(a), torch.nan_to_num(b)
    assert a.shape == b.shape and bool(((a - b).abs() <= tol * torch.maximum(a.abs(), b.abs()).clamp_min(1e-30)).all()), float((a - b).abs().max())


def _maps(B, H, W, nan, seed, positive=False):
    p, t = _rand(B, H, W, seed=seed), _rand(B, H, W, seed=seed + 1)
    if positive:
        p, t = p.abs() + 0.1, t.abs() + 0.1
    t[torch.rand(B, H, W, generator=torch.Generator().manual_seed(seed + 2)) < nan] = float("nan")
    return p, t


# ------------------------------------------------------------------------------------------------ SI, SI-log, mse
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("nan", [0.0, 0.2])
def test_si_against_oracle_and_autograd(nan, log):
    p, t = _maps(2, 9, 11, nan, 1, positive=log)
    st = rr.si_stats(p, t, log)
    d = (torch.log(p) - torch.log(t)) if log else p - t
    assert float(st[2]) == float((~torch.isnan(d)).sum())
    for w, lam in ((1.0, 1.0), (0.5, 0.85)):
        pp = p.clone().requires_grad_(True)
        ref = loss_ref.scale_invariant_log_loss(pp, t, lam) * w if log else loss_ref.scale_invariant_loss(pp, t, w, lam)
        ref.backward()
        # (the statement rounds d = p - t to fp32: 2^-24 relative per term)
        _close(rr.si_loss_from_stats(st, w, lam), ref.detach(), 1e-12 if log else 1e-5)
        g = rr.si_bwd(p, t, st, w, lam, 0.75, log)
        assert float((g - 0.75 * pp.grad).abs().max()) <= (1e-12 if log else 1e-6) * float(pp.grad.abs().max())
        assert bool((g[torch.isnan(d)] == 0).all())
        if not log:
            ref_g = loss_ref.si_loss_grad(p, t, w, lam)
            assert float((rr.si_bwd(p, t, st, w, lam) - ref_g).abs().max()) <= 1e-6 * float(ref_g.abs().max())
    assert torch.isnan(rr.si_loss_from_stats(torch.zeros(3, dtype=F64)))


def test_si_against_the_reference_fixtures():
    z = load_golden("loss_metrics.npz")
    for i in range(3):
        p, t = torch.from_numpy(z["si%d.pred" % i]).to(F64)[:, 0], torch.from_numpy(z["si%d.target" % i]).to(F64)[:, 0]
        st = rr.si_stats(p, t)
        _close(rr.si_loss_from_stats(st), float(z["si%d.loss" % i]), 2e-5)
        _close(rr.si_loss_from_stats(st, 0.5, 0.85), float(z["si%d.loss_w05_l085" % i]), 2e-5)
        g, ref = rr.si_bwd(p, t, st), torch.from_numpy(z["si%d.grad" % i]).to(F64)[:, 0]
        assert float((g - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
        _close(rr.mse_loss(rr.mse_stats(p, t, False)), float(z["si%d.mse" % i]), 2e-5)


def test_silog_and_mse_against_the_reference_fixtures():
    z = load_golden("loss_extra.npz")
    for c in ("c0", "c1", "c2"):
        p, t = torch.from_numpy(z[c + ".pred"]).to(F64)[:, 0], torch.from_numpy(z[c + ".target"]).to(F64)[:, 0]
        for key, lam in (("silog100", 1.0), ("silog85", 0.85)):
            st = rr.si_stats(p, t, log=True)
            _close(rr.si_loss_from_stats(st, 1.0, lam), float(z["%s.%s.loss" % (c, key)]), 2e-5)
            g, ref = rr.si_bwd(p, t, st, 1.0, lam, log=True), torch.from_numpy(z["%s.%s.grad" % (c, key)]).to(F64)[:, 0]
            assert float((g - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
        for key, half in (("mse100", False), ("mse50", True)):
            st = rr.mse_stats(p, t, half)
            _close(rr.mse_loss(st), float(z["%s.%s.loss" % (c, key)]), 2e-5)
            g, ref = rr.mse_bwd(p, t, half, st), torch.from_numpy(z["%s.%s.grad" % (c, key)]).to(F64)[:, 0]
            assert float((g - ref).abs().max()) <= 2e-5 * float(ref.abs().max())


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("B,H,W", [(1, 2, 2), (2, 5, 7), (1, 8, 9)])
def test_mse_against_oracle_and_autograd(B, H, W, half):
    p, t = _maps(B, H, W, 0.2, 5)
    st = rr.mse_stats(p, t, half)
    if st[1] == 0:
        t = torch.nan_to_num(t)
        st = rr.mse_stats(p, t, half)
    pp = p.clone().requires_grad_(True)
    ref = loss_ref.mse_loss_downsampled(pp[:, None], t[:, None], 0.5 if half else 1.0)
    ref.backward()
    _close(rr.mse_loss(st), ref.detach(), 1e-5)
    g = rr.mse_bwd(p, t, half, st, 2.0)
    assert float((g - 2.0 * pp.grad).abs().max()) <= 1e-5 * float(pp.grad.abs().max()) + 1e-300
    if half:          # the dropped odd row / column
        assert float(g[:, 2 * (H // 2):].abs().sum()) == 0.0 and float(g[:, :, 2 * (W // 2):].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ depth metrics
@pytest.mark.parametrize("cutoff", [float("inf"), 20.0])
def test_depth_metrics_against_oracle(cutoff):
    clip, reg = 80.0, 3.7
    rng = torch.Generator().manual_seed(7)
    tn, pn = torch.rand(600, generator=rng).float().to(F64), (torch.rand(600, generator=rng) * 1.2 - 0.1).float().to(F64)
    tn[::7] = float("nan")
    out = rr.depth_metrics(pn, tn, clip, reg, cutoff)
    t, p = loss_ref.prepare_depth_data(tn.numpy(), pn.numpy(), clip, reg)       # (float32 metric depths)
    with np.errstate(invalid="ignore"):
        mask = np.nan_to_num(t) < cutoff
    assert float(out[1]) == mask.sum() and float(out[0]) == (mask & ~np.isnan(t)).sum()
    tab = loss_ref.evaluation_table(t.astype(np.float64), p.astype(np.float64), mask)
    n, nm = float(out[0]), float(out[1])
    _close(out[2] / n, tab["abs_rel_diff"], 1e-5)
    _close(out[3] / n, tab["squ_rel_diff"], 1e-5)
    _close(torch.sqrt(out[4] / n), tab["RMS_linear"], 1e-5)
    _close(out[7] / n, tab["mean_depth_error"], 1e-5)
    _close(out[5] / n - (out[6] / n) ** 2, tab["SILog"], 1e-4)
    for k in range(3):      # the table's thresholds are means over the mask, NaN targets counting as misses
        assert abs(float(out[8 + k]) / nm - tab["threshold_delta_1.25" + ("", "^2", "^3")[k]]) <= 1.5 / nm


def test_depth_metrics_against_the_reference_fixture():
    z = load_golden("loss_metrics.npz")
    for key, clip, reg in (("depth80", 80.0, 3.70378), ("depth1000", 1000.0, 5.70378)):
        tn, pn = torch.from_numpy(z[key + ".target_in"]).to(F64), torch.from_numpy(z[key + ".pred_in"]).to(F64)
        t, p = rr.metric_depths(pn, tn, clip, reg)
        _close(t, torch.from_numpy(z[key + ".target"]).to(F64), 1e-5)
        _close(p, torch.from_numpy(z[key + ".pred"]).to(F64), 1e-5)
        out = rr.depth_metrics(pn, tn, clip, reg, float("inf"))
        assert float(out[0]) == float(out[1]) == tn.numel()
        _close(out[2] / out[0], float(z[key + ".abs_rel"]), 1e-4)


# ------------------------------------------------------------------------------------------------ multi-scale gradient loss
@pytest.mark.parametrize("ns", [1, 2, 3, 4])
@pytest.mark.parametrize("B,H,W,nan", [(1, 8, 8, 0.0), (2, 9, 11, 0.0), (1, 21, 27, 0.2), (1, 13, 8, 0.2)])
def test_msg_against_oracle(B, H, W, nan, ns):
    p, t = _maps(B, H, W, nan, 9)
    p, t = (p * 8).round(), (t * 8).round()          # integers: the statement's fp32 steps are exact
    st, loss, ws = rr.msg_forward(p, t, ns)
    assert ws.numel() == rr.msg_workspace_elems(B, H, W, ns)
    pp = p.clone().requires_grad_(True)
    ref = loss_ref.multi_scale_grad_loss(pp[:, None], t[:, None], 1, ns)
    _close(loss, ref.detach(), 1e-12)
    g, ag, nterm = rr.msg_backward(ws, st, B, H, W, ns, 0.5)
    assert bool((g.abs() <= ag * (1 + 1e-12)).all()) and 0 < nterm <= 8 * 9
    assert bool((g[torch.isnan(t)] == 0).all())
    if nan == 0.0:
        ref.backward()
        assert float((g - 0.5 * pp.grad).abs().max()) <= 1e-12 * float(pp.grad.abs().max())


def test_msg_empty_scale():
    assert rr.msg_scales(7, 8, 4) is None and rr.msg_workspace_elems(1, 7, 8, 4) == 0 and rr.msg_workspace_elems(1, 8, 8, 4) == 64 + 16 + 4 + 1


# ------------------------------------------------------------------------------------------------ nonzero normalisation
def test_normalize_nonzero_against_its_definition():
    g = _rand(5, 6, 7, seed=11)
    g[g.abs() < 0.5] = 0.0
    out = rr.normalize_nonzero(g)
    nz = g[g != 0]
    _close(out[g != 0], (nz - nz.mean()) / nz.std(unbiased=False), 1e-12)
    assert bool((out[g == 0] == 0).all())
    _close(rr.nonzero_stats(g), torch.stack([nz.sum(), (nz * nz).sum(), torch.tensor(float(nz.numel()), dtype=F64)]))
    one = torch.zeros(12, dtype=F64)
    one[[1, 5]] = 0.3
    assert torch.equal(rr.normalize_nonzero(one), one) and torch.equal(rr.normalize_nonzero(torch.zeros(4, dtype=F64)), torch.zeros(4, dtype=F64))


# ------------------------------------------------------------------------------------------------ norm
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("inst", [False, True])
@pytest.mark.parametrize("train", [True, False])
def test_norm_against_torch(train, inst, act):
    """[B][C][H][W] through torch's batch_norm / instance_norm + activation (+ residual) in float64, forward, running buffers and
    autograd gradients, against the five statements on the [groups][npix][C] layout"""
    B, Cc, H, W, eps, mom = 3, 5, 4, 6, 1e-5, 0.3
    x, res, dy = _rand(B, Cc, H, W, seed=12) * 2 + 0.5, _rand(B, Cc, H, W, seed=13), _rand(B, Cc, H, W, seed=14)
    gamma, beta = _rand(Cc, seed=15), _rand(Cc, seed=16)
    rm0, rv0 = _rand(Cc, seed=17), _rand(Cc, seed=18).abs() + 0.5
    groups, npix = (B, H * W) if inst else (1, B * H * W)
    lay = lambda t: t.permute(0, 2, 3, 1).reshape(groups, npix, Cc)
    xt, rt, gt, bt = (t.clone().requires_grad_(True) for t in (x, res, gamma, beta))
    rm, rv = rm0.clone(), rv0.clone()
    if inst:
        z = F.instance_norm(xt, rm, rv, gt, bt, use_input_stats=train, momentum=mom, eps=eps)
    else:
        z = F.batch_norm(xt, rm, rv, gt, bt, training=train, momentum=mom, eps=eps)
    z = z + rt
    y = z if act == 0 else F.relu(z) if act == 1 else torch.sigmoid(z)
    (y * dy).sum().backward()
    sums = rr.norm_partial(lay(x), lay(x))
    mean, rstd, scale, shift, nrm, nrv = rr.norm_finalize(sums, npix, eps, gamma, beta, rm0, rv0, mom, update=train, use_running=not train)
    out = rr.norm_apply(lay(x), scale, shift, lay(res), act)
    _close(out, lay(y.detach()), 1e-10)
    _close(nrm, rm, 1e-12)
    _close(nrv, rv, 1e-12)
    bs = rr.norm_partial(lay(dy), lay(x), lay(y.detach()), act)
    c1, c2, c3, dgamma, dbeta = rr.norm_finalize_bwd(bs, npix, mean, rstd, gamma, batch_stats=train)
    dx, dres = rr.norm_bwd(lay(dy), lay(x), c1, c2, c3, lay(y.detach()), act)
    tol = lambda ref: 1e-10 * float(ref.abs().max())
    assert float((dx - lay(xt.grad)).abs().max()) <= tol(xt.grad) and float((dres - lay(rt.grad)).abs().max()) <= tol(rt.grad)
    assert float((dgamma - gt.grad).abs().max()) <= tol(gt.grad) and float((dbeta - bt.grad).abs().max()) <= tol(bt.grad)


def test_norm_null_affine():
    sums = rr.norm_partial(_rand(2, 9, 3, seed=19), _rand(2, 9, 3, seed=19))
    mean, rstd, scale, shift, _, _ = rr.norm_finalize(sums, 9, 1e-5)
    _close(scale, rstd)
    _close(shift, -mean * rstd)


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("trans_a", [False, True])
def test_gemm_against_matmul(trans_a):
    A, Bm, C0 = _rand(3, 5, 8, seed=20), _rand(3, 8, 7, seed=21), _rand(3, 5, 7, seed=22)
    At = A.transpose(1, 2).contiguous() if trans_a else A
    _close(rr.gemm(At, Bm, None, trans_a), torch.matmul(A, Bm))
    _close(rr.gemm(At, Bm, C0, trans_a), C0 + torch.matmul(A, Bm))
