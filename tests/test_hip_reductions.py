"""GPU: the reduction entry points outside the convolutions (the loss / statistics half of csrc/loss_voxel.hip, csrc/norm.hip,
csrc/gemm_skinny.hip), each called alone through the C ABI with raw pointers, against its own float64 statement
(tests/reduction_restatement.py; anchored on the CPU by tests/test_reduction_restatement_cpu.py).

Every launch goes through `call` (tests/guarded.py): outputs between sentinel guards, pitched outputs with sentinel gaps, inputs with NaN
gaps and guards, `+=` outputs start non-zero.  Rules (profiles/pointwise_tests_notes.md §1, profiles/reduction_tests_notes.md):
  bit        selection and data movement: masked pixels give exactly 0, untouched grids, zeros that stay zeros;
  exact      integer-valued data, every partial sum below 2^24 (fp32) / 2^53 (fp64), asserted on the float64 side; counts always;
  derived    (n + 2) x u x sum |term|, u = 2^-53 for the fp64 accumulations and 2^-24 for the fp32 ones, + one 2^-24 per fp32 result, + the
             cancellation term on the absolute values of the two parts where a variance or the SI loss is a difference;
  measured   derived + 4 x the measured error of logf / expf / sigmoidf_ x the sensitivity (LOGF_ERR, EXPF_REL: test_intrinsic_errors_log_exp;
             SIGMOID_ERR is the point-wise suite's).
No bound is taken from the kernel under test."""
import pytest
import torch

from rpg_ramnet_amd import _hip
import reduction_restatement as rr
from guarded import (BADARG, F64, SENT, SIG_RANGE, SIGMOID_ERR, TRIP2, U, In, Out, _bits, assert_bits, assert_exact, assert_within, call,
                     rn, ri, settle)

pytestmark = pytest.mark.gpu

E64 = 2.0 ** -53
I64 = torch.int64
# Measured on the MI355X by test_intrinsic_errors_log_exp (profiles/reduction_tests_notes.md §2): the largest absolute error of logf over
# [2^-5, 2^5] (through ramnet_si_log_loss_bwd) and the largest relative error of expf over [-6.5, 1] (through ramnet_metric_depth), against float64
LOGF_ERR = 5.3e-7               # measured 5.2673e-07
EXPF_REL = 8.1e-8               # measured 8.0345e-08
LOG_LO, LOG_HI = 2.0 ** -5, 2.0 ** 5
EXP_LO, EXP_HI = -6.5, 1.0
SI_BIG = 2 * 262144 + 4 * 777 + 3          # past the 64 x 1024 x 4 first trip of the one-launch SI statistics, ragged, with a tail
SI_CAPTURE = 4 * 262144 + 4 * 777 + 3      # the same for the 256 workgroups of the form used inside a capture


def f32v(x):
    """the fp32 value a float argument has behind the C ABI"""
    return float(torch.tensor(x, dtype=torch.float32))


def d64(data):
    return In(data, dtype=F64)


def nan_mask(n, share, seed):
    """share: 0.0, 0.2, 'one' (all but one pixel NaN), 'all'"""
    if share == "all":
        return torch.ones(n, dtype=torch.bool)
    if share == "one":
        m = torch.ones(n, dtype=torch.bool)
        m[n // 2] = False
        return m
    return torch.rand(n, generator=torch.Generator().manual_seed(seed)) < share


def same_or_nan(got, ref, what):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), "%s: NaN where the statement has a number (or the reverse): %r / %r" % (what, got[:4], ref[:4])
    return ~torch.isnan(ref)


def assert_same64(got, ref, unit, what):
    """exact in float64: the statement is a multiple of 1 / unit below 2^53 / unit (NaN where the statement is NaN)"""
    ok = same_or_nan(got, ref, what)
    g, r = got.double().reshape(-1)[ok], ref.reshape(-1)[ok]
    assert torch.equal(r * unit, (r * unit).round()) and (r.numel() == 0 or float(r.abs().max()) * unit < 2 ** 53), "%s: the case is not exact" % what
    assert torch.equal(g, r), "%s: %r != %r" % (what, g[g != r][:4].tolist(), r[g != r][:4].tolist())


def within_or_nan(got, ref, bound, what):
    ok = same_or_nan(got, ref, what)
    if bool(ok.any()):
        assert_within(got.reshape(-1)[ok], ref.reshape(-1)[ok], bound.reshape(-1)[ok], what)


def assert_count(got, ref, what):
    assert float(got) == float(ref), "%s: %r != %r" % (what, float(got), float(ref))


# ------------------------------------------------------------------------------------------------ the two measured intrinsics
def test_intrinsic_errors_log_exp():
    """logf through ramnet_si_log_loss_bwd (pred = 1, lambda = 0, stats = (0, 0, 2): dpred = (float)((double)(logf(1) - logf(x)) / 1) = -logf(x)
    itself) and expf through ramnet_metric_depth (reg = clip = 1, y = x + 1 with x a multiple of 2^-20: reg (y - 1) = x exactly, the result is
    expf(x) itself), each over the argument range the tests below stay in, against float64.  The recorded constants are these maxima; the
    tests use 4 x them."""
    n = 1 << 17
    g = torch.Generator().manual_seed(90)
    xs = torch.cat([torch.exp2(torch.linspace(-5.0, 5.0, n, dtype=F64)).float(), torch.exp(torch.randn(n, generator=g)).clamp(LOG_LO, LOG_HI)]).to(F64)
    out = Out(1, 2 * n)
    call("ramnet_si_log_loss_bwd", In(torch.ones(2 * n)), In(xs), 2 * n, 0.0, d64(torch.tensor([0.0, 0.0, 2.0, 0.0])), None, out, )
    el = float((out.value().double().view(-1) + torch.log(xs)).abs().max())
    step = (EXP_HI - EXP_LO) / n                       # 7.5 / 2^17 = 60 x 2^-20
    grid = EXP_LO + step * torch.arange(n, dtype=F64)
    rnd = ((torch.randn(n, generator=g).to(F64) * 2.0 - 1.5).clamp(EXP_LO, EXP_HI) * 2 ** 20).round() / 2 ** 20
    xe = torch.cat([grid, rnd])
    assert torch.equal((xe + 1.0).float().to(F64) - 1.0, xe)
    out = Out(1, 2 * n)
    call("ramnet_metric_depth", In(xe + 1.0), 2 * n, 1.0, 1.0, 0, out)
    ee = float(((out.value().double().view(-1) - torch.exp(xe)).abs() / torch.exp(xe)).max())
    print("measured: logf max |err| %.4e over [%g, %g]; expf max relative err %.4e over [%g, %g]" % (el, LOG_LO, LOG_HI, ee, EXP_LO, EXP_HI))
    assert el <= LOGF_ERR and ee <= EXPF_REL


# ------------------------------------------------------------------------------------------------ SI / SI-log statistics and loss
def _si_data(n, log, kind, share, seed):
    if log:
        p, t = (torch.exp(rn(n, seed=sd)).clamp(LOG_LO, LOG_HI).float().to(F64) for sd in (seed, seed + 1))
    elif kind == "int":
        p, t = ri(n, seed=seed, m=8), ri(n, seed=seed + 1, m=8)
    else:
        p, t = rn(n, seed=seed), rn(n, seed=seed + 1)
    t[nan_mask(n, share, seed + 2)] = float("nan")
    return p, t


def _si_bounds(p, t, log, w, lam):
    """bounds of (S1, S2) and of the loss.  Plain form: d is the same fp32 difference on both sides, d^2 is exact in fp64, the sums run in
    fp64: (n + 2) 2^-53 sum |term|.  Log form: each logf carries 4 x LOGF_ERR, the fp32 difference one rounding."""
    sa, st = rr.si_stats_abs(p, t, log), rr.si_stats(p, t, log)
    nv = float(st[2])
    n = p.numel()
    b1, b2 = (n + 2) * E64 * sa[0], (n + 2) * E64 * sa[1]
    if log:
        d = rr.si_diff(p, t, True)
        d = d[~torch.isnan(d)].abs()
        ed = 8 * LOGF_ERR + U * d
        b1, b2 = b1 + ed.sum(), b2 + (2 * d * ed + ed * ed).sum()
    if nv == 0:
        return torch.stack([b1, b2]), None
    m = (sa[0] / nv)
    lb = w * (b2 / nv + lam * 2 * m * b1 / nv + lam * (b1 / nv) ** 2) + (8 * E64 + U) * w * (sa[1] / nv + lam * m * m)
    return torch.stack([b1, b2]), lb


def _si_args(p, t, log, w, lam, skp=0, skt=0):
    stats, loss = Out(1, 4, dtype=F64), Out(1, 1)
    args = (In(p, skew=skp), In(t, skew=skt), p.numel()) + ((lam,) if log else (w, lam)) + (stats, loss)
    return stats, loss, ("ramnet_si_log_loss_fwd" if log else "ramnet_si_loss_fwd",) + args


def _si_fwd(p, t, log, w, lam, skp=0, skt=0):
    stats, loss, args = _si_args(p, t, log, w, lam, skp, skt)
    call(*args)
    return stats, loss


def _si_check(stats, loss, p, t, log, kind, w, lam, what):
    ref = rr.si_stats(p, t, log)
    if log:          # the arguments of logf stay inside the measured range
        tv = t[~torch.isnan(t)]
        assert float(p.min()) >= LOG_LO and float(p.max()) <= LOG_HI and (tv.numel() == 0 or (float(tv.min()) >= LOG_LO and float(tv.max()) <= LOG_HI))
    got = stats.value().view(-1)[:3]
    assert_count(got[2], ref[2], what + " count")
    sb, lb = _si_bounds(p, t, log, w, lam)
    if kind == "int" and not log:
        assert_exact(got[:2], ref[:2], what + " S1, S2", abs_sum=rr.si_stats_abs(p, t, log))
    else:
        assert_within(got[:2], ref[:2], sb, what + " S1, S2")
    if float(ref[2]) == 0:
        assert bool(torch.isnan(loss.value()).all()), "%s: the loss of an all-NaN target is NaN" % what
        assert float(got[0]) == 0.0 and float(got[1]) == 0.0
    else:
        assert_within(loss.value().view(-1), rr.si_loss_from_stats(ref, w, lam).view(-1), lb.view(-1), what + " loss")


@pytest.mark.parametrize("skew", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, SI_BIG])
def test_si_forward(n, log, skew):
    """count exact, S1 / S2 exact on integers and derived on normal data (measured for the log form), the loss derived; aligned and skewed
    pointers (the scalar branch), every NaN share.  The all-NaN case pins that the call returns, with count 0 and a NaN loss."""
    w, lam = f32v(0.5), f32v(0.85)
    for share in (0.0, 0.2, "one", "all"):
        for kind in (("normal",) if log else ("int", "normal")):
            p, t = _si_data(n, log, kind, share, 100)
            stats, loss = _si_fwd(p, t, log, w, lam, *skew)
            _si_check(stats, loss, p, t, log, kind, 1.0 if log else w, lam, "si%s_fwd[%s, %s]" % ("_log" if log else "", share, kind))


@pytest.mark.parametrize("log", [False, True])
def test_si_forward_is_reproducible_across_sizes(log):
    """two calls with a call of another size in between give identical bits (the one-launch form keeps partial sums and a self-resetting
    ticket in a scratch of the library)"""
    p, t = _si_data(SI_BIG, log, "normal", 0.2, 110)
    q, u = _si_data(1027, log, "normal", 0.2, 113)
    a, la = _si_fwd(p, t, log, 1.0, 1.0)
    _si_fwd(q, u, log, 1.0, 1.0)
    b, lb = _si_fwd(p, t, log, 1.0, 1.0)
    assert torch.equal(_bits(a.value()[:, :3]), _bits(b.value()[:, :3])), "the statistics differ between two calls: %r / %r" % (a.value(), b.value())
    assert torch.equal(_bits(la.value()), _bits(lb.value())), "the loss differs between two calls"


@pytest.mark.parametrize("log", [False, True])
def test_si_forward_capture_form(log):
    """Inside a stream capture the library hands out no scratch: zero-fill + atomics on `stats` (si_stats_kernel, both instances; 256
    workgroups, so SI_CAPTURE takes a ragged second trip).  Recorded once on a single stream (one chain, no parallel branches), replayed
    once, against the one-launch form: equal count, sums and loss within the derived (log: measured) bound."""
    p, t = _si_data(SI_CAPTURE, log, "normal", 0.2, 120)
    w, lam = (1.0 if log else f32v(0.5)), f32v(0.85)
    eager, eloss = _si_fwd(p, t, log, w, lam)
    stats, loss, args = _si_args(p, t, log, w, lam)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(*args, stream=torch.cuda.current_stream().cuda_stream, defer=True)
    g.replay()
    settle(*args)
    _si_check(stats, loss, p, t, log, "normal", w, lam, "si%s_fwd (captured)" % ("_log" if log else ""))
    assert_count(stats.value()[0, 2], eager.value()[0, 2], "si_fwd captured against one-launch: count")
    sb, lb = _si_bounds(p, t, log, w, lam)
    assert_within(stats.value()[0, :2], eager.value()[0, :2].double(), 2 * sb, "si_fwd captured against one-launch")
    assert_within(loss.value().view(-1), eloss.value().double().view(-1), 2 * lb.view(-1), "si_fwd loss captured against one-launch")


@pytest.mark.parametrize("stats", [(3.0, 5.0, 4.0), (-7.25, 1234.5, 1027.0), (0.0, 0.0, 0.0), (1e-3, 1e-6 + 3e-9, 1.0)])
def test_si_loss_from_stats(stats):
    st = torch.tensor(stats + (0.0,), dtype=F64)
    for w, lam in ((1.0, 1.0), (f32v(0.5), f32v(0.85))):
        loss = Out(1, 1)
        call("ramnet_si_loss_from_stats", d64(st), w, lam, loss)
        ref = rr.si_loss_from_stats(st, w, lam)
        if st[2] == 0:
            assert bool(torch.isnan(loss.value()).all()) and bool(torch.isnan(ref))
        else:
            m = st[0].abs() / st[2]
            assert_within(loss.value().view(-1), ref.view(-1), ((8 * E64 + U) * w * (st[1].abs() / st[2] + lam * m * m)).view(-1), "si_loss_from_stats")


@pytest.mark.parametrize("wl", [(1.0, 1.0), (0.5, 0.85)])
@pytest.mark.parametrize("with_gscale", [False, True])
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("n", [1, 5, 1027, TRIP2])
def test_si_backward(n, log, with_gscale, wl):
    """statistics supplied by the test (not a forward's): g = gscale w 2 / N (d - lambda mean) in fp64, rounded once; NaN positions are
    exactly 0.  The log form divides by pred and carries 4 x LOGF_ERR per logarithm."""
    w, lam = (1.0 if log else f32v(wl[0])), f32v(wl[1])
    p, t = _si_data(n, log, "normal", 0.2 if n > 1 else 0.0, 130)
    nv = float((~torch.isnan(t)).sum())
    st = torch.tensor([0.37 * (nv + 3), 2.0 * (nv + 3), nv + 3, 0.0], dtype=F64)
    gs = 0.75
    dp = Out(1, n)
    args = (In(p), In(t), n) + ((lam,) if log else (w, lam)) + (d64(st), In(torch.tensor([gs])) if with_gscale else None, dp)
    call("ramnet_si_log_loss_bwd" if log else "ramnet_si_loss_bwd", *args)
    gsv = gs if with_gscale else 1.0
    ref = rr.si_bwd(p, t, st, w, lam, gsv, log)
    d = torch.nan_to_num(rr.si_diff(p, t, log))
    s2 = 2.0 * gsv * w / st[2]
    bound = U * ref.abs() + 8 * E64 * s2 * (d.abs() + lam * (st[0] / st[2]).abs()) / (p if log else 1.0)
    if log:
        assert float(p.min()) >= LOG_LO and float(p.max()) <= LOG_HI and float(t[~torch.isnan(t)].min()) >= LOG_LO and float(t[~torch.isnan(t)].max()) <= LOG_HI
        bound = bound + s2 * (8 * LOGF_ERR + U * d.abs()) / p
    nan = torch.isnan(t)
    assert_bits(dp.value().view(-1)[nan], torch.zeros(int(nan.sum()), dtype=F64), "si_bwd at NaN targets")
    assert_within(dp.value().view(-1)[~nan], ref[~nan], bound[~nan], "si%s_bwd" % ("_log" if log else ""))


# ------------------------------------------------------------------------------------------------ mse term
MSE_SHAPES = [(1, 2, 2), (2, 5, 7), (1, 8, 9), (3, 33, 46), (2, 725, 727)]     # the last: a second trip of the 256 x 1024 statistics grid (also
#                                                                                under `half`: 2 x 362 x 363 cells) and of the backward's 2048 x 256


def _mse_data(B, H, W, kind, share, seed):
    p, t = (ri(B, H, W, seed=seed, m=8), ri(B, H, W, seed=seed + 1, m=8)) if kind == "int" else (rn(B, H, W, seed=seed), rn(B, H, W, seed=seed + 1))
    t.view(-1)[nan_mask(B * H * W, share, seed + 2)] = float("nan")
    return p, t


def mse_check(got, loss, p, t, half, kind, what):
    """test_mse_forward's rule (tests/stream_worker.py holds the launch to it on other streams): got = (sum d^2, count, ...) as the device left them"""
    ref = rr.mse_stats(p, t, bool(half))
    assert_count(got[1], ref[1], what + " count")
    ncell = p.numel() // (4 if half else 1)
    if kind == "int":
        assert_exact(got[:1], ref[:1], what + " sum d^2")
    else:
        assert_within(got[:1], ref[:1], (ncell + 2) * E64 * ref[:1], what + " sum d^2")
    if float(ref[1]) == 0:
        assert bool(torch.isnan(loss).all()) and float(got[0]) == 0.0
    else:
        assert_within(loss.view(-1), rr.mse_loss(ref).view(-1), ((ncell + 4) * E64 + U) * rr.mse_loss(ref).view(-1), what + " loss")


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("B,H,W", MSE_SHAPES)
def test_mse_forward(B, H, W, half):
    """sum d^2 and count exact on integers (d a multiple of 1/4 after the 2 x 2 mean), derived on normal data (the cell and d are the same
    fp32 operations on both sides); the loss one fp32 rounding of S / N"""
    for share in (0.0, 0.2, "one", "all"):
        for kind in ("int", "normal"):
            p, t = _mse_data(B, H, W, kind, share, 140)
            stats, loss = Out(1, 4, dtype=F64), Out(1, 1)
            call("ramnet_mse_loss_fwd", In(p.view(-1)), In(t.view(-1)), B, H, W, half, stats, loss)
            mse_check(stats.value().view(-1), loss.value(), p, t, half, kind, "mse_fwd[%s, %s]" % (share, kind))


@pytest.mark.parametrize("with_gscale", [False, True])
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("B,H,W", MSE_SHAPES)
def test_mse_backward(B, H, W, half, with_gscale):
    """count supplied by the test.  g = (float)(2 gscale / N [/ 4] d): one fp32 rounding of an fp64 product.  Masked cells (all four pixels of
    a block under `half`) and the dropped odd row / column receive exactly 0."""
    for share in (0.0, 0.2, "one", "all"):
        p, t = _mse_data(B, H, W, "normal", share, 150)
        st = torch.tensor([1.0, float(B * H * W) + 5.0, 0.0, 0.0], dtype=F64)
        dp = Out(1, B * H * W)
        call("ramnet_mse_loss_bwd", In(p.view(-1)), In(t.view(-1)), B, H, W, half, d64(st), In(torch.tensor([0.75])) if with_gscale else None, dp)
        ref = rr.mse_bwd(p, t, bool(half), st, 0.75 if with_gscale else 1.0)
        got = dp.value().view(B, H, W)
        zero = ref == 0
        assert_bits(got[zero], ref[zero], "mse_bwd at masked / dropped pixels")
        if half:
            assert bool(zero[:, 2 * (H // 2):].all()) and bool(zero[:, :, 2 * (W // 2):].all())
            tc = rr.mse_cell(t, True)
            blk = torch.isnan(tc).repeat_interleave(2, 1).repeat_interleave(2, 2)
            assert bool(zero[:, :2 * (H // 2), :2 * (W // 2)][blk].all())
        assert_within(got, ref, (U + 8 * E64) * ref.abs(), "mse_bwd[half=%d, %s]" % (half, share))


# ------------------------------------------------------------------------------------------------ depth metrics
def _depth_inputs(n, clip, reg, cutoff_share, seed):
    """normalised log depths whose float64 metric depth / ratio keep 1e-4 relative clear of the cut-off and of 1.25^k: pixels that come too
    close are MOVED, none is dropped"""
    g = torch.Generator().manual_seed(seed)
    tn = torch.rand(n, generator=g).float().to(F64)
    pn = (torch.rand(n, generator=g) * 1.2 - 0.1).float().to(F64)
    tn[nan_mask(n, 0.15 if n > 1 else 0.0, seed + 1)] = float("nan")
    cutoff = float("inf")
    if cutoff_share:
        t, _ = rr.metric_depths(pn, tn, clip, reg)
        cutoff = f32v(float(t[~torch.isnan(t)].median())) if bool((~torch.isnan(t)).any()) else 1.0
    near = lambda v, c: (v - c).abs() <= 1e-4 * c
    for _ in range(50):
        t, p = rr.metric_depths(pn, tn, clip, reg)
        _, ratio = rr.depth_metric_terms(t, p)
        bad = near(ratio, 1.25) | near(ratio, 1.25 ** 2) | near(ratio, 1.25 ** 3)
        if cutoff_share:
            bad |= near(t, cutoff)
        bad &= ~torch.isnan(tn)
        if not bool(bad.any()):
            break
        tn[bad] = ((tn[bad] + 0.0137) % 1.0).float().to(F64)
    assert not bool(bad.any())
    return pn, tn, cutoff


@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("n", [1, 5, 1027, TRIP2])
def test_depth_metrics(n, cut):
    """the four counts exact (no pixel's metric depth or ratio within 1e-4 relative of a decision, asserted in float64); the seven sums
    measured: the fp32 metric depths carry a relative error of (2 |x| + 2) 2^-24 + 4 EXPF_REL (two roundings of the argument x = reg (y - 1),
    expf, the product with clip), which reaches each sum through its first derivatives (autograd, float64; second order: a factor 1.001)."""
    clip, reg = 80.0, f32v(3.70378)
    pn, tn, cutoff = _depth_inputs(n, clip, reg, cut, 160)
    out = Out(1, 11, dtype=F64)
    call("ramnet_depth_metrics", In(pn), In(tn), n, clip, reg, cutoff, out)
    ref, got = rr.depth_metrics(pn, tn, clip, reg, cutoff), out.value().view(-1)
    for k in (0, 1, 8, 9, 10):
        assert_count(got[k], ref[k], "depth_metrics out[%d]" % k)
    xmax = reg * 1.101
    assert -xmax >= EXP_LO and 0.101 * reg <= EXP_HI and float(pn.min()) >= -0.101 and float(pn.max()) <= 1.101
    e = (2 * xmax + 2) * U + 4 * EXPF_REL
    t, p = rr.metric_depths(pn, tn, clip, reg)
    ok = ~torch.isnan(tn) & (t < cutoff)
    if not bool(ok.any()):
        assert float(got[2:8].abs().max()) == 0.0
        return
    t, p = t[ok].clone().requires_grad_(True), p[ok].clone().requires_grad_(True)
    terms, _ = rr.depth_metric_terms(t, p)
    bounds = []
    for term in terms:
        gt, gp = torch.autograd.grad(term.sum(), (t, p), retain_graph=True)
        bounds.append(1.001 * e * ((gt.abs() * t).sum() + (gp.abs() * p).sum()).detach() + (n + 2) * E64 * term.sum().detach())
    assert_within(got[2:8], ref[2:8], torch.stack(bounds), "depth_metrics sums")


# ------------------------------------------------------------------------------------------------ multi-scale gradient loss
MSG_SHAPES = [(1, 8, 8), (2, 9, 11), (1, 21, 27), (3, 16, 40), (1, 13, 8)]


def _msg_data(B, H, W, variant, seed):
    p, t = ri(B, H, W, seed=seed, m=16), ri(B, H, W, seed=seed + 1, m=16)
    if variant == "nan20":
        t.view(-1)[nan_mask(B * H * W, 0.2, seed + 2)] = float("nan")
    elif variant == "image":
        t[B - 1] = float("nan")
    return p, t


@pytest.mark.parametrize("variant", ["full", "nan20", "image"])
@pytest.mark.parametrize("ns", [1, 2, 3, 4])
@pytest.mark.parametrize("case", range(len(MSG_SHAPES)))
def test_msg_loss(case, ns, variant):
    """Integer data: the pooled maps (multiples of 1/64) and the Sobel responses (multiples of 1/512) are exact in fp32, so the sign of every
    response is the same on both sides; per-scale sums and counts exact, the workspace bit for bit.  Backward from the statement's pooled maps
    and counts CHOSEN by the test: (terms + 2 + 2 + 4) 2^-24 x the adjoint on absolute values (terms: the scatter adds that meet in a cell; the
    coefficient has 2 roundings; up to 4 scales are added).  Sizes that are no multiple of 2^(ns-1): the cropped rows / columns get what
    the statement gives (exactly 0 where no scale reaches them)."""
    B, H, W = MSG_SHAPES[case]
    p, t = _msg_data(B, H, W, variant, 170)
    L = _hip.lib()
    total = int(L.ramnet_msg_workspace_elems(B, H, W, ns))
    assert total == rr.msg_workspace_elems(B, H, W, ns) > 0
    ws, stats, loss = Out(1, total), Out(1, 2 * ns, dtype=F64), Out(1, 1)
    call("ramnet_msg_loss_fwd", In(p.view(-1)), In(t.view(-1)), B, H, W, ns, ws, stats, loss)
    rstats, rloss, rws = rr.msg_forward(p, t, ns)
    assert_same64(stats.value(), rstats, 512, "msg_fwd per-scale (sum, count)")
    ok = same_or_nan(ws.value(), rws, "msg_fwd workspace")
    assert_bits(ws.value().view(-1)[ok], rws[ok], "msg_fwd workspace")
    within_or_nan(loss.value(), rloss.view(-1), (U + 16 * E64) * rloss.abs().view(-1), "msg_fwd loss")
    given = rstats.clone()
    given[1::2] += 5.0
    gs = 0.75 if (case + ns) % 2 else None
    dws, dp = Out(1, total), Out(1, B * H * W)
    call("ramnet_msg_loss_bwd", In(rws, fill=float("nan")), d64(given), None if gs is None else In(torch.tensor([gs])), B, H, W, ns, dws, dp)
    ref, aref, nterm = rr.msg_backward(rws, given, B, H, W, ns, 1.0 if gs is None else gs)
    assert nterm <= 72
    got = dp.value().view(B, H, W)
    assert_within(got, ref, (nterm + 2 + 2 + 4) * U * aref, "msg_bwd")
    assert_bits(got[aref == 0], ref[aref == 0], "msg_bwd where nothing arrives (NaN cells, cropped rows / columns)")
    assert bool((aref[torch.isnan(t)] == 0).all())


def test_msg_empty_scale_is_refused():
    L = _hip.lib()
    assert L.ramnet_msg_workspace_elems(1, 7, 8, 4) == 0 and L.ramnet_msg_workspace_elems(1, 8, 8, 5) == 0 and L.ramnet_msg_workspace_elems(1, 8, 8, 0) == 0
    i, o, st = In(torch.zeros(256)), Out(1, 256), Out(1, 8, dtype=F64)
    call("ramnet_msg_loss_fwd", i, i, 1, 7, 8, 4, o, st, Out(1, 1), rc=BADARG)
    call("ramnet_msg_loss_bwd", i, d64(torch.ones(8)), None, 1, 7, 8, 4, o, Out(1, 56), rc=BADARG)


# ------------------------------------------------------------------------------------------------ nonzero statistics / normalisation
def _grid(n, seed, kind="normal"):
    if kind == "zero":
        return torch.zeros(n, dtype=F64)
    if kind in ("one", "one_up"):                  # a single distinct non-zero value whose square is no fp32 number: 0.3f * 0.3f rounds down,
        g = torch.zeros(n, dtype=F64)              # 0.2f * 0.2f up (a fused ms - mean * mean would leave a negative / a positive variance)
        g[::2] = f32v(0.3 if kind == "one" else 0.2)
        return g
    if n <= 4:
        return torch.tensor([1.5, 0.0, -0.5, 2.0][:n], dtype=F64)
    g = (rn(n, seed=seed) + 0.5).float().to(F64)
    g[nan_mask(n, 0.3, seed + 1)] = 0.0
    g[1] = -0.0 if n > 8 else g[1]
    return g


def _normalize_bound(g):
    """mean, mean square and their difference in fp32: the variance carries 4 x 2^-24 (ms + mean^2), the standard deviation half of that
    relative to the variance + 1 rounding; (v - mean) / sd: the rounded mean, the difference, the quotient"""
    S1, S2, cnt = rr.nonzero_stats(g)
    mean, ms = S1 / cnt, S2 / cnt
    var = ms - mean * mean
    assert float(var) >= 0.1 * float(ms), "the case cancels too much for a derived bound"
    sd = torch.sqrt(var)
    out = (g - mean) / sd
    esd = 0.5 * 4 * U * (ms + mean * mean) / var + 2 * U
    return torch.where(g != 0, (U * mean.abs() + U * (g - mean).abs()) / sd + out.abs() * (esd + 2 * U), torch.zeros_like(g))


def _check_normalized(got, g, what):
    ref = rr.normalize_nonzero(g)
    if torch.equal(ref, g):
        assert_bits(got, g, what + " (left unchanged)")
        return
    zero = g == 0
    assert_bits(got[zero], torch.zeros(int(zero.sum()), dtype=F64), what + ": zeros stay +0")
    assert_within(got, ref, _normalize_bound(g), what)


def _check_nonzero_stats(got, g, what):
    ref = rr.nonzero_stats(g)
    assert_count(got[2], ref[2], what + " count")
    n = g.numel()
    assert_within(got[:2], ref[:2], (n + 2) * E64 * torch.stack([g.abs().sum(), ref[1]]), what + " sums")


@pytest.mark.parametrize("kind", ["normal", "zero", "one", "one_up"])
@pytest.mark.parametrize("n", [1, 3, 5, 1027, TRIP2])
def test_normalize_nonzero(n, kind):
    g = _grid(n, 180, kind)
    grid, scratch = Out(1, n, prefill=g), Out(1, 3, dtype=F64)
    call("ramnet_normalize_nonzero", grid, n, scratch)
    _check_nonzero_stats(scratch.value().view(-1), g, "normalize_nonzero scratch")
    _check_normalized(grid.value().view(-1), g, "normalize_nonzero[%s]" % kind)


@pytest.mark.parametrize("G,n", [(1, 4), (5, 4), (64, 4), (1, 1028), (5, 1028), (64, 1028), (64, 131072 + 1028)])
def test_nonzero_batch(G, n):
    """grid 1 is all zero and grids 2 / 3 hold a single distinct value (0.3f / 0.2f) when there are that many; 64 grids of 132 100 floats run a second trip of
    the 128 workgroups x 256 threads x 4 floats each grid gets"""
    gs = torch.stack([_grid(n, 190 + 2 * k, {1: "zero", 2: "one", 3: "one_up"}.get(k, "normal")) for k in range(G)])
    stats = Out(1, 3 * G, dtype=F64)
    call("ramnet_nonzero_stats_batch", In(gs.view(-1)), G, n, stats)
    grids, scratch = Out(1, G * n, prefill=gs), Out(1, 3 * G, dtype=F64)
    call("ramnet_normalize_nonzero_batch", grids, G, n, scratch)
    for k in (range(G) if G * n < 100000 else (0, 1, 2, 31, 63)):
        _check_nonzero_stats(stats.value().view(G, 3)[k], gs[k], "nonzero_stats_batch grid %d" % k)
        _check_nonzero_stats(scratch.value().view(G, 3)[k], gs[k], "normalize_nonzero_batch scratch %d" % k)
        _check_normalized(grids.value().view(G, n)[k], gs[k], "normalize_nonzero_batch grid %d" % k)


# ------------------------------------------------------------------------------------------------ norm
NORM_C = [1, 6, 12, 32, 48, 2048 + 4]
NORM_GN = [(1, 1), (1, 2), (3, 91), (2, 4099)]


def _layout(C_, lay):
    """(ld, skew): 0 dense, 1 pitched (a multiple of 4 beyond C), 2 pitch C + 1 (breaks the 16-byte alignment of the rows), 3 skewed pointer"""
    return [(C_, 0), (C_ + 8, 0), (C_ + 1, 0), (C_, 1)][lay]


def _nin(t, C_, lay):
    ld, skew = _layout(C_, lay)
    return In(t.reshape(-1, C_), ld, skew=skew), ld


def _nout(rows, C_, lay, **kw):
    ld, skew = _layout(C_, lay)
    return Out(rows, C_, ld=ld, skew=skew, **kw), ld


def _split_slabs(sums, nslab, seed):
    """[groups][C][2] -> part [groups][nslab][C][2] whose float64 sum over the slabs the statement then takes as the given statistics"""
    w = torch.rand(nslab, generator=torch.Generator().manual_seed(seed)).to(F64) + 0.1
    return sums[:, None] * (w / w.sum())[None, :, None, None]


@pytest.mark.parametrize("gi", range(len(NORM_GN)))
@pytest.mark.parametrize("ci", range(len(NORM_C)))
def test_norm_partial_exact(ci, gi):
    """forward (a = b = x) and backward (a = dy act'(y), b = x) partial sums on integer data, summed over the slabs: exact in fp64.  Layout
    and activation rotate with the two indices, so that every C meets every layout (dense, pitched, a pitch of C + 1 and a skewed pointer,
    which both take the scalar kernel at C % 4 == 0) and every activation; nslab as ramnet_norm_slabs gives it, and another one."""
    C_, (G, npix) = NORM_C[ci], NORM_GN[gi]
    lay, act = (ci + gi) % 4, (ci + 2 * gi) % 3
    x, dy = ri(G, npix, C_, seed=200, m=8), 16 * ri(G, npix, C_, seed=201, m=4)
    y = (ri(G, npix, C_, seed=202, m=1) + 2) / 4 if act == 2 else ri(G, npix, C_, seed=202, m=2)      # sigmoid outputs 1/4, 1/2, 3/4: y (1 - y) = 3/16, 1/4
    L = _hip.lib()
    ns0 = L.ramnet_norm_slabs(G, npix, C_)
    assert ns0 >= 1
    (xi, ld), (di, ldd), (yi, ldy) = _nin(x, C_, lay), _nin(dy, C_, lay), _nin(y, C_, (lay + 1) % 2 if lay < 2 else lay)
    for nslab in (ns0, ns0 + 3):
        part = Out(1, G * nslab * C_ * 2, dtype=F64)
        call("ramnet_norm_partial", xi, ld, None, 0, 0, xi, ld, G, npix, C_, nslab, part)
        assert_exact(part.value().view(G, nslab, C_, 2).sum(1), rr.norm_partial(x, x), "norm_partial forward", abs_sum=rr.norm_partial(x.abs(), x.abs()))
        part = Out(1, G * nslab * C_ * 2, dtype=F64)
        call("ramnet_norm_partial", di, ldd, yi, ldy, act, xi, ld, G, npix, C_, nslab, part)
        assert_exact(part.value().view(G, nslab, C_, 2).sum(1), rr.norm_partial(dy, x, y, act), "norm_partial backward",
                     abs_sum=rr.norm_partial(dy.abs(), x.abs(), y.abs(), act if act != 1 else 0))


@pytest.mark.parametrize("gi", range(len(NORM_GN)))
@pytest.mark.parametrize("ci", range(len(NORM_C)))
def test_norm_finalize(ci, gi):
    """statistics GIVEN as partial sums chosen by the test.  groups = 1: running statistics (use_running) at one of npix 1 / 2 per C, batch
    statistics at the other (npix = 1: no update, and the update refused; npix = 2: momentum 0.1 with num_batches_tracked); groups > 1:
    update with momentum 1.0 / 0.1, with / without num_batches_tracked.  use_running with update_running set as well leaves buffers and
    counter alone, as torch's eval mode does.  NULL gamma / beta rotate.  fp64 results: a few 2^-53 of the
    expression on absolute values (the variance is a difference: its two parts); fp32 results: one 2^-24 more."""
    C_, (G, npix) = NORM_C[ci], NORM_GN[gi]
    use_running = G == 1 and (ci + gi) % 2 == 0
    update = not use_running and npix > 1
    momentum = 1.0 if gi == 2 else 0.1
    tracked = update and (gi == 1 or (ci + gi) % 2 == 0)
    eval_flagged = use_running and ci % 2 == 1          # update_running given together with use_running: eval mode, nothing is updated or counted
    affine = (ci + gi) % 3 != 0
    eps = 1e-5
    L = _hip.lib()
    nslab = L.ramnet_norm_slabs(G, npix, C_) + (ci % 2) * 3
    m, v = rn(G, C_, seed=210), rn(G, C_, seed=211).abs() + 0.25
    sums = torch.stack([m * npix, (v + m * m) * npix], -1)
    part = _split_slabs(sums, nslab, 212)
    sums = part.sum(1)
    gamma, beta = (rn(C_, seed=213), rn(C_, seed=214)) if affine else (None, None)
    rm0, rv0 = rn(C_, seed=215), (rn(C_, seed=216).abs() + 0.5).float().to(F64)
    mean, rstd = Out(1, G * C_, dtype=F64), Out(1, G * C_, dtype=F64)
    scale, shift = Out(1, G * C_), Out(1, G * C_)
    rm, rv, nt = Out(1, C_, prefill=rm0), Out(1, C_, prefill=rv0), Out(1, 1, dtype=I64, prefill=torch.tensor([7]))
    args = lambda upd: (d64(part.view(-1)), G, nslab, C_, npix, eps, In(gamma) if affine else None, In(beta) if affine else None, rm, rv, momentum,
                        int(upd), int(use_running), nt if tracked or eval_flagged else None, mean, rstd, scale, shift)
    if npix == 1 and not use_running:
        call("ramnet_norm_finalize", *args(True), rc=BADARG)
    call("ramnet_norm_finalize", *args(update or eval_flagged))
    rmean, rrstd, rscale, rshift, nrm, nrv = rr.norm_finalize(sums, npix, eps, gamma, beta, rm0, rv0, momentum, update, use_running)
    pa = part.abs().sum(1)
    bm = (nslab + 4) * E64 * pa[..., 0] / npix
    bv = (nslab + 8) * E64 * (pa[..., 1] / npix + 2 * rmean * rmean) + 2 * rmean.abs() * bm
    if use_running:
        bm, bv = torch.zeros_like(bm), torch.zeros_like(bv)
    var = 1.0 / (rrstd * rrstd) - eps
    br = rrstd * (0.5 * bv / (var + eps) + 4 * E64)
    assert_within(mean.value().view(G, C_), rmean, bm + E64 * rmean.abs(), "norm_finalize mean")
    assert_within(rstd.value().view(G, C_), rrstd, br, "norm_finalize rstd")
    ga = torch.ones(C_, dtype=F64) if gamma is None else gamma.abs()
    be = torch.zeros(C_, dtype=F64) if beta is None else beta.abs()
    bs = ga[None] * br + (U + 2 * E64) * rscale.abs()
    assert_within(scale.value().view(G, C_), rscale, bs, "norm_finalize scale")
    assert_within(shift.value().view(G, C_), rshift, (U + 4 * E64) * (be[None] + (rmean * rscale).abs()) + bm * rscale.abs() + rmean.abs() * bs,
                  "norm_finalize shift")
    if update:
        unb = npix / (npix - 1.0)
        assert_within(rm.value().view(-1), nrm, (U + 8 * E64) * ((1 - momentum) * rm0.abs() + momentum * rmean.abs().mean(0)) + momentum * bm.mean(0),
                      "norm_finalize running_mean")
        assert_within(rv.value().view(-1), nrv, (U + 8 * E64) * ((1 - momentum) * rv0 + momentum * unb * var.mean(0)) + momentum * unb * bv.mean(0),
                      "norm_finalize running_var")
    else:
        assert_bits(rm.value().view(-1), rm0, "norm_finalize running_mean without update")
        assert_bits(rv.value().view(-1), rv0, "norm_finalize running_var without update")
    assert int(nt.value()[0, 0]) == (8 if tracked and update else 7), "num_batches_tracked"


@pytest.mark.parametrize("gi", range(len(NORM_GN)))
@pytest.mark.parametrize("ci", range(len(NORM_C)))
def test_norm_apply_and_bwd(ci, gi):
    """apply: x scale + shift [+ res] is 3 roundings (2 without res), ReLU keeps the bound, the sigmoid is measured (1/4-Lipschitz).
    bwd: dy' = dy act'(y) has 0 / 0 / 3 roundings (exactly dy or 0 without / with ReLU), dx = c1 dy' + c2 x + c3 four more."""
    C_, (G, npix) = NORM_C[ci], NORM_GN[gi]
    lay, act = (ci + gi) % 4, (ci + 2 * gi) % 3
    k = ci + gi
    with_res, with_dres, with_y = k % 2 == 0, (k // 2) % 2 == 0, act != 0 or k % 2 == 1
    x, res = rn(G, npix, C_, seed=220), rn(G, npix, C_, seed=221, scale=0.5)
    scale, shift = rn(G, C_, seed=222, scale=0.5), rn(G, C_, seed=223, scale=0.5)
    (xi, ldx), (resi, ldr) = _nin(x, C_, lay), _nin(res, C_, lay)
    out, ldo = _nout(G * npix, C_, lay)
    call("ramnet_norm_apply", xi, ldx, In(scale.view(-1)), In(shift.view(-1)), resi if with_res else None, ldr if with_res else 0, act, out, ldo, G, npix, C_)
    r = res if with_res else None
    ref = rr.norm_apply(x, scale, shift, r, act)
    zb = (3 + 1) * U * rr.norm_apply(x.abs(), scale.abs(), shift.abs(), None if r is None else r.abs(), 0)
    if act == 2:
        z = rr.norm_apply(x, scale, shift, r, 0)
        assert float(z.abs().max()) + float(zb.max()) <= SIG_RANGE
        zb = 0.25 * zb + 4 * SIGMOID_ERR
    assert_within(out.value().view(G, npix, C_), ref, zb, "norm_apply[act=%d]" % act)
    dy = rn(G, npix, C_, seed=224)
    y = torch.sigmoid(rn(G, npix, C_, seed=225)).float().to(F64) if act == 2 else rn(G, npix, C_, seed=225)
    y.view(-1)[::7] = 0.0
    c1, c2, c3 = rn(G, C_, seed=226), rn(G, C_, seed=227), rn(G, C_, seed=228)
    (di, ldd), (yi, ldy) = _nin(dy, C_, lay), _nin(y, C_, lay)
    dx, lddx = _nout(G * npix, C_, lay)
    dres, lddr = _nout(G * npix, C_, lay)
    call("ramnet_norm_bwd", di, ldd, yi if with_y else None, ldy if with_y else 0, act, xi, ldx, In(c1.view(-1)), In(c2.view(-1)), In(c3.view(-1)), dx, lddx,
         dres if with_dres else None, lddr if with_dres else 0, G, npix, C_)
    yy = y if with_y else None
    rdx, rg = rr.norm_bwd(dy, x, c1, c2, c3, yy, act)
    ga = dy.abs() * y * (1 + y) if act == 2 else rg.abs()
    adx = c1.abs()[:, None] * ga + c2.abs()[:, None] * x.abs() + c3.abs()[:, None]
    assert_within(dx.value().view(G, npix, C_), rdx, (7 + 1) * U * adx, "norm_bwd dx[act=%d]" % act)
    if with_dres:
        if act == 2:
            assert_within(dres.value().view(G, npix, C_), rg, (3 + 1) * U * ga, "norm_bwd dres")
        else:
            assert_bits(dres.value().view(G, npix, C_), rg, "norm_bwd dres")


@pytest.mark.parametrize("gi", range(len(NORM_GN)))
@pytest.mark.parametrize("ci", range(len(NORM_C)))
def test_norm_finalize_bwd(ci, gi):
    """partial sums, mean and rstd GIVEN by the test; dgamma / dbeta are assigned (they start from other values), NULL pairs rotate;
    batch_stats = 0 gives c2 = c3 = 0 exactly"""
    C_, (G, npix) = NORM_C[ci], NORM_GN[gi]
    batch_stats = (ci + gi) % 2
    affine, want_d = (ci + gi) % 3 != 0, (ci + gi) % 3 != 1
    L = _hip.lib()
    nslab = L.ramnet_norm_slabs(G, npix, C_) + (ci % 2) * 3
    part = _split_slabs(rn(G, C_, 2, seed=230, scale=float(npix)), nslab, 231)
    sums = part.sum(1)
    mean, rstd = rn(G, C_, seed=232), rn(G, C_, seed=233).abs() + 0.5
    gamma = rn(C_, seed=234) if affine else None
    c1, c2, c3 = Out(1, G * C_), Out(1, G * C_), Out(1, G * C_)
    dg, db = Out(1, C_, prefill=rn(C_, seed=235)), Out(1, C_, prefill=rn(C_, seed=236))
    call("ramnet_norm_finalize_bwd", d64(part.view(-1)), G, nslab, C_, npix, d64(mean.view(-1)), d64(rstd.view(-1)), In(gamma) if affine else None, batch_stats,
         c1, c2, c3, dg if want_d else None, db if want_d else None)
    r1, r2, r3, rdg, rdb = rr.norm_finalize_bwd(sums, npix, mean, rstd, gamma, bool(batch_stats))
    pa = part.abs().sum(1)
    a1, a2, a3, adg, adb = rr.norm_finalize_bwd(torch.stack([pa[..., 0], pa[..., 1] + 2 * mean.abs() * pa[..., 0]], -1), npix, -mean.abs(), rstd,
                                                None if gamma is None else gamma.abs(), bool(batch_stats))
    e = U + (nslab + 12) * E64
    assert_within(c1.value().view(G, C_), r1, e * a1.abs(), "norm_finalize_bwd c1")
    if batch_stats:
        assert_within(c2.value().view(G, C_), r2, e * a2.abs(), "norm_finalize_bwd c2")
        assert_within(c3.value().view(G, C_), r3, e * (a3.abs() + 2 * a2.abs() * mean.abs()), "norm_finalize_bwd c3")
    else:
        assert_bits(c2.value().view(G, C_), r2, "norm_finalize_bwd c2 without batch statistics")
        assert_bits(c3.value().view(G, C_), r3, "norm_finalize_bwd c3 without batch statistics")
    if want_d:
        assert_within(dg.value().view(-1), rdg, (e + G * E64) * adg.abs(), "norm_finalize_bwd dgamma (assigned)")
        assert_within(db.value().view(-1), rdb, (e + G * E64) * adb.abs(), "norm_finalize_bwd dbeta (assigned)")


def test_norm_pointwise_second_trip():
    """16 384 workgroups x 256 threads is the first trip of norm_pointwise_kernel: C = 4 with 4 194 304 + 777 pixels takes a ragged second"""
    C_, G, npix = 4, 1, 16384 * 256 + 777
    x = rn(npix, C_, seed=240)
    scale, shift = rn(G, C_, seed=241), rn(G, C_, seed=242)
    out = Out(npix, C_)
    call("ramnet_norm_apply", In(x), C_, In(scale.view(-1)), In(shift.view(-1)), None, 0, 1, out, C_, G, npix, C_)
    ref = rr.norm_apply(x[None], scale, shift, None, 1)
    assert_within(out.value().view(G, npix, C_), ref, (3 + 1) * U * rr.norm_apply(x[None].abs(), scale.abs(), shift.abs(), None, 0), "norm_apply second trip")


# ------------------------------------------------------------------------------------------------ GEMM
GEMM_SHAPES = [(1, 1, 4), (5, 31, 36), (33, 33, 124), (33, 8, 128), (40, 129, 132), (64, 161, 260), (7, 40, 516)]


class _Problem:
    """one batched product: A, B behind NaN gaps and a NaN row between the batch entries (strides larger than the matrices), C between
    sentinel gaps and a sentinel row between the entries"""

    def __init__(self, M, N, K, trans, acc, batch, pitched, kind, seed, lda=None):
        make = (lambda *s, seed: ri(*s, seed=seed, m=4)) if kind == "int" else rn
        self.M, self.N, self.K, self.batch, self.trans, self.acc = M, N, K, batch, trans, acc
        ar, ac = (K, M) if trans else (M, K)
        self.A, self.B = make(batch, ar, ac, seed=seed), make(batch, K, N, seed=seed + 1)
        self.C0 = make(batch, M, N, seed=seed + 2) if acc else None
        self.lda = ac + ((4 if not trans else 3) if pitched else 0) if lda is None else lda
        self.ldb, self.ldc = N + (5 if pitched else 0), N + (3 if pitched else 0)
        pad = lambda t, r: torch.cat([t, torch.full((batch, r, t.shape[2]), float("nan"), dtype=F64)], 1)
        ra = next(r for r in range(1, 5) if (ar + r) * self.lda % 4 == 0)           # (stride_a is a multiple of 4 floats)
        self.a, self.b = In(pad(self.A, ra), self.lda), In(pad(self.B, 1), self.ldb)
        pre = torch.full((batch, M + 1, N), SENT, dtype=F64)
        if acc:
            pre[:, :M] = self.C0
        self.c = Out(batch * (M + 1), N, ld=self.ldc, prefill=pre)
        self.sa, self.sb, self.sc = (ar + ra) * self.lda, (K + 1) * self.ldb, (M + 1) * self.ldc

    def check(self, kind, what, ksplit=4):
        got = self.c.value().view(self.batch, self.M + 1, self.N)
        assert bool((got[:, self.M] == torch.tensor(SENT, dtype=torch.float32)).all()), "%s wrote a row beyond its M" % what
        got = got[:, :self.M]
        ref = rr.gemm(self.A, self.B, self.C0, self.trans)
        aref = rr.gemm(self.A.abs(), self.B.abs(), None if self.C0 is None else self.C0.abs(), self.trans)
        if kind == "int":
            assert_exact(got, ref, what, abs_sum=aref)
        else:       # K products, and under `accumulate` up to ksplit partial sums and the value already there
            assert_within(got, ref, (self.K + 2 + (ksplit + 1 if self.acc else 0)) * U * aref, what)
        return got


def _gemm_call(p, rc=0):
    call("ramnet_gemm", p.a, p.b, p.c, p.M, p.N, p.K, p.lda, p.ldb, p.ldc, int(p.trans), int(p.acc), p.batch, p.sa, p.sb, p.sc, rc=rc)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm(M, N, K, trans, acc):
    """K >= 128 without `accumulate` joins four waves; K = 36, 124, 132, 260, 516 are no multiples of 32 (the rounding of the slice
    length); K = 260 / 516 split the reduction over workgroups under `accumulate`; N = 129 / 161 have more than four 32-column blocks"""
    for batch in (1, 3):
        for pitched in (False, True):
            for kind in ("int", "normal"):
                p = _Problem(M, N, K, trans, acc, batch, pitched, kind, 250)
                _gemm_call(p)
                got = p.check(kind, "gemm[batch=%d, pitched=%d, %s]" % (batch, pitched, kind))
                if not acc:
                    q = _Problem(M, N, K, trans, acc, batch, pitched, kind, 250)
                    _gemm_call(q)
                    assert torch.equal(_bits(got), _bits(q.check(kind, "gemm (second call)"))), "gemm without accumulate is not bit-reproducible"


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("M,M2,K,K2,batch,batch2", [(33, 8, 36, 36, 2, 2), (8, 40, 36, 36, 1, 3), (33, 33, 132, 36, 3, 1), (5, 70, 36, 260, 2, 1), (40, 7, 128, 124, 1, 1)])
def test_gemm2(M, M2, K, K2, batch, batch2, trans, acc):
    """two products in one launch, the grid sized by max(M, M2) and max(K, K2): every C sits between guards and has a sentinel row behind each
    entry's M rows, so that a row written by the other product's blocks shows"""
    N = 40
    for pitched in (False, True):
        for kind in ("int", "normal"):
            lda = (max(M, M2) + (3 if pitched else 0)) if trans else (max(K, K2) + (4 if pitched else 0))      # one leading dimension for both
            p, q = _Problem(M, N, K, trans, acc, batch, pitched, kind, 260, lda), _Problem(M2, N, K2, trans, acc, batch2, pitched, kind, 263, lda)
            call("ramnet_gemm2", p.a, p.b, p.c, M, p.sa, p.sb, p.sc, batch, q.a, q.b, q.c, M2, q.sa, q.sb, q.sc, batch2, N, K, K2, lda, p.ldb, p.ldc,
                 int(trans), int(acc))
            p.check(kind, "gemm2 first product[%s]" % kind)
            q.check(kind, "gemm2 second product[%s]" % kind)


def _gemm_refusals():
    p = _Problem(8, 8, 8, 0, 0, 1, False, "int", 270)
    a1 = In(torch.zeros(9, 8), skew=1)
    return [("ramnet_gemm", p.a, p.b, p.c, 8, 8, 6, 8, 8, 8, 0, 0, 1, 0, 0, 0),            # K % 4
         ("ramnet_gemm", a1, p.b, p.c, 8, 8, 8, 8, 8, 8, 0, 0, 1, 0, 0, 0),             # misaligned A
         ("ramnet_gemm", p.a, p.b, p.c, 8, 8, 8, 4, 8, 8, 0, 0, 1, 0, 0, 0),            # lda < K
         ("ramnet_gemm", p.a, p.b, p.c, 8, 8, 8, 4, 8, 8, 1, 0, 1, 0, 0, 0),            # trans_a: lda < M
         ("ramnet_gemm", p.a, p.b, p.c, 8, 8, 8, 8, 4, 8, 0, 0, 1, 0, 0, 0),            # ldb < N
         ("ramnet_gemm", p.a, p.b, p.c, 8, 8, 8, 8, 8, 4, 0, 0, 1, 0, 0, 0),            # ldc < N
         ("ramnet_gemm", p.a, p.b, p.c, 8, 8, 8, 8, 8, 8, 0, 0, 0, 0, 0, 0),            # batch < 1
         ("ramnet_gemm2", p.a, p.b, p.c, 4, 0, 0, 0, 1, p.a, p.b, p.c, 8, 0, 0, 0, 1, 8, 8, 8, 6, 8, 8, 1, 0),      # trans_a: lda < max(M, M2)
         ("ramnet_gemm2", p.a, p.b, p.c, 8, 0, 0, 0, 1, p.a, p.b, p.c, 8, 0, 0, 0, 0, 8, 8, 8, 8, 8, 8, 0, 0),      # batch2 < 1
         ("ramnet_gemm2", p.a, p.b, p.c, 8, 0, 0, 0, 1, a1, p.b, p.c, 8, 0, 0, 0, 1, 8, 8, 8, 8, 8, 8, 0, 0)]       # misaligned A2


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks():
    """every entry point of the three files with each documented precondition violated once: RAMNET_E_BADARG, the message, outputs untouched.
    All pointers are valid buffers large enough for the nearest accepted call."""
    i, o = In(torch.zeros(64, 64)), Out(64, 64)
    s, so = d64(torch.ones(64)), Out(1, 64, dtype=F64)
    isk, osk = In(torch.zeros(4096), skew=1), Out(1, 4096, skew=1)
    bad = [
        ("ramnet_si_loss_fwd", i, i, 0, 1.0, 1.0, so, o), ("ramnet_si_loss_fwd", None, i, 16, 1.0, 1.0, so, o), ("ramnet_si_loss_fwd", i, i, 16, 1.0, 1.0, None, o),
        ("ramnet_si_loss_fwd", i, i, 16, 1.0, 1.0, so, None),
        ("ramnet_si_log_loss_fwd", i, i, 0, 1.0, so, o), ("ramnet_si_log_loss_fwd", i, None, 16, 1.0, so, o),
        ("ramnet_si_loss_from_stats", None, 1.0, 1.0, o), ("ramnet_si_loss_from_stats", s, 1.0, 1.0, None),
        ("ramnet_si_loss_bwd", i, i, 0, 1.0, 1.0, s, None, o), ("ramnet_si_loss_bwd", i, i, 16, 1.0, 1.0, None, None, o),
        ("ramnet_si_log_loss_bwd", i, i, 0, 1.0, s, None, o), ("ramnet_si_log_loss_bwd", i, i, 16, 1.0, s, None, None),
        ("ramnet_mse_loss_fwd", i, i, 0, 4, 4, 0, so, o), ("ramnet_mse_loss_fwd", i, i, 1, 1, 4, 1, so, o), ("ramnet_mse_loss_fwd", i, i, 1, 4, 1, 1, so, o),
        ("ramnet_mse_loss_fwd", i, i, 1, 4, 0, 0, so, o),
        ("ramnet_mse_loss_bwd", i, i, 1, 1, 4, 1, s, None, o), ("ramnet_mse_loss_bwd", i, i, 1, 4, 1, 1, s, None, o), ("ramnet_mse_loss_bwd", i, i, 1, 0, 4, 0, s, None, o),
        ("ramnet_mse_loss_bwd", i, i, 1, 4, 4, 0, None, None, o),
        ("ramnet_depth_metrics", i, i, 0, 80.0, 3.7, 10.0, so), ("ramnet_depth_metrics", i, i, 16, 0.0, 3.7, 10.0, so), ("ramnet_depth_metrics", i, None, 16, 80.0, 3.7, 10.0, so),
        ("ramnet_msg_loss_fwd", i, i, 0, 8, 8, 1, o, so, o), ("ramnet_msg_loss_fwd", i, i, 1, 8, 8, 5, o, so, o), ("ramnet_msg_loss_fwd", i, i, 1, 8, 8, 0, o, so, o),
        ("ramnet_msg_loss_fwd", i, i, 1, 8, 3, 3, o, so, o),
        ("ramnet_msg_loss_bwd", i, s, None, 0, 8, 8, 1, o, o), ("ramnet_msg_loss_bwd", i, s, None, 1, 8, 8, 5, o, o), ("ramnet_msg_loss_bwd", i, None, None, 1, 8, 8, 1, o, o),
        ("ramnet_normalize_nonzero", o, 0, so), ("ramnet_normalize_nonzero", o, 16, None),
        ("ramnet_normalize_nonzero_batch", o, 2, 6, so), ("ramnet_normalize_nonzero_batch", o, 0, 8, so), ("ramnet_normalize_nonzero_batch", o, 65536, 4, so),
        ("ramnet_normalize_nonzero_batch", osk, 2, 8, so),
        ("ramnet_nonzero_stats_batch", i, 2, 6, so), ("ramnet_nonzero_stats_batch", i, 0, 8, so), ("ramnet_nonzero_stats_batch", isk, 2, 8, so),
        ("ramnet_norm_partial", i, 8, None, 0, 0, i, 8, 1, 4, 8, 0, so), ("ramnet_norm_partial", i, 4, None, 0, 0, i, 8, 1, 4, 8, 1, so),
        ("ramnet_norm_partial", i, 8, None, 0, 0, i, 4, 1, 4, 8, 1, so), ("ramnet_norm_partial", i, 8, i, 4, 1, i, 8, 1, 4, 8, 1, so),
        ("ramnet_norm_partial", i, 8, i, 8, 3, i, 8, 1, 4, 8, 1, so), ("ramnet_norm_partial", i, 8, None, 0, 0, i, 8, 0, 4, 8, 1, so),
        ("ramnet_norm_partial", i, 8, None, 0, 0, i, 8, 1, 0, 8, 1, so), ("ramnet_norm_partial", i, 8, None, 0, 0, i, 8, 1, 4, 0, 1, so),
        ("ramnet_norm_finalize", s, 1, 1, 8, 4, 1e-5, None, None, None, None, 0.1, 0, 0, None, None, so, o, o),
        ("ramnet_norm_finalize", None, 1, 1, 8, 4, 1e-5, None, None, None, None, 0.1, 0, 0, None, so, so, o, o),
        ("ramnet_norm_finalize", s, 1, 0, 8, 4, 1e-5, None, None, None, None, 0.1, 0, 0, None, so, so, o, o),
        ("ramnet_norm_finalize", s, 2, 1, 8, 4, 1e-5, None, None, o, o, 0.1, 0, 1, None, so, so, o, o),
        ("ramnet_norm_finalize", s, 1, 1, 8, 4, 1e-5, None, None, None, None, 0.1, 0, 1, None, so, so, o, o),
        ("ramnet_norm_finalize", s, 1, 1, 8, 1, 1e-5, None, None, o, o, 0.1, 1, 0, None, so, so, o, o),
        ("ramnet_norm_finalize", s, 1, 1, 8, 4, 1e-5, None, None, o, None, 0.1, 1, 0, None, so, so, o, o),
        ("ramnet_norm_finalize", s, 1, 1, 0, 4, 1e-5, None, None, None, None, 0.1, 0, 0, None, so, so, o, o),
        ("ramnet_norm_finalize_bwd", None, 1, 1, 8, 4, s, s, None, 1, o, o, o, None, None), ("ramnet_norm_finalize_bwd", s, 1, 0, 8, 4, s, s, None, 1, o, o, o, None, None),
        ("ramnet_norm_finalize_bwd", s, 1, 1, 8, 4, None, s, None, 1, o, o, o, None, None), ("ramnet_norm_finalize_bwd", s, 1, 1, 8, 4, s, s, None, 1, o, None, o, None, None),
        ("ramnet_norm_finalize_bwd", s, 1, 1, 8, 0, s, s, None, 1, o, o, o, None, None),
        ("ramnet_norm_apply", i, 4, i, i, None, 0, 0, o, 8, 1, 4, 8), ("ramnet_norm_apply", i, 8, i, i, None, 0, 0, o, 4, 1, 4, 8),
        ("ramnet_norm_apply", i, 8, i, i, i, 4, 0, o, 8, 1, 4, 8), ("ramnet_norm_apply", i, 8, i, i, None, 0, 3, o, 8, 1, 4, 8),
        ("ramnet_norm_apply", i, 8, None, i, None, 0, 0, o, 8, 1, 4, 8), ("ramnet_norm_apply", i, 8, i, i, None, 0, 0, o, 8, 1, 0, 8),
        ("ramnet_norm_bwd", i, 4, None, 0, 0, i, 8, i, i, i, o, 8, None, 0, 1, 4, 8), ("ramnet_norm_bwd", i, 8, None, 0, 0, i, 4, i, i, i, o, 8, None, 0, 1, 4, 8),
        ("ramnet_norm_bwd", i, 8, None, 0, 0, i, 8, i, i, i, o, 4, None, 0, 1, 4, 8), ("ramnet_norm_bwd", i, 8, i, 4, 1, i, 8, i, i, i, o, 8, None, 0, 1, 4, 8),
        ("ramnet_norm_bwd", i, 8, None, 0, 1, i, 8, i, i, i, o, 8, None, 0, 1, 4, 8), ("ramnet_norm_bwd", i, 8, None, 0, 0, i, 8, i, i, i, o, 8, o, 4, 1, 4, 8),
        ("ramnet_norm_bwd", i, 8, None, 0, 0, i, 8, i, None, i, o, 8, None, 0, 1, 4, 8), ("ramnet_norm_bwd", i, 8, None, 0, -1, i, 8, i, i, i, o, 8, None, 0, 1, 4, 8),
    ]
    bad += [("ramnet_msg_loss_fwd", i, i, 1, 7, 8, 4, o, so, o), ("ramnet_msg_loss_bwd", i, s, None, 1, 7, 8, 4, o, o)]      # an empty fourth scale
    for args in bad + _gemm_refusals():
        call(*args, rc=BADARG)
