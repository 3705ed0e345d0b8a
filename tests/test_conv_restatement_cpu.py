"""No GPU: anchors tests/conv_restatement.py (the float64 statement of a convolution descriptor that tests/test_hip_conv_launch.py
compares the kernels with) against torch's float64 convolutions and their autograd gradients, the 5x5 stride-2 layer a space-to-depth
launch stands for and the oracle's ConvGRU / ConvLSTM cells; and asserts for every row of tests/conv_launch_cases.py the conditions its
comparison rule relies on (exactness on the float64 side, activation arguments in range, at most 0.1 % of the elements on a kink)."""
import types

import pytest
import torch
import torch.nn.functional as F

import conv_launch_cases as cc
import conv_restatement as cr
from oracle import ramnet_ref

F64 = torch.float64


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def close(a, b, what):
    scale = max(float(b.abs().max()), 1e-30)
    assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * scale, what


def statement(c, fam):
    return cr.conv_statement(cc.build(c), fam)


SMALL = [c for c in cc.CASES if c.H * c.W <= 4096]


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
def test_reduction_against_torch(c):
    """the tap sum of the statement = F.conv2d (forward rows) / F.conv_transpose2d (backward-data rows: the flipped slices) in float64"""
    d = cc.build(c)
    x = nchw(cr.logical_input(d))
    p = c.k // 2
    if c.transposed:
        ref = F.conv_transpose2d(x, d.w_oihw, None, 1, p)
    else:
        ref = F.conv2d(x, d.w_oihw, None, c.stride, p)
    acc, terms = cr.reduction(cr.logical_input(d), d.W, d.taps, d.stride, d.Ho, d.Wo)
    close(acc, nhwc(ref), c.name)
    ones = F.conv2d(torch.ones(1, 1, c.H, c.W, dtype=F64), torch.ones(1, 1, c.k, c.k, dtype=F64), None, c.stride, p)[0, 0]
    assert torch.equal(terms, ones * d.Cin)
    if c.k == 3 and c.stride == 1:                  # the matrices of both Winograd families reproduce the tap sum
        for fam in ("2x2", "2x4"):
            close(cr.wino_abs(cr.logical_input(d), d.W, d.taps, d.Ho, d.Wo, fam, absolute=False), acc, (c.name, fam))
            assert bool((cr.wino_abs(cr.logical_input(d, True), d.W.abs(), d.taps, d.Ho, d.Wo, fam) >= acc.abs() * (1 - 1e-12)).all())


def test_space_to_depth_is_the_5x5_stride2_layer():
    g = torch.Generator().manual_seed(5)
    B, H, W, C, N = 2, 6, 10, 8, 12
    x = torch.randn(B, 2 * H, 2 * W, C, generator=g, dtype=F64)
    w5 = torch.randn(N, C, 5, 5, generator=g, dtype=F64)
    w3 = cc.s2d_weights(w5)
    d = types.SimpleNamespace(in_mode=cr.IN_S2D, x0=x)
    taps = [(a - 1, b - 1, a * 3 + b) for a in range(3) for b in range(3)]
    acc, _ = cr.reduction(cr.logical_input(d), w3.permute(2, 3, 1, 0).reshape(9, 4 * C, N), taps, 1, H, W)
    close(acc, nhwc(F.conv2d(nchw(x), w5, None, 2, 2)), "s2d")
    # 11 of the 36 (tap, parity group) slices are zero, the ones ramnet_conv_desc.s2d_5x5 names
    zero = (w3.view(N, 4, C, 3, 3).abs().sum((0, 2)) == 0)
    assert int(zero.sum()) == 11 and bool(zero[2:, 2, :].all()) and bool(zero[1::2, :, 2].all())
    # out_s2d: the adjoint view
    dy = torch.randn(B, H, W, N, generator=g, dtype=F64)
    xr = x.clone().requires_grad_(True)
    (nhwc(F.conv2d(nchw(xr), w5, None, 2, 2)) * dy).sum().backward()
    dd = types.SimpleNamespace(in_mode=cr.IN_PLAIN, x0=dy, W=w3.permute(2, 3, 0, 1).reshape(9, N, 4 * C).contiguous(),
                               taps=[(a - 1, b - 1, (2 - a) * 3 + (2 - b)) for a in range(3) for b in range(3)], stride=1, Ho=H, Wo=W,
                               HoF=2 * H, WoF=2 * W, os=(1, 1, 0, 0), bias=None, beta=0.0, epi=cr.EPI_LINEAR, active=None, out_s2d=C,
                               Cout=4 * C, e0=None, e1=None, out_old=None)
    close(cr.conv_statement(dd).out, xr.grad, "out_s2d")


def _desc(x0, w, bias, epi, **kw):
    N, Cin = w.shape[:2]
    B, H, W, _ = x0.shape
    d = dict(in_mode=cr.IN_PLAIN, x0=x0, x1=None, xm=None, W=w.permute(2, 3, 1, 0).reshape(9, Cin, N).contiguous(),
             taps=[(a - 1, b - 1, a * 3 + b) for a in range(3) for b in range(3)], stride=1, Ho=H, Wo=W, HoF=H, WoF=W, os=(1, 1, 0, 0),
             bias=bias, beta=0.0, epi=epi, active=None, out_s2d=0, Cout=N, e0=None, e1=None, out_old=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_gru_chain_and_lstm_cell_against_the_oracle():
    g = torch.Generator().manual_seed(7)
    B, H, W, C = 2, 5, 7, 8
    x, h = torch.randn(B, H, W, C, generator=g, dtype=F64), torch.randn(B, H, W, C, generator=g, dtype=F64)
    sd = {"g.%s.%s" % (n, k): torch.randn(*s, generator=g, dtype=F64) * 0.2 for n in ("update_gate", "reset_gate", "out_gate")
          for k, s in (("weight", (C, 2 * C, 3, 3)), ("bias", (C,)))}
    ref = nhwc(ramnet_ref.conv_gru(sd, "g", nchw(x), nchw(h)))
    # launch 1: [u | r] = sigmoid, h.r on the side; launch 2: candidate over the plain concatenation [x | h.r], blended with u out of [u | r]
    wur = torch.cat([sd["g.update_gate.weight"], sd["g.reset_gate.weight"]], 0)
    bur = torch.cat([sd["g.update_gate.bias"], sd["g.reset_gate.bias"]], 0)
    s1 = cr.conv_statement(_desc(x, wur, bur, cr.EPI_SIGMOID_HR, in_mode=cr.IN_CAT, x1=h, Cout=2 * C, e1=h))
    s2 = cr.conv_statement(_desc(x, sd["g.out_gate.weight"], sd["g.out_gate.bias"], cr.EPI_GRU_BLEND, in_mode=cr.IN_CAT, x1=s1.o1,
                                 e0=s1.out[..., :C], e1=h))
    close(s2.out, ref, "gru")
    # the same candidate with the product formed by the loader (CAT_MUL) from r
    s3 = cr.conv_statement(_desc(x, sd["g.out_gate.weight"], sd["g.out_gate.bias"], cr.EPI_GRU_BLEND, in_mode=cr.IN_CAT_MUL, x1=h,
                                 xm=s1.out[..., C:], e0=s1.out[..., :C], e1=h))
    close(s3.out, ref, "gru, CAT_MUL")
    # launch 3 (backward): GRU_BWD on the candidate's backward-data against autograd
    xr, hr = x.clone().requires_grad_(True), h.clone().requires_grad_(True)
    u, r = s1.out[..., :C], s1.out[..., C:]
    o_pre = nhwc(F.conv2d(nchw(torch.cat([xr, hr * r], 3)), sd["g.out_gate.weight"], sd["g.out_gate.bias"], 1, 1))
    dpo = torch.randn(B, H, W, C, generator=g, dtype=F64)
    (o_pre * dpo).sum().backward()                  # r held constant: hr.grad = d(h.r) * r
    wo = sd["g.out_gate.weight"]
    old = torch.randn(B, H, W, 2 * C, generator=g, dtype=F64)
    db = types.SimpleNamespace(**vars(_desc(dpo, wo, None, cr.EPI_GRU_BWD, Cout=2 * C, e0=s1.out, e1=h, out_old=old)))
    db.W = wo.permute(2, 3, 0, 1).reshape(9, C, 2 * C).contiguous()
    db.taps = [(a - 1, b - 1, (2 - a) * 3 + (2 - b)) for a in range(3) for b in range(3)]
    s4 = cr.conv_statement(db)
    close(s4.out[..., :C], xr.grad, "gru_bwd dx")
    close(s4.out[..., C:], old[..., C:] + hr.grad, "gru_bwd dh")
    ghr = hr.grad / r
    close(s4.o1[..., C:], ghr * h * r * (1 - r), "gru_bwd dpr")
    assert not bool(s4.w_o1[..., :C].any()) and bool(s4.w_o1[..., C:].all())
    # ConvLSTM cell
    c0 = torch.randn(B, H, W, C, generator=g, dtype=F64)
    sdl = {"l.Gates.weight": torch.randn(4 * C, 2 * C, 3, 3, generator=g, dtype=F64) * 0.2, "l.Gates.bias": torch.randn(4 * C, generator=g, dtype=F64)}
    hn, cn = ramnet_ref.conv_lstm(sdl, "l", nchw(x), (nchw(h), nchw(c0)))
    dl = _desc(x, sdl["l.Gates.weight"], sdl["l.Gates.bias"], cr.EPI_LSTM, in_mode=cr.IN_CAT, x1=h, Cout=C, e1=c0)
    sl = cr.conv_statement(dl)
    close(sl.out, nhwc(hn), "lstm h")
    close(sl.o1, nhwc(cn), "lstm c")
    assert sl.o2.shape[3] == 4 * C
    # active = all ones equals no mask; a zero passes the state through and zeroes what the backward reads
    dl.e0 = h
    dl.active = torch.ones(B, dtype=torch.int32)
    sm = cr.conv_statement(dl)
    assert torch.equal(sm.out, sl.out) and torch.equal(sm.o1, sl.o1) and torch.equal(sm.o2, sl.o2) and torch.equal(sm.b_out, sl.b_out)
    dl.active = torch.tensor([1, 0], dtype=torch.int32)
    sm = cr.conv_statement(dl)
    assert torch.equal(sm.out[1], h[1]) and torch.equal(sm.o1[1], c0[1]) and not bool(sm.o2[1].any()) and torch.equal(sm.out[0], sl.out[0])
    assert not bool(sm.b_out[1].any()) and not bool(sm.b_o1[1].any())


def test_wgrad_statement_against_autograd():
    g = torch.Generator().manual_seed(9)
    for k, stride, B, H, W, C0, C1, N in ((3, 1, 2, 5, 7, 4, 0, 8), (5, 2, 3, 9, 11, 4, 4, 12), (3, 2, 1, 1, 1, 4, 0, 4)):
        p = k // 2
        x0 = torch.randn(B, H, W, C0, generator=g, dtype=F64)
        x1 = torch.randn(B, H, W, C1, generator=g, dtype=F64) if C1 else None
        Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
        dout, gm = torch.randn(B, Ho, Wo, N, generator=g, dtype=F64), torch.randn(B, Ho, Wo, N, generator=g, dtype=F64)
        w = torch.zeros(N, C0 + C1, k, k, dtype=F64, requires_grad=True)
        b = torch.zeros(N, dtype=F64, requires_grad=True)
        xin = x0 if x1 is None else torch.cat([x0, x1], 3)
        (nhwc(F.conv2d(nchw(xin), w, b, stride, p)) * dout * (gm > 0)).sum().backward()
        d = types.SimpleNamespace(in_mode=cr.IN_CAT if C1 else cr.IN_PLAIN, x0=x0, x1=x1, xm=None, dout=dout, gmask=gm, stride=stride, Ho=Ho, Wo=Wo,
                                  taps=[(a - p, c - p) for a in range(k) for c in range(k)])
        s = cr.wgrad_statement(d)
        close(s.dW, w.grad.permute(2, 3, 1, 0).reshape(k * k, C0 + C1, N), "dW")
        close(s.dbias, b.grad, "dbias")
        assert bool((s.dW_abs >= s.dW.abs() * (1 - 1e-12)).all())
        if k == 3 and stride == 1:                 # the transformed-domain form of both Winograd families is the same gradient
            for fam in ("2x2", "2x4"):
                close(cr.wgrad_wino(d, fam, absolute=False)[0], s.dW, ("wgrad_wino", fam))
                assert bool((cr.wgrad_wino(d, fam)[0] >= s.dW.abs() * (1 - 1e-12)).all())
        two = types.SimpleNamespace(**vars(d))
        two.segs = [d, d]
        close(cr.wgrad_statement(two).dW, 2 * s.dW, "segments add up")
        old = torch.randn(N - 4, C0, k, k, generator=g, dtype=F64) if N > 4 else torch.randn(N, C0, k, k, generator=g, dtype=F64)
        n_off = 4 if N > 4 else 0
        got = cr.unpack_statement(old, s.dW, old.shape[0], C0, n_off)
        close(got, old + w.grad[n_off:n_off + old.shape[0], :C0], "unpack window")


@pytest.mark.parametrize("c", cc.CASES, ids=lambda c: c.name)
def test_case_can_be_judged(c):
    """what the GPU rules rely on, per row and family, from the statement alone"""
    d = cc.build(c)
    for t in (d.x0, d.x1, d.xm, d.w_oihw, d.bias, d.e0, d.e1, d.out_old):
        assert t is None or torch.equal(t, t.float().to(F64)), "operands must be fp32 numbers"
    assert d.W.numel() * 8 + d.x0.numel() * 8 + c.B * d.HoF * d.WoF * d.N * 8 < 2 * (64 << 20), "a case stays within a few tens of megabytes in fp32: the 128 x 128 tile needs 98 304 pixels x 128 channels = 48 MB (this sum is of float64 copies)"
    for fam in c.fams:
        st = statement(c, fam)
        if c.kind == "int":
            assert c.epi not in cc.CELL_EPIS
            assert cr.exact_ok(st, fam), "%s on %s is not exact in fp32: abs statement %.0f" % (c.name, fam, float(st.pre_abs.max()))
        else:
            assert st.sig_arg <= cr.SIG_RANGE and st.tanh_arg <= cr.TANH_RANGE
            assert bool(torch.isfinite(st.b_out).all()) and bool((st.b_out[st.w_out] >= 0).all())
            assert int(st.kink.sum()) <= 1e-3 * int(st.w_out.sum()), "more than 0.1 % of the elements on a kink"
        assert bool(st.w_out.all())


@pytest.mark.parametrize("i", range(len(cc.WGRAD_ROWS)))
def test_wgrad_row_can_be_judged(i):
    d = cc.build_wgrad(i)
    st = cr.wgrad_statement(d)
    for fam in ("2x2", "2x4"):
        a, n = cr.wgrad_wino(d, fam)
        if cc.WGRAD_ROWS[i][9] == "int":
            assert float(a.max()) * 16 < 2 ** 24 and torch.equal(st.dW, st.dW.round())
        assert bool((a >= st.dW.abs() * (1 - 1e-12)).all()) and n > 0


def test_coherent_row_separates_the_third_term():
    c, d = cc.build_coherent()
    st = cr.conv_statement(d, "2x4split")
    lost = 16 * 57 * 2.0 ** -23
    assert abs(float(st.out[0, 0, 0, 0]) - 16 * cc.COHERENT_V) < 1e-5
    assert lost > 3 * float(st.b_out[0, 0, 0, 0]) and lost < 2e-5 * float(st.out.abs().max())
