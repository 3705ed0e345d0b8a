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


# ================================================================================================ head, folded decoders, UP2X loaders
import fold_head_cases as fh                        # noqa: E402


def _layer(seed, B, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(seed)
    x, skip = torch.randn(B, H, W, Cin, generator=g, dtype=F64), torch.randn(B, H, W, Cin, generator=g, dtype=F64)
    return x, skip, torch.randn(Cout, Cin, 5, 5, generator=g, dtype=F64), torch.randn(Cout, generator=g, dtype=F64)


def test_up2x_is_bilinear_align_corners_false():
    x = torch.randn(2, 5, 7, 3, generator=torch.Generator().manual_seed(3), dtype=F64)
    close(cr.up2x(x), nhwc(F.interpolate(nchw(x), scale_factor=2, mode="bilinear", align_corners=False)), "up2x")
    d = types.SimpleNamespace(in_mode=cr.IN_UP2X_SKIP, x0=x, x1=2 * x)
    close(cr.logical_input(d), 3 * cr.up2x(x), "UP2X_SKIP")


@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (6, 4)])
def test_fold_with_frame_is_the_layer_on_the_whole_image(H, W):
    """fold_statement on pad2(x + skip) with the frame operands of border_operands = relu(conv5x5, zero-padded, of up2x(x + skip) + b) on
    EVERY pixel; without the frame the interior alone agrees; frame operands of zero equal no frame; both families and the pair tiling
    reproduce the class tap sums with their signed matrices"""
    B, Cin, Cout = 2, 3, 4
    x, skip, w, b = _layer(H * 10 + W, B, H, W, Cin, Cout)
    ref = nhwc(F.conv2d(F.interpolate(nchw(x + skip), scale_factor=2, mode="bilinear", align_corners=False), w, b, 1, 2)).clamp_min(0)
    e0, e1 = cr.border_operands(x + skip, w)
    d = types.SimpleNamespace(x0=cr.pad2(x + skip), w5=w, bias=b, epi=cr.EPI_RELU, frame=2, e0=e0, e1=e1, Ho=H, Wo=W, HoF=2 * H, WoF=2 * W, Cout=Cout)
    for fam in ("fold2x2", "fold2x3"):
        st = cr.fold_statement(d, fam)
        close(st.out, ref, fam)
        assert bool((st.pre_abs >= st.pre.abs() * (1 - 1e-12)).all())
    bare = types.SimpleNamespace(**dict(vars(d), frame=0, e0=None, e1=None))
    zero = types.SimpleNamespace(**dict(vars(d), e0=torch.zeros_like(e0), e1=torch.zeros_like(e1)))
    s0, sz = cr.fold_statement(bare, "fold2x2"), cr.fold_statement(zero, "fold2x2")
    assert torch.equal(s0.out, sz.out) and torch.equal(s0.pre_abs, sz.pre_abs)
    if H > 2 and W > 2:
        close(s0.out[:, 2:-2, 2:-2], ref[:, 2:-2, 2:-2], "interior without the frame")
        assert float((s0.out - ref).abs().max()) > 1e-3
    W4 = cr.fold_w4(w)
    for py in range(2):
        for px in range(2):
            Wc = W4[:, :, py, px].permute(2, 3, 1, 0).reshape(16, Cin, Cout)
            acc, _ = cr.reduction(d.x0, Wc, cr.fold_taps(py, px), 1, H, W)
            for fam in ("fold2x2", "fold2x3"):
                for shift in (0, 1) if px == 1 else (0,):
                    close(cr.fold_wino(d.x0, Wc, py, px, H, W, fam, shift=shift, absolute=False), acc, (fam, py, px, shift))


def test_frame_on_the_direct_statement():
    """the four parity classes as direct sub-grid descriptors with frame = 2 (the folded_direct path) give the same image"""
    B, H, W, Cin, Cout = 1, 3, 4, 2, 3
    x, skip, w, b = _layer(11, B, H, W, Cin, Cout)
    e0, e1 = cr.border_operands(x + skip, w)
    ref = nhwc(F.conv2d(F.interpolate(nchw(x + skip), scale_factor=2, mode="bilinear", align_corners=False), w, b, 1, 2))
    W4 = cr.fold_w4(w)
    out = torch.zeros_like(ref)
    for py in range(2):
        for px in range(2):
            d = types.SimpleNamespace(in_mode=cr.IN_PLAIN, x0=cr.pad2(x + skip), W=W4[:, :, py, px].permute(2, 3, 1, 0).reshape(16, Cin, Cout),
                                      taps=cr.fold_taps(py, px), stride=1, Ho=H, Wo=W, HoF=2 * H, WoF=2 * W, os=(2, 2, py, px), bias=b, epi=cr.EPI_LINEAR,
                                      beta=0.0, e0=e0, e1=e1, frame=2, out_old=None, active=None, out_s2d=0, Cout=Cout)
            st = cr.conv_statement(d)
            out = out + st.out * st.w_out
    close(out, ref, "direct classes with frame")


def test_parity4_is_the_gradient_of_the_fold():
    B, H, W, Cin, Cout = 2, 3, 4, 3, 2
    g = torch.Generator().manual_seed(9)
    xpad = torch.randn(B, H + 4, W + 4, Cin, generator=g, dtype=F64, requires_grad=True)
    w, gy = torch.randn(Cout, Cin, 5, 5, generator=g, dtype=F64), torch.randn(B, 2 * H, 2 * W, Cout, generator=g, dtype=F64)
    W4 = cr.fold_w4(w)
    out = torch.zeros(B, 2 * H, 2 * W, Cout, dtype=F64)
    for py in range(2):
        for px in range(2):
            out[:, py::2, px::2] = nhwc(F.conv2d(nchw(xpad)[:, :, py:py + H + 3, px:px + W + 3], W4[:, :, py, px]))
    (out * gy).sum().backward()
    taps, Wt = cr.parity4_taps_weights(w)
    d = types.SimpleNamespace(in_mode=cr.IN_PARITY4, x0=gy)
    acc, _ = cr.reduction(cr.logical_input(d), Wt, taps, 1, H + 4, W + 4)
    close(acc, xpad.grad, "PARITY4")
    for fam in ("fold2x2", "fold2x3"):
        close(cr.parity4_wino(gy, w, fam, absolute=False), acc, fam)
        assert bool((cr.parity4_wino(gy, w, fam) >= acc.abs() * (1 - 1e-12)).all())


def test_fold_backward_weights_against_autograd():
    """fold_wgrad_statement + fold_unpack_statement = the autograd gradient of the 5x5 weights through the four parity convolutions (mask
    and bias included); both transformed-domain forms fold back to the same dW4; HEAD and the sub-grid form of DIRECT are wgrad_statement on
    their tap lists, which test_wgrad_statement_against_autograd anchors"""
    g = torch.Generator().manual_seed(1)
    B, H, W, C, N = 2, 3, 5, 3, 2
    xpad = torch.randn(B, H + 4, W + 4, C, generator=g, dtype=F64)
    w = torch.zeros(N, C, 5, 5, dtype=F64, requires_grad=True)
    b = torch.zeros(N, dtype=F64, requires_grad=True)
    dout, gm = torch.randn(B, 2 * H, 2 * W, N, generator=g, dtype=F64), torch.randn(B, 2 * H, 2 * W, N, generator=g, dtype=F64)
    W4 = cr.fold_w4(w)
    out = torch.zeros(B, 2 * H, 2 * W, N, dtype=F64)
    for py in range(2):
        for px in range(2):
            out[:, py::2, px::2] = nhwc(F.conv2d(nchw(xpad)[:, :, py:py + H + 3, px:px + W + 3], W4[:, :, py, px], b))
    (out * dout * (gm > 0)).sum().backward()
    d = types.SimpleNamespace(x0=xpad, dout=dout, gmask=gm, Ho=H, Wo=W)
    st = cr.fold_wgrad_statement(d)
    old = torch.randn(N, C, 5, 5, generator=g, dtype=F64)
    w4, wr = torch.randn(4, 16, C, N, generator=g, dtype=F64), torch.randn(2, 5 * C, 2 * N, generator=g, dtype=F64)
    close(cr.fold_unpack_statement(old, st.dW4, torch.zeros_like(w4), torch.zeros_like(wr), torch.zeros_like(wr)), old + w.grad, "dW5")
    close(st.dbias, b.grad, "dbias")
    import torch_restatements as tr
    ref = tr.fold_unpack_torch(w4.float().reshape(-1), None, wr.float(), (2 * wr).float(), N, C, C)      # (the fp32 restatement of the product path)
    got = cr.fold_unpack_statement(torch.zeros_like(old), torch.zeros_like(w4), w4, wr, 2 * wr)
    assert float((got - ref.to(F64)).abs().max()) < 1e-5 * float(got.abs().max()), "direct and border workspaces"
    for fam in ("fold2x2", "fold2x3"):
        dU, folded, n = cr.fold_wgrad_wino(d, fam, absolute=False)
        close(folded, st.dW4, fam)
        assert bool((cr.fold_wgrad_wino(d, fam)[1] >= st.dW4.abs() * (1 - 1e-12)).all()) and n == B * 2 * -(-W // cr.FOLD_TW[fam])


def test_pack_statements_are_the_rounding_of_the_rational():
    """fold_u through the integer matrices = G W4 Gc^T with the fractions of the header; on the exact rule's weights (9 x integers) it is a
    multiple of 2^-6 (F(2x2)) / 2^-5 (F(2x3)) with few bits: an fp32 number; the layouts against the header's index formula by hand"""
    import torch_restatements as tr
    import test_fold_wino2x3_cpu as t23
    w = fh.pack_weights(32, 32, "normal")
    close(cr.fold_u(w, 2).reshape(4, 25, 32, 32), tr.fold_weights_wino(w), "fold_u 2x2")
    close(cr.fold_u(w, 3).reshape(4, 30, 32, 32), t23.fold_weights_wino2x3(w), "fold_u 2x3")
    close(cr.fold_w4(w), tr.fold_weights(w), "W4")
    for Cout, Cin in fh.PACK_SHAPES:
        wi = fh.pack_weights(Cout, Cin, "int")
        for tw, k in ((2, 6), (3, 5)):
            u = cr.fold_u(wi, tw) * 2 ** k
            assert torch.equal(u, u.round()) and float(u.abs().max()) < 2 ** 24
            assert bool((cr.fold_u_abs(wi, tw) >= cr.fold_u(wi, tw).abs() * (1 - 1e-12)).all())
    # one element of each layout by the header's formula, written out
    w = fh.pack_weights(64, 32, "normal")
    U = cr.fold_u(w, 2).reshape(4, 25, 32, 64)
    p = cr.pack_fold_statement(w, 2)
    cls, pos, k, n, KC, NCQ = 3, 17, 21, 45, 16, 4
    i = ((((cls * (32 // KC) + k // KC) * (64 // (16 * NCQ)) + n // (16 * NCQ)) * 25 + pos) * NCQ + (n % (16 * NCQ)) // 16) * 16 * KC + (((k % KC) // (KC // 4)) * 16 + n % 16) * (KC // 4) + k % (KC // 4)
    assert float(p[i]) == float(U[cls, pos, k, n])
    assert torch.equal(torch.sort(p.abs())[0], torch.sort(U.reshape(-1).abs())[0])          # a permutation
    w = fh.pack_weights(32, 32, "normal")
    for pair in (False, True):
        for tw in (2, 3):
            p, U = cr.pack_fold_statement(w, tw, pair=pair), cr.fold_u(w, tw)
            assert torch.equal(torch.sort(p.abs())[0], torch.sort(U.reshape(-1).abs())[0])
    w = fh.pack_weights(32, 64, "normal")
    for tw in (2, 3):
        p, U = cr.pack_fold_dgrad_statement(w, tw), cr.fold_u(w, tw, dgrad=True)
        assert torch.equal(torch.sort(p.abs())[0], torch.sort(U.reshape(-1).abs())[0])
    rows, cols, rows_t, cols_t = cr.border_statement(w)
    r2, c2 = tr.border_matrices(w)
    assert torch.equal(rows, r2) and torch.equal(cols, c2) and torch.equal(rows_t, rows.transpose(1, 2))


@pytest.mark.parametrize("c", fh.FOLD, ids=lambda c: c.name)
def test_fold_row_can_be_judged(c):
    d = fh.build_fold(c)
    for t in (d.x0, d.w5, d.bias, d.e0, d.e1):
        assert t is None or torch.equal(t, t.float().to(F64))
    st = cr.fold_statement(d, c.fam, pair=fh.is_pair(c))
    if c.kind == "int":
        assert cr.fold_exact_ok(st, c.fam), "%s is not exact in fp32: abs statement x 2^%d = %.3f x 2^24" % (
            c.name, cr.GRID_BITS[c.fam], float(st.pre_abs.max()) * 2.0 ** (cr.GRID_BITS[c.fam] - 24))
        u = cr.fold_u(d.w5, cr.FOLD_TW[c.fam])
        assert torch.equal(u, u.float().to(F64)), "the transformed weights must be fp32 numbers"
    else:
        assert bool(torch.isfinite(st.b_out).all()) and int(st.kink.sum()) <= 1e-3 * st.kink.numel(), "more than 0.1 % of the elements on a kink"
    assert bool((st.pre_abs >= st.pre.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("c", fh.HEAD + [fh.HEAD_BIG], ids=lambda c: c.name)
def test_head_row_can_be_judged(c):
    d = fh.build_head(c)
    if c is not fh.HEAD_BIG:
        st = cr.conv_statement(d, "direct")
        if c.kind == "int":
            assert cr.exact_ok(st, "direct")
        else:
            assert int(st.kink.sum()) <= 1e-3 * st.kink.numel()
    if c.kind == "int":
        wg = cr.wgrad_statement(types.SimpleNamespace(**dict(vars(d), taps=[t[:2] for t in d.taps])))
        assert float(wg.dW_abs.max()) * 16 < 2 ** 24 and float(wg.dbias_abs.max()) * 16 < 2 ** 24
