"""GPU: every point-wise and glue entry point of csrc/pointwise.hip, called directly through the C ABI with raw pointers, against its
own float64 statement (tests/pointwise_restatement.py; anchored on the CPU by tests/test_pointwise_restatement_cpu.py).

Every launch goes through `call`: outputs live between sentinel guards (and sentinel gaps when pitched) that must come back untouched,
pitched inputs carry NaN in their gaps and guards, `+=` outputs start from non-zero values.  Comparison rules, per test:
  bit        data movement, selection, a single fp32 add: the fp32 rounding of the float64 statement, bit for bit;
  exact      integer-valued data: every intermediate is a multiple of 1/16 below 2^24, fp32 is exact whatever the order of summation;
  derived    (roundings of the documented expression + 1) x 2^-24 x the expression on absolute values, (n + 2) x 2^-24 x sum |term| for sums;
  measured   the derived bound + 4 x the measured error of the v_exp_f32 / v_rcp_f32 sigmoid / tanh x the expression's sensitivity to it
             (SIGMOID_ERR, TANH_ERR: profiles/pointwise_tests_notes.md; test_intrinsic_errors repeats the measurement)."""
import ctypes as C

import pytest
import torch

import pointwise_restatement as pr
from guarded import (BADARG, F64, SIG_RANGE, SIGMOID_ERR, TANH_ERR, TANH_RANGE, TRIP2, U, In, Out, _bits, _dev, assert_bits, assert_exact,
                     assert_within, call, rn, ri)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ flat maps
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 4 * TRIP2 + 3])
def test_relu_bwd_and_add_tails_and_second_trip(n):
    dy, y = rn(n, seed=1), rn(n, seed=2)
    y[::5] = 0.0
    y[1::7] = -0.0
    dx = Out(1, n)
    call("ramnet_relu_bwd", In(dy), In(y), dx, n)
    assert_bits(dx.value(), pr.relu_bwd(dy, y), "relu_bwd")
    a, b, s = rn(n, seed=3), rn(n, seed=4, scale=3.0), Out(1, n)
    call("ramnet_add", In(a), In(b), s, n)
    assert_bits(s.value(), pr.add(a, b), "add")


@pytest.mark.parametrize("Ca,Cb,npix,pa,pb", [(4, 4, 1, 0, 0), (8, 4, 91, 4, 4), (4, 36, 91, 0, 4), (32, 32, 333, 32, 4), (12, 8, 5, 8, 0),
                                               (4, 4, (TRIP2 + 1) // 2, 0, 0)])
def test_concat2_split2(Ca, Cb, npix, pa, pb):
    a, b = rn(npix, Ca, seed=5), rn(npix, Cb, seed=6)
    y = Out(npix, Ca + Cb)
    call("ramnet_concat2", In(a, Ca + pa), Ca + pa, Ca, In(b, Cb + pb), Cb + pb, Cb, y, npix)
    assert_bits(y.value(), pr.concat2(a, b), "concat2")
    src = rn(npix, Ca + Cb, seed=7)
    ra, rb = pr.split2(src, Ca, Cb)
    oa, ob = Out(npix, Ca), Out(npix, Cb)
    call("ramnet_split2", In(src, Ca + Cb + pa), Ca + Cb + pa, Ca, Cb, oa, ob, npix)
    assert_bits(oa.value(), ra, "split2 a")
    assert_bits(ob.value(), rb, "split2 b")


# ------------------------------------------------------------------------------------------------ layout maps
@pytest.mark.parametrize("B,Cc,H,W,Cpad", [(2, 5, 3, 7, 8), (1, 8, 4, 4, 8), (3, 1, 5, 5, 4), (1, 2, 1, 1, 12), (1, 1, 725, 725, 4)])
def test_nchw_to_nhwc_pad(B, Cc, H, W, Cpad):
    src = rn(B, Cc, H, W, seed=8)
    dst = Out(B * H * W, Cpad)
    call("ramnet_nchw_to_nhwc_pad", In(src.reshape(1, -1)), dst, B, Cc, H, W, Cpad)
    assert_bits(dst.value(), pr.nchw_to_nhwc_pad(src, Cpad), "nchw_to_nhwc_pad")


@pytest.mark.parametrize("nhwc", [0, 1])
@pytest.mark.parametrize("H,W,Cc,B", [(260, 346, 5, 2), (5, 7, 5, 2), (5, 7, 1, 1), (5, 7, 8, 1), (260, 346, 1, 1)])
def test_reflect_pad(H, W, Cc, B, nhwc):
    Hc, Wc, top, _, left, _ = pr.crop_parameters(H, W, 3)
    assert (Hc, Wc) == ((264, 352) if H == 260 else (8, 8))
    Cpad = (Cc + 3) // 4 * 4
    src = rn(B, Cc, H, W, seed=9)
    dst = Out(B * Hc * Wc, Cpad) if nhwc else Out(1, B * Cc * Hc * Wc)
    call("ramnet_reflect_pad", In(src.reshape(1, -1)), dst, B, Cc, H, W, Cpad, top, left, Hc, Wc, nhwc)
    assert_bits(dst.value(), pr.reflect_pad(src, top, left, Hc, Wc, Cpad, nhwc), "reflect_pad")


@pytest.mark.parametrize("B,H,W,Cc", [(1, 2, 2, 4), (2, 6, 10, 12), (1, 2, 2 * ((TRIP2 + 7) // 8), 8)])
def test_space_to_depth2_both_ways(B, H, W, Cc):
    x = rn(B, H, W, Cc, seed=10)
    deep = Out(B * H * W // 4, 4 * Cc)
    call("ramnet_space_to_depth2", In(x), deep, B, H, W, Cc, 0)
    ref = pr.space_to_depth2(x)
    assert_bits(deep.value(), ref, "space_to_depth2")
    back = Out(B * H * W, Cc)
    call("ramnet_space_to_depth2", In(ref), back, B, H, W, Cc, 1)
    assert_bits(back.value(), x, "space_to_depth2 inverse")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Cc", [4, 36])
@pytest.mark.parametrize("H2,W2", [(4, 4), (4, 10), (10, 22)])
def test_frame_gather(H2, W2, Cc, masked):
    B = 2
    dy = rn(B, H2, W2, Cc, seed=11)
    mask = rn(B, H2, W2, Cc, seed=12) if masked else None
    if masked:
        mask[..., ::3] = 0.0
    rows, cols = Out(2 * B * W2 * 2, Cc), Out(2 * B * H2 * 2, Cc)
    call("ramnet_frame_gather", In(dy), In(mask) if masked else None, rows, cols, B, H2, W2, Cc)
    rr, rc = pr.frame_gather(dy, mask)
    assert_bits(rows.value(), rr, "frame_gather rows")
    assert_bits(cols.value(), rc, "frame_gather cols")


# ------------------------------------------------------------------------------------------------ bias gradient
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("npix", [1, 5376 + 11])
@pytest.mark.parametrize("Cc", [4, 48, 64, 1024])
def test_bias_grad_exact(Cc, npix, masked):
    """C = 48 leaves 256 % 12 = 4 threads of every workgroup idle; 5376 = 256 workgroups x 21 rows is one trip at that C"""
    dy, db0 = ri(npix, Cc, seed=13, m=64), ri(Cc, seed=14, m=64)
    mask = ri(npix, Cc, seed=15, m=2) if masked else None
    db = Out(1, Cc, prefill=db0)
    call("ramnet_bias_grad", In(dy), In(mask) if masked else None, db, npix, Cc)
    assert_exact(db.value(), pr.bias_grad(dy, mask, db0), "bias_grad", abs_sum=pr.bias_grad(dy.abs(), mask, db0.abs()))


# ------------------------------------------------------------------------------------------------ prediction head
@pytest.mark.parametrize("sig", [False, True])
@pytest.mark.parametrize("npix,Cc,pad,bias", [(480, 32, 0, True), (91, 4, 4, False), (333, 36, 4, True), (257, 128, 8, True), (1, 8, 0, True),
                                              (65536 + 37, 32, 0, True)])
def test_pred_fwd(npix, Cc, pad, bias, sig):
    x, w = rn(npix, Cc, seed=16), rn(Cc, seed=17, scale=0.5)
    b = rn(1, seed=18) if bias else None
    y = Out(1, npix)
    call("ramnet_pred_sigmoid_fwd" if sig else "ramnet_pred_linear_fwd", In(x, Cc + pad), Cc + pad, Cc, In(w), In(b) if bias else None, y, npix)
    ref = pr.pred_fwd(x, w, b[0] if bias else None, sigmoid=sig)
    # z: a sum of C products and the bias, n = C + 1 terms
    zb = (Cc + 1 + 2) * U * (x.abs() @ w.abs() + (b.abs()[0] if bias else 0))
    if not sig:
        assert_within(y.value(), ref, zb, "pred_linear_fwd")
        return
    z = pr.pred_fwd(x, w, b[0] if bias else None, sigmoid=False)
    assert float(z.abs().max()) + float(zb.max()) <= SIG_RANGE
    # sigma is 1/4-Lipschitz: the rounding of z reaches y through at most 0.25; the intrinsic's own error is measured
    assert_within(y.value(), ref, 0.25 * zb + 4 * SIGMOID_ERR, "pred_sigmoid_fwd")


PRED_BWD_CASES = [(npix, Cc) for npix in (480, 2 * 16384 + 3, 65536 + 16384 + 5) for Cc in (4, 32, 36, 128)]


def _pred_bwd_call(sig, npix, Cc, x, w, y, dy, dw0, db0, ldx, lddx, want_dx, want_db):
    dx = Out(npix, Cc, ld=lddx) if want_dx else None
    dw = Out(1, Cc, prefill=dw0)
    db = Out(1, 1, prefill=db0) if want_db else None
    if sig:
        call("ramnet_pred_sigmoid_bwd", In(x, ldx), ldx, Cc, In(w), In(y), In(dy), dx, lddx if want_dx else 0, dw, db, npix)
    else:
        call("ramnet_pred_linear_bwd", In(x, ldx), ldx, Cc, In(w), In(dy), dx, lddx if want_dx else 0, dw, db, npix)
    return dx, dw, db


@pytest.mark.parametrize("sig", [False, True])
@pytest.mark.parametrize("case", range(len(PRED_BWD_CASES)))
def test_pred_bwd_exact(case, sig):
    """Integer x, w, dy and y = 1/2 (dz = dy / 4): every dropped or doubled pixel changes dw / db.  The launch is capped at 512 workgroups
    = 16 384 pixels per lane of the four-pixel unroll: 480 runs u = 0 alone, 2 x 16 384 + 3 stops inside a trip, 65 536 + 16 384 + 5 takes a
    second trip.  Pitches and absent operands rotate with k = (index of npix) + (index of C), so that every C
    meets every variant: dx absent at C = 128 / 36 / 32 (one npix each), padded lddx and ldx at every C."""
    npix, Cc = PRED_BWD_CASES[case]
    k = case // 4 + case % 4
    ldx, lddx = Cc + 4 * (k % 3), Cc + 8 * (k % 2)
    want_dx, want_db = k != 3, sig or k % 3 != 1
    x, w, dy = ri(npix, Cc, seed=19, m=8), ri(Cc, seed=20, m=8), ri(npix, seed=21, m=4)
    y = torch.full((npix,), 0.5, dtype=F64) if sig else None
    dw0, db0 = ri(Cc, seed=22, m=64), ri(1, seed=23, m=64)
    dx, dw, db = _pred_bwd_call(sig, npix, Cc, x, w, y, dy, dw0, db0, ldx, lddx, want_dx, want_db)
    rdx, rdw, rdb = pr.pred_bwd(x, w, dy, y, dw0, db0[0])
    _, adw, adb = pr.pred_bwd(x.abs(), w.abs(), dy.abs(), y, dw0.abs(), db0.abs()[0])
    if want_dx:
        assert_exact(dx.value(), rdx, "pred_bwd dx")
    assert_exact(dw.value(), rdw, "pred_bwd dw", abs_sum=adw)
    if want_db:
        assert_exact(db.value(), rdb.reshape(1, 1), "pred_bwd db", abs_sum=adb.reshape(1, 1))


@pytest.mark.parametrize("Cc", [4, 32, 36, 128])
def test_pred_sigmoid_bwd_general_y(Cc):
    """dz = dy y (1 - y): 3 roundings; dx = dz w: 4; dw / db: sums of n = npix + 1 terms (the value already there is one):
    (n + 2) x 2^-24 x sum |term|, |term| = the expression of dz on absolute values times |x|.  npix = 480 keeps n below 2048."""
    npix = 480
    x, w, dy = rn(npix, Cc, seed=24), rn(Cc, seed=25), rn(npix, seed=26)
    y = torch.sigmoid(rn(npix, seed=27, scale=2.0)).float().to(F64)
    dw0, db0 = rn(Cc, seed=28), rn(1, seed=29)
    dx, dw, db = _pred_bwd_call(True, npix, Cc, x, w, y, dy, dw0, db0, Cc + 4, Cc + 8, True, True)
    rdx, rdw, rdb = pr.pred_bwd(x, w, dy, y, dw0, db0[0])
    dza = dy.abs() * y * (1 + y)
    assert_within(dx.value(), rdx, (4 + 1) * U * dza[:, None] * w.abs()[None], "pred_sigmoid_bwd dx")
    n = npix + 1
    assert_within(dw.value(), rdw, (n + 2) * U * ((dza[:, None] * x.abs()).sum(0) + dw0.abs()), "pred_sigmoid_bwd dw")
    assert_within(db.value(), rdb.reshape(1, 1), (n + 2) * U * (dza.sum() + db0.abs()).reshape(1, 1), "pred_sigmoid_bwd db")


# ------------------------------------------------------------------------------------------------ decoder glue
def _glue_data(B, H, W, Cc, kind, seed):
    make = (lambda *s, seed: ri(*s, seed=seed, m=32)) if kind == "int" else rn
    return make(B, H, W, Cc, seed=seed), make(B, H, W, Cc, seed=seed + 1)


def _glue_cmp(kind, got, ref, abs_ref, roundings, what):
    if kind == "int":
        assert_exact(got, ref, what, abs_sum=abs_ref)
    else:
        assert_within(got, ref, (roundings + 1) * U * abs_ref, what)


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("Cc", [4, 36])
@pytest.mark.parametrize("B,H,W", [(1, 2, 2), (2, 2, 7), (1, 5, 11), (2, 8, 16), (1, 1, 3)])
def test_decoder_glue_forward(B, H, W, Cc, with_skip, kind):
    """pad2_sum (bit: a copy, or one fp32 add), up2x_border_im2col (exact on integers; on normal data: x + skip, two scalings and an add per
    axis pair = 13 roundings, 9 without skip) and the fused launch, bit-identical to the two separate ones."""
    x, skip = _glue_data(B, H, W, Cc, kind, 30)
    skip = skip if with_skip else None
    npad, nr, nc = B * (H + 4) * (W + 4), 2 * B * 2 * W * 5, 2 * B * 2 * H * 5
    pad = Out(npad, Cc)
    call("ramnet_pad2_sum", In(x), In(skip) if with_skip else None, pad, B, H, W, Cc)
    assert_bits(pad.value(), pr.pad2_sum(x, skip), "pad2_sum")
    rows, cols = Out(nr, Cc), Out(nc, Cc)
    call("ramnet_up2x_border_im2col", In(x), In(skip) if with_skip else None, rows, cols, B, H, W, Cc)
    rr, rc = pr.up2x_border_im2col(x, skip)
    ar, ac = pr.up2x_border_im2col(x.abs(), skip.abs() if with_skip else None)
    nround = 13 if with_skip else 9
    _glue_cmp(kind, rows.value(), rr, ar.reshape(nr, Cc), nround, "up2x_border_im2col rows")
    _glue_cmp(kind, cols.value(), rc, ac.reshape(nc, Cc), nround, "up2x_border_im2col cols")
    pad2, rows2, cols2 = Out(npad, Cc), Out(nr, Cc), Out(nc, Cc)
    call("ramnet_pad2_sum_im2col", In(x), In(skip) if with_skip else None, pad2, rows2, cols2, B, H, W, Cc)
    for a, b, what in ((pad2, pad, "pad"), (rows2, rows, "rows"), (cols2, cols, "cols")):
        assert torch.equal(_bits(a.value()), _bits(b.value())), "pad2_sum_im2col: %s differs from the separate launch" % what


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("Cc", [4, 36])
@pytest.mark.parametrize("B,H,W", [(1, 2, 2), (2, 2, 7), (1, 5, 11), (2, 8, 16), (1, 1, 3)])
def test_decoder_glue_adjoints(B, H, W, Cc, kind):
    """upsample2x_bwd: at most 16 weighted terms per pixel (the products of the weights 1/4, 3/4, 1 are exact); unpad2_fold: at most 9
    terms; up2x_border_col2im: a border pixel adds, onto what dx holds, at most 4 line positions x 6 entries per launch, a corner pixel from
    both launches: n <= 49 terms.  Bound of a sum: (n + 2) x 2^-24 x sum |term|."""
    make = (lambda *s, seed: ri(*s, seed=seed, m=64)) if kind == "int" else rn
    dup = make(B, 2 * H, 2 * W, Cc, seed=32)
    dx = Out(B * H * W, Cc)
    call("ramnet_upsample2x_bwd", In(dup), dx, B, H, W, Cc)
    _glue_cmp(kind, dx.value(), pr.upsample2x_bwd(dup), pr.upsample2x_bwd(dup.abs()).reshape(-1, Cc), 16 + 1, "upsample2x_bwd")
    if H < 2:          # the other two adjoints refuse H = 1 (test_argument_checks)
        return
    dxpad = make(B, H + 4, W + 4, Cc, seed=33)
    dx = Out(B * H * W, Cc)
    call("ramnet_unpad2_fold", In(dxpad), dx, B, H, W, Cc)
    _glue_cmp(kind, dx.value(), pr.unpad2_fold(dxpad), pr.unpad2_fold(dxpad.abs()).reshape(-1, Cc), 9 + 1, "unpad2_fold")
    gr, gc, dx0 = make(2, B, 2 * W, 5, Cc, seed=34), make(2, B, 2 * H, 5, Cc, seed=35), make(B, H, W, Cc, seed=36)
    dx = Out(B * H * W, Cc, prefill=dx0)
    call("ramnet_up2x_border_col2im", In(gr), In(gc), dx, B, H, W, Cc)
    ref, aref = pr.up2x_border_col2im(gr, gc, dx0), pr.up2x_border_col2im(gr.abs(), gc.abs(), dx0.abs())
    got = dx.value().view(B, H, W, Cc)
    corner = lambda t: t.reshape(B, H, W, Cc)[:, [0, 0, -1, -1], [0, -1, 0, -1]].reshape(-1, Cc)
    _glue_cmp(kind, corner(got), corner(ref), corner(aref), 49 + 1, "up2x_border_col2im corners (row and column launch)")
    _glue_cmp(kind, got.reshape(-1, Cc), ref, aref.reshape(-1, Cc), 49 + 1, "up2x_border_col2im")
    if H > 2 and W > 2:
        assert_bits(got[:, 1:-1, 1:-1], dx0[:, 1:-1, 1:-1], "up2x_border_col2im interior")


def test_pad2_sum_second_trip():
    B, H, W, Cc = 1, 510, 509, 8
    assert B * (H + 4) * (W + 4) * (Cc // 4) >= TRIP2
    x, skip = rn(B, H, W, Cc, seed=37), rn(B, H, W, Cc, seed=38)
    pad = Out(B * (H + 4) * (W + 4), Cc)
    call("ramnet_pad2_sum", In(x), In(skip), pad, B, H, W, Cc)
    assert_bits(pad.value(), pr.pad2_sum(x, skip), "pad2_sum")


# ------------------------------------------------------------------------------------------------ ConvGRU backward maps
def _gru_case(npix, Cc, seed):
    u, r = torch.sigmoid(rn(npix, Cc, seed=seed)).float().to(F64), torch.sigmoid(rn(npix, Cc, seed=seed + 1)).float().to(F64)
    o = torch.tanh(rn(npix, Cc, seed=seed + 2)).float().to(F64)
    return u, r, o, rn(npix, Cc, seed=seed + 3), rn(npix, Cc, seed=seed + 4)


def _run_gru(Cc, npix, pitched, with_h):
    """Roundings of the documented expressions: dpo = dh' u (1 - o^2): 4; dpu = dh' (o - h) u (1 - u): 5; dh = dh' (1 - u): 2;
    dpr = dhr h r (1 - r): 4; dh + dhr r: 2."""
    u, r, o, h, dhn = _gru_case(npix, Cc, 40)
    ld = 2 * Cc + 4 if pitched else Cc
    hin = In(h) if with_h else None
    hv = h if with_h else torch.zeros_like(h)
    rdpo, rdpu, rdh = pr.gru_bwd_a(dhn, u, o, h if with_h else None)
    g = dhn.abs()
    bounds = ((4 + 1) * U * g * u * (1 + o * o), (5 + 1) * U * g * (o.abs() + hv.abs()) * u * (1 + u), (2 + 1) * U * g * (1 + u))
    for a2 in (False, True):
        dpo, dpur = Out(npix, Cc), Out(npix, Cc, ld=2 * Cc)                   # stage A writes the u half of dpur alone
        dh = Out(npix, Cc, ld=ld if a2 else Cc)
        ur = In(torch.cat([u, r], 1))
        if a2:
            call("ramnet_gru_bwd_a2", In(dhn, ld), ur, In(o), hin, dpo, dpur, dh, npix, Cc, ld, ld)
        else:
            call("ramnet_gru_bwd_a", In(dhn, ld), ur, In(o), hin, dpo, dpur, dh, npix, Cc, ld)
        name = "gru_bwd_a2" if a2 else "gru_bwd_a"
        assert_within(dpo.value(), rdpo, bounds[0], name + " dpo")
        assert_within(dpur.value(), rdpu, bounds[1], name + " dpu")
        assert_within(dh.value(), rdh, bounds[2], name + " dh")
    # stage B: in place on the second half of dxhr = [dx1 | d(h.r)]; it reads r alone (the u half of `ur` is poisoned)
    dx1, dhr, d0 = rn(npix, Cc, seed=50), rn(npix, Cc, seed=51), rn(npix, Cc, seed=52)
    dxhr = Out(npix, 2 * Cc, prefill=torch.cat([dx1, dhr], 1))
    dpur = Out(npix, Cc, ld=2 * Cc, col0=Cc)
    call("ramnet_gru_bwd_b", dxhr, In(torch.cat([torch.full_like(u, float("nan")), r], 1)), hin, dpur, In(d0), npix, Cc)
    rdpr, rd = pr.gru_bwd_b(dhr, r, d0, h if with_h else None)
    assert_bits(dxhr.value()[:, :Cc], dx1, "gru_bwd_b dx half")
    assert_within(dxhr.value()[:, Cc:], rd, (2 + 1) * U * (d0.abs() + dhr.abs() * r), "gru_bwd_b dh")
    assert_within(dpur.value(), rdpr, (4 + 1) * U * dhr.abs() * hv.abs() * r * (1 + r), "gru_bwd_b dpr")


@pytest.mark.parametrize("with_h", [True, False])
@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("npix", [1, 91])
@pytest.mark.parametrize("Cc", [4, 12, 64])
def test_gru_bwd_maps(Cc, npix, pitched, with_h):
    _run_gru(Cc, npix, pitched, with_h)


def test_gru_bwd_maps_second_trip():
    _run_gru(8, (TRIP2 + 1) // 2, False, True)


# ------------------------------------------------------------------------------------------------ ConvLSTM backward maps
def _lstm_case(npix, Cc, seed):
    gates = torch.cat([torch.sigmoid(rn(npix, 3 * Cc, seed=seed)), torch.tanh(rn(npix, Cc, seed=seed + 1))], 1).float().to(F64)
    cp = rn(npix, Cc, seed=seed + 2, scale=1.5)
    cn = (gates[:, Cc:2 * Cc] * cp + gates[:, :Cc] * gates[:, 3 * Cc:]).float().to(F64)
    return gates, cp, cn, rn(npix, Cc, seed=seed + 3), rn(npix, Cc, seed=seed + 4)


def _lstm_bounds(gates, cp, cn, dh, dc):
    """tc = tanhf_(c') carries the measured error TANH_ERR (et).  dct = dc + dh o (1 - tc^2): 5 roundings, |d dct / d tc| = 2 |dh| o |tc|;
    dpo = dh tc o (1 - o): 4; dpf = dct c f (1 - f), dpi = dct g i (1 - i), dpg = dct i (1 - g^2): 5 + 4; dc_prev = dct f: 5 + 1."""
    Cc = cn.shape[1]
    gi, gf, go, gc = (gates[:, k * Cc:(k + 1) * Cc] for k in range(4))
    assert float(cn.abs().max()) <= TANH_RANGE
    tc, dh, dc, cp, et = torch.tanh(cn), dh.abs(), dc.abs(), cp.abs(), 4 * TANH_ERR
    A, S = dc + dh * go * (1 + tc * tc), 2 * dh * go * tc.abs()
    bi = (9 + 1) * U * A * gc.abs() * gi * (1 + gi) + et * S * gc.abs() * gi * (1 - gi)
    bf = (9 + 1) * U * A * cp * gf * (1 + gf) + et * S * cp * gf * (1 - gf)
    bo = (4 + 1) * U * dh * tc.abs() * go * (1 + go) + et * dh * go * (1 - go)
    bg = (9 + 1) * U * A * gi * (1 + gc * gc) + et * S * gi * (1 - gc * gc)
    return torch.cat([bi, bf, bo, bg], 1), (6 + 1) * U * A * gf + et * S * gf


@pytest.mark.parametrize("absent", ["none", "cprev", "dhn", "dcn"])
@pytest.mark.parametrize("Cc,npix", [(4, 1), (12, 1), (64, 1), (4, 91), (12, 91), (64, 91), (8, (TRIP2 + 1) // 2)])
def test_lstm_bwd(Cc, npix, absent):
    """(the last case: the second grid-stride trip, at C = 8)"""
    gates, cp, cn, dh, dc = _lstm_case(npix, Cc, 60)
    cp, dh, dc = (None if absent == k else t for k, t in (("cprev", cp), ("dhn", dh), ("dcn", dc)))
    if cp is None:
        cn = (gates[:, :Cc] * gates[:, 3 * Cc:]).float().to(F64)
    opt = lambda t: None if t is None else In(t)
    dpre, dcp = Out(npix, 4 * Cc), Out(npix, Cc)
    call("ramnet_lstm_bwd", In(gates), opt(cp), In(cn), opt(dh), opt(dc), dpre, dcp, npix, Cc)
    rpre, rdcp = pr.lstm_bwd(gates, cn, cp, dh, dc)
    z = torch.zeros_like(cn)
    bpre, bdcp = _lstm_bounds(gates, z if cp is None else cp, cn, z if dh is None else dh, z if dc is None else dc)
    assert_within(dpre.value(), rpre, bpre, "lstm_bwd dpre")
    assert_within(dcp.value(), rdcp, bdcp, "lstm_bwd dc_prev")


@pytest.mark.parametrize("absent", ["none", "dhn", "dcn"])
@pytest.mark.parametrize("active", [[1, 0, 1], [0, 0, 0], [1, 1, 1]])
@pytest.mark.parametrize("Cc,hw", [(4, 1), (12, 7), (64, 31)])
def test_lstm_bwd_masked(Cc, hw, active, absent):
    npix = 3 * hw
    gates, cp, cn, dh, dc = _lstm_case(npix, Cc, 70)
    dh, dc = (None if absent == k else t for k, t in (("dhn", dh), ("dcn", dc)))
    opt = lambda t: None if t is None else In(t)
    act = torch.tensor(active, dtype=torch.int32, device=_dev())
    dpre, dcp, dxh = Out(npix, 4 * Cc), Out(npix, Cc), Out(npix, 2 * Cc)
    call("ramnet_lstm_bwd_masked", In(gates), In(cp), In(cn), opt(dh), opt(dc), act, dpre, dcp, dxh, npix, hw, Cc)
    rpre, rdcp, rdxh = pr.lstm_bwd_masked(gates, cn, active, hw, cp, dh, dc)
    z = torch.zeros_like(cn)
    bpre, bdcp = _lstm_bounds(gates, cp, cn, z if dh is None else dh, z if dc is None else dc)
    on = (torch.tensor(active) != 0).repeat_interleave(hw)
    assert_bits(dxh.value(), rdxh, "lstm_bwd_masked dxh")
    assert_bits(dpre.value()[~on], rpre[~on], "lstm_bwd_masked dpre of inactive samples")
    assert_bits(dcp.value()[~on], rdcp[~on], "lstm_bwd_masked dc_prev of inactive samples")
    assert_within(dpre.value()[on], rpre[on], bpre[on], "lstm_bwd_masked dpre")
    assert_within(dcp.value()[on], rdcp[on], bdcp[on], "lstm_bwd_masked dc_prev")


# ------------------------------------------------------------------------------------------------ the two measured intrinsics
def test_intrinsic_errors():
    """sigmoidf_ through ramnet_pred_sigmoid_fwd (C = 4, w = (1, 0, 0, 0), no bias: the dot product is x itself) and tanhf_ through
    ramnet_lstm_bwd (dh' = 1, o = 1/2, dc' = 0: dpo = tc / 4 exactly), each over the argument range the tests above stay in, against float64.
    The recorded constants are these maxima; the tests use 4 x them."""
    n = 1 << 17
    zs = torch.cat([torch.linspace(-SIG_RANGE, SIG_RANGE, n), rn(n, seed=80, scale=3.0).float().clamp(-SIG_RANGE, SIG_RANGE)]).to(F64)
    x = torch.zeros(2 * n, 4, dtype=F64)
    x[:, 0] = zs
    y = Out(1, 2 * n)
    call("ramnet_pred_sigmoid_fwd", In(x), 4, 4, In(torch.tensor([1.0, 0, 0, 0])), None, y, 2 * n)
    es = float((y.value().double().view(-1) - torch.sigmoid(zs)).abs().max())
    cs = torch.cat([torch.linspace(-TANH_RANGE, TANH_RANGE, n), rn(n, seed=81, scale=1.5).float().clamp(-TANH_RANGE, TANH_RANGE)]).to(F64)
    Cc, npix = 4, 2 * n // 4
    gates = torch.full((npix, 4 * Cc), 0.5, dtype=F64)
    dpre, dcp = Out(npix, 4 * Cc), Out(npix, Cc)
    call("ramnet_lstm_bwd", In(gates), None, In(cs.view(npix, Cc)), In(torch.ones(npix, Cc)), None, dpre, dcp, npix, Cc)
    tc = 4 * dpre.value().double()[:, 2 * Cc:3 * Cc]
    et = float((tc - torch.tanh(cs.view(npix, Cc))).abs().max())
    print("measured: sigmoidf_ max |err| %.4e over [-%g, %g]; tanhf_ max |err| %.4e over [-%g, %g]" % (es, SIG_RANGE, SIG_RANGE, et, TANH_RANGE, TANH_RANGE))
    assert es <= SIGMOID_ERR and et <= TANH_ERR


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks():
    """Every refusal returns RAMNET_E_BADARG with a message and launches nothing (the outputs keep their sentinel).  All pointers are valid
    buffers large enough for the nearest accepted call."""
    i, o = In(torch.zeros(64, 64)), Out(64, 64)
    act = torch.ones(4, dtype=torch.int32, device=_dev())
    tg = (C.c_void_p * 1)(i.ptr)                      # host array of segment targets
    bad = [
        ("ramnet_nchw_to_nhwc_pad", i, o, 1, 5, 2, 2, 6), ("ramnet_nchw_to_nhwc_pad", i, o, 1, 5, 2, 2, 4), ("ramnet_nchw_to_nhwc_pad", None, o, 1, 4, 2, 2, 4),
        ("ramnet_reflect_pad", i, o, 1, 5, 5, 7, 6, 2, 1, 8, 8, 1), ("ramnet_reflect_pad", i, o, 1, 5, 5, 7, 4, 2, 1, 8, 8, 1),
        ("ramnet_reflect_pad", i, o, 1, 1, 2, 7, 4, 2, 1, 8, 8, 0), ("ramnet_reflect_pad", i, o, 1, 1, 5, 7, 4, 2, 1, 6, 8, 0),
        ("ramnet_relu_bwd", None, i, o, 16), ("ramnet_add", i, None, o, 16), ("ramnet_add", i, i, None, 16),
        ("ramnet_concat2", i, 8, 6, i, 8, 4, o, 4), ("ramnet_concat2", i, 4, 8, i, 8, 4, o, 4), ("ramnet_concat2", i, 8, 8, i, 6, 4, o, 4),
        ("ramnet_concat2", i, 8, 8, i, 4, 8, o, 4),
        ("ramnet_split2", i, 12, 6, 6, o, o, 4), ("ramnet_split2", i, 8, 8, 4, o, o, 4), ("ramnet_split2", i, 14, 8, 4, o, o, 4),
        ("ramnet_bias_grad", i, None, o, 4, 6), ("ramnet_bias_grad", i, None, o, 1, 1028), ("ramnet_bias_grad", i, None, o, 4, 0),
        ("ramnet_pred_sigmoid_fwd", i, 8, 6, i, i, o, 4), ("ramnet_pred_sigmoid_fwd", i, 10, 8, i, i, o, 4), ("ramnet_pred_sigmoid_fwd", i, 4, 8, i, i, o, 4),
        ("ramnet_pred_linear_fwd", i, 8, 6, i, None, o, 4), ("ramnet_pred_linear_fwd", i, 4, 8, i, None, o, 4), ("ramnet_pred_linear_fwd", i, 8, 0, i, None, o, 4),
        ("ramnet_pred_sigmoid_bwd", i, 8, 6, i, i, i, o, 8, o, o, 4), ("ramnet_pred_sigmoid_bwd", i, 132, 132, i, i, i, o, 132, o, o, 4),
        ("ramnet_pred_sigmoid_bwd", i, 4, 8, i, i, i, o, 8, o, o, 4), ("ramnet_pred_sigmoid_bwd", i, 8, 8, i, i, i, o, 4, o, o, 4),
        ("ramnet_pred_sigmoid_bwd", i, 8, 8, i, i, i, o, 10, o, o, 4), ("ramnet_pred_sigmoid_bwd", i, 8, 8, i, i, i, o, 8, o, None, 4),
        ("ramnet_pred_linear_bwd", i, 8, 6, i, i, o, 8, o, o, 4), ("ramnet_pred_linear_bwd", i, 132, 132, i, i, o, 132, o, o, 4),
        ("ramnet_pred_linear_bwd", i, 4, 8, i, i, o, 8, o, o, 4), ("ramnet_pred_linear_bwd", i, 8, 8, i, i, o, 4, o, o, 4),
        ("ramnet_upsample2x_bwd", i, o, 1, 2, 2, 6), ("ramnet_upsample2x_bwd", i, o, 1, 0, 2, 4),
        ("ramnet_pad2_sum", i, None, o, 1, 2, 2, 6), ("ramnet_pad2_sum", i, None, o, 0, 2, 2, 4),
        ("ramnet_up2x_border_im2col", i, None, o, o, 1, 2, 2, 6), ("ramnet_pad2_sum_im2col", i, None, o, o, o, 1, 2, 2, 6),
        ("ramnet_unpad2_fold", i, o, 1, 1, 3, 4), ("ramnet_unpad2_fold", i, o, 1, 3, 1, 4), ("ramnet_unpad2_fold", i, o, 1, 2, 2, 6),
        ("ramnet_up2x_border_col2im", i, i, o, 1, 1, 3, 4), ("ramnet_up2x_border_col2im", i, i, o, 1, 3, 1, 4), ("ramnet_up2x_border_col2im", i, i, o, 1, 2, 2, 6),
        ("ramnet_frame_gather", i, None, o, o, 1, 3, 4, 4), ("ramnet_frame_gather", i, None, o, o, 1, 4, 2, 4), ("ramnet_frame_gather", i, None, o, o, 1, 4, 4, 6),
        ("ramnet_space_to_depth2", i, o, 1, 3, 4, 4, 0), ("ramnet_space_to_depth2", i, o, 1, 4, 4, 6, 1),
        ("ramnet_gru_bwd_a", i, i, i, i, o, o, o, 4, 6, 8), ("ramnet_gru_bwd_a", i, i, i, i, o, o, o, 4, 8, 4), ("ramnet_gru_bwd_a", i, i, i, i, o, o, o, 4, 8, 10),
        ("ramnet_gru_bwd_a", i, i, i, i, o, o, o, 4, 0, 8),
        ("ramnet_gru_bwd_a2", i, i, i, i, o, o, o, 4, 6, 8, 8), ("ramnet_gru_bwd_a2", i, i, i, i, o, o, o, 4, 8, 4, 8), ("ramnet_gru_bwd_a2", i, i, i, i, o, o, o, 4, 8, 8, 4),
        ("ramnet_gru_bwd_a2", i, i, i, i, o, o, o, 4, 8, 8, 10), ("ramnet_gru_bwd_a2", i, i, i, i, o, o, o, 4, -4, 8, 8),
        ("ramnet_gru_bwd_b", o, i, i, o, i, 4, 6), ("ramnet_gru_bwd_b", o, i, i, o, i, 4, 0), ("ramnet_gru_bwd_b", o, None, i, o, i, 4, 4),
        ("ramnet_lstm_bwd", i, i, i, i, i, o, o, 4, 6), ("ramnet_lstm_bwd", i, i, i, i, i, o, o, 4, -4), ("ramnet_lstm_bwd", i, i, None, i, i, o, o, 4, 4),
        ("ramnet_lstm_bwd_masked", i, i, i, i, i, act, o, o, o, 4, 1, 6), ("ramnet_lstm_bwd_masked", i, i, i, i, i, act, o, o, o, 4, 3, 4),
        ("ramnet_lstm_bwd_masked", i, i, i, i, i, act, o, o, o, 4, 0, 4), ("ramnet_lstm_bwd_masked", i, i, i, i, i, None, o, o, o, 4, 1, 4),
        ("ramnet_lstm_bwd_masked", i, i, i, i, i, act, o, o, o, 4, 1, 0),
        ("ramnet_pred_sigmoid_si_fwd", i, 4, 8, i, i, o, 4, 1, tg, 1.0, 1.0, i, o, o), ("ramnet_pred_sigmoid_si_fwd", i, 8, 6, i, i, o, 4, 1, tg, 1.0, 1.0, i, o, o),
        ("ramnet_pred_sigmoid_si_bwd", i, 4, 8, i, i, i, 4, 1, tg, i, i, 1.0, 1.0, o, 8, o, o, None, 0),
        ("ramnet_pred_sigmoid_si_bwd", i, 8, 8, i, i, i, 4, 1, tg, i, i, 1.0, 1.0, o, 4, o, o, None, 0),
        ("ramnet_pred_sigmoid_si_bwd", i, 8, 8, i, i, i, 4, 1, tg, i, i, 1.0, 1.0, o, 10, o, o, None, 0),
    ]
    for args in bad:
        call(*args, rc=BADARG)
