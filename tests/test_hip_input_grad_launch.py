"""GPU: the three input-gradient entry points, launch by launch through tests/guarded.py — buffers between guards, NaN in the pitch gaps,
guards and gaps intact afterwards — against the float64 statements of tests/input_grad_restatement.py.

ramnet_head_dgrad tiles the map in 16 rows x 32 columns per workgroup (a wave: 4 rows x two 16-pixel MFMA tiles).  Sizes: 1 x 1; 3 x 5
(smaller than the 5 x 5 window); 17 x 33 (one pixel past a tile in each direction: 2 x 2 workgroups); 2 x 36 x 70 (3 x 3 tiles per image, two
images, ragged 16-pixel halves).  Bounds: (a) integer operands whose absolute-value statement stays below 2^24 / 16 — every partial sum is
exact in fp32 and the result is the statement bit for bit; (b) Gaussian operands, per element (800 + 2) U S_abs + U |ref|, the summation
bound of the convolution launch tests (800 = 25 taps x 32 feature maps terms meet in an element), derived and not measured."""
import pytest
import torch

import input_grad_restatement as R
from guarded import BADARG, F64, In, Out, U, assert_bits, assert_exact, assert_within, call, ri, rn

pytestmark = pytest.mark.gpu

SIZES = [(1, 1, 1), (1, 3, 5), (1, 17, 33), (2, 36, 70)]
VARIANTS = [(32, True, 32), (32, False, 40), (7, True, 40), (7, False, 32), (7, True, 32), (32, True, 40)]     # (Cout, mask operand, pitch of dy and y)


def head_launch(dy, w, y, ldg, B, H, W, cin, cout):
    ld = (cin + 3) // 4 * 4
    dx = Out(B * H * W, ld)
    call("ramnet_head_dgrad", In(dy, ld=ldg), ldg, In(y, ld=ldg) if y is not None else None, ldg if y is not None else 0, In(w.reshape(1, -1)),
         dx, ld, B, H, W, cin, cout)
    return dx.value().view(B, H, W, ld)


@pytest.mark.parametrize("B,H,W", SIZES, ids=["%dx%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("cin", [1, 3, 5, 10])
def test_head_dgrad(cin, B, H, W):
    from rpg_ramnet_amd import _hip
    for cout, masked, ldg in VARIANTS:
        what = "head_dgrad cin %d cout %d mask %d pitch %d %dx%dx%d" % (cin, cout, masked, ldg, B, H, W)
        # (a) integers: bit for bit the statement
        dy, w = ri(B, H, W, cout, seed=11, m=4), ri(cout, cin, 5, 5, seed=12, m=3)
        y = ri(B, H, W, cout, seed=13, m=2) if masked else None
        got = head_launch(dy, w, y, ldg, B, H, W, cin, cout)
        assert _hip.lib().ramnet_last_kernel().decode() == "conv_head_dgrad_kernel"
        assert R.head_dgrad_partial_max(dy, w, y) * 16 < 2 ** 24
        assert_exact(got, R.head_dgrad(dy, w, y), what + " (integers)", abs_sum=R.head_dgrad(dy, w, y, absolute=True))
        # (b) Gaussian operands: the summation bound
        dy, w = rn(B, H, W, cout, seed=14), rn(cout, cin, 5, 5, seed=15, scale=0.2)
        y = rn(B, H, W, cout, seed=16) if masked else None
        got = head_launch(dy, w, y, ldg, B, H, W, cin, cout)
        ref, s_abs = R.head_dgrad(dy, w, y), R.head_dgrad(dy, w, y, absolute=True)
        assert_within(got, ref, (800 + 2) * U * s_abs + U * ref.abs(), what + " (gaussian)")
        assert not bool(got[..., cin:].view(torch.int32).any()), what + ": a pad lane is not +0"


def test_head_dgrad_refuses_its_preconditions():
    B, H, W, cin, cout = 1, 3, 5, 5, 32
    dy, y, w = In(rn(B, H, W, cout, seed=1)), In(rn(B, H, W, cout, seed=2)), In(rn(1, cout * cin * 25, seed=3))
    dy1, y1 = In(rn(B, H, W, cout, seed=1), skew=1), In(rn(B, H, W, cout, seed=2), skew=2)
    good = dict(dy=dy, ldg=32, y=y, ldgm=32, w=w, dx=None, ld=8, B=B, H=H, W=W, Cin=cin, Cout=cout)
    order = ("dy", "ldg", "y", "ldgm", "w", "dx", "ld", "B", "H", "W", "Cin", "Cout")
    bad = [dict(dy=None), dict(w=None), dict(B=0), dict(H=0), dict(W=0), dict(Cin=2), dict(Cin=6), dict(Cin=3), dict(Cout=33), dict(Cout=0),
           dict(ld=12), dict(ld=4), dict(ldg=30), dict(ldg=28), dict(dy=dy1), dict(ldgm=30), dict(ldgm=28), dict(y=y1)]
    for over in bad:
        dx = Out(B * H * W, 8)
        a = dict(good, dx=dx, **over)
        call("ramnet_head_dgrad", *[a[k] for k in order], rc=BADARG)
    dx = Out(B * H * W, 8)
    call("ramnet_head_dgrad", dy, 32, y, 32, w, None, 8, B, H, W, cin, cout, rc=BADARG)
    a = dict(good, dx=dx)
    call("ramnet_head_dgrad", *[a[k] for k in order])           # and the untouched arguments launch


@pytest.mark.parametrize("Cc", [1, 5, 6, 10])
def test_nhwc_unpad_to_nchw(Cc):
    B, H, W = 2, 5, 7
    Cpad = (Cc + 3) // 4 * 4
    src = rn(B * H * W, Cpad, seed=20 + Cc)
    dst = Out(1, B * Cc * H * W, skew=3)
    call("ramnet_nhwc_unpad_to_nchw", In(src, skew=1), dst, B, Cc, H, W, Cpad)
    assert_bits(dst.value(), R.nhwc_unpad(src.view(B, H, W, Cpad), Cc), "nhwc_unpad_to_nchw")
    wide = Out(1, B * Cc * H * W)
    call("ramnet_nhwc_unpad_to_nchw", In(src[:, :Cc], ld=Cpad + 4), wide, B, Cc, H, W, Cpad + 4)      # a wider pitch: the gap lanes (NaN) are not read
    assert_bits(wide.value(), dst.value(), "nhwc_unpad_to_nchw at a wider pitch")
    new = Out(1, B * Cc * H * W)
    for args in ((None, new, B, Cc, H, W, Cpad), (In(src), new, 0, Cc, H, W, Cpad), (In(src), new, B, Cc, H, W, Cpad + 2), (In(src), new, B, Cpad + 1, H, W, Cpad)):
        call("ramnet_nhwc_unpad_to_nchw", *args, rc=BADARG)


def pad_launch(g, B, Cc, H, W, Cpad, top, left, Hc, Wc, nhwc):
    gin = In(g.permute(0, 2, 3, 1).reshape(-1, Cc), ld=Cpad) if nhwc else In(g.reshape(1, -1))
    dx = Out(1, B * Cc * H * W)
    call("ramnet_reflect_pad_bwd", gin, dx, B, Cc, H, W, Cpad, top, left, Hc, Wc, nhwc)
    return dx.value().view(B, Cc, H, W)


@pytest.mark.parametrize("nhwc", [0, 1])
@pytest.mark.parametrize("H,W,Hc,Wc,top,left", R.PAD_CASES)
def test_reflect_pad_bwd(H, W, Hc, Wc, top, left, nhwc):
    B, Cc, Cpad = 2, 5, 8
    what = "reflect_pad_bwd %dx%d -> %dx%d nhwc %d" % (H, W, Hc, Wc, nhwc)
    g = ri(B, Cc, Hc, Wc, seed=31, m=9)
    got = pad_launch(g, B, Cc, H, W, Cpad, top, left, Hc, Wc, nhwc)
    assert_exact(got, R.reflect_pad_bwd(g, Cc, H, W, top, left, 0), what + " (integers)", abs_sum=R.reflect_pad_bwd(g, Cc, H, W, top, left, 0, absolute=True))
    g = rn(B, Cc, Hc, Wc, seed=32)
    got = pad_launch(g, B, Cc, H, W, Cpad, top, left, Hc, Wc, nhwc)
    assert_within(got, R.reflect_pad_bwd(g, Cc, H, W, top, left, 0), 9 * U * R.reflect_pad_bwd(g, Cc, H, W, top, left, 0, absolute=True), what + " (gaussian)")
    # the header's order, term by term in fp32: the same bits
    assert_bits(got, R.reflect_pad_bwd(g, Cc, H, W, top, left, 0, dtype=torch.float32), what + " (the stated order in fp32)")
    dx = Out(1, B * Cc * H * W)
    for args in ((In(g.reshape(1, -1)), dx, B, Cc, H, W, 6, top, left, Hc, Wc, 1), (In(g.reshape(1, -1)), dx, B, Cc, H, W, Cpad, H, left, Hc + H, Wc, 0),
                 (In(g.reshape(1, -1)), dx, B, Cc, H, W, Cpad, top, left, H + top - 1, Wc, 0), (None, dx, B, Cc, H, W, Cpad, top, left, Hc, Wc, 0)):
        call("ramnet_reflect_pad_bwd", *args, rc=BADARG)


def test_repeat_launches_give_the_same_bits():
    B, H, W, cin, cout = 2, 36, 70, 5, 32
    dy, w, y = rn(B, H, W, cout, seed=41), rn(cout, cin, 5, 5, seed=42, scale=0.2), rn(B, H, W, cout, seed=43)
    a, b = (head_launch(dy, w, y, 32, B, H, W, cin, cout) for _ in range(2))
    assert_bits(a, b.double(), "head_dgrad twice")
    src = rn(B * H * W, 8, seed=44)
    outs = []
    for _ in range(2):
        dst = Out(1, B * cin * H * W)
        call("ramnet_nhwc_unpad_to_nchw", In(src), dst, B, cin, H, W, 8)
        outs.append(dst.value())
    assert_bits(outs[0], outs[1].double(), "nhwc_unpad_to_nchw twice")
    H, W, Hc, Wc, top, left = R.PAD_CASES[2]
    g = rn(B, cin, Hc, Wc, seed=45)
    a, b = (pad_launch(g, B, cin, H, W, 8, top, left, Hc, Wc, 1) for _ in range(2))
    assert_bits(a, b.double(), "reflect_pad_bwd twice")
