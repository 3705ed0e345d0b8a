"""GPU: the head (RAMNET_ALGO_HEAD), folded-decoder (RAMNET_ALGO_WINOGRAD24 / _2X3: forward, RAMNET_IN_PARITY4 backward-data, backward-weights
with the library's own unpack) and weight-pack entry points called alone through the C ABI, every launch through guarded.call /
guarded.call_desc, compared element by element with the float64 statements of tests/conv_restatement.py under the rules of
profiles/fold_head_launch_tests_notes.md (those of profiles/conv_launch_tests_notes.md): exact on integer data, derived on normal data,
bit for the packs on integer data and for repeated split reductions.  The rows are tests/fold_head_cases.py."""
import contextlib
import ctypes as C
import types

import pytest
import torch

import conv_restatement as cr
import fold_head_cases as fh
from guarded import BADARG, F64, In, Out, _bits, assert_bits, assert_exact, assert_within, call, call_desc
from rpg_ramnet_amd import _hip

pytestmark = pytest.mark.gpu

ALGO = {"fold2x2": _hip.ALGO_WINOGRAD24, "fold2x3": _hip.ALGO_WINOGRAD24_2X3}
U = cr.U


@contextlib.contextmanager
def option(name, value):
    L = _hip.lib()
    old = L.ramnet_get_option(name)
    try:
        assert L.ramnet_set_option(name, value) == 0
        yield
    finally:
        L.ramnet_set_option(name, old)


def _struct(cls, f):
    s = cls()
    for k, v in f.items():
        if isinstance(v, (In, Out)):
            v = v.ptr
        if isinstance(v, list):
            for j, e in enumerate(v):
                getattr(s, k)[j] = e
        else:
            setattr(s, k, v)
    return s


def _taps(taps):
    return dict(ntaps=len(taps), dy=[t[0] for t in taps], dx=[t[1] for t in taps], wtap=[t[2] for t in taps])


# ---------------------------------------------------------------------------------------------------- packs
def pack_fold(w5, fam, dgrad=False):
    """the library's own fold pack into a guarded buffer of the library's own size (under the current `fold_pair` option), frozen"""
    L = _hip.lib()
    Cout, Cin = w5.shape[:2]
    size = L.ramnet_packed_weight_elems_fold_wino(Cout, Cin) if fam == "fold2x2" else L.ramnet_packed_weight_elems_fold_wino2x3(Cout, Cin)
    wp = Out(1, size)
    name = "ramnet_pack_weight_fold_wino" + ("2x3" if fam == "fold2x3" else "") + ("_dgrad" if dgrad else "")
    call(name, In(w5.reshape(-1)), wp, Cout, Cin)
    return wp.freeze()


def _judge_pack(got, ref, ref_abs, kind, what):
    if kind == "int":
        assert_bits(got, ref, what)
    else:                                           # one rounding of the documented expression (evaluated in double)
        assert_within(got, ref.reshape(got.shape), (U * ref_abs + 2.0 ** -50 * ref_abs).reshape(got.shape), what)


PACKS = [(fam, Cout, Cin, pair, kind) for fam in ("fold2x2", "fold2x3") for Cout, Cin in fh.PACK_SHAPES for pair in (1, 0) for kind in ("int", "normal")
         if (pair == 1 or (Cout == 32 and Cin % 32 == 0)) and (fam == "fold2x2" or Cout % 64 == 0 or (pair and Cout == 32 and Cin % 32 == 0))]


@pytest.mark.parametrize("fam,Cout,Cin,pair,kind", PACKS, ids=["%s-%dx%d-pair%d-%s" % p for p in PACKS])
def test_pack_fold(fam, Cout, Cin, pair, kind):
    """ramnet_pack_weight_fold_wino / ...2x3 in their three / two layouts ((8, 2) chunks for 32-column workgroups, (16, 4), the pair layout):
    the fp32 rounding of the rational U = G W4 Gc^T, bit for bit on 9 x integer weights, within one rounding on normal data"""
    w5 = fh.pack_weights(Cout, Cin, kind)
    tw = cr.FOLD_TW[fam]
    is_pair = bool(pair) and Cout == 32 and Cin % 32 == 0
    with option(b"fold_pair", pair):
        wp = pack_fold(w5, fam)
    _judge_pack(wp.value()[0], cr.pack_fold_statement(w5, tw, pair=is_pair), cr.pack_fold_statement(w5, tw, pair=is_pair, absolute=True), kind,
                "%s pack %dx%d pair %d" % (fam, Cout, Cin, pair))


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("Cout,Cin", [(128, 64), (64, 64), (32, 64), (16, 128)])
@pytest.mark.parametrize("fam", ["fold2x2", "fold2x3"])
def test_pack_fold_dgrad(fam, Cout, Cin, kind):
    w5 = fh.pack_weights(Cout, Cin, kind)
    tw = cr.FOLD_TW[fam]
    wp = pack_fold(w5, fam, dgrad=True)
    _judge_pack(wp.value()[0], cr.pack_fold_dgrad_statement(w5, tw), cr.pack_fold_dgrad_statement(w5, tw, absolute=True), kind,
                "%s dgrad pack %dx%d" % (fam, Cout, Cin))


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("Cout,Cin", [(32, 16), (64, 32), (20, 12)])
def test_pack_border_weights(Cout, Cin, kind):
    w5 = fh.pack_weights(Cout, Cin, kind)
    n = 2 * 5 * Cin * 2 * Cout
    bufs = [Out(1, n) for _ in range(4)]
    call("ramnet_pack_border_weights", In(w5.reshape(-1)), *bufs, Cout, Cin)
    for got, ref, what in zip(bufs, cr.border_statement(w5), ("rows", "cols", "rows_t", "cols_t")):
        assert_bits(got.value()[0], ref.float().double(), "border weights %s" % what)      # (a sum of two fp32 numbers, rounded once)


@pytest.mark.parametrize("cin,Cout", [(1, 32), (3, 20), (5, 32), (10, 8), (10, 32)])
def test_pack_head(cin, Cout):
    L = _hip.lib()
    assert L.ramnet_head_supported(cin, Cout) == 1
    w = fh._rn(fh._gen("head_pack%d" % cin), (Cout, cin, 5, 5))
    wp = Out(1, L.ramnet_packed_weight_elems_head(cin))
    call("ramnet_pack_weight_head", In(w.reshape(-1)), wp, Cout, cin)
    assert_bits(wp.value()[0], cr.pack_head_statement(w), "head pack")


# ---------------------------------------------------------------------------------------------------- folded forward
def fold_layout(c, d, wp=None):
    p = c.pitch
    f = dict(in_mode=_hip.IN_PLAIN, B=c.B, Hin=c.H + 4, Win=c.W + 4, C0=c.C0, stride=1, Cout=c.Cout, Ho=c.H, Wo=c.W, HoF=2 * c.H, WoF=2 * c.W,
             osy=1, osx=1, ooy=0, oox=0, epi=c.epi, beta=0.0, algo=ALGO[c.fam], frame=c.frame, **_taps(cr.fold_taps(0, 0)))
    f["x0"], f["ld0"] = In(d.x0, ld=c.C0 + p), c.C0 + p
    f["w"] = pack_fold(d.w5, c.fam) if wp is None else wp
    if d.bias is not None:
        f["bias"] = In(d.bias)
    out = Out(c.B * 4 * c.H * c.W, c.Cout, ld=c.Cout + p)
    f["out"], f["ldo"] = out, c.Cout + p
    if c.frame:
        w = c.frame * c.Cout
        f["e0"], f["lde0"], f["e1"], f["lde1"] = In(d.e0, ld=w + p), w + p, In(d.e1, ld=w + 2 * p), w + 2 * p
    return f, out


def judge(c, st, out, what):
    got = out.value()
    ref = st.out.reshape(got.shape)
    assert bool(torch.isfinite(got).all()), "%s: not finite" % what
    if c.kind == "int":
        assert_exact(got, ref, what)
    else:
        keep = ~st.kink.reshape(got.shape)
        assert_within(got[keep], ref[keep], st.b_out.reshape(got.shape)[keep], what)


@pytest.mark.parametrize("c", fh.FOLD, ids=lambda c: c.name)
def test_fold_forward(c):
    """RAMNET_ALGO_WINOGRAD24 / _2X3 forward: every instantiation by ramnet_last_kernel, `frame` on every border pixel (side and slot of e0 /
    e1, corners with both), the pair form's shifted tiling at both edges, ragged tiles, surplus workgroups, pitched operands"""
    L = _hip.lib()
    d = fh.build_fold(c)
    st = cr.fold_statement(d, c.fam, pair=fh.is_pair(c))
    if c.kind == "int":
        assert cr.fold_exact_ok(st, c.fam)
    with option(b"fold_pair", c.fold_pair):
        f, out = fold_layout(c, d)
        if c.fam == "fold2x3":
            assert L.ramnet_fold_wino_variant(C.byref(_struct(_hip.ConvDesc, dict(f, algo=_hip.ALGO_WINOGRAD24))), 1) == 1
        call_desc("ramnet_conv_launch", _hip.ConvDesc, f)
    assert L.ramnet_last_kernel().decode() == c.kernel
    judge(c, st, out, "%s on %s" % (c.name, c.fam))


@pytest.mark.parametrize("ksplit,C0", [(2, 64), (3, 192), (4, 128)])
def test_fold_split_reduction(ksplit, C0):
    """option wino_ksplit forced on a 5 x 6 map (4 workgroups): the partial tiles meet in the workspace, the last arrival joins them in split
    order: exact on integers, bit-equal across two launches on one workspace, arrival counters back at zero, workspace inside its guards"""
    L = _hip.lib()
    c = fh._fold("ksplit%d" % ksplit, "fold2x2", 1, 5, 6, C0, 64, "conv_wino24_kernel<4,0,4,0>", wd=0.125, xd=0.25)
    d = fh.build_fold(c)
    st = cr.fold_statement(d, c.fam)
    assert cr.fold_exact_ok(st, c.fam)
    with option(b"wino_ksplit", ksplit):
        f, out = fold_layout(c, d)
        n = L.ramnet_conv_splitk_floats(C.byref(_struct(_hip.ConvDesc, f)))
        assert n == 64 + 4 * ksplit * 8192, "4 workgroups x %d splits" % ksplit
        ws = Out(1, n, prefill=torch.zeros(n))
        f["splitk_ws"], f["splitk_floats"] = ws, n
        call_desc("ramnet_conv_launch", _hip.ConvDesc, f)
        assert L.ramnet_last_kernel().decode() == c.kernel
        first = out.value()
        assert_exact(first, st.out.reshape(first.shape), "split reduction x%d" % ksplit)
        assert not bool(ws.value()[0, :64].view(torch.int32).any()), "arrival counters must be left at zero"
        assert bool(ws.value()[0, 64:].abs().max() > 0), "the partial tiles went through the workspace"
        f2, out2 = fold_layout(c, d, wp=f["w"])
        f2["splitk_ws"], f2["splitk_floats"] = ws, n
        call_desc("ramnet_conv_launch", _hip.ConvDesc, f2)
        assert_bits(out2.value(), first.double(), "second launch on the same workspace")
        assert not bool(ws.value()[0, :64].view(torch.int32).any())


# ---------------------------------------------------------------------------------------------------- PARITY4 backward-data
# (family, H, W, C0 = the layer's output channels, Cout = its input channels, kernel, kind)
DGRAD = [("fold2x2", 2, 2, 16, 64, "conv_wino24_kernel<4,1,4,0>", "int"), ("fold2x2", 13, 4, 16, 64, "conv_wino24_kernel<4,1,4,0>", "int"),
         ("fold2x2", 3, 20, 16, 64, "conv_wino24_kernel<4,1,8,0>", "int"), ("fold2x2", 5, 7, 32, 128, "conv_wino24_kernel<4,1,4,0>", "normal"),
         ("fold2x3", 9, 6, 16, 64, "conv_wino24_kernel<4,1,4,0,3>", "int"), ("fold2x3", 20, 2, 16, 64, "conv_wino24_kernel<4,1,2,0,3>", "int"),
         ("fold2x3", 2, 40, 16, 64, "conv_wino24_kernel<4,1,16,0,3>", "int"), ("fold2x3", 7, 9, 32, 64, "conv_wino24_kernel<4,1,4,0,3>", "normal")]


@pytest.mark.parametrize("fam,H,W,C0,Cout,kernel,kind", DGRAD, ids=["%s-%dx%d-%s" % (r[0], r[1], r[2], r[6]) for r in DGRAD])
def test_fold_backward_data(fam, H, W, C0, Cout, kernel, kind):
    """RAMNET_IN_PARITY4: the gradient of the padded low-res tensor on its whole (H + 4) x (W + 4) grid from the full-resolution gradient
    (the four parity sub-grids as reduction blocks, zero outside), every element written (sentinel prefill), B = 2, pitched"""
    L = _hip.lib()
    g = fh._gen("dgrad%s%dx%d" % (fam, H, W))
    B, p = 2, 4
    if kind == "int":
        gy, w5 = fh._sparse(g, (B, 2 * H, 2 * W, C0), 1, 0.25), 9.0 * fh._sparse(g, (C0, Cout, 5, 5), 1, 0.125)
    else:
        gy, w5 = fh._rn(g, (B, 2 * H, 2 * W, C0)), fh._rn(g, (C0, Cout, 5, 5), 0.05)
    taps, Wt = cr.parity4_taps_weights(w5)
    d = types.SimpleNamespace(in_mode=cr.IN_PARITY4, x0=gy)
    ref, _ = cr.reduction(cr.logical_input(d), Wt, taps, 1, H + 4, W + 4)
    rabs = cr.parity4_wino(gy, w5, fam)
    f = dict(in_mode=_hip.IN_PARITY4, B=B, Hin=2 * H, Win=2 * W, C0=C0, ld0=C0 + p, x0=In(gy, ld=C0 + p), stride=1, Cout=Cout, Ho=H + 4, Wo=W + 4,
             HoF=H + 4, WoF=W + 4, osy=1, osx=1, epi=_hip.EPI_LINEAR, beta=0.0, algo=ALGO[fam], w=pack_fold(w5, fam, dgrad=True), **_taps(cr.fold_taps(0, 0)))
    out = Out(B * (H + 4) * (W + 4), Cout, ld=Cout + p)
    f["out"], f["ldo"] = out, Cout + p
    if fam == "fold2x3":
        assert L.ramnet_fold_wino_variant(C.byref(_struct(_hip.ConvDesc, dict(f, algo=_hip.ALGO_WINOGRAD24))), 1) == 1
    call_desc("ramnet_conv_launch", _hip.ConvDesc, f)
    assert L.ramnet_last_kernel().decode() == kernel
    got = out.value()
    assert bool(torch.isfinite(got).all())
    if kind == "int":
        assert float(rabs.max()) * 2.0 ** cr.GRID_BITS[fam] < 2 ** 24
        assert_exact(got, ref.reshape(got.shape), "PARITY4 %s" % fam)
    else:
        assert_within(got, ref, (4 * C0 + cr.R_TRANSFORMS[fam] + 2) * U * rabs, "PARITY4 %s" % fam)


# ---------------------------------------------------------------------------------------------------- folded backward-weights
# (family, B, H, W, C0, Cout, gmask, dbias, which Winograd workspaces the unpack gets besides this launch's, kind): the four (GM, WCI) of each
# kernel; tile counts below, at and above one batch (8 tiles of F(2x2), 6 of F(2x3)); more batches than splits (256 / workgroups per split)
FWG = [("fold2x2", 1, 2, 2, 32, 64, False, True, "none", "int"), ("fold2x2", 1, 4, 8, 32, 64, True, False, "other", "int"),
       ("fold2x2", 1, 6, 6, 64, 32, False, True, "none", "int"), ("fold2x2", 4, 16, 18, 128, 32, True, True, "other", "int"),
       ("fold2x2", 2, 16, 18, 64, 128, True, True, "none", "normal"),
       ("fold2x3", 1, 2, 3, 32, 64, False, True, "none", "int"), ("fold2x3", 1, 4, 9, 32, 64, True, False, "other", "int"),
       ("fold2x3", 1, 2, 21, 64, 32, False, True, "none", "int"), ("fold2x3", 3, 16, 26, 128, 32, True, True, "other", "int"),
       ("fold2x3", 2, 16, 26, 64, 128, True, True, "none", "normal")]


@pytest.mark.parametrize("row", FWG, ids=["%s-B%d-%dx%d-%d_%d-gm%d" % r[:7] for r in FWG])
def test_fold_wgrad(row):
    """conv_wgrad_wino24_kernel<GM,WCI> / _2x3 and ramnet_fold_unpack_wgrad / ...2x3: the launch's dU (dU3) workspace, then the library's own
    unpack onto a non-zero gradient together with a non-zero direct workspace w4, border-GEMM gradients wr / wc and ("other") the other
    family's Winograd workspace; exact on integers (the folded gradient is an integer, the transformed-domain sums stay below 2^24 on their
    grid), derived on normal data; every workspace comes back zero"""
    L = _hip.lib()
    fam, B, H, W, C0, Cout, gm, want_bias, others, kind = row
    g = fh._gen("fwg" + "%s%d%d%d" % (fam, H, W, C0))
    integer = kind == "int"
    mk = (lambda s, m=1, dens=0.5: fh._sparse(g, s, m, dens)) if integer else (lambda s, m=1, dens=0.5: fh._rn(g, s))
    d = types.SimpleNamespace(x0=mk((B, H + 4, W + 4, C0)), dout=mk((B, 2 * H, 2 * W, Cout), 2), gmask=mk((B, 2 * H, 2 * W, Cout)) if gm else None, Ho=H, Wo=W)
    st = cr.fold_wgrad_statement(d)
    dUabs, fabs, ntiles = cr.fold_wgrad_wino(d, fam)
    NP = 5 * (cr.FOLD_TW[fam] + 3)
    n = 4 * NP * C0 * Cout
    dw = Out(1, n, prefill=torch.zeros(n))
    dbias = Out(1, Cout, prefill=torch.zeros(Cout)) if want_bias else None
    f = dict(x0=In(d.x0, ld=C0 + 4), ld0=C0 + 4, C0=C0, in_mode=_hip.IN_PLAIN, B=B, Hin=H + 4, Win=W + 4, stride=1, dout=In(d.dout, ld=Cout + 4), ldg=Cout + 4,
             Cout=Cout, Ho=H, Wo=W, HoG=2 * H, WoG=2 * W, dw=dw, algo=ALGO[fam], ntaps=16, dy=[t[0] for t in cr.fold_taps(0, 0)], dx=[t[1] for t in cr.fold_taps(0, 0)])
    if gm:
        f["gmask"], f["ldgm"] = In(d.gmask, ld=Cout + 8), Cout + 8
    if want_bias:
        f["dbias"] = dbias
    if fam == "fold2x3":
        assert L.ramnet_fold_wgrad_variant(C.byref(_struct(_hip.WgradDesc, dict(f, algo=_hip.ALGO_WINOGRAD24))), 1) == 1
    call_desc("ramnet_wgrad_launch", _hip.WgradDesc, f)
    assert L.ramnet_last_kernel().decode() == "conv_wgrad_wino24_kernel%s<%d,%d>" % ("_2x3" if fam == "fold2x3" else "", int(gm), int(Cout % 64 != 0))
    if integer:
        assert float(dUabs.max()) * 2.0 ** cr.WGRAD_GRID_BITS[fam] < 2 ** 24 and torch.equal(st.dW4, st.dW4.round())
    if want_bias:
        if integer:
            assert_exact(dbias.value()[0], st.dbias, "fold wgrad dbias", abs_sum=st.dbias_abs)
        else:
            assert_within(dbias.value()[0], st.dbias, (st.n_bias + 2) * U * st.dbias_abs, "fold wgrad dbias")
    # ---- the library's own unpack: this launch's workspace, a direct workspace, border gradients, optionally the other family's workspace
    ints = (lambda s, m: fh._ri(g, s, m)) if integer else (lambda s, m: fh._rn(g, s))
    gold, w4v = ints((Cout, C0, 5, 5), 8), ints((4, 16, C0, Cout), 4)
    wrv, wcv = ints((2, 5 * C0, 2 * Cout), 4), ints((2, 5 * C0, 2 * Cout), 4)
    grad = Out(1, gold.numel(), prefill=gold.reshape(-1))
    w4, wr, wc = Out(1, w4v.numel(), prefill=w4v.reshape(-1)), Out(1, wrv.numel(), prefill=wrv.reshape(-1)), Out(1, wcv.numel(), prefill=wcv.reshape(-1))
    other_fam = "fold2x3" if fam == "fold2x2" else "fold2x2"
    extra, other = torch.zeros(4, 16, C0, Cout, dtype=F64), None
    if others == "other":                           # a second Winograd workspace holding an integer dU of its own: e_(0,0) e_(0,0)^T folds to G[0][t] Gc[0][s]
        NPo = 5 * (cr.FOLD_TW[other_fam] + 3)
        ov = torch.zeros(4, NPo, C0, Cout, dtype=F64)
        ov[:, 0] = 4.0 * ints((4, C0, Cout), 2)
        other = Out(1, ov.numel(), prefill=ov.reshape(-1))
        Gr, Gc = cr.WINO[other_fam][1], cr.WINO[other_fam][4]
        extra = torch.einsum("t,s,zkn->ztskn", Gr[0], Gc[0], ov[:, 0]).reshape(4, 16, C0, Cout)
    dU2, dU3 = (dw, other) if fam == "fold2x2" else (other, dw)
    if dU3 is None:
        call("ramnet_fold_unpack_wgrad", w4, dU2, wr, wc, grad, Cout, C0, C0)
    else:
        call("ramnet_fold_unpack_wgrad2x3", w4, dU2, dU3, wr, wc, grad, Cout, C0, C0)
    ref = cr.fold_unpack_statement(gold, st.dW4 + extra, w4v, wrv, wcv)
    got = grad.value()
    if integer:
        assert_exact(got, ref.reshape(got.shape), "%s gradient after the fold's unpack" % fam)
    else:
        FA = cr.fold_matrix()
        babs = torch.einsum("ptk,qsl,pqtsio->oikl", FA, FA, ((ntiles + cr.R_WGRAD[fam] + 2) * U * fabs + U * w4v.abs()).view(2, 2, 4, 4, C0, Cout))
        bound = babs + 2 * U * ref.abs()            # (the fold itself runs in double: one rounding of the sum, one of the +=)
        assert_within(got, ref, bound, "%s gradient after the fold's unpack" % fam)
    for buf, what in ((dw, "dU"), (w4, "w4"), (wr, "wr"), (wc, "wc"), (other, "the other workspace")):
        if buf is not None:
            assert not bool(_bits(buf.value()).any()), "%s must come back +0" % what


# ---------------------------------------------------------------------------------------------------- head
def head_fields(c, d):
    p = c.pitch
    return dict(in_mode=_hip.IN_PLAIN, B=c.B, Hin=c.H, Win=c.W, C0=c.C0, ld0=c.C0 + p, x0=In(d.x0_phys, ld=c.C0 + p), stride=1, Cout=c.Cout, Ho=c.H, Wo=c.W,
                algo=_hip.ALGO_HEAD, head_cin=c.cin)


@pytest.mark.parametrize("c", fh.HEAD, ids=lambda c: c.name)
def test_head_forward(c):
    """conv_head_fwd_kernel<1 | 3 | 5 | 10>: maps of one pixel, exact tiles (16 x 32), one row / column more, a 5 x 70 strip; Cout 32, 20, 8;
    padded input channels that must not reach the result; pitched x0 / out"""
    L = _hip.lib()
    d = fh.build_head(c)
    st = cr.conv_statement(d, "direct")
    wp = Out(1, L.ramnet_packed_weight_elems_head(c.cin))
    call("ramnet_pack_weight_head", In(d.w_oihw.reshape(-1)), wp, c.Cout, c.cin)
    out = Out(c.B * c.H * c.W, c.Cout, ld=c.Cout + c.pitch)
    f = dict(head_fields(c, d), w=wp.freeze(), out=out, ldo=c.Cout + c.pitch, HoF=c.H, WoF=c.W, osy=1, osx=1, epi=c.epi, beta=0.0, **_taps(fh.HEAD_TAPS))
    if d.bias is not None:
        f["bias"] = In(d.bias)
    call_desc("ramnet_conv_launch", _hip.ConvDesc, f)
    assert L.ramnet_last_kernel().decode() == "conv_head_fwd_kernel<%d>" % c.cin
    judge(c, st, out, "head %s" % c.name)


@pytest.mark.parametrize("c", fh.HEAD + [fh.HEAD_BIG], ids=lambda c: c.name)
def test_head_wgrad(c):
    """conv_head_wgrad_kernel<CR>: dw [25][C0][Cout] (rows of the padded channels stay zero) and dbias by atomics, gmask / dbias given and absent,
    pitched x0 / dout / gmask; the last row has 527 tiles (a second trip of the 512 persistent workgroups); then ramnet_unpack_wgrad with n_off != 0"""
    L = _hip.lib()
    d = fh.build_head(c)
    st = cr.wgrad_statement(types.SimpleNamespace(**dict(vars(d), taps=[t[:2] for t in d.taps])))
    p = c.pitch
    dw = Out(25 * c.C0, c.Cout, prefill=torch.zeros(25 * c.C0, c.Cout))
    dbias = Out(1, c.Cout, prefill=torch.zeros(c.Cout)) if c.dbias else None
    f = dict(head_fields(c, d), dout=In(d.dout, ld=c.Cout + p), ldg=c.Cout + p, dw=dw, ntaps=25, dy=[t[0] for t in fh.HEAD_TAPS], dx=[t[1] for t in fh.HEAD_TAPS])
    if d.gmask is not None:
        f["gmask"], f["ldgm"] = In(d.gmask, ld=c.Cout + p + 4), c.Cout + p + 4
    if c.dbias:
        f["dbias"] = dbias
    call_desc("ramnet_wgrad_launch", _hip.WgradDesc, f)
    assert L.ramnet_last_kernel().decode() == "conv_head_wgrad_kernel<%d>" % c.cin
    ref = torch.zeros(25, c.C0, c.Cout, dtype=F64)
    ref[:, :c.cin] = st.dW
    rabs = torch.zeros_like(ref)
    rabs[:, :c.cin] = st.dW_abs
    what = "head wgrad %s" % c.name
    if c.kind == "int":
        assert_exact(dw.value(), ref.reshape(25 * c.C0, c.Cout), what + " dW", abs_sum=rabs.reshape(25 * c.C0, c.Cout))
        if c.dbias:
            assert_exact(dbias.value()[0], st.dbias, what + " dbias", abs_sum=st.dbias_abs)
    else:
        assert_within(dw.value(), ref, (float(st.n.max()) + cr.R_WGRAD["direct"] + 2) * U * rabs, what + " dW")
        if c.dbias:
            assert_within(dbias.value()[0], st.dbias, (st.n_bias + 2) * U * st.dbias_abs, what + " dbias")
    if c.kind == "int":                             # the window [n_off, n_off + Cn) of the output channels onto a non-zero gradient
        n_off, Cn = 4, c.Cout - 4
        gold = fh._ri(fh._gen("gold" + c.name), (Cn, c.cin, 5, 5), 8)
        grad = Out(1, gold.numel(), prefill=gold.reshape(-1))
        call("ramnet_unpack_wgrad", dw.freeze(), grad, Cn, c.cin, c.C0, c.Cout, n_off, 5, 5)
        assert_exact(grad.value(), cr.unpack_statement(gold, ref, Cn, c.cin, n_off).reshape(1, -1), what + " after ramnet_unpack_wgrad")


# ---------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks():
    """every refusal: RAMNET_E_BADARG with a message, all outputs untouched (none of these descriptors is ever launched)"""
    L = _hip.lib()
    for name in ("tall_9x5", "pair_tall_9x5", "tx4_9x10", "pair_tx4_9x10"):
        c = fh.FOLD_BY_NAME[name]
        d = fh.build_fold(c)
        f, out = fold_layout(c, d)
        out.freeze()
        for e in (dict(ld0=c.C0 - 4), dict(ldo=c.Cout - 4), dict(lde0=2 * c.Cout - 4), dict(lde1=2 * c.Cout - 4), dict(frame=3), dict(ld0=0),
                  dict(HoF=2 * c.H + 2), dict(Hin=c.H + 3), dict(beta=1.0), dict(frame=2, e0=None)):
            call_desc("ramnet_conv_launch", _hip.ConvDesc, dict(f, **e), rc=BADARG)
    # backward-data
    fam, H, W, C0, Cout = "fold2x2", 3, 4, 16, 64
    w5 = fh.pack_weights(C0, Cout, "int")
    out = Out(2 * (H + 4) * (W + 4), Cout).freeze()
    f = dict(in_mode=_hip.IN_PARITY4, B=2, Hin=2 * H, Win=2 * W, C0=C0, ld0=C0, x0=In(torch.zeros(2, 2 * H, 2 * W, C0)), stride=1, Cout=Cout, Ho=H + 4, Wo=W + 4,
             HoF=H + 4, WoF=W + 4, osy=1, osx=1, epi=_hip.EPI_LINEAR, beta=0.0, algo=ALGO[fam], w=pack_fold(w5, fam, dgrad=True), out=out, ldo=Cout,
             **_taps(cr.fold_taps(0, 0)))
    for e in (dict(ld0=C0 - 4), dict(ldo=Cout - 4), dict(Ho=H + 5), dict(frame=2)):
        call_desc("ramnet_conv_launch", _hip.ConvDesc, dict(f, **e), rc=BADARG)
    # head forward and backward-weights
    c = fh.HEAD[4]
    d = fh.build_head(c)
    wp = Out(1, L.ramnet_packed_weight_elems_head(c.cin))
    call("ramnet_pack_weight_head", In(d.w_oihw.reshape(-1)), wp, c.Cout, c.cin)
    out = Out(c.B * c.H * c.W, c.Cout, ld=c.Cout + c.pitch).freeze()
    f = dict(head_fields(c, d), w=wp.freeze(), out=out, ldo=c.Cout + c.pitch, HoF=c.H, WoF=c.W, osy=1, osx=1, epi=c.epi, beta=0.0, **_taps(fh.HEAD_TAPS))
    for e in (dict(ld0=4), dict(ldo=c.Cout - 4), dict(head_cin=4), dict(head_cin=10), dict(Cout=36), dict(frame=2)):
        call_desc("ramnet_conv_launch", _hip.ConvDesc, dict(f, **e), rc=BADARG)
    dw = Out(25 * c.C0, 32, prefill=torch.zeros(25 * c.C0, 32)).freeze()
    g = dict(head_fields(c, d), dout=In(d.dout, ld=c.Cout + 4), ldg=c.Cout + 4, dw=dw, ntaps=25, dy=[t[0] for t in fh.HEAD_TAPS], dx=[t[1] for t in fh.HEAD_TAPS])
    for e in (dict(Cout=30), dict(ldg=c.Cout - 4), dict(ld0=4), dict(gmask=In(d.dout), ldgm=c.Cout - 4), dict(ldg=c.Cout + 2), dict(HoG=c.H, WoG=c.W, gsy=1, gsx=1)):
        call_desc("ramnet_wgrad_launch", _hip.WgradDesc, dict(g, **e), rc=BADARG)
    # the fold's unpack takes the Winograd workspaces as optional, the direct workspace w4 and the border gradients not
    C0, Cout = 32, 32
    bufs = [Out(1, n, prefill=torch.ones(n)).freeze() for n in (64 * C0 * Cout, 100 * C0 * Cout, 20 * C0 * Cout, 20 * C0 * Cout, 25 * C0 * Cout)]
    w4, dU, wr, wc, grad = bufs
    for args in ((None, dU, wr, wc, grad), (w4, dU, None, wc, grad), (w4, dU, wr, wc, None)):
        call("ramnet_fold_unpack_wgrad", *args, Cout, C0, C0, rc=BADARG)
    call("ramnet_fold_unpack_wgrad", w4, dU, wr, wc, grad, Cout, C0, C0 - 4, rc=BADARG)          # CinWs < Cin
    for b in bufs:
        b.check("ramnet_fold_unpack_wgrad", untouched=True)
    # `frame` on the direct family: the operands' leading dimensions and bands that would meet
    B, H, W, Cin, Cout = 1, 3, 4, 8, 32
    w = Out(1, L.ramnet_packed_weight_elems(Cout, Cin, 4, 4, 0, 1))
    call("ramnet_pack_weight", In(torch.zeros(Cout * Cin * 16)), w, Cout, Cin, 4, 4, 0, 1)
    out = Out(B * 4 * H * W, Cout)
    f = dict(in_mode=_hip.IN_PLAIN, B=B, Hin=H + 4, Win=W + 4, C0=Cin, ld0=Cin, x0=In(torch.zeros(B, H + 4, W + 4, Cin)), stride=1, Cout=Cout, Ho=H, Wo=W,
             HoF=2 * H, WoF=2 * W, osy=2, osx=2, ooy=1, oox=0, epi=_hip.EPI_RELU, beta=0.0, algo=_hip.ALGO_DIRECT, w=w.freeze(), out=out, ldo=Cout, frame=2,
             e0=In(torch.zeros(2, B, 2 * H, 2 * Cout)), lde0=2 * Cout, e1=In(torch.zeros(2, B, 2 * W, 2 * Cout)), lde1=2 * Cout, **_taps(cr.fold_taps(1, 0)))
    call_desc("ramnet_conv_launch", _hip.ConvDesc, f)                        # (the descriptor itself is fine)
    out.freeze()
    for e in (dict(lde0=2 * Cout - 4), dict(lde1=Cout), dict(frame=4)):
        call_desc("ramnet_conv_launch", _hip.ConvDesc, dict(f, **e), rc=BADARG)


# ---------------------------------------------------------------------------------------------------- direct kernel: UP2X loaders, folded classes
def _direct_pack(w_oihw, k):
    L = _hip.lib()
    O, I = w_oihw.shape[:2]
    wp = Out(1, L.ramnet_packed_weight_elems(O, I, k, k, 0, 1))
    call("ramnet_pack_weight", In(w_oihw.reshape(-1)), wp, O, I, k, k, 0, 1)
    return wp.freeze()


@pytest.mark.parametrize("H2,W2", [(2, 2), (10, 14), (18, 34)])
@pytest.mark.parametrize("mode", [cr.IN_UP2X, cr.IN_UP2X_SKIP])
def test_direct_up2x(mode, H2, W2):
    """RAMNET_IN_UP2X / _UP2X_SKIP on the direct kernel, 5x5 stride 1 over the upsampled map (Hin, Win = the extent after the x2), forward and
    ramnet_wgrad_launch: integer sources make the bilinear samples multiples of 1/16, so both are exact; x1 pitched"""
    L = _hip.lib()
    B, C0, Cout, k = 2, 8, 32, 5
    g = fh._gen("up2x%d_%d_%d" % (mode, H2, W2))
    taps = [(a - 2, b - 2, a * 5 + b) for a in range(5) for b in range(5)]
    w = fh._sparse(g, (Cout, C0, k, k), 2, 0.5)
    d = types.SimpleNamespace(in_mode=mode, Hin=H2, Win=W2, B=B, C0=C0, C1=0, Cin=C0, Cout=Cout, N=Cout, stride=1, epi=cr.EPI_RELU, beta=0.0, out_s2d=0,
                              x0=fh._sparse(g, (B, H2 // 2, W2 // 2, C0), 2, 0.5), x1=fh._sparse(g, (B, H2 // 2, W2 // 2, C0), 2, 0.5) if mode == cr.IN_UP2X_SKIP else None,
                              xm=None, bias=fh._ri(g, (Cout,), 8), e0=None, e1=None, out_old=None, active=None, W=w.permute(2, 3, 1, 0).reshape(25, C0, Cout).contiguous(),
                              taps=taps, Ho=H2, Wo=W2, HoF=H2, WoF=W2, os=(1, 1, 0, 0), dout=fh._sparse(g, (B, H2, W2, Cout), 2, 0.5), gmask=None)
    st = cr.conv_statement(d, "direct")
    assert cr.exact_ok(st, "direct")
    out = Out(B * H2 * W2, Cout, ld=Cout + 4)
    f = dict(in_mode=mode, B=B, Hin=H2, Win=W2, C0=C0, ld0=C0, x0=In(d.x0), stride=1, Cout=Cout, Ho=H2, Wo=W2, HoF=H2, WoF=W2, osy=1, osx=1, epi=cr.EPI_RELU,
             beta=0.0, algo=_hip.ALGO_DIRECT, w=_direct_pack(w, k), bias=In(d.bias), out=out, ldo=Cout + 4, **_taps(taps))
    if d.x1 is not None:
        f["x1"], f["ld1"] = In(d.x1, ld=C0 + 4), C0 + 4
    call_desc("ramnet_conv_launch", _hip.ConvDesc, f)
    assert L.ramnet_last_kernel().decode().startswith("conv_igemm_kernel<")
    assert_exact(out.value(), st.out.reshape(-1, Cout), "UP2X mode %d forward" % mode)
    wst = cr.wgrad_statement(types.SimpleNamespace(**dict(vars(d), taps=[t[:2] for t in taps])))
    dw, dbias = Out(25 * C0, Cout, prefill=torch.zeros(25 * C0, Cout)), Out(1, Cout, prefill=torch.zeros(Cout))
    gf = dict(in_mode=mode, B=B, Hin=H2, Win=W2, C0=C0, ld0=C0, x0=f["x0"], stride=1, Cout=Cout, Ho=H2, Wo=W2, dout=In(d.dout, ld=Cout + 4), ldg=Cout + 4, dw=dw,
              dbias=dbias, algo=_hip.ALGO_DIRECT, ntaps=25, dy=[t[0] for t in taps], dx=[t[1] for t in taps])
    if d.x1 is not None:
        gf["x1"], gf["ld1"] = f["x1"], C0 + 4
    call_desc("ramnet_wgrad_launch", _hip.WgradDesc, gf)
    assert_exact(dw.value(), wst.dW.reshape(25 * C0, Cout), "UP2X mode %d dW" % mode, abs_sum=wst.dW_abs.reshape(25 * C0, Cout))
    assert_exact(dbias.value()[0], wst.dbias, "UP2X mode %d dbias" % mode, abs_sum=wst.dbias_abs)


@pytest.mark.parametrize("B,H,W", [(1, 2, 2), (3, 5, 9)])
def test_direct_folded_classes_with_frame(B, H, W):
    """the `folded_direct` path: the four 4x4 parity classes of the fold as ONE ramnet_conv_launch_multi on the 64 slices (py, px, t, s) with
    frame = 2, and their backward-weights through gsy = gsx = 2, goy, gox, HoG, WoG: exact on integers (5x5 weights 16 x integers: W4 integral)"""
    L = _hip.lib()
    Cin, Cout = 8, 32
    g = fh._gen("folded_direct%d" % H)
    w5 = 16.0 * fh._sparse(g, (Cout, Cin, 5, 5), 1, 0.5)
    W4 = cr.fold_w4(w5)                                                             # [n][c][py][px][t][s]
    assert torch.equal(W4, W4.round())
    xpad = fh._sparse(g, (B, H + 4, W + 4, Cin), 2, 0.5)
    bias, e0, e1 = fh._ri(g, (Cout,), 8), fh._ri(g, (2, B, 2 * H, 2 * Cout), 8), fh._ri(g, (2, B, 2 * W, 2 * Cout), 8)
    dout = fh._sparse(g, (B, 2 * H, 2 * W, Cout), 2, 0.5)
    Wsl = W4.permute(2, 3, 4, 5, 1, 0).reshape(64, Cin, Cout).contiguous()
    x0, out = In(xpad, ld=Cin + 4), Out(B * 4 * H * W, Cout, ld=Cout + 4)
    wp, be0, be1, bb = _direct_pack(W4.reshape(Cout, Cin, 8, 8), 8), In(e0, ld=2 * Cout + 4), In(e1), In(bias)
    descs, ref = [], torch.zeros(B, 2 * H, 2 * W, Cout, dtype=F64)
    for py in range(2):
        for px in range(2):
            taps = [(dy, dx, (py * 2 + px) * 16 + t) for dy, dx, t in cr.fold_taps(py, px)]
            d = types.SimpleNamespace(in_mode=cr.IN_PLAIN, x0=xpad, W=Wsl, taps=taps, stride=1, Ho=H, Wo=W, HoF=2 * H, WoF=2 * W, os=(2, 2, py, px), bias=bias,
                                      epi=cr.EPI_RELU, beta=0.0, e0=e0, e1=e1, frame=2, out_old=None, active=None, out_s2d=0, Cout=Cout)
            st = cr.conv_statement(d, "direct")
            assert cr.exact_ok(st, "direct")
            ref = ref + st.out * st.w_out
            descs.append(dict(x0=x0, ld0=Cin + 4, C0=Cin, in_mode=_hip.IN_PLAIN, B=B, Hin=H + 4, Win=W + 4, stride=1, w=wp, bias=bb, Cout=Cout, Ho=H, Wo=W,
                              HoF=2 * H, WoF=2 * W, osy=2, osx=2, ooy=py, oox=px, epi=_hip.EPI_RELU, out=out, ldo=Cout + 4, algo=_hip.ALGO_DIRECT, frame=2,
                              e0=be0, lde0=2 * Cout + 4, e1=be1, lde1=2 * Cout, **_taps(taps)))
    call_desc("ramnet_conv_launch_multi", _hip.ConvDesc, descs)
    assert_exact(out.value(), ref.reshape(-1, Cout), "four folded classes with frame in one launch")
    # backward-weights of each class: the parity sub-grid of the full-resolution gradient
    gin = In(dout, ld=Cout + 4)
    for py in range(2):
        for px in range(2):
            taps = cr.fold_taps(py, px)
            wst = cr.wgrad_statement(cr.fold_class_wgrad(types.SimpleNamespace(x0=xpad, dout=dout, gmask=None, Ho=H, Wo=W), py, px))
            dw = Out(16 * Cin, Cout, prefill=torch.zeros(16 * Cin, Cout))
            gf = dict(in_mode=_hip.IN_PLAIN, B=B, Hin=H + 4, Win=W + 4, C0=Cin, ld0=Cin + 4, x0=x0, stride=1, Cout=Cout, Ho=H, Wo=W, dout=gin, ldg=Cout + 4, dw=dw,
                      algo=_hip.ALGO_DIRECT, ntaps=16, dy=[t[0] for t in taps], dx=[t[1] for t in taps], gsy=2, gsx=2, goy=py, gox=px, HoG=2 * H, WoG=2 * W)
            call_desc("ramnet_wgrad_launch", _hip.WgradDesc, gf)
            assert_exact(dw.value(), wst.dW.reshape(16 * Cin, Cout), "class (%d, %d) dW through gsy / HoG" % (py, px), abs_sum=wst.dW_abs.reshape(16 * Cin, Cout))


# ---------------------------------------------------------------------------------------------------- the whole folded layer through the C ABI
@pytest.mark.parametrize("fam,Cout,pair", [("fold2x2", 64, 1), ("fold2x3", 64, 1), ("fold2x2", 32, 1), ("fold2x3", 32, 1)])
def test_folded_layer_composition(fam, Cout, pair):
    """ramnet_pad2_sum_im2col -> ramnet_pack_border_weights -> ramnet_gemm2 -> the folded launch with frame = 2 against
    relu(conv5x5, zero-padded, of up2x(x + skip) + b) in float64 on the WHOLE image; integer data (weights 9 x integers) keep every stage on
    a dyadic grid, so the comparison is exact.  Once per fold family and on the pair form of each."""
    import torch.nn.functional as F
    L = _hip.lib()
    B, H, W, Cin = 2, 5, 7, 32
    g = fh._gen("composition%s%d" % (fam, Cout))
    x, skip = fh._sparse(g, (B, H, W, Cin), 1, 0.2), fh._sparse(g, (B, H, W, Cin), 1, 0.2)
    w5, bias = 9.0 * fh._sparse(g, (Cout, Cin, 5, 5), 1, 0.125), fh._ri(g, (Cout,), 8)
    up = F.interpolate((x + skip).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
    ref = F.conv2d(up, w5, bias, 1, 2).permute(0, 2, 3, 1).clamp_min(0)
    H2, W2 = 2 * H, 2 * W
    xpad, a_rows, a_cols = Out(B * (H + 4) * (W + 4), Cin), Out(2 * B * W2, 5 * Cin), Out(2 * B * H2, 5 * Cin)
    call("ramnet_pad2_sum_im2col", In(x), In(skip), xpad, a_rows, a_cols, B, H, W, Cin)
    assert_exact(xpad.value(), cr.pad2(x + skip).reshape(-1, Cin), "pad2_sum")
    n = 2 * 5 * Cin * 2 * Cout
    bw = [Out(1, n) for _ in range(4)]
    call("ramnet_pack_border_weights", In(w5.reshape(-1)), *bw, Cout, Cin)
    g_rows, g_cols = Out(2 * B * W2, 2 * Cout), Out(2 * B * H2, 2 * Cout)
    call("ramnet_gemm2", a_rows.freeze(), bw[0].freeze(), g_rows, B * W2, B * W2 * 5 * Cin, 5 * Cin * 2 * Cout, B * W2 * 2 * Cout, 2,
         a_cols.freeze(), bw[1].freeze(), g_cols, B * H2, B * H2 * 5 * Cin, 5 * Cin * 2 * Cout, B * H2 * 2 * Cout, 2, 2 * Cout, 5 * Cin, 5 * Cin, 5 * Cin, 2 * Cout,
         2 * Cout, 0, 0)
    e0, e1 = cr.border_operands(x + skip, w5)
    assert_exact(g_cols.value(), e0.reshape(-1, 2 * Cout), "column corrections")
    assert_exact(g_rows.value(), e1.reshape(-1, 2 * Cout), "row corrections")
    d = types.SimpleNamespace(x0=cr.pad2(x + skip), w5=w5, bias=bias, epi=cr.EPI_RELU, frame=2, e0=e0, e1=e1, Ho=H, Wo=W, HoF=H2, WoF=W2, Cout=Cout)
    is_pair = bool(pair) and Cout == 32
    st = cr.fold_statement(d, fam, pair=is_pair)
    assert cr.fold_exact_ok(st, fam) and float((st.out - ref).abs().max()) < 1e-9
    out = Out(B * H2 * W2, Cout)
    with option(b"fold_pair", pair):
        f = dict(in_mode=_hip.IN_PLAIN, B=B, Hin=H + 4, Win=W + 4, C0=Cin, ld0=Cin, x0=xpad.freeze(), stride=1, Cout=Cout, Ho=H, Wo=W, HoF=H2, WoF=W2, osy=1, osx=1,
                 epi=_hip.EPI_RELU, beta=0.0, algo=ALGO[fam], frame=2, w=pack_fold(w5, fam), bias=In(bias), out=out, ldo=Cout, e0=g_cols.freeze(), lde0=2 * Cout,
                 e1=g_rows.freeze(), lde1=2 * Cout, **_taps(cr.fold_taps(0, 0)))
        call_desc("ramnet_conv_launch", _hip.ConvDesc, f)
    assert ("1,3>" in L.ramnet_last_kernel().decode() or L.ramnet_last_kernel().decode().endswith(",1>")) == is_pair
    assert_exact(out.value(), ref.reshape(-1, Cout), "the folded layer on %s" % fam)
