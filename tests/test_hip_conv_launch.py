"""GPU: ramnet_conv_launch / ramnet_conv_launch_multi / ramnet_wgrad_launch called alone through the C ABI, every launch through
guarded.call_desc (sentinel guards and gaps around every output, NaN around every input, packed weights in guarded buffers sized by the
library's own ramnet_packed_weight_elems*), compared element by element with the float64 statement of the descriptor
(tests/conv_restatement.py) under the rules of profiles/conv_launch_tests_notes.md: exact on integer data, derived on normal data,
measured for the cell epilogues, bit for what must not compute.  The rows are tests/conv_launch_cases.py."""
import ctypes as C

import pytest
import torch

import conv_launch_cases as cc
import conv_restatement as cr
import wgrad_plan_cases as cp
from guarded import BADARG, F64, In, Out, _bits, assert_bits, assert_exact, assert_within, call, call_desc
from rpg_ramnet_amd import _hip

pytestmark = pytest.mark.gpu

ALGO = {"direct": _hip.ALGO_DIRECT, "2x2": _hip.ALGO_WINOGRAD, "2x4": _hip.ALGO_WINOGRAD_2X4, "2x4split": _hip.ALGO_WINOGRAD_2X4_SPLIT}
KERNEL = {"direct": "conv_igemm_kernel<", "2x2": "conv_wino_r_kernel<", "2x4": "conv_wino_r6_kernel<", "2x4split": "conv_wino_r6s_kernel<"}
PAIRS = [(c, f) for c in cc.CASES for f in c.fams]


def _struct(f):
    s = _hip.ConvDesc()
    for k, v in f.items():
        if isinstance(v, (In, Out)):
            v = v.ptr
        if isinstance(v, list):
            for j, e in enumerate(v):
                getattr(s, k)[j] = e
        else:
            setattr(s, k, v)
    return s


def pack(d, fam, k):
    """the library's own packer into a guarded buffer of the library's own size: a packer that writes past it fails the guard check"""
    L = _hip.lib()
    O, I = d.w_oihw.shape[:2]
    gates = 4 if d.epi == cr.EPI_LSTM else 1
    tr = int(d.transposed)
    w = In(d.w_oihw.reshape(-1))
    if fam == "direct":
        wp = Out(1, L.ramnet_packed_weight_elems(O, I, k, k, tr, gates))
        call("ramnet_pack_weight", w, wp, O, I, k, k, tr, gates)
    elif fam == "2x2":
        wp = Out(1, L.ramnet_packed_weight_elems_wino(O, I, tr, gates))
        call("ramnet_pack_weight_wino", w, wp, O, I, tr, gates)
    elif fam == "2x4":
        wp = Out(1, L.ramnet_packed_weight_elems_wino2x4_gates(O, I, tr, gates))
        call("ramnet_pack_weight_wino2x4_gates", w, wp, O, I, tr, gates)
    else:
        wp = Out(1, L.ramnet_packed_weight_elems_wino2x4_split(O, I, tr))
        call("ramnet_pack_weight_wino2x4_split", w, wp, O, I, tr)
    return wp.freeze()


def layout(c, d, fam, k=None, out_skew=0, ldo_extra=0, bias_skew=0, e0_skew=0):
    """the descriptor fields of a row with every tensor between guards: pitched by c.pitch, `window` rows with the epilogue operands as
    column windows of wider buffers (u out of [u | r], h.r into the second half of [x | h.r], ...)"""
    p, win = c.pitch, 8 if c.window else 0
    f = dict(in_mode=d.in_mode, B=d.B, Hin=d.Hin, Win=d.Win, C0=d.C0, C1=d.C1 if d.x1 is not None else 0, stride=d.stride, ntaps=len(d.taps),
             dy=[t[0] for t in d.taps], dx=[t[1] for t in d.taps], wtap=[t[2] for t in d.taps], Cout=d.Cout, Ho=d.Ho, Wo=d.Wo, HoF=d.HoF, WoF=d.WoF,
             osy=d.os[0], osx=d.os[1], ooy=d.os[2], oox=d.os[3], epi=d.epi, beta=d.beta, algo=ALGO[fam], out_s2d=d.out_s2d, s2d_5x5=d.s2d_5x5)
    f["x0"], f["ld0"] = In(d.x0, ld=d.C0 + p + win, col0=win), d.C0 + p + win
    if d.x1 is not None:
        f["x1"], f["ld1"] = In(d.x1, ld=d.C1 + p), d.C1 + p
    if d.xm is not None:
        cm = d.xm.shape[3]
        f["xm"], f["ldm"] = In(d.xm, ld=cm + p + win, col0=win), cm + p + win
    f["w"] = pack(d, fam, c.k if k is None else k)
    if d.bias is not None:
        f["bias"] = In(d.bias, skew=bias_skew)
    npix = d.B * d.HoF * d.WoF
    outs = {}
    Co = d.out_s2d if d.out_s2d else d.Cout
    ldo = Co + p + ldo_extra
    outs["out"] = Out(npix, Co, ld=ldo, prefill=d.out_old, skew=out_skew)
    f["out"], f["ldo"] = outs["out"], ldo
    if d.e0 is not None:
        ce = d.e0.shape[3]
        f["e0"], f["lde0"] = In(d.e0, ld=ce + p + win, col0=win, skew=e0_skew), ce + p + win
    if d.e1 is not None:
        ce = d.e1.shape[3]
        f["e1"], f["lde1"] = In(d.e1, ld=ce + p), ce + p
    if d.epi == cr.EPI_SIGMOID_HR:                  # h.r into the second half of [x | h.r]
        Ch = d.Cout // 2
        outs["o1"] = Out(npix, Ch, ld=Ch + p + 2 * win, col0=2 * win, at_window=True)
        f["o1"], f["ldo1"] = outs["o1"], Ch + p + 2 * win
    elif d.epi == cr.EPI_GRU_BLEND or d.epi == cr.EPI_LSTM:
        outs["o1"] = Out(npix, d.Cout, ld=d.Cout + p)
        f["o1"], f["ldo1"] = outs["o1"], d.Cout + p
    elif d.epi == cr.EPI_GRU_BWD:                   # only the channels n >= C of o1 are written: the first half is a gap
        outs["o1"] = Out(npix, d.Cout // 2, ld=d.Cout + p, col0=d.Cout // 2)
        f["o1"], f["ldo1"] = outs["o1"], d.Cout + p
    if d.epi == cr.EPI_LSTM and c.o2:
        outs["o2"] = Out(npix, 4 * d.Cout, ld=4 * d.Cout + p)
        f["o2"], f["ldo2"] = outs["o2"], 4 * d.Cout + p
    if d.active is not None:
        f["active"] = In(d.active, dtype=torch.int32, fill=7)
    return f, outs


def judge(c, d, st, outs, what):
    B = d.B
    for name, ref, bound in (("out", st.out, st.b_out), ("o1", st.o1, st.b_o1), ("o2", st.o2, st.b_o2)):
        if name not in outs:
            continue
        got = outs[name].value()
        if name == "o1" and d.epi == cr.EPI_GRU_BWD:
            ref, bound = ref[..., d.Cout // 2:], bound[..., d.Cout // 2:]
        ref, bound = ref.reshape(got.shape), bound.reshape(got.shape)
        assert bool(torch.isfinite(got).all()), "%s %s: not finite" % (what, name)
        if c.kind == "int":
            assert_exact(got, ref, "%s %s" % (what, name))
            continue
        keep = ~st.kink.reshape(got.shape) if name == "out" else torch.ones_like(got, dtype=torch.bool)
        assert_within(got[keep], ref[keep], bound[keep], "%s %s" % (what, name))
        if d.active is not None:                    # inactive samples: copies bit for bit, zeros as +0
            rows = got.shape[0] // B
            for b in range(B):
                if int(d.active[b]) == 0:
                    assert_bits(got[b * rows:(b + 1) * rows], ref[b * rows:(b + 1) * rows], "%s %s of inactive sample %d" % (what, name, b))


_ST = {}
_REUSED = ("map17x17_B1", "res_relu", "chan36_20", "normal17")        # rows of test_scalar_epilogue


def statement(c, fam):
    """(descriptor, statement) of a row on a family; kept only for the rows that several tests use"""
    if (c.name, fam) in _ST:
        return _ST[(c.name, fam)]
    d = cc.build(c)
    got = (d, cr.conv_statement(d, fam))
    if c.name in _REUSED:
        _ST[(c.name, fam)] = got
    return got


@pytest.mark.parametrize("c,fam", PAIRS, ids=["%s-%s" % (c.name, f) for c, f in PAIRS])
def test_conv_launch(c, fam):
    L = _hip.lib()
    d, st = statement(c, fam)
    f, outs = layout(c, d, fam)
    if fam in ("2x4", "2x4split"):                  # the library's own eligibility question must agree with the launch
        s = _struct(dict(f, algo=_hip.ALGO_WINOGRAD))
        assert L.ramnet_conv_wino_variant(C.byref(s), 1) == 1
        if fam == "2x4split" or c.epi == cr.EPI_LSTM:
            assert L.ramnet_conv_wino_split_ok(C.byref(s), 1) == int(fam == "2x4split")
    call_desc("ramnet_conv_launch", _hip.ConvDesc, f)
    name = L.ramnet_last_kernel().decode()
    judge(c, d, st, outs, "%s on %s" % (c.name, fam))
    assert name.startswith(KERNEL[fam]), name
    if fam == "direct" and c.name in cc.DIRECT_KERNEL:
        assert name == cc.DIRECT_KERNEL[c.name], name
    if fam == "2x2" and c.name in cc.WINO_KERNEL:
        assert name == cc.WINO_KERNEL[c.name], name
    if c.active is not None:
        assert "masked" in name
    if c.name == "s2d8_big_5x5_1":                  # the position skip (kernel <8,1,6,1>, pinned above) against the dense evaluation of the same
        f2, outs2 = layout(c, d, fam)               # filter (<8,0,6,1>): the skipped positions are zeros, so the results agree bit for bit
        f2["s2d_5x5"] = 0
        call_desc("ramnet_conv_launch", _hip.ConvDesc, f2)
        assert L.ramnet_last_kernel().decode() == "conv_wino_r_kernel<8,0,6,1>"
        assert_bits(outs2["out"].value(), outs["out"].value().double(), "s2d_5x5 0 against 1")


# ---------------------------------------------------------------------------------------------------- scalar epilogues
SKEWS = [("out_skew", dict(out_skew=1)), ("ldo_plus1", dict(ldo_extra=1)), ("bias_skew", dict(bias_skew=1)), ("e0_skew", dict(e0_skew=1))]


SCALAR = [(n, how, kw, fam) for n in ("map17x17_B1", "res_relu", "chan36_20", "normal17") for how, kw in SKEWS for fam in ("2x2", "direct")
          if how != "e0_skew" or n == "res_relu"]


@pytest.mark.parametrize("name,how,kw,fam", SCALAR, ids=["%s-%s-%s" % (n, h, f) for n, h, _, f in SCALAR])
def test_scalar_epilogue(name, how, kw, fam):
    """an output, bias or epilogue operand that rules out 16-byte accesses: F(2x2,3x3) takes its scalar epilogue (the `else` of
    `else if (q.vec4)`), the direct kernel stores element by element anyway; F(2x4,3x3) refuses such a descriptor"""
    c = cc.BY_NAME[name]
    d, st = statement(c, fam)
    f, outs = layout(c, d, fam, **kw)
    call_desc("ramnet_conv_launch", _hip.ConvDesc, f)
    judge(c, d, st, outs, "%s on %s, %s" % (name, fam, how))
    if fam == "2x2" and c.Cout % 64 == 0:
        f["w"], f["algo"] = pack(d, "2x4", 3), _hip.ALGO_WINOGRAD_2X4
        outs["out"].freeze()
        call_desc("ramnet_conv_launch", _hip.ConvDesc, f, rc=BADARG)


@pytest.mark.parametrize("name", ["lstm16", "gru_bwd", "out_s2d16"])
def test_quad_only_epilogues_refuse_a_skewed_output(name):
    c = cc.BY_NAME[name]
    d, _ = statement(c, "2x2")
    f, outs = layout(c, d, "2x2", out_skew=1)
    call_desc("ramnet_conv_launch", _hip.ConvDesc, f, rc=BADARG)


# ---------------------------------------------------------------------------------------------------- split reduction of F(2x2,3x3)
@pytest.mark.parametrize("ksplit,cin", [(2, 32), (3, 48), (4, 64)])
def test_wino_split_reduction(ksplit, cin):
    """option wino_ksplit forced: partial tiles meet in the workspace, the last arrival joins them in split order: exact on integers, bit-equal
    across two launches on one workspace, arrival counters back at zero, workspace guards intact"""
    L = _hip.lib()
    c = cc._case("ksplit%d" % ksplit, ("2x2",), 1, 9, 11, cin, 64, density=0.25)
    d = cc.build(c)
    st = cr.conv_statement(d, "2x2")
    assert cr.exact_ok(st, "2x2")
    old = L.ramnet_get_option(b"wino_ksplit")
    try:
        assert L.ramnet_set_option(b"wino_ksplit", ksplit) == 0
        f, outs = layout(c, d, "2x2")
        s = _struct(f)
        n = L.ramnet_conv_splitk_floats(C.byref(s))
        assert n > 0
        ws = Out(1, n, prefill=torch.zeros(n))
        f["splitk_ws"], f["splitk_floats"] = ws, n
        call_desc("ramnet_conv_launch", _hip.ConvDesc, f)
        first = outs["out"].value()
        assert_exact(first, st.out, "split reduction x%d" % ksplit)
        counters = ws.value()[0, :64].view(torch.int32)
        assert not bool(counters.any()), "arrival counters must be left at zero"
        f2, outs2 = layout(c, d, "2x2")
        f2["splitk_ws"], f2["splitk_floats"] = ws, n
        call_desc("ramnet_conv_launch", _hip.ConvDesc, f2)
        assert_bits(outs2["out"].value(), first.double(), "second launch on the same workspace")
    finally:
        L.ramnet_set_option(b"wino_ksplit", old)


# ---------------------------------------------------------------------------------------------------- multi-class launch
def test_stride2_backward_data_as_one_multi_launch():
    """the four output-parity classes of a 5x5 stride-2 backward-data as ONE ramnet_conv_launch_multi, non-identity wtap, against
    conv_transpose2d in float64 (exact on integers)"""
    import torch.nn.functional as F
    k, p, B, Hx, Wx, O, I = 5, 2, 2, 11, 13, 8, 20
    Hy, Wy = (Hx + 2 * p - k) // 2 + 1, (Wx + 2 * p - k) // 2 + 1
    g = torch.Generator().manual_seed(77)
    dy = (torch.randint(-2, 3, (B, Hy, Wy, O), generator=g) * (torch.rand(B, Hy, Wy, O, generator=g) < 0.5)).to(F64)
    w = (48 * torch.randint(-1, 2, (O, I, k, k), generator=g)).to(F64)
    ref = F.conv_transpose2d(dy.permute(0, 3, 1, 2), w, None, 2, p, output_padding=(Hx - ((Hy - 1) * 2 - 2 * p + k), Wx - ((Wy - 1) * 2 - 2 * p + k)))
    ref = ref.permute(0, 2, 3, 1).contiguous()
    L = _hip.lib()
    wp = Out(1, L.ramnet_packed_weight_elems(O, I, k, k, 1, 1))
    call("ramnet_pack_weight", In(w.reshape(-1)), wp, O, I, k, k, 1, 1)
    wp.freeze()
    x0, out = In(dy, ld=O + 4), Out(B * Hx * Wx, I, ld=I + 4)
    descs = []
    for py in range(2):
        for px in range(2):
            taps = [((py + p - u) // 2, (px + p - v) // 2, u * k + v) for u in range(k) for v in range(k) if (py + p - u) % 2 == 0 and (px + p - v) % 2 == 0]
            descs.append(dict(x0=x0, ld0=O + 4, C0=O, in_mode=_hip.IN_PLAIN, B=B, Hin=Hy, Win=Wy, stride=1, ntaps=len(taps),
                              dy=[t[0] for t in taps], dx=[t[1] for t in taps], wtap=[t[2] for t in taps], w=wp, Cout=I,
                              Ho=(Hx - py + 1) // 2, Wo=(Wx - px + 1) // 2, HoF=Hx, WoF=Wx, osy=2, osx=2, ooy=py, oox=px, epi=_hip.EPI_LINEAR,
                              out=out, ldo=I + 4, algo=_hip.ALGO_DIRECT))
    assert any(t != i for dd in descs for i, t in enumerate(dd["wtap"]))
    call_desc("ramnet_conv_launch_multi", _hip.ConvDesc, descs)
    assert_exact(out.value(), ref, "stride-2 backward-data, four classes in one launch")
    # a class whose own HoF differs from descs[0]'s is refused (the kernel takes it from descs[0])
    bad = [dict(dd) for dd in descs]
    bad[3]["HoF"] = Hx + 2
    call_desc("ramnet_conv_launch_multi", _hip.ConvDesc, bad, rc=BADARG, also=[out.freeze()])


# ---------------------------------------------------------------------------------------------------- refused siblings
def test_eligibility_answers_zero_for_the_refused_siblings():
    L = _hip.lib()

    def ask(c, **kw):
        d = cc.build(c)
        f, _ = layout(c, d, "2x2", **kw)
        s = _struct(f)
        return L.ramnet_conv_wino_variant(C.byref(s), 1), L.ramnet_conv_wino_split_ok(C.byref(s), 1)

    assert ask(cc.BY_NAME["cat16_12"]) == (1, 1)
    assert ask(cc.BY_NAME["chan36_20"]) == (0, 0)                                           # Cout % 64 != 0
    assert ask(cc._case("cat12", cc.ALL3, 1, 5, 7, 12, 64, C1=4, mode=cr.IN_CAT)) == (0, 0)    # a chunk of 8 would straddle the concatenation
    assert ask(cc.BY_NAME["cat8_4"]) == (1, 0)                                              # ... a chunk of 16 of the split family
    assert ask(cc.BY_NAME["lstm16"]) == (1, 0)                                              # the cell: exact-fp32 kernel only
    assert ask(cc.BY_NAME["map17x17_B1"], out_skew=1) == (0, 0)                             # a skewed pointer
    assert ask(cc.BY_NAME["map17x17_B1"], bias_skew=1) == (0, 0)


# ---------------------------------------------------------------------------------------------------- backward-weights, DIRECT
WG_MAPS = [(1, 1), (5, 7), (9, 43), (16, 22)]
WG_MODES = [(cr.IN_PLAIN, 8, 0), (cr.IN_CAT, 8, 4), (cr.IN_CAT_MUL, 4, 12), (cr.IN_RELUMASK, 12, 0)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("i", range(4))
def test_wgrad_direct(i, B):
    """RAMNET_ALGO_DIRECT backward-weights with ramnet_unpack_wgrad: the atomic form is exact on integers; `wgrad_blocks` lowered so that a
    small map still splits its tiles; gmask / dbias given and absent; unpack into a window (n_off > 0) onto a non-zero gradient"""
    import types
    L = _hip.lib()
    H, W = WG_MAPS[i]
    mode, C0, C1 = WG_MODES[(i + B) % 4]
    k, stride = (3, 1) if i % 2 == 0 else (5, 2)
    p = k // 2
    Cout = (20, 64)[i % 2]
    Cin = C0 + C1
    g = torch.Generator().manual_seed(100 + 10 * i + B)

    def ints(shape, m=2):
        return (torch.randint(-m, m + 1, shape, generator=g) * (torch.rand(shape, generator=g) < 0.5)).to(F64)
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    d = types.SimpleNamespace(in_mode=mode, x0=ints((B, H, W, C0)), x1=ints((B, H, W, C1)) if C1 else None, xm=None, stride=stride, Ho=Ho, Wo=Wo,
                              taps=[(a - p, b - p) for a in range(k) for b in range(k)], dout=ints((B, Ho, Wo, Cout), 4),
                              gmask=ints((B, Ho, Wo, Cout), 1) if (i + B) % 2 else None)
    if mode == cr.IN_CAT_MUL:
        d.xm = ints((B, H, W, C1))
    if mode == cr.IN_RELUMASK:
        d.xm = ints((B, H, W, C0), 1)
    st = cr.wgrad_statement(d)
    assert float(st.dW_abs.max()) * 16 < 2 ** 24
    want_bias = (i + B) % 3 != 0
    dw = Out(k * k * Cin, Cout, prefill=torch.zeros(k * k * Cin, Cout))
    dbias = Out(1, Cout, prefill=torch.zeros(Cout)) if want_bias else None
    f = dict(x0=In(d.x0, ld=C0 + 4), ld0=C0 + 4, C0=C0, C1=C1, in_mode=mode, B=B, Hin=H, Win=W, ntaps=k * k, stride=stride,
             dy=[t[0] for t in d.taps], dx=[t[1] for t in d.taps], dout=In(d.dout, ld=Cout + 4), ldg=Cout + 4, Cout=Cout, Ho=Ho, Wo=Wo, dw=dw,
             algo=_hip.ALGO_DIRECT)
    if d.x1 is not None:
        f["x1"], f["ld1"] = In(d.x1, ld=C1 + 8), C1 + 8
    if d.xm is not None:
        f["xm"], f["ldm"] = In(d.xm, ld=d.xm.shape[3] + 4), d.xm.shape[3] + 4
    if d.gmask is not None:
        f["gmask"], f["ldgm"] = In(d.gmask, ld=Cout + 8), Cout + 8
    if want_bias:
        f["dbias"] = dbias
    old = L.ramnet_get_option(b"wgrad_blocks")
    try:
        assert L.ramnet_set_option(b"wgrad_blocks", 512 if i % 2 else 6) == 0
        call_desc("ramnet_wgrad_launch", _hip.WgradDesc, f)
    finally:
        L.ramnet_set_option(b"wgrad_blocks", old)
    assert L.ramnet_last_kernel().decode().startswith("conv_wgrad_kernel<")
    assert_exact(dw.value(), st.dW.reshape(k * k * Cin, Cout), "wgrad dW", abs_sum=st.dW_abs.reshape(k * k * Cin, Cout))
    if want_bias:
        assert_exact(dbias.value(), st.dbias, "wgrad dbias", abs_sum=st.dbias_abs.reshape(1, Cout))
    # unpack the output channels [n_off, n_off + Cn) and the input channels [0, C0) onto a non-zero gradient
    n_off, Cn = 4, Cout - 8
    gold = ints((Cn, C0, k, k), 8)
    grad = Out(1, gold.numel(), prefill=gold.reshape(-1))
    call("ramnet_unpack_wgrad", dw.freeze(), grad, Cn, C0, Cin, Cout, n_off, k, k)
    assert_exact(grad.value(), cr.unpack_statement(gold, st.dW, Cn, C0, n_off).reshape(1, -1), "unpack_wgrad window")


WG_FAMS = {"2x2": (_hip.ALGO_WINOGRAD, "ramnet_wgrad_wino_slabs", "ramnet_unpack_wgrad_wino", "conv_wgrad_wino_r_kernel<"),
           "2x4": (_hip.ALGO_WINOGRAD_2X4, "ramnet_wgrad_wino2x4_slabs", "ramnet_unpack_wgrad_wino2x4", "conv_wgrad_wino_r6_kernel<"),
           "dsplit": (_hip.ALGO_DIRECT_SPLIT, "ramnet_wgrad_dsplit_slabs", "ramnet_unpack_wgrad_dsplit", "conv_wgrad_dsplit_kernel<")}


def _ws_floats(fam, Cin, Cout):
    L = _hip.lib()
    return (16 * Cin * Cout if fam == "2x2" else L.ramnet_wgrad_wino2x4_ws_floats(Cin, Cout) if fam == "2x4" else
            L.ramnet_wgrad_dsplit_ws_floats(Cin, Cout))


def _wgrad_fields(i, d, fam, dw, dbias, S):
    """descriptor fields of backward-weights row i with every tensor pitched between guards; returns (fields, the In objects of this segment)"""
    H, W, B, mode, C0, C1, Cout = cc.WGRAD_ROWS[i][:7]
    seg = dict(x0=In(d.x0, ld=C0 + 4), dout=In(d.dout, ld=Cout + 4))
    f = dict(ld0=C0 + 4, C0=C0, C1=C1, in_mode=mode, B=B, Hin=H, Win=W, ntaps=9, stride=1, dy=[t[0] for t in d.taps], dx=[t[1] for t in d.taps],
             ldg=Cout + 4, Cout=Cout, Ho=H, Wo=W, dw=dw, algo=WG_FAMS[fam][0], dw_slabs=S)
    if d.x1 is not None:
        seg["x1"], f["ld1"] = In(d.x1, ld=C1 + 8), C1 + 8
    if d.xm is not None:
        seg["xm"], f["ldm"] = In(d.xm, ld=d.xm.shape[3] + 4), d.xm.shape[3] + 4
    if d.gmask is not None:
        seg["gmask"], f["ldgm"] = In(d.gmask, ld=Cout + 8), Cout + 8
    if dbias is not None:
        f["dbias"] = dbias
    f.update(seg)
    return f, seg


def _wgrad_judge(i, d, st, fam, dw, dbias, S, what):
    """fold the slabs, unpack slab 0 with the library's own unpack into a window (n_off = 4) onto a non-zero gradient, compare"""
    H, W, B, mode, C0, C1, Cout, _, _, kind = cc.WGRAD_ROWS[i]
    Cin, one = d.Cin, _ws_floats(fam, d.Cin, Cout)
    if S > 1:
        call("ramnet_reduce_slabs", dw, S, one)
        assert not bool(_bits(dw.value()[1:]).any()), "slabs 1.. must be +0 after the fold"
        if dbias is not None:
            call("ramnet_reduce_slabs", dbias, S, Cout)
    bw, bb = cr.wgrad_bound(d, st, fam)
    if dbias is not None:
        if kind == "int":
            assert_exact(dbias.value()[0], st.dbias, "%s dbias" % what, abs_sum=st.dbias_abs)
        else:
            assert_within(dbias.value()[0], st.dbias, bb, "%s dbias" % what)
    n_off, Cn, Ck = 4, Cout - 8, min(Cin, 40)       # output channels [4, Cout - 4), input channels [0, Ck)
    g = torch.Generator().manual_seed(i)
    gold = torch.randint(-8, 9, (Cn, Ck, 3, 3), generator=g).to(F64)
    grad = Out(1, gold.numel(), prefill=gold.reshape(-1))
    call(WG_FAMS[fam][2], In(dw.value()[0]), grad, Cn, Ck, Cin, Cout, n_off)      # (slab 0 alone, NaN behind it)
    ref = cr.unpack_statement(gold, st.dW, Cn, Ck, n_off).reshape(1, -1)
    if kind == "int":
        assert_exact(grad.value(), ref, "%s gradient after its unpack" % what)
    else:
        bound = bw[:, :Ck, n_off:n_off + Cn].permute(2, 1, 0).reshape(1, -1) + cr.U * ref.abs()
        assert_within(grad.value(), ref, bound, "%s gradient after its unpack" % what)


@pytest.mark.parametrize("slab_form", [False, True])
@pytest.mark.parametrize("fam", sorted(WG_FAMS))
@pytest.mark.parametrize("i", range(len(cc.WGRAD_ROWS)))
def test_wgrad_3x3_families(i, fam, slab_form):
    """RAMNET_ALGO_WINOGRAD (F(2x2,3x3) domain), RAMNET_ALGO_WINOGRAD_2X4 (F(2x4,3x3) domain, blocked workspace) and RAMNET_ALGO_DIRECT_SPLIT
    (bf16 split operands) backward-weights, compared AFTER the library's own unpack with the OIHW gradient of the statement: exact on the
    integer rows (the folded gradient is an integer, the transformed-domain absolute statement x 16 stays below 2^24: asserted), derived on
    the normal rows; atomic form (dw_slabs = 0) and slab form with the library's slab count (ramnet_reduce_slabs first), whose two runs
    must agree bit for bit.  Odd rows lower `wgrad_wino_blocks` so that a small map still splits its tiles and run F(2x2,3x3) with
    `wgrad_wino_nf` = 2 (64-channel workgroups).  Rows: PLAIN / CAT / CAT_MUL / RELUMASK / S2D, gmask and dbias given and absent."""
    L = _hip.lib()
    algo, slabs_fn, unpack, kernel = WG_FAMS[fam]
    H, W, B, mode, C0, C1, Cout, _, want_bias, kind = cc.WGRAD_ROWS[i]
    d = cc.build_wgrad(i)
    st = cr.wgrad_statement(d)
    if kind == "int":
        top = st.dW_abs if fam == "dsplit" else cr.wgrad_wino(d, fam)[0]
        assert float(top.max()) * 16 < 2 ** 24 and torch.equal(st.dW, st.dW.round())
    one = _ws_floats(fam, d.Cin, Cout)
    S = getattr(L, slabs_fn)(d.Cin, Cout) if slab_form else 1
    old = (L.ramnet_get_option(b"wgrad_wino_blocks"), L.ramnet_get_option(b"wgrad_wino_nf"))
    runs = []
    try:
        assert L.ramnet_set_option(b"wgrad_wino_blocks", 384 if i % 2 == 0 else 8) == 0
        assert L.ramnet_set_option(b"wgrad_wino_nf", 1 + i % 2) == 0
        for run in range(2 if slab_form else 1):
            dw = Out(S, one, prefill=torch.zeros(S, one))
            dbias = Out(S, Cout, prefill=torch.zeros(S, Cout)) if want_bias else None
            f, _ = _wgrad_fields(i, d, fam, dw, dbias, S if slab_form else 0)
            call_desc("ramnet_wgrad_launch", _hip.WgradDesc, f)
            name = L.ramnet_last_kernel().decode()
            assert name.startswith(kernel), name
            if fam == "2x2":
                assert name.endswith(",%d>" % (1 + i % 2)), name
            runs.append((dw, dbias))
    finally:
        L.ramnet_set_option(b"wgrad_wino_blocks", old[0])
        L.ramnet_set_option(b"wgrad_wino_nf", old[1])
    if slab_form:
        assert_bits(runs[1][0].value(), runs[0][0].value().double(), "%s slab form, second run" % fam)
        if want_bias:
            assert_bits(runs[1][1].value(), runs[0][1].value().double(), "%s slab form dbias, second run" % fam)
    _wgrad_judge(i, d, st, fam, runs[0][0], runs[0][1], S, "%s row %d" % (fam, i))


@pytest.mark.parametrize("slab_form", [False, True])
@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("i", [1, 2, 5])
def test_wgrad_segments(i, nseg, slab_form):
    """nseg = 1, 3 on RAMNET_ALGO_WINOGRAD_2X4: one launch over several tensor sets of the same layer gives the sum of the single launches
    (the statement over all segments): exact on the integer rows, derived on the normal one"""
    import types
    L = _hip.lib()
    H, W, B, mode, C0, C1, Cout, _, want_bias, kind = cc.WGRAD_ROWS[i]
    segs = [cc.build_wgrad(i, seed=k) for k in range(nseg)]
    d = types.SimpleNamespace(**vars(segs[0]))
    d.segs = segs
    st = cr.wgrad_statement(d)
    if kind == "int":
        assert float(cr.wgrad_wino(d, "2x4")[0].max()) * 16 < 2 ** 24
    one = _ws_floats("2x4", d.Cin, Cout)
    S = L.ramnet_wgrad_wino2x4_slabs(d.Cin, Cout) if slab_form else 1
    dw = Out(S, one, prefill=torch.zeros(S, one))
    dbias = Out(S, Cout, prefill=torch.zeros(S, Cout)) if want_bias else None
    f, first = _wgrad_fields(i, segs[0], "2x4", dw, dbias, S if slab_form else 0)
    keep, arr = [first], (_hip.WgradSeg * nseg)()
    for k in range(nseg):
        if k:
            keep.append(_wgrad_fields(i, segs[k], "2x4", dw, dbias, 0)[1])
        for name, buf in keep[k].items():
            setattr(arr[k], name, buf.ptr)
    f["nseg"], f["segs"] = nseg, C.cast(arr, C.POINTER(_hip.WgradSeg))
    old = L.ramnet_get_option(b"wgrad_wino_blocks")
    try:
        assert L.ramnet_set_option(b"wgrad_wino_blocks", 24) == 0
        call_desc("ramnet_wgrad_launch", _hip.WgradDesc, f)
    finally:
        L.ramnet_set_option(b"wgrad_wino_blocks", old)
    _wgrad_judge(i, d, st, "2x4", dw, dbias, S, "2x4 row %d, %d segments" % (i, nseg))


PLANNED = cp.EXPECTED + cp.EXPECTED_DSPLIT


@pytest.mark.parametrize("fam,opts,shape,want", PLANNED, ids=["%s-%s-%s" % (f, "x".join(map(str, s)), "-".join("%s%s" % kv for kv in o.items()) or "default")
                                                             for f, o, s, _ in PLANNED])
def test_wgrad_launch_uses_the_planned_splits(fam, opts, shape, want):
    """How many tile splits a launch really uses, seen in the slab form: after ONE launch into a zeroed [S][one] workspace, S = the library's
    slab query, exactly the slabs 0 .. splits - 1 hold something (normal data: every split's batches sum to non-zero values) and the rest is
    bit-zero, for dw and for the dbias rows alike; splits, tile shape and nf as the restatement of the rule says (tests/wgrad_plan_cases.py),
    which is first held to the values written down for this row.  PLAIN input, no masks; `dw_slabs` below S, lowered `wgrad_wino_blocks`,
    `wgrad_wino_nf` and several segments as the row says."""
    L = _hip.lib()
    B, H, W, Cin, Cout = shape
    p = cp.plan(fam, *shape, **opts)
    assert {k: p[k] for k in want} == want, p
    algo, slabs_fn, _, _ = WG_FAMS[fam]
    S, one, nseg = getattr(L, slabs_fn)(Cin, Cout), _ws_floats(fam, Cin, Cout), opts.get("nseg", 1)
    assert S == p["cap"] and 1 <= p["splits"] <= p["slabs"] <= S
    g = cc._gen("planned splits %s %r" % (fam, shape))
    segs = [dict(x0=In(cc._rn(g, (B, H, W, Cin)), ld=Cin + 4), dout=In(cc._rn(g, (B, H, W, Cout)), ld=Cout + 4)) for _ in range(nseg)]
    dw, dbias = Out(S, one, prefill=torch.zeros(S, one)), Out(S, Cout, prefill=torch.zeros(S, Cout))
    f = dict(ld0=Cin + 4, C0=Cin, in_mode=cr.IN_PLAIN, B=B, Hin=H, Win=W, ntaps=9, stride=1, dy=[t // 3 - 1 for t in range(9)],
             dx=[t % 3 - 1 for t in range(9)], ldg=Cout + 4, Cout=Cout, Ho=H, Wo=W, dw=dw, dbias=dbias, algo=algo, dw_slabs=p["slabs"], **segs[0])
    if nseg > 1:
        arr = (_hip.WgradSeg * nseg)()
        for k, seg in enumerate(segs):
            arr[k].x0, arr[k].dout = seg["x0"].ptr, seg["dout"].ptr
        f["nseg"], f["segs"] = nseg, C.cast(arr, C.POINTER(_hip.WgradSeg))
    old = (L.ramnet_get_option(b"wgrad_wino_blocks"), L.ramnet_get_option(b"wgrad_wino_nf"))
    try:
        assert L.ramnet_set_option(b"wgrad_wino_blocks", opts.get("blocks", 384)) == 0
        assert L.ramnet_set_option(b"wgrad_wino_nf", opts.get("nf", 1)) == 0
        call_desc("ramnet_wgrad_launch", _hip.WgradDesc, f)
        assert L.ramnet_last_kernel().decode() == p["kernel"]
    finally:
        L.ramnet_set_option(b"wgrad_wino_blocks", old[0])
        L.ramnet_set_option(b"wgrad_wino_nf", old[1])
    for what, buf in (("dw", dw), ("dbias", dbias)):
        used = _bits(buf.value()).ne(0).any(dim=1)
        print("%s: slabs in use %d of %d, planned %d" % (what, int(used.sum()), S, p["splits"]))
        assert used.tolist() == [s < p["splits"] for s in range(S)], "%s: slabs in use %r, planned 0 .. %d" % (
            what, used.nonzero().view(-1).tolist(), p["splits"] - 1)


def test_split_third_term_adds_up():
    """one F(2x4,3x3) tile whose transformed input has the same value in all 16 channels, chosen so that its THIRD bf16 term is as large as
    one gets and of one sign (tests/conv_launch_cases.py: build_coherent): the derived bound of the split family is 3.4 times smaller than
    what the six-product expression loses with the (third term of V) x (first term of U) product, so a split kernel without it fails here
    although its error stays far below 2e-5 of the tensor maximum.  The exact-fp32 kernel runs the same row."""
    c, d = cc.build_coherent()
    for fam in c.fams:
        st = cr.conv_statement(d, fam)
        if fam == "2x4split":
            assert 16 * 57 * 2.0 ** -23 > 3 * float(st.b_out[0, 0, 0, 0]) and 16 * 57 * 2.0 ** -23 < 2e-5 * float(st.out.abs().max())
        f, outs = layout(c, d, fam)
        call_desc("ramnet_conv_launch", _hip.ConvDesc, f)
        assert _hip.lib().ramnet_last_kernel().decode().startswith(KERNEL[fam])
        judge(c, d, st, outs, "coherent third term on %s" % fam)


@pytest.mark.parametrize("slabs,n", [(1, 8), (2, 4), (3, 1028), (5, 40), (4, 300004), (2, 4194312)])
def test_reduce_slabs(slabs, n):
    """slab 0 <- ((slab 0 + slab 1) + slab 2) + ..., bit for bit (the ordered fold in fp32), slabs 1.. zero afterwards; the last size has a
    second trip of the 4096 x 256 x 4 grid with a ragged end"""
    g = torch.Generator().manual_seed(slabs * 1000 + n)
    x = torch.randn(slabs, n, generator=g)
    ws = Out(slabs, n, prefill=x)
    call("ramnet_reduce_slabs", ws, slabs, n)
    got = ws.value()
    ref = x[0].clone()
    for s in range(1, slabs):
        ref = ref + x[s]                            # fp32, slab order
    assert_bits(got[0], ref.double(), "reduce_slabs: the fp32 fold in slab order")
    assert not bool(_bits(got[1:]).any()), "slabs 1.. must be +0 afterwards"


# ---------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks():
    """every refusal: RAMNET_E_BADARG with a message, all outputs untouched (none of these descriptors is ever launched)"""
    for fam in ("direct", "2x2", "2x4", "2x4split"):
        for name, edits in (
                ("cat16_12", [dict(ld0=12), dict(ld1=8), dict(ldo=124), dict(Ho=18), dict(Wo=18), dict(ooy=1), dict(oox=-1), dict(HoF=16), dict(C0=0),
                              dict(C1=-4), dict(ld0=18)]),
                ("catmul16_4", [dict(ldm=0)]),
                ("relumask16", [dict(ldm=12)]),
                ("res_relu", [dict(lde0=60)]),
                ("gru_bwd", [dict(lde0=124), dict(ldo1=124), dict(lde1=60), dict(beta=1.0)]),
                ("sigmoid_hr", [dict(lde1=60), dict(ldo1=60)]),
                ("gru_blend", [dict(lde0=60), dict(lde1=60), dict(ldo1=60)]),
                ("out_s2d16", [dict(HoF=9), dict(WoF=13), dict(ldo=12)]),
                ("beta1", [dict(active=1)])):
            c = cc.BY_NAME[name]
            if fam not in c.fams:
                continue
            d = cc.build(c)
            f, outs = layout(c, d, fam)
            for o in outs.values():
                o.freeze()
            for e in edits:
                g = dict(f)
                if "active" in e:
                    g["active"] = In(torch.ones(d.B), dtype=torch.int32, fill=1)
                else:
                    g.update(e)
                call_desc("ramnet_conv_launch", _hip.ConvDesc, g, rc=BADARG)
    # the cell's operands
    for fam in ("direct", "2x2", "2x4"):
        c = cc.BY_NAME["lstm16_masked"]
        d = cc.build(c)
        f, outs = layout(c, d, fam)
        for e in (dict(ldo1=12), dict(lde1=12), dict(ldo2=60), dict(lde0=12), dict(ldo=12)):
            call_desc("ramnet_conv_launch", _hip.ConvDesc, dict(f, **e), rc=BADARG)
    # backward-weights
    x, g_, dw = In(torch.zeros(2 * 5 * 7, 8)), In(torch.zeros(2 * 5 * 7, 8)), Out(9 * 8, 8, prefill=torch.zeros(72, 8))
    base = dict(x0=x, ld0=8, C0=8, in_mode=_hip.IN_PLAIN, B=2, Hin=5, Win=7, ntaps=9, stride=1, dy=[t // 3 - 1 for t in range(9)],
                dx=[t % 3 - 1 for t in range(9)], dout=g_, ldg=8, Cout=8, Ho=5, Wo=7, dw=dw, algo=_hip.ALGO_DIRECT)
    for e in (dict(ld0=4), dict(ldg=4), dict(gmask=g_, ldgm=4), dict(in_mode=_hip.IN_RELUMASK, xm=x, ldm=4), dict(in_mode=_hip.IN_CAT, x1=x, C1=8, ld1=4),
              dict(nseg=1)):
        call_desc("ramnet_wgrad_launch", _hip.WgradDesc, dict(base, **e), rc=BADARG)
