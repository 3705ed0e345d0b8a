"""No GPU: the rows of tests/address_limit_cases.py before any of them is launched (tests/test_hip_address_limits.py).  Every "below" row
must reach its limit — the pitch is the largest its guard accepts and the highest byte the launch addresses in the inflated operand lies
within one pitch of the limit —, its "first refused" sibling (the pitch 4 floats larger) must be refused with RAMNET_E_BADARG by a message that
names the condition, before any HIP call, and the quiet queries must answer for both without touching ramnet_last_error().  No accepted
descriptor is launched here: a "below" row is asked only through the queries."""
import ctypes as C

import pytest
import torch

import address_limit_cases as al
import conv_restatement as cr
from rpg_ramnet_amd import _hip

BADARG = 10001
CONV = [r for r in al.CONV_ROWS]
WGRAD = [r for r in al.WGRAD_ROWS]
FOLDHEAD = [r for r in al.FH_ROWS]
FH_FRAGMENT = {"fold_fwd": b"xb < FOLD_X_LIMIT", "fold_dgrad": b"xb < FOLD_DGRAD_X_LIMIT", "fold_wgrad": b"2 * q.xbytes < WOOB && 2 * q.gbytes < WOOB"}
# the text of the guard that refuses the sibling of a row (the stringised condition in ramnet_last_error)
FRAGMENT = {("conv", "src"): b"px * ldmax * 4ull < (unsigned long long)WOOB", ("conv", "dst"): b"d.HoF * d.WoF * lo * 4ull < (unsigned long long)WOOB",
            ("conv", "direct"): b"px * ld < (1ull << 32)", ("wgrad", "tensor"): b"px * ldx * 4ull < WOOB && mpx * d.ldm * 4ull < WOOB && gpx * d.ldg * 4ull < WOOB"}


def _lib():
    return _hip.lib()


def _mark_error(L):
    """leave a known message in ramnet_last_error(): a query that touches it would change it"""
    assert L.ramnet_conv_launch(None, None) == BADARG
    return L.ramnet_last_error()


def _conv_struct(row, refused, algo=None):
    d = al.conv_build(row)
    f, _ = al.conv_fields(row, d, al.Dummy(), refused)
    if algo is not None:
        f["algo"] = algo
    return d, f, al.struct(_hip.ConvDesc, f)


def _wgrad_struct(row, refused):
    segs = [al.wgrad_build(row, k) for k in range(row.nseg)]
    f, per_seg = al.wgrad_fields(row, segs, al.Dummy(), 1 << 30, (1 << 30) + 4096, 0, refused)
    arr = None
    if row.nseg > 1:
        arr = (_hip.WgradSeg * row.nseg)()
        for k, one in enumerate(per_seg):
            for name, ptr in one.items():
                setattr(arr[k], name, ptr)
        f["nseg"], f["segs"] = row.nseg, C.cast(arr, C.POINTER(_hip.WgradSeg))
    return segs, f, al.struct(_hip.WgradDesc, f), arr


# ---------------------------------------------------------------------------------------------------- closeness
@pytest.mark.parametrize("row", CONV, ids=[r.name for r in CONV])
def test_conv_row_reaches_its_limit(row):
    d = al.conv_build(row)
    px, limit, unit = al.conv_limit(row, d)
    ld, ch = al.conv_ld(row, d), al.conv_channels(row, d)
    highest = ((px - 1) * ld + ch) * unit               # one past the last byte (element: direct) the launch addresses behind the operand's pointer
    print("%s: pitch %d floats, %d pixels, highest %d, limit %d, distance %d = %.4f pitches" % (row.name, ld, px, highest, limit, limit - highest,
                                                                                                (limit - highest) / (ld * unit)))
    assert ld % 4 == 0 and ld >= ch
    if row.kind == "none":
        assert highest > 1 << 31, "the row does not leave the range of a 32-bit byte offset"
        return
    assert px * ld * unit < limit <= px * (ld + 4) * unit, "the pitch is not the largest the guard accepts"
    # the last address lies within one pitch of the extent the guard measures (px pitches), and that extent within one step of the
    # pitch's 4-float granularity of the limit: the next pitch is refused
    assert 0 <= px * ld * unit - highest < ld * unit and 0 < limit - px * ld * unit <= 4 * px * unit, "the row does not reach its limit"


@pytest.mark.parametrize("row", WGRAD, ids=[r.name for r in WGRAD])
def test_wgrad_row_reaches_its_limit(row):
    ld, ch = al.wgrad_ld(row), al.wgrad_channels(row)
    assert ld % 4 == 0 and ld >= ch
    whole = row.B * al.H * al.W * (4 if row.mode == cr.IN_S2D and row.operand == "x0" else 1)
    if row.kind == "none":
        assert ((whole - 1) * ld + ch) * 4 > 1 << 32, "the row does not leave the range of a 32-bit byte offset"
        return
    px, limit = al.wgrad_limit(row)
    assert px * ld * 4 < limit <= px * (ld + 4) * 4, "the pitch is not the largest the guard accepts"
    # the highest byte addressed: the last pixel of the tensor; the resource of a source begins one halo in front of it, so the offset the
    # hardware checks is longer by the halo's pitches (px - whole of them): within one pitch of the limit, up to the granularity of a pitch
    highest = ((px - 1) * ld + ch) * 4
    print("%s: pitch %d floats, %d pixels (%d of them halo), highest offset %d, limit %d, distance %d = %.4f pitches" % (
        row.name, ld, px, px - whole, highest, limit, limit - highest, (limit - highest) / (ld * 4)))
    assert 0 <= px * ld * 4 - highest < ld * 4 and 0 < limit - px * ld * 4 <= 16 * px, "the row does not reach its limit"


# ---------------------------------------------------------------------------------------------------- the refused sibling
@pytest.mark.parametrize("row", [r for r in CONV if r.kind != "none"], ids=[r.name for r in CONV if r.kind != "none"])
def test_conv_sibling_is_refused_before_any_launch(row):
    L = _lib()
    d, f, s = _conv_struct(row, True)
    assert L.ramnet_conv_launch(C.byref(s), None) == BADARG
    err = L.ramnet_last_error()
    want = FRAGMENT[("conv", "direct" if row.fam == "direct" else "src" if row.operand in al.SOURCES else "dst")]
    assert b"bad argument" in err and want in err, err


@pytest.mark.parametrize("row", [r for r in WGRAD if r.kind != "none"], ids=[r.name for r in WGRAD if r.kind != "none"])
def test_wgrad_sibling_is_refused_before_any_launch(row):
    L = _lib()
    segs, f, s, keep = _wgrad_struct(row, True)
    assert L.ramnet_wgrad_launch(C.byref(s), None) == BADARG
    err = L.ramnet_last_error()
    assert b"bad argument" in err and FRAGMENT[("wgrad", "tensor")] in err, err


# ---------------------------------------------------------------------------------------------------- the quiet queries
@pytest.mark.parametrize("row", CONV, ids=[r.name for r in CONV])
def test_conv_queries_answer_as_the_launch_does(row):
    """ramnet_conv_wino_variant / ramnet_conv_wino_split_ok run the plan of the launch (csrc/conv_plan.hpp: wino6_plan), its offset guard
    included: 1 for the "below" row of an F(2x4) family, 0 for the refused sibling of every 3x3 row, ramnet_last_error() untouched"""
    L = _lib()
    lstm = row.case.epi == cr.EPI_LSTM
    for refused in (False, True):
        if refused and row.kind == "none":
            continue
        d, f, s = _conv_struct(row, refused, algo=_hip.ALGO_WINOGRAD)
        mark = _mark_error(L)
        variant, split = L.ramnet_conv_wino_variant(C.byref(s), 1), L.ramnet_conv_wino_split_ok(C.byref(s), 1)
        fold = (L.ramnet_fold_wino_variant(C.byref(s), 1), L.ramnet_fold_halfwg_variant(C.byref(s), 1))
        own = al.struct(_hip.ConvDesc, f)
        own.algo = al.ALGO[row.fam]
        fits = L.ramnet_conv_addressable(C.byref(own))
        assert L.ramnet_last_error() == mark, "a query touched ramnet_last_error()"
        assert fold == (0, 0)                           # (not a folded launch)
        assert fits == int(not refused), "ramnet_conv_addressable answers %d" % fits
        if row.fam == "direct":                         # the guard of check_desc is the launch's alone: no query runs it
            continue
        if refused:
            if not (row.fam == "2x2" and row.operand == "o2"):
                assert (variant, split) == (0, 0), "a query accepts what the launch refuses"
        elif row.fam in ("2x4", "2x4split"):
            assert variant == 1 and split == int(row.fam == "2x4split" or (not lstm and row.case.C0 % 16 == 0)), (variant, split)


@pytest.mark.parametrize("row", WGRAD, ids=[r.name for r in WGRAD])
def test_wgrad_queries_answer_without_a_trace(row):
    """ramnet_wgrad_slabs is a function of the shape alone (no pitch, no pointer): the same answer for both siblings, the channel-only
    query's; ramnet_fold_wgrad_variant answers 0 (not a folded launch); ramnet_last_error() untouched"""
    L = _lib()
    per_fam = {"2x2": L.ramnet_wgrad_wino_slabs, "2x4": L.ramnet_wgrad_wino2x4_slabs, "dsplit": L.ramnet_wgrad_dsplit_slabs}[row.fam]
    Cin = 4 * row.C0 if row.mode == cr.IN_S2D else row.C0 + row.C1
    for refused in (False, True):
        if refused and row.kind == "none":
            continue
        segs, f, s, keep = _wgrad_struct(row, refused)
        mark = _mark_error(L)
        slabs, fold = L.ramnet_wgrad_slabs(C.byref(s)), L.ramnet_fold_wgrad_variant(C.byref(s), 1)
        fits = L.ramnet_wgrad_addressable(C.byref(s))
        assert L.ramnet_last_error() == mark, "a query touched ramnet_last_error()"
        assert fits == int(not refused), "ramnet_wgrad_addressable answers %d" % fits
        assert slabs == per_fam(Cin, row.Cout) >= 1 and fold == 0


# ---------------------------------------------------------------------------------------------------- folded decoders and head
def _fh_struct(row, refused):
    c, d = al.fh_data(row)
    cls, entry, f, _ = al.fh_fields(row, c, d, al.Dummy(), refused, dw=1 << 30, dbias=(1 << 30) + 4096)
    return c, d, entry, al.struct(cls, f)


@pytest.mark.parametrize("row", FOLDHEAD, ids=[r.name for r in FOLDHEAD])
def test_fold_head_row_reaches_its_limit(row):
    px, limit, unit = al.fh_limit(row)
    ld, ch = al.fh_ld(row), al.fh_channels(row)
    highest = ((px - 1) * ld + ch) * unit               # (unit 8: the backward-weights guard counts every byte twice)
    print("%s: pitch %d floats, %d pixels, highest %d, limit %d, distance %d = %.4f pitches" % (row.name, ld, px, highest, limit, limit - highest,
                                                                                                (limit - highest) / (ld * unit)))
    assert ld % 4 == 0 and ld >= ch
    if row.kind == "none":
        assert ((px - 1) * ld + ch) * 4 > 1 << 32, "the row does not leave the range of a 32-bit byte offset"
        return
    assert px * ld * unit < limit <= px * (ld + 4) * unit, "the pitch is not the largest the guard accepts"
    assert 0 <= px * ld * unit - highest < ld * unit and 0 < limit - px * ld * unit <= 4 * px * unit, "the row does not reach its limit"


@pytest.mark.parametrize("row", [r for r in FOLDHEAD if r.kind != "none"], ids=[r.name for r in FOLDHEAD if r.kind != "none"])
def test_fold_sibling_is_refused_before_any_launch(row):
    L = _lib()
    c, d, entry, s = _fh_struct(row, True)
    assert getattr(L, entry)(C.byref(s), None) == BADARG
    err = L.ramnet_last_error()
    assert b"bad argument" in err and FH_FRAGMENT[row.launch] in err, err


@pytest.mark.parametrize("row", FOLDHEAD, ids=[r.name for r in FOLDHEAD])
def test_fold_head_queries_answer_without_a_trace(row):
    """ramnet_fold_wino_variant / ramnet_fold_halfwg_variant / ramnet_fold_wgrad_variant / ramnet_wgrad_slabs choose the form of a launch from
    its shape (no pitch enters them): the same answer for both siblings — the form the "below" launch runs and the refused one would —,
    ramnet_last_error() untouched"""
    L = _lib()
    answers = []
    for refused in (False, True):
        if refused and row.kind == "none":
            continue
        c, d, entry, s = _fh_struct(row, refused)
        mark = _mark_error(L)
        if entry == "ramnet_conv_launch":
            as24 = al.struct(_hip.ConvDesc, {})
            C.memmove(C.byref(as24), C.byref(s), C.sizeof(s))
            if row.fam != "head":
                as24.algo = _hip.ALGO_WINOGRAD24
            got = (L.ramnet_fold_wino_variant(C.byref(as24), 1), L.ramnet_fold_halfwg_variant(C.byref(s), 1), L.ramnet_conv_wino_variant(C.byref(s), 1),
                   L.ramnet_conv_wino_split_ok(C.byref(s), 1))
            want = (int(row.fam != "head" and not (row.C0 % 32 and row.launch == "fold_fwd")), int(row.fam == "fold2x3"), 0, 0)
        else:
            as24 = al.struct(_hip.WgradDesc, {})
            C.memmove(C.byref(as24), C.byref(s), C.sizeof(s))
            if row.fam != "head":
                as24.algo = _hip.ALGO_WINOGRAD24
            got = (L.ramnet_fold_wgrad_variant(C.byref(as24), 1), int(L.ramnet_wgrad_slabs(C.byref(s)) >= 1))
            want = (int(row.fam != "head"), 1)
        fits = (L.ramnet_conv_addressable if entry == "ramnet_conv_launch" else L.ramnet_wgrad_addressable)(C.byref(s))
        assert L.ramnet_last_error() == mark, "a query touched ramnet_last_error()"
        assert got == want, (got, want)
        assert fits == int(not refused), "the addressable query answers %d" % fits
        answers.append(got)
    assert len(set(answers)) == 1


@pytest.mark.parametrize("row", [r for r in FOLDHEAD if r.launch.startswith("fold")], ids=[r.name for r in FOLDHEAD if r.launch.startswith("fold")])
def test_fold_rows_are_exact_in_fp32(row):
    c, d = al.fh_data(row)
    if row.launch == "fold_fwd":
        assert cr.fold_exact_ok(cr.fold_statement(d, row.fam, pair=row.Cout == 32 and row.C0 % 32 == 0), row.fam)
    elif row.launch == "fold_dgrad":
        assert float(cr.parity4_wino(d.x0, d.w5, row.fam).max()) * 2.0 ** cr.GRID_BITS[row.fam] < 2 ** 24
    else:
        st = cr.fold_wgrad_statement(d)
        assert float(cr.fold_wgrad_wino(d, row.fam)[0].max()) * 2.0 ** cr.WGRAD_GRID_BITS[row.fam] < 2 ** 24 and torch.equal(st.dW4, st.dW4.round())
        assert float(st.dbias_abs.max()) * 16 < 2 ** 24


@pytest.mark.parametrize("row", [r for r in FOLDHEAD if r.fam == "head"], ids=[r.name for r in FOLDHEAD if r.fam == "head"])
def test_head_rows_are_exact_in_fp32(row):
    import types
    c, d = al.fh_data(row)
    if row.launch == "head_fwd":
        assert cr.exact_ok(cr.conv_statement(d, "direct"), "direct")
    else:
        st = cr.wgrad_statement(types.SimpleNamespace(**dict(vars(d), taps=[t[:2] for t in d.taps])))
        assert float(st.dW_abs.max()) * 16 < 2 ** 24 and float(st.dbias_abs.max()) * 16 < 2 ** 24


def test_head_forward_is_bounded_like_the_direct_family():
    """check_desc bounds the sources of EVERY family by 2^32 elements: the head's x0 at the first refused pitch (no GPU row: a buffer that spans
    it takes 17 GB, and the direct family's row exercises the same line)"""
    L = _lib()
    row = al.BY_NAME["head_x0-head"]
    c, d = al.fh_data(row)
    cls, entry, f, _ = al.fh_fields(row, c, d, al.Dummy())
    f["ld0"] = al.largest_ld(row.B * al.H * al.W, 1 << 32, 1) + 4
    assert L.ramnet_conv_launch(C.byref(al.struct(cls, f)), None) == BADARG
    assert FRAGMENT[("conv", "direct")] in L.ramnet_last_error()


# ---------------------------------------------------------------------------------------------------- weight limits: refusal side only
def _fold_desc(C0, Cout, dgrad):
    Hc, Wc, B = 10, 12, 1
    f = dict(x0=1 << 20, w=2 << 20, out=3 << 20, B=B, C0=C0, Cout=Cout, ld0=C0, ldo=Cout, stride=1, ntaps=25, epi=_hip.EPI_LINEAR,
             osy=1, osx=1, algo=_hip.ALGO_WINOGRAD24)
    if dgrad:
        f.update(in_mode=_hip.IN_PARITY4, Hin=2 * Hc, Win=2 * Wc, Ho=Hc + 4, Wo=Wc + 4, HoF=Hc + 4, WoF=Wc + 4)
    else:
        f.update(in_mode=_hip.IN_PLAIN, Hin=Hc + 4, Win=Wc + 4, Ho=Hc, Wo=Wc, HoF=2 * Hc, WoF=2 * Wc)
    return f


@pytest.mark.parametrize("algo", ["WINOGRAD24", "WINOGRAD24_2X3"])
@pytest.mark.parametrize("dgrad", [False, True])
def test_folded_weight_limit_is_refused(algo, dgrad):
    """packed weights of the folded families: 100 (F(2x2,4x4)) or 120 (F(2x3,4x4)) x C0 x Cout floats below 0x7fffffff bytes — the smallest
    channel product beyond it is refused, the one below it is not refused FOR THAT (asked through nothing: it would launch)"""
    L = _lib()
    per = 120 if algo.endswith("2X3") else 100
    C0 = 2304
    Cout = -(-0x7fffffff // (per * 4 * C0)) // 64 * 64 + 64          # the first multiple of 64 with per * C0 * Cout * 4 >= 0x7fffffff
    assert per * C0 * Cout * 4 >= 0x7fffffff > per * C0 * (Cout - 64) * 4
    f = dict(_fold_desc(C0, Cout, dgrad), algo=getattr(_hip, "ALGO_" + algo))
    assert L.ramnet_conv_launch(C.byref(al.struct(_hip.ConvDesc, f)), None) == BADARG
    err = L.ramnet_last_error()
    assert b"bad argument" in err and b"wb < FOLD_W_LIMIT" in err, err


# ---------------------------------------------------------------------------------------------------- the data rule
@pytest.mark.parametrize("row", [r for r in CONV if r.case.kind == "int"], ids=[r.name for r in CONV if r.case.kind == "int"])
def test_conv_rows_are_exact_in_fp32(row):
    """the exact integer rule of tests/conv_launch_cases.py: statement and absolute-value statement (transformed domain for the Winograd
    families) are multiples of 1/16 below 2^24 / 16"""
    d = al.conv_build(row)
    assert cr.exact_ok(cr.conv_statement(d, row.fam), row.fam)


@pytest.mark.parametrize("row", WGRAD, ids=[r.name for r in WGRAD])
def test_wgrad_rows_are_exact_in_fp32(row):
    d = al.wgrad_build_all(row)
    st = cr.wgrad_statement(d)
    top = st.dW_abs if row.fam == "dsplit" else cr.wgrad_wino(d, row.fam)[0]
    assert float(top.max()) * 16 < 2 ** 24 and torch.equal(st.dW, st.dW.round())
    assert float(st.dbias_abs.max()) * 16 < 2 ** 24


# ---------------------------------------------------------------------------------------------------- the callers: ops.py at the limits
def _meta(*shape):
    return torch.empty(*shape, device="meta")


def test_ops_asks_the_library_before_it_picks_a_family():
    """The decisions of ops.py at the smallest real sizes that cross (host arithmetic: tensors without storage).  Decoder backward-weights
    (UpsampleConvLayer(64, 32)): at dy = [2][2048][2048][32] twice its bytes reach WOOB, the one-launch folded kernel cannot address it and
    the four direct parity launches take the pass; one row short it can.  Decoder backward-data: both sides of 2^30 bytes of dy.
    F(2x4,3x3) / F(2x2,3x3) backward-weights of a 64-channel 3x3 layer: at [2][2048][2048][64] the whole tensor reaches 2^31 bytes and the
    layer's pass takes the direct layout; one row below the Winograd one."""
    import types
    from rpg_ramnet_amd import ops
    assert ops._fold_desc_fits("wgrad", 2, 1023, 1024, 64, 32) and not ops._fold_desc_fits("wgrad", 2, 1024, 1024, 64, 32)
    assert 2 * 2048 * 2048 * 32 * 4 == 2 ** 30
    assert ops._fold_desc_fits("dgrad", 2, 1023, 1024, 64, 32) and not ops._fold_desc_fits("dgrad", 2, 1024, 1024, 64, 32)
    cp = types.SimpleNamespace(Cout=32, Cin=64)
    with ops.switches(fold_dgrad=True, fold_upsample=True):
        assert ops._fold_dgrad_ok(2, 2046, 2048, cp) and not ops._fold_dgrad_ok(2, 2048, 2048, cp)
    big, below = _meta(2, 2048, 2048, 64), _meta(2, 2047, 2048, 64)
    assert ops._wino_wgrad_fits(below, below, gmask=below) and not ops._wino_wgrad_fits(big, big)
    assert not ops._wino_wgrad_fits(below, big) and not ops._wino_wgrad_fits(below, below, gmask=_meta(2, 2047, 2048, 128)[..., :64])    # (a mask of twice the pitch)
    layer = ops.ConvParam([torch.zeros(64, 64, 3, 3)], [torch.zeros(64)])
    layer._slabs = 1
    with ops.switches(wgrad_winograd_2x4="force"):
        assert layer._choose_layout(True, True)[0] in ("wino6", "dsplit") and layer._choose_layout(True, False)[0] == "direct"
    with ops.switches(wgrad_winograd_2x4="off"):
        assert layer._choose_layout(True, True)[0] == "wino" and layer._choose_layout(True, False)[0] == "direct"


# ---------------------------------------------------------------------------------------------------- the layers of section 5: the data rule
import address_limit_layers as ll


@pytest.mark.parametrize("c", ll.CASES, ids=[c.name for c in ll.CASES])
def test_layer_rows_are_exact_in_fp32(c):
    """The generated data of the whole-layer rows: every statement on absolute values (pre-activations, the hidden map, every weight, bias
    and input gradient) times the growth of the transforms stays below 2^24 on its grid — the decoder's values are multiples of 1/16 (the
    bilinear weights) and the folded Winograd transforms grow them by at most 2^6 (rows of |B^T| sum to 6 per axis: 36), the block's are
    integers and the F(2x4,3x3) transforms grow them by at most 100 < 2^7 (rows of |B^T| sum to 10) — and the samples cover what the issue
    asks: all of dW and dbias, at least 256 input pixels, the four corners and the last rows of the last image."""
    r = ll.reference_once(c)
    grow = 2 ** 10 if c.layer == "decoder" else 2 ** 8
    assert r.top * grow < 2 ** 24, "absolute statement %.1f" % r.top
    for k, v in r.grads.items():
        assert torch.equal(v * 16, (v * 16).round()) and int((v != 0).sum()) >= (256 if v.dim() > 1 else 16), k
    assert r.dx_pix.numel() >= 256 and torch.equal(r.dx * 16, (r.dx * 16).round())
    Ho, Wo = ll.out_map(c)
    have = {tuple(p) for p in r.S.tolist()}
    assert all((b, y, x) in have for b in (0, c.B - 1) for y in (0, Ho - 1) for x in (0, Wo - 1))
    assert sum(1 for b, y, x in have if b == c.B - 1 and y >= Ho - 2) >= 16
    last = (c.B * c.H * c.W) - 1                       # the last input pixel of the last image carries a gradient
    assert int(r.dx_pix.max()) == last and bool(r.dx[-1].abs().sum() > 0)
    # the sizes are the ones that cross (bytes of the tensor the limit is about)
    bytes_ = c.B * Ho * Wo * c.Cout * 4
    if c.layer == "decoder":
        assert (bytes_ >= 2 ** 30) == c.name.endswith("_at") and (2 * bytes_ >= al.WOOB) == c.name.endswith("_at")
    else:                                              # (the conv rows: B = 1, the image is the tensor)
        assert (bytes_ >= al.WOOB) == c.name.endswith("_at")
