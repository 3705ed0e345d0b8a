"""The case table of the 32-bit addressing limits of the convolution launches (profiles/address_limit_tests_notes.md), shared by
tests/test_address_limits_cpu.py (no GPU: how close every row gets to its limit, the refusal of its sibling, the quiet queries, the data
rule) and tests/test_hip_address_limits.py (the launches, every operand in allocated memory).

The size comes from the PITCH, not from the map: a 9 x 11 map (ragged in every tile shape of every family) whose inflated operand has a
leading dimension of millions of floats spans just under its limit while the launch computes a few hundred pixels.  A row inflates ONE
operand; every other operand keeps its channels + 4 floats.  `ld` of a row is the LARGEST pitch (a multiple of 4 floats, which every family
requires) its guard accepts; the "first refused" sibling is the same descriptor at ld + 4.

Row kinds:  "image"   the guard bounds ONE image of the operand: B = 2, image 1 starts 2 GB behind the base
            "tensor"  the guard bounds the whole tensor (of a segment)
            "none"    the family claims no limit for the operand: one row beyond 2^32 bytes, no sibling
"""
import types

import torch

import conv_launch_cases as cc
import conv_restatement as cr
from rpg_ramnet_amd import _hip

F64 = torch.float64
WOOB = 0x7fffff00                # csrc/common.hpp
H, W = 9, 11                     # the map of every row
SURPLUS = 4                      # floats by which every other operand's pitch exceeds its channels
LD_FIELD = {"x0": "ld0", "x1": "ld1", "xm": "ldm", "out": "ldo", "o1": "ldo1", "o2": "ldo2", "e0": "lde0", "e1": "lde1", "dout": "ldg", "gmask": "ldgm"}
SOURCES = ("x0", "x1", "xm")
ALGO = {"direct": _hip.ALGO_DIRECT, "2x2": _hip.ALGO_WINOGRAD, "2x4": _hip.ALGO_WINOGRAD_2X4, "2x4split": _hip.ALGO_WINOGRAD_2X4_SPLIT,
        "dsplit": _hip.ALGO_DIRECT_SPLIT}
WINO3 = ("2x2", "2x4", "2x4split")


def largest_ld(span_px, limit, unit):
    """the largest multiple of 4 floats with span_px * ld * unit < limit"""
    return (limit - 1) // (span_px * unit) // 4 * 4


# ---------------------------------------------------------------------------------------------------- forward / backward-data
def _conv(name, fams, operand, kind="image", **kw):
    """`kw`: the row of tests/conv_launch_cases.py the launch is (map and batch fixed here; kind_data: its data kind, "int" = the exact rule)"""
    C0, Cout, data = kw.pop("C0", 16), kw.pop("Cout", 64), kw.pop("kind_data", "int")
    return [types.SimpleNamespace(name="%s-%s" % (name, f), launch="conv", fam=f, operand=operand, kind=kind,
                                  case=cc._case("limit_" + name, (f,), 2, H, W, C0, Cout, kind=data, **kw)) for f in fams]


def _conv_rows():
    t = []
    t += _conv("x0", WINO3, "x0")
    t += _conv("x1_cat", WINO3, "x1", C1=16, mode=cr.IN_CAT)
    t += _conv("xm_catmul", WINO3, "xm", C1=16, mode=cr.IN_CAT_MUL)
    t += _conv("xm_relumask", WINO3, "xm", mode=cr.IN_RELUMASK)
    t += _conv("x0_s2d", WINO3, "x0", mode=cr.IN_S2D)
    t += _conv("out_beta1", WINO3, "out", epi=cr.EPI_LINEAR, beta=1.0)
    t += _conv("out_s2d", WINO3, "out", epi=cr.EPI_LINEAR, bias=False, out_s2d=16, transposed=True)
    t += _conv("e0_res", WINO3, "e0", epi=cr.EPI_RES_RELU)
    for op in ("e0", "e1", "o1"):                   # exact on integers: the three epilogue operands of the ConvGRU backward stage
        t += _conv("%s_grubwd" % op, WINO3, op, Cout=128, epi=cr.EPI_GRU_BWD, bias=False, transposed=True)
    for op in ("o1", "e1"):                         # the cell epilogues: normal data, the measured rule of tests/test_hip_conv_launch.py
        t += _conv("%s_hr" % op, WINO3, op, Cout=128, epi=cr.EPI_SIGMOID_HR, kind_data="normal", C1=16, mode=cr.IN_CAT)
    for op in ("o1", "e0"):
        t += _conv("%s_blend" % op, WINO3, op, epi=cr.EPI_GRU_BLEND, kind_data="normal", C1=16, mode=cr.IN_CAT_MUL)
    for op in ("out", "o1", "e1", "o2"):
        fams = ("2x4",) if op == "o2" else ("2x2", "2x4")
        t += _conv("%s_lstm" % op, fams, op, C0=8, Cout=16, epi=cr.EPI_LSTM, kind_data="normal", C1=16, mode=cr.IN_CAT)
    # F(2x2,3x3) stores the gates through 64-bit pointers and bounds them by nothing: one image of o2 BEYOND 2^31 bytes
    t += _conv("o2_lstm", ("2x2",), "o2", kind="none", C0=8, Cout=16, epi=cr.EPI_LSTM, kind_data="normal", C1=16, mode=cr.IN_CAT)
    # the direct family: 64-bit addresses, the guard of check_desc alone (B * Hin * Win * ld < 2^32 ELEMENTS of the sources)
    t += _conv("x0", ("direct",), "x0", kind="tensor")
    return t


def conv_build(row):
    """the float64 descriptor of a forward row (conv_launch_cases.build)"""
    return cc.build(row.case)


def conv_limit(row, d):
    """(pixels the guard multiplies the pitch by, limit, unit of the limit in bytes per float) — the restatement of check_offsets32
    (csrc/conv_plan.hpp) and, for the direct family, of check_desc (csrc/conv_igemm.hip)"""
    src = row.operand in SOURCES
    if row.fam == "direct":
        assert src
        return d.B * d.Hin * d.Win, 1 << 32, 1
    if src:
        return d.Hin * d.Win * (4 if d.in_mode == cr.IN_S2D else 1), WOOB, 4
    return d.HoF * d.WoF, WOOB, 4


def conv_channels(row, d):
    """channels the launch addresses through the inflated pitch (the window behind the operand's pointer)"""
    C = d.Cout
    return {"x0": d.C0, "x1": d.C1, "xm": d.C1 if d.in_mode == cr.IN_CAT_MUL else d.C0, "out": d.out_s2d or C,
            "o1": C // 2 if d.epi == cr.EPI_SIGMOID_HR else C, "o2": 4 * C,
            "e0": C, "e1": C // 2 if d.epi in (cr.EPI_SIGMOID_HR, cr.EPI_GRU_BWD) else C}[row.operand]


def conv_ld(row, d):
    """the row's pitch: the largest its guard accepts (kind "none": an image of 2^31 bytes and a quarter)"""
    px, limit, unit = conv_limit(row, d)
    if row.kind == "none":
        return ((5 << 29) // (px * 4) + 3) // 4 * 4
    return largest_ld(px, limit, unit)


def conv_fields(row, d, mk, refused=False):
    """The descriptor fields of a forward row, every tensor made by `mk` (GPU: guarded buffers, the inflated one on the device; CPU: dummy
    addresses): mk.inp(operand, data, ld), mk.out(operand, rows, cols, ld, col0, prefill), mk.weights(d, fam, k).  Returns (fields, outputs)."""
    c, fam, p = row.case, row.fam, SURPLUS
    big = conv_ld(row, d) + (4 if refused else 0)

    def ld(op, natural):
        return big if op == row.operand else natural + p
    f = dict(in_mode=d.in_mode, B=d.B, Hin=d.Hin, Win=d.Win, C0=d.C0, C1=d.C1 if d.x1 is not None else 0, stride=d.stride, ntaps=len(d.taps),
             dy=[t[0] for t in d.taps], dx=[t[1] for t in d.taps], wtap=[t[2] for t in d.taps], Cout=d.Cout, Ho=d.Ho, Wo=d.Wo, HoF=d.HoF, WoF=d.WoF,
             osy=1, osx=1, ooy=0, oox=0, epi=d.epi, beta=d.beta, algo=ALGO[fam], out_s2d=d.out_s2d, s2d_5x5=d.s2d_5x5)
    f["ld0"] = ld("x0", d.C0)
    f["x0"] = mk.inp("x0", d.x0, f["ld0"])
    if d.x1 is not None:
        f["ld1"] = ld("x1", d.C1)
        f["x1"] = mk.inp("x1", d.x1, f["ld1"])
    if d.xm is not None:
        f["ldm"] = ld("xm", d.xm.shape[3])
        f["xm"] = mk.inp("xm", d.xm, f["ldm"])
    f["w"] = mk.weights(d, fam, c.k)
    if d.bias is not None:
        f["bias"] = mk.inp("bias", d.bias, d.bias.numel())
    npix, outs = d.B * d.HoF * d.WoF, {}
    Co = d.out_s2d if d.out_s2d else d.Cout
    f["ldo"] = ld("out", Co)
    outs["out"] = f["out"] = mk.out("out", npix, Co, f["ldo"], 0, d.out_old)
    if d.e0 is not None:
        f["lde0"] = ld("e0", d.e0.shape[3])
        f["e0"] = mk.inp("e0", d.e0, f["lde0"])
    if d.e1 is not None:
        f["lde1"] = ld("e1", d.e1.shape[3])
        f["e1"] = mk.inp("e1", d.e1, f["lde1"])
    if d.epi == cr.EPI_SIGMOID_HR:
        f["ldo1"] = ld("o1", d.Cout // 2)
        outs["o1"] = f["o1"] = mk.out("o1", npix, d.Cout // 2, f["ldo1"], 0, None)
    elif d.epi in (cr.EPI_GRU_BLEND, cr.EPI_LSTM):
        f["ldo1"] = ld("o1", d.Cout)
        outs["o1"] = f["o1"] = mk.out("o1", npix, d.Cout, f["ldo1"], 0, None)
    elif d.epi == cr.EPI_GRU_BWD:                   # only the channels n >= C of o1 are written: the first half is a gap
        f["ldo1"] = ld("o1", d.Cout)
        outs["o1"] = f["o1"] = mk.out("o1", npix, d.Cout // 2, f["ldo1"], d.Cout // 2, None)
    if d.epi == cr.EPI_LSTM:
        f["ldo2"] = ld("o2", 4 * d.Cout)
        outs["o2"] = f["o2"] = mk.out("o2", npix, 4 * d.Cout, f["ldo2"], 0, None)
    assert LD_FIELD[row.operand] in f and f[LD_FIELD[row.operand]] == big, "the row's operand is not part of its launch"
    return f, outs


# ---------------------------------------------------------------------------------------------------- backward-weights
def _wgrad(name, fams, operand, kind, mode=cr.IN_PLAIN, C0=32, C1=0, Cout=64, gmask=False, B=2, nseg=1):
    return [types.SimpleNamespace(name="wgrad_%s-%s" % (name, f), launch="wgrad", fam=f, operand=operand, kind=kind if f != "dsplit" else "none",
                                  mode=mode, C0=C0, C1=C1, Cout=Cout, gmask=gmask or operand == "gmask", B=B, nseg=nseg) for f in fams]


def _wgrad_rows():
    t = []
    for fam in ("2x2", "2x4"):                      # both bound the WHOLE tensor: two images, the second one 1 GB behind the first
        f = (fam,)
        t += _wgrad("x0", f, "x0", "tensor")
        t += _wgrad("x1_cat", f, "x1", "tensor", cr.IN_CAT, C1=8, gmask=True)
        t += _wgrad("xm_catmul", f, "xm", "tensor", cr.IN_CAT_MUL, C1=12)
        t += _wgrad("xm_relumask", f, "xm", "tensor", cr.IN_RELUMASK, C0=36, gmask=True)
        t += _wgrad("x0_s2d", f, "x0", "tensor", cr.IN_S2D)
        t += _wgrad("dout", f, "dout", "tensor")
        t += _wgrad("gmask", f, "gmask", "tensor")
        t += _wgrad("x0_B3", f, "x0", "tensor", B=3)
        t += _wgrad("dout_B3", f, "dout", "tensor", B=3, gmask=True)
    # F(2x4,3x3): three segments with the inflated operand in the last one (the pitch is the descriptor's: every segment's tensor has it,
    # and every one is allocated)
    t += _wgrad("x0_seg3", ("2x4",), "x0", "tensor", nseg=3)
    t += _wgrad("dout_seg3", ("2x4",), "dout", "tensor", cr.IN_CAT, C1=8, nseg=3)
    # dsplit claims no limit (64-bit pixel indices): x0 beyond 2^32 bytes
    t += _wgrad("x0", ("dsplit",), "x0", "none")
    return t


def wgrad_build(row, seg=0):
    """the float64 backward-weights descriptor of a row (tests/conv_restatement.py: wgrad_statement): integers, half of them zero"""
    g = cc._gen("limit %s seg %d" % (row.name, seg))

    def data(shape, m=2):
        return cc._ri(g, shape, m) * (torch.rand(shape, generator=g) < 0.5).to(F64)
    s2 = 2 if row.mode == cr.IN_S2D else 1
    B, C0, C1, Cout = row.B, row.C0, row.C1, row.Cout
    d = types.SimpleNamespace(in_mode=row.mode, x0=data((B, s2 * H, s2 * W, C0)), x1=data((B, H, W, C1)) if C1 else None, xm=None, stride=1, Ho=H, Wo=W,
                              taps=[(a - 1, b - 1) for a in range(3) for b in range(3)], dout=data((B, H, W, Cout), 4),
                              gmask=data((B, H, W, Cout), 1) if row.gmask else None, Cin=4 * C0 if row.mode == cr.IN_S2D else C0 + C1, Cout=Cout, B=B)
    if row.mode == cr.IN_CAT_MUL:
        d.xm = data((B, H, W, C1))
    if row.mode == cr.IN_RELUMASK:
        d.xm = data((B, H, W, C0), 1)
    return d


def wgrad_build_all(row):
    """the descriptor over all segments of a row (d.segs) as wgrad_statement takes it"""
    segs = [wgrad_build(row, k) for k in range(row.nseg)]
    d = types.SimpleNamespace(**vars(segs[0]))
    d.segs = segs
    return d


def wgrad_limit(row):
    """(pixels, limit in bytes): pixels * ld * 4 < limit is what the pitch of the row's operand must satisfy — the restatement of
    wgrad_offsets32 (csrc/conv_plan.hpp): lane and scalar offset are range-checked together, so the whole tensor of B images and, for the
    sources, the halo in front of the first strip (one row and one pixel; the space-to-depth view: two rows and two pixels of the stored
    image) end below WOOB"""
    s2d = row.mode == cr.IN_S2D
    if row.operand in ("x0", "x1"):
        return row.B * H * W * (4 if s2d else 1) + ((4 * W + 2) if s2d else W + 1), WOOB
    if row.operand == "xm":
        return row.B * H * W + W + 1, WOOB
    return row.B * H * W, WOOB


def wgrad_ld(row):
    if row.kind == "none":                          # the whole tensor: 2^32 bytes and an eighth
        return ((9 << 29) // (row.B * H * W * 4) + 3) // 4 * 4
    return largest_ld(*wgrad_limit(row), 4)


def wgrad_channels(row):
    return {"x0": row.C0, "x1": row.C1, "xm": row.C1 if row.mode == cr.IN_CAT_MUL else row.C0, "dout": row.Cout, "gmask": row.Cout}[row.operand]


def wgrad_fields(row, segs, mk, dw, dbias, slabs, refused=False):
    """descriptor fields of a backward-weights row; `segs`: the float64 descriptors of its segments; returns (fields, the ctypes segment
    array or None — the caller keeps it alive)"""
    p, big = SURPLUS, wgrad_ld(row) + (4 if refused else 0)

    def ld(op, natural):
        return big if op == row.operand else natural + p
    d = segs[0]
    f = dict(C0=row.C0, C1=row.C1, in_mode=row.mode, B=row.B, Hin=H, Win=W, ntaps=9, stride=1, dy=[t[0] for t in d.taps], dx=[t[1] for t in d.taps],
             Cout=row.Cout, Ho=H, Wo=W, dw=dw, algo=ALGO[row.fam], dw_slabs=slabs, ld0=ld("x0", row.C0), ldg=ld("dout", row.Cout))
    if dbias is not None:
        f["dbias"] = dbias
    if d.x1 is not None:
        f["ld1"] = ld("x1", row.C1)
    if d.xm is not None:
        f["ldm"] = ld("xm", d.xm.shape[3])
    if d.gmask is not None:
        f["ldgm"] = ld("gmask", row.Cout)
    per_seg = []
    for k, s in enumerate(segs):
        one = dict(x0=mk.inp("x0", s.x0, f["ld0"], k), dout=mk.inp("dout", s.dout, f["ldg"], k))
        if s.x1 is not None:
            one["x1"] = mk.inp("x1", s.x1, f["ld1"], k)
        if s.xm is not None:
            one["xm"] = mk.inp("xm", s.xm, f["ldm"], k)
        if s.gmask is not None:
            one["gmask"] = mk.inp("gmask", s.gmask, f["ldgm"], k)
        per_seg.append(one)
    f.update(per_seg[0])
    assert f[LD_FIELD[row.operand]] == big, "the row's operand is not part of its launch"
    return f, per_seg


# ---------------------------------------------------------------------------------------------------- folded decoders and head
# 10 x 12 low-resolution maps: x0 is the padded [B][14][16][C0] tensor, the full-resolution side [B][20][24][.]
FH, FW = 10, 12
FOLD_ALGO = {"fold2x2": _hip.ALGO_WINOGRAD24, "fold2x3": _hip.ALGO_WINOGRAD24_2X3}
FOLD_TAPS = cr.fold_taps(0, 0)


def _fold_rows():
    def row(name, launch, fam, operand, kind="tensor", **kw):
        r = dict(name="%s-%s" % (name, fam), launch=launch, fam=fam, operand=operand, kind=kind, B=2, C0=32, Cout=64, gmask=False, fold_pair=1, half=0)
        r.update(kw)
        return types.SimpleNamespace(**r)
    t = []
    for fam in ("fold2x2", "fold2x3"):
        # forward: the whole x0 below 0xffffffff bytes; 64-column workgroups, the pair form of the 32-channel layers
        t.append(row("fold_x0", "fold_fwd", fam, "x0"))
        t.append(row("fold_x0_pair", "fold_fwd", fam, "x0", Cout=32))
        # PARITY4 backward-data: the whole full-resolution gradient below 2^30 bytes (invalid window elements use offsets from 2^30 up)
        t.append(row("fold_dgrad_x0", "fold_dgrad", fam, "x0", C0=16))
        # backward-weights: twice the bytes of x0 / dout / gmask below WOOB (a tile past the last one stands up to a grid stride beyond)
        t.append(row("fold_wgrad_x0", "fold_wgrad", fam, "x0"))
        t.append(row("fold_wgrad_dout", "fold_wgrad", fam, "dout", gmask=True))
        t.append(row("fold_wgrad_gmask", "fold_wgrad", fam, "gmask", gmask=True, C0=64, Cout=32))
    t.append(row("fold_x0_c16", "fold_fwd", "fold2x2", "x0", C0=16, Cout=32))             # 32-column workgroups, chunks of 8
    t.append(row("fold_x0_half", "fold_fwd", "fold2x3", "x0", half=1))                    # the half-workgroup form of F(2x3,4x4)
    t.append(row("fold_x0_pair_half", "fold_fwd", "fold2x3", "x0", Cout=32, half=1))
    t.append(row("fold_dgrad_x0_half", "fold_dgrad", "fold2x3", "x0", C0=16, half=1))
    # the folded forward stores through 64-bit indices: `out` beyond 2^32 bytes
    t.append(row("fold_out", "fold_fwd", "fold2x2", "out", kind="none"))
    # the head addresses everything through 64-bit indices; check_desc bounds the forward's x0 by 2^32 ELEMENTS like the direct family's
    # (one row of 17 GB there, none here): x0, out, dout beyond 2^32 BYTES
    t.append(row("head_x0", "head_fwd", "head", "x0", kind="none", C0=8, Cout=32))
    t.append(row("head_out", "head_fwd", "head", "out", kind="none", C0=8, Cout=32))
    t.append(row("head_wgrad_x0", "head_wgrad", "head", "x0", kind="none", C0=8, Cout=32, gmask=True))
    t.append(row("head_wgrad_dout", "head_wgrad", "head", "dout", kind="none", C0=8, Cout=32, gmask=True))
    return t


def fh_limit(row):
    """(pixels, limit, bytes the guard counts per float): launch_wino24 / launch_wino24_dgrad (csrc/conv_wino24.hip) and
    launch_wgrad_wino24 (csrc/conv_wgrad_wino24.hip); kind "none": 2^32 bytes, which the row exceeds"""
    low, full = row.B * (FH + 4) * (FW + 4), row.B * 2 * FH * 2 * FW
    if row.launch == "fold_fwd":
        return (low, 0xffffffff, 4) if row.operand == "x0" else (full, 1 << 32, 4)
    if row.launch == "fold_dgrad":
        return full, 1 << 30, 4
    if row.launch == "fold_wgrad":
        return (low if row.operand == "x0" else full), WOOB, 8
    return row.B * H * W, 1 << 32, 4                # the head: a 9 x 11 map


def fh_ld(row):
    px, limit, unit = fh_limit(row)
    if row.kind == "none":
        return ((9 << 29) // (px * 4) + 3) // 4 * 4
    return largest_ld(px, limit, unit)


def fh_channels(row):
    if row.launch == "fold_dgrad":
        return row.C0
    return {"x0": row.C0, "out": row.Cout, "dout": row.Cout, "gmask": row.Cout}[row.operand]


def fh_data(row):
    """the float64 operands of a folded / head row: integers by the rules of tests/fold_head_cases.py"""
    import fold_head_cases as fh
    if row.launch == "fold_fwd":
        c = fh._fold("limit_" + row.name, row.fam, row.B, FH, FW, row.C0, row.Cout, "", wd=0.125, xd=0.25, fold_pair=row.fold_pair)
        return c, fh.build_fold(c)
    g = fh._gen("limit_" + row.name)
    if row.launch == "fold_dgrad":                  # C0 = the layer's output channels, Cout = its input channels
        return None, types.SimpleNamespace(in_mode=cr.IN_PARITY4, x0=fh._sparse(g, (row.B, 2 * FH, 2 * FW, row.C0), 1, 0.25),
                                           w5=9.0 * fh._sparse(g, (row.C0, row.Cout, 5, 5), 1, 0.125))
    if row.launch == "fold_wgrad":
        return None, types.SimpleNamespace(x0=fh._sparse(g, (row.B, FH + 4, FW + 4, row.C0), 1, 0.5), dout=fh._sparse(g, (row.B, 2 * FH, 2 * FW, row.Cout), 2, 0.5),
                                           gmask=fh._sparse(g, (row.B, 2 * FH, 2 * FW, row.Cout), 1, 0.5) if row.gmask else None, Ho=FH, Wo=FW)
    c = fh._head("limit_" + row.name, 5, row.C0, row.Cout, row.B, H, W, gmask=row.gmask)
    return c, fh.build_head(c)


def fh_fields(row, c, d, mk, refused=False, dw=None, dbias=None, slabs=0):
    """(struct class, entry point, fields, outputs) of a folded / head row"""
    p, big = SURPLUS, fh_ld(row) + (4 if refused else 0)

    def ld(op, natural):
        return big if op == row.operand else natural + p
    B, C0, Cout, outs = row.B, row.C0, row.Cout, {}
    if row.launch == "fold_fwd":
        f = dict(in_mode=_hip.IN_PLAIN, B=B, Hin=FH + 4, Win=FW + 4, C0=C0, stride=1, Cout=Cout, Ho=FH, Wo=FW, HoF=2 * FH, WoF=2 * FW, osy=1, osx=1,
                 epi=c.epi, beta=0.0, algo=FOLD_ALGO[row.fam], frame=c.frame, ntaps=16, dy=[t[0] for t in FOLD_TAPS], dx=[t[1] for t in FOLD_TAPS],
                 wtap=[t[2] for t in FOLD_TAPS], ld0=ld("x0", C0), ldo=ld("out", Cout), lde0=c.frame * Cout + p, lde1=c.frame * Cout + 2 * p)
        f["x0"], f["w"], f["bias"] = mk.inp("x0", d.x0, f["ld0"]), mk.fold_weights(d.w5, row.fam, False), mk.inp("bias", d.bias, Cout)
        f["e0"], f["e1"] = mk.inp("e0", d.e0, f["lde0"]), mk.inp("e1", d.e1, f["lde1"])
        outs["out"] = f["out"] = mk.out("out", B * 4 * FH * FW, Cout, f["ldo"], 0, None)
        return _hip.ConvDesc, "ramnet_conv_launch", f, outs
    if row.launch == "fold_dgrad":
        f = dict(in_mode=_hip.IN_PARITY4, B=B, Hin=2 * FH, Win=2 * FW, C0=C0, ld0=ld("x0", C0), stride=1, Cout=Cout, Ho=FH + 4, Wo=FW + 4, HoF=FH + 4, WoF=FW + 4,
                 osy=1, osx=1, epi=_hip.EPI_LINEAR, beta=0.0, algo=FOLD_ALGO[row.fam], ntaps=16, dy=[t[0] for t in FOLD_TAPS], dx=[t[1] for t in FOLD_TAPS],
                 wtap=[t[2] for t in FOLD_TAPS], ldo=Cout + p)
        f["x0"], f["w"] = mk.inp("x0", d.x0, f["ld0"]), mk.fold_weights(d.w5, row.fam, True)
        outs["out"] = f["out"] = mk.out("out", B * (FH + 4) * (FW + 4), Cout, f["ldo"], 0, None)
        return _hip.ConvDesc, "ramnet_conv_launch", f, outs
    if row.launch == "fold_wgrad":
        f = dict(ld0=ld("x0", C0), C0=C0, in_mode=_hip.IN_PLAIN, B=B, Hin=FH + 4, Win=FW + 4, stride=1, ldg=ld("dout", Cout), Cout=Cout, Ho=FH, Wo=FW,
                 HoG=2 * FH, WoG=2 * FW, dw=dw, dbias=dbias, algo=FOLD_ALGO[row.fam], ntaps=16, dy=[t[0] for t in FOLD_TAPS], dx=[t[1] for t in FOLD_TAPS],
                 dw_slabs=slabs)
        f["x0"], f["dout"] = mk.inp("x0", d.x0, f["ld0"]), mk.inp("dout", d.dout, f["ldg"])
        if d.gmask is not None:
            f["ldgm"] = ld("gmask", Cout)
            f["gmask"] = mk.inp("gmask", d.gmask, f["ldgm"])
        return _hip.WgradDesc, "ramnet_wgrad_launch", f, outs
    import fold_head_cases as fh
    f = dict(in_mode=_hip.IN_PLAIN, B=B, Hin=H, Win=W, C0=C0, ld0=ld("x0", C0), stride=1, Cout=Cout, Ho=H, Wo=W, algo=_hip.ALGO_HEAD, head_cin=c.cin,
             ntaps=25, dy=[t[0] for t in fh.HEAD_TAPS], dx=[t[1] for t in fh.HEAD_TAPS])
    f["x0"] = mk.inp("x0", d.x0_phys, f["ld0"])
    if row.launch == "head_fwd":
        f.update(wtap=[t[2] for t in fh.HEAD_TAPS], HoF=H, WoF=W, osy=1, osx=1, epi=c.epi, beta=0.0, ldo=ld("out", Cout), w=mk.head_weights(d, c),
                 bias=mk.inp("bias", d.bias, Cout))
        outs["out"] = f["out"] = mk.out("out", B * H * W, Cout, f["ldo"], 0, None)
        return _hip.ConvDesc, "ramnet_conv_launch", f, outs
    f.update(ldg=ld("dout", Cout), dw=dw, dbias=dbias, dw_slabs=slabs, dout=mk.inp("dout", d.dout, ld("dout", Cout)), ldgm=Cout + 2 * p,
             gmask=mk.inp("gmask", d.gmask, Cout + 2 * p))
    return _hip.WgradDesc, "ramnet_wgrad_launch", f, outs


# ---------------------------------------------------------------------------------------------------- the table
CONV_ROWS = _conv_rows()
WGRAD_ROWS = _wgrad_rows()
FH_ROWS = _fold_rows()
ROWS = CONV_ROWS + WGRAD_ROWS + FH_ROWS
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)
SIDES = [(r, refused) for r in ROWS for refused in (False, True) if not (refused and r.kind == "none")]

# weight limits (the folded families: packed weights below 0x7fffffff bytes) have rows on the refusal side only: tests/test_address_limits_cpu.py


class Dummy:
    """`mk` of the CPU test: 16-byte aligned dummy addresses, nothing allocated (no accepted descriptor is ever launched there)"""

    def __init__(self):
        self.next = 1 << 20

    def _addr(self):
        self.next += 1 << 20
        return self.next

    def inp(self, op, data, ld, seg=0):
        return self._addr()

    def out(self, op, rows, cols, ld, col0, prefill):
        return self._addr()

    def weights(self, d, fam, k):
        return self._addr()

    def fold_weights(self, w5, fam, dgrad):
        return self._addr()

    def head_weights(self, d, c):
        return self._addr()


def struct(cls, f):
    """a ctypes descriptor from a field dict (buffers by their pointer)"""
    s = cls()
    for k, v in f.items():
        v = getattr(v, "ptr", v)
        if isinstance(v, (list, tuple)):
            a = getattr(s, k)
            for j, e in enumerate(v):
                a[j] = e
        else:
            setattr(s, k, v)
    return s
