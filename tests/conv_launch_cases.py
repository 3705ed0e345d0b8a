"""The case table of the direct convolution-launch tests: shapes, channels, modes and data kinds, shared by
tests/test_conv_restatement_cpu.py (conditions every case must meet to be judged, without a GPU) and tests/test_hip_conv_launch.py.
`build(case)` makes the float64 descriptor of tests/conv_restatement.py from a row, seeded by the row's name.

Families: "direct" (RAMNET_ALGO_DIRECT), "2x2" (WINOGRAD), "2x4" (WINOGRAD_2X4), "2x4split" (WINOGRAD_2X4_SPLIT).
Data kinds: "int" (the exact rule: inputs in {-2..2} with zeros, weights 48 x {-1, 0, 1}: a multiple of 4 and of 48, so G g G^T of both
Winograd families is integral) and "normal" (the derived / measured rules)."""
import types
import zlib

import torch

import conv_restatement as cr

F64 = torch.float64
ALL3 = ("direct", "2x2", "2x4")
ALL4 = ALL3 + ("2x4split",)
CELL_EPIS = (cr.EPI_SIGMOID, cr.EPI_SIGMOID_HR, cr.EPI_GRU_BLEND, cr.EPI_LSTM)


def _case(name, fams, B, H, W, C0, Cout, **kw):
    c = dict(name=name, fams=fams, B=B, H=H, W=W, C0=C0, Cout=Cout, C1=0, mode=cr.IN_PLAIN, epi=cr.EPI_RELU, kind="int", k=3, stride=1,
             bias=True, beta=0.0, active=None, out_s2d=0, s2d_5x5=0, transposed=False, pitch=0, e1=True, o2=True, window=False, density=0.5, xscale=1, wscale=1)
    assert not set(kw) - set(c), kw
    c.update(kw)
    return types.SimpleNamespace(**c)


def _table():
    t = []
    # ---- the maps of the three F(2x4,3x3) workgroup tiles (16x16, 32x8, 8x32), exact and ragged both ways, B = 1 and 3 (tiles x B no
    # multiple of 8: surplus workgroups of the rounded-up grid); (33,7) and (40,3) take the `tall` tile of F(2x2,3x3), the others the wide one
    maps = [(1, 1), (2, 4), (16, 16), (17, 17), (33, 7), (7, 33), (9, 43)]
    for i, (h, w) in enumerate(maps):
        for B in (1, 3):
            j = i + B
            t.append(_case("map%dx%d_B%d" % (h, w, B), ALL3, B, h, w, (4, 8, 12, 40)[j % 4], (64, 128)[j % 2], pitch=4 * (j % 2),
                           epi=(cr.EPI_RELU, cr.EPI_LINEAR)[i % 2]))
            t.append(_case("map%dx%d_B%d_s" % (h, w, B), ("2x4split",), B, h, w, (4, 16, 20)[j % 3], (128, 64)[j % 2], pitch=4 * ((j + 1) % 2)))
    t.append(_case("tall40x3", ("2x2", "direct"), 2, 40, 3, 8, 64))
    # ---- channel counts off the 8 / 64 blocking of F(2x2,3x3)
    for cin, cout in ((36, 20), (68, 36), (40, 64)):
        t.append(_case("chan%d_%d" % (cin, cout), ("2x2", "direct"), 2, 9, 11, cin, cout, pitch=4))
    # ---- input modes
    t.append(_case("cat8_4", ALL3, 2, 9, 11, 8, 64, C1=4, mode=cr.IN_CAT, pitch=4))
    t.append(_case("cat16_12", ALL4, 2, 17, 17, 16, 128, C1=12, mode=cr.IN_CAT))
    t.append(_case("catmul8_12", ALL3, 2, 9, 11, 8, 64, C1=12, mode=cr.IN_CAT_MUL))
    t.append(_case("catmul16_4", ALL4, 3, 7, 33, 16, 64, C1=4, mode=cr.IN_CAT_MUL, pitch=4))
    t.append(_case("relumask12", ALL3, 2, 9, 11, 12, 64, mode=cr.IN_RELUMASK, pitch=4))
    t.append(_case("relumask16", ALL4, 1, 17, 17, 16, 64, mode=cr.IN_RELUMASK))
    for five in (0, 1):
        t.append(_case("s2d8_5x5_%d" % five, ("2x2", "2x4"), 2, 9, 11, 8, 64, mode=cr.IN_S2D, s2d_5x5=five, pitch=4 * five))
        t.append(_case("s2d16_5x5_%d" % five, ("2x2", "2x4", "2x4split"), 3, 7, 9, 16, 64, mode=cr.IN_S2D, s2d_5x5=five))
        # 256 workgroups of 64 channels: the launch keeps the position skip of s2d_5x5 = 1 (smaller ones fall back to the dense evaluation)
        t.append(_case("s2d8_big_5x5_%d" % five, ("2x2",), 2, 64, 128, 8, 128, mode=cr.IN_S2D, s2d_5x5=five, density=0.25))
    # ---- epilogues, exact
    t.append(_case("beta1", ALL4, 2, 9, 11, 16, 64, epi=cr.EPI_LINEAR, beta=1.0, pitch=4))
    t.append(_case("beta1_relu", ALL3, 1, 17, 17, 8, 64, epi=cr.EPI_RELU, beta=1.0))
    t.append(_case("res_relu", ALL4, 2, 9, 11, 16, 64, epi=cr.EPI_RES_RELU, pitch=4, window=True))
    t.append(_case("gru_bwd", ALL4, 2, 9, 11, 16, 128, epi=cr.EPI_GRU_BWD, bias=False, transposed=True, window=True))
    t.append(_case("gru_bwd_noh", ALL4, 1, 7, 9, 16, 128, epi=cr.EPI_GRU_BWD, bias=False, transposed=True, e1=False, pitch=4))
    t.append(_case("out_s2d8", ("2x2",), 2, 5, 7, 8, 32, epi=cr.EPI_LINEAR, bias=False, out_s2d=8, transposed=True))
    t.append(_case("out_s2d16", ("2x2", "2x4", "2x4split"), 2, 5, 7, 16, 64, epi=cr.EPI_LINEAR, bias=False, out_s2d=16, transposed=True, pitch=4))
    t.append(_case("out_s2d32_5x5", ("2x2",), 1, 5, 7, 8, 128, epi=cr.EPI_LINEAR, bias=False, out_s2d=32, s2d_5x5=1, transposed=True))
    # ---- the cell epilogues, normal data (measured rule); `window`: e0 = u out of [u | r], o1 = h.r into the second half of [x | h.r]
    t.append(_case("sigmoid", ALL4, 2, 9, 11, 16, 64, epi=cr.EPI_SIGMOID, kind="normal", C1=16, mode=cr.IN_CAT, pitch=4))
    t.append(_case("sigmoid_hr", ALL4, 2, 9, 11, 16, 128, epi=cr.EPI_SIGMOID_HR, kind="normal", C1=16, mode=cr.IN_CAT, window=True))
    t.append(_case("sigmoid_hr_masked", ALL4, 3, 5, 7, 16, 128, epi=cr.EPI_SIGMOID_HR, kind="normal", C1=16, mode=cr.IN_CAT, active=(1, 0, 1), pitch=4))
    t.append(_case("gru_blend", ALL4, 2, 9, 11, 16, 64, epi=cr.EPI_GRU_BLEND, kind="normal", C1=16, mode=cr.IN_CAT_MUL, window=True))
    t.append(_case("gru_blend_masked", ALL4, 3, 5, 7, 16, 64, epi=cr.EPI_GRU_BLEND, kind="normal", C1=16, mode=cr.IN_CAT_MUL, active=(0, 1, 0), e1=True))
    t.append(_case("gru_blend_noh", ALL3, 1, 5, 7, 8, 64, epi=cr.EPI_GRU_BLEND, kind="normal", C1=8, mode=cr.IN_CAT, e1=False, pitch=4))
    t.append(_case("lstm16", ALL3, 2, 9, 11, 8, 16, epi=cr.EPI_LSTM, kind="normal", C1=16, mode=cr.IN_CAT))
    t.append(_case("lstm48_no_o2", ALL3, 1, 7, 9, 8, 48, epi=cr.EPI_LSTM, kind="normal", C1=48, mode=cr.IN_CAT, o2=False, pitch=4))
    t.append(_case("lstm16_masked", ALL3, 3, 5, 7, 8, 16, epi=cr.EPI_LSTM, kind="normal", C1=16, mode=cr.IN_CAT, active=(1, 0, 0)))
    t.append(_case("lstm32_direct", ("direct",), 2, 9, 11, 8, 32, epi=cr.EPI_LSTM, kind="normal", C1=32, mode=cr.IN_CAT, pitch=4))
    # ---- derived rule on normal data, every family, ragged maps
    t.append(_case("normal17", ALL4, 2, 17, 17, 16, 64, kind="normal"))
    t.append(_case("normal9x43", ALL4, 1, 9, 43, 20, 128, kind="normal", epi=cr.EPI_LINEAR, pitch=4))
    t.append(_case("normal_cat", ALL4, 3, 7, 33, 16, 64, kind="normal", C1=4, mode=cr.IN_CAT_MUL))
    # ---- integers beyond the first bf16 term of the split operands (weights 17 x 48 x {-1, 0, 1}: transformed values of up to 10 bits;
    # inputs 9 / 16 x {-2..2}: up to 9 where several meet): still exact with the mixed partial products in place
    t.append(_case("split_bits", ("2x4", "2x4split"), 1, 9, 11, 16, 64, density=0.25, xscale=9 / 16, wscale=17, epi=cr.EPI_LINEAR))
    # ---- XCD groups of F(2x4,3x3): 256 -> 256 channels are 6 MB of Winograd-domain weights, two groups
    t.append(_case("xcd256_256", ("2x4",), 1, 8, 12, 256, 256, epi=cr.EPI_LINEAR, bias=False, density=0.25))
    # ---- DIRECT: 3x3 and 5x5 at stride 1 and 2, output channel counts, tile configurations of launch_classes (Cin = 4)
    for k in (3, 5):
        for s in (1, 2):
            t.append(_case("direct_k%d_s%d" % (k, s), ("direct",), 2, 11, 13, 8, (20, 96)[s - 1], k=k, stride=s, pitch=4 * (s - 1)))
    t.append(_case("direct_c32", ("direct",), 1, 9, 11, 4, 32))                                             # <128,32,4,1>
    t.append(_case("direct_c64_small", ("direct",), 1, 9, 11, 4, 64))                                       # <64,64,2,2>
    t.append(_case("direct_c128_small", ("direct",), 1, 9, 11, 4, 128, epi=cr.EPI_LINEAR))                  # <64,64,2,2> from 128 columns
    t.append(_case("direct_128x64", ("direct",), 1, 256, 384, 4, 64, epi=cr.EPI_LINEAR, bias=False))        # 768 tiles of 128 pixels
    t.append(_case("direct_128x128", ("direct",), 1, 256, 384, 4, 128, epi=cr.EPI_LINEAR, bias=False))
    t.append(_case("direct_64x128", ("direct",), 1, 128, 384, 4, 128, epi=cr.EPI_LINEAR, bias=False))       # 768 tiles of 64 pixels
    t.append(_case("direct_256x32", ("direct",), 1, 512, 512, 4, 32, epi=cr.EPI_LINEAR, bias=False))        # 1024 tiles of 256 pixels
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the kernel ramnet_last_kernel must name for the DIRECT tile configurations
DIRECT_KERNEL = {"direct_c32": "conv_igemm_kernel<128,32,4,1>", "direct_c64_small": "conv_igemm_kernel<64,64,2,2>",
                 "direct_c128_small": "conv_igemm_kernel<64,64,2,2>", "direct_128x64": "conv_igemm_kernel<128,64,2,2>",
                 "direct_128x128": "conv_igemm_kernel<128,128,2,2>", "direct_64x128": "conv_igemm_kernel<64,128,2,2>",
                 "direct_256x32": "conv_igemm_kernel<256,32,4,1>", "lstm32_direct": "conv_igemm_kernel<128,128,4,1>"}
# ... and for F(2x2,3x3) <tile columns, sparse mode, input mode, 32-channel blocks per workgroup>: the rows that must keep the position skip,
# their dense siblings, the tall tile, the 64-channel workgroups of the out_s2d skip
WINO_KERNEL = {"s2d8_big_5x5_1": "conv_wino_r_kernel<8,1,6,1>", "s2d8_big_5x5_0": "conv_wino_r_kernel<8,0,6,1>", "tall40x3": "conv_wino_r_kernel<2,0,0,1>",
               "out_s2d32_5x5": "conv_wino_r_kernel<8,2,0,2>", "map33x7_B1": "conv_wino_r_kernel<2,0,0,1>"}


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _ri(g, shape, m):
    return torch.randint(-m, m + 1, shape, generator=g).to(F64)


def _rn(g, shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).float().to(F64)          # fp32-representable


def s2d_weights(w5):
    """the 3x3 filter over the space-to-depth view that a 5x5 stride-2 (padding 2) filter stands for: tap u = 2*dy + a + 2"""
    N, C, _, _ = w5.shape
    w3 = torch.zeros(N, 4 * C, 3, 3, dtype=w5.dtype)
    for a in range(2):
        for c in range(2):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    u, v = 2 * dy + a + 2, 2 * dx + c + 2
                    if 0 <= u < 5 and 0 <= v < 5:
                        w3[:, (a * 2 + c) * C:(a * 2 + c + 1) * C, dy + 1, dx + 1] = w5[:, :, u, v]
    return w3


def build(c):
    """the float64 descriptor of a row (tests/conv_restatement.py), with w_oihw = the OIHW weights the library's packers take"""
    g = _gen(c.name)
    integer = c.kind == "int"
    k, p = c.k, c.k // 2
    s2d = c.mode == cr.IN_S2D
    Cin = 4 * c.C0 if s2d else c.C0 + (c.C1 if c.mode in (cr.IN_CAT, cr.IN_CAT_MUL) else 0)
    N = 4 * c.Cout if c.epi == cr.EPI_LSTM else c.Cout
    Hx, Wx = (2 * c.H, 2 * c.W) if s2d else (c.H, c.W)

    def data(shape, m=2, scale=1.0):
        if integer:
            return _ri(g, shape, m) * (torch.rand(shape, generator=g) < c.density).to(F64)
        return _rn(g, shape, scale)

    d = types.SimpleNamespace(in_mode=c.mode, Hin=c.H, Win=c.W, B=c.B, C0=c.C0, C1=c.C1, Cin=Cin, Cout=c.Cout, N=N, stride=c.stride, epi=c.epi,
                              beta=c.beta, out_s2d=c.out_s2d, s2d_5x5=c.s2d_5x5, x1=None, xm=None, bias=None, e0=None, e1=None, out_old=None,
                              active=None, transposed=c.transposed)
    d.x0 = data((c.B, Hx, Wx, c.C0)) * c.xscale
    if c.mode in (cr.IN_CAT, cr.IN_CAT_MUL):
        d.x1 = data((c.B, c.H, c.W, c.C1))
    if c.mode == cr.IN_CAT_MUL:
        d.xm = data((c.B, c.H, c.W, c.C1)) if integer else torch.rand(c.B, c.H, c.W, c.C1, generator=g).float().to(F64)
    if c.mode == cr.IN_RELUMASK:
        d.xm = _ri(g, (c.B, c.H, c.W, c.C0), 1) if integer else _rn(g, (c.B, c.H, c.W, c.C0))
    # weights: OIHW [N][Cin] forward, [Cin = reduced O][N = produced I] for a backward-data (transposed) launch
    wshape = (Cin, N, k, k) if c.transposed else (N, Cin, k, k)
    if integer:
        w = 48.0 * c.wscale * _ri(g, wshape, 1) * (torch.rand(wshape, generator=g) < c.density).to(F64)
    else:
        w = _rn(g, wshape, 1.0 / (k * k * Cin) ** 0.5)
    if c.s2d_5x5:                                   # the zero slices of the 3x3 view of a 5x5 stride-2 filter
        if s2d:
            keep = s2d_weights(torch.ones(1, c.C0, 5, 5, dtype=F64))            # [1][4*C0][3][3] of 0 / 1
            w = w * keep
        else:                                       # backward-data of such a layer: the produced channels are the view
            keep = s2d_weights(torch.ones(1, c.out_s2d, 5, 5, dtype=F64))       # [1][N][3][3], forward orientation
            w = w * keep
    d.w_oihw = w
    d.W = (w.permute(2, 3, 0, 1) if c.transposed else w.permute(2, 3, 1, 0)).reshape(k * k, Cin, N).contiguous()
    # taps: the dense k x k window; a backward-data launch reads the flipped slice (what the Winograd packs bake in)
    d.taps = [(a - p, b - p, ((k - 1 - a) * k + (k - 1 - b)) if c.transposed else a * k + b) for a in range(k) for b in range(k)]
    d.Ho, d.Wo = (c.H + 2 * p - k) // c.stride + 1, (c.W + 2 * p - k) // c.stride + 1
    d.HoF, d.WoF = (2 * d.Ho, 2 * d.Wo) if c.out_s2d else (d.Ho, d.Wo)
    d.os = (1, 1, 0, 0)
    if c.bias:
        d.bias = _ri(g, (N,), 8) if integer else _rn(g, (N,), 0.1)
    full = (c.B, d.HoF, d.WoF)
    if c.beta != 0.0:
        d.out_old = _ri(g, full + (c.Cout,), 8) if integer else _rn(g, full + (c.Cout,))
    if c.epi == cr.EPI_RES_RELU:
        d.e0 = data(full + (c.Cout,), 8)
    if c.epi == cr.EPI_GRU_BWD:                     # e0 = [u | r] (r read at channel n >= C), e1 = h, out_old = dh'(1 - u) in the second half
        C = c.Cout // 2
        d.e0 = torch.randint(0, 3, full + (c.Cout,), generator=g).to(F64) if integer else torch.rand(*full, c.Cout, generator=g).float().to(F64)
        d.e1 = data(full + (C,)) if c.e1 else None
        d.out_old = _ri(g, full + (c.Cout,), 8) if integer else _rn(g, full + (c.Cout,))
    if c.epi == cr.EPI_SIGMOID_HR:
        d.e1 = _rn(g, full + (c.Cout // 2,))
    if c.epi == cr.EPI_GRU_BLEND:
        d.e0 = torch.rand(*full, c.Cout, generator=g).float().to(F64)
        d.e1 = _rn(g, full + (c.Cout,)) if c.e1 else None
    if c.epi == cr.EPI_LSTM:
        d.e1 = _rn(g, full + (c.Cout,)) if c.e1 else None
        if c.active is not None:
            d.e0 = _rn(g, full + (c.Cout,))
    if c.active is not None:
        d.active = torch.tensor(c.active, dtype=torch.int32)
    return d


FAMILY_OF_ALGO = {"direct": 0, "2x2": 1, "2x4": 4, "2x4split": 5}


# ---------------------------------------------------------------------------------------------------- backward-weights rows (3x3 families)
# (H, W, B, input mode, C0, C1, Cout, gmask, dbias, data kind); S2D: x0 is [B][2H][2W][C0], Cin = 4 * C0
WGRAD_ROWS = [(1, 1, 1, cr.IN_PLAIN, 8, 0, 20, False, True, "int"), (5, 7, 3, cr.IN_CAT, 32, 4, 64, True, True, "int"),
              (9, 43, 1, cr.IN_CAT_MUL, 32, 12, 36, False, False, "int"), (16, 22, 3, cr.IN_RELUMASK, 36, 0, 128, True, True, "int"),
              (5, 7, 2, cr.IN_S2D, 32, 0, 64, False, True, "int"), (9, 11, 2, cr.IN_CAT, 32, 8, 64, True, True, "normal"),
              (16, 22, 1, cr.IN_PLAIN, 20, 0, 36, False, True, "normal")]


def build_wgrad(i, seed=0):
    """the float64 backward-weights descriptor of WGRAD_ROWS[i] (tests/conv_restatement.py: wgrad_statement); seed: another segment"""
    H, W, B, mode, C0, C1, Cout, gm, _, kind = WGRAD_ROWS[i]
    g = _gen("wgrad%d_%d" % (i, seed))

    def data(shape, m=2):
        if kind == "int":
            return _ri(g, shape, m) * (torch.rand(shape, generator=g) < 0.5).to(F64)
        return _rn(g, shape)
    s2 = 2 if mode == cr.IN_S2D else 1
    d = types.SimpleNamespace(in_mode=mode, x0=data((B, s2 * H, s2 * W, C0)), x1=data((B, H, W, C1)) if C1 else None, xm=None, stride=1, Ho=H, Wo=W,
                              taps=[(a - 1, b - 1) for a in range(3) for b in range(3)], dout=data((B, H, W, Cout), 4),
                              gmask=data((B, H, W, Cout), 1) if gm else None, Cin=4 * C0 if mode == cr.IN_S2D else C0 + C1, Cout=Cout, B=B)
    if mode == cr.IN_CAT_MUL:
        d.xm = data((B, H, W, C1))
    if mode == cr.IN_RELUMASK:
        d.xm = data((B, H, W, C0), 1)
    return d


# ---------------------------------------------------------------------------------------------------- the third bf16 term, coherently
# One F(2x4,3x3) tile (Ho x Wo = 2 x 4 read from a 4 x 6 input through the tap window dy, dx in 0..2, so that the whole tile is free) whose
# transformed input is V = v e_0 e_0^T in every one of 16 channels, v = 1 + 2^-9 + 57 x 2^-23: its bf16 terms are 1, 2^-9 and 57 x 2^-23, the
# third as large as a third term gets (0.89 x 2^-17 v) and of one sign in all channels.  Only the filter tap (0, 0) meets position (0, 0)
# (U = g[0][0] / 4), the weights are 4 there: output pixel (0, 0) = sum_c V_c = 16 v, and a split kernel that loses the (third term of V) x
# (first term of U) product is off by 16 x 57 x 2^-23 = 109 x 2^-24 x 16 v, against a derived bound of (16 + 12 + 2 + 3) x 2^-24 x 16 v.
COHERENT_V = 1.0 + 2.0 ** -9 + 57 * 2.0 ** -23


def build_coherent():
    C0, Cout = 16, 64
    BT2i, BT4i = torch.linalg.inv(cr.BT2), torch.linalg.inv(cr.BT4)
    V = torch.zeros(4, 6, dtype=F64)
    V[0, 0] = COHERENT_V
    tile = (BT2i @ V @ BT4i.T).float().to(F64)                     # d with B2^T d B4 = V (up to the fp32 rounding of d, which the statement sees)
    x0 = tile[None, :, :, None].repeat(1, 1, 1, C0).contiguous()
    w = torch.zeros(Cout, C0, 3, 3, dtype=F64)
    w[:, :, 0, 0] = 4.0
    d = types.SimpleNamespace(in_mode=cr.IN_PLAIN, Hin=4, Win=6, B=1, C0=C0, C1=0, Cin=C0, Cout=Cout, N=Cout, stride=1, epi=cr.EPI_LINEAR, beta=0.0,
                              out_s2d=0, s2d_5x5=0, x0=x0, x1=None, xm=None, bias=None, e0=None, e1=None, out_old=None, active=None, transposed=False,
                              w_oihw=w, W=w.permute(2, 3, 1, 0).reshape(9, C0, Cout).contiguous(),
                              taps=[(a, b, a * 3 + b) for a in range(3) for b in range(3)], Ho=2, Wo=4, HoF=2, WoF=4, os=(1, 1, 0, 0))
    c = _case("coherent_third_term", ("2x4", "2x4split"), 1, 2, 4, C0, Cout, kind="normal", epi=cr.EPI_LINEAR, bias=False)
    return c, d
