"""The descriptors behind tests/golden/wino_plan.json: shared by its generator (tests/golden/make_golden_wino_plan.py, run against the
PARENT commit's library) and by tests/test_wino_plan_cpu.py (run against the tree's).  Nothing here launches: the pointers are dummy
16-byte aligned addresses, the three entry points asked are host-only."""
import ctypes
import itertools

from rpg_ramnet_amd import _hip

MODES = ["PLAIN", "CAT", "CAT_MUL", "RELUMASK", "S2D"]
EPIS = ["LINEAR", "RES_RELU", "SIGMOID", "GRU_BWD", "LSTM"]
CHANNELS = [(32, 0, 64), (40, 0, 64), (36, 0, 64), (64, 64, 64), (128, 128, 256), (256, 256, 512), (512, 0, 512)]      # (C0, C1, Cout)
MAPS = [(1, 2, 2), (1, 7, 13), (2, 9, 43), (1, 32, 8), (2, 8, 32), (1, 32, 43), (1, 64, 86), (8, 32, 43), (8, 128, 172)]  # (B, Ho, Wo)
OUT_S2D = [0, 1]          # 0, or Cout / 4
FORCE = [0, 1]
AXES = {"mode": MODES, "epi": EPIS, "channels": [list(c) for c in CHANNELS], "map": [list(m) for m in MAPS], "out_s2d": OUT_S2D, "force": FORCE}

X0, X1, XM, W, BIAS, OUT, O1, O2, E0, E1 = (4096 * (i + 1) for i in range(10))


def conv_desc(mode, epi, channels, mp, s2d):
    """One 3x3 stride-1 launch of the grid, as ops.py would describe it (algo = RAMNET_ALGO_WINOGRAD: what ramnet_conv_wino_variant expects)."""
    C0, C1, Cout = channels
    B, Ho, Wo = mp
    d = _hip.ConvDesc()
    d.x0, d.w, d.out, d.bias = X0, W, OUT, BIAS
    d.C0, d.ld0, d.in_mode = C0, C0, getattr(_hip, "IN_" + mode)
    if mode in ("CAT", "CAT_MUL"):
        d.x1, d.C1, d.ld1 = X1, C1, C1
    if mode in ("CAT_MUL", "RELUMASK"):
        d.xm, d.ldm = XM, C1 if mode == "CAT_MUL" else C0
    d.B, d.Hin, d.Win, d.Ho, d.Wo, d.HoF, d.WoF = B, Ho, Wo, Ho, Wo, Ho, Wo
    d.ntaps, d.stride, d.osy, d.osx = 9, 1, 1, 1
    for t in range(9):
        d.dy[t], d.dx[t], d.wtap[t] = t // 3 - 1, t % 3 - 1, t
    d.Cout, d.ldo = Cout, Cout
    d.epi, d.algo = getattr(_hip, "EPI_" + epi), _hip.ALGO_WINOGRAD
    if epi == "RES_RELU":
        d.e0, d.lde0 = E0, Cout
    if epi == "GRU_BWD":          # Cout = 2C: [dx | d(h.r)]; e0 = r, e1 = h, o1 <- dr; no bias
        d.e0, d.e1, d.o1, d.lde0, d.lde1, d.ldo1, d.bias = E0, E1, O1, Cout // 2, Cout // 2, Cout // 2, None
    if epi == "LSTM":             # Cout = hidden size, 4 Cout gate columns
        d.e1, d.o1, d.o2, d.lde1, d.ldo1, d.ldo2 = E1, O1, O2, Cout, Cout, 4 * Cout
    if s2d:                       # the output is the space-to-depth view of a [2 Ho][2 Wo][Cout / 4] tensor
        d.out_s2d, d.ldo, d.HoF, d.WoF, d.bias = Cout // 4, Cout // 4, 2 * Ho, 2 * Wo, None
    return d


def in_grid(mode, channels):
    """What the launchers can take at all: a concatenation needs its second tensor and a boundary on the 8-channel chunk, the
    space-to-depth view a power-of-two C0."""
    C0, C1, _ = channels
    if mode in ("CAT", "CAT_MUL"):
        return C1 > 0 and C0 % 8 == 0
    if mode == "S2D":
        return C0 & (C0 - 1) == 0
    return True


def grid():
    """(mode, epi, channels, map, out_s2d, force) in grid order."""
    for mode, epi, ch, mp, s2d, force in itertools.product(MODES, EPIS, CHANNELS, MAPS, OUT_S2D, FORCE):
        if in_grid(mode, ch):
            yield mode, epi, ch, mp, s2d, force


def lstm_desc(C=64, B=2, Hh=32, W=48, **over):
    """tests/test_lstm_wino2x4_cpu.lstm_desc"""
    d = conv_desc("CAT", "LSTM", (C, C, C), (B, Hh, W), 0)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def plain_desc(**over):
    d = conv_desc("PLAIN", "RES_RELU", (64, 0, 64), (2, 32, 48), 0)
    for k, v in over.items():
        setattr(d, k, v)
    return d


# every row breaks ONE structural condition of the F(2x4,3x3) launch
VIOLATIONS = [
    ("lstm: hidden size 24", lambda: lstm_desc(Cout=24, C0=24, C1=24, ld0=24, ld1=24, ldo=24, ldo1=24, ldo2=96, lde1=24)),
    ("lstm: C0 = 36", lambda: lstm_desc(C0=36, ld0=36)),
    ("lstm: misaligned o1", lambda: lstm_desc(o1=O1 + 4)),
    ("lstm: misaligned o2", lambda: lstm_desc(o2=O2 + 8)),
    ("lstm: misaligned bias", lambda: lstm_desc(bias=BIAS + 4)),
    ("lstm: in_mode PLAIN", lambda: lstm_desc(in_mode=_hip.IN_PLAIN)),
    ("lstm: out_s2d", lambda: lstm_desc(out_s2d=16)),
    ("lstm: no o1", lambda: lstm_desc(o1=None)),
    ("lstm: no bias", lambda: lstm_desc(bias=None)),
    ("lstm: output stride", lambda: lstm_desc(osy=2, osx=2)),
    ("lstm: frame", lambda: lstm_desc(frame=2)),
    ("misaligned out", lambda: plain_desc(out=OUT + 4)),
    ("misaligned e0", lambda: plain_desc(e0=E0 + 8)),
    ("misaligned bias", lambda: plain_desc(bias=BIAS + 4)),
]


def ask(L, d, force):
    """[ramnet_conv_wino_variant, ramnet_conv_wino_split_ok, ramnet_conv_splitk_floats] of a descriptor"""
    return [L.ramnet_conv_wino_variant(ctypes.byref(d), force), L.ramnet_conv_wino_split_ok(ctypes.byref(d), force),
            L.ramnet_conv_splitk_floats(ctypes.byref(d))]


def table(L):
    """The three answers over the grid (one integer array each, grid order) and over the violation rows (force = 0, 1)."""
    rows = [ask(L, conv_desc(mode, epi, ch, mp, s2d), force) for mode, epi, ch, mp, s2d, force in grid()]
    return {"axes": AXES, "rows": len(rows),
            "variant": [r[0] for r in rows], "split_ok": [r[1] for r in rows], "splitk_floats": [r[2] for r in rows],
            "violations": [[name, ask(L, make(), 0), ask(L, make(), 1)] for name, make in VIOLATIONS]}
