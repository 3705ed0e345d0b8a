"""The backward-weights descriptors behind tests/golden/wgrad_plan.json — shared by its generator (tests/golden/make_golden_wgrad_plan.py, run
against the PARENT commit's library) and by tests/test_wgrad_plan_cpu.py (run against the tree's) — and the Python restatement of the split
rule of csrc/conv_plan.hpp (own figure, cap, clamp chain, XCD step, tile-shape choice per family), which tests/test_hip_conv_launch.py holds
real launches to.  Nothing here launches: the pointers are dummy 16-byte aligned addresses, the queries are host-only and the violation
rows are refused before any HIP call."""
import ctypes
import itertools

from rpg_ramnet_amd import _hip

SLAB_CAP = 64                   # RAMNET_WGRAD_SLAB_CAP
ALGOS = ["DIRECT", "WINOGRAD", "WINOGRAD_2X4", "DIRECT_SPLIT", "HEAD", "WINOGRAD24", "WINOGRAD24_2X3"]
CHANNEL_ONLY = {"WINOGRAD": "ramnet_wgrad_wino_slabs", "WINOGRAD_2X4": "ramnet_wgrad_wino2x4_slabs", "DIRECT_SPLIT": "ramnet_wgrad_dsplit_slabs"}
MODES = ["PLAIN", "CAT", "CAT_MUL", "RELUMASK", "S2D"]
CH = [4, 20, 32, 36, 64, 96, 128, 160, 256]
# (C0, Cout) of the algorithms whose answer depends on the map: the axes thinned to a walk that meets every value of CH on both sides
PAIRS = [(4, 4), (4, 256), (20, 32), (32, 20), (32, 64), (36, 96), (64, 36), (64, 64), (96, 128), (128, 160), (160, 4), (256, 256)]
MAPS = [(1, 1), (5, 7), (9, 43), (16, 22), (64, 86), (256, 344)]
BATCH = [1, 8]
BLOCKS = [512, 64]              # "wgrad_blocks"
C1 = {"CAT": 12, "CAT_MUL": 32}
AXES = {"algo": ALGOS, "mode": MODES, "ch": CH, "pairs": [list(p) for p in PAIRS], "map": [list(m) for m in MAPS], "B": BATCH, "blocks": BLOCKS}

X0, X1, XM, DOUT, GMASK, DW = (4096 * (i + 1) for i in range(6))


def wgrad_desc(algo, mode, C0, Cout, H, W, B, k=3, stride=1):
    """One backward-weights launch as ops.py would describe it: a k x k filter in forward tap order over an H x W input"""
    d = _hip.WgradDesc()
    d.x0, d.dout, d.dw = X0, DOUT, DW
    d.C0, d.ld0, d.in_mode = C0, C0, getattr(_hip, "IN_" + mode)
    if mode in C1:
        d.x1, d.C1, d.ld1 = X1, C1[mode], C1[mode]
    if mode in ("CAT_MUL", "RELUMASK"):
        d.xm, d.ldm = XM, C1[mode] if mode == "CAT_MUL" else C0
    p = k // 2
    d.B, d.Hin, d.Win, d.Ho, d.Wo = B, H, W, (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    d.ntaps, d.stride = k * k, stride
    for t in range(k * k):
        d.dy[t], d.dx[t] = t // k - p, t % k - p
    d.Cout, d.ldg, d.algo = Cout, Cout, getattr(_hip, "ALGO_" + algo)
    if algo == "HEAD":
        d.head_cin = min(C0, 5)
    if algo.startswith("WINOGRAD24"):           # the folded decoders: padded low-resolution input, gradient at twice the size
        d.Hin, d.Win, d.HoG, d.WoG = H + 4, W + 4, 2 * H, 2 * W
    return d


def grid():
    """(algo, mode, C0, Cout, (H, W), B, blocks, k, stride) in grid order.  The three families whose answer is a function of the channels
    alone walk the full channel square on one map; the others the thinned pairs over every map, batch and `wgrad_blocks`, DIRECT as a 3x3
    stride-1 and a 5x5 stride-2 layer in turn."""
    for algo in ALGOS:
        if algo in CHANNEL_ONLY:
            for mode, C0, Cout in itertools.product(MODES, CH, CH):
                yield algo, mode, C0, Cout, MAPS[1], 1, 512, 3, 1
            continue
        for mode, (i, (C0, Cout)), (j, mp), B, blocks in itertools.product(MODES, enumerate(PAIRS), enumerate(MAPS), BATCH, BLOCKS):
            k, stride = (5, 2) if algo == "DIRECT" and (i + j) % 2 else (5, 1) if algo == "HEAD" else (3, 1)
            yield algo, mode, C0, Cout, mp, B, blocks, k, stride


def logical_cin(mode, C0):
    return 4 * C0 if mode == "S2D" else C0 + C1.get(mode, 0)


# ---------------------------------------------------------------------------------------------------- refusals
FAMILIES = {"2x2": ("WINOGRAD", 32, False), "2x4": ("WINOGRAD_2X4", 32, True), "dsplit": ("DIRECT_SPLIT", 4, False)}     # algo, group, segments


def _v(fam, mode="PLAIN", C0=32, B=2, H=8, W=12, **over):
    d = wgrad_desc(FAMILIES[fam][0], mode, C0, 64, H, W, B)
    for k, v in over.items():
        if k in ("dy", "dx"):
            for t, e in v.items():
                getattr(d, k)[t] = e
        else:
            setattr(d, k, v)
    return d


def violations():
    """(name, family, make): every descriptor breaks ONE structural condition of its family's launch (csrc/conv_plan.hpp: wgrad3x3_check,
    wgrad_offsets32) and nothing else, so it is refused with RAMNET_E_BADARG before any HIP call"""
    rows = []
    for fam, (_, group, segments) in FAMILIES.items():
        def add(name, **kw):
            rows.append(("%s: %s" % (fam, name), fam, lambda fam=fam, kw=kw: _v(fam, **kw)))
        add("eight taps", ntaps=8)
        add("stride 2", stride=2)
        add("output one row short", Ho=7)
        add("output one column short", Wo=11)
        add("upsampling input", mode="PLAIN", in_mode=_hip.IN_UP2X)
        add("taps 1 and 2 swapped", dy={1: -1, 2: -1}, dx={1: 1, 2: 0})
        add("a tap outside the 3x3 window", dy={8: 2})
        add("S2D group not a power of two", mode="S2D", C0=48 if group == 32 else 12)
        if group == 32:
            add("S2D group below 32 channels", mode="S2D", C0=16)
            add("concatenation inside a 32-channel block", mode="CAT", C0=48)
        if not segments:
            add("segments", nseg=1)
    # 32-bit byte offsets: one image of F(2x2), the whole tensor of F(2x4) (2^31 bytes each); dsplit has no such limit
    rows.append(("2x2: an image beyond 32-bit offsets", "2x2", lambda: _v("2x2", H=64, W=64, ld0=1 << 17)))
    rows.append(("2x4: a tensor beyond 32-bit offsets", "2x4", lambda: _v("2x4", B=8, H=64, W=64, ld0=1 << 14)))
    rows.append(("2x2: a gradient image beyond 32-bit offsets", "2x2", lambda: _v("2x2", H=64, W=64, ldg=1 << 17)))
    rows.append(("2x4: a gradient tensor beyond 32-bit offsets", "2x4", lambda: _v("2x4", B=8, H=64, W=64, ldg=1 << 14)))
    return rows


VIOLATIONS = violations()


def table(L):
    """ramnet_wgrad_slabs over the grid (grid order), the three channel-only queries over the channel square, the return code of
    ramnet_wgrad_launch(d, NULL) on every violation row"""
    old = L.ramnet_get_option(b"wgrad_blocks")
    try:
        slabs = []
        for algo, mode, C0, Cout, (H, W), B, blocks, k, stride in grid():
            assert L.ramnet_set_option(b"wgrad_blocks", blocks) == 0
            d = wgrad_desc(algo, mode, C0, Cout, H, W, B, k, stride)
            slabs.append(L.ramnet_wgrad_slabs(ctypes.byref(d)))
    finally:
        L.ramnet_set_option(b"wgrad_blocks", old)
    chan = {fn: [getattr(L, fn)(ci, co) for ci, co in itertools.product(CH, CH)] for fn in CHANNEL_ONLY.values()}
    return {"axes": AXES, "rows": len(slabs), "slabs": slabs, "channel_only": chan,
            "violations": [[name, L.ramnet_wgrad_launch(ctypes.byref(make()), None)] for name, _, make in VIOLATIONS]}


# ---------------------------------------------------------------------------------------------------- the split rule, restated
def cdiv(a, b):
    return -(-a // b)


def own_figure(fam, Cin, Cout, blocks=384, nf=1, ds_target=512):
    """workgroups the launch aims at / its channel blocks: `blocks` = "wgrad_wino_blocks" (the two Winograd families)"""
    if fam == "2x2":
        return blocks * (2 // nf) // (cdiv(Cin, 32) * cdiv(Cout, 32 * nf))
    if fam == "2x4":
        return blocks // (cdiv(Cin, 32) * cdiv(Cout, 32))
    return ds_target // (cdiv(Cin, 64) * cdiv(Cout, 64))


def cap(fam, Cin, Cout):
    """what ramnet_wgrad_*_slabs(Cin, Cout) answers: channels only, no option"""
    blocks = cdiv(Cin, 32) * cdiv(Cout, 64) if fam == "2x2" else cdiv(Cin, 32) * cdiv(Cout, 32) if fam == "2x4" else cdiv(Cin, 64) * cdiv(Cout, 64)
    return max(1, (512 if fam == "dsplit" else 384) // blocks)


def clamp(own, units, dw_slabs):
    s = min(own, units)
    if dw_slabs > 0:
        s = min(s, dw_slabs)
    return max(s, 1)


def xcd_step(splits, units, dw_slabs, nearest):
    """(splits, on the XCD map): from 8 splits up a multiple of 8 — the nearest one that units and dw_slabs allow (F(2x4)), else the one below"""
    if splits < 8:
        return splits, False
    up = (splits + 4) // 8 * 8
    if nearest and up <= units and (dw_slabs <= 0 or up <= dw_slabs):
        return up, True
    return splits // 8 * 8, True


def tile_shape(fam, H, W):
    """(name in ramnet_last_kernel(), output pixels of a batch as rows x columns)"""
    if fam == "2x2":            # 8 tiles: 2 x 16 or 8 x 4, whichever pads less (ties: wide)
        tall = cdiv(W, 4) * 4 * cdiv(H, 8) * 8 < cdiv(W, 16) * 16 * cdiv(H, 2) * 2
        return (2, 8, 4) if tall else (8, 2, 16)
    if fam == "2x4":            # 8 tiles: 4 x 16, 8 x 8 or 16 x 4, whichever pads least (ties: the widest)
        t = min((4, 2, 1), key=lambda t: (cdiv(W, 4 * t) * 4 * t * cdiv(H, 16 // t) * (16 // t), -t))
        return t, 16 // t, 4 * t
    return None, 4, 8


def plan(fam, B, H, W, Cin, Cout, dw_slabs=None, blocks=384, nf=1, nseg=1):
    """The launch of an H x W map: dw_slabs None = the slab form a caller sizes with the library's query (the cap), 0 = the atomic form"""
    txb, bh, bw = tile_shape(fam, H, W)
    batches = cdiv(W, bw) * cdiv(H, bh) * B * nseg
    own, cp = own_figure(fam, Cin, Cout, blocks, nf), cap(fam, Cin, Cout)
    slabs = cp if dw_slabs is None else dw_slabs
    splits, on_map = clamp(own, batches, slabs), False
    if fam != "2x2":
        splits, on_map = xcd_step(splits, batches, slabs, fam == "2x4")
    kernel = {"2x2": "conv_wgrad_wino_r_kernel<0,0,%s,%d>" % (txb, nf), "2x4": "conv_wgrad_wino_r6_kernel<0,0,%s>" % txb,
              "dsplit": "conv_wgrad_dsplit_kernel<0,0>"}[fam]
    return dict(txb=txb, batches=batches, own=own, cap=cp, slabs=slabs, splits=splits, xcd=on_map, kernel=kernel)


# (family, options of plan(), (B, H, W, Cin, Cout), what the plan must say): computed from the launchers before they shared the rule
G24, G22 = (2, 9, 43, 96, 64), (3, 16, 22, 64, 64)
EXPECTED = [
    ("2x4", {}, G24, dict(txb=4, batches=18, cap=64, splits=16, xcd=True)),
    ("2x4", dict(dw_slabs=12), G24, dict(splits=8, xcd=True)),
    ("2x4", dict(dw_slabs=5), G24, dict(splits=5, xcd=False)),
    ("2x4", dict(blocks=24), G24, dict(splits=4)),
    ("2x4", dict(nseg=3), G24, dict(batches=54, splits=48)),
    ("2x4", {}, (1, 8, 20, 32, 32), dict(txb=2, batches=3, splits=3)),
    ("2x4", dict(nseg=3), (1, 8, 20, 32, 32), dict(batches=9, splits=8, xcd=True)),
    ("2x4", {}, (1, 16, 8, 32, 32), dict(txb=2, splits=2)),
    ("2x4", {}, (2, 16, 16, 32, 64), dict(batches=8, splits=8, xcd=True)),
    ("2x2", dict(nf=1), (4, 32, 48, 64, 96), dict(txb=8, own=128, cap=96, splits=96)),
    ("2x2", dict(nf=2), (4, 32, 48, 64, 96), dict(own=96)),
    ("2x2", {}, G22, dict(txb=2, batches=36, splits=36)),
    ("2x2", dict(blocks=8), G22, dict(splits=4)),
    ("2x2", dict(nf=1), (1, 8, 20, 32, 32), dict(txb=2, batches=5, own=768, cap=384, splits=5)),
]
# dsplit, by its own rule (64 x 64-channel blocks, 4 x 8 pixel batches, 512 workgroups, the multiple of 8 BELOW): hand-computed
EXPECTED_DSPLIT = [
    ("dsplit", {}, G24, dict(batches=36, own=256, cap=256, splits=32, xcd=True)),
    ("dsplit", dict(dw_slabs=12), G24, dict(splits=8, xcd=True)),
    ("dsplit", {}, (1, 8, 20, 32, 32), dict(batches=6, splits=6, xcd=False)),
    ("dsplit", {}, (4, 32, 48, 64, 96), dict(batches=192, own=256, splits=192, xcd=True)),
]
