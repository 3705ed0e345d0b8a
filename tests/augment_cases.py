"""The rows of tests/test_hip_augment_launch.py and tests/test_augment_restatement_cpu.py: sources, parameter sets, windows and layouts of
`ramnet_augment_batch`, and what the statement of tests/augment_restatement.py gives for each.

A row: G sources [C][H][W] -> windows th x tw, `params` = [(theta6, top, left, exact, flips)], `pidx` (None: tensor g uses set g), `kinds` = what
each source holds, `stats` = the fused normalisation, `nhwc` / `Cpad`, `skew` = floats by which every destination is moved off 16 bytes."""
import functools
from math import cos, pi, sin

import torch

import augment_restatement as ar

F64 = torch.float64
NAN = float("nan")
SHAPES = {"s1": (9, 13, 9, 13), "s2": (20, 30, 17, 23), "s3": (33, 40, 32, 32), "s4": (40, 56, 32, 32), "big": (26, 30, 24, 25)}
BIG_G = 4100          # the launcher caps the grid at ceil(8192 / G) = 2 workgroups per source: 512 threads for 600 pixels


def theta(deg=0.0, hflip=False, vflip=False, tx=0.0, ty=0.0, scale=1.0):
    """the 2 x 3 matrix as the host transform builds it (fp32), flips as sign changes of its columns"""
    a = deg * pi / 180.0
    M = torch.tensor([[cos(a) * scale, -sin(a) * scale, tx], [sin(a) * scale, cos(a) * scale, ty]], dtype=torch.float32)
    if hflip:
        M[:, 0] *= -1
    if vflip:
        M[:, 1] *= -1
    return M.reshape(-1).to(F64)


def flip_sets(H, W, th, tw, windows):
    """the four flips in exact mode, one window each"""
    return [(theta(0.0, bool(f & 1), bool(f & 2)), top, left, 1, f) for f, (top, left) in enumerate(windows)]


def corner_windows(H, W, th, tw):
    return [(0, 0), (H - th, W - tw), (0, W - tw), (H - th, 0)]


def general_sets(H, W, th, tw, finite):
    """finite: identity, 180 and 90 degrees, the translations onto the image's edge and the all-outside scale are included (on NaN data
    their sample points sit on integers or half-integers, where the tap sets of fp32 and float64 may differ)"""
    mid = ((H - th) // 2, (W - tw) // 2)
    corners = corner_windows(H, W, th, tw)
    sets = [(theta(30.0), *mid), (theta(-7.3), *corners[1]), (theta(30.0, hflip=True), *corners[0]), (theta(-7.3, vflip=True), *corners[2]),
            (theta(12.5, True, True), *corners[3]), (theta(3.0, tx=0.013, ty=-0.021), *mid)]
    if finite:
        e = 1.0 / 64
        sets += [(theta(0.0), *mid), (theta(180.0), *corners[1]), (theta(90.0), *corners[0]), (theta(90.0, tx=0.6, ty=-0.4), *mid),
                 (theta(-90.0, hflip=True), *corners[2]),
                 (theta(0.0, tx=-1.0 / W, ty=-1.0 / H), *corners[0]), (theta(0.0, tx=1.0 / W, ty=1.0 / H), *corners[1]),          # ix = -0.5 at X = 0, W - 0.5 at X = W - 1
                 (theta(0.0, tx=-(1 + e) / W, ty=-(1 - e) / H), *corners[0]), (theta(0.0, tx=(1 - e) / W, ty=(1 + e) / H), *corners[1]),
                 (theta(0.0, tx=-(1 - e) / W, ty=(1 + e) / H), *corners[2]), (theta(0.0, tx=(1 + e) / W, ty=-(1 + e) / H), *corners[3]),
                 (theta(0.0, tx=8.0, ty=8.0, scale=4.0), *mid)]                                                                    # every tap outside
    return [(t, top, left, 0, 0) for t, top, left in sets]


OUTSIDE = -1          # index of the all-outside set among general_sets(finite=True)


def _source(kind, C, H, W, gen):
    if kind == "zeros":
        return torch.zeros(C, H, W, dtype=F64)
    if kind in ("c03", "c02"):                     # a single distinct non-zero value: 0.3f squared rounds down, 0.2f squared up
        s = torch.zeros(C * H * W, dtype=F64)
        s[::2] = float(torch.tensor(0.3 if kind == "c03" else 0.2, dtype=torch.float32))
        return s.view(C, H, W)
    s = (torch.randn(C, H, W, generator=gen) + 0.5).to(F64)
    if kind in ("sparse", "nan"):
        s[torch.rand(C, H, W, generator=gen) < 0.3] = 0.0
        s.view(-1)[1] = -0.0
    if kind == "nan":
        s[torch.rand(C, H, W, generator=gen) < 0.03] = NAN
        s[:, H // 2:H // 2 + 2, W // 3:W // 3 + 3] = NAN
    return s


def _row(shape, C, sets, kinds=None, pidx=None, stats=False, nhwc=False, Cpad=0, skew=0, G=None):
    H, W, th, tw = SHAPES[shape]
    params = sets(H, W, th, tw) if callable(sets) else sets
    G = G or (len(params) if pidx is None else len(pidx))
    kinds = kinds or ["normal"]
    return dict(C=C, H=H, W=W, th=th, tw=tw, params=params, G=G, pidx=pidx, stats=stats, nhwc=nhwc, Cpad=Cpad, skew=skew,
                kinds=[kinds[g % len(kinds)] for g in range(G)])


def _flips(windows=None):
    return lambda H, W, th, tw: flip_sets(H, W, th, tw, windows or corner_windows(H, W, th, tw))


def _gen(finite=True):
    return lambda H, W, th, tw: general_sets(H, W, th, tw, finite)


STAT_KINDS = ["sparse", "zeros", "c03", "c02", "normal"]
N_FIN = len(general_sets(40, 56, 32, 32, True))
ROWS = {
    # exact mode: bit for bit
    "x_s1_c1_nchw": _row("s1", 1, _flips(), ["nan"]),
    "x_s1_c1_nhwc4": _row("s1", 1, _flips(), ["nan"], nhwc=True, Cpad=4),
    "x_s2_c2_nhwc4": _row("s2", 2, _flips([(0, 0), (3, 7), (1, 4), (2, 0)]), ["nan"], pidx=[3, 1, 0, 2, 2], nhwc=True, Cpad=4),
    "x_s3_c5_nchw": _row("s3", 5, _flips([(0, 0), (1, 8), (0, 3), (1, 5)]), ["nan"]),                          # the 16-byte path
    "x_s3_c5_nchw_skew": _row("s3", 5, _flips([(0, 0), (1, 8), (0, 3), (1, 5)]), ["nan"], skew=1),             # the per-pixel path
    "x_s4_c2_nchw": _row("s4", 2, _flips(), ["nan"], pidx=[0, 1, 2, 3, 1, 1]),
    "x_s4_c5_nhwc8": _row("s4", 5, _flips(), ["nan"], nhwc=True, Cpad=8),
    "x_s3_c5_nhwc16": _row("s3", 5, _flips([(1, 8), (0, 0), (1, 0), (0, 8)]), ["nan"], nhwc=True, Cpad=16),
    "x_s3_c2_nchw_stats": _row("s3", 2, _flips([(0, 0), (1, 8), (0, 4), (1, 4)]), STAT_KINDS, pidx=[0, 1, 2, 3, 1, 2, 3, 0, 0, 1], stats=True),
    "x_s2_c2_nhwc4_stats": _row("s2", 2, _flips(), STAT_KINDS, pidx=[1] * 5, stats=True, nhwc=True, Cpad=4),   # all tensors on one set
    # general mode on finite data: per pixel
    "g_s1_c1_nchw": _row("s1", 1, _gen()),
    "g_s2_c2_nhwc4": _row("s2", 2, _gen(), nhwc=True, Cpad=4),
    "g_s3_c5_nhwc8": _row("s3", 5, _gen(), nhwc=True, Cpad=8, pidx=list(reversed(range(N_FIN)))),
    "g_s4_c5_nhwc16": _row("s4", 5, _gen(), nhwc=True, Cpad=16),
    "g_s4_c2_nchw": _row("s4", 2, _gen()),
    "g_s2_c2_nchw_skew": _row("s2", 2, _gen(), skew=1),
    "g_s2_c2_nchw_stats": _row("s2", 2, _gen(), STAT_KINDS, stats=True),
    "g_s3_c5_nhwc8_stats": _row("s3", 5, _gen(), STAT_KINDS, stats=True, nhwc=True, Cpad=8),
    # general mode on NaN data: the NaN masks
    "g_s2_c2_nchw_nan": _row("s2", 2, _gen(False), ["nan"]),
    "g_s4_c5_nhwc8_nan": _row("s4", 5, _gen(False), ["nan"], nhwc=True, Cpad=8),
    # the grid-stride loop's second trip: 4100 sources in one arena, four sets (two exact, two general)
    "big": _row("big", 1, lambda H, W, th, tw: flip_sets(H, W, th, tw, [(0, 0), (2, 5), (1, 3), (2, 0)])[1:3] + general_sets(H, W, th, tw, False)[:2],
                ["sparse"], pidx=[(g * 7) % 4 for g in range(BIG_G)]),
}


@functools.lru_cache(maxsize=None)
def sources(name):
    r = ROWS[name]
    gen = torch.Generator().manual_seed(2000 + sorted(ROWS).index(name))
    return [_source(k, r["C"], r["H"], r["W"], gen) for k in r["kinds"]]


def set_of(r, g):
    """the set tensor g uses: pidx[g] clamped into the table, as the kernel does"""
    p = g if r["pidx"] is None else r["pidx"][g]
    return min(max(p, 0), len(r["params"]) - 1)


@functools.lru_cache(maxsize=None)
def expected(name):
    """per parameter set in use: (tensors [n], ref [n][C][th][tw], bound or None (exact mode: bit for bit), near [th][tw] or None)"""
    return expected_of(ROWS[name], sources(name))


def expected_of(r, srcs):
    C, H, W, th, tw = r["C"], r["H"], r["W"], r["th"], r["tw"]
    bx, by = ar.base_coords(W), ar.base_coords(H)
    read, vb = [], []
    for s in srcs:
        v, b = ar.normalized(s) if r["stats"] else (s, None)
        read.append(v)
        vb.append(torch.zeros_like(s) if b is None else b)
    out = []
    for p in sorted({set_of(r, g) for g in range(r["G"])}):
        gs = [g for g in range(r["G"]) if set_of(r, g) == p]
        th6, top, left, exact, flips = r["params"][p]
        top, left = ar.clamp_window(top, left, H, W, th, tw)
        stack = torch.cat([read[g] for g in gs])
        if exact:
            ref, bound, near = ar.exact(stack, H, W, th, tw, top, left, flips), None, None
            if r["stats"]:                        # the copied values are normalised in fp32 on the way (bound 0: bit for bit)
                bound = ar.exact(torch.cat([vb[g] for g in gs]), H, W, th, tw, top, left, flips)
        else:
            ref, bound, near = ar.general(stack, th6, bx, by, th, tw, top, left, torch.cat([vb[g] for g in gs]) if r["stats"] else None)
        shape = (len(gs), C, th, tw)
        out.append((gs, ref.view(shape), None if bound is None else bound.view(shape), near))
    return out


def stats_of(name):
    """[G][3] float64: the statistics handed to the launch"""
    return torch.stack([ar.nonzero_stats(s) for s in sources(name)])
