#!/usr/bin/env python3
"""tests/golden/render.npz: the REFERENCE's colour maps, as ITS make_colormap (RAM_Net/test.py:36-43) computes them with matplotlib's
ScalarMappable(Normalize(vmin, vmax), 'magma'), on seeded 37 x 53 maps.  Stored per case: the input map, (vmin, vmax) and the float RGBA
array make_colormap returned (BGR order in its first three channels: it is made for cv2.imwrite).

Cases (tests/render_restatement.py states what is expected of them; the assertions below are made on the reference output alone):
  pred        a prediction-like map in [0, 1]
  nan_target  a target with 20 % NaN: amax is NaN, nan_to_num(nan=1) makes the image constant
  constant    a constant map: 0 / 0 -> NaN -> 0
  zero        an all-zero map
  boundary    holds 0 and 1, so both amax are 1 and q = 1 - v exactly; the other values are, for every integer k = 1..256, the two
              neighbouring float32 v between which x * 256 crosses k — found by bisection on the float64-then-float32 arithmetic of
              Normalize (a float32 evaluation of `-= vmin` or `/= (vmax - vmin)` flips some of them, which the script counts)
  over        `pred` under a mapper with vmax < 1: over-range pixels
  degenerate  `pred` under vmin == vmax == 1, the mapper a NaN target frame gives (test.py:197-204)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference, _stub  # noqa: E402
import render_restatement as RR  # noqa: E402

H, W = 37, 53
MAPPER = (0.0625 + 1e-3, 0.9)           # vmin, vmax of every case but the last two (Python floats, as Normalize keeps them)
MAPPER_OVER = (0.1, 0.5)
CASES = ("pred", "nan_target", "constant", "zero", "boundary", "over", "degenerate")


def import_make_colormap():
    import_reference()
    _stub("train", concatenate_subfolders=None)
    _stub("skimage.io", imread=None)
    if not hasattr(np, "alltrue"):
        np.alltrue = np.all
    import test as ref_test
    return ref_test.make_colormap


def xa_of(v, vmin, vmax, single=False):
    """x * 256 of a pixel v of a map whose amax are both 1, under Normalize(vmin, vmax); single: the float32 evaluation that is NOT
    what matplotlib does (counted below)."""
    q = np.float32(1) - np.float32(v)
    if single:
        x = (q - np.float32(vmin)) / (np.float32(vmax) - np.float32(vmin))
    else:
        x = np.float32(np.float64(np.float32(np.float64(q) - vmin)) / (vmax - vmin))
    return np.float32(x) * np.float32(256)


def boundary_map(vmin, vmax):
    """0, 1 and for k = 1..256 the float32 pair (v_lo, v_hi), one ulp apart, with xa(v_lo) >= k > xa(v_hi) (xa falls as v grows)."""
    vals = [np.float32(0), np.float32(1)]
    for k in range(1, 257):
        lo, hi = np.float32(0).view(np.uint32), np.float32(1).view(np.uint32)        # bit patterns order like the values on [0, 1]
        assert xa_of(0.0, vmin, vmax) >= k > xa_of(1.0, vmin, vmax)
        while hi - lo > 1:
            mid = np.uint32((int(lo) + int(hi)) // 2)
            if xa_of(mid.view(np.float32), vmin, vmax) >= k:
                lo = mid
            else:
                hi = mid
        vals += [lo.view(np.float32), hi.view(np.float32)]
    vals = np.array(vals, np.float32)
    flips = sum(int(xa_of(v, vmin, vmax)) != int(xa_of(v, vmin, vmax, single=True)) for v in vals)
    rng = np.random.default_rng(7)
    m = rng.random(H * W).astype(np.float32)
    m[:len(vals)] = vals
    return rng.permutation(m).reshape(H, W), flips


def main():
    import matplotlib as mpl
    import matplotlib.cm as cm
    make_colormap = import_make_colormap()
    rng = np.random.default_rng(44)
    pred = np.clip(rng.random((H, W)) + 0.05 * rng.standard_normal((H, W)), 0, 1).astype(np.float32)
    target = rng.random((H, W)).astype(np.float32)
    target[rng.random((H, W)) < 0.2] = np.nan
    bmap, flips = boundary_map(*MAPPER)
    print("boundary map: %d of its crossing values change their colour under a float32 normalisation" % flips)
    assert flips > 0
    maps = {"pred": pred, "nan_target": target, "constant": np.full((H, W), 0.37, np.float32), "zero": np.zeros((H, W), np.float32),
            "boundary": bmap, "over": pred, "degenerate": pred}
    limits = {c: MAPPER for c in CASES}
    limits["over"], limits["degenerate"] = MAPPER_OVER, (1.0, 1.0)
    magma = mpl.colormaps["magma"]
    magma._init()
    lut = np.asarray(magma._lut)[:258]                  # (the last row is the colour of masked values: none here)
    out = {}
    for c in CASES:
        vmin, vmax = limits[c]
        mapper = cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=vmin, vmax=vmax), cmap="magma")
        with np.errstate(all="ignore"):
            rgba = make_colormap(maps[c][None].copy(), mapper)
        assert rgba.shape == (H, W, 4) and rgba.dtype == np.float64 and np.all(rgba[..., 3] == 1.0)
        out[c + ".map"], out[c + ".limits"], out[c + ".rgba"] = maps[c], np.array([vmin, vmax], np.float64), rgba
        colours = {tuple(p) for p in rgba.reshape(-1, 4)}
        print("%-10s vmin %.6f vmax %.6f: %d distinct colours" % (c, vmin, vmax, len(colours)))
        rows = {tuple(r[[2, 1, 0, 3]]) for r in lut}       # make_colormap's BGR
        assert colours <= rows
        if c in ("nan_target", "constant", "zero", "degenerate"):
            assert len(colours) == 1
        if c == "nan_target":                               # q = 1 everywhere: over the mapper's vmax
            assert colours == {tuple(lut[257][[2, 1, 0, 3]])}
        if c in ("constant", "zero"):                       # q = 0 < vmin: under
            assert colours == {tuple(lut[256][[2, 1, 0, 3]])}
        if c == "degenerate":
            assert colours == {tuple(lut[0][[2, 1, 0, 3]])}
        if c == "boundary":
            assert colours == rows and np.amax(bmap) == 1 and np.amin(bmap) == 0      # every row (magma's under / over repeat its ends)
        if c == "over":
            assert tuple(lut[257][[2, 1, 0, 3]]) in colours and tuple(lut[256][[2, 1, 0, 3]]) in colours
    # test.py:197-204 is inline in main(): the mapper limits can only be restated, with matplotlib's Normalize holding what it was given
    vmin, vmax = RR.mapper_limits(pred[None])
    n = mpl.colors.Normalize(vmin=np.float32(vmin), vmax=vmax)
    assert type(n.vmin) is float and n.vmin == vmin
    path = os.path.join(HERE, "render.npz")
    np.savez_compressed(path, **out)
    print("render.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
