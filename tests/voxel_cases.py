"""The rows of tests/test_hip_voxel_launch.py and tests/test_voxel_restatement_cpu.py: shape, list lengths, data kind, the geometry
(rows of a band, bands, rows of the last band) every banded form is meant to have on the row, and the form that takes
`ramnet_voxelize_batch` by default, with option voxel_sorted = 0, and inside a stream capture.  profiles/voxel_launch_tests_notes.md.

Data kinds.  dyadic: integer stamps, first = offset, last = offset + (bins - 1) * 1024, so every time fraction is a multiple of 2^-10 and
every vote and partial sum is exact in fp32 in any order (asserted per row on the CPU); polarities 0.5 sit on even stamps.  normal:
recipe.synth_events.  Both carry the hand-placed events of `specials`: coordinates on and beyond every edge of the image and of every
form's bands, NaN, +-inf, +-1e300, polarities 0 / 1 / -1 / 2 / 0.5, stamps below the first, above the last, equal to the last, NaN."""
import functools
import zlib

import numpy as np

from recipe import synth_events
import voxel_restatement as vr

# list lengths around the id-less batch (4096), the sort chunk and the batch with ids (8192), and past one and two chunks
LENS16 = (0, 1, 2, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 16385, 0, 64, 1000, 3, 0)          # empty first, in the middle and last
HOT = 4096                                                                                        # events of the cancelling cell
OFFSETS = (0.0, 1e9, 0.0, 1.6e15)                                                                 # first stamp of list g: OFFSETS[g % 4]


def _row(bins, W, H, lens, kind="dyadic", slack=0, geo=None, batch="sorted", unsorted="atomic_batch", capture="atomic_batch", flat=()):
    """slack: max_events = longest list + slack.  geo: {form: (rows, bands, last)}.  batch / unsorted / capture: the form that takes
    ramnet_voxelize_batch by default / with voxel_sorted = 0 / inside a capture.  flat: lists whose stamps are all equal (dT = 0)."""
    return dict(bins=bins, W=W, H=H, lens=tuple(lens), kind=kind, slack=slack, geo=geo or {}, batch=batch, unsorted=unsorted, capture=capture,
                flat=tuple(flat))


A = dict(sorted=(3, 3, 1))
A16 = dict(sorted=(3, 3, 1), ids=(4, 2, 3), idless=(5, 2, 2))
BANDED = dict(unsorted="ids", capture="idless")
ROWS = {
    # 5 x 1360 x 7: three sorted bands with a last band of one row; list counts against the deal-by-8
    "a2": _row(5, 1360, 7, (8193, 16385), geo=A),
    "a3": _row(5, 1360, 7, (0, 4097, 2), geo=A),
    "a9": _row(5, 1360, 7, (1, 4095, 0, 4096, 8191, 8192, 12289, 2, 0), geo=A),
    "a16": _row(5, 1360, 7, LENS16, geo=A16, **BANDED),
    "a16n": _row(5, 1360, 7, LENS16, kind="normal", geo=A16, **BANDED),
    # max_events 5000 above the longest list (12289): a third chunk that is empty in every grid
    "a16_slack": _row(5, 1360, 7, LENS16[:10] + (100,) + LENS16[11:], slack=5000, geo=A16, **BANDED),
    "b17": _row(5, 1363, 7, LENS16 + (8193,), geo=dict(sorted=(2, 4, 1), ids=(4, 2, 3), idless=(5, 2, 2)), **BANDED),
    "c16": _row(10, 700, 9, (20000, 0, 4097, 8193, 1, 12289, 2, 16385, 4095, 4096, 0, 8191, 8192, 17, 300, 0),
                geo=dict(sorted=(2, 5, 1), ids=(4, 3, 1), idless=(5, 2, 4)), **BANDED),
    "c16n": _row(10, 700, 9, (20000, 0, 4097, 8193, 1, 12289, 2, 16385, 4095, 4096, 0, 8191, 8192, 17, 300, 0), kind="normal",
                 geo=dict(sorted=(2, 5, 1), ids=(4, 3, 1), idless=(5, 2, 4)), **BANDED),
    "d16": _row(2, 3400, 8, LENS16, geo=dict(sorted=(3, 3, 2), ids=(4, 2, 4), idless=(5, 2, 3)), **BANDED),
    # the 254-band limit: one-row bands; 255 bands fall back
    "e254": _row(5, 2048, 254, (8193, 300), geo=dict(sorted=(1, 254, 1))),
    "e255": _row(5, 2048, 255, (8193, 300), batch="atomic_batch"),
    # not even one row of 8-byte cells fits; one row of 4-byte cells does
    "f16": _row(5, 5000, 3, (4097, 0, 8193, 1) + (300,) * 11 + (0,), geo=dict(ids=(1, 3, 1), idless=(1, 3, 1)), batch="ids", **BANDED),
    # one band
    "s1": _row(5, 24, 16, (700,), geo=dict(sorted=(16, 1, 16)), batch="atomic_batch"),
    "s2": _row(5, 24, 16, (700, 0), geo=dict(sorted=(16, 1, 16))),
    "s3": _row(5, 24, 16, (0, 1, 4097), geo=dict(sorted=(16, 1, 16)), flat=(2,)),
    "s2n": _row(5, 24, 16, (4097, 700), kind="normal", geo=dict(sorted=(16, 1, 16))),
    "m1": _row(1, 40, 9, (300,), geo=dict(sorted=(9, 1, 9)), batch="atomic_batch"),
    "m2": _row(1, 40, 9, (0, 300), geo=dict(sorted=(9, 1, 9))),
    "m3": _row(1, 40, 9, (8193, 1, 0), geo=dict(sorted=(9, 1, 9))),
    # H against the x | y << 16 record
    "t32767": _row(1, 1, 32767, (4097, 5), geo=dict(sorted=(20406, 2, 12361))),
    "t32768": _row(1, 1, 32768, (4097, 5), batch="atomic_batch"),
    # 66 chunks: the second trip of the sorted form's prefix scan, with its carry
    "chunks65": _row(5, 24, 16, (65 * 8192 + 3, 10), geo=dict(sorted=(16, 1, 16))),
    # all lists empty, events = NULL
    "empty16": _row(5, 1360, 7, (0,) * 16, geo=dict(idless=(5, 2, 2)), batch="idless", unsorted="idless", capture="idless"),
    "empty2": _row(5, 1360, 7, (0, 0), batch="zero_fill", unsorted="zero_fill", capture="zero_fill"),
}
DYADIC = [n for n, r in ROWS.items() if r["kind"] == "dyadic"]
NORMAL = [n for n, r in ROWS.items() if r["kind"] == "normal"]
# the three rows ramnet_voxelize_batch_sorted refuses (bins, W, H)
REFUSED = {"e255": (5, 2048, 255), "f16": (5, 5000, 3), "t32768": (1, 1, 32768)}


def max_events(name):
    return max(ROWS[name]["lens"]) + ROWS[name]["slack"]


def band_edges(name):
    """the rows r * rows - 1, r * rows of every form's bands on this row, the first and the last row"""
    r = ROWS[name]
    ys = {0, r["H"] - 1}
    for rows, bands, _ in r["geo"].values():
        for b in range(1, bands):
            ys |= {b * rows - 1, b * rows}
    return sorted(ys)


def specials(name):
    """[(stamp kind, x, y, p)]: stamp kind "in" keeps the stamp of the event it replaces"""
    r = ROWS[name]
    W, H = r["W"], r["H"]
    pol = (0.0, 1.0, -1.0, 2.0, 0.5)
    out = []
    edge = lambda v: (-0.5, -1.0, v - 1.0, v - 0.01, float(v), float("nan"), float("inf"), float("-inf"), 1e300, -1e300)
    for i, x in enumerate(edge(W)):
        out.append(("in", x, float(i % H), pol[i % 5]))
    for i, y in enumerate(edge(H)):
        out.append(("in", 0.0, y, pol[(i + 2) % 5]))
    out.append(("in", float("nan"), float("nan"), 1.0))
    for i, y in enumerate(band_edges(name)):
        out.append(("in", float((7 * i) % W), float(y), pol[i % 5]))
        out.append(("in", float(W - 1 - (3 * i) % W), y + 0.75, pol[(i + 1) % 5]))
    for i, kind in enumerate(("below", "above", "far", "last", "nan") * 3):
        out.append((kind, float(i % W), float((2 * i) % H), pol[i % 5]))
    return out


def _hot_cell(r):
    return r["W"] // 2, r["H"] - 1


def _list(name, g, n):
    r = ROWS[name]
    bins, W, H = r["bins"], r["W"], r["H"]
    rng = np.random.default_rng(zlib.crc32(("%s/%d" % (name, g)).encode()))
    off = OFFSETS[g % 4]
    if n == 0:
        return np.zeros((0, 4))
    if r["kind"] == "normal":
        ev = synth_events(rng, n, W, H, t0=off, t1=off + 0.05)
        t0, t1 = ev[0, 0], ev[-1, 0]
    else:
        span = (bins - 1) * 1024 if g not in r["flat"] else 0
        ev = np.empty((n, 4))
        ev[:, 0] = np.sort(rng.integers(0, span + 1, n))
        if n >= 2:
            ev[0, 0], ev[-1, 0] = 0, span
        ev[:, 0] += off
        ev[:, 1], ev[:, 2], ev[:, 3] = rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)
        t0, t1 = off, off + span
    hot = r["kind"] == "dyadic" and n >= 2 * HOT and W >= 3
    hx, hy = _hot_cell(r)
    if hot:
        on = (ev[:, 1] == hx) & (ev[:, 2] == hy)
        ev[on, 1] = hx - 1
    # the specials go into the first quarter of a list (from 3 events: the first and the last event stay, they set t0 and t1)
    sp = specials(name)
    room = (n // 4 - 1) if hot else n - 2
    m = max(0, min(len(sp), room))
    # (a short list takes a window of the specials that moves with g, so that the short lists of a row cover different ones)
    start = 0 if m == len(sp) else (g * 7) % (len(sp) - m + 1) if m else 0
    for j, (kind, x, y, p) in enumerate(sp[start:start + m]):
        i = 1 + j
        if hot and (int(x) if x == x and abs(x) < 1e9 else -9, int(y) if y == y and abs(y) < 1e9 else -9) == (hx, hy):
            x = float(hx + 1)
        t = ev[i, 0]
        if r["kind"] == "dyadic" and p == 0.5:
            t = t0 + 2 * ((t - t0) // 2)                     # an even stamp: half a vote stays a multiple of 2^-10
        # (above the last stamp by less than a bin is still a left vote into the last bin: an even distance keeps half a vote dyadic)
        t = {"in": t, "below": t0 - 6, "above": t1 + 8, "far": t1 + 2048, "last": t1, "nan": float("nan")}[kind]
        ev[i] = (t, x, y, p)
    if hot:                                                 # 4096 events of alternating polarity and equal fraction in one cell: the sum is +0
        a = n // 4
        ev[a:a + HOT, 0] = t0 + (512 if t1 > t0 else 0)
        ev[a:a + HOT, 1], ev[a:a + HOT, 2] = hx, hy
        ev[a:a + HOT, 3] = np.arange(HOT) % 2
    return ev


@functools.lru_cache(maxsize=None)
def data(name):
    """the event lists of a row (float64 [n, 4] each); computed once, never modified"""
    lists = tuple(_list(name, g, n) for g, n in enumerate(ROWS[name]["lens"]))
    for ev in lists:
        ev.setflags(write=False)
    return lists


@functools.lru_cache(maxsize=None)
def statement(name):
    r = ROWS[name]
    st = vr.batch(data(name), r["bins"], r["W"], r["H"])
    for a in st.values():
        a.setflags(write=False)
    return st


def hot_cells(name):
    """[(g, x, y)] of the cancelling cells of a row"""
    r = ROWS[name]
    return [(g, ) + _hot_cell(r) for g, n in enumerate(r["lens"]) if r["kind"] == "dyadic" and n >= 2 * HOT and r["W"] >= 3]
