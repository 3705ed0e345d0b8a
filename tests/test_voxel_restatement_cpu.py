"""CPU anchors of tests/voxel_restatement.py and tests/voxel_cases.py (no GPU): the float64 statement against the oracle and the reference's
recorded grids, the exactness condition of every dyadic row, the restated launcher geometry and form selection against the table of
the rows, and the vote count the derived bound uses.  profiles/voxel_launch_tests_notes.md."""
import os

import numpy as np
import pytest

from oracle import voxel_ref
import voxel_cases as vc
import voxel_restatement as vr

VOX = ["rand", "rand10", "onebin", "single", "same_t", "corners", "int_ts_pm1"]
SMALL = [n for n in vc.ROWS if n not in ("e254", "e255", "chunks65")]           # (the three large rows are anchored by the sums below)


@pytest.mark.parametrize("name", VOX)
def test_statement_against_the_reference_grids(golden_dir, name):
    """well-formed events: the float64 sum of the votes, rounded once, is the reference's sequential fp32 sum up to its own roundings,
    and where a cell has one vote it is the reference's number"""
    z = np.load(os.path.join(golden_dir, "voxel.npz"), allow_pickle=False)
    ev = z["%s.events" % name]
    bins, W, H = [int(v) for v in z["%s.dims" % name]]
    st = vr.grid(ev, bins, W, H)
    ref = z["%s.grid_torch" % name]
    assert np.array_equal(voxel_ref.events_to_voxel_grid(ev, bins, W, H), ref)
    assert np.all(np.abs(ref - st["exact"]) <= vr.bound_atomic(st))
    one = st["k"] == 1
    assert np.array_equal(ref[one], st["exact"][one].astype(np.float32)) and np.all(ref[st["k"] == 0] == 0)
    assert np.all(np.abs(st["fixed"] - st["exact"]) <= vr.bound_sorted(st))
    il, ir = vr.indices(ev, bins, W, H)
    zi = np.load(os.path.join(golden_dir, "voxel_indices.npz"), allow_pickle=False)
    assert np.array_equal(il[il >= 0], zi["%s.ref_idx_left" % name]) and np.array_equal(ir[ir >= 0], zi["%s.ref_idx_right" % name])


def test_in_image_rule():
    """-1 < v < N on the double; the integer conversion truncates towards zero; NaN, +-inf and 1e300 cast no vote"""
    W, H = 6, 4
    ev = np.array([[0, x, 1, 1] for x in (-0.5, -1.0, W - 1, W - 0.01, W, np.nan, np.inf, -np.inf, 1e300, -1e300)]
                  + [[0, 2, y, 1] for y in (-0.5, -1.0, H - 1, H - 0.01, H, np.nan, np.inf, -np.inf, 1e300, -1e300)] + [[1, 0, 0, 1]], np.float64)
    il, ir = vr.indices(ev, 1, W, H)
    assert il.tolist() == [6, -1, 11, 11, -1, -1, -1, -1, -1, -1, 2, -1, 20, 20, -1, -1, -1, -1, -1, -1, 0] and np.all(ir == -1)
    st = vr.grid(ev, 1, W, H)
    assert st["k"].sum() == 7 and st["exact"][0, 1, 5] == 2 and st["exact"][0, 3, 2] == 2


@pytest.mark.parametrize("name", [n for n in vc.DYADIC if n in SMALL])
def test_dyadic_rows_are_exact_in_fp32(name):
    st = vc.statement(name)
    r = vc.ROWS[name]
    for ev in vc.data(name):
        if len(ev):
            _, vl, okl, _, vr_, okr = vr.votes(ev, r["bins"], r["W"], r["H"])
            v = np.concatenate([vl[okl], vr_[okr]]).astype(np.float64) * 1024
            assert np.array_equal(v, np.round(v)), "%s: a vote is no multiple of 2^-10" % name
    assert float(st["abs"].max()) * 2 ** 10 < 2 ** 24
    # then the reference's own sequential fp32 accumulation is the float64 sum, bit for bit
    for g, ev in enumerate(vc.data(name)):
        if 0 < len(ev) <= 20000:
            with np.errstate(invalid="ignore"):          # (the NaN stamps: converted, then masked by the oracle's own guards)
                ref = voxel_ref.events_to_voxel_grid(_clean(ev, r["W"], r["H"]), r["bins"], r["W"], r["H"])
            assert np.array_equal(ref.astype(np.float64), st["exact"][g])
    for g, x, y in vc.hot_cells(name):
        assert np.all(st["exact"][g, :, y, x] == 0) and st["k"][g, 0, y, x] == vc.HOT and not np.signbit(st["exact"][g, :, y, x]).any()
    assert np.all(st["dyadic40"]) and np.array_equal(st["fixed"].astype(np.float64), st["exact"])


def _clean(ev, W, H):
    """the events of a list the oracle can take (inside the image), the first and the last event kept for t0 and t1"""
    keep = vr.in_image(ev[:, 1], W) & vr.in_image(ev[:, 2], H)
    keep[[0, -1]] = True
    return ev[keep]


@pytest.mark.parametrize("name", vc.NORMAL)
def test_normal_rows_vote_counts(name):
    st = vc.statement(name)
    assert int(st["k"].max()) <= 2 ** 12 and int(st["k"].max()) >= 2
    assert (st["k"] == 1).any() and (st["k"] == 0).any()


@pytest.mark.parametrize("name", list(vc.ROWS))
def test_geometry_and_selection(name):
    r = vc.ROWS[name]
    G, bins, W, H, mx = len(r["lens"]), r["bins"], r["W"], r["H"], vc.max_events(name)
    rows = dict(sorted=vr.sorted_rows(bins, W, H, G, mx, vr.MIN_SORTED_ENTRY), ids=vr.band_rows(bins, W, H, G, vr.QUEUE_IDS) if mx else 0,
                idless=vr.band_rows(bins, W, H, G, vr.QUEUE_IDLESS))
    for form, rw in rows.items():
        if form in r["geo"]:
            assert vr.geometry(rw, H) == r["geo"][form], (name, form, vr.geometry(rw, H))
        else:
            assert rw == 0, (name, form, rw)
    for key, kw in (("batch", {}), ("unsorted", dict(voxel_sorted=False)), ("capture", dict(capture=True))):
        form, rw = vr.select(G, mx, bins, W, H, **kw)
        assert form == r[key], (name, key, form)
        if rw:
            assert vr.geometry(rw, H) == r["geo"][form]
    form, rw = vr.select(G, mx, bins, W, H, entry="sorted")
    assert form == (None if name in vc.REFUSED else "zero_fill" if mx == 0 else "sorted")
    assert (name in vc.REFUSED) == (vc.REFUSED.get(name) == (bins, W, H))
    # every list length of the row is what the row says, max_events covers them, and the specials are in (where a list has room)
    assert tuple(len(e) for e in vc.data(name)) == r["lens"] and mx >= max(r["lens"])


def test_limits_of_the_restated_launcher():
    assert vr.band_rows(10, 346, 260, 16, vr.QUEUE_IDS) == 9 and vr.band_rows(5, 346, 260, 15, vr.QUEUE_IDS) == 0
    assert vr.geometry(vr.sorted_rows(5, 2048, 254, 2, 8193), 254) == (1, 254, 1) and vr.sorted_rows(5, 2048, 255, 2, 8193) == 0
    assert vr.sorted_rows(5, 24, 16, 1, 100) == 0 and vr.sorted_rows(5, 24, 16, 1, 100, vr.MIN_SORTED_ENTRY) == 16
    assert vr.sorted_rows(1, 1, 32768, 2, 100) == 0 and vr.sorted_rows(1, 32768, 1, 2, 100) == 0 and vr.sorted_rows(5, 24, 16, 2, 2 ** 30) == 0
    assert vr.select(1, 5, 5, 24, 16) == ("atomic_batch", 0) and vr.select(1, 0, 5, 24, 16, entry="single") == ("zero_fill", 0)
    assert vr.kernel_name("sorted", 3) == "voxel_sort_chunks_kernel + voxelize_sorted_kernel<rows=3>"


def test_large_rows():
    """chunks65: 66 chunks, more than one trip of 64; e254: every band a single row; both exact in fp32"""
    assert -(-vc.max_events("chunks65") // vr.CHUNK) == 66
    for name in ("chunks65", "e254", "e255"):
        st = vc.statement(name)
        assert float(st["abs"].max()) * 2 ** 10 < 2 ** 24 and np.array_equal(st["exact"] * 1024, np.round(st["exact"] * 1024))
        assert np.all(st["dyadic40"]) and np.array_equal(st["fixed"].astype(np.float64), st["exact"])
        assert vc.hot_cells(name) and all(np.all(st["exact"][g, :, y, x] == 0) for g, x, y in vc.hot_cells(name))
    assert int(vc.statement("chunks65")["k"].sum()) > 10 ** 6
