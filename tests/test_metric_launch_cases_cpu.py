"""No GPU: the rows of tests/metric_launch_cases.py reach the branches their names say, the plans restated there are the library's own
(its host-only workspace functions), the statements have the NaN patterns the rows claim, one guard element read as a pixel would change
count, sum and median, and the resize statement is torch's F.interpolate."""
import numpy as np
import pytest
import torch

import eval_table_restatement as R
import metric_launch_cases as K

F32 = np.float32


def lib():
    from rpg_ramnet_amd import _hip
    return _hip.lib()


# ------------------------------------------------------------------------------------------------ plans
def test_batch_metrics_rows_reach_their_plan():
    L = lib()
    for (N, npix), (Ws, P) in K.BM_PLAN_ROWS.items():
        assert K.bm_plan(N, npix) == (Ws, P), (N, npix)
    assert K.bm_plan(16, 8192) == (1, 16) and K.bm_plan(1, 32 * 8192) == (32, 32) and K.bm_plan(1, 33 * 8192) == (32, 32)
    got = {}
    for (N, npix), s in K.BM_STAGE_ROWS.items():
        Ws, P = K.bm_plan(N, npix)
        assert Ws == 1 and P == N and (s >= K.BM_STAGE or P == K.BM_STAGE) and s < N
        got[P] = -(-P // K.BM_STAGE)
    assert got == {64: 1, 65: 2, 70: 2, 128: 2, 130: 3}                      # chunks of staged rows; 130: a ragged third
    # P through the size the library states: the slab term, 16384 bytes per workgroup and pair, dominates
    for G in (1, 2):
        for N, npix in list(K.BM_PLAN_ROWS) + list(K.BM_STAGE_ROWS) + [(n, p) for n, p, _ in K.BM_RANK_SHAPES.values()]:
            assert L.ramnet_batch_metrics_workspace(G, N, npix) == K.bm_workspace_bytes(G, N, npix), (G, N, npix)
    for N, npix in K.BM_PLAN_ROWS:
        P = K.bm_plan(N, npix)[1]
        assert (L.ramnet_batch_metrics_workspace(1, N, npix) - K.TICKET_BYTES) // K.BM_SLAB_BYTES == P


def test_eval_table_rows_reach_their_plan():
    L = lib()
    for tag, npix in K.ET_CAP_ROWS.items():
        assert K.et_plan(npix, 1, True) == (4, 32)
    assert K.et_plan(31 * 16384, 1, True) == (4, 31) and K.et_plan(260 * 346, 6, True) == (14, 6)        # (the largest map of the older tests)
    assert K.et_plan(15, 8, True)[0] == 18 and 300 * 18 == 5400
    for G, npix, ncut, has_mask in ((1, 31 * 16384 + 1, 1, 1), (1, 32 * 16384 + 7, 1, 1), (300, 15, 8, 1), (4096, 1, 0, 0), (2, 37 * 53, 8, 1), (3, 7, 2, 1)):
        assert L.ramnet_eval_table_workspace(G, npix, ncut, has_mask) == K.et_workspace_bytes(G, npix, ncut, has_mask)
        for flags in K.FLAG_SETS:
            assert L.ramnet_eval_table_ex_workspace(G, npix, ncut, has_mask, flags) == K.et_workspace_bytes(G, npix, ncut, has_mask, flags)
    # cells beyond the tickets: 65536 of them (RAMNET_EVAL_TABLE_TICKET_BYTES / 4)
    assert K.ET_MAX_CELLS == 65536 and 3641 * 18 == 65538
    assert L.ramnet_eval_table_workspace(3641, 15, 8, 1) == 0 and L.ramnet_eval_table_workspace(3640, 15, 8, 1) > 0
    assert L.ramnet_eval_table_workspace(911, 15, 8, 1) > 0                  # 16398 cells are within the tickets


def test_workspace_functions_return_zero_for_what_the_calls_reject():
    L = lib()
    assert L.ramnet_batch_metrics_workspace(1, 65536, 1) == 0 and L.ramnet_batch_metrics_workspace(65536, 1, 1) == 0
    assert L.ramnet_batch_metrics_workspace(1, 1, 0) == 0 and L.ramnet_batch_metrics_workspace(1, 2, 1 << 30) == 0
    assert L.ramnet_batch_metrics_workspace(0, 1, 8) == 0 and L.ramnet_batch_metrics_workspace(1, 0, 8) == 0
    assert L.ramnet_eval_table_workspace(0, 8, 0, 0) == 0 and L.ramnet_eval_table_workspace(65536, 8, 0, 0) == 0
    assert L.ramnet_eval_table_workspace(1, 0, 0, 0) == 0 and L.ramnet_eval_table_workspace(1, 8, 9, 0) == 0 and L.ramnet_eval_table_workspace(1, 8, -1, 0) == 0
    assert L.ramnet_eval_table_ex_workspace(1, 8, 0, 0, 4) == 0 and L.ramnet_eval_table_ex_workspace(1, 8, 0, 0, 3) > 0


# ------------------------------------------------------------------------------------------------ rank parting
@pytest.mark.parametrize("name", list(K.BM_RANK_ROWS))
def test_batch_metrics_rank_rows_part_where_they_say(name):
    vals, want = K.BM_RANK_ROWS[name]
    assert list(vals) == sorted(vals) and len(vals) == 6
    for shape, (N, npix, odd) in K.BM_RANK_SHAPES.items():
        p, t = K.bm_rank_pair(name, shape)
        d = np.abs(t - p)
        assert np.array_equal(d[~np.isnan(d)], t[~np.isnan(t)]) and int((~np.isnan(d)).sum()) == (7 if odd else 6)
        assert K.parting_pass(d) == (0 if odd else want), (name, shape)
        if N == 2 and not odd:                                               # the two middle elements in different workgroups
            s = np.sort(d.ravel())
            assert s[2] in d[0] and s[3] in d[1] and (want == 0 or (s[2] not in d[1] and s[3] not in d[0]))
    if name.startswith("ties"):
        run = [i for i, v in enumerate(vals) if v == F32(0.25)]
        assert {"ties_inside": run[0] < 2 and run[-1] > 3, "ties_first": run[0] == 2, "ties_last": run[-1] == 3}[name]


def test_batch_metrics_extreme_rows_have_the_medians_and_nan_patterns_they_claim():
    want = {"zero": 0.0, "denormal": float(F32((F32(1e-40) + F32(2e-40)) * F32(0.5))), "inf": np.inf}
    for name, (p, t) in K.BM_EXTREME_ROWS.items():
        row, bound = K.bm_statement(p.reshape(1, 6), t.reshape(1, 6))
        assert row[0] == row[1] == 6, name                                  # an infinite prediction still counts: column 0 == column 1
        if name in want:
            assert row[8] == want[name], (name, row[8])
        assert K.parting_pass(np.abs(t - p)) == {"zero": 0, "denormal": 2, "fltmax_half": 3, "inf": 1}[name]
    row = K.bm_statement(*[x.reshape(1, 6) for x in K.BM_EXTREME_ROWS["denormal"]])[0]
    assert 0 < row[8] < np.finfo(F32).tiny and np.isfinite(row).all()
    row = K.bm_statement(*[x.reshape(1, 6) for x in K.BM_EXTREME_ROWS["fltmax_half"]])[0]
    assert np.isfinite(row[[3, 7, 8]]).all() and np.isposinf(row[[2, 5, 6]]).all() and np.isnan(row[4])      # d^2 overflows in float32; inf / inf
    row = K.bm_statement(*[x.reshape(1, 6) for x in K.BM_EXTREME_ROWS["inf"]])[0]
    assert np.isposinf(row[[2, 3, 4, 5, 7, 8]]).all() and np.isnan(row[6])                       # inf - inf


def test_batch_metrics_stage_rows_have_one_nan_mse():
    for (N, npix), s in K.BM_STAGE_ROWS.items():
        for g in range(2):
            p, t = K.bm_pair(100 * N + g, N, npix, nan_sample=s)
            row, _ = K.bm_statement(p, t)
            assert np.isnan(row[2]) and np.isfinite(np.delete(row, 2)).all() and row[0] == row[1] > 0
            p, t = K.bm_pair(100 * N + g, N, npix)
            assert np.isfinite(K.bm_statement(p, t)[0]).all()


# ------------------------------------------------------------------------------------------------ poison
def test_one_guard_element_read_as_a_pixel_changes_count_sum_and_median():
    """the guards are finite: read as a pixel, one of them changes count, sums and median of the statement (a NaN guard would vanish)"""
    p, t = K.bm_pair(7, 2, 9)
    row, bound = K.bm_statement(p, t)
    for pp, tt in ((K.POISON_P, K.POISON_T), (K.POISON_P, t[1, 1]), (p[1, 1], K.POISON_T)):      # both maps over-read, or one of them
        p2, t2 = np.append(p.ravel(), pp).reshape(1, -1), np.append(t.ravel(), tt).reshape(1, -1)
        row2, _ = K.bm_statement(p2.astype(F32), t2.astype(F32))
        assert row2[0] == row[0] + 1 and row2[8] != row[8]
        assert all(not abs(row2[c] - row[c]) <= bound[c] for c in (3, 4, 5, 6, 7))
    ps, ts, ms = K.et_pairs(8, 1, (3, 5))
    tm, pm = R.metric_depth_numpy(ts[0], K.CLIP, K.REG), R.metric_depth_numpy(ps[0], K.CLIP, K.REG, clamp=True)
    for flags in (K.TARGET_METRIC, K.TARGET_METRIC | K.RESCALE):
        rows, bound = K.et_statement(tm.ravel(), pm.ravel(), np.ones(15, np.uint8), (20.0,), flags)
        tm2, pm2 = np.append(tm.ravel(), K.POISON_T), np.append(pm.ravel(), F32(K.CLIP))              # (a poison prediction clamps to clip)
        rows2, _ = K.et_statement(tm2, pm2, np.append(np.ones(15, np.uint8), np.uint8(0xA5)), (20.0,), flags)
        for v in (0, 2):                                                     # all pixels, and under the mask (whose guard reads as inside)
            assert rows2[v, 0] == rows[v, 0] + 1 and rows2[v, 11] != rows[v, 11]
            assert all(not abs(rows2[v, c] - rows[v, c]) <= bound[v, c] for c in (2, 3, 4, 7))
    assert np.isfinite(K.POISON_P) and np.isfinite(K.POISON_T)


# ------------------------------------------------------------------------------------------------ evaluation table rows
@pytest.mark.parametrize("name", list(K.ET_STREAM_ROWS))
def test_eval_table_stream_rows_part_where_they_say(name):
    tm, pn, pass_t, pass_p = K.ET_STREAM_ROWS[name]
    pm = R.metric_depth_numpy(pn, K.CLIP, K.REG, clamp=True)
    assert K.parting_pass(tm) == pass_t and K.parting_pass(pm) == pass_p, (K.parting_pass(tm), K.parting_pass(pm))
    assert K.parting_pass(tm[:5]) == 0 and K.parting_pass(pm[:5]) == 0                        # the odd sibling
    if name == "both_pass2_other_prefixes":
        a, b = np.sort(K.bits(tm))[2:4], np.sort(K.bits(pm))[2:4]
        assert a[0] >> 20 == a[1] >> 20 and b[0] >> 20 == b[1] >> 20 and a[0] >> 20 != b[0] >> 20
    if "never" in name and pass_p == 0:
        lo = F32(np.exp(F32(-K.REG)) * F32(K.CLIP))
        assert len(set(pm.tolist())) == 1 and pm[0] in (F32(K.CLIP), lo)


def test_eval_table_cutoff_row_is_strict_and_keeps_nan_inside():
    cut = (10.0, 30.0)
    tm = K.cutoff_targets(cut)
    rows, _ = K.et_statement(tm, np.full(tm.size, 20.0, F32), None, cut, K.TARGET_METRIC)
    below10 = int((tm < F32(10)).sum())
    assert below10 == 2 and int((tm < F32(30)).sum()) == 5                 # 1, nextafter(10, 0); + 10, nextafter(10, inf), nextafter(30, 0)
    assert rows[1, 0] == below10 + 1 and rows[1, 1] == below10              # the NaN target: inside (column 0), not counted (column 1)
    assert rows[2, 0] == 6 and rows[2, 1] == 5 and rows[0, 0] == tm.size
    assert np.isnan(rows[:, 11]).all()                                      # a NaN inside every variant


def test_conversion_values_cover_the_clamp_bounds():
    y = K.conversion_values()
    assert y.size == 4096 and y.min() == F32(-0.5) and y.max() == F32(1.5)
    for e in (0.0, 1.0):
        assert (y == F32(e)).any() and (y == np.nextafter(F32(e), F32(9))).any() and (y == np.nextafter(F32(e), F32(-9))).any()
    m = R.metric_depth_numpy(y, K.CLIP, K.REG, clamp=True)
    assert (m == F32(K.CLIP)).sum() > 1000 and (m == m.min()).sum() > 1000


def test_big_rows_keep_finite_medians_under_the_mask():
    ps, ts, ms = K.et_pairs(41, 1, (1, 4096), nan_frac=0.1)
    tm, pm = R.metric_depth_numpy(ts[0], K.CLIP, K.REG), R.metric_depth_numpy(ps[0], K.CLIP, K.REG, clamp=True)
    rows, _ = K.et_statement(tm, pm, ms[0], (20.0,), 0)
    assert np.isnan(rows[:2, 11]).all() and np.isfinite(rows[2:, 2:13]).all() and rows[0, 0] > rows[0, 1] and (rows[2:, 0] == rows[2:, 1]).all()


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("H,W,s", K.RESIZE_ROWS)
def test_resize_statement_is_interpolate(H, W, s):
    import torch.nn.functional as Fn
    if int(np.floor(H * s)) == 0:
        return                                                               # (1, 9, 0.5): the row the entry point refuses
    rng = np.random.default_rng(H * 100 + W)
    md = R.metric_depth_numpy(rng.random((H, W)).astype(F32), K.CLIP, K.REG)
    want = Fn.interpolate(torch.from_numpy(md).double()[None, None], scale_factor=s, mode="bilinear")[0, 0].numpy()
    got = K.resize_statement(md, s)
    assert got.shape == want.shape == (int(np.floor(H * s)), int(np.floor(W * s))) and got.dtype == F32
    # one float32 rounding of the float64 value (2^-24 relative), and the float64 evaluation orders of the two (a few 2^-53)
    assert np.all(np.abs(got.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) * (1 + 1e-6))
    if s == 1.0:
        assert np.array_equal(got, md)


def test_resize_rows_sit_beside_an_integer():
    near = [(n, s) for H, W, s in K.RESIZE_ROWS for n in (H, W) if abs(n * s - round(n * s)) < 1e-9 and n * s != round(n * s)]
    assert near == [(100, 0.29)]                                            # just below 29: floor gives 28
    assert 10 * 0.3 == 3.0 and 9 * (1.0 / 3.0) == 3.0 and 30 * 0.7 == 21.0 and 10 * 0.7 == 7.0      # inexact factors whose product rounds to the integer itself
    assert int(np.floor(10 * 0.3)) == 3 and int(np.floor(100 * 0.29)) == 28 and int(np.floor(10 * 0.7)) == 7 and int(np.floor(9 * (1.0 / 3.0))) == 3
