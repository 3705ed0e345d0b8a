"""No GPU: the float64 restatement of a RESCALED evaluation table and of the target resize (tests/eval_rescale_restatement.py) against the
REFERENCE's own cells (tests/golden/eval_rescale.npz: prepare_depth_data, then add_to_metrics(..., rescale=True) per file and variant, and
the same with --down_scale_factor 0.5 / 0.7) — the test that keeps the GPU tests of the HIP kernels honest —, the host part on rescaled
rows, the argument checks of the new entry points and their header / binding.

Measured here (profiles/eval_rescale_notes.md): over the 54 finite rescaled cells abs_rel_diff differs from the reference by 1.050e-3
relative at most (asserted: 4 x that, 4.2e-3); every other column stays inside rtol 1e-4 / atol 2e-5 (worst 5.7e-5 relative, SILog)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eval_rescale_restatement as RS
import eval_table_restatement as R
from util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated_cells():
    """[(tag, rescale, [V, 16] rows, [V, 10] cells of the restatement, [V, 10] reference cells, [V] raised)]"""
    out = []
    for tag, clip, reg, s, t_in, p_in, mask, cells, raised, n_mask in RS.golden_files(load_golden("eval_rescale.npz")):
        t, p = R.metric_depth_numpy(t_in, clip, reg), R.metric_depth_numpy(p_in, clip, reg, clamp=True)
        if s < 1.0:
            t = RS.resize_bilinear(t, s).astype(np.float32)
            assert t.shape == p.shape == mask.shape
        for rescale in sorted(cells):
            rows = (RS.restate_rescaled_rows if rescale else R.restate_rows)(t, p, mask)
            assert np.array_equal(rows[:, 0], n_mask), tag
            out.append((tag, rescale, rows, RS.rows_to_cells(rows), cells[rescale], raised[rescale]))
    return out


def test_restatement_meets_every_reference_cell():
    worst, finite, nraised = 0.0, 0, 0
    for tag, rescale, rows, got, want, raised in restated_cells():
        if not rescale:
            assert not raised.any()
            R.check_cells(got, want, (tag, "plain"))
            continue
        RS.check_rescaled_cells(got, want, raised, tag)
        keep = ~raised & np.isfinite(want[:, RS.ABS_REL])
        if keep.any():
            worst = max(worst, float(np.max(np.abs(got[keep, RS.ABS_REL] - want[keep, RS.ABS_REL]) / np.abs(want[keep, RS.ABS_REL]))))
        finite, nraised = finite + int(keep.sum()), nraised + int(raised.sum())
    print("rescaled abs_rel_diff, restatement - reference: %.3e relative at most over %d finite cells (asserted %.1e); %d cells raised"
          % (worst, finite, RS.ABS_REL_RTOL, nraised))
    assert finite >= 40 and nraised >= 10
    assert RS.ABS_REL_RTOL / 8 < worst <= RS.ABS_REL_RTOL / 4 * 1.001          # the asserted bound IS 4 x what is measured here


def test_fixture_holds_the_cases_the_rescaled_table_must_get_right():
    files = {(tag, rescale): (rows, got, want, raised) for tag, rescale, rows, got, want, raised in restated_cells()}
    # zero spread: a constant clipped prediction; the reference raises on every variant with a pixel, IEEE gives thresholds 0 and NaN
    rows, got, want, raised = files[("flat0", True)]
    assert raised[rows[:, 0] > 0].all() and np.isnan(rows[rows[:, 0] > 0][:, 2:8]).all() and (rows[:, 8:11] == 0).all()
    assert np.isnan(got[rows[:, 0] > 0][:, :7]).all() and (got[rows[:, 0] > 0][:, 7:] == 0).all()
    # an empty variant: ten NaN; a NaN target inside: thresholds 0 and NaN elsewhere, not raised
    rows, got, want, raised = files[("sim3", True)]
    assert (rows[7:, 0] == 0).all() and raised[7:].all() and np.isnan(got[7:]).all()
    rows, got, want, raised = files[("sim1", True)]
    assert not raised.any() and (rows[:, 1] < rows[:, 0]).all() and np.isnan(want[:, :7]).all() and (want[:, 7:] == 0).all()
    # odd and even counts among the finite cells, and the aligned medians
    fin = [(rows[v, 0], got[v]) for (tag, rs), (rows, got, want, raised) in files.items() if rs for v in range(len(rows)) if np.isfinite(got[v, 0])]
    assert {int(n) % 2 for n, _ in fin} == {0, 1}
    assert max(c[6] for _, c in fin) < 1e-6 and len(fin) >= 40
    # the resize: both factors hold NaN and finite targets, and the plain cells of the down-scaled files are finite where NaN is skipped
    for tag, s in RS.DOWN.items():
        rows, got, want, raised = files[(tag, False)]
        assert 0 < rows[0, 1] < rows[0, 0] == int(np.floor(R.H * s)) * int(np.floor(R.W * s)) and np.isfinite(want[0, 0]) and np.isnan(want[0, 3])


def test_resize_restatement_is_torchs_interpolate():
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(8)
    for shape in ((37, 53), (8, 8)):
        x = rng.random(shape) * 80
        x[rng.random(shape) < 0.2] = np.nan
        for s in (0.5, 0.25, 0.7):
            want = F.interpolate(torch.from_numpy(x)[None, None], scale_factor=s, mode="bilinear")[0, 0].numpy()
            got = RS.resize_bilinear(x, s)
            assert got.shape == want.shape == (int(np.floor(shape[0] * s)), int(np.floor(shape[1] * s)))
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any() and (np.isfinite(got).any() or got.size <= 4)
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def test_finish_eval_rows_on_hand_made_rescaled_rows():
    from rpg_ramnet_amd import metrics as M
    nan = np.nan
    rows = np.zeros((3, 2, 16))
    #              n_mask n   |d|/t  d2/t2 d2    ld2   |ld|  |d|   d1 d2 d3 med_t med_p
    rows[0, 0, :13] = [4, 4, 2.0, 1.0, 16.0, 4.0, 2.0, 8.0, 1, 2, 4, 1.5, 1.5]
    rows[1, 0, :13] = [2, 2, 4.0, 2.0, 2.0, 8.0, 2.0, 2.0, 0, 1, 2, 0.25, 0.75]
    rows[2, 0, :13] = [5, 3, nan, nan, nan, nan, nan, nan, 0, 0, 0, nan, nan]           # a NaN target inside
    rows[0, 1, :13] = [3, 3, nan, nan, nan, nan, nan, nan, 0, 0, 0, nan, nan]           # zero spread
    rows[1, 1, :13] = [0, 0, nan, nan, nan, nan, nan, nan, 0, 0, 0, nan, nan]           # empty
    rows[2, 1, :13] = [1, 1, nan, nan, nan, nan, nan, nan, 0, 0, 0, nan, nan]           # one pixel
    one = M.finish_eval_rows(rows[:1], (10,), False, skip_empty=False)
    assert one["abs_rel_diff"] == 0.5 and one["squ_rel_diff"] == 0.25 and one["RMS_linear"] == 2.0 and one["RMS_log"] == 1.0
    assert one["SILog"] == 0.75 and one["mean_depth_error"] == 2.0 and one["median_diff"] == 0.0
    assert [one["threshold_delta_1.25" + e] for e in ("", "^2", "^3")] == [0.25, 0.5, 1.0]
    assert np.isnan([one["10_" + k] for k in R.KEYS[:7]]).all() and [one["10_" + k] for k in R.KEYS[7:]] == [0.0, 0.0, 0.0]
    two = M.finish_eval_rows(rows[:2], (10,), False)
    assert two["abs_rel_diff"] == 1.25 and two["median_diff"] == 0.25 and two["files"] == 2
    assert np.isnan(two["10_abs_rel_diff"]) and two["10_threshold_delta_1.25"] == 0.0        # the empty file does not count, the flat one does
    ref = M.finish_eval_rows(rows, (10,), False, skip_empty=False)
    assert np.isnan(ref["abs_rel_diff"]) and ref["threshold_delta_1.25^3"] == (1.0 + 1.0 + 0.0) / 3 and np.isnan(ref["10_threshold_delta_1.25"])
    assert np.array_equal(M.eval_file_counts(rows), [3, 2])


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    from rpg_ramnet_amd import _hip
    L = _hip.lib()
    cut = (C.c_float * 8)(10, 20, 30, 80, 250, 500, 600, 700)
    ok = dict(pred=4096, target=4096, mask=None, G=1, npix=16, clip=80.0, reg=3.7, cut=cut, ncut=6, flags=1, ws=4096, out=4096)

    def call(**over):
        a = dict(ok, **over)
        return L.ramnet_eval_table_ex(a["pred"], a["target"], a["mask"], a["G"], a["npix"], a["clip"], a["reg"], a["cut"], a["ncut"], a["flags"],
                                      a["ws"], a["out"], None)

    assert call(flags=4) == 10001 and b"bad argument" in L.ramnet_last_error()
    assert call(flags=-1) == 10001 and call(flags=8) == 10001
    for flags in (0, 1, 2, 3):
        assert call(flags=flags, pred=None) == 10001 and call(flags=flags, ws=None) == 10001 and call(flags=flags, out=None) == 10001
        assert call(flags=flags, G=0) == 10001 and call(flags=flags, npix=0) == 10001 and call(flags=flags, ncut=9) == 10001
        assert call(flags=flags, ws=4100) == 10001 and call(flags=flags, clip=0.0) == 10001
        assert call(flags=flags, cut=(C.c_float * 8)(10, 30, 20, 80, 250, 500, 0, 0)) == 10001
    W = L.ramnet_eval_table_ex_workspace
    assert W(1, 16, 6, 0, 4) == 0 and W(1, 16, 6, 0, -1) == 0 and W(0, 16, 6, 0, 1) == 0 and W(1, 0, 6, 0, 1) == 0 and W(1, 16, 9, 0, 1) == 0
    assert W(9363, 16, 6, 0, 1) == 0 and W(9362, 16, 6, 0, 1) > 0
    for G, npix, ncut, has_mask in ((1, 16, 0, 0), (5, 37 * 53, 6, 1), (64, 260 * 346, 6, 1)):
        plain = L.ramnet_eval_table_workspace(G, npix, ncut, has_mask)
        assert W(G, npix, ncut, has_mask, 0) == W(G, npix, ncut, has_mask, 2) == plain          # flags = 0 is the plain table
        assert plain < W(G, npix, ncut, has_mask, 1) == W(G, npix, ncut, has_mask, 3) < plain + (plain >> 6) + 4096

    def resize(target=4096, G=1, Hh=8, Ww=8, s=0.5, clip=80.0, out=4096):
        return L.ramnet_resize_metric_target(target, G, Hh, Ww, s, clip, 3.7, out, None)

    assert resize(target=None) == 10001 and resize(out=None) == 10001 and resize(G=0) == 10001 and resize(G=65536) == 10001
    assert resize(Hh=0) == 10001 and resize(Ww=0) == 10001 and resize(Hh=1 << 16, Ww=1 << 15) == 10001 and resize(clip=0.0) == 10001
    assert resize(s=0.0) == 10001 and resize(s=-0.5) == 10001 and resize(s=1.5) == 10001 and resize(s=float("nan")) == 10001
    assert resize(s=0.1) == 10001                               # floor(8 * 0.1) = 0: no pixel left


def test_python_surface_rejects_bad_arguments_without_a_gpu():
    import torch
    from rpg_ramnet_amd import metrics as M
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            M.EvalTable(80.0, 3.7, down_scale_factor=bad)
        with pytest.raises(ValueError):
            M.resize_metric_target([torch.zeros(8, 8)], 80.0, 3.7, bad)
    tab = M.EvalTable(80.0, 3.7, rescale=True, down_scale_factor=0.5)
    assert tab.rescale is True and tab.down_scale_factor == 0.5 and M.EvalTable(80.0, 3.7).rescale is False
    with pytest.raises(ValueError, match="no CPU fallback"):
        M.resize_metric_target([torch.zeros(8, 8)], 80.0, 3.7, 0.5)
    with pytest.raises(ValueError, match="no CPU fallback"):
        tab.add([torch.zeros(4, 4)], [torch.zeros(8, 8)])
    assert M.resized_shape((37, 53), 0.7) == (25, 37) and M.resized_shape((1, 37, 53), 0.5) == (18, 26) and M.resized_shape((8, 8), 0.25) == (2, 2)
    assert (M.EVAL_RESCALE, M.EVAL_TARGET_METRIC) == (1, 2)


def test_header_and_binding_carry_the_new_entry_points():
    from rpg_ramnet_amd import _hip, metrics as M
    src = open(os.path.join(ROOT, "include", "ramnet_hip.h")).read()
    assert re.search(r"size_t\s+ramnet_eval_table_ex_workspace\(int G, size_t npix, int ncut, int has_mask, int flags\);", src)
    assert re.search(r"int\s+ramnet_eval_table_ex\(const float \*const \*pred, const float \*const \*target, const unsigned char \*const \*mask, int G,"
                     r"\s*size_t npix,\s*float clip_distance, float reg_factor, const float \*cutoffs, int ncut, int flags, void \*workspace,"
                     r"\s*double \*out,\s*void \*stream\);", src)
    assert re.search(r"int\s+ramnet_resize_metric_target\(const float \*const \*target, int G, int H, int W, double scale_factor, float clip_distance,"
                     r"\s*float reg_factor,\s*float \*out, void \*stream\);", src)
    assert re.search(r"#define\s+RAMNET_ABI_VERSION\s+27\b", src)
    for name, value in (("RAMNET_EVAL_RESCALE", M.EVAL_RESCALE), ("RAMNET_EVAL_TARGET_METRIC", M.EVAL_TARGET_METRIC)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, src)
        assert m and int(m.group(1)) == value
    for name in ("ramnet_eval_table_ex_workspace", "ramnet_eval_table_ex", "ramnet_resize_metric_target"):
        assert name in _hip.EXPORTS
    assert set(re.findall(r"\b(ramnet_[a-z0-9_]+)\(", src)) == set(_hip.EXPORTS)
    assert _hip.lib().ramnet_abi_version() == 27
