"""No GPU: the float64 restatement of the evaluation table's rows (tests/eval_table_restatement.py) and the host part of the table
(metrics.finish_eval_rows) against the REFERENCE's own cells (tests/golden/eval_table.npz: its add_to_metrics per file and variant, event
masks included) — the test that keeps the GPU tests of the HIP table honest —, the two aggregation rules, the argument checks of the
new entry points and their header / binding."""
import os
import re

import numpy as np

import eval_table_restatement as R
from util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated_rows():
    """{group: ([F, V, 16] rows from numpy's metric depths, [F, V, 10] reference cells)}"""
    out = {}
    for group, clip, reg, t_in, p_in, mask, cells, n_mask in R.golden_files(load_golden("eval_table.npz")):
        t, p = R.metric_depth_numpy(t_in, clip, reg), R.metric_depth_numpy(p_in, clip, reg, clamp=True)
        rows = R.restate_rows(t, p, mask)
        assert np.array_equal(rows[:, 0], n_mask), group
        out.setdefault(group, ([], []))
        out[group][0].append(rows), out[group][1].append(cells)
    return {g: (np.stack(r), np.stack(c)) for g, (r, c) in out.items()}


def test_restatement_and_host_part_meet_every_reference_cell():
    from rpg_ramnet_amd import metrics as M
    assert M.EVAL_KEYS == R.KEYS and M.EVAL_CUTOFFS == R.CUTOFFS and M.EVAL_ROW == R.ROW
    prefixes = M.eval_variant_prefixes(R.CUTOFFS, True)
    assert prefixes[:3] == ["", "10_", "20_"] and prefixes[7:9] == ["event_masked_", "event_masked_10_"] and len(prefixes) == 14
    worst = 0.0
    for group, (rows, cells) in restated_rows().items():
        for f in range(rows.shape[0]):                      # a table of one file: its averages ARE the file's cells
            res = M.finish_eval_rows(rows[f:f + 1], R.CUTOFFS, True, skip_empty=False)
            got = np.array([[res[pre + k] for k in R.KEYS] for pre in prefixes])
            R.check_cells(got, cells[f], (group, f))
            with np.errstate(all="ignore"):
                rel = np.abs(got - cells[f]) / np.abs(cells[f])
            worst = max(worst, float(np.nanmax(np.where(np.abs(cells[f]) > 1e-3, rel, 0.0))))
            assert res["files"] == 1
    print("largest relative difference restatement - reference over the cells above 1e-3: %.3e" % worst)


def test_fixture_holds_the_cases_the_table_must_get_right():
    cells = np.concatenate([c.reshape(-1, 10) for _, c in restated_rows().values()])
    rows = np.concatenate([r.reshape(-1, 16) for r, _ in restated_rows().values()])
    empty, nan_only = rows[:, 0] == 0, (rows[:, 0] > 0) & (rows[:, 1] == 0)
    assert empty.any() and np.isnan(cells[empty]).all()
    assert nan_only.any() and (cells[nan_only][:, 7:] == 0).all() and np.isnan(cells[nan_only][:, :7]).all()
    finite = np.isfinite(cells[:, 6])
    assert (rows[finite, 0] % 2 == 1).any() and (rows[finite, 0] % 2 == 0).any()
    assert (1 + len(R.CUTOFFS)) * 2 == 14 and (R.H * R.W) % 4 == 1
    # medians: np.median itself agrees with the sorted-middle rule of the restatement
    x = np.random.default_rng(0).random(1000).astype(np.float32)
    assert np.float32(np.median(x)) == R.median_f32(x) and np.float32(np.median(x[:999])) == R.median_f32(x[:999])


def test_aggregation_rules_and_file_counts():
    from rpg_ramnet_amd import metrics as M
    prefixes = M.eval_variant_prefixes(R.CUTOFFS, True)
    for group, (rows, cells) in restated_rows().items():
        F = rows.shape[0]
        want_counts = (rows[:, :, 1] > 0).sum(axis=0)
        assert np.array_equal(M.eval_file_counts(rows, skip_empty=True), want_counts)
        assert np.array_equal(M.eval_file_counts(rows, skip_empty=False), np.full(14, F))
        if group == "sim":       # file 3: nothing valid inside 10 / 20 / 30 m, an all-zero event mask
            assert want_counts.tolist() == [4, 3, 3, 3, 4, 4, 4, 3, 3, 3, 3, 3, 3, 3]
        else:                    # file 2: nothing inside 10 m
            assert want_counts.tolist() == [3, 2, 3, 3, 3, 3, 3, 3, 2, 3, 3, 3, 3, 3]
        ref = M.finish_eval_rows(rows, R.CUTOFFS, True, skip_empty=False)
        skip = M.finish_eval_rows(rows, R.CUTOFFS, True, skip_empty=True)
        assert ref["files"] == F and skip["files"] == F and len(ref) == 14 * 10 + 1
        for v, pre in enumerate(prefixes):
            for k, name in enumerate(R.KEYS):
                want = cells[:, v, k].sum() / F                      # the reference: sum / number of files, NaN propagating
                if np.isnan(want):
                    assert np.isnan(ref[pre + name]), (group, pre + name)
                else:
                    np.testing.assert_allclose(ref[pre + name], want, rtol=1e-4, atol=2e-5, err_msg=pre + name)
                keep = rows[:, v, 1] > 0
                want = cells[keep, v, k].sum() / keep.sum()
                if np.isnan(want):
                    assert np.isnan(skip[pre + name]), (group, pre + name)
                else:
                    np.testing.assert_allclose(skip[pre + name], want, rtol=1e-4, atol=2e-5, err_msg=pre + name)
    # a variant that no file counts for has no keys under skip_empty, NaN under the reference's rule
    rows = restated_rows()["sim"][0][3:4]
    assert "event_masked_abs_rel_diff" not in M.finish_eval_rows(rows, R.CUTOFFS, True)
    assert np.isnan(M.finish_eval_rows(rows, R.CUTOFFS, True, skip_empty=False)["event_masked_abs_rel_diff"])
    # without masks: the first seven variants alone
    res = M.finish_eval_rows(restated_rows()["mvsec"][0][:, :7], R.CUTOFFS, False)
    assert "500_median_diff" in res and not any(k.startswith("event_masked") for k in res)


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    import ctypes as C
    from rpg_ramnet_amd import _hip
    L = _hip.lib()
    cut = (C.c_float * 8)(10, 20, 30, 80, 250, 500, 600, 700)
    ok = dict(pred=4096, target=4096, mask=None, G=1, npix=16, clip=80.0, reg=3.7, cut=cut, ncut=6, ws=4096, out=4096)

    def call(**over):
        a = dict(ok, **over)
        return L.ramnet_eval_table(a["pred"], a["target"], a["mask"], a["G"], a["npix"], a["clip"], a["reg"], a["cut"], a["ncut"], a["ws"], a["out"], None)

    assert call(pred=None) == 10001 and b"bad argument" in L.ramnet_last_error()
    assert call(target=None) == 10001 and call(ws=None) == 10001 and call(out=None) == 10001
    assert call(G=0) == 10001 and call(G=-1) == 10001
    assert call(npix=0) == 10001 and call(npix=1 << 32) == 10001
    assert call(ncut=-1) == 10001 and call(ncut=9) == 10001 and call(cut=None) == 10001
    assert call(cut=(C.c_float * 8)(10, 30, 20, 80, 250, 500, 0, 0)) == 10001                  # not ascending
    assert call(cut=(C.c_float * 8)(10, 10, 20, 80, 250, 500, 0, 0)) == 10001
    assert call(cut=(C.c_float * 8)(0, 10, 20, 80, 250, 500, 0, 0)) == 10001                   # not positive
    assert call(cut=(C.c_float * 8)(float("nan"), 10, 20, 80, 250, 500, 0, 0)) == 10001
    assert call(ws=4100) == 10001                                                              # workspace not 256-byte aligned
    assert call(G=9363, ncut=6) == 10001 and call(G=4682, ncut=6, mask=4096) == 10001          # G * V beyond the 65536 tickets
    assert L.ramnet_metric_depth(None, 16, 80.0, 3.7, 0, 4096, None) == 10001
    assert L.ramnet_metric_depth(4096, 16, 80.0, 3.7, 0, None, None) == 10001
    assert L.ramnet_metric_depth(4096, 0, 80.0, 3.7, 1, 4096, None) == 10001
    assert L.ramnet_eval_table_workspace(0, 16, 6, 0) == 0 and L.ramnet_eval_table_workspace(1, 0, 6, 0) == 0
    assert L.ramnet_eval_table_workspace(1, 1 << 32, 6, 0) == 0 and L.ramnet_eval_table_workspace(1, 16, 9, 0) == 0
    assert L.ramnet_eval_table_workspace(9363, 16, 6, 0) == 0 and L.ramnet_eval_table_workspace(9362, 16, 6, 0) > 0
    small, big = L.ramnet_eval_table_workspace(1, 16, 0, 0), L.ramnet_eval_table_workspace(64, 260 * 346, 6, 1)
    assert 262144 < small < big < (128 << 20)


def test_header_and_binding_carry_the_new_entry_points():
    from rpg_ramnet_amd import _hip, build, metrics as M
    src = open(os.path.join(ROOT, "include", "ramnet_hip.h")).read()
    assert re.search(r"int\s+ramnet_metric_depth\(const float \*y, size_t n, float clip_distance, float reg_factor, int clamp, float \*out,"
                     r"\s*void \*stream\);", src)
    assert re.search(r"size_t\s+ramnet_eval_table_workspace\(int G, size_t npix, int ncut, int has_mask\);", src)
    assert re.search(r"int\s+ramnet_eval_table\(const float \*const \*pred, const float \*const \*target, const unsigned char \*const \*mask,", src)
    assert re.search(r"#define\s+RAMNET_ABI_VERSION\s+27\b", src)
    m = re.search(r"#define\s+RAMNET_EVAL_TABLE_TICKET_BYTES\s+(\d+)", src)
    assert m and int(m.group(1)) == M.EVAL_TICKET_BYTES
    for name in ("ramnet_metric_depth", "ramnet_eval_table_workspace", "ramnet_eval_table"):
        assert name in _hip.EXPORTS
    assert set(re.findall(r"\b(ramnet_[a-z0-9_]+)\(", src)) == set(_hip.EXPORTS)
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["metrics.hip"]            # (the table kernels live in metrics.hip)
    assert _hip.lib().ramnet_abi_version() == 27
