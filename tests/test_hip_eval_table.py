"""GPU: ramnet_metric_depth / ramnet_eval_table (csrc/metrics.hip) and their Python surface (metrics.metric_depth, metrics.EvalTable,
inference.evaluate_table, inference.stream_dataset(table=...)) against the float64 restatement fed the kernel's own float32 metric depths
(tests/eval_table_restatement.py), against the reference's cells (tests/golden/eval_table.npz) at the bound of
tests/test_eval_table_cpu.py, and against the existing per-pair path metrics.depth_metrics / inference.evaluate_folders.

Measured on the MI355X (profiles/eval_table_notes.md): metric_depth against float64 exp 5.3e-7 relative at most (bound 1e-6); sums of the
kernel against the restatement 4.2e-16 relative at most (bound 1e-10); sums-based entries against depth_metrics 9.5e-16 relative at
most (bound 1e-9); median_diff against depth_metrics 0 ulp apart on all 45 cells of the fixture (bound 4 ulp)."""
import os

import numpy as np
import pytest
import torch

import eval_table_restatement as R
from util import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# Kernel and restatement add the SAME float64 terms in different orders: at most 9e4 additions per cell (260 x 346), 9e4 x 1.1e-16 ~ 1e-11:
# the argument and the value of REL in tests/test_hip_train_metrics.py.
REL = 1e-10
# finish_eval_rows against depth_metrics: the same element arithmetic, another addition order, and possibly a double FMA in loss_voxel.hip
PER_PAIR_REL = 1e-9


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def table_rows(ps, ts, ms, clip, reg, cutoffs):
    from rpg_ramnet_amd import metrics as M
    tab = M.EvalTable(clip, reg, cutoffs)
    rows = tab.add([to_dev(p) for p in ps], [to_dev(t) for t in ts], None if ms is None else [None if m is None else to_dev(m) for m in ms])
    V = (1 + len(cutoffs)) * (1 if ms is None else 2)
    assert rows.device.type == "cuda" and rows.dtype == torch.float64 and tuple(rows.shape) == (len(ps), V, 16)
    assert tab.rows().data_ptr() == rows.data_ptr() and len(tab) == len(ps)
    return rows.cpu().numpy()


def restated(ps, ts, ms, clip, reg, cutoffs):
    """The restatement on the float32 maps that metric_depth returned: the kernel's own conversion."""
    from rpg_ramnet_amd import metrics as M
    out = []
    for g in range(len(ps)):
        t = M.metric_depth(to_dev(ts[g]), clip, reg).cpu().numpy()
        p = M.metric_depth(to_dev(ps[g]), clip, reg, clamp=True).cpu().numpy()
        m = None if ms is None else (np.ones(t.shape, bool) if ms[g] is None else ms[g])
        out.append(R.restate_rows(t, p, m, cutoffs))
    return np.stack(out)


def check_rows(got, want, tag):
    """Counts exact, sums to REL, medians bit-equal as float32, NaN where the restatement has NaN, the spare columns zero."""
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.array_equal(got[..., :2], want[..., :2]), (tag, got[..., :2], want[..., :2])
    assert np.array_equal(got[..., 8:11], want[..., 8:11]), (tag, got[..., 8:11], want[..., 8:11])
    err = np.abs(got[..., 2:8] - want[..., 2:8])
    worst = float(np.max(err / np.maximum(np.abs(want[..., 2:8]), 1e-300)))
    print("%s: largest relative difference of a sum %.3e" % (tag, worst))
    assert np.all(err <= REL * np.abs(want[..., 2:8])), (tag, worst)
    gm, wm = got[..., 11:13], want[..., 11:13]
    assert np.array_equal(np.isnan(gm), np.isnan(wm)), (tag, gm, wm)
    assert gm.astype(np.float32).tobytes() == wm.astype(np.float32).tobytes(), (tag, gm, wm)
    assert np.array_equal(gm[~np.isnan(gm)], gm[~np.isnan(gm)].astype(np.float32).astype(np.float64))
    assert np.all(got[..., 13:] == 0)


def seeded_pairs(seed, G, shape, nan_frac=0.0):
    rng = np.random.default_rng(seed)
    ps, ts, ms = [], [], []
    for _ in range(G):
        t = rng.random(shape).astype(np.float32)
        p = (t + 0.1 * rng.standard_normal(shape)).astype(np.float32)            # (some predictions leave [0, 1]: clipped)
        if nan_frac:
            t[rng.random(shape) < nan_frac] = np.nan
        ps.append(p), ts.append(t), ms.append(rng.random(shape) < 0.3)
    return ps, ts, ms


@pytest.fixture(scope="module")
def fixture_files():
    return R.golden_files(load_golden("eval_table.npz"))


# ------------------------------------------------------------------------------------------------ metric_depth
def test_metric_depth_against_float64_exp_clamp_bounds_and_nan():
    from rpg_ramnet_amd import metrics as M
    rng = np.random.default_rng(5)
    worst = 0.0
    for clip, reg, n in ((80.0, 3.70378, 37 * 53), (1000.0, 5.70378, 1200003)):       # the larger one: more pixels than threads in the grid
        y = rng.random(n).astype(np.float32)
        y[:4] = [0.0, 1.0, 0.5, np.float32(1e-3)]
        got = M.metric_depth(to_dev(y), clip, reg).cpu().numpy()
        want = np.exp(np.float64(np.float32(reg)) * (y.astype(np.float64) - 1.0)) * clip
        rel = float(np.max(np.abs(got - want) / want))
        worst = max(worst, rel)
        assert got.dtype == np.float32 and got.shape == y.shape
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
        assert np.array_equal(M.metric_depth(to_dev(y), clip, reg, clamp=True).cpu().numpy(), got)          # inside the bounds: untouched
        z = np.array([-3.0, -0.25, 0.0, 0.25, 1.0, 1.25, 40.0, np.nan, -np.inf, np.inf], np.float32)
        free = M.metric_depth(to_dev(z), clip, reg).cpu().numpy()
        held = M.metric_depth(to_dev(z), clip, reg, clamp=True).cpu().numpy()
        lo = free[2]                                       # y = 0 IS exp(-reg) * clip
        np.testing.assert_allclose(lo, np.exp(-np.float64(np.float32(reg))) * clip, rtol=1e-6)
        assert np.isnan(held[7]) and np.delete(held, 7).tobytes() == np.array([lo, lo, lo, free[3], clip, clip, clip, lo, clip], np.float32).tobytes()
        assert np.isnan(free[7]) and free[8] == 0.0 and np.isinf(free[9]) and free[4] == np.float32(clip)
    print("metric_depth: largest relative difference to float64 exp %.3e" % worst)
    out = M.metric_depth(torch.rand(2, 1, 5, 7, device=DEV), 80.0, 3.70378)
    assert tuple(out.shape) == (2, 1, 5, 7) and out.dtype == torch.float32
    with pytest.raises(ValueError):
        M.metric_depth(torch.rand(4), 80.0, 3.70378)


# ------------------------------------------------------------------------------------------------ kernel against restatement
CASES = {   # tag: (seed, G, shape, nan_frac, cut-offs, masks: None / "all" / "some" (NULL entries among them))
    "g1_37x53_ncut6_masks": (1, 1, (37, 53), 0.0, R.CUTOFFS, "all"),
    "g7_37x53_ncut6_some_null_masks": (2, 7, (37, 53), 0.1, R.CUTOFFS, "some"),
    "g2_3x5_ncut1": (3, 2, (3, 5), 0.0, (40,), None),
    "g3_37x53_ncut0": (4, 3, (37, 53), 0.0, (), None),
    "g2_3x5_ncut0_masks": (6, 2, (3, 5), 0.2, (), "all"),
    "g3_37x53_ncut1_masks": (7, 3, (37, 53), 0.0, (20,), "some"),
}


@pytest.mark.parametrize("tag", list(CASES))
def test_table_against_restatement(tag):
    seed, G, shape, nan_frac, cutoffs, masks = CASES[tag]
    ps, ts, ms = seeded_pairs(seed, G, shape, nan_frac)
    if nan_frac and G > 1:
        ts[0] = np.where(np.isnan(ts[0]), np.float32(0.5), ts[0])           # pair 0 keeps finite medians
    if masks is None:
        ms = None
    elif masks == "some":
        ms = [None if g % 2 == 0 else m for g, m in enumerate(ms)]
    clip, reg = 80.0, 3.70378
    got, want = table_rows(ps, ts, ms, clip, reg, cutoffs), restated(ps, ts, ms, clip, reg, cutoffs)
    check_rows(got, want, tag)
    assert np.isfinite(got[0, :, 11]).any()


def test_large_map_joins_across_workgroups():
    """260 x 346 with 15 % NaN targets: six workgroups per (map, variant): partial rows, slabs and tickets.  The event mask keeps clear of
    the NaN targets, so the masked variants have medians that are selected across the workgroups."""
    ps, ts, ms = seeded_pairs(11, 1, (260, 346), 0.15)
    ms[0] &= ~np.isnan(ts[0])
    if len({int((ms[0] & (ts[0] < y)).sum()) % 2 for y in (0.4, 2.0)}) == 1:      # odd and even counts: drop one masked pixel beyond 30 m
        k = np.flatnonzero(ms[0] & (ts[0] > 0.8) & (ts[0] < 0.95))[0]
        ms[0].flat[k] = False
    got, want = table_rows(ps, ts, ms, 80.0, 3.70378, R.CUTOFFS), restated(ps, ts, ms, 80.0, 3.70378, R.CUTOFFS)
    check_rows(got, want, "260x346")
    assert np.isnan(got[0, :7, 11]).all() and np.isfinite(got[0, 7:, 11]).all() and got[0, 0, 0] == 260 * 346 > got[0, 0, 1]
    assert (got[0, 7:, 0] % 2 == 1).any() and (got[0, 7:, 0] % 2 == 0).any()


def test_one_pixel_empty_and_nan_only_variants():
    ps, ts, ms = seeded_pairs(12, 2, (37, 53))
    clip, reg = 80.0, 3.70378
    ts[0] = (0.75 + 0.25 * ts[0]).astype(np.float32)                   # beyond 30 m ...
    ts[0][5, 7] = 0.1                                                   # ... but one pixel at 3 m
    ts[0][9, 9] = np.nan
    ms[0][:] = False
    ms[0][20, 31] = True                                                # a one-pixel event mask
    ts[1] = (0.75 + 0.25 * ts[1]).astype(np.float32)
    ts[1][::5, ::3] = np.nan                                            # 10 m: NaN targets only
    ms[1][:] = False                                                    # an empty mask
    cutoffs = (5, 10)
    got, want = table_rows(ps, ts, ms, clip, reg, cutoffs), restated(ps, ts, ms, clip, reg, cutoffs)
    check_rows(got, want, "edge")
    assert got[0, 1, 0] == 2 and got[0, 1, 1] == 1 and np.isnan(got[0, 1, 11])            # the pixel and the NaN
    assert got[0, 3, 0] == 1 and got[0, 3, 1] == 1 and np.isfinite(got[0, 3, 11:13]).all() and (got[0, 4:, 0] == 0).all()
    assert got[1, 1, 0] > 0 and got[1, 1, 1] == 0 and (got[1, 3:, 0] == 0).all()
    from rpg_ramnet_amd import metrics as M
    res = M.finish_eval_rows(got[1:2], cutoffs, True, skip_empty=False)
    assert res["5_threshold_delta_1.25"] == 0.0 and np.isnan(res["5_abs_rel_diff"]) and np.isnan(res["event_masked_threshold_delta_1.25"])
    one = M.finish_eval_rows(got[0:1], cutoffs, True)
    assert np.isfinite([one["event_masked_" + k] for k in R.KEYS]).all()
    ts[0][9, 9] = 0.9
    got = table_rows(ps[:1], ts[:1], None, clip, reg, cutoffs)
    check_rows(got, restated(ps[:1], ts[:1], None, clip, reg, cutoffs), "one pixel")
    assert got[0, 1, 0] == 1 and got[0, 1, 11] == np.float64(np.float32(got[0, 1, 11])) and abs(got[0, 1, 11] - 80 * np.exp(-0.9 * 3.70378)) < 1e-4


def test_workspace_reuse_without_memset_and_bit_reproducibility():
    from rpg_ramnet_amd import metrics as M
    big = seeded_pairs(21, 7, (37, 53), 0.05)
    big[1][0] = np.where(np.isnan(big[1][0]), np.float32(0.25), big[1][0])
    first = table_rows(*big, 80.0, 3.70378, R.CUTOFFS)
    key = (0, M._st().value or 0)
    ws = M._eval_workspaces[key]
    a = seeded_pairs(22, 1, (3, 5))
    b = seeded_pairs(23, 3, (37, 53))
    ra = table_rows(a[0], a[1], None, 1000.0, 5.70378, ())
    rb = table_rows(b[0], b[1], b[2], 80.0, 3.70378, (30,))
    again = table_rows(*big, 80.0, 3.70378, R.CUTOFFS)
    assert M._eval_workspaces[key] is ws                       # one allocation, zeroed once
    assert again.tobytes() == first.tobytes()
    check_rows(ra, restated(a[0], a[1], None, 1000.0, 5.70378, ()), "reuse a")
    check_rows(rb, restated(b[0], b[1], b[2], 80.0, 3.70378, (30,)), "reuse b")
    check_rows(first, restated(*big, 80.0, 3.70378, R.CUTOFFS), "reuse first")
    assert int(ws[:M.EVAL_TICKET_BYTES].count_nonzero()) == 0  # every ticket is back at zero


# ------------------------------------------------------------------------------------------------ against the reference and the per-pair path
def test_table_meets_every_reference_cell_and_the_restatement(fixture_files):
    from rpg_ramnet_amd import metrics as M
    prefixes = M.eval_variant_prefixes(R.CUTOFFS, True)
    for group, (clip, reg, nfiles) in R.GROUPS.items():
        files = [f for f in fixture_files if f[0] == group]
        ps, ts, ms = [f[4] for f in files], [f[3] for f in files], [f[5] for f in files]
        tab = M.EvalTable(clip, reg)
        tab.add(to_dev(np.stack(ps))[:, None], to_dev(np.stack(ts))[:, None], to_dev(np.stack(ms)))         # [G, 1, H, W] tensors, bool masks
        rows = tab.rows().cpu().numpy()
        check_rows(rows, restated(ps, ts, ms, clip, reg, R.CUTOFFS), group)
        for f in range(nfiles):
            res = M.finish_eval_rows(rows[f:f + 1], R.CUTOFFS, True, skip_empty=False)
            R.check_cells(np.array([[res[pre + k] for k in R.KEYS] for pre in prefixes]), files[f][6], (group, f))
        assert tab.result(skip_empty=False)["files"] == nfiles


def test_table_equals_the_per_pair_depth_metrics(fixture_files):
    from rpg_ramnet_amd import metrics as M
    prefixes = M.eval_variant_prefixes(R.CUTOFFS, False)
    worst_sum, worst_ulps, cells = 0.0, 0.0, 0
    for group, clip, reg, t_in, p_in, mask, _, _ in fixture_files:
        pt, tt = to_dev(p_in), to_dev(t_in)
        tab = M.EvalTable(clip, reg)
        rows = tab.add([pt], [tt]).cpu().numpy()
        for v, pre in enumerate(prefixes):
            want = M.depth_metrics(pt, tt, clip, reg, cutoff=float("inf") if v == 0 else float(R.CUTOFFS[v - 1]))
            if want.get("n", 0) == 0:
                assert rows[0, v, 1] == 0
                continue
            got = M.finish_eval_rows(rows[:, v:v + 1], (), False)
            assert rows[0, v, 1] == want["n"]
            for k in R.KEYS:
                if np.isnan(want[k]):
                    assert np.isnan(got[k]), (group, pre, k)
                elif k == "median_diff":
                    bound = 4 * np.spacing(np.float32(max(rows[0, v, 11], rows[0, v, 12])))
                    worst_ulps = max(worst_ulps, abs(got[k] - want[k]) / float(np.spacing(np.float32(max(rows[0, v, 11], rows[0, v, 12])))))
                    assert abs(got[k] - want[k]) <= bound, (group, pre, got[k], want[k], bound)
                else:
                    worst_sum = max(worst_sum, abs(got[k] - want[k]) / max(abs(want[k]), 1e-300))
                    assert abs(got[k] - want[k]) <= PER_PAIR_REL * abs(want[k]), (group, pre, k, got[k], want[k])
            cells += 1
    assert cells >= 40
    print("against depth_metrics over %d cells: sums-based entries %.3e relative, median_diff %.2f ulp of the larger median" % (cells, worst_sum, worst_ulps))


# ------------------------------------------------------------------------------------------------ drivers, end to end
def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def test_drivers_end_to_end(tmp_path):
    from PIL import Image
    from recipe import FOLDERS, make_dataset_dir
    from rpg_ramnet_amd import data as D, inference, metrics as M
    from util import build_hip_model, ref_cfg
    clip, reg, K = 1000.0, 5.70378, 3
    root = make_dataset_dir(str(tmp_path / "data"), n_seq=2, n_frames=15, H=32, W=48)
    ds = D.concatenate_subfolders(root, "SequenceSynchronizedFramesEventsDataset", sequence_length=1, step_size=1, transform=D.CenterCrop(32),
                                  clip_distance=clip, every_x_rgb_frame=K, reg_factor=reg, dataset_idx_flag=True, **FOLDERS)
    cfg, _ = ref_cfg("net_seeded_ramnet.npz", every_x_rgb_frame=K)
    model = build_hip_model("ERGB2DepthRecurrent", cfg)
    out = str(tmp_path / "out")
    info = inference.stream_dataset(model, ds, K, output_folder=out, reg_factor=reg, clip_distance=clip)
    assert "tables" not in info
    keys = ["events%d" % k for k in range(K)] + ["image"]

    # the table straight from the stream, no folder
    live = inference.stream_dataset(model, ds, K, reg_factor=reg, clip_distance=clip, table=True)
    assert live["saved"] == 0 and sorted(live["tables"]) == sorted(keys)
    for key in keys:
        pd, td = os.path.join(out, "npy", key), os.path.join(out, "ground_truth/npy", "depth_" + key)
        res = inference.evaluate_table(pd, td, clip, reg, batch_files=5)
        assert len(live["tables"][key]) == info["saved"] == res["files"]
        got = live["tables"][key].result()
        assert sorted(got) == sorted(res) and all(_same(got[k], res[k]) for k in res), key       # the same rows: the same predictions, bit for bit
    # ... and it leaves what the run writes alone
    part = str(tmp_path / "out_table")
    inference.stream_dataset(model, ds, K, output_folder=part, reg_factor=reg, clip_distance=clip, max_items=5, table={"image": M.EvalTable(clip, reg)})
    for name in sorted(os.listdir(os.path.join(part, "npy", "image"))):
        assert np.array_equal(np.load(os.path.join(part, "npy", "image", name)), np.load(os.path.join(out, "npy", "image", name))), name

    # evaluate_table without masks == evaluate_folders, key for key
    pd, td = os.path.join(out, "npy", "image"), os.path.join(out, "ground_truth/npy", "depth_image")
    old = inference.evaluate_folders(pd, td, clip_distance=clip, reg_factor=reg)
    new = inference.evaluate_table(pd, td, clip, reg, batch_files=7)
    assert sorted(old) == sorted(new) and old["files"] == new["files"]
    names = sorted(os.listdir(pd))
    ps = [np.load(os.path.join(pd, n))[0] for n in names]
    ts = [np.load(os.path.join(td, n.replace("depth_", "frame_")))[0] for n in names]
    for k, v in old.items():
        if np.isnan(v):
            assert np.isnan(new[k]), k
        elif k.endswith("median_diff"):
            assert abs(new[k] - v) <= 4 * np.spacing(np.float32(clip)), (k, new[k], v)           # (no median is larger than clip_distance)
        else:
            assert abs(new[k] - v) <= PER_PAIR_REL * abs(v), (k, new[k], v)

    # event frames as PNG: the event_masked_* keys against the restatement; rows [:30] of the maps only
    ed = str(tmp_path / "event_frames")
    os.makedirs(ed)
    rng = np.random.default_rng(3)
    frames = []
    for i in range(len(names) + 1):
        f = (rng.random((32, 32, 3)) < 0.12).astype(np.uint8) * rng.integers(1, 255, (32, 32, 3), dtype=np.uint8)
        if i == 2:
            f[:] = 0
        frames.append(f)
        Image.fromarray(f).save(os.path.join(ed, "events_%04d.png" % i))
    res = inference.evaluate_table(pd, td, clip, reg, crop_ymax=30, prediction_offset=1, target_offset=1, event_masks_dir=ed, batch_files=64)
    ms = [f[:30].astype("float32").sum(-1) > 0 for f in frames[1:len(names)]]
    want_rows = restated([p[:30] for p in ps[1:]], [t[:30] for t in ts[1:]], ms, clip, reg, R.CUTOFFS)
    want = M.finish_eval_rows(want_rows, R.CUTOFFS, True)
    assert res["files"] == len(names) - 1 and sorted(res) == sorted(want) and any(k.startswith("event_masked_") for k in res)
    for k, v in want.items():
        if np.isnan(v):
            assert np.isnan(res[k]), k
        else:
            assert abs(res[k] - v) <= PER_PAIR_REL * abs(v), (k, res[k], v)
