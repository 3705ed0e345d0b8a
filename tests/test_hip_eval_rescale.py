"""GPU: the rescaled evaluation table and the target resize (ramnet_eval_table_ex, ramnet_resize_metric_target; csrc/metrics.hip) and their
Python surface (metrics.EvalTable(rescale=, down_scale_factor=), metrics.resize_metric_target, inference.evaluate_table / stream_dataset)
against the float64 restatement fed the kernel's own float32 metric depths (tests/eval_rescale_restatement.py), against the reference's
cells (tests/golden/eval_rescale.npz) at the bounds of tests/test_eval_rescale_cpu.py, and against torch's F.interpolate on the CPU.

Measured on the MI355X (profiles/eval_rescale_notes.md): sums of the rescaled table against the restatement 2.2e-14 relative at most (bound
1e-10), medians of the transformed maps 3.3e-16; the resize against float64 F.interpolate 4.7e-8 of the largest tap at most (bound 1e-6)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import eval_rescale_restatement as RS
import eval_table_restatement as R
from util import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REL = 1e-10      # tests/test_hip_eval_table.py: kernel and restatement add the same float64 terms in different orders


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def direct(ps, ts, ms, clip, reg, cutoffs, flags, ws=None, ex=True):
    """One call of ramnet_eval_table_ex (ex=False: ramnet_eval_table) on a workspace of the caller's -> ([G, V, 16] rows, the workspace)."""
    from rpg_ramnet_amd import _hip as H, metrics as M
    L = H.lib()
    dp, dt = [to_dev(p) for p in ps], [to_dev(t) for t in ts]
    dm = None if ms is None else [None if m is None else to_dev(np.asarray(m).astype(np.uint8)) for m in ms]
    G, npix, has_mask = len(ps), int(ps[0].size), int(ms is not None)
    ptrs = [[x.data_ptr() for x in dp], [x.data_ptr() for x in dt], [0 if m is None else m.data_ptr() for m in (dm or [None] * G)]]
    tab = torch.tensor(ptrs, dtype=torch.int64).to(DEV)
    nbytes = L.ramnet_eval_table_ex_workspace(G, npix, len(cutoffs), has_mask, flags)
    assert nbytes > 0
    if ws is None:
        ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
        ws[:M.EVAL_TICKET_BYTES].zero_()
    assert ws.numel() >= nbytes
    V = (1 + len(cutoffs)) * (2 if has_mask else 1)
    out = torch.full((G, V, 16), -7.0, device=DEV, dtype=torch.float64)
    cut = (C.c_float * max(len(cutoffs), 1))(*[float(c) for c in cutoffs])
    a = (C.c_void_p(tab[0].data_ptr()), C.c_void_p(tab[1].data_ptr()), C.c_void_p(tab[2].data_ptr()) if has_mask else None, G, npix, clip, reg, cut,
         len(cutoffs))
    b = (C.c_void_p(ws.data_ptr()), C.c_void_p(out.data_ptr()), M._st())
    H.check(L.ramnet_eval_table_ex(*a, flags, *b) if ex else L.ramnet_eval_table(*a, *b), "ramnet_eval_table(_ex)")
    torch.cuda.synchronize()
    return out.cpu().numpy(), ws


def table_rows(ps, ts, ms, clip, reg, cutoffs, rescale=True, down=1.0):
    from rpg_ramnet_amd import metrics as M
    tab = M.EvalTable(clip, reg, cutoffs, rescale=rescale, down_scale_factor=down)
    rows = tab.add([to_dev(p) for p in ps], [to_dev(t) for t in ts], None if ms is None else [None if m is None else to_dev(m) for m in ms])
    V = (1 + len(cutoffs)) * (1 if ms is None else 2)
    assert rows.device.type == "cuda" and rows.dtype == torch.float64 and tuple(rows.shape) == (len(ps), V, 16)
    return rows.cpu().numpy()


def metric_maps(ps, ts, clip, reg):
    """The float32 metric depths that metric_depth returned: the kernel's own conversion."""
    from rpg_ramnet_amd import metrics as M
    return ([M.metric_depth(to_dev(p), clip, reg, clamp=True).cpu().numpy() for p in ps],
            [M.metric_depth(to_dev(t), clip, reg).cpu().numpy() for t in ts])


def restated(ps, ts, ms, clip, reg, cutoffs):
    pm, tm = metric_maps(ps, ts, clip, reg)
    return np.stack([RS.restate_rescaled_rows(tm[g], pm[g], None if ms is None else (np.ones(tm[g].shape, bool) if ms[g] is None else ms[g]), cutoffs)
                     for g in range(len(ps))])


def check_rows(got, want, tag):
    """Counts and threshold counts exact, sums and medians to REL, NaN exactly where the restatement has NaN, the spare columns zero."""
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.array_equal(got[..., :2], want[..., :2]), (tag, got[..., :2], want[..., :2])
    assert np.array_equal(got[..., 8:11], want[..., 8:11]), (tag, got[..., 8:11], want[..., 8:11])
    for name, cols in (("sum", slice(2, 8)), ("median", slice(11, 13))):
        g, w = got[..., cols], want[..., cols]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, name, g, w)
        ok = ~np.isnan(w)
        err = np.abs(g[ok] - w[ok])
        worst = float(np.max(err / np.maximum(np.abs(w[ok]), 1e-300))) if ok.any() else 0.0
        print("%s: largest relative difference of a %s %.3e over %d" % (tag, name, worst, int(ok.sum())))
        assert np.all(err <= REL * np.abs(w[ok])), (tag, name, worst)
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
    return RS.golden_files(load_golden("eval_rescale.npz"))


# ------------------------------------------------------------------------------------------------ (i) flags = 0 is the plain table
def test_flags_zero_rows_are_the_plain_table_byte_for_byte():
    for seed, G, shape, nan_frac, cutoffs, masks in ((1, 5, (37, 53), 0.1, R.CUTOFFS, True), (2, 1, (260, 346), 0.0, (30,), False), (3, 2, (3, 5), 0.0, (), True)):
        ps, ts, ms = seeded_pairs(seed, G, shape, nan_frac)
        ts[0] = np.where(np.isnan(ts[0]), np.float32(0.5), ts[0])
        ms = ms if masks else None
        plain, ws = direct(ps, ts, ms, 80.0, 3.70378, cutoffs, 0, ex=False)
        same, _ = direct(ps, ts, ms, 80.0, 3.70378, cutoffs, 0, ws=ws)
        assert same.tobytes() == plain.tobytes() and np.isfinite(plain[0, :, 11]).any() and not (plain == -7.0).any()
        # RAMNET_EVAL_TARGET_METRIC alone: the same rows from the metric targets
        pm, tm = metric_maps(ps, ts, 80.0, 3.70378)
        metric, _ = direct(ps, tm, ms, 80.0, 3.70378, cutoffs, 2, ws=ws)
        assert metric.tobytes() == plain.tobytes()


# ------------------------------------------------------------------------------------------------ (ii) kernel against restatement
CASES = {   # tag: (seed, G, shape, nan_frac, cut-offs, masks: None / "all" / "some" (NULL entries among them))
    "g1_37x53_no_masks": (1, 1, (37, 53), 0.0, R.CUTOFFS, None),
    "g5_37x53_some_masks_nan20": (2, 5, (37, 53), 0.2, R.CUTOFFS, "some"),
    "g5_37x53_all_masks": (3, 5, (37, 53), 0.0, R.CUTOFFS, "all"),
    "g1_37x53_all_masks_nan20_ncut1": (4, 1, (37, 53), 0.2, (20,), "all"),
}


@pytest.mark.parametrize("tag", list(CASES))
def test_rescaled_table_against_restatement(tag):
    seed, G, shape, nan_frac, cutoffs, masks = CASES[tag]
    ps, ts, ms = seeded_pairs(seed, G, shape, nan_frac)
    if nan_frac and G > 1:
        ts[0] = np.where(np.isnan(ts[0]), np.float32(0.5), ts[0])           # pair 0 keeps finite rows
    if nan_frac and G == 1:
        ms[0] &= ~np.isnan(ts[0])                                           # the masked half keeps clear of the NaN targets
    if masks is None:
        ms = None
    elif masks == "some":
        ms = [None if g % 2 == 0 else m for g, m in enumerate(ms)]
    clip, reg = 80.0, 3.70378
    got, want = table_rows(ps, ts, ms, clip, reg, cutoffs), restated(ps, ts, ms, clip, reg, cutoffs)
    check_rows(got, want, tag)
    assert np.isfinite(got[0, :, 2]).any() and np.isfinite(got[0, :, 11]).any()
    if nan_frac:
        assert np.isnan(got[..., 2]).any() and (got[np.isnan(got[..., 2])][:, 8:11] == 0).all()


def test_one_and_two_pixel_maps_constant_prediction_and_empty_variant():
    clip, reg, cutoffs = 80.0, 3.70378, (10, 40)
    for shape in ((1, 1), (1, 2)):                                              # zero spread / an even count of two
        ps, ts, _ = seeded_pairs(31, 3, shape)
        ps[2][:] = ps[2].flat[0]
        ts[2][:] = ts[2].flat[0]                                                # 1 x 2 with equal values: zero spread again
        if shape == (1, 2):
            ts[0][:], ps[0][:] = [[0.3, 0.6]], [[0.35, 0.5]]
        got, want = table_rows(ps, ts, None, clip, reg, cutoffs), restated(ps, ts, None, clip, reg, cutoffs)
        check_rows(got, want, "%dx%d" % shape)
        assert got[0, 0, 0] == shape[1] and np.isnan(got[2, 0, 2:8]).all() and (got[2, 0, 8:11] == 0).all()
        if shape == (1, 2):
            assert np.isfinite(got[0, 0, 2:8]).all() and abs(got[0, 0, 11] - got[0, 0, 12]) < 1e-12      # two distinct values per side: a finite row, medians aligned
        else:
            assert np.isnan(got[:, :, 2:8]).all()
    ps, ts, ms = seeded_pairs(32, 3, (37, 53))
    ps[0][:] = 0.4                                                              # a constant prediction: zero spread on one side only
    ps[1][:] = 1.5                                                              # ... and one that the clip makes constant
    ms[2][:] = False                                                            # an empty masked half
    ts[2] = (0.75 + 0.25 * ts[2]).astype(np.float32)                            # ... and nothing inside 10 m
    got, want = table_rows(ps, ts, ms, clip, reg, cutoffs), restated(ps, ts, ms, clip, reg, cutoffs)
    check_rows(got, want, "edge")
    assert (got[:2, :, 0] > 1).all() and np.isnan(got[:2, :, 2:8]).all() and (got[:2, :, 8:11] == 0).all()
    assert np.isfinite(got[0, :, 11]).all() and np.isnan(got[0, :, 12]).all()   # IEEE: the target side of file 0 keeps its median
    assert (got[2, 3:, 0] == 0).all() and got[2, 1, 0] == 0 and np.isnan(got[2, 3:, 2:8]).all() and np.isfinite(got[2, 0, 2:8]).all()
    from rpg_ramnet_amd import metrics as M
    res = M.finish_eval_rows(got[2:], cutoffs, True, skip_empty=False)
    assert np.isnan([res["event_masked_" + k] for k in R.KEYS]).all() and np.isfinite([res[k] for k in R.KEYS]).all()
    flat = M.finish_eval_rows(got[:1], cutoffs, True, skip_empty=False)
    assert np.isnan([flat[k] for k in R.KEYS[:7]]).all() and [flat[k] for k in R.KEYS[7:]] == [0.0, 0.0, 0.0]


def test_large_map_joins_across_workgroups():
    """260 x 346 with 15 % NaN targets: six workgroups per (map, variant) in all four passes.  The event mask keeps clear of the NaN targets, so
    the masked variants are rescaled from partial rows, slabs and tickets of six workgroups; odd and even counts among them."""
    ps, ts, ms = seeded_pairs(11, 1, (260, 346), 0.15)
    ms[0] &= ~np.isnan(ts[0])
    if len({int((ms[0] & (ts[0] < y)).sum()) % 2 for y in (0.4, 2.0)}) == 1:      # odd and even counts: drop one masked pixel beyond 30 m
        k = np.flatnonzero(ms[0] & (ts[0] > 0.8) & (ts[0] < 0.95))[0]
        ms[0].flat[k] = False
    got, want = table_rows(ps, ts, ms, 80.0, 3.70378, R.CUTOFFS), restated(ps, ts, ms, 80.0, 3.70378, R.CUTOFFS)
    check_rows(got, want, "260x346")
    assert np.isnan(got[0, :7, 2]).all() and np.isfinite(got[0, 7:, 2:13]).all() and got[0, 0, 0] == 260 * 346 > got[0, 0, 1]
    assert (got[0, 7:, 0] % 2 == 1).any() and (got[0, 7:, 0] % 2 == 0).any()


# ------------------------------------------------------------------------------------------------ (iii) against the reference
def test_table_meets_every_reference_cell(fixture_files):
    cells = 0
    for tag, clip, reg, s, t_in, p_in, mask, want, raised, n_mask in fixture_files:
        for rescale in sorted(want):
            rows = table_rows([p_in], [t_in], [mask], clip, reg, R.CUTOFFS, rescale=rescale, down=s)[0]
            assert np.array_equal(rows[:, 0], n_mask), (tag, rescale)
            got = RS.rows_to_cells(rows)
            if rescale:
                RS.check_rescaled_cells(got, want[True], raised[True], tag)
            else:
                R.check_cells(got, want[False], (tag, "plain"))
            cells += int((~raised[rescale]).sum())
    assert cells >= 89 + 28


# ------------------------------------------------------------------------------------------------ (iv) one workspace, no memset
def test_one_workspace_for_rescaled_and_plain_calls_without_memset():
    from rpg_ramnet_amd import metrics as M
    clip, reg = 80.0, 3.70378
    big = seeded_pairs(21, 5, (37, 53), 0.05)
    big[1][0] = np.where(np.isnan(big[1][0]), np.float32(0.25), big[1][0])
    first, ws = direct(*big, clip, reg, R.CUTOFFS, 1)
    a = seeded_pairs(22, 2, (3, 5))
    b = seeded_pairs(23, 3, (29, 31))
    ra, _ = direct(a[0], a[1], None, 1000.0, 5.70378, (), 0, ws=ws)                      # plain, on what the rescaled call left behind
    rb, _ = direct(b[0], b[1], b[2], clip, reg, (30,), 1, ws=ws)
    again, _ = direct(*big, clip, reg, R.CUTOFFS, 1, ws=ws)
    assert again.tobytes() == first.tobytes()
    assert int(ws[:M.EVAL_TICKET_BYTES].count_nonzero()) == 0                            # every ticket is back at zero
    check_rows(first, restated(*big, clip, reg, R.CUTOFFS), "reuse first")
    check_rows(rb, restated(b[0], b[1], b[2], clip, reg, (30,)), "reuse b")
    pm, tm = metric_maps(a[0], a[1], 1000.0, 5.70378)
    plain = np.stack([R.restate_rows(tm[g], pm[g], None, ()) for g in range(2)])
    assert np.array_equal(ra[..., :2], plain[..., :2]) and np.array_equal(ra[..., 8:11], plain[..., 8:11])
    np.testing.assert_allclose(ra[..., 2:8], plain[..., 2:8], rtol=REL, atol=0)
    assert ra[..., 11:13].astype(np.float32).tobytes() == plain[..., 11:13].astype(np.float32).tobytes() and not (ra == -7.0).any()


# ------------------------------------------------------------------------------------------------ (v) the target resize
@pytest.mark.parametrize("shape", [(37, 53), (8, 8)])
def test_resize_metric_target_against_interpolate(shape):
    import torch.nn.functional as F
    from rpg_ramnet_amd import metrics as M
    clip, reg = 80.0, 3.70378
    rng = np.random.default_rng(9)
    ts = rng.random((3,) + shape).astype(np.float32)
    ts[1][rng.random(shape) < 0.2] = np.nan
    ts[2][0, 0] = np.nan
    dev = to_dev(ts)
    md = M.metric_depth(dev, clip, reg).cpu().double()                          # the kernel's own metric depths
    for s in (0.5, 0.25, 0.7):
        got = M.resize_metric_target(dev, clip, reg, s)
        want = F.interpolate(md[:, None], scale_factor=s, mode="bilinear")[:, 0].numpy()
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (3, int(np.floor(shape[0] * s)), int(np.floor(shape[1] * s)))
        got = got.cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[1]).any() and np.isfinite(got[0]).all()
        worst = 0.0
        for g in range(3):
            bound = 1e-6 * RS.resize_largest_tap(md[g].numpy(), s)
            ok = ~np.isnan(want[g])
            assert np.all(np.abs(got[g] - want[g])[ok] <= bound[ok]), (shape, s, g, float(np.max((np.abs(got[g] - want[g]) / bound)[ok])))
            worst = max(worst, float(np.max((np.abs(got[g] - want[g]) / bound)[ok]) * 1e-6))
        print("resize %s x %.2f: %.3e of the largest tap at most" % (shape, s, worst))
        one = M.resize_metric_target([dev[1]], clip, reg, s)                    # a list of maps: the same bits
        assert one[0].cpu().numpy().tobytes() == M.resize_metric_target(dev, clip, reg, s)[1].cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ (vi) drivers, end to end
def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def test_drivers_end_to_end(tmp_path):
    from recipe import FOLDERS, make_dataset_dir
    from rpg_ramnet_amd import _hip, data as D, inference, metrics as M
    from util import build_hip_model, ref_cfg
    clip, reg, K = 1000.0, 5.70378, 3
    root = make_dataset_dir(str(tmp_path / "data"), n_seq=2, n_frames=15, H=32, W=48)
    for f in glob.glob(os.path.join(root, "*", "depth", "data", "*.npy")):      # NaN-free ground truth: a NaN inside makes a rescaled row NaN
        d = np.load(f)
        np.save(f, np.where(np.isnan(d), np.float32(500.0), d))
    ds = D.concatenate_subfolders(root, "SequenceSynchronizedFramesEventsDataset", sequence_length=1, step_size=1, transform=D.CenterCrop(32),
                                  clip_distance=clip, every_x_rgb_frame=K, reg_factor=reg, dataset_idx_flag=True, **FOLDERS)
    cfg, _ = ref_cfg("net_seeded_ramnet.npz", every_x_rgb_frame=K)
    model = build_hip_model("ERGB2DepthRecurrent", cfg)
    out = str(tmp_path / "out")
    live = inference.stream_dataset(model, ds, K, output_folder=out, reg_factor=reg, clip_distance=clip, table=True, rescale=True)
    keys = ["events%d" % k for k in range(K)] + ["image"]
    assert sorted(live["tables"]) == sorted(keys) and all(t.rescale for t in live["tables"].values()) and live["saved"] > 0

    # stream_dataset(table=True, rescale=True) == evaluate_table(rescale=True) over what the same run wrote
    for key in keys:
        pd, td = os.path.join(out, "npy", key), os.path.join(out, "ground_truth/npy", "depth_" + key)
        res = inference.evaluate_table(pd, td, clip, reg, batch_files=5, rescale=True)
        got = live["tables"][key].result()
        assert len(live["tables"][key]) == live["saved"] == res["files"]
        assert sorted(got) == sorted(res) and all(_same(got[k], res[k]) for k in res), key

    # evaluate_table(rescale=True) == an EvalTable(rescale=True) fed the same files; and it is not the plain table
    pd, td = os.path.join(out, "npy", "image"), os.path.join(out, "ground_truth/npy", "depth_image")
    names = sorted(os.listdir(pd))
    ps = [np.load(os.path.join(pd, n))[0] for n in names]
    ts = [np.load(os.path.join(td, n.replace("depth_", "frame_")))[0] for n in names]
    res = inference.evaluate_table(pd, td, clip, reg, crop_ymax=30, batch_files=7, rescale=True)
    tab = M.EvalTable(clip, reg, rescale=True)
    tab.add([to_dev(p[:30]) for p in ps], [to_dev(t[:30]) for t in ts])
    want = tab.result()
    assert sorted(res) == sorted(want) and all(_same(res[k], want[k]) for k in want) and res["files"] == len(names)
    plain = inference.evaluate_table(pd, td, clip, reg, crop_ymax=30, batch_files=7)
    assert np.isfinite(res["abs_rel_diff"]) and res["abs_rel_diff"] != plain["abs_rel_diff"] and res["median_diff"] < 1e-6 < plain["median_diff"]
    check_rows(tab.rows().cpu().numpy(), restated([p[:30] for p in ps], [t[:30] for t in ts], None, clip, reg, R.CUTOFFS), "driver rows")

    # --down_scale_factor 0.5: predictions at 16 x 24 against the targets of the run, with and without rescaling
    small = str(tmp_path / "small")
    os.makedirs(small)
    for n, p in zip(names, ps):
        np.save(os.path.join(small, n), p[None, ::2, ::2])
    for rescale in (False, True):
        res = inference.evaluate_table(small, td, clip, reg, batch_files=4, rescale=rescale, down_scale_factor=0.5)
        tab = M.EvalTable(clip, reg, rescale=rescale, down_scale_factor=0.5)
        rows = tab.add([to_dev(p[::2, ::2]) for p in ps], [to_dev(t) for t in ts])
        want = tab.result()
        assert sorted(res) == sorted(want) and all(_same(res[k], want[k]) for k in want) and np.isfinite(res["abs_rel_diff"])
        tm = M.resize_metric_target(to_dev(np.stack(ts)), clip, reg, 0.5).cpu().numpy()
        pm = [M.metric_depth(to_dev(p[::2, ::2]), clip, reg, clamp=True).cpu().numpy() for p in ps]
        restate = RS.restate_rescaled_rows if rescale else R.restate_rows
        want_rows = np.stack([restate(tm[g], pm[g], None, R.CUTOFFS) for g in range(len(ps))])
        got_rows = rows.cpu().numpy()
        assert np.array_equal(got_rows[..., :2], want_rows[..., :2]) and np.array_equal(got_rows[..., 8:11], want_rows[..., 8:11])
        ok = ~np.isnan(want_rows[..., 2:8])
        assert np.array_equal(np.isnan(got_rows[..., 2:8]), ~ok)
        assert np.all(np.abs(got_rows[..., 2:8] - want_rows[..., 2:8])[ok] <= REL * np.abs(want_rows[..., 2:8])[ok])

    # masks of the targets' size: refused before anything is launched
    calls = []
    _hip.set_tracer(lambda name, fn, a: (calls.append(name), fn(*a))[1])
    try:
        tab = M.EvalTable(clip, reg, down_scale_factor=0.5)
        with pytest.raises(ValueError, match="masks must have the size of the predictions"):
            tab.add([to_dev(p[::2, ::2]) for p in ps[:2]], [to_dev(t) for t in ts[:2]], [to_dev(np.ones(ts[0].shape, bool))] * 2)
        other = M.EvalTable(clip, reg, rescale=True, down_scale_factor=0.5)
        with pytest.raises(ValueError, match="targets must resize"):
            other.add([to_dev(p) for p in ps[:2]], [to_dev(t) for t in ts[:2]])
    finally:
        _hip.set_tracer(None)
    assert calls == [] and len(tab._chunks) == 0 and len(other._chunks) == 0
