"""GPU: ramnet_render_depth / ramnet_render_inputs / ramnet_least_squares_scale (csrc/render.hip) and their Python surface
(rpg_ramnet_amd.render, inference.stream_dataset(images=, calculate_scale="device", metrics=)) against the numpy statement
tests/render_restatement.py — bit for bit for every image — and the reference's colour maps (tests/golden/render.npz).

Every uint8 output of the raw calls sits between 256 guard bytes of 0xA5 on either side, which must stay.

Bounds of the scale (derived, not measured; profiles/render_notes.md holds what was measured):
  against the float64 sum of the float32 products of metrics.metric_depth's own outputs: n * 2^-52 relative — the same positive terms,
  only the order of the float64 additions differs (two sums of n terms, each within (n - 1) * 2^-53 of the exact sum);
  against numpy's float32 statement of test.py:365-378: 64 * 2^-24 relative — a pairwise float32 sum of 1961 positive terms costs at most
  about 23 u, two sums, plus about 2 ulp of exp per factor."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import render_restatement as RR
from util import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 256
CASES = ("pred", "nan_target", "constant", "zero", "boundary", "over", "degenerate")
CLIP, REG = 1000.0, 5.70378


@pytest.fixture(scope="module")
def golden():
    return load_golden("render.npz")


@pytest.fixture(scope="module")
def lut():
    return RR.lut_bytes()


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


class Guarded:
    """nbytes of uint8 on the device between two guards of 0xA5."""

    def __init__(self, nbytes):
        self.n = nbytes
        self.t = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + GUARD)

    def get(self, shape=None):
        h = self.t.cpu().numpy()
        assert np.all(h[:GUARD] == 0xA5) and np.all(h[GUARD + self.n:] == 0xA5), "guard bytes overwritten"
        body = h[GUARD:GUARD + self.n]
        return body if shape is None else body.reshape(shape)


def raw_depth(maps, vmin, vmax, lut, pairs=None):
    """ramnet_render_depth on guarded outputs -> (code, grey, colour, scale)."""
    from rpg_ramnet_amd import _hip as H, metrics as M, render
    from rpg_ramnet_amd.ops import _st
    G = len(maps)
    hw = maps[0].shape if G else (4, 4)
    npix = hw[0] * hw[1]
    dm = [to_dev(m) for m in maps]
    dp = [to_dev(p) for p, _ in pairs] if pairs else []
    dt = [to_dev(t) for _, t in pairs] if pairs else []
    L = H.lib()
    ws = render._workspace(torch.device(DEV), max(L.ramnet_render_depth_workspace(max(G, 1), len(dp), npix), 1))
    tab = M._fill_table(torch.device(DEV), [t.data_ptr() for t in dm + dp + dt] or [0], 1)[0]
    at = lambda i: C.c_void_p(tab.data_ptr() + 8 * i)
    grey, color = Guarded(max(G, 1) * npix), Guarded(4 * max(G, 1) * npix)
    scale = torch.full((max(len(dp), 1),), -7.0, device=DEV, dtype=torch.float64)
    dl = None if lut is None else to_dev(lut)
    code = L.ramnet_render_depth(at(0), G, hw[0], hw[1], float(vmin), float(vmax), None if dl is None else C.c_void_p(dl.data_ptr()),
                                 at(G) if dp else None, at(G + len(dp)) if dp else None, len(dp), CLIP, REG, C.c_void_p(ws.data_ptr()), grey.ptr,
                                 color.ptr, C.c_void_p(scale.data_ptr()) if dp else None, _st())
    torch.cuda.synchronize()
    return code, grey.get((max(G, 1),) + tuple(hw)), color.get((max(G, 1),) + tuple(hw) + (4,)), scale.cpu().numpy()


def restated(maps, vmin, vmax, lut):
    both = [RR.render_depth(m, vmin, vmax, lut) for m in maps]
    return np.stack([g for g, _ in both]), np.stack([c for _, c in both])


@pytest.mark.parametrize("case", CASES)
def test_render_depth_golden_cases_one_map(golden, lut, case):
    vmin, vmax = golden[case + ".limits"]
    m = golden[case + ".map"]
    code, grey, color, _ = raw_depth([m], vmin, vmax, lut)
    assert code == 0
    wg, wc = restated([m], vmin, vmax, lut)
    assert np.array_equal(grey, wg) and np.array_equal(color, wc), (case, int((color != wc).any(axis=-1).sum()), int((grey != wg).sum()))
    assert np.array_equal(color[0], RR.saturate_u8(golden[case + ".rgba"][..., [2, 1, 0, 3]] * 255.0))      # the reference itself


@pytest.mark.parametrize("limits_of", ("pred", "over", "degenerate"))
def test_render_depth_seven_mixed_maps_in_one_call(golden, lut, limits_of):
    vmin, vmax = golden[limits_of + ".limits"]
    maps = [golden[c + ".map"] for c in CASES]
    code, grey, color, _ = raw_depth(maps, vmin, vmax, lut)
    assert code == 0
    wg, wc = restated(maps, vmin, vmax, lut)
    assert np.array_equal(grey, wg) and np.array_equal(color, wc)
    code, grey2, color2, _ = raw_depth(maps, vmin, vmax, lut)                # a repeat: the same bytes
    assert code == 0 and grey2.tobytes() == grey.tobytes() and color2.tobytes() == color.tobytes()


@pytest.mark.parametrize("shape", ((3, 5), (64, 257)))
def test_render_depth_ragged_tails(lut, shape):
    """3 x 5: fewer pixels than a thread's four, one workgroup; 64 x 257: three workgroups per map join, the last one short; a NaN in the
    last workgroup's part has to reach the whole map; values outside [0, 1] saturate the grey image."""
    rng = np.random.default_rng(11)
    a = (1.4 * rng.random(shape) - 0.2).astype(np.float32)
    b = rng.random(shape).astype(np.float32)
    b[-1, -1] = np.nan
    c = rng.random(shape).astype(np.float32)
    c[0, 0], c[-1, -2] = 1.0, 0.0                                            # the extrema in the first and in the last part
    code, grey, color, _ = raw_depth([a, b, c], 0.07, 0.83, lut)
    assert code == 0
    wg, wc = restated([a, b, c], 0.07, 0.83, lut)
    assert np.array_equal(grey, wg) and np.array_equal(color, wc)
    assert len({tuple(p) for p in color[1].reshape(-1, 4).tolist()}) == 1 and grey[1][-1, -1] == 0


def test_render_depth_bad_arguments_leave_the_outputs_alone(golden, lut):
    m = golden["pred.map"]
    for maps, table in (([], lut), ([m], None)):                             # G = 0; a NULL LUT
        code, grey, color, _ = raw_depth(maps, 0.1, 0.9, table)
        assert code == 10001
        assert np.all(grey == 0xA5) and np.all(color == 0xA5)


def test_render_surface(golden, lut):
    from rpg_ramnet_amd import render
    mapper = render.ColorMapper(*golden["pred.limits"])
    maps = [to_dev(golden[c + ".map"]) for c in ("pred", "nan_target", "boundary")]
    grey, color = render.render_depth([maps[0][None, None], maps[1][None], maps[2]], mapper)
    assert grey.device.type == "cuda" and grey.dtype == color.dtype == torch.uint8
    assert tuple(grey.shape) == (3, 37, 53) and tuple(color.shape) == (3, 37, 53, 4)
    wg, wc = restated([m.cpu().numpy() for m in maps], mapper.vmin, mapper.vmax, lut)
    assert np.array_equal(grey.cpu().numpy(), wg) and np.array_equal(color.cpu().numpy(), wc)
    with pytest.raises(ValueError):
        render.render_depth([maps[0].cpu()], mapper)
    with pytest.raises(ValueError):
        render.render_depth([maps[0], maps[1][:30]], mapper)


# ------------------------------------------------------------------------------------------------ inputs
def crafted_inputs():
    """C = 5 events whose channel sums sit at, just below and just above 0.9 and -0.5, and a C = 1 frame at k / 255 and (k + 0.5) / 255
    and their float32 neighbours; the rest is seeded noise."""
    rng = np.random.default_rng(21)
    H, W = 37, 53
    f32 = np.float32
    ev = (rng.integers(-3, 4, (5, H, W)) * 0.25 + rng.standard_normal((5, H, W)) * 0.01).astype(np.float32)
    flat = ev.reshape(5, -1)
    wanted = []
    for thr in (f32(0.9), f32(-0.5)):
        wanted += [thr, np.nextafter(thr, f32(4)), np.nextafter(thr, f32(-4))]
    for j, s in enumerate(wanted):
        flat[:4, j] = (0.5, -0.5, 0.25, -0.25)                               # every partial sum is exact, the last one is s
        flat[4, j] = s
    sums = np.sum(ev, axis=0).ravel()
    assert all(s in sums[:len(wanted)] for s in wanted)
    vals = []
    for k in range(256):
        for c in (f32(k) / f32(255), (f32(k) + f32(0.5)) / f32(255)):
            vals += [np.nextafter(c, f32(-4)), c, np.nextafter(c, f32(4))]
    fr = rng.random(H * W).astype(np.float32)
    fr[:len(vals)] = vals
    fr[len(vals):len(vals) + 3] = (np.nan, 2.0, -1.0)
    return ev, fr.reshape(1, H, W)


def test_render_inputs_thresholds_bit_for_bit():
    from rpg_ramnet_amd import _hip as H, metrics as M, render
    from rpg_ramnet_amd.ops import _st
    ev, fr = crafted_inputs()
    want = np.stack([RR.render_input(ev, RR.KIND_EVENTS), RR.render_input(fr, RR.KIND_FRAME), RR.render_input(ev[:2], RR.KIND_FRAME)])
    assert want[0, ..., 0].any() and want[0, ..., 2].any() and not want[0, ..., 1].any() and len(np.unique(want[1])) == 256
    dev = [to_dev(ev), to_dev(fr), to_dev(ev[:2])]
    tab = M._fill_table(torch.device(DEV), [t.data_ptr() for t in dev], 1)
    out = Guarded(3 * 37 * 53 * 3)
    code = H.lib().ramnet_render_inputs(C.c_void_p(tab.data_ptr()), (C.c_int * 3)(5, 1, 2), (C.c_int * 3)(0, 1, 1), 3, 37, 53, out.ptr, _st())
    torch.cuda.synchronize()
    assert code == 0
    got = out.get((3, 37, 53, 3))
    assert np.array_equal(got, want), [int((got[i] != want[i]).sum()) for i in range(3)]
    rgb = render.render_inputs([dev[0][None], dev[1], dev[2]], ["events0", "image", render.KIND_FRAME])
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (3, 37, 53, 3) and np.array_equal(rgb.cpu().numpy(), want)
    # bad arguments: nothing is written
    bad = Guarded(37 * 53 * 3)
    assert H.lib().ramnet_render_inputs(C.c_void_p(tab.data_ptr()), (C.c_int * 1)(0), (C.c_int * 1)(0), 1, 37, 53, bad.ptr, _st()) == 10001
    assert H.lib().ramnet_render_inputs(C.c_void_p(tab.data_ptr()), (C.c_int * 1)(5), (C.c_int * 1)(0), 0, 37, 53, bad.ptr, _st()) == 10001
    torch.cuda.synchronize()
    assert np.all(bad.get() == 0xA5)


# ------------------------------------------------------------------------------------------------ scale
def scale_bound(n):
    """relative bound of a least-squares scale of n pixels against the float64 sums of the same float32 products"""
    return n * 2.0 ** -52


def scale_pairs(shape, G, seed):
    rng = np.random.default_rng(seed)
    return [(np.clip(rng.random(shape) + 0.05 * rng.standard_normal(shape), 0, 1).astype(np.float32), rng.random(shape).astype(np.float32))
            for _ in range(G)]


@pytest.mark.parametrize("shape", ((37, 53), (64, 257)))
def test_least_squares_scale(shape):
    from rpg_ramnet_amd import metrics as M, render
    n = shape[0] * shape[1]
    pairs = scale_pairs(shape, 4, 31)
    pairs[2][1][shape[0] // 2, 3] = np.nan                                   # a NaN target: the scale of that pair is NaN
    ps, ts = [to_dev(p) for p, _ in pairs], [to_dev(t) for _, t in pairs]
    got_t = render.least_squares_scale(ps, ts, CLIP, REG)
    assert got_t.device.type == "cuda" and got_t.dtype == torch.float64 and tuple(got_t.shape) == (4,)
    got = got_t.cpu().numpy()
    again = render.least_squares_scale(ps, ts, CLIP, REG).cpu().numpy()
    assert got.tobytes() == again.tobytes()
    assert np.isnan(got[2]) and np.all(np.isfinite(got[[0, 1, 3]]))
    for g in (0, 1, 3):
        pm, tm = M.metric_depth(ps[g], CLIP, REG).cpu().numpy(), M.metric_depth(ts[g], CLIP, REG).cpu().numpy()
        want = RR.scale_float64(pm, tm)
        rel = abs(got[g] - want) / abs(want)
        print("%s pair %d: against the float64 sums %.3e (bound %.3e)" % (shape, g, rel, scale_bound(n)))
        assert rel <= scale_bound(n), (g, rel)
        if shape == (37, 53):
            ref = float(RR.scale_numpy(pairs[g][0], pairs[g][1], CLIP, REG))
            rel32 = abs(got[g] - ref) / abs(ref)
            print("%s pair %d: against numpy's float32 statement %.3e (bound %.3e)" % (shape, g, rel32, 64 * 2.0 ** -24))
            assert rel32 <= 64 * 2.0 ** -24, (g, rel32)


def test_scale_rides_in_the_depth_call(golden, lut):
    from rpg_ramnet_amd import render
    pairs = scale_pairs((37, 53), 3, 32)
    maps = [golden["pred.map"], golden["boundary.map"]]
    vmin, vmax = golden["pred.limits"]
    code, grey, color, scale = raw_depth(maps, vmin, vmax, lut, pairs)
    assert code == 0
    wg, wc = restated(maps, vmin, vmax, lut)
    assert np.array_equal(grey, wg) and np.array_equal(color, wc)
    alone = render.least_squares_scale([to_dev(p) for p, _ in pairs], [to_dev(t) for _, t in pairs], CLIP, REG).cpu().numpy()
    assert scale.tobytes() == alone.tobytes()


# ------------------------------------------------------------------------------------------------ the streaming driver
def test_stream_dataset_images_scale_and_metrics(tmp_path, lut):
    from PIL import Image
    from recipe import FOLDERS, make_dataset_dir
    from rpg_ramnet_amd import data as D, inference, metrics as M, render
    from util import build_hip_model, ref_cfg
    K = 3
    root = make_dataset_dir(str(tmp_path / "data"), n_seq=2, n_frames=15, H=32, W=48)
    ds = D.concatenate_subfolders(root, "SequenceSynchronizedFramesEventsDataset", sequence_length=1, step_size=1, transform=D.CenterCrop(32),
                                  clip_distance=CLIP, every_x_rgb_frame=K, reg_factor=REG, dataset_idx_flag=True, **FOLDERS)
    cfg, _ = ref_cfg("net_seeded_ramnet.npz", every_x_rgb_frame=K)
    model = build_hip_model("ERGB2DepthRecurrent", cfg)
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    base = inference.stream_dataset(model, ds, K, output_folder=plain, calculate_scale=True, reg_factor=REG, clip_distance=CLIP)
    assert "total_metrics" not in base and not os.path.exists(os.path.join(plain, "depth"))
    mapper = render.ColorMapper(0.05, 0.8)
    info = inference.stream_dataset(model, ds, K, output_folder=out, calculate_scale="device", reg_factor=REG, clip_distance=CLIP, images=True,
                                    color_mapper=mapper, metrics=True)
    keys = ["events%d" % k for k in range(K)] + ["image"]
    assert info["saved"] == base["saved"] > 0 and info["items"] == base["items"]
    if len(ds) <= 20:                                                        # test.py takes its mapper from package 20
        with pytest.raises(ValueError):
            inference.stream_dataset(model, ds, K, output_folder=str(tmp_path / "none"), images=True, max_items=1)

    # the layout of test.py
    assert sorted(os.listdir(out)) == ["color_map", "depth", "ground_truth", "npy", "video"]
    assert sorted(os.listdir(os.path.join(out, "ground_truth"))) == ["color_map", "grey", "npy"]
    assert sorted(os.listdir(os.path.join(out, "video"))) == ["gt", "inputs", "predictions"]
    names = sorted(os.listdir(os.path.join(out, "npy", "image")))
    assert len(names) == info["saved"]
    frames = [n.replace("depth_", "frame_").replace(".npy", ".png") for n in names]
    for key in keys:
        assert sorted(os.listdir(os.path.join(out, "depth", key))) == frames and sorted(os.listdir(os.path.join(out, "color_map", key))) == frames
        for sub in ("grey", "color_map"):
            assert sorted(os.listdir(os.path.join(out, "ground_truth", sub, "depth_" + key))) == frames
    assert sorted(os.listdir(os.path.join(out, "depth"))) == sorted(keys)
    video = ['frame_{:010d}.png'.format(i) for i in range(info["saved"] * len(keys))]
    for sub in ("predictions", "gt", "inputs"):
        assert sorted(os.listdir(os.path.join(out, "video", sub))) == video

    def png(*parts):
        with Image.open(os.path.join(out, *parts)) as im:
            return np.asarray(im)

    # .npy byte-identical with and without images; every PNG == the restatement of the saved .npy / of the input
    rows, video_idx = [], 0
    for n, f in zip(names, frames):
        idx = int(n[len("depth_"):-len(".npy")])
        item = ds[idx][0][0]
        for key in keys:
            for a in (("npy", key, n), ("ground_truth/npy", "depth_" + key, n.replace("depth_", "frame_"))):
                with open(os.path.join(out, *a), "rb") as fa, open(os.path.join(plain, *a), "rb") as fb:
                    assert fa.read() == fb.read(), a
            p = np.load(os.path.join(out, "npy", key, n))
            t = np.load(os.path.join(out, "ground_truth/npy", "depth_" + key, n.replace("depth_", "frame_")))
            gp, cp = RR.render_depth(p[0], mapper.vmin, mapper.vmax, lut)
            gt, ct = RR.render_depth(t[0], mapper.vmin, mapper.vmax, lut)
            assert np.array_equal(png("depth", key, f), gp) and np.array_equal(png("color_map", key, f), cp), (key, f)
            assert np.array_equal(png("ground_truth/grey", "depth_" + key, f), gt), (key, f)
            assert np.array_equal(png("ground_truth/color_map", "depth_" + key, f), ct), (key, f)
            v = 'frame_{:010d}.png'.format(video_idx)
            assert np.array_equal(png("video/predictions", v), cp) and np.array_equal(png("video/gt", v), ct), (key, v)
            want_in = RR.render_input(item[key].numpy(), RR.KIND_EVENTS if "event" in key else RR.KIND_FRAME)
            assert np.array_equal(png("video/inputs", v), want_in), (key, v)
            video_idx += 1
            rows.append(M.eval_metrics(to_dev(p[None]), to_dev(t[None]), inference.TEST_METRICS))
    assert video_idx == info["saved"] * len(keys)
    want = np.sum(np.array(rows), 0) / len(rows)
    assert info["total_metrics"].shape == (6,) and info["total_metrics"].tobytes() == want.tobytes()

    # the device scale: same shape of answer; NaN here as on the host path (the synthetic targets hold NaN pixels and test.py:378 uses np.sum)
    assert len(info["scale"]) == 3
    assert all(np.isnan(a) == np.isnan(b) for a, b in zip(info["scale"], base["scale"]))
