"""CPU: the numpy statement of csrc/render.hip (tests/render_restatement.py) against the reference's make_colormap
(tests/golden/render.npz, made by tests/golden/make_golden_render.py), and the host side of rpg_ramnet_amd.render: the colormap table,
the run's colour mapper, the PNG writer, the C interface and the defaults of inference.stream_dataset.

Unpinned (cv2 is not installed where the fixture is made): the float -> uint8 step of cv2.imwrite is OpenCV's documented saturate_cast
(round half to even, saturate, NaN -> 0), applied by the restatement; test.py builds its mapper inline in main(), so
ColorMapper.from_target is pinned against the restatement and matplotlib's Normalize only."""
import inspect
import os
import re

import numpy as np
import pytest

import render_restatement as RR
from util import load_golden

CASES = ("pred", "nan_target", "constant", "zero", "boundary", "over", "degenerate")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return load_golden("render.npz")


@pytest.fixture(scope="module")
def lut():
    return RR.lut_bytes()


def file_order(rgba):
    """make_colormap's float BGRA -> the bytes cv2.imwrite(rgba * 255.0) leaves in the file, RGBA."""
    return RR.saturate_u8(rgba[..., [2, 1, 0, 3]] * 255.0)


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_reference(golden, lut, case):
    vmin, vmax = golden[case + ".limits"]
    g, color = RR.render_depth(golden[case + ".map"], vmin, vmax, lut)
    want = file_order(golden[case + ".rgba"])
    assert color.dtype == np.uint8 and color.shape == want.shape == (37, 53, 4)
    assert np.array_equal(color, want), (case, int((color != want).any(axis=-1).sum()))
    assert g.shape == (37, 53) and g.dtype == np.uint8
    if case == "nan_target":
        assert np.all(g[np.isnan(golden[case + ".map"])] == 0)


def test_boundary_fixture_decides_the_precision(golden, lut):
    """The boundary map holds 0 and 1 and, for every k = 1..256, both float32 neighbours of the crossing of x * 256 = k: every colour occurs,
    and a float32 evaluation of Normalize's two steps would colour some pixels differently."""
    m = golden["boundary.map"]
    vmin, vmax = golden["boundary.limits"]
    assert m.min() == 0 and m.max() == 1
    idx = RR.lut_index(RR.normalised_inverse(m), vmin, vmax)
    assert set(range(256)) <= set(idx.ravel().tolist())
    q = RR.normalised_inverse(m)
    single = ((q - np.float32(vmin)) / (np.float32(vmax) - np.float32(vmin))) * np.float32(256)
    assert int(np.sum(np.clip(single, 0, 255).astype(np.int64) != np.clip(idx, 0, 255))) > 0


def test_lut_bytes(golden, lut):
    from rpg_ramnet_amd import render
    m = render.ColorMapper(0.1, 0.9)
    assert m.lut.dtype == np.uint8 and m.lut.shape == (258, 4) and np.array_equal(m.lut, lut)
    assert np.all(lut[:, 3] == 255)
    assert lut[0].tolist() == [0, 0, 4, 255] and lut[255].tolist() == [252, 253, 191, 255]          # magma's published end colours
    assert np.array_equal(lut[256], lut[0]) and np.array_equal(lut[257], lut[255])                  # under / over default to the ends
    seen = {tuple(p) for p in file_order(golden["boundary.rgba"]).reshape(-1, 4).tolist()}
    assert seen == {tuple(r) for r in lut.tolist()}
    assert (m.vmin, m.vmax) == (0.1, 0.9) and type(m.vmin) is float
    assert type(render.ColorMapper(np.float32(0.1), np.float64(0.9)).vmin) is float
    with pytest.raises(ValueError):
        render.ColorMapper(0.9, 0.1)
    with pytest.raises(ValueError):
        render.ColorMapper(float("nan"), 0.1)


def test_from_target(golden):
    import matplotlib as mpl
    from rpg_ramnet_amd import render
    frame = golden["pred.map"][None]
    m = render.ColorMapper.from_target(frame)
    vmin, vmax = RR.mapper_limits(frame)
    assert (m.vmin, m.vmax) == (vmin, vmax) and vmin < vmax
    q = RR.normalised_inverse(frame[0])
    n = mpl.colors.Normalize(vmin=q.min(), vmax=np.percentile(q, 95))      # test.py:203-204
    assert (n.vmin, n.vmax) == (m.vmin, m.vmax)
    # Normalize on the float32 map == the restatement's two float64 steps
    x = np.asarray(n(q.copy()))
    want = ((q.astype(np.float64) - vmin).astype(np.float32).astype(np.float64) / (vmax - vmin)).astype(np.float32)
    assert x.dtype == np.float32 and np.array_equal(x, want)
    import torch
    assert render.ColorMapper.from_target(torch.from_numpy(frame)).vmax == vmax
    nan = render.ColorMapper.from_target(golden["nan_target.map"][None])    # a NaN frame: the degenerate mapper
    assert (nan.vmin, nan.vmax) == (1.0, 1.0)
    assert np.all(RR.lut_index(q, nan.vmin, nan.vmax) == 0)


def test_input_and_scale_restatement():
    s = np.array([[np.float32(0.9), np.nextafter(np.float32(0.9), np.float32(2)), np.float32(-0.5), np.nextafter(np.float32(-0.5), np.float32(0))]])
    ev = RR.render_input(s[None], RR.KIND_EVENTS)
    assert ev.tolist() == [[[0, 0, 0], [255, 0, 0], [0, 0, 255], [0, 0, 0]]]
    fr = RR.render_input(np.array([[[0.5 / 255, 1.5 / 255, 2.0, -1.0, np.nan]]], np.float32), RR.KIND_FRAME)
    assert fr[0, :, 0].tolist()[2:] == [255, 0, 0] and np.all(fr[..., 0] == fr[..., 1]) and np.all(fr[..., 0] == fr[..., 2])
    assert RR.saturate_u8(np.array([0.5, 1.5, 2.5, 254.5, 255.5, -0.5])).tolist() == [0, 2, 2, 254, 255, 0]
    rng = np.random.default_rng(3)
    p, t = rng.random((5, 7)).astype(np.float32), rng.random((5, 7)).astype(np.float32)
    a = RR.scale_numpy(p, t, 1000.0, 5.70378)
    pm = np.exp(np.float32(5.70378) * (p - np.float32(1))) * np.float32(1000.0)
    tm = np.exp(np.float32(5.70378) * (t - np.float32(1))) * np.float32(1000.0)
    assert abs(RR.scale_float64(pm, tm) / a - 1) < 1e-5
    t[2, 3] = np.nan
    assert np.isnan(RR.scale_numpy(p, t, 1000.0, 5.70378))


def test_write_png_round_trip(tmp_path):
    from PIL import Image
    from rpg_ramnet_amd import render
    rng = np.random.default_rng(5)
    for shape, mode in (((9, 13), "L"), ((9, 13, 3), "RGB"), ((9, 13, 4), "RGBA")):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        path = str(tmp_path / ("%s.png" % mode))
        render.write_png(path, a)
        with Image.open(path) as im:
            assert im.mode == mode and im.format == "PNG"
            assert np.array_equal(np.asarray(im), a)
    import torch
    render.write_png(str(tmp_path / "t.png"), torch.from_numpy(a))
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "t.png"))), a)
    with pytest.raises(ValueError):
        render.write_png(str(tmp_path / "bad.png"), a.astype(np.float32))
    with pytest.raises(ValueError):
        render.write_png(str(tmp_path / "bad.png"), a[..., :2])


def test_c_interface():
    from rpg_ramnet_amd import _hip, render
    with open(os.path.join(ROOT, "include", "ramnet_hip.h")) as f:
        src = f.read()
    assert re.search(r"size_t\s+ramnet_render_depth_workspace\(int G, int n_scale, size_t npix\);", src)
    assert re.search(r"int\s+ramnet_render_depth\(const float \*const \*maps, int G, int H, int W, double vmin, double vmax, const unsigned char \*lut,"
                     r"\s*const float \*const \*scale_pred, const float \*const \*scale_target, int n_scale, float clip_distance,"
                     r"\s*float reg_factor, void \*workspace, unsigned char \*grey, unsigned char \*color, double \*scale, void \*stream\);", src)
    assert re.search(r"int\s+ramnet_least_squares_scale\(const float \*const \*pred, const float \*const \*target, int G, size_t npix, float clip_distance,"
                     r"\s*float reg_factor, void \*workspace, double \*scale, void \*stream\);", src)
    assert re.search(r"int\s+ramnet_render_inputs\(const float \*const \*inputs, const int \*channels, const int \*kinds, int G, int H, int W,"
                     r"\s*unsigned char \*rgb,\s*void \*stream\);", src)
    assert re.search(r"#define\s+RAMNET_ABI_VERSION\s+27\b", src)
    for name, value in (("RAMNET_RENDER_TICKET_BYTES", render.TICKET_BYTES), ("RAMNET_RENDER_EVENTS", render.KIND_EVENTS),
                        ("RAMNET_RENDER_FRAME", render.KIND_FRAME)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, src)
        assert m and int(m.group(1)) == value
    assert (render.KIND_EVENTS, render.KIND_FRAME) == (RR.KIND_EVENTS, RR.KIND_FRAME)
    for name in ("ramnet_render_depth_workspace", "ramnet_render_depth", "ramnet_least_squares_scale", "ramnet_render_inputs"):
        assert name in _hip.EXPORTS
    assert set(re.findall(r"\b(ramnet_[a-z0-9_]+)\s*\(", src)) == set(_hip.EXPORTS)
    assert "out of contract" in src.lower()                  # +-inf maps
    L = _hip.lib()
    assert L.ramnet_abi_version() == 27

    # what the calls refuse, before anything is launched (no device needed)
    import ctypes as C
    W = L.ramnet_render_depth_workspace
    assert W(0, 0, 16) == 0 and W(1, 0, 0) == 0 and W(-1, 2, 16) == 0 and W(1, -1, 16) == 0 and W(65535, 1, 16) == 0 and W(1, 0, 1 << 31) == 0
    assert W(12, 6, 260 * 346) >= render.TICKET_BYTES + 18 * 2 * 8 and W(0, 6, 16) > 0 and W(65535, 0, 16) > 0
    assert W(1, 0, 1961) == W(1, 0, 8192) < W(1, 0, 8193)      # one workgroup per map up to 8192 pixels
    ok = dict(maps=4096, G=1, H=4, W=4, vmin=0.0, vmax=1.0, lut=4096, sp=None, st=None, ns=0, clip=80.0, ws=4096, grey=4096, color=4096, scale=None)

    def depth(**over):
        a = dict(ok, **over)
        return L.ramnet_render_depth(a["maps"], a["G"], a["H"], a["W"], a["vmin"], a["vmax"], a["lut"], a["sp"], a["st"], a["ns"], a["clip"], 3.7,
                                     a["ws"], a["grey"], a["color"], a["scale"], None)

    assert depth(G=0) == 10001 and b"bad argument" in L.ramnet_last_error()
    assert depth(lut=None) == 10001 and depth(maps=None) == 10001 and depth(ws=None) == 10001 and depth(grey=None) == 10001 and depth(color=None) == 10001
    assert depth(H=0) == 10001 and depth(W=0) == 10001 and depth(H=1 << 16, W=1 << 15) == 10001 and depth(G=65536) == 10001
    assert depth(vmin=1.0, vmax=0.5) == 10001 and depth(vmin=float("nan")) == 10001 and depth(vmax=float("inf")) == 10001
    assert depth(ns=1) == 10001 and depth(ns=1, sp=4096, st=4096, scale=4096, clip=0.0) == 10001 and depth(ns=-1) == 10001
    assert depth(ws=4097) == 10001 and depth(color=4098) == 10001

    def scale(pred=4096, target=4096, G=1, npix=16, clip=80.0, ws=4096, out=4096):
        return L.ramnet_least_squares_scale(pred, target, G, npix, clip, 3.7, ws, out, None)

    assert scale(G=0) == 10001 and scale(pred=None) == 10001 and scale(target=None) == 10001 and scale(out=None) == 10001 and scale(ws=None) == 10001
    assert scale(npix=0) == 10001 and scale(clip=0.0) == 10001 and scale(out=4100) == 10001 and scale(G=65536) == 10001

    def inputs(inp=4096, ch=(5,), kinds=(0,), G=1, Hh=4, Ww=4, rgb=4096):
        c = None if ch is None else (C.c_int * len(ch))(*ch)
        k = None if kinds is None else (C.c_int * len(kinds))(*kinds)
        return L.ramnet_render_inputs(inp, c, k, G, Hh, Ww, rgb, None)

    assert inputs(G=0) == 10001 and inputs(inp=None) == 10001 and inputs(rgb=None) == 10001 and inputs(ch=None) == 10001 and inputs(kinds=None) == 10001
    assert inputs(ch=(0,)) == 10001 and inputs(kinds=(2,)) == 10001 and inputs(kinds=(-1,)) == 10001 and inputs(Hh=0) == 10001 and inputs(Ww=0) == 10001


def test_stream_dataset_defaults_are_off():
    from rpg_ramnet_amd import inference
    p = inspect.signature(inference.stream_dataset).parameters
    assert p["images"].default is False and p["color_mapper"].default is None and p["metrics"].default is False
    assert p["calculate_scale"].default is False
    assert list(p)[:12] == ["model", "dataset", "every_x_rgb_frame", "output_folder", "settle", "calculate_scale", "reg_factor", "clip_distance",
                            "max_items", "time_batched", "table", "rescale"]
    assert inference.TEST_METRICS == ("mse", "abs_rel_diff", "scale_invariant_error", "median_error", "mean_error", "rms_linear")

    class M:
        baseline = False
    assert inference.video_keys(M(), 3) == ["events0", "events1", "events2", "image"]
    M.baseline = "e"
    assert inference.video_keys(M(), 3) == ["events0", "events1", "image"]
    M.baseline = "rgb"
    assert inference.video_keys(M(), 3) == ["image"]
