"""numpy statement of csrc/render.hip: what RAM_Net/test.py writes as images for a saved package (test.py:36-43, 259-360) and its
least-squares scale (test.py:365-378), as uint8 planes in FILE order (RGBA / RGB: cv2.imwrite swaps the BGR that make_colormap builds back).

The colour map follows numpy and matplotlib 3.10 operation by operation:
  make_colormap      a = amax(map) (NaN propagates), inv = nan_to_num(a - map, nan=1), q = nan_to_num(inv / amax(inv)), all float32
  Normalize.__call__ works in place on the float32 array with vmin / vmax as np.float64 scalars (the setters keep Python floats and
                     process_value makes them float64): under NumPy 2's promotion both `-= vmin` and `/= (vmax - vmin)` are evaluated in
                     float64 and rounded to float32, one after the other; vmin == vmax fills zeros
  Colormap.__call__  xa = x * 256 in float32, xa == 256 -> 255, xa < 0 -> under, xa >= 256 -> over, else truncation; rows of the LUT
cv2.imwrite's float -> uint8 step is OpenCV's documented saturate_cast: round half to even, saturate, and (here) NaN -> 0."""
import numpy as np

KIND_EVENTS, KIND_FRAME = 0, 1


def saturate_u8(x):
    """cv::saturate_cast<uchar>(float / double): cvRound (half to even), clamped to [0, 255]; NaN -> 0."""
    with np.errstate(invalid="ignore"):
        r = np.rint(np.asarray(x))
        r = np.where(np.isnan(r), 0, np.clip(r, 0, 255))
    return r.astype(np.uint8)


def lut_bytes(cmap="magma"):
    """[258, 4] uint8: the 256 colours of the matplotlib colormap, then its under and over colours — the rows Colormap.__call__ indexes,
    each as cv2.imwrite stores it (saturate_u8(rgba * 255.0))."""
    import matplotlib
    cm = matplotlib.colormaps[cmap]
    cm._init()
    assert cm.N == 256 and cm._i_under == 256 and cm._i_over == 257
    return saturate_u8(np.asarray(cm._lut[:258], np.float64) * 255.0)


def normalised_inverse(depth_map):
    """q of make_colormap / test.py:199-202 for one H x W float32 map."""
    v = np.asarray(depth_map, np.float32)
    with np.errstate(all="ignore"):
        inv = np.ones_like(v) * np.amax(v) - v
        inv = np.nan_to_num(inv, nan=1)
        q = inv / np.amax(inv)
        return np.nan_to_num(q)


def lut_index(q, vmin, vmax):
    """Row of the 258-row LUT for every element of the float32 array q under Normalize(vmin, vmax)."""
    vmin, vmax = np.float64(vmin), np.float64(vmax)
    if vmin > vmax:
        raise ValueError("minvalue must be less than or equal to maxvalue")
    q = np.asarray(q, np.float32)
    if vmin == vmax:
        x = np.zeros_like(q)
    else:
        x = (q.astype(np.float64) - vmin).astype(np.float32)
        x = (x.astype(np.float64) / (vmax - vmin)).astype(np.float32)
    xa = x * np.float32(256)
    xa[xa == 256] = 255
    with np.errstate(invalid="ignore"):
        idx = xa.astype(np.int64)
    idx[xa < 0] = 256
    idx[xa >= 256] = 257
    return idx


def grey(depth_map):
    """cv2.imwrite(img * 255.0) of a float32 map -> [H, W] uint8."""
    return saturate_u8(np.asarray(depth_map, np.float32) * np.float32(255.0))


def render_depth(depth_map, vmin, vmax, lut):
    """-> (grey [H, W] uint8, colour [H, W, 4] uint8 RGBA)."""
    return grey(depth_map), lut[lut_index(normalised_inverse(depth_map), vmin, vmax)]


def render_input(x, kind):
    """x: [C, H, W] float32 -> [H, W, 3] uint8 RGB (test.py:338-358)."""
    s = np.sum(np.asarray(x, np.float32), axis=0)
    if kind == KIND_EVENTS:
        neg, pos = np.where(s <= -0.5, 1.0, 0.0), np.where(s > 0.9, 1.0, 0.0)
        bgr = np.concatenate((neg[:, :, None], np.zeros_like(s)[:, :, None], pos[:, :, None]), axis=2)
        return saturate_u8(bgr * 255.0)[:, :, ::-1]
    g = saturate_u8(s * np.float32(255.0))
    return np.repeat(g[:, :, None], 3, axis=2)


def mapper_limits(depth_image):
    """(vmin, vmax) of test.py:197-204 for the [1, H, W] target of package 20."""
    q = normalised_inverse(np.asarray(depth_image, np.float32)[0])
    return float(q.min()), float(np.percentile(q, 95))


def scale_float64(p_metric, t_metric):
    """sum(p * t) / sum(p * p) over float32 metric depths: float32 products, float64 sums."""
    p, t = np.asarray(p_metric, np.float32).ravel(), np.asarray(t_metric, np.float32).ravel()
    return np.sum((p * t).astype(np.float64)) / np.sum((p * p).astype(np.float64))


def scale_numpy(pred, target, clip_distance, reg_factor):
    """test.py:365-378 as numpy evaluates it on float32 maps."""
    with np.errstate(all="ignore"):
        p = np.exp(reg_factor * (pred - np.ones(pred.shape, dtype=np.float32)))
        t = np.exp(reg_factor * (target - np.ones(target.shape, dtype=np.float32)))
        t *= clip_distance
        p *= clip_distance
        return np.sum(p * t) / np.sum(p * p)
