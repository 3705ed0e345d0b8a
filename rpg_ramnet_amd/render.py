"""The images RAM_Net/test.py writes next to its .npy files (test.py:36-43, 197-205, 259-360) and its least-squares scale (test.py:365-378),
on the device: csrc/render.hip restates numpy's and matplotlib's arithmetic bit for bit, for all maps of a data package in two launches
(plus one for the input previews), and leaves uint8 planes in FILE order — grey [H, W], RGB [H, W, 3], RGBA [H, W, 4] — that `write_png`
stores as they are.  Nothing here synchronises; everything is enqueued on the current stream.

matplotlib is needed for the colormap's table only (`ColorMapper`), and imported there."""
import ctypes as C

import numpy as np
import torch

from . import _hip as H
from .metrics import _fill_table
from .ops import _p, _st

KIND_EVENTS, KIND_FRAME = 0, 1          # RAMNET_RENDER_EVENTS, RAMNET_RENDER_FRAME
TICKET_BYTES = 262144                   # RAMNET_RENDER_TICKET_BYTES: the part of a workspace that has to be zero when it is allocated

_workspaces = {}                        # (device index, raw stream) -> uint8 workspace (tickets zeroed once, at allocation)


def _extremum(v):
    """What matplotlib's Normalize keeps of a limit: a Python scalar (`.item()` of a numpy scalar or a 0-d tensor)."""
    return float(v.item() if hasattr(v, "item") else v)


def normalised_inverse(depth_map):
    """make_colormap's map before the colormap (test.py:37-40): nan_to_num(inv / amax(inv)), inv = nan_to_num(amax(v) - v, nan=1), float32."""
    v = np.asarray(depth_map, np.float32)
    with np.errstate(all="ignore"):
        inv = np.ones_like(v) * np.amax(v) - v
        inv = np.nan_to_num(inv, nan=1)
        return np.nan_to_num(inv / np.amax(inv))


class ColorMapper:
    """matplotlib's ScalarMappable(Normalize(vmin, vmax), cmap) as the kernel needs it: the two limits as Python floats and the colormap's
    table as 258 x 4 uint8 (its 256 colours, then `under`, then `over`; each entry rint(rgba * 255), what cv2.imwrite stores of it)."""

    def __init__(self, vmin, vmax, cmap="magma"):
        self.vmin, self.vmax = _extremum(vmin), _extremum(vmax)
        if not self.vmin <= self.vmax or not np.isfinite(self.vmax - self.vmin):
            raise ValueError("ColorMapper: finite vmin <= vmax, got %r, %r" % (vmin, vmax))
        import matplotlib                  # (only this option needs it)
        cm = matplotlib.colormaps[cmap] if isinstance(cmap, str) else cmap
        if cm.N != 256:
            raise ValueError("ColorMapper: a colormap of 256 colours, got %d" % cm.N)
        cm._init()
        rows = np.asarray(cm._lut, np.float64)[[*range(256), cm._i_under, cm._i_over]]
        self.lut = np.clip(np.rint(rows * 255.0), 0, 255).astype(np.uint8)
        self._tables = {}

    @classmethod
    def from_target(cls, depth_image, cmap="magma"):
        """test.py:197-205: the limits of the whole run from ONE target frame [1, H, W] (test.py takes package 20), vmin = the minimum of
        its inverted, normalised map and vmax = its 95th percentile.  A frame with a NaN gives vmin == vmax == 1: every image of the run is
        one colour, as in the reference.  Host-side, once per run."""
        frame = depth_image.detach().cpu().numpy() if torch.is_tensor(depth_image) else np.asarray(depth_image)
        q = normalised_inverse(frame[0])
        return cls(q.min(), np.percentile(q, 95), cmap)

    def table(self, device):
        """The uint8 table on `device` (uploaded once per device)."""
        device = torch.device(device)
        t = self._tables.get(device)
        if t is None:
            t = self._tables[device] = torch.from_numpy(self.lut).to(device)
        return t


def _workspace(device, nbytes):
    key = (device.index, _st().value or 0)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, device=device, dtype=torch.uint8)
        ws[:TICKET_BYTES].zero_()
        _workspaces[key] = ws
    return ws


def _maps(xs, what, device=None):
    """A list of H x W maps (leading dimensions of size 1 allowed) -> (contiguous float32 tensors on the device, (H, W))."""
    xs = list(xs)
    if not xs:
        raise ValueError("%s: nothing to render" % what)
    device = xs[0].device if device is None else device
    if device.type != "cuda":
        raise ValueError("%s: the maps must live on the GPU (no CPU fallback)" % what)
    hw = tuple(xs[0].shape[-2:])
    out = []
    for x in xs:
        if x.dim() < 2 or tuple(x.shape[-2:]) != hw or x.numel() != hw[0] * hw[1]:
            raise ValueError("%s: every map is one %s map, got %s" % (what, hw, tuple(x.shape)))
        out.append(x.detach().to(device=device, dtype=torch.float32, non_blocking=True).contiguous())
    return out, hw


def _kind(k):
    if isinstance(k, str):
        return KIND_EVENTS if "event" in k else KIND_FRAME          # test.py:339 decides by the key
    if k in (KIND_EVENTS, KIND_FRAME):
        return int(k)
    raise ValueError("render_inputs: a kind is KIND_EVENTS, KIND_FRAME or the key of the input, got %r" % (k,))


def _inputs(xs, kinds, hw, device):
    xs = list(xs)
    kinds = [_kind(k) for k in kinds]
    if len(xs) != len(kinds):
        raise ValueError("render_inputs: %d inputs, %d kinds" % (len(xs), len(kinds)))
    ts, cs = [], []
    for x in xs:
        if x.dim() == 4 and x.shape[0] == 1:
            x = x[0]
        if x.dim() != 3 or (hw is not None and tuple(x.shape[-2:]) != hw) or x.shape[0] < 1:
            raise ValueError("render_inputs: every input is C x H x W%s, got %s" % ("" if hw is None else " with H x W = %s" % (hw,), tuple(x.shape)))
        hw = tuple(x.shape[-2:])
        ts.append(x.detach().to(device=device, dtype=torch.float32, non_blocking=True).contiguous())
        cs.append(int(x.shape[0]))
    return ts, cs, kinds, hw


def render_package(maps, mapper, inputs=(), kinds=(), scale=None):
    """Everything test.py draws for one data package, in ONE uint8 buffer on the device (so that one copy brings it to the host):
    maps    G maps of normalised log depth, H x W each (predictions and targets alike)
    inputs  network inputs C x H x W (or 1 x C x H x W) with a kind each: KIND_EVENTS / KIND_FRAME, or the input's key ("events3", "image")
    scale   None or (preds, targets, clip_distance, reg_factor): the least-squares scale of those pairs rides in the first launch
    -> (buffer, colour [G, H, W, 4], grey [G, H, W], rgb [len(inputs), H, W, 3], scale float64 [pairs] or None); the three images are
    views of the buffer.  Two launches, three with inputs."""
    ms, hw = _maps(maps, "render_depth")
    device = ms[0].device
    npix, G = hw[0] * hw[1], len(ms)
    with torch.cuda.device(device):
        ins, cs, ks, _ = _inputs(inputs, kinds, hw, device) if len(inputs) else ([], [], [], hw)
        sp, st, clip, reg = [], [], 1.0, 0.0
        if scale is not None:
            sp, _ = _maps(scale[0], "least_squares_scale", device)
            st, hw_t = _maps(scale[1], "least_squares_scale", device)
            clip, reg = float(scale[2]), float(scale[3])
            if len(sp) != len(st) or hw_t != hw or tuple(sp[0].shape[-2:]) != hw:
                raise ValueError("render_package: the scale takes as many targets as predictions, of the maps' size %s" % (hw,))
        L = H.lib()
        nbytes = L.ramnet_render_depth_workspace(G, len(sp), npix)
        if nbytes == 0:
            raise ValueError("render_depth: unsupported sizes G=%d pairs=%d npix=%d" % (G, len(sp), npix))
        ws = _workspace(device, nbytes)
        tab = _fill_table(device, [t.data_ptr() for t in ms + sp + st + ins], 1)[0]
        buf = torch.empty(npix * (5 * G + 3 * len(ins)), device=device, dtype=torch.uint8)
        color, grey, rgb = buf[:4 * G * npix], buf[4 * G * npix:5 * G * npix], buf[5 * G * npix:]
        out = torch.empty(len(sp), device=device, dtype=torch.float64) if sp else None
        at = lambda i: C.c_void_p(tab.data_ptr() + 8 * i)
        H.check(L.ramnet_render_depth(at(0), G, hw[0], hw[1], mapper.vmin, mapper.vmax, C.c_void_p(mapper.table(device).data_ptr()),
                                      at(G) if sp else None, at(G + len(sp)) if sp else None, len(sp), clip, reg, C.c_void_p(ws.data_ptr()),
                                      C.c_void_p(grey.data_ptr()), C.c_void_p(color.data_ptr()), None if out is None else C.c_void_p(out.data_ptr()),
                                      _st()), "ramnet_render_depth")
        if ins:
            H.check(L.ramnet_render_inputs(at(G + 2 * len(sp)), (C.c_int * len(ins))(*cs), (C.c_int * len(ins))(*ks), len(ins), hw[0], hw[1],
                                           C.c_void_p(rgb.data_ptr()), _st()), "ramnet_render_inputs")
    return buf, color.view(G, hw[0], hw[1], 4), grey.view(G, hw[0], hw[1]), rgb.view(len(ins), hw[0], hw[1], 3), out


def split_package(buf, G, n_inputs, hw):
    """The views `render_package` returns, of a copy of its buffer (a host array or tensor): (colour, grey, rgb)."""
    npix = hw[0] * hw[1]
    return (buf[:4 * G * npix].reshape(G, hw[0], hw[1], 4), buf[4 * G * npix:5 * G * npix].reshape(G, hw[0], hw[1]),
            buf[5 * G * npix:].reshape(n_inputs, hw[0], hw[1], 3))


def render_depth(maps, mapper):
    """G maps of normalised log depth (H x W each, on the GPU) -> (grey [G, H, W], colour [G, H, W, 4] RGBA) uint8 on the device: test.py's
    `cv2.imwrite(img * 255.0)` and `cv2.imwrite(make_colormap(img, mapper) * 255.0)` as the files hold them.  Two launches for all maps."""
    _, color, grey, _, _ = render_package(maps, mapper)
    return grey, color


def render_inputs(tensors, kinds):
    """The input previews of test.py:338-358: tensors C x H x W (or 1 x C x H x W) on the GPU, kinds as in `render_package` ->
    [G, H, W, 3] RGB uint8 on the device; events: red where the channel sum is > 0.9, blue where it is <= -0.5; a frame: the sum as grey.
    One launch."""
    tensors = list(tensors)
    if not tensors:
        raise ValueError("render_inputs: nothing to render")
    device = tensors[0].device
    if device.type != "cuda":
        raise ValueError("render_inputs: the inputs must live on the GPU (no CPU fallback)")
    with torch.cuda.device(device):
        ins, cs, ks, hw = _inputs(tensors, kinds, None, device)
        tab = _fill_table(device, [t.data_ptr() for t in ins], 1)
        rgb = torch.empty((len(ins), hw[0], hw[1], 3), device=device, dtype=torch.uint8)
        H.check(H.lib().ramnet_render_inputs(C.c_void_p(tab.data_ptr()), (C.c_int * len(ins))(*cs), (C.c_int * len(ins))(*ks), len(ins), hw[0], hw[1],
                                             C.c_void_p(rgb.data_ptr()), _st()), "ramnet_render_inputs")
    return rgb


def least_squares_scale(preds, targets, clip_distance, reg_factor):
    """test.py:365-378 for G pairs of normalised log depth on the GPU: sum(p * t) / sum(p * p) over the unclamped metric depths of
    `metrics.metric_depth`, float32 products, float64 sums in a fixed order -> float64 [G] ON THE DEVICE.  NaN propagates.  One launch."""
    ps, hw = _maps(preds, "least_squares_scale")
    device = ps[0].device
    with torch.cuda.device(device):
        ts, hw_t = _maps(targets, "least_squares_scale", device)
        if len(ts) != len(ps) or hw_t != hw:
            raise ValueError("least_squares_scale: %d predictions of %s, %d targets of %s" % (len(ps), hw, len(ts), hw_t))
        L = H.lib()
        npix = hw[0] * hw[1]
        nbytes = L.ramnet_render_depth_workspace(0, len(ps), npix)
        if nbytes == 0:
            raise ValueError("least_squares_scale: unsupported sizes G=%d npix=%d" % (len(ps), npix))
        ws = _workspace(device, nbytes)
        tab = _fill_table(device, [t.data_ptr() for t in ps + ts], 2)
        out = torch.empty(len(ps), device=device, dtype=torch.float64)
        H.check(L.ramnet_least_squares_scale(C.c_void_p(tab[0].data_ptr()), C.c_void_p(tab[1].data_ptr()), len(ps), npix, float(clip_distance),
                                             float(reg_factor), C.c_void_p(ws.data_ptr()), _p(out), _st()), "ramnet_least_squares_scale")
    return out


def write_png(path, array):
    """A uint8 array as a PNG: [H, W] greyscale, [H, W, 3] RGB, [H, W, 4] RGBA — the channel order of the file."""
    from PIL import Image
    a = np.ascontiguousarray(array.cpu().numpy() if torch.is_tensor(array) else array)
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] in (3, 4))):
        raise ValueError("write_png: uint8 [H, W], [H, W, 3] or [H, W, 4], got %s %s" % (a.dtype, a.shape))
    Image.fromarray(a).save(path, format="PNG")             # (uint8: mode L, RGB or RGBA by the shape)
