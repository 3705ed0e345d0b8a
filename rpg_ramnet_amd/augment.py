"""Training augmentation on the device: the reference's ``Compose([RandomRotationFlip(0.0, 0.5, 0.0), RandomCrop(224)])`` recipe
(train.py:149-150, utils/data_augmentation.py) for tensors that already live on the GPU — voxel grids from the device voxeliser, uploaded
frames and targets — in one HIP launch per (channel count, layout) group of a sequence (csrc/augment.hip).

``draw`` replays the host classes' use of the ``random`` stream, so a device run and a host run with the same seeds choose the same flip,
angle and window.  What is computed differs from the host transform on purpose: with angle 0 the device path is an EXACT
flip + crop (values copied bit for bit, NaN included), where the host's ``grid_sample`` blurs by ~1e-4 and spreads every NaN over a 2x2
window.  Any other angle is ``affine_grid`` + ``grid_sample`` (bilinear, zeros, align_corners=False) in fp32.

``scale_factor`` < 1 (the datasets' ``scale_factor``, dataset.py:127-140: a bilinear ``F.interpolate`` AFTER the flip and crop) is fused into
the same launch: the window is read, the reduced output is written.  Coordinates, weights and blend are evaluated in double and rounded
once, where the host's ``F.interpolate`` rounds in fp32 at every step.

No CPU or eager fallback: without the library ``HipLibraryMissing`` is raised."""
import ctypes as C
import random as _random
from collections import namedtuple
from math import cos, pi, sin

import torch

from . import _hip as H
from . import data as D

Params = namedtuple("Params", "theta top left th tw exact hflip vflip")
Params.__doc__ = """One sample's transform: theta = the six fp32 values of the 2x3 matrix the host hands to affine_grid, (top, left, th, tw) =
the crop window in the flipped / rotated image, exact = theta is diag(+-1, +-1) (a pure flip), hflip / vflip = columns / rows mirrored."""

_launches = 0


def launch_count():
    """Number of ramnet_augment_batch / ramnet_augment_scale_batch launches this process has enqueued through this module."""
    return _launches


# ------------------------------------------------------------------------------------------------ the draws
def _split(transform):
    """transform -> (rotation-flip or None, crop or None); ValueError for anything the device path does not cover."""
    if transform is None:
        return None, None
    ts = list(transform.transforms) if isinstance(transform, D.Compose) else [transform]
    rot = crop = None
    for t in ts:
        if type(t) is D.RandomRotationFlip:
            if rot is not None or crop is not None:
                raise ValueError("augment: %s after %s is not supported (at most one RandomRotationFlip, followed by at most one crop)"
                                 % (type(t).__name__, type(crop or rot).__name__))
            rot = t
        elif type(t) in (D.RandomCrop, D.CenterCrop):
            if crop is not None:
                raise ValueError("augment: a second crop (%s) is not supported" % type(t).__name__)
            crop = t
        else:
            raise ValueError("augment: unsupported transform %s" % type(t).__name__)
    return rot, crop


def draw(transform, seed, height, width, is_flow=False, rng=None):
    """The parameters the host transform would choose for a [C, height, width] tensor under ``random.seed(seed)``, consuming the stream
    exactly as it does: one ``uniform`` and two ``random()`` for the rotation-flip, two ``randint`` for a RandomCrop unless the size
    already fits.  rng: a ``random.Random`` to draw from instead of the module-level stream (a loader thread that must not disturb it).
    transform None: the identity, nothing is seeded or drawn (the datasets do not seed then either)."""
    if is_flow:
        raise ValueError("augment: is_flow (optical-flow tensors) is not supported")
    rot, crop = _split(transform)
    h, w = int(height), int(width)
    r = _random if rng is None else rng
    if transform is not None:
        r.seed(seed)
    theta, hflip, vflip, exact = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), False, False, True
    if rot is not None:
        a = r.uniform(rot.degrees[0], rot.degrees[1]) * pi / 180.0
        M = torch.FloatTensor([[cos(a), -sin(a), 0], [sin(a), cos(a), 0], [0, 0, 1]])
        if r.random() < rot.p_hflip:
            M[:, 0] *= -1
            hflip = True
        if r.random() < rot.p_vflip:
            M[:, 1] *= -1
            vflip = True
        theta = tuple(float(v) for v in M[:2].reshape(-1).tolist())
        exact = (abs(theta[0]) == 1.0 and abs(theta[4]) == 1.0 and theta[1] == 0.0 and theta[3] == 0.0 and theta[2] == 0.0 and theta[5] == 0.0)
    top = left = 0
    th, tw = h, w
    if crop is not None:
        th, tw = (int(v) for v in crop.size)
        if th > h or tw > w or th <= 0 or tw <= 0:
            raise ValueError("augment: a %d x %d window does not fit a %d x %d image" % (th, tw, h, w))
        if type(crop) is D.CenterCrop:
            top, left = int(round((h - th) / 2.)), int(round((w - tw) / 2.))
        elif w == tw and h == th:
            top = left = 0
        else:
            top = r.randint(0, h - th)
            left = r.randint(0, w - tw)
        top, left = D._even(top, left, crop.preserve)
        if top + th > h or left + tw > w:
            raise ValueError("augment: window rows %d..%d, columns %d..%d leave the %d x %d image (preserve_mosaicing_pattern moved it)"
                             % (top, top + th, left, left + tw, h, w))
    return Params(theta, top, left, th, tw, exact, hflip, vflip)


# ------------------------------------------------------------------------------------------------ parameter tables
class ParamTable:
    """The parameter sets of one launch as two small tensors (theta [P, 6] fp32, win [P, 4] int32 = top, left, exact, flips), built on the
    host — every window is checked against the image here — and uploaded with ``to``."""

    def __init__(self, params, height, width, pin=False):
        params = [params] if isinstance(params, Params) else list(params)
        if not params:
            raise ValueError("augment: no parameter set")
        self.H, self.W, self.th, self.tw = int(height), int(width), params[0].th, params[0].tw
        for p in params:
            if (p.th, p.tw) != (self.th, self.tw):
                raise ValueError("augment: the windows of one launch must have one size")
            if p.top < 0 or p.left < 0 or p.top + p.th > self.H or p.left + p.tw > self.W or p.th <= 0 or p.tw <= 0:
                raise ValueError("augment: window (top %d, left %d, %d x %d) leaves the %d x %d image" % (p.top, p.left, p.th, p.tw, self.H, self.W))
        self.n = len(params)
        self.theta = torch.tensor([p.theta for p in params], dtype=torch.float32).reshape(self.n, 6)
        self.win = torch.tensor([[p.top, p.left, int(p.exact), int(p.hflip) | (int(p.vflip) << 1)] for p in params], dtype=torch.int32)
        if pin:
            self.theta, self.win = self.theta.pin_memory(), self.win.pin_memory()
        self.theta_d = self.win_d = None

    def to(self, device, non_blocking=False):
        self.theta_d = self.theta.to(device, non_blocking=non_blocking)
        self.win_d = self.win.to(device, non_blocking=non_blocking)
        return self


def _table(params, height, width, device):
    if isinstance(params, ParamTable):
        if (params.H, params.W) != (int(height), int(width)):
            raise ValueError("augment: parameter table built for %d x %d, tensors are %d x %d" % (params.H, params.W, height, width))
        if params.theta_d is None or params.theta_d.device != torch.device(device):
            params.to(device)
        return params
    return ParamTable(params, height, width).to(device)


_coords = {}       # (H, W, device) -> (bx, by): torch's own normalised pixel-centre coordinates of affine_grid(align_corners=False)
_ptrs = {}         # (device, base pointer, G, stride in bytes) -> int64 [G] device table of the slices of one contiguous tensor


def _base_coords(height, width, device):
    key = (int(height), int(width), str(device))
    if key not in _coords:
        def lin(n):
            return (torch.linspace(-1, 1, n) * (n - 1) / n) if n > 1 else torch.zeros(1)
        _coords[key] = (lin(int(width)).to(device), lin(int(height)).to(device))
    return _coords[key]


def _slices(t, G):
    """Device table of the G equal slices of the contiguous tensor t along its first dimension(s)."""
    nbytes = t.numel() // G * 4
    key = (str(t.device), t.data_ptr(), G, nbytes)
    tab = _ptrs.get(key)
    if tab is None:
        if len(_ptrs) >= 256:
            _ptrs.clear()
        tab = torch.tensor([t.data_ptr() + g * nbytes for g in range(G)], dtype=torch.int64).to(t.device)
        _ptrs[key] = tab
    return tab


def scaled_shape(th, tw, scale_factor, who="augment"):
    """scale_factor -> None where nothing is resized (s >= 1, as the reference's ``if self.scale_factor < 1.0``), else (s, oh, ow) of a
    th x tw window; ValueError for s <= 0, NaN and a window that keeps no pixel."""
    s = float(scale_factor)
    if not s > 0.0:
        raise ValueError("%s: scale_factor must be positive, got %r" % (who, scale_factor))
    if s >= 1.0:
        return None
    from .metrics import resized_shape
    oh, ow = resized_shape((th, tw), s)
    if oh < 1 or ow < 1:
        raise ValueError("%s: a %d x %d window has no pixel left at scale_factor %r" % (who, th, tw, scale_factor))
    return s, oh, ow


def _launch(src_tab, dst_tab, pidx, tab, stats, G, Cc, th, tw, cpad, nhwc, device, scaled=None):
    global _launches
    from .ops import _p, _st
    bx, by = _base_coords(tab.H, tab.W, device)
    if scaled is not None:
        s, oh, ow = scaled
        H.check(H.lib().ramnet_augment_scale_batch(_p(src_tab), _p(dst_tab), _p(pidx), _p(tab.theta_d), _p(tab.win_d), C.c_void_p(tab.win.data_ptr()),
                                                   _p(stats), _p(bx), _p(by), G, tab.n, Cc, tab.H, tab.W, th, tw, oh, ow, C.c_double(s), cpad,
                                                   1 if nhwc else 0, _st()), "ramnet_augment_scale_batch")
        _launches += 1
        return
    H.check(H.lib().ramnet_augment_batch(_p(src_tab), _p(dst_tab), _p(pidx), _p(tab.theta_d), _p(tab.win_d), C.c_void_p(tab.win.data_ptr()),
                                         _p(stats), _p(bx), _p(by), G, tab.n, Cc, tab.H, tab.W, th, tw, cpad, 1 if nhwc else 0, _st()),
            "ramnet_augment_batch")
    _launches += 1


def _out_shape(G, Cc, th, tw, nhwc, cpad):
    return (G, th, tw, cpad) if nhwc else (G, Cc, th, tw)


def apply(x, params, pidx=None, out=None, nhwc=False, cpad=None, stats=None, scale_factor=1.0):
    """x: [G, C, H, W] fp32 on the device.  params: one ``Params`` (for every tensor), a list of them or a ``ParamTable``; pidx: which set
    tensor g uses (int32 [G] on the device, or a list; default: g, or 0 when there is one set).  Returns [G, C, th, tw], or with
    nhwc=True the model's input layout [G, th, tw, cpad] (channels zero-padded; default cpad: C rounded up to 4) — bitwise
    ``ops.pack_input`` of the NCHW result.  stats: [G, 3] float64 nonzero statistics (ramnet_nonzero_stats_batch) to normalise the source
    values with while they are read.  scale_factor < 1: every window is resized to floor(th * s) x floor(tw * s) in the same launch (the
    datasets' bilinear ``F.interpolate``, evaluated in double on the window's fp32 values and rounded once); >= 1: nothing is resized.
    One launch, on the current stream."""
    if not (torch.is_tensor(x) and x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous()):
        raise ValueError("augment.apply: x must be a contiguous fp32 [G, C, H, W] tensor")
    if not float(scale_factor) > 0.0:
        raise ValueError("augment.apply: scale_factor must be positive, got %r" % (scale_factor,))
    H.lib()
    if not x.is_cuda:
        raise ValueError("augment.apply: x must be on the GPU (the host transform is rpg_ramnet_amd.data's)")
    G, Cc, Hh, W = x.shape
    tab = _table(params, Hh, W, x.device)
    if pidx is None:
        if tab.n not in (1, G):
            raise ValueError("augment.apply: %d parameter sets for %d tensors need a pidx" % (tab.n, G))
        pidx = None if tab.n == G else torch.zeros(G, dtype=torch.int32, device=x.device)
    elif not torch.is_tensor(pidx):
        if len(pidx) != G or min(pidx) < 0 or max(pidx) >= tab.n:
            raise ValueError("augment.apply: pidx must hold %d indices into %d parameter sets" % (G, tab.n))
        pidx = torch.tensor(list(pidx), dtype=torch.int32).to(x.device)
    cp = 0
    if nhwc:
        cp = (Cc + 3) // 4 * 4 if cpad is None else int(cpad)
        if cp < Cc or cp % 4:
            raise ValueError("augment.apply: cpad=%d cannot hold %d channels in steps of 4" % (cp, Cc))
    scaled = scaled_shape(tab.th, tab.tw, scale_factor, "augment.apply")
    oh, ow = (tab.th, tab.tw) if scaled is None else scaled[1:]
    shape = _out_shape(G, Cc, oh, ow, nhwc, cp)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != shape or not out.is_contiguous() or out.dtype != torch.float32 or out.device != x.device:
        raise ValueError("augment.apply: out must be a contiguous fp32 %s tensor on %s" % (shape, x.device))
    if stats is not None and not (stats.dtype == torch.float64 and stats.numel() == 3 * G and stats.is_contiguous() and stats.device == x.device):
        raise ValueError("augment.apply: stats must be [G, 3] float64 on the device")
    if G:
        _launch(_slices(x, G), _slices(out, G), pidx, tab, stats, G, Cc, tab.th, tab.tw, cp, nhwc, x.device, scaled)
    return out


# ------------------------------------------------------------------------------------------------ collated sequences
def _augmented_key(key):
    return key.startswith("events") or key == "image" or key.startswith("depth_")


def _seed_list(seeds):
    if torch.is_tensor(seeds):
        return [int(v) for v in seeds.reshape(-1).tolist()]
    return [int(v) for v in seeds]


class _Plan:
    """Everything one sequence's launches need, prepared (and uploaded) ahead of them: per (C, H, W) group the pointer tables, the
    parameter indices and the output buffer."""

    def __init__(self, sequence, table, device, non_blocking=False, scale_factor=1.0):
        self.sequence, self.table, self.device = sequence, table, device
        self.scaled = scaled_shape(table.th, table.tw, scale_factor, "augment")
        groups = {}
        for l, item in enumerate(sequence):
            for key, t in item.items():
                if not _augmented_key(key) or not torch.is_tensor(t):
                    continue
                if not (t.dim() == 4 and t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda):
                    raise ValueError("augment: %r of package %d must be a contiguous fp32 [B, C, H, W] device tensor" % (key, l))
                if tuple(t.shape[2:]) != (table.H, table.W) or t.shape[0] != table.n:
                    raise ValueError("augment: %r of package %d is %s, the parameters are for %d samples of %d x %d"
                                     % (key, l, tuple(t.shape), table.n, table.H, table.W))
                groups.setdefault(int(t.shape[1]), []).append((l, key, t))
        B = table.n
        th, tw = (table.th, table.tw) if self.scaled is None else self.scaled[1:]          # what a launch writes
        self.groups = []
        words, total = [], 0
        for Cc, members in sorted(groups.items()):
            out = torch.empty(len(members), B, Cc, th, tw, device=device, dtype=torch.float32)
            src = [t.data_ptr() + b * Cc * table.H * table.W * 4 for _, _, t in members for b in range(B)]
            dst = [out.data_ptr() + g * Cc * th * tw * 4 for g in range(len(src))]
            words += src + dst
            self.groups.append((Cc, members, out, total, len(src)))
            total += 2 * len(src)
        host = torch.tensor(words, dtype=torch.int64)
        pidx = torch.arange(B, dtype=torch.int32).repeat(max((g[4] // B for g in self.groups), default=0))
        if non_blocking:
            host, pidx = host.pin_memory(), pidx.pin_memory()
        self.ptrs = host.to(device, non_blocking=non_blocking)
        self.pidx = pidx.to(device, non_blocking=non_blocking)
        if table.theta_d is None or table.theta_d.device != torch.device(device):
            table.to(device, non_blocking=non_blocking)
        _base_coords(table.H, table.W, device)
        self._keep = (host, pidx)                 # pinned staging stays alive until the plan is dropped

    def record_stream(self, stream):
        for t in [self.ptrs, self.pidx, self.table.theta_d, self.table.win_d] + [g[2] for g in self.groups]:
            t.record_stream(stream)

    def run(self):
        """The launches (one per group) on the current stream; returns the augmented sequence."""
        out_seq = [{k: v for k, v in item.items() if k != "transform_seed"} for item in self.sequence]
        for Cc, members, out, first, n in self.groups:
            _launch(self.ptrs[first:first + n], self.ptrs[first + n:first + 2 * n], self.pidx[:n], self.table, None, n, Cc, self.table.th,
                    self.table.tw, 0, False, self.device, self.scaled)
            for i, (l, key, _) in enumerate(members):
                out_seq[l][key] = out[i]
        return out_seq


def _sequence_extent(sequence):
    for item in sequence:
        for key, t in item.items():
            if _augmented_key(key) and torch.is_tensor(t) and t.dim() == 4:
                return int(t.shape[2]), int(t.shape[3]), t.device
    raise ValueError("augment: the sequence holds no events* / image / depth_* tensor")


def augment_sequence(sequence, seeds, transform, rng=None, scale_factor=1.0):
    """A collated sequence (list of L dicts of [B, C, H, W] device tensors) -> the same structure with every ``events*``, ``image`` and
    ``depth_*`` tensor transformed by its sample's parameters (``draw(transform, seeds[b], H, W)``; one seed per sample for the whole
    sequence, dataset.py:392), other keys passed through and ``transform_seed`` removed.  One launch per channel count — three for the
    RAM-Net recipe (event grids, frames, targets) — on the current stream.  seeds: [B] ints or a CPU tensor; None: the CPU tensor
    ``sequence[0]['transform_seed']``.  scale_factor < 1: the datasets' resize of every transformed tensor, in the same launches (``apply``);
    the tensors must then be at full resolution (datasets built with ``defer_scale=True``)."""
    H.lib()
    sequence = list(sequence)
    if seeds is None:
        seeds = sequence[0].get("transform_seed")
        if seeds is None:
            raise ValueError("augment_sequence: no seeds given and the sequence carries no 'transform_seed'")
    Hh, W, device = _sequence_extent(sequence)
    table = ParamTable([draw(transform, s, Hh, W, rng=rng) for s in _seed_list(seeds)], Hh, W)
    return _Plan(sequence, table, device, scale_factor=scale_factor).run()


# ------------------------------------------------------------------------------------------------ voxelise + normalise + transform
def voxelize_augmented(cat, off, max_count, num_bins, width, height, params, pidx=None, out=None, scratch=None, normalize=True, nhwc=False,
                       cpad=None, scale_factor=1.0):
    """Packed event lists (voxel.pack_event_lists) -> augmented grids: batched voxelisation into full-sensor grids, their nonzero statistics,
    then ONE launch that normalises and flips / rotates / crops while it reads (the reference normalises the full grid and then transforms,
    event_dataset.py:146-155, so the statistics cannot be had from cropped events).  Bitwise ``voxel.events_to_voxel_grids_packed(normalize=
    True)`` followed by ``apply``.  Allocation-free when ``params`` is an uploaded ParamTable, ``pidx`` a device tensor, and ``out`` and
    ``scratch`` (``voxel_scratch``) are given; everything runs on the current stream.  scale_factor < 1: the windows leave at the reduced
    size (``apply``), normalised with the statistics of the full-resolution grids as before."""
    from . import voxel
    from .ops import _p, _st
    G = int(off.shape[0]) - 1
    if scratch is None:
        scratch = voxel_scratch(G, num_bins, height, width, off.device)
    grids, stats = scratch["grids"], scratch["stats"]
    voxel.events_to_voxel_grids_packed(cat, off, max_count, num_bins, width, height, out=grids, normalize=False)
    if normalize:
        n = num_bins * int(height) * int(width)
        from . import ops
        if ops.deterministic():         # the statistics joined in workgroup order
            L = H.lib()
            part = torch.empty(L.ramnet_nonzero_stats_scratch_doubles(G, n), device=grids.device, dtype=torch.float64)
            H.check(L.ramnet_nonzero_stats_batch_ordered(_p(grids), G, n, _p(stats), _p(part), _st()), "ramnet_nonzero_stats_batch_ordered")
        else:
            H.check(H.lib().ramnet_nonzero_stats_batch(_p(grids), G, n, _p(stats), _st()), "ramnet_nonzero_stats_batch")
    return apply(grids, params, pidx=pidx, out=out, nhwc=nhwc, cpad=cpad, stats=stats if normalize else None, scale_factor=scale_factor)


def voxel_scratch(G, num_bins, height, width, device):
    """The buffers voxelize_augmented works in: the full-sensor grids and their statistics."""
    return {"grids": torch.empty(G, num_bins, int(height), int(width), device=device, dtype=torch.float32),
            "stats": torch.empty(G, 3, device=device, dtype=torch.float64)}


# ------------------------------------------------------------------------------------------------ loader
def _datasets_of(loader):
    """The datasets behind a loader as far as they can be seen: through DataLoader.dataset and ConcatDataset.datasets."""
    from torch.utils.data import DataLoader
    seen, todo = [], [loader]
    while todo:
        ds = todo.pop()
        if isinstance(ds, DataLoader):
            todo.append(ds.dataset)
        elif isinstance(getattr(ds, "datasets", None), (list, tuple)):
            todo.extend(ds.datasets)
        else:
            seen.append(ds)
    return seen


class AugmentedLoader(D.DevicePrefetcher):
    """``data.DevicePrefetcher`` over a loader of ``defer_transform=True`` sequences, followed by ``augment_sequence``: while the caller
    trains on sequence k, sequence k + 1 — its untransformed tensors, pointer tables and parameter tables — is uploaded on the copy
    stream; the launches run on the consumer's stream when the sequence is handed out.  The seeds are read from the CPU batch before it
    is uploaded: no device-to-host read and no synchronisation.  Yields what the trainer takes (lists of item dicts on the device).
    scale_factor < 1: the datasets' resize runs in the same launches; the datasets must then hand out full-resolution tensors
    (``scale_factor=s, defer_transform=True, defer_scale=True``).  A dataset that this loader can reach (through ``DataLoader.dataset`` and
    ``ConcatDataset.datasets``) and that has already resized on the host raises ValueError; behind any other wrapper the rule is the caller's."""

    def __init__(self, loader, device, transform, pin=True, scale_factor=1.0):
        super().__init__(loader, device, pin)
        if self.stream is None:
            raise ValueError("AugmentedLoader needs a GPU device (the host transform is the datasets' own)")
        H.lib()
        _split(transform)
        self.transform, self._rng = transform, _random.Random()
        self.scale_factor = float(scale_factor)
        if not self.scale_factor > 0.0:
            raise ValueError("AugmentedLoader: scale_factor must be positive, got %r" % (scale_factor,))
        if self.scale_factor < 1.0:
            for ds in _datasets_of(loader):
                s = getattr(ds, "scale_factor", None)
                if isinstance(s, (int, float)) and s < 1.0 and not getattr(ds, "defer_scale", False):
                    raise ValueError("AugmentedLoader: scale_factor=%r over a dataset that already resizes by %r on the host (build it with "
                                     "defer_scale=True)" % (scale_factor, s))

    def _stage(self, sequence):
        sequence = list(sequence)
        seeds = sequence[0].get("transform_seed")
        if seeds is None:
            raise ValueError("AugmentedLoader: the packages carry no 'transform_seed' (build the dataset with defer_transform=True)")
        seeds = _seed_list(seeds)
        sequence = [{k: v for k, v in item.items() if k != "transform_seed"} for item in sequence]
        Hh, W, _ = _sequence_extent(sequence)
        table = ParamTable([draw(self.transform, s, Hh, W, rng=self._rng) for s in seeds], Hh, W, pin=self.pin)
        with torch.cuda.stream(self.stream):
            moved = self._move(sequence)
            return _Plan(moved, table, self.device, non_blocking=self.pin, scale_factor=self.scale_factor)

    def __iter__(self):
        it = iter(self.loader)
        try:
            nxt = self._stage(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur = nxt
            here = torch.cuda.current_stream(self.device)
            here.wait_stream(self.stream)
            self._release(cur.sequence, here)
            cur.record_stream(here)
            out = cur.run()
            try:
                nxt = self._stage(next(it))
            except StopIteration:
                nxt = None
            yield out
