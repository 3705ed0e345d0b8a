"""The float64 statement of the event voxeliser (`ramnet_voxelize`, `ramnet_voxelize_batch`, `ramnet_voxelize_batch_sorted`,
`ramnet_voxel_indices` of include/ramnet_hip.h), and a Python restatement of the launcher's arithmetic: the rows of a band
(`voxel_band_rows`), the sorted form's cells and table, and which form takes a launch.  No GPU; anchored by
tests/test_voxel_restatement_cpu.py, used by tests/test_hip_voxel_launch.py.  profiles/voxel_launch_tests_notes.md.

The statement: list g of a batch is rows offsets[g] .. offsets[g + 1] of [t, x, y, p]; an event lies in the image where
-1 < x < W and -1 < y < H ON THE DOUBLE (the integer conversion truncates towards zero, so (-1, 0) is column / row 0; NaN, +-inf and
values no integer holds cast no vote); its two fp32 votes and their flat indices are `oracle.voxel_ref.voxel_votes` (pinned bit for bit to
the reference's index_add_ arguments by tests/golden/voxel_indices.npz); a cell is the sum of its votes, and every cell is written."""
import numpy as np

from oracle import voxel_ref

U = 2.0 ** -24
FIX = 2.0 ** 40                  # the sorted form adds votes as integers in units of 2^-40


def in_image(v, n):
    with np.errstate(invalid="ignore"):
        return (v > -1.0) & (v < float(n))


def votes(ev, bins, W, H):
    """(idx_left, val_left, ok_left, idx_right, val_right, ok_right) of one non-empty list: voxel_ref.voxel_votes under the in-image rule.
    (numpy's conversion of NaN or 1e300 to int64 is undefined, so the events outside the image are converted at (0, 0) and masked.)"""
    ev = np.asarray(ev, np.float64)
    inside = in_image(ev[:, 1], W) & in_image(ev[:, 2], H)
    safe = ev.copy()
    safe[~inside, 1:3] = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        il, vl, okl, ir, vr, okr = voxel_ref.voxel_votes(safe, bins, W, H)
    return il, vl, okl & inside, ir, vr, okr & inside


def indices(ev, bins, W, H):
    """what ramnet_voxel_indices writes: the flat indices, -1 where the vote is dropped"""
    il, _, okl, ir, _, okr = votes(ev, bins, W, H)
    return np.where(okl, il, -1), np.where(okr, ir, -1)


def grid(ev, bins, W, H):
    """One grid [bins, H, W], per cell: `exact` the float64 sum of the fp32 votes, `abs` of their magnitudes, `k` their number, `fixed`
    the sorted form's own result (each vote rounded to 2^-40 half-to-even, added as integers, one conversion to double, one product with
    2^-40, one rounding to fp32), `dyadic40` whether every vote of the cell is a multiple of 2^-40 (then `fixed` is the rounding of `exact`)."""
    n = bins * W * H
    z = dict(exact=np.zeros(n), abs=np.zeros(n), k=np.zeros(n, np.int64), fixed=np.zeros(n, np.float32), dyadic40=np.ones(n, bool))
    if len(ev):
        il, vl, okl, ir, vr, okr = votes(ev, bins, W, H)
        idx = np.concatenate([il[okl], ir[okr]])
        v = np.concatenate([vl[okl], vr[okr]]).astype(np.float64)
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < n)
        z["exact"] = np.bincount(idx, weights=v, minlength=n)
        z["abs"] = np.bincount(idx, weights=np.abs(v), minlength=n)
        z["k"] = np.bincount(idx, minlength=n)
        q = np.rint(v * FIX)                                    # (exact in double: an fp32 number times a power of two)
        acc = np.zeros(n, np.int64)
        np.add.at(acc, idx, q.astype(np.int64))
        z["fixed"] = (acc.astype(np.float64) * (1.0 / FIX)).astype(np.float32)
        z["dyadic40"] = np.bincount(idx, weights=(q != v * FIX), minlength=n) == 0
    return {k: a.reshape(bins, H, W) for k, a in z.items()}


def batch(lists, bins, W, H):
    """the statement of every grid of a batch, stacked [G, bins, H, W]"""
    gs = [grid(ev, bins, W, H) for ev in lists]
    return {k: np.stack([g[k] for g in gs]) for k in gs[0]}


def gamma(n):
    n = np.maximum(np.asarray(n, np.float64), 0.0)
    return n * U / (1.0 - n * U)


def bound_atomic(st):
    """fp32 additions in any order: k - 1 roundings on the magnitudes"""
    return gamma(st["k"] - 1) * st["abs"]


def bound_sorted(st):
    """half a fixed-point unit per vote, one rounding at the final conversion"""
    return U * np.abs(st["exact"]) + st["k"] * 2.0 ** -41


# ---------------------------------------------------------------------------------------- the launcher, restated
LDS_WORDS = (160 * 1024 - 512) // 4      # 4-byte words of a workgroup's LDS that a band and its queue or table share
CHUNK = 8192                             # events per sort chunk; also the batch of the walk with band ids
QUEUE_IDS, QUEUE_IDLESS = 8192, 4096
MIN_SORTED, MIN_SORTED_ENTRY, MIN_BANDS = 2, 1, 16
MAX_BANDS = 254                          # band ids are bytes, 255 = outside the image
MAX_COORD = 32767                        # the sorted record holds x | y << 16


def band_rows(bins, W, H, n_grids, queue_ints, min_grids=MIN_BANDS):
    """voxel_band_rows: rows of a band, 0 = this form does not take the launch"""
    if n_grids < min_grids:
        return 0
    rows = min((LDS_WORDS - (queue_ints + 2)) // (bins * W), H)
    if rows > 0 and -(-H // rows) > MAX_BANDS:
        return 0
    return rows


def sorted_rows(bins, W, H, n_grids, max_events, min_grids=MIN_SORTED):
    """rows of the sorted form: 8-byte cells (2 * bins words per pixel) beside a table of 2 * nchunks + 16 ints"""
    if not (0 < max_events < 2 ** 30 and W <= MAX_COORD and H <= MAX_COORD):
        return 0
    nchunks = -(-max_events // CHUNK)
    return band_rows(2 * bins, W, H, n_grids, 2 * nchunks + 16, min_grids)


def geometry(rows, H):
    """(rows, bands, rows of the last band)"""
    nb = -(-H // rows)
    return rows, nb, H - (nb - 1) * rows


NAMES = {"sorted": "voxel_sort_chunks_kernel + voxelize_sorted_kernel<rows=%d>", "ids": "voxel_band_ids_kernel + voxelize_bands_kernel<true,rows=%d>",
         "idless": "voxelize_bands_kernel<false,rows=%d>", "atomic_batch": "voxelize_batch_kernel", "atomic": "voxelize_kernel", "zero_fill": "zero_fill"}


def select(n_grids, max_events, bins, W, H, voxel_sorted=True, capture=False, entry="batch"):
    """(form, rows) of a launch: entry "batch" = ramnet_voxelize_batch, "sorted" = ramnet_voxelize_batch_sorted ((None, 0): refused),
    "single" = ramnet_voxelize.  capture: inside a stream capture the library hands out no scratch (no records, no band ids)."""
    if entry == "single":
        return ("atomic", 0) if max_events else ("zero_fill", 0)
    if entry == "sorted":
        if max_events == 0:
            return "zero_fill", 0
        r = 0 if capture else sorted_rows(bins, W, H, n_grids, max_events, MIN_SORTED_ENTRY)
        return ("sorted", r) if r else (None, 0)
    if n_grids >= 2:
        if voxel_sorted and not capture:
            r = sorted_rows(bins, W, H, n_grids, max_events)
            if r:
                return "sorted", r
        r = band_rows(bins, W, H, n_grids, QUEUE_IDS)
        if r and max_events > 0 and not capture:
            return "ids", r
        r = band_rows(bins, W, H, n_grids, QUEUE_IDLESS)
        if r:
            return "idless", r
    return ("atomic_batch", 0) if max_events else ("zero_fill", 0)


def kernel_name(form, rows):
    return NAMES[form] % rows if "%d" in NAMES[form] else NAMES[form]
