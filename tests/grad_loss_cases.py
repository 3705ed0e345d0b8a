"""The rows of tests/test_hip_grad_loss_launch.py and tests/test_grad_loss_restatement_cpu.py: shapes, data and NaN placements of the batched
multi-scale gradient loss.  Integer rows: predictions and targets are integers in [-16, 16], so diff, the 2 x 2 means (multiples of 1/64)
and the Sobel responses (multiples of 1/512) are fp32 numbers and every sign is the same in fp32 and in float64.

A row: G pairs of [B][H][W]; `nan`: a function (g, target) that places the NaN of pair g."""
import functools

import torch

import grad_loss_restatement as gr

F64 = torch.float64
NAN = float("nan")
HALO_DIST = (7, 8, 9, 15, 16, 17)         # around the 8-pixel halo of the statistics and the 16-pixel halo of the backward pass


def _pix(*yx):
    def place(g, t):
        for y, x in yx:
            t[0, y, x] = NAN
    return place


def _per_pair(places):
    def place(g, t):
        places[g](g, t)
    return place


def _halo_places():
    """single NaN pixels of a (90, 92) map with the tile edge between 63 and 64 in both axes: the three pixels at the tile corner, then d
    pixels outside the lower tile's edge (63 + d) and outside the upper tile's (64 - d), in rows (at column 30 and 70) and in columns"""
    out = [_pix((63, 63)), _pix((64, 64)), _pix((63, 64))]
    for d in HALO_DIST:
        out += [_pix((63 + d, 30)), _pix((64 - d, 70)), _pix((30, 63 + d)), _pix((70, 64 - d))]
    return out


def _block(g, t):          # straddles the tile corner (64, 64) and the 8 x 8-cell boundaries at 56 / 64 and 64 / 72
    t[0, 59:67, 61:70] = NAN


def _sample(g, t):         # one whole sample of the batch
    t[1] = NAN


def _empty_scale(g, t):    # pair 1 of three: both cells of the 1 x 2 coarsest level hold a NaN, the finer levels keep valid windows
    if g == 1:
        t[0, 0, 0] = NAN
        t[0, 7, 15] = NAN


HALO_PLACES = _halo_places()

# name: (G, B, H, W, ns, kind, nan)
ROWS = {
    "m1x1": (1, 1, 1, 1, 1, "int", None),
    "m2x3": (1, 1, 2, 3, 2, "int", None),
    "m8x8": (1, 3, 8, 8, 4, "int", None),
    "m8x21": (3, 1, 8, 21, 4, "int", None),
    "m64x64": (1, 1, 64, 64, 4, "int", None),
    "m70x131": (1, 1, 70, 131, 4, "int", None),
    "m66x69": (1, 1, 66, 69, 4, "int", None),               # W % 4 = 1 (63 x 66: 2, 65 x 67 and 70 x 131: 3)
    "m72x136": (1, 3, 72, 136, 4, "int", None),
    "g70": (70, 1, 8, 8, 4, "int", None),
    "join2": (1, 9, 65, 65, 4, "int", None),
    "halo": (len(HALO_PLACES), 1, 90, 92, 4, "int", _per_pair(HALO_PLACES)),
    "block": (1, 1, 70, 131, 4, "int", _block),
    "sample": (3, 3, 9, 15, 3, "int", _sample),
    "empty": (3, 1, 8, 21, 4, "int", _empty_scale),
    "empty_without": (3, 1, 8, 21, 4, "int", None),
    "normal": (1, 2, 70, 131, 4, "normal", None),
}
for _ns in (1, 2, 3, 4):
    ROWS["m9x15_ns%d" % _ns] = (1, 1, 9, 15, _ns, "int", None)
    ROWS["m63x66_ns%d" % _ns] = (3, 1, 63, 66, _ns, "int", None)
    ROWS["m65x67_ns%d" % _ns] = (1, 3, 65, 67, _ns, "int", None)
SEEDS = {"empty_without": "empty"}        # the same data as the row it is compared with
INT_ROWS = [n for n, r in ROWS.items() if r[5] == "int"]


@functools.lru_cache(maxsize=None)
def data(name):
    """-> (preds, targets): G tensors [B][H][W] each, float64 holding fp32 values"""
    G, B, H, W, ns, kind, nan = ROWS[name]
    gen = torch.Generator().manual_seed(1000 + sorted(ROWS).index(SEEDS.get(name, name)))
    preds, targets = [], []
    for g in range(G):
        if kind == "int":
            p, t = (torch.randint(-16, 17, (B, H, W), generator=gen).to(F64) for _ in range(2))
        else:
            p, t = (torch.randn(B, H, W, generator=gen).to(F64) for _ in range(2))
        if nan is not None:
            nan(g, t)
        preds.append(p)
        targets.append(t)
    return preds, targets


@functools.lru_cache(maxsize=None)
def statement(name):
    """-> (stats [G][ns][2], abs sums [G][ns]) of the row"""
    preds, targets = data(name)
    ns = ROWS[name][4]
    both = [gr.stats(p, t, ns) for p, t in zip(preds, targets)]
    return torch.stack([b[0] for b in both]), torch.stack([b[1] for b in both])
