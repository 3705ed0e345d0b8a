"""Rows and restatements of the deterministic-mode tests (tests/test_deterministic_cpu.py without a GPU, tests/test_hip_deterministic_launch.py
on one): the slab forms of the backward-weights families (ramnet_wgrad_desc.dw_slabs on RAMNET_ALGO_WINOGRAD24 / _2X3 / _HEAD / _DIRECT) and
the ordered forms of the joins that end on atomics.  Data are normal throughout: on integers every order of a sum gives the same bits."""
import types

import torch

import conv_restatement as cr
import fold_head_cases as fh

F64 = torch.float64
SLAB_CAP = 64                       # RAMNET_WGRAD_SLAB_CAP of include/ramnet_hip.h


def ordered_join(slabs):
    """ramnet_reduce_slabs as documented: slab 0 <- ((slab 0 + slab 1) + slab 2) + ... in fp32, one addition after the other"""
    acc = slabs[0].clone().float()
    for s in range(1, slabs.shape[0]):
        acc = acc + slabs[s].float()
    return acc


def accumulate(p, times):
    """what `times` launches leave in a zeroed slab that each of them read-modify-writes with the same partial sums p: ((0 + p) + p) + ..."""
    acc = torch.zeros_like(p)
    for _ in range(times):
        acc = acc + p
    return acc


# ---- folded decoders: (B, H, W, C0, Cout, slabs the query must answer).  6 x 7: ragged 2 x 3 tiles and an overhanging window, 3 batches of 8
# (F(2x2): 24 tiles) or 6 (F(2x3): 18 tiles) tiles -> 3 splits of one batch each; 10 x 9 at 256 -> 128: 256 / (8 x 8) = 4 splits over 13 batches
# of F(2x2) (100 tiles), the uneven 4 / 3 / 3 / 3 walk with a clamped tail (F(2x3): 60 tiles, 10 batches)
FOLD_ROWS = [(2, 6, 7, 32, 64, 3), (2, 6, 7, 64, 32, 3), (4, 10, 9, 256, 128, 4)]
FOLD_FAMS = {"fold2x2": 3, "fold2x3": 7}          # RAMNET_ALGO_WINOGRAD24, RAMNET_ALGO_WINOGRAD24_2X3


def build_fold(fam, row, gm):
    B, H, W, C0, Cout, _ = row
    g = fh._gen("det_fold%s%d%d%d%d" % (fam, H, W, C0, int(gm)))
    return types.SimpleNamespace(x0=fh._rn(g, (B, H + 4, W + 4, C0)), dout=fh._rn(g, (B, 2 * H, 2 * W, Cout)),
                                 gmask=fh._rn(g, (B, 2 * H, 2 * W, Cout)) if gm else None, Ho=H, Wo=W)


# ---- head: Cin 1 and 5 at 12 x 20 (two tiles of 8 x 32 pixels per image), and 3 x 5 x 5 = 75 tiles: more than the 64 workgroups of the slab form
HEAD_ROWS = [fh._head("det_cin1", 1, 4, 32, 2, 12, 20, kind="normal", gmask=True), fh._head("det_cin5", 5, 8, 32, 2, 12, 20, kind="normal", pitch=4),
             fh._head("det_cin1_75tiles", 1, 4, 32, 3, 40, 160, kind="normal", gmask=True)]


# ---- direct: a 1 x 1 (9 x 11, the map of tests/conv_launch_cases.py's mode rows), a 5 x 5 stride 2 over a concatenation (9 x 43 of its map
# rows), one parity class of the transposed-conv decoder through gsy ... WoG (5 x 9, test_direct_folded_classes_with_frame)
def build_direct(name):
    g = fh._gen("det_direct_" + name)
    if name == "k1":
        B, H, W, C0, C1, Cout, k, s = 2, 9, 11, 8, 0, 20, 1, 1
    elif name == "k5_s2_cat":
        B, H, W, C0, C1, Cout, k, s = 3, 9, 43, 8, 4, 64, 5, 2
    else:
        assert name == "parity"
        B, H, W, C0, Cout = 3, 5, 9, 8, 32
        full = types.SimpleNamespace(x0=fh._rn(g, (B, H + 4, W + 4, C0)), dout=fh._rn(g, (B, 2 * H, 2 * W, Cout)), gmask=fh._rn(g, (B, 2 * H, 2 * W, Cout)), Ho=H, Wo=W)
        d = cr.fold_class_wgrad(full, 1, 0)
        d.full, d.gview, d.C0, d.C1, d.Cout, d.B, d.Hin, d.Win = full, (2, 2, 1, 0, 2 * H, 2 * W), C0, 0, Cout, B, H + 4, W + 4
        return d
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    d = types.SimpleNamespace(in_mode=cr.IN_CAT if C1 else cr.IN_PLAIN, x0=fh._rn(g, (B, H, W, C0)), x1=fh._rn(g, (B, H, W, C1)) if C1 else None, xm=None,
                              stride=s, Ho=Ho, Wo=Wo, taps=[(a - p, b - p) for a in range(k) for b in range(k)], dout=fh._rn(g, (B, Ho, Wo, Cout)),
                              gmask=fh._rn(g, (B, Ho, Wo, Cout)) if C1 else None)
    d.full, d.gview, d.C0, d.C1, d.Cout, d.B, d.Hin, d.Win = None, None, C0, C1, Cout, B, H, W
    return d


DIRECT_ROWS = ["k1", "k5_s2_cat", "parity"]


def spread(g, shape):
    """normal values times powers of two over 2^-12 .. 2^12: the order of an fp32 sum of them shows in its last bits"""
    e = torch.randint(-12, 13, shape, generator=g).to(F64)
    return (torch.randn(*shape, generator=g).float().to(F64) * 2.0 ** e).float().to(F64)
