"""The case table of the head, folded-decoder and upsample launch tests (tests/test_hip_fold_head_launch.py), shared with the CPU anchors
of tests/test_conv_restatement_cpu.py, which assert per row what the comparison rules rely on.  A sibling of tests/conv_launch_cases.py.

Families: "fold2x2" (RAMNET_ALGO_WINOGRAD24), "fold2x3" (RAMNET_ALGO_WINOGRAD24_2X3), "head" (RAMNET_ALGO_HEAD).
Data kinds: "int" (the exact rule: 5x5 weights 9 x {-1, 0, 1}, a quarter non-zero: the 9 clears the thirds of G and Gc, everything else
of the fold and the transforms is dyadic; inputs {-1, 0, 1}, half zero; bias and frame operands integers) and "normal" (derived rule)."""
import types
import zlib

import torch

import conv_restatement as cr

F64 = torch.float64


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _ri(g, shape, m):
    return torch.randint(-m, m + 1, shape, generator=g).to(F64)


def _rn(g, shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).float().to(F64)


def _sparse(g, shape, m, density):
    return _ri(g, shape, m) * (torch.rand(shape, generator=g) < density).to(F64)


# ---------------------------------------------------------------------------------------------------- folded forward
def _fold(name, fam, B, H, W, C0, Cout, kernel, **kw):
    c = dict(name=name, fam=fam, B=B, H=H, W=W, C0=C0, Cout=Cout, kernel=kernel, kind="int", bias=True, epi=cr.EPI_RELU, frame=2, pitch=0,
             fold_pair=1, wd=0.25, xd=0.5)
    assert not set(kw) - set(c), kw
    c.update(kw)
    return types.SimpleNamespace(**c)


def _fold_table():
    K2, K3 = "conv_wino24_kernel<%d,0,%d,%d>", "conv_wino24_kernel<4,0,%d,%d,3>"
    t = [
        # ---- F(2x2,4x4): 32-channel workgroups (chunks of 8), the tall / flat 64-column tiles, the pair form tall / flat
        _fold("n2_c16_32", "fold2x2", 1, 9, 5, 16, 32, K2 % (2, 8, 0)),
        _fold("n2_nopair", "fold2x2", 3, 5, 7, 32, 32, K2 % (2, 8, 0), fold_pair=0, epi=cr.EPI_LINEAR, pitch=4),
        _fold("tall_9x5", "fold2x2", 1, 9, 5, 32, 64, K2 % (4, 4, 0), pitch=4),
        _fold("flat_3x13", "fold2x2", 3, 3, 13, 32, 64, K2 % (4, 8, 0), epi=cr.EPI_LINEAR),
        _fold("pair_tall_9x5", "fold2x2", 3, 9, 5, 32, 32, K2 % (4, 4, 1)),
        _fold("pair_flat_3x13", "fold2x2", 1, 3, 13, 32, 32, K2 % (4, 8, 1), pitch=4, epi=cr.EPI_LINEAR),
        # ---- the minimum maps, odd sizes, more than one workgroup tile per axis, no bias, no frame
        _fold("min_2x2", "fold2x2", 1, 2, 2, 32, 64, K2 % (4, 4, 0)),
        _fold("min_2x7_pair", "fold2x2", 3, 2, 7, 32, 32, K2 % (4, 8, 1), bias=False),
        _fold("min_7x2_pair", "fold2x2", 1, 7, 2, 32, 32, K2 % (4, 4, 1), frame=0),
        _fold("two_tiles_17x8", "fold2x2", 1, 17, 8, 32, 64, K2 % (4, 4, 0), bias=False, frame=0, pitch=4),
        _fold("pair_three_tiles_9x15", "fold2x2", 1, 9, 15, 32, 32, K2 % (4, 4, 1), wd=0.2),
        _fold("c64_128", "fold2x2", 1, 5, 6, 64, 128, K2 % (4, 4, 0), wd=0.125, xd=0.25),
        # ---- F(2x3,4x4): the three tiles of wino23_tile, without and with the pair form (which tiles Wo + 1 columns); Wo % 3 = 1, 2, 0
        _fold("tx4_9x10", "fold2x3", 1, 9, 10, 32, 64, K3 % (4, 0), wd=0.125, xd=0.25),
        _fold("tx2_20x5", "fold2x3", 1, 20, 5, 32, 64, K3 % (2, 0), wd=0.125, xd=0.25, pitch=4, epi=cr.EPI_LINEAR),
        _fold("tx16_3x40", "fold2x3", 3, 3, 40, 32, 64, K3 % (16, 0), wd=0.125, xd=0.25),
        _fold("tx4_5x9", "fold2x3", 3, 5, 9, 32, 64, K3 % (4, 0), wd=0.125, xd=0.25, bias=False, frame=0),
        _fold("pair_tx4_9x10", "fold2x3", 3, 9, 10, 32, 32, K3 % (4, 1), wd=0.125, xd=0.25),
        _fold("pair_tx2_20x5", "fold2x3", 1, 20, 5, 32, 32, K3 % (2, 1), wd=0.125, xd=0.25, epi=cr.EPI_LINEAR),
        _fold("pair_tx16_3x40", "fold2x3", 1, 3, 40, 32, 32, K3 % (16, 1), wd=0.125, xd=0.25, pitch=4),
        _fold("pair_tx4_2x2", "fold2x3", 1, 2, 2, 32, 32, K3 % (4, 1), wd=0.125, xd=0.25),
        _fold("pair_tx4_9x12", "fold2x3", 1, 9, 12, 32, 32, K3 % (4, 1), wd=0.125, xd=0.25, bias=False),
        # ---- normal data (derived rule): ragged maps on every form
        _fold("normal_n2", "fold2x2", 2, 7, 9, 16, 32, K2 % (2, 8, 0), kind="normal", pitch=4),
        _fold("normal_tall", "fold2x2", 2, 17, 7, 64, 128, K2 % (4, 4, 0), kind="normal", epi=cr.EPI_LINEAR),
        _fold("normal_pair", "fold2x2", 2, 7, 19, 32, 32, K2 % (4, 8, 1), kind="normal", epi=cr.EPI_LINEAR),
        _fold("normal_tx4", "fold2x3", 2, 11, 13, 64, 64, K3 % (4, 0), kind="normal", pitch=4, epi=cr.EPI_LINEAR),
        _fold("normal_pair_tx16", "fold2x3", 2, 3, 41, 32, 32, K3 % (16, 1), kind="normal"),
        _fold("normal_pair_tx2", "fold2x3", 1, 21, 5, 64, 32, K3 % (2, 1), kind="normal", epi=cr.EPI_LINEAR),
    ]
    return t


FOLD = _fold_table()
FOLD_BY_NAME = {c.name: c for c in FOLD}
assert len(FOLD_BY_NAME) == len(FOLD)


def is_pair(c):
    return c.Cout == 32 and c.C0 % 32 == 0 and bool(c.fold_pair)


def build_fold(c):
    """the float64 descriptor of a folded forward row (conv_restatement.fold_statement): x0 is ANY [B][H + 4][W + 4][C0] tensor (the launch
    does not know that ramnet_pad2_sum made it), w5 the OIHW 5x5 weights, e0 / e1 the frame operands"""
    g = _gen(c.name)
    integer = c.kind == "int"
    H2, W2 = 2 * c.H, 2 * c.W
    d = types.SimpleNamespace(B=c.B, Ho=c.H, Wo=c.W, HoF=H2, WoF=W2, C0=c.C0, Cout=c.Cout, epi=c.epi, frame=c.frame, bias=None, e0=None, e1=None)
    if integer:
        d.x0 = _sparse(g, (c.B, c.H + 4, c.W + 4, c.C0), 1, c.xd)
        d.w5 = 9.0 * _sparse(g, (c.Cout, c.C0, 5, 5), 1, c.wd)
    else:
        d.x0 = _rn(g, (c.B, c.H + 4, c.W + 4, c.C0))
        d.w5 = _rn(g, (c.Cout, c.C0, 5, 5), 1.0 / (25 * c.C0) ** 0.5)
    if c.bias:
        d.bias = _ri(g, (c.Cout,), 8) if integer else _rn(g, (c.Cout,), 0.1)
    if c.frame:
        mk = (lambda s: _ri(g, s, 8)) if integer else (lambda s: _rn(g, s, 0.5))
        d.e0, d.e1 = mk((2, c.B, H2, c.frame * c.Cout)), mk((2, c.B, W2, c.frame * c.Cout))
    return d


# ---------------------------------------------------------------------------------------------------- head
def _head(name, cin, C0, Cout, B, H, W, **kw):
    c = dict(name=name, cin=cin, C0=C0, Cout=Cout, B=B, H=H, W=W, kind="int", bias=True, epi=cr.EPI_RELU, pitch=0, gmask=False, dbias=True)
    assert not set(kw) - set(c), kw
    c.update(kw)
    return types.SimpleNamespace(**c)


HEAD = [
    _head("cin1_1x1", 1, 4, 32, 1, 1, 1),
    _head("cin1_17x33", 1, 4, 20, 3, 17, 33, pitch=4, gmask=True),
    _head("cin3_16x32", 3, 4, 32, 1, 16, 32, epi=cr.EPI_LINEAR, gmask=True, dbias=False),
    _head("cin3_5x70", 3, 4, 8, 3, 5, 70, bias=False, pitch=8),
    _head("cin5_17x33", 5, 8, 32, 1, 17, 33, pitch=4),
    _head("cin5_wide_16x32", 5, 16, 20, 3, 16, 32, epi=cr.EPI_LINEAR, gmask=True),
    _head("cin10_5x70", 10, 12, 32, 1, 5, 70, gmask=True, dbias=False),
    _head("cin10_17x33", 10, 12, 8, 3, 17, 33, pitch=4, bias=False),
    _head("normal_cin5", 5, 8, 32, 2, 17, 33, kind="normal", pitch=4, gmask=True),
    _head("normal_cin10", 10, 12, 20, 1, 5, 70, kind="normal", epi=cr.EPI_LINEAR),
]
# more than 512 tiles of 8 x 32 pixels: the persistent loop of the backward-weights kernel takes a second trip (backward-weights only)
HEAD_BIG = _head("cin1_136x992", 1, 4, 32, 1, 136, 992, gmask=True)
HEAD_TAPS = [(t // 5 - 2, t % 5 - 2, t) for t in range(25)]


def build_head(c):
    """descriptor of a head row for conv_restatement.conv_statement / wgrad_statement: x0 = the head_cin real channels (PLAIN, dense padded
    5x5); x0_phys = the [B][H][W][C0] tensor the launch reads, whose padded channels hold 7 (they must not reach the result)"""
    g = _gen("head_" + c.name)
    integer = c.kind == "int"
    k = 5
    d = types.SimpleNamespace(in_mode=cr.IN_PLAIN, Hin=c.H, Win=c.W, B=c.B, C0=c.C0, C1=0, Cin=c.cin, Cout=c.Cout, N=c.Cout, stride=1, epi=c.epi, beta=0.0,
                              out_s2d=0, s2d_5x5=0, x1=None, xm=None, bias=None, e0=None, e1=None, out_old=None, active=None, transposed=False,
                              taps=HEAD_TAPS, Ho=c.H, Wo=c.W, HoF=c.H, WoF=c.W, os=(1, 1, 0, 0))
    d.x0 = _sparse(g, (c.B, c.H, c.W, c.cin), 2, 0.5) if integer else _rn(g, (c.B, c.H, c.W, c.cin))
    d.x0_phys = torch.full((c.B, c.H, c.W, c.C0), 7.0, dtype=F64)
    d.x0_phys[..., :c.cin] = d.x0
    d.w_oihw = _sparse(g, (c.Cout, c.cin, k, k), 3, 0.5) if integer else _rn(g, (c.Cout, c.cin, k, k), 1.0 / (25 * c.cin) ** 0.5)
    d.W = d.w_oihw.permute(2, 3, 1, 0).reshape(25, c.cin, c.Cout).contiguous()
    if c.bias:
        d.bias = _ri(g, (c.Cout,), 8) if integer else _rn(g, (c.Cout,), 0.1)
    # backward-weights operands of the same row
    d.dout = _sparse(g, (c.B, c.H, c.W, c.Cout), 4, 0.5) if integer else _rn(g, (c.B, c.H, c.W, c.Cout))
    d.gmask = (_ri(g, (c.B, c.H, c.W, c.Cout), 1) if integer else _rn(g, (c.B, c.H, c.W, c.Cout))) if c.gmask else None
    return d


# ---------------------------------------------------------------------------------------------------- packs
# (Cout, Cin, entry points it serves): fold2x2 in its three layouts ((8, 2), (16, 4), pair), fold2x3 in its two, the _dgrad packs (Cin % 64)
PACK_SHAPES = [(32, 16), (32, 32), (64, 32), (128, 64), (64, 64), (32, 64)]


def pack_weights(Cout, Cin, kind):
    g = _gen("pack%d_%d_%s" % (Cout, Cin, kind))
    if kind == "int":
        return 9.0 * _sparse(g, (Cout, Cin, 5, 5), 1, 0.5)
    return _rn(g, (Cout, Cin, 5, 5))
