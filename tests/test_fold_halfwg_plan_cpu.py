"""No GPU: the host plan of the half-workgroup form of the F(2x3,4x4) decoder launches (csrc/conv_wino24.hip: wino23_tile_half,
wino23_grid, fold_halfwg_variant) through ramnet_fold_halfwg_grid / ramnet_fold_halfwg_variant — the 16-tile block of every decoder map
of the flagship workload covers the map with no more padding than the 32-tile block, the grid is the block count, and the query turns
down what the 4-wave kernel is not built for."""
import ctypes as C

import pytest

from rpg_ramnet_amd import _hip as Hh

# the three decoder layers at 256 x 344: (Cin, Cout, low-res H, W) — parity grids 32x43, 64x86, 128x172, backward-data grids 36x47, 68x90, 132x176
DECODERS = [(256, 128, 32, 43), (128, 64, 64, 86), (64, 32, 128, 172)]
BLOCKS16 = {(8, 12), (16, 6), (4, 24), (2, 48)}           # 16 tiles of 2 x 3 outputs
BLOCKS32 = {(16, 12), (32, 6), (4, 48)}


def _cdiv(a, b):
    return -(-a // b)


def _fwd(B, H, W, Cin, Cout, algo=Hh.ALGO_WINOGRAD24_2X3):
    d = Hh.ConvDesc()
    d.ld0, d.C0, d.in_mode = Cin, Cin, Hh.IN_PLAIN
    d.B, d.Hin, d.Win, d.stride, d.ntaps = B, H + 4, W + 4, 1, 16
    d.Cout, d.Ho, d.Wo, d.HoF, d.WoF = Cout, H, W, 2 * H, 2 * W
    d.osy, d.osx, d.epi, d.ldo, d.algo = 1, 1, Hh.EPI_LINEAR, Cout, algo
    return d


def _dgrad(B, H, W, Cin, Cout, algo=Hh.ALGO_WINOGRAD24_2X3):
    d = Hh.ConvDesc()
    d.ld0, d.C0, d.in_mode = Cout, Cout, Hh.IN_PARITY4
    d.B, d.Hin, d.Win, d.stride, d.ntaps = B, 2 * H, 2 * W, 1, 16
    d.Cout, d.Ho, d.Wo, d.HoF, d.WoF = Cin, H + 4, W + 4, H + 4, W + 4
    d.osy, d.osx, d.epi, d.ldo, d.algo = 1, 1, Hh.EPI_LINEAR, Cin, algo
    return d


def _grid(d, half):
    r, c, n = C.c_int(), C.c_int(), C.c_long()
    assert Hh.lib().ramnet_fold_halfwg_grid(C.byref(d), half, C.byref(r), C.byref(c), C.byref(n)) == 0, Hh.lib().ramnet_last_error()
    return r.value, c.value, n.value


def _maps():
    for Cin, Cout, H, W in DECODERS:
        pair = Cout == 32
        # (descriptor maker, map rows, map columns the tiles cover, workgroups per tile block and sample)
        yield "forward %d->%d" % (Cin, Cout), (lambda B, a=(H, W, Cin, Cout): _fwd(B, *a)), H, W + 1 if pair else W, 2 if pair else 4 * (Cout // 64)
        yield "backward-data %d->%d" % (Cin, Cout), (lambda B, a=(H, W, Cin, Cout): _dgrad(B, *a)), H + 4, W + 4, Cin // 64


@pytest.mark.parametrize("name,make,Hm,Wm,per_block", list(_maps()), ids=[m[0] for m in _maps()])
@pytest.mark.parametrize("B", [1, 8, 32])
def test_sixteen_tile_block_covers_the_map_with_no_more_padding(name, make, Hm, Wm, per_block, B):
    d = make(B)
    assert Hh.lib().ramnet_fold_halfwg_variant(C.byref(d), 1) == 1
    r16, c16, n16 = _grid(d, 1)
    r32, c32, n32 = _grid(d, 0)
    assert (r16, c16) in BLOCKS16 and (r32, c32) in BLOCKS32
    by16, bx16, by32, bx32 = _cdiv(Hm, r16), _cdiv(Wm, c16), _cdiv(Hm, r32), _cdiv(Wm, c32)
    assert by16 * r16 >= Hm and bx16 * c16 >= Wm                          # the blocks cover the map
    assert n16 == by16 * bx16 * B * per_block and n32 == by32 * bx32 * B * per_block      # grid = block count x batch x channel blocks x classes
    area16, area32 = by16 * bx16 * r16 * c16, by32 * bx32 * r32 * c32
    assert area16 <= area32
    # the least padding among the four 16-tile shapes
    assert area16 == min(_cdiv(Hm, r) * r * _cdiv(Wm, c) * c for r, c in BLOCKS16)


def test_padded_area_never_exceeds_the_32_tile_block_on_any_small_map():
    for H in range(2, 41):
        for W in range(2, 60):
            d = _fwd(1, H, W, 64, 64)
            r16, c16, n16 = _grid(d, 1)
            r32, c32, n32 = _grid(d, 0)
            assert n16 * r16 * c16 <= n32 * r32 * c32, (H, W)
            assert _cdiv(H, r16) * _cdiv(W, c16) * 4 == n16, (H, W)


def test_variant_query_refuses_what_the_half_workgroup_is_not_built_for():
    L = Hh.lib()
    before = L.ramnet_last_error()
    assert L.ramnet_fold_halfwg_variant(None, 1) == 0
    for Cin, Cout, H, W in DECODERS:
        for make in (_fwd, _dgrad):
            assert L.ramnet_fold_halfwg_variant(C.byref(make(8, H, W, Cin, Cout)), 1) == 1
            # F(2x2,4x4) launches stay what they are
            assert L.ramnet_fold_halfwg_variant(C.byref(make(8, H, W, Cin, Cout, Hh.ALGO_WINOGRAD24)), 1) == 0
        # a split reduction (a workspace on the descriptor): the existing kernels
        d = _fwd(8, H, W, Cin, Cout)
        d.splitk_ws, d.splitk_floats = C.c_void_p(256), 1 << 20
        assert L.ramnet_fold_halfwg_variant(C.byref(d), 1) == 0
    # NCQ = 2 (32-column workgroups, chunks of 8): 32 output channels without the pair form, and reductions that are no multiple of 32
    assert L.ramnet_fold_halfwg_variant(C.byref(_fwd(8, 32, 43, 48, 32)), 1) == 0
    assert L.ramnet_fold_halfwg_variant(C.byref(_fwd(8, 32, 43, 16, 32)), 1) == 0
    old = L.ramnet_get_option(b"fold_pair")
    try:
        assert L.ramnet_set_option(b"fold_pair", 0) == 0
        assert L.ramnet_fold_halfwg_variant(C.byref(_fwd(8, 128, 172, 64, 32)), 1) == 0
    finally:
        assert L.ramnet_set_option(b"fold_pair", old) == 0
    assert L.ramnet_fold_halfwg_variant(C.byref(_fwd(8, 128, 172, 64, 32)), 1) == 1
    # other input modes and strides
    d = _fwd(8, 32, 43, 256, 128)
    d.in_mode = Hh.IN_CAT
    assert L.ramnet_fold_halfwg_variant(C.byref(d), 1) == 0
    d = _fwd(8, 32, 43, 256, 128)
    d.stride = 2
    assert L.ramnet_fold_halfwg_variant(C.byref(d), 1) == 0
    assert L.ramnet_last_error() == before                                  # asking is quiet
    r, c, n = C.c_int(), C.c_int(), C.c_long()
    assert L.ramnet_fold_halfwg_grid(C.byref(d), 1, C.byref(r), C.byref(c), C.byref(n)) == 10001      # no grid for what is refused


def test_option_selects_and_auto_keeps_batch_one_on_the_eight_wave_kernels():
    L = Hh.lib()
    old = L.ramnet_get_option(b"fold_half_wg")
    assert old in (0, 2)                                                   # never "force" by default
    d8, d1 = _fwd(8, 64, 86, 128, 64), _fwd(1, 64, 86, 128, 64)
    try:
        assert L.ramnet_set_option(b"fold_half_wg", 3) == 10001 and L.ramnet_set_option(b"fold_half_wg", -1) == 10001
        assert L.ramnet_get_option(b"fold_half_wg") == old
        assert L.ramnet_set_option(b"fold_half_wg", 0) == 0
        assert L.ramnet_fold_halfwg_variant(C.byref(d8), 0) == 0 and L.ramnet_fold_halfwg_variant(C.byref(d8), 1) == 1
        assert L.ramnet_set_option(b"fold_half_wg", 1) == 0
        assert L.ramnet_fold_halfwg_variant(C.byref(d8), 0) == 1 and L.ramnet_fold_halfwg_variant(C.byref(d1), 0) == 1
        assert L.ramnet_set_option(b"fold_half_wg", 2) == 0
        for Cin, Cout, H, W in DECODERS:
            assert L.ramnet_fold_halfwg_variant(C.byref(_fwd(1, H, W, Cin, Cout)), 0) == 0
            assert L.ramnet_fold_halfwg_variant(C.byref(_dgrad(1, H, W, Cin, Cout)), 0) == 0
    finally:
        assert L.ramnet_set_option(b"fold_half_wg", old) == 0
