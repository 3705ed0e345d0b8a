"""No GPU: the host side of the deterministic mode — the new entry points are declared and exported under ABI 27, ramnet_wgrad_slabs answers
the split rules of the launchers (host arithmetic, no device), the switch of rpg_ramnet_amd.ops round-trips and refuses what contradicts it,
and the restatement of the ordered slab join (tests/deterministic_cases.py) stands on a hand-computed example whose result depends on the
order."""
import ctypes as C
import os
import re

import pytest
import torch

import conv_restatement as cr
import deterministic_cases as dc
import fold_head_cases as fh
from rpg_ramnet_amd import _hip

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ramnet_hip.h")
NEW = ["ramnet_wgrad_slabs", "ramnet_gemm_partial_floats", "ramnet_gemm_ordered", "ramnet_gemm2_ordered", "ramnet_bias_grad_partial_floats",
       "ramnet_bias_grad_ordered", "ramnet_pred_bwd_partial_floats", "ramnet_pred_sigmoid_bwd_ordered", "ramnet_pred_linear_bwd_ordered",
       "ramnet_voxelize_batch_sorted", "ramnet_nonzero_stats_scratch_doubles", "ramnet_nonzero_stats_batch_ordered", "ramnet_normalize_nonzero_batch_ordered",
       "ramnet_normalize_nonzero_ordered"]


def test_header_declares_the_entry_points_and_the_abi_version_stays():
    with open(HEADER) as f:
        src = f.read()
    L = _hip.lib()
    for name in NEW:
        assert re.search(r"\b(int|size_t) %s\(" % name, src), name
        assert name in _hip.EXPORTS and getattr(L, name) is not None
    assert int(re.search(r"#define RAMNET_WGRAD_SLAB_CAP (\d+)", src).group(1)) == dc.SLAB_CAP
    assert "#define RAMNET_ABI_VERSION 27 " in src and L.ramnet_abi_version() == 27
    # no field was added to the descriptor: 8 pointers, 26 ints, 2 x 25 tap bytes, 2 + 4 bytes of padding in front of the pointers that follow them
    assert C.sizeof(_hip.WgradDesc) == 8 * 8 + 26 * 4 + 50 + 6 == 224


def _desc(**f):
    d = _hip.WgradDesc()
    for k, v in f.items():
        if isinstance(v, list):
            for j, e in enumerate(v):
                getattr(d, k)[j] = e
        else:
            setattr(d, k, v)
    return d


def _slabs(**f):
    return _hip.lib().ramnet_wgrad_slabs(C.byref(_desc(**f)))


@pytest.mark.parametrize("fam", sorted(dc.FOLD_FAMS))
@pytest.mark.parametrize("row", dc.FOLD_ROWS, ids=lambda r: "B%d-%dx%d-%d_%d" % r[:5])
def test_decoder_rows_answer_the_split_rule(fam, row):
    B, H, W, C0, Cout, want = row
    wci = Cout % 64 != 0
    tiles = -(-W // (3 if fam == "fold2x3" else 2)) * -(-H // 2) * B
    nbatch = -(-tiles // (6 if fam == "fold2x3" else 8))
    rule = max(1, min(256 // ((C0 // (64 if wci else 32)) * -(-Cout // (32 if wci else 64)) * 4), nbatch))      # `splits` of launch_wgrad_wino24
    got = _slabs(algo=dc.FOLD_FAMS[fam], in_mode=_hip.IN_PLAIN, stride=1, B=B, Hin=H + 4, Win=W + 4, Ho=H, Wo=W, HoG=2 * H, WoG=2 * W, C0=C0, Cout=Cout, ntaps=16)
    assert got == rule == want


def test_decoder_shapes_the_kernel_does_not_take_answer_zero():
    base = dict(algo=_hip.ALGO_WINOGRAD24, in_mode=_hip.IN_PLAIN, stride=1, B=2, Hin=10, Win=11, Ho=6, Wo=7, HoG=12, WoG=14, ntaps=16)
    assert _slabs(**base, C0=32, Cout=64) == 3
    assert _slabs(**base, C0=16, Cout=64) == 0 and _slabs(**base, C0=32, Cout=48) == 0 and _slabs(**base, C0=32, Cout=32) == 0
    assert _hip.lib().ramnet_wgrad_slabs(None) == 0


@pytest.mark.parametrize("c", dc.HEAD_ROWS, ids=lambda c: c.name)
def test_head_rows_stay_below_the_cap(c):
    taps = fh.HEAD_TAPS
    got = _slabs(algo=_hip.ALGO_HEAD, head_cin=c.cin, in_mode=_hip.IN_PLAIN, stride=1, B=c.B, Hin=c.H, Win=c.W, Ho=c.H, Wo=c.W, C0=c.C0, Cout=c.Cout,
                 ntaps=25, dy=[t[0] for t in taps], dx=[t[1] for t in taps])
    tiles = -(-c.W // 32) * -(-c.H // 8) * c.B
    assert got == min(tiles, dc.SLAB_CAP) and 1 <= got <= dc.SLAB_CAP
    assert (tiles > dc.SLAB_CAP) == (c.name == "det_cin1_75tiles")
    assert _slabs(algo=_hip.ALGO_HEAD, head_cin=2, in_mode=_hip.IN_PLAIN, stride=1, B=1, Hin=8, Win=8, Ho=8, Wo=8, C0=4, Cout=32, ntaps=25) == 0


@pytest.mark.parametrize("name", dc.DIRECT_ROWS)
def test_direct_rows_stay_below_the_cap(name):
    d = dc.build_direct(name)
    f = dict(algo=_hip.ALGO_DIRECT, in_mode=d.in_mode, stride=d.stride, B=d.B, Hin=d.Hin, Win=d.Win, Ho=d.Ho, Wo=d.Wo, C0=d.C0, C1=d.C1, Cout=d.Cout,
             ntaps=len(d.taps), dy=[t[0] for t in d.taps], dx=[t[1] for t in d.taps])
    if d.gview:
        f.update(zip(("gsy", "gsx", "goy", "gox", "HoG", "WoG"), d.gview))
    got = _slabs(**f)
    assert 2 <= got <= dc.SLAB_CAP                  # (every row has at least two pixel tiles: its launch really splits)
    # pixel tiles of TH x 16, TH = 8, or 4 where the patch of an 8-row tile and the gradient tile pass 80 KB (the 5 x 5 at stride 2: 19 x 35 x 32 floats)
    ext = max(t[0] for t in d.taps) - min(t[0] for t in d.taps)
    th = 4 if ((7 * d.stride + ext + 1) * (15 * d.stride + ext + 1) * 32 + 128 * 32) * 4 > 80 * 1024 else 8
    assert th == (4 if name == "k5_s2_cat" else 8)
    assert got == min(dc.SLAB_CAP, -(-d.Wo // 16) * -(-d.Ho // th) * d.B)
    big = dict(f, B=64, Ho=256, Wo=344, Hin=256 * d.stride, Win=344 * d.stride)
    assert _slabs(**big) == dc.SLAB_CAP


def test_families_without_a_slab_form_answer_zero_and_the_3x3_families_their_own_counts():
    L = _hip.lib()
    taps = [(a - 1, b - 1) for a in range(3) for b in range(3)]
    f = dict(in_mode=_hip.IN_CAT, stride=1, B=2, Hin=9, Win=11, Ho=9, Wo=11, C0=32, C1=8, Cout=64, ntaps=9, dy=[t[0] for t in taps], dx=[t[1] for t in taps])
    assert _slabs(algo=_hip.ALGO_WINOGRAD, **f) == L.ramnet_wgrad_wino_slabs(40, 64) >= 1
    assert _slabs(algo=_hip.ALGO_WINOGRAD_2X4, **f) == L.ramnet_wgrad_wino2x4_slabs(40, 64) >= 1
    assert _slabs(algo=_hip.ALGO_DIRECT_SPLIT, **f) == L.ramnet_wgrad_dsplit_slabs(40, 64) >= 1
    s2d = dict(f, in_mode=_hip.IN_S2D, C1=0)
    assert _slabs(algo=_hip.ALGO_WINOGRAD, **s2d) == L.ramnet_wgrad_wino_slabs(128, 64)
    assert _slabs(algo=_hip.ALGO_WINOGRAD_2X4_SPLIT, **f) == 0 and _slabs(algo=99, **f) == 0      # (no backward-weights form of that algorithm)


def test_partial_buffer_sizes():
    L = _hip.lib()
    # K >= 256 is where an accumulating launch starts to split: 2 entries x 1 x 2 blocks -> 4 slices of 128 at K = 512
    assert L.ramnet_gemm_partial_floats(10, 64, 512, 2, 0, 0, 0) == 2 * 4 * 32 * 64
    assert L.ramnet_gemm_partial_floats(10, 64, 252, 2, 0, 0, 0) == 0
    assert L.ramnet_gemm_partial_floats(10, 64, 64, 2, 40, 512, 1) == 3 * 4 * 64 * 64
    assert L.ramnet_bias_grad_partial_floats(32) == 256 * 32 and L.ramnet_pred_bwd_partial_floats() == 512 * 132
    assert L.ramnet_nonzero_stats_scratch_doubles(3, 1200) == 3 * 3 * 2


def test_ordered_join_depends_on_the_order_and_follows_reduce_slabs():
    """1 + 2^-24 rounds back to 1 (ties to even) and so does the next + 2^-24; 2^-24 + 2^-24 = 2^-23 is exact and 2^-23 + 1 is representable:
    the fold in slab order gives 1 for (1, 2^-24, 2^-24) and 1 + 2^-23 for (2^-24, 2^-24, 1)"""
    e = 2.0 ** -24
    a = torch.tensor([[1.0], [e], [e]], dtype=torch.float64)
    assert float(dc.ordered_join(a)[0]) == 1.0
    assert float(dc.ordered_join(a.flip(0))[0]) == 1.0 + 2.0 ** -23
    assert float(dc.accumulate(torch.tensor([1.0 + 2.0 ** -23]), 3)[0]) == 3.0 + 2.0 ** -21       # (2 + 2^-22) + (1 + 2^-23): the tie rounds up to even


def test_fold_rows_are_what_the_issue_states():
    for B, H, W, C0, Cout, S in dc.FOLD_ROWS:
        d = dc.build_fold("fold2x2", (B, H, W, C0, Cout, S), True)
        assert d.x0.shape == (B, H + 4, W + 4, C0) and d.dout.shape == d.gmask.shape == (B, 2 * H, 2 * W, Cout)
    assert cr.FOLD_TW == {"fold2x2": 2, "fold2x3": 3}


def test_the_switch_round_trips_and_the_conflicting_settings_raise():
    from rpg_ramnet_amd import ops
    assert ops.deterministic() is False             # off by default
    with ops.switches(wgrad_slabs=True, grad_loss_batched=True, deterministic=False):       # (the body's own changes are put back as well)
        ops.set_deterministic(True)
        assert ops.deterministic() is True
        for setter in (ops.set_wgrad_slabs, ops.set_grad_loss_batched):
            with pytest.raises(RuntimeError, match="deterministic"):
                setter(False)
            setter(True)
        with pytest.raises(RuntimeError, match="mse_loss"):
            ops.not_deterministic("mse_loss")
        ops.set_deterministic(False)
        assert ops.deterministic() is False
        ops.not_deterministic("anything")           # silent outside the mode
        for setter in (ops.set_wgrad_slabs, ops.set_grad_loss_batched):
            setter(False)
            try:
                with pytest.raises(RuntimeError):
                    ops.set_deterministic(True)
                assert ops.deterministic() is False
            finally:
                setter(True)


def test_the_trainer_key_is_read_and_defaults_to_false():
    from rpg_ramnet_amd import ops, trainer
    with ops.switches(deterministic=ops.deterministic()):           # (what the trainer sets is put back)
        assert trainer.apply_deterministic_config({"trainer": {}}) is False and trainer.apply_deterministic_config({}) is False
        assert trainer.apply_deterministic_config({"trainer": {"deterministic": True}}) is True and ops.deterministic()
