"""No GPU: the host-only entry points behind the ConvLSTM launches of the F(2x4,3x3) family (ABI 27; csrc/conv_wino6.hip) — which
RAMNET_EPI_LSTM descriptors ramnet_conv_wino_variant() accepts, the ONE size rule, the size of the gate-interleaved pack."""
import ctypes
import os
import re

import pytest

from rpg_ramnet_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lstm_desc(C=64, B=2, Hh=32, W=48, **over):
    """A well-formed ConvLSTM cell descriptor as ops.LSTMCell builds it (dummy 16-byte aligned non-null pointers: nothing is launched)."""
    d = _hip.ConvDesc()
    d.x0, d.x1, d.w, d.bias, d.out, d.o1, d.o2, d.e1 = 4096, 8192, 12288, 16384, 20480, 24576, 28672, 32768
    d.ld0, d.ld1, d.C0, d.C1, d.in_mode = C, C, C, C, _hip.IN_CAT
    d.B, d.Hin, d.Win, d.Ho, d.Wo, d.HoF, d.WoF = B, Hh, W, Hh, W, Hh, W
    d.ntaps, d.stride = 9, 1
    for t in range(9):
        d.dy[t], d.dx[t], d.wtap[t] = t // 3 - 1, t % 3 - 1, t
    d.Cout, d.ldo, d.ldo1, d.ldo2, d.lde1 = C, C, C, 4 * C, C
    d.osy, d.osx = 1, 1
    d.epi, d.algo = _hip.EPI_LSTM, _hip.ALGO_WINOGRAD
    for k, v in over.items():
        setattr(d, k, v)
    return d


def variant(d, force):
    return _hip.lib().ramnet_conv_wino_variant(ctypes.byref(d), force)


def test_abi_version_27():
    hdr = open(os.path.join(ROOT, "include", "ramnet_hip.h")).read()
    assert int(re.search(r"#define RAMNET_ABI_VERSION (\d+)", hdr).group(1)) == 27
    assert _hip.lib().ramnet_abi_version() == 27


def test_lstm_descriptor_is_eligible_when_well_formed():
    assert variant(lstm_desc(), 1) == 1
    assert variant(lstm_desc(C=16), 1) == 1                      # 4C = 64: one block
    assert variant(lstm_desc(o2=None, ldo2=0), 1) == 1           # inference: no gates
    assert variant(lstm_desc(e1=None, lde1=0), 1) == 1           # zero cell state
    assert variant(lstm_desc(e0=36864, lde0=64), 1) == 1         # masked launches pass h


@pytest.mark.parametrize("what,over", [
    ("hidden size 24", dict(Cout=24, C0=24, C1=24, ld0=24, ld1=24, ldo=24, ldo1=24, ldo2=96, lde1=24)),
    ("C0 = 36", dict(C0=36, ld0=36)),
    ("misaligned o1", dict(o1=24576 + 4)),
    ("misaligned o2", dict(o2=28672 + 8)),
    ("misaligned bias", dict(bias=16384 + 4)),
    ("in_mode PLAIN", dict(in_mode=_hip.IN_PLAIN)),
    ("out_s2d", dict(out_s2d=16)),
    ("no o1", dict(o1=None)),
    ("no bias", dict(bias=None)),
    ("output stride", dict(osy=2, osx=2)),
    ("frame", dict(frame=2)),
])
def test_lstm_descriptor_single_violations(what, over):
    assert variant(lstm_desc(**over), 1) == 0, what


def test_split_operands_never_take_the_cell():
    L = _hip.lib()
    assert L.ramnet_conv_wino_split_ok(ctypes.byref(lstm_desc()), 1) == 0
    d = lstm_desc(Cout=256, epi=_hip.EPI_SIGMOID)                # the same launch as a plain gate convolution: accepted
    assert L.ramnet_conv_wino_split_ok(ctypes.byref(d), 1) == 1


@pytest.mark.parametrize("B", [1, 2, 8])
@pytest.mark.parametrize("C,Hh,W", [(64, 128, 172), (128, 64, 86), (256, 32, 43)])
def test_one_size_rule(B, C, Hh, W):
    """Without force the answer for a ConvLSTM cell of hidden size C equals the answer for the same launch as a RAMNET_EPI_SIGMOID
    convolution with Cout = 4C: the existing rule on the 4C gate columns.  At B = 8: 2816 / 1408 / 768 workgroups against 150."""
    lstm = variant(lstm_desc(C=C, B=B, Hh=Hh, W=W), 0)
    sig = variant(lstm_desc(C=C, B=B, Hh=Hh, W=W, epi=_hip.EPI_SIGMOID, Cout=4 * C, ldo=4 * C, o1=None, o2=None, ldo1=0, ldo2=0, e1=None, lde1=0), 0)
    assert lstm == sig
    if B == 8:
        assert lstm == 1
    if B == 1:                                                   # 352 / 176 / 96 workgroups
        assert lstm == (1 if C < 256 else 0)


def test_launch_rejects_bad_lstm_descriptors_before_any_hip_call():
    L = _hip.lib()
    d = lstm_desc(in_mode=_hip.IN_PLAIN, x1=None, C1=0, algo=_hip.ALGO_WINOGRAD_2X4)
    assert L.ramnet_conv_launch(ctypes.byref(d), None) == 10001 and b"bad argument" in L.ramnet_last_error()
    d = lstm_desc(C=24, algo=_hip.ALGO_WINOGRAD_2X4)
    assert L.ramnet_conv_launch(ctypes.byref(d), None) == 10001
    d = lstm_desc(algo=_hip.ALGO_WINOGRAD_2X4_SPLIT)             # the split-operand kernel has no cell epilogue
    assert L.ramnet_conv_launch(ctypes.byref(d), None) == 10001
    d = lstm_desc(algo=_hip.ALGO_WINOGRAD_2X4, active=40960)     # masked without e0 = h
    assert L.ramnet_conv_launch(ctypes.byref(d), None) == 10001


@pytest.mark.parametrize("C", [16, 64, 128, 256])
def test_gate_pack_size(C):
    L = _hip.lib()
    n = L.ramnet_packed_weight_elems_wino2x4_gates(4 * C, 2 * C, 0, 4)
    assert n == L.ramnet_packed_weight_elems_wino2x4(4 * C, 2 * C, 0)
    assert n == (2 * C // 8) * (4 * C // 64) * 24 * 64 * 8
    assert L.ramnet_packed_weight_elems_wino2x4_gates(4 * C, 2 * C, 0, 1) == n
    # the pack refuses what the kernel cannot read (host checks, no HIP call): transposed or ragged gate packs
    assert L.ramnet_pack_weight_wino2x4_gates(4096, 8192, 4 * C, 2 * C, 1, 4, None) == 10001
    assert L.ramnet_pack_weight_wino2x4_gates(4096, 8192, 96, 48, 0, 4, None) == 10001
