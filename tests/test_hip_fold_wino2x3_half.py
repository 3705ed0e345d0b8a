"""GPU: the half-workgroup form of the F(2x3,4x4) decoder launches (conv_wino24_kernel<4, .., 3, HALF>: 4 waves, 16 tiles, two workgroups
per CU; ramnet_set_option("fold_half_wg")) against the 8-wave launch of the SAME raw descriptor, bit for bit — a wave runs the same
tiles' arithmetic in the same chunk and MFMA order, only the tile blocks and the LDS plane differ — for the forward, pair and
backward-data launches of the three decoder layers on maps with one partial block, blocks that hang over both edges, and the bench's
ragged width; with the border frame, bias and ReLU of the forward epilogue; and with nothing written outside the map."""
import ctypes as C

import pytest
import torch

from rpg_ramnet_amd import _hip as Hh

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 4), (2, 9, 13), (1, 32, 43)]           # B, H, W (low resolution)
DEV = "cuda:0"


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture
def half_option():
    """set(mode) selects the form; the option is restored afterwards."""
    L = Hh.lib()
    old = L.ramnet_get_option(b"fold_half_wg")

    def set_mode(v):
        assert L.ramnet_set_option(b"fold_half_wg", v) == 0

    yield set_mode
    assert L.ramnet_set_option(b"fold_half_wg", old) == 0


_PACKS = {}


def _pack(Cin, Cout, dgrad):
    """Packed F(2x3) weights of a layer, made once per module run."""
    key = (Cin, Cout, dgrad)
    if key not in _PACKS:
        L = Hh.lib()
        g = torch.Generator(device="cpu").manual_seed(17 + Cin + dgrad)
        w = (torch.randn(Cout, Cin, 5, 5, generator=g) * 0.1).to(DEV)
        wp = torch.empty(L.ramnet_packed_weight_elems_fold_wino2x3(Cout, Cin), device=DEV)
        fn = L.ramnet_pack_weight_fold_wino2x3_dgrad if dgrad else L.ramnet_pack_weight_fold_wino2x3
        assert fn(ptr(w), ptr(wp), Cout, Cin, None) == 0, L.ramnet_last_error()
        _PACKS[key] = wp
    return _PACKS[key]


def _fwd_desc(x, wp, bias, e0, e1, y, ldo, B, H, W, Cin, Cout, relu):
    d = Hh.ConvDesc()
    d.x0, d.ld0, d.C0, d.in_mode = ptr(x), Cin, Cin, Hh.IN_PLAIN
    d.B, d.Hin, d.Win, d.stride, d.ntaps = B, H + 4, W + 4, 1, 16
    d.w, d.bias, d.Cout = ptr(wp), ptr(bias), Cout
    d.Ho, d.Wo, d.HoF, d.WoF = H, W, 2 * H, 2 * W
    d.osy, d.osx = 1, 1
    d.frame, d.e0, d.e1, d.lde0, d.lde1 = 2, ptr(e0), ptr(e1), 2 * Cout, 2 * Cout
    d.epi, d.out, d.ldo, d.algo = (Hh.EPI_RELU if relu else Hh.EPI_LINEAR), ptr(y), ldo, Hh.ALGO_WINOGRAD24_2X3
    return d


def _dgrad_desc(g, wp, dx, ldo, B, H, W, Cin, Cout):
    d = Hh.ConvDesc()
    d.x0, d.ld0, d.C0, d.in_mode = ptr(g), Cout, Cout, Hh.IN_PARITY4
    d.B, d.Hin, d.Win, d.stride, d.ntaps = B, 2 * H, 2 * W, 1, 16
    d.w, d.Cout = ptr(wp), Cin
    d.Ho, d.Wo, d.HoF, d.WoF = H + 4, W + 4, H + 4, W + 4
    d.osy, d.osx = 1, 1
    d.epi, d.out, d.ldo, d.algo = Hh.EPI_LINEAR, ptr(dx), ldo, Hh.ALGO_WINOGRAD24_2X3
    return d


GUARD = 4096          # floats in front of and behind the output tensor


def _both(make_desc, out_shape, set_mode, want_prefix, pad=0):
    """Launch the descriptor on the 8-wave and on the half-workgroup kernel, each into its own buffer pre-filled with the same garbage;
    returns the two whole buffers as int32 (guards and row gaps included) and the garbage."""
    L = Hh.lib()
    n = 1
    for s in out_shape[:-1]:
        n *= s
    ldo = out_shape[-1] + pad
    gen = torch.Generator(device="cpu").manual_seed(99)
    garbage = torch.randint(-2 ** 31, 2 ** 31 - 1, (2 * GUARD + n * ldo,), generator=gen, dtype=torch.int64).to(torch.int32).to(DEV)
    bufs = []
    for mode, suffix in ((0, b",3>"), (1, b",3,1>")):
        buf = garbage.clone()
        out = buf.view(torch.float32)[GUARD:GUARD + n * ldo]
        d = make_desc(out, ldo)
        set_mode(mode)
        assert L.ramnet_fold_halfwg_variant(C.byref(d), 0) == mode
        assert L.ramnet_conv_launch(C.byref(d), None) == 0, L.ramnet_last_error()
        k = L.ramnet_last_kernel()
        assert k.startswith(want_prefix) and k.endswith(suffix), k
        torch.cuda.synchronize()
        bufs.append(buf)
    return bufs[0], bufs[1], garbage, n, ldo


def _check(ref, got, garbage, n, ldo, cout):
    assert torch.equal(ref, got)                                            # bit-identical, guards and gaps included
    body = got[GUARD:GUARD + n * ldo].view(n, ldo)
    gb = garbage[GUARD:GUARD + n * ldo].view(n, ldo)
    assert torch.equal(got[:GUARD], garbage[:GUARD]) and torch.equal(got[GUARD + n * ldo:], garbage[GUARD + n * ldo:])
    assert torch.equal(body[:, cout:], gb[:, cout:])                        # the gap of every pixel row
    vals = body[:, :cout].contiguous().view(torch.float32)
    assert bool(torch.isfinite(vals).all())
    assert bool((body[:, :cout] != gb[:, :cout]).any(dim=1).all())          # every pixel of the map was written
    return vals


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("Cin,Cout", [(256, 128), (128, 64), (64, 32)], ids=["256-128", "128-64", "64-32pair"])
def test_forward_half_workgroup_is_bit_identical(Cin, Cout, B, H, W, relu, half_option):
    """Forward (Cout = 32: the pair form) with frame = 2 and random e0 / e1, bias, ReLU on and off."""
    torch.manual_seed(B * 1000 + H * 10 + W)
    x = torch.randn(B, H + 4, W + 4, Cin, device=DEV)
    bias = torch.randn(Cout, device=DEV) * 0.1
    e0 = torch.randn(2, B, 2 * H, 2 * Cout, device=DEV)
    e1 = torch.randn(2, B, 2 * W, 2 * Cout, device=DEV)
    wp = _pack(Cin, Cout, False)
    ref, got, garbage, n, ldo = _both(lambda out, ldo: _fwd_desc(x, wp, bias, e0, e1, out, ldo, B, H, W, Cin, Cout, relu),
                                      (B, 2 * H, 2 * W, Cout), half_option, b"conv_wino24_kernel<4,0,")
    vals = _check(ref, got, garbage, n, ldo, Cout)
    if relu:
        assert float(vals.min()) == 0.0
    else:
        assert float(vals.min()) < 0.0
    assert (b",1,3" in Hh.lib().ramnet_last_kernel()) == (Cout == 32)      # the pair form for 32 output channels


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("Cin,Cout", [(256, 128), (128, 64), (64, 32)], ids=["256-128", "128-64", "64-32"])
def test_backward_data_half_workgroup_is_bit_identical(Cin, Cout, B, H, W, half_option):
    """Backward-data: the gradient of the padded low-resolution input, a dense (H + 4) x (W + 4) grid."""
    torch.manual_seed(B * 1000 + H * 10 + W + 1)
    g = torch.randn(B, 2 * H, 2 * W, Cout, device=DEV)
    wp = _pack(Cin, Cout, True)
    ref, got, garbage, n, ldo = _both(lambda out, ldo: _dgrad_desc(g, wp, out, ldo, B, H, W, Cin, Cout), (B, H + 4, W + 4, Cin), half_option,
                                      b"conv_wino24_kernel<4,1,")
    _check(ref, got, garbage, n, ldo, Cin)


@pytest.mark.parametrize("direction", ["forward", "pair", "backward-data"])
def test_nothing_outside_the_map_is_written(direction, half_option):
    """Blocks hang over the 9 x 13 map in both directions and the rows of the output tensor have a gap (ldo = channels + 4): the guard
    floats around the tensor and the gaps keep their garbage, every pixel of the map is written."""
    B, H, W = 2, 9, 13
    Cin, Cout = (64, 32) if direction == "pair" else (128, 64)
    torch.manual_seed(7)
    if direction == "backward-data":
        g = torch.randn(B, 2 * H, 2 * W, Cout, device=DEV)
        wp = _pack(Cin, Cout, True)
        ref, got, garbage, n, ldo = _both(lambda out, ldo: _dgrad_desc(g, wp, out, ldo, B, H, W, Cin, Cout), (B, H + 4, W + 4, Cin),
                                          half_option, b"conv_wino24_kernel<4,1,", pad=4)
        _check(ref, got, garbage, n, ldo, Cin)
        return
    x = torch.randn(B, H + 4, W + 4, Cin, device=DEV)
    bias = torch.randn(Cout, device=DEV) * 0.1
    e0 = torch.randn(2, B, 2 * H, 2 * Cout, device=DEV)
    e1 = torch.randn(2, B, 2 * W, 2 * Cout, device=DEV)
    wp = _pack(Cin, Cout, False)
    ref, got, garbage, n, ldo = _both(lambda out, ldo: _fwd_desc(x, wp, bias, e0, e1, out, ldo, B, H, W, Cin, Cout, False),
                                      (B, 2 * H, 2 * W, Cout), half_option, b"conv_wino24_kernel<4,0,", pad=4)
    _check(ref, got, garbage, n, ldo, Cout)


def test_forward_half_workgroup_matches_float64_away_from_the_border(half_option):
    """One absolute anchor: the half-workgroup forward against conv5x5(bilinear_x2(x)) in float64 away from the border (the frame
    needs the border GEMMs), with the bound of tests/test_hip_fold_wino2x3.py's raw-descriptor test."""
    import torch.nn.functional as F
    L = Hh.lib()
    torch.manual_seed(13)
    B, H, W, Cin, Cout = 2, 9, 14, 128, 64
    x = torch.randn(B, H, W, Cin, device=DEV)
    w = torch.randn(Cout, Cin, 5, 5, device=DEV) * 0.1
    b = torch.randn(Cout, device=DEV) * 0.1
    wp = torch.empty(L.ramnet_packed_weight_elems_fold_wino2x3(Cout, Cin), device=DEV)
    assert L.ramnet_pack_weight_fold_wino2x3(ptr(w), ptr(wp), Cout, Cin, None) == 0
    xpad = torch.empty(B, H + 4, W + 4, Cin, device=DEV)
    assert L.ramnet_pad2_sum(ptr(x), None, ptr(xpad), B, H, W, Cin, None) == 0
    y = torch.zeros(B, 2 * H, 2 * W, Cout, device=DEV)
    d = _fwd_desc(xpad, wp, b, None, None, y, Cout, B, H, W, Cin, Cout, False)
    d.frame, d.lde0, d.lde1 = 0, 0, 0
    half_option(1)
    assert L.ramnet_conv_launch(C.byref(d), None) == 0, L.ramnet_last_error()
    assert L.ramnet_last_kernel().endswith(b",3,1>")
    xr = x.permute(0, 3, 1, 2).cpu().double()
    ref = F.conv2d(F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=False), w.cpu().double(), b.cpu().double(), 1, 2)
    got = y.permute(0, 3, 1, 2).cpu().double()
    assert float((got - ref)[:, :, 2:-2, 2:-2].abs().max() / ref.abs().max()) < 2e-5
