"""GPU: F(2x3,4x4) folded decoders (RAMNET_ALGO_WINOGRAD24_2X3, conv_wino24_kernel<.., TW = 3>) forced on every eligible launch,
against the oracle; their packs against the torch statement (tests/test_fold_wino2x3_cpu.py); the raw C ABI; bit-reproducibility;
and the "auto" choice of ramnet_fold_wino_variant."""
import ctypes as C

import pytest
import torch

from oracle import ramnet_ref
from rpg_ramnet_amd import _hip as Hh
from test_fold_wino2x3_cpu import pack_fold_wino2x3, pack_fold_wino2x3_dgrad
from test_hip_ops import TOL, dev, run_pair
from util import assert_close, nchw, nhwc

pytestmark = pytest.mark.gpu


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture
def fold2x3():
    """The folded Winograd path (forward, backward-data through the folded adjoint, Winograd-domain backward-weights) with F(2x3,4x4)
    on every structurally eligible forward / backward-data launch; records which descriptors took it."""
    from rpg_ramnet_amd import ops
    with ops.switches(fold_upsample=True, fold_winograd=True, fold_winograd_wgrad=True, fold_dgrad=True, fold_winograd_2x3="force"):
        ops._DESC_CACHE.clear()
        yield ops


def _kinds(ops):
    return {v[1] for v in ops._DESC_CACHE.values()}


def _eligible(cin, cout):
    return cin % 32 == 0 and (cout % 64 == 0 or cout == 32)


@pytest.mark.parametrize("B,H,W", [(2, 8, 16), (1, 5, 11), (2, 16, 24), (1, 4, 4), (1, 32, 43)])
@pytest.mark.parametrize("cin,cout,skip", [(64, 32, True), (64, 32, False), (256, 128, True), (128, 64, True), (48, 64, False)])
def test_upsample_conv_2x3(B, H, W, cin, cout, skip, fold2x3):
    """Forward, dx, dskip, dW and db of every shape of test_hip_ops.test_upsample_conv (the pair form: cout = 32) on F(2x3)."""
    from rpg_ramnet_amd.model.submodules import UpsampleConvLayer
    torch.manual_seed(3)
    m = UpsampleConvLayer(cin, cout, 5, padding=2)
    x, s = torch.randn(B, cin, H, W), (torch.randn(B, cin, H, W) if skip else None)

    def oracle(sd, a, sk=None):
        return ramnet_ref.upsample_conv_layer({"L." + k: v for k, v in sd.items()}, "L", a if sk is None else a + sk)

    run_pair(m, oracle, [x, s] if skip else [x])
    if fold2x3._DESC_CACHE_ON and _eligible(cin, cout):
        assert {"f23", "f23d"} <= _kinds(fold2x3)


def test_upsample_conv_2x3_without_activation(fold2x3):
    """A linear folded layer (no ReLU) on F(2x3): forward and all four gradients against float64."""
    import torch.nn.functional as F
    ops = fold2x3
    torch.manual_seed(4)
    B, H, W, cin, cout = 2, 7, 10, 64, 64
    w = torch.nn.Parameter((torch.randn(cout, cin, 5, 5) * 0.05).to(dev()))
    b = torch.nn.Parameter((torch.randn(cout) * 0.1).to(dev()))
    cp = ops.ConvParam([w], [b])
    x, s = torch.randn(B, cin, H, W), torch.randn(B, cin, H, W)
    xg, sg = nhwc(x).to(dev()).requires_grad_(True), nhwc(s).to(dev()).requires_grad_(True)
    y = ops.ConvAct.apply(xg, sg, w, b, cp, 1, False, True)
    xr, sr = x.double().requires_grad_(True), s.double().requires_grad_(True)
    wr, br = w.detach().cpu().double().requires_grad_(True), b.detach().cpu().double().requires_grad_(True)
    ref = F.conv2d(F.interpolate(xr + sr, scale_factor=2, mode="bilinear", align_corners=False), wr, br, 1, 2)
    assert_close(nchw(y).detach().cpu().numpy(), ref.detach().numpy(), TOL, "linear upsample-conv forward")
    g = torch.randn(ref.shape)
    (ref * g.double()).sum().backward()
    (nchw(y) * g.to(dev())).sum().backward()
    assert_close(w.grad.cpu().numpy(), wr.grad.numpy(), TOL, "dW")
    assert_close(b.grad.cpu().numpy(), br.grad.numpy(), TOL, "db")
    assert_close(nchw(xg.grad).cpu().numpy(), xr.grad.numpy(), TOL, "dx")
    assert_close(nchw(sg.grad).cpu().numpy(), sr.grad.numpy(), TOL, "dskip")
    if ops._DESC_CACHE_ON:
        assert {"f23", "f23d"} <= _kinds(ops)


# the three decoder layers of the flagship workload (256 x 344 input, base 32 channels): (Cin, Cout, low-res H, W)
DECODERS = [(256, 128, 32, 43), (128, 64, 64, 86), (64, 32, 128, 172)]


@pytest.mark.parametrize("B", [8, 16])
@pytest.mark.parametrize("cin,cout,H,W", DECODERS)
def test_full_size_decoder_2x3(B, cin, cout, H, W, fold2x3):
    """The full-size decoder layers on F(2x3) against the float64 oracle (evaluated on the device): forward, dx, dskip, dW, db."""
    from rpg_ramnet_amd.model.submodules import UpsampleConvLayer
    torch.manual_seed(5)
    m = UpsampleConvLayer(cin, cout, 5, padding=2).to(dev())
    x, s = torch.randn(B, cin, H, W, device=dev()), torch.randn(B, cin, H, W, device=dev())
    xg, sg = nhwc(x).requires_grad_(True), nhwc(s).requires_grad_(True)
    y = m(xg, sg)
    sd = {"L." + k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}
    xr, sr = x.double().requires_grad_(True), s.double().requires_grad_(True)
    ref = ramnet_ref.upsample_conv_layer(sd, "L", xr + sr)
    assert_close(nchw(y).detach().cpu().numpy(), ref.detach().cpu().numpy(), TOL, "forward")
    g = torch.randn(ref.shape, device=dev())
    g[(nchw(y).detach() == 0) != (ref.detach() == 0)] = 0.0          # outputs on the ReLU kink (see test_hip_ops.run_pair)
    (ref * g.double()).sum().backward()
    (nchw(y) * g).sum().backward()
    assert_close(nchw(xg.grad).cpu().numpy(), xr.grad.cpu().numpy(), TOL, "dx")
    assert_close(nchw(sg.grad).cpu().numpy(), sr.grad.cpu().numpy(), TOL, "dskip")
    assert_close(m.conv2d.weight.grad.cpu().numpy(), sd["L.conv2d.weight"].grad.cpu().numpy(), TOL, "dW")
    assert_close(m.conv2d.bias.grad.cpu().numpy(), sd["L.conv2d.bias"].grad.cpu().numpy(), TOL, "db")
    if fold2x3._DESC_CACHE_ON:
        assert {"f23", "f23d"} <= _kinds(fold2x3)


@pytest.mark.parametrize("cin,cout", [(64, 32), (128, 64), (256, 128)])
def test_fold_wino2x3_packs_equal_their_torch_statements(cin, cout):
    from rpg_ramnet_amd import ops
    torch.manual_seed(3)
    w = (torch.randn(cout, cin, 5, 5) * 0.1).to(dev())
    L = Hh.lib()
    n = L.ramnet_packed_weight_elems_fold_wino2x3(cout, cin)
    assert n == 120 * cout * cin
    out = torch.empty(n, device=dev())
    Hh.check(L.ramnet_pack_weight_fold_wino2x3(ops._p(w), ops._p(out), cout, cin, ops._st()), "pack 2x3")
    assert_close(out.cpu().numpy(), pack_fold_wino2x3(w).cpu().numpy(), 1e-6, "fold 2x3 pack")
    Hh.check(L.ramnet_pack_weight_fold_wino2x3_dgrad(ops._p(w), ops._p(out), cout, cin, ops._st()), "pack 2x3 dgrad")
    assert_close(out.cpu().numpy(), pack_fold_wino2x3_dgrad(w).cpu().numpy(), 1e-6, "fold 2x3 dgrad pack")
    assert L.ramnet_pack_weight_fold_wino2x3(ops._p(w), ops._p(out), 32, 16, ops._st()) == 10001      # 32-channel chunks of 8: no F(2x3)


def _fwd_desc(xpad, wp, b, y, B, H, W, Cin, Cout, algo):
    d = Hh.ConvDesc()
    d.x0, d.ld0, d.C0, d.in_mode = ptr(xpad), Cin, Cin, Hh.IN_PLAIN
    d.B, d.Hin, d.Win, d.stride, d.ntaps = B, H + 4, W + 4, 1, 16
    d.w, d.bias, d.Cout = ptr(wp), ptr(b), Cout
    d.Ho, d.Wo, d.HoF, d.WoF = H, W, 2 * H, 2 * W
    d.osy, d.osx = 1, 1
    d.epi, d.out, d.ldo, d.algo = Hh.EPI_LINEAR, ptr(y), Cout, algo
    return d


def _dgrad_desc(g, wp, dxpad, B, H, W, Cin, Cout, algo):
    d = Hh.ConvDesc()
    d.x0, d.ld0, d.C0, d.in_mode = ptr(g), Cout, Cout, Hh.IN_PARITY4
    d.B, d.Hin, d.Win, d.stride, d.ntaps = B, 2 * H, 2 * W, 1, 16
    d.w, d.Cout = ptr(wp), Cin
    d.Ho, d.Wo, d.HoF, d.WoF = H + 4, W + 4, H + 4, W + 4
    d.osy, d.osx = 1, 1
    d.epi, d.out, d.ldo, d.algo = Hh.EPI_LINEAR, ptr(dxpad), Cin, algo
    return d


@pytest.mark.parametrize("Cin,Cout", [(64, 32), (128, 64)])
def test_folded_upsample_conv_2x3_through_raw_descriptors(Cin, Cout):
    """RAMNET_ALGO_WINOGRAD24_2X3 with raw descriptors: forward away from the border against torch in float64, backward-data against
    the F(2x2) launch of the same descriptor, and the refusals (a split workspace; an unsupported channel count)."""
    import torch.nn.functional as F
    L = Hh.lib()
    torch.manual_seed(13)
    B, H, W = 2, 9, 14
    x = torch.randn(B, H, W, Cin, device=dev())
    w = torch.randn(Cout, Cin, 5, 5, device=dev()) * 0.1
    b = torch.randn(Cout, device=dev()) * 0.1
    wp = torch.empty(L.ramnet_packed_weight_elems_fold_wino2x3(Cout, Cin), device=dev())
    assert L.ramnet_pack_weight_fold_wino2x3(ptr(w), ptr(wp), Cout, Cin, None) == 0
    xpad = torch.empty(B, H + 4, W + 4, Cin, device=dev())
    assert L.ramnet_pad2_sum(ptr(x), None, ptr(xpad), B, H, W, Cin, None) == 0
    y = torch.zeros(B, 2 * H, 2 * W, Cout, device=dev())
    d = _fwd_desc(xpad, wp, b, y, B, H, W, Cin, Cout, Hh.ALGO_WINOGRAD24)
    assert L.ramnet_fold_wino_variant(C.byref(d), 1) == 1 and L.ramnet_fold_wino_variant(C.byref(d), 0) == 0     # batch 2: F(2x2)
    d.algo = Hh.ALGO_WINOGRAD24_2X3
    assert L.ramnet_fold_wino_variant(C.byref(d), 1) == 0                      # only RAMNET_ALGO_WINOGRAD24 descriptors are asked
    assert L.ramnet_conv_launch(C.byref(d), None) == 0, L.ramnet_last_error()
    assert b"conv_wino24_kernel<4,0," in L.ramnet_last_kernel() and L.ramnet_last_kernel().endswith(b",3>")
    xr = x.permute(0, 3, 1, 2).cpu().double()
    ref = F.conv2d(F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=False), w.cpu().double(), b.cpu().double(), 1, 2)
    got = y.permute(0, 3, 1, 2).cpu().double()
    assert float((got - ref)[:, :, 2:-2, 2:-2].abs().max() / ref.abs().max()) < 2e-5          # the frame needs the border GEMMs
    ws = torch.zeros(1 << 16, device=dev())
    d.splitk_ws, d.splitk_floats = ptr(ws), ws.numel()
    assert L.ramnet_conv_launch(C.byref(d), None) == 10001                     # F(2x3) has no split reduction
    d.splitk_ws, d.splitk_floats = None, 0
    d.Cout = 48
    assert L.ramnet_conv_launch(C.byref(d), None) == 10001

    # backward-data: the F(2x3) launch equals the F(2x2) one (itself checked against torch in test_hip_ops)
    g = torch.randn(B, 2 * H, 2 * W, Cout, device=dev())
    w22 = torch.empty(L.ramnet_packed_weight_elems_fold_wino(Cout, Cin), device=dev())
    w23 = torch.empty(L.ramnet_packed_weight_elems_fold_wino2x3(Cout, Cin), device=dev())
    assert L.ramnet_pack_weight_fold_wino_dgrad(ptr(w), ptr(w22), Cout, Cin, None) == 0
    assert L.ramnet_pack_weight_fold_wino2x3_dgrad(ptr(w), ptr(w23), Cout, Cin, None) == 0
    dx22, dx23 = (torch.full((B, H + 4, W + 4, Cin), float("nan"), device=dev()) for _ in range(2))
    d22 = _dgrad_desc(g, w22, dx22, B, H, W, Cin, Cout, Hh.ALGO_WINOGRAD24)
    assert L.ramnet_fold_wino_variant(C.byref(d22), 1) == 1
    d23 = _dgrad_desc(g, w23, dx23, B, H, W, Cin, Cout, Hh.ALGO_WINOGRAD24_2X3)
    assert L.ramnet_conv_launch(C.byref(d22), None) == 0, L.ramnet_last_error()
    assert L.ramnet_conv_launch(C.byref(d23), None) == 0, L.ramnet_last_error()
    assert L.ramnet_last_kernel().startswith(b"conv_wino24_kernel<4,1,") and L.ramnet_last_kernel().endswith(b",3>")
    assert bool(torch.isfinite(dx23).all())
    assert float((dx23 - dx22).abs().max() / dx22.abs().max()) < 2e-5


def test_repeated_2x3_launches_are_bit_identical(fold2x3):
    """Two forward + backward passes of a decoder layer on F(2x3) give bit-identical outputs and input gradients."""
    from rpg_ramnet_amd.model.submodules import UpsampleConvLayer
    torch.manual_seed(6)
    m = UpsampleConvLayer(128, 64, 5, padding=2).to(dev())
    x, s = torch.randn(4, 128, 24, 30, device=dev()), torch.randn(4, 128, 24, 30, device=dev())
    outs = []
    for _ in range(2):
        xg, sg = nhwc(x).requires_grad_(True), nhwc(s).requires_grad_(True)
        y = m(xg, sg)
        y.backward(torch.ones_like(y))
        outs.append((y.detach().clone(), xg.grad.clone(), sg.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert {"f23", "f23d"} <= _kinds(fold2x3) or not fold2x3._DESC_CACHE_ON


@pytest.mark.parametrize("B,want", [(1, 0), (16, 1), (64, 1)])
def test_auto_picks_2x3_at_the_training_batch(B, want):
    """ramnet_fold_wino_variant without force: F(2x3) for the forward and backward-data launches of the three decoders at the training
    batch (the bench step decodes several measurements of its B = 8 sequences per launch), F(2x2) at batch 1 (streaming; split
    reductions)."""
    L = Hh.lib()
    for Cin, Cout, H, W in DECODERS:
        d = _fwd_desc(torch.empty(0), torch.empty(0), None, torch.empty(0), B, H, W, Cin, Cout, Hh.ALGO_WINOGRAD24)
        assert L.ramnet_fold_wino_variant(C.byref(d), 0) == want, (Cin, Cout, B, "forward")
        d = _dgrad_desc(torch.empty(0), torch.empty(0), torch.empty(0), B, H, W, Cin, Cout, Hh.ALGO_WINOGRAD24)
        assert L.ramnet_fold_wino_variant(C.byref(d), 0) == want, (Cin, Cout, B, "backward-data")
