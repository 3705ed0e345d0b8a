"""GPU: backward-weights of the folded decoders on F(2x3,4x4) tiles (RAMNET_ALGO_WINOGRAD24_2X3 on ramnet_wgrad_desc,
conv_wgrad_wino24_kernel_2x3, ramnet_fold_unpack_wgrad2x3) forced on every launch the kernel takes: layer gradients against the oracle,
the raw C ABI against the float64 statements of tests/test_fold_wino2x3_wgrad_cpu.py, accumulation over passes, a frozen weight, and
the "auto" choice of ramnet_fold_wgrad_variant."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import ramnet_ref
from rpg_ramnet_amd import _hip as Hh
from test_fold_wino2x3_wgrad_cpu import du_to_parity_filters, fold_unpack_torch_2x3, fold_wgrad_du
from test_hip_ops import TOL, dev, run_pair
from util import assert_close, nchw, nhwc

pytestmark = pytest.mark.gpu


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture
def wgrad2x3():
    """The folded Winograd path with F(2x3,4x4) forced on the backward-weights launches (forward / backward-data stay on "auto")."""
    from rpg_ramnet_amd import ops
    with ops.switches(fold_upsample=True, fold_winograd=True, fold_winograd_wgrad=True, fold_dgrad=True, fold_winograd_wgrad_2x3="force"):
        ops._WDESC_CACHE.clear()
        yield ops


def _algos(ops):
    return {d.algo for d in ops._WDESC_CACHE.values()}


def _ran_2x3(ops):
    return not ops._DESC_CACHE_ON or _algos(ops) == {Hh.ALGO_WINOGRAD24_2X3}


class _Layer(torch.nn.Module):
    """conv5x5(bilinear_x2(x [+ skip])) with or without the ReLU, on ops.ConvAct like model.submodules.UpsampleConvLayer."""

    def __init__(self, cin, cout, relu):
        super().__init__()
        self.conv2d, self.relu, self._cp = torch.nn.Conv2d(cin, cout, 5, 1, 2), relu, None

    def forward(self, x, skip=None):
        from rpg_ramnet_amd import ops
        if self._cp is None:
            self._cp = ops.ConvParam([self.conv2d.weight], [self.conv2d.bias])
        return ops.ConvAct.apply(x, skip, self.conv2d.weight, self.conv2d.bias, self._cp, 1, self.relu, True)


def _oracle(relu):
    def f(sd, a, sk=None):
        x = a if sk is None else a + sk
        if relu:
            return ramnet_ref.upsample_conv_layer({"L." + k: v for k, v in sd.items()}, "L", x)
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False), sd["conv2d.weight"], sd["conv2d.bias"], 1, 2)
    return f


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("B,H,W", [(1, 4, 4), (1, 5, 11), (2, 8, 16), (1, 32, 43)])
@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 32), (128, 64)])
def test_layer_gradients_on_2x3_backward_weights(cin, cout, B, H, W, skip, relu, wgrad2x3):
    """Forward, dx, dskip, dW and db against the oracle at the project's tolerance; the backward-weights launch ran as F(2x3)."""
    torch.manual_seed(3)
    m = _Layer(cin, cout, relu)
    x, s = torch.randn(B, cin, H, W), (torch.randn(B, cin, H, W) if skip else None)
    run_pair(m, _oracle(relu), [x, s] if skip else [x])
    assert _ran_2x3(wgrad2x3), _algos(wgrad2x3)


def _one_pass(m, x, s, g):
    xg, sg = nhwc(x).requires_grad_(True), nhwc(s).requires_grad_(True)
    (nchw(m(xg, sg)) * g).sum().backward()


def _reference_grads(m, x, s, g):
    sd = {"L." + k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}
    ref = ramnet_ref.upsample_conv_layer(sd, "L", x.double() + s.double())
    (ref * g.double()).sum().backward()
    return sd["L.conv2d.weight"].grad, sd["L.conv2d.bias"].grad


def test_two_passes_accumulate(wgrad2x3):
    """Two backward passes without an optimizer step in between: .grad holds twice the gradient — the unpack zeroed the [4][30] workspace
    after the first pass and the second pass reused it."""
    torch.manual_seed(7)
    m = _Layer(128, 64, True).to(dev())
    x, s = torch.randn(2, 128, 9, 14, device=dev()), torch.randn(2, 128, 9, 14, device=dev())
    with torch.no_grad():
        y = nchw(m(nhwc(x), nhwc(s)))
    g = torch.randn(y.shape, device=dev())
    dw, db = _reference_grads(m, x, s, g)
    _one_pass(m, x, s, g)
    recs = dict(m._cp.workspaces())
    ws = recs["fold23"].t
    assert ws is not None and float(ws.abs().max()) == 0.0 and recs["fold24"].t is None
    assert_close(m.conv2d.weight.grad.cpu().numpy(), dw.cpu().numpy(), TOL, "dW, one pass")
    _one_pass(m, x, s, g)
    assert recs["fold23"].t is ws
    assert_close(m.conv2d.weight.grad.cpu().numpy(), 2 * dw.cpu().numpy(), TOL, "dW, two passes")
    assert_close(m.conv2d.bias.grad.cpu().numpy(), 2 * db.cpu().numpy(), TOL, "db, two passes")
    assert _ran_2x3(wgrad2x3)


def test_frozen_decoder_forms_no_weight_gradient(wgrad2x3):
    """requires_grad = False on the weight: no weight gradient, the bias still trains, and the pass after thawing starts from zeroed workspaces."""
    torch.manual_seed(8)
    m = _Layer(64, 32, True).to(dev())
    x, s = torch.randn(1, 64, 8, 10, device=dev()), torch.randn(1, 64, 8, 10, device=dev())
    with torch.no_grad():
        y = nchw(m(nhwc(x), nhwc(s)))
    g = torch.randn(y.shape, device=dev())
    dw, db = _reference_grads(m, x, s, g)
    m.conv2d.weight.requires_grad_(False)
    _one_pass(m, x, s, g)
    assert m.conv2d.weight.grad is None
    assert_close(m.conv2d.bias.grad.cpu().numpy(), db.cpu().numpy(), TOL, "db, frozen weight")
    m.conv2d.weight.requires_grad_(True)
    m.conv2d.bias.grad = None
    _one_pass(m, x, s, g)
    assert_close(m.conv2d.weight.grad.cpu().numpy(), dw.cpu().numpy(), TOL, "dW after thawing")


def _wgrad_desc(xpad, g, gm, dw, dbias, B, H, W, Cin, Cout, algo):
    d = Hh.WgradDesc()
    d.x0, d.ld0, d.C0, d.in_mode = ptr(xpad), Cin, Cin, Hh.IN_PLAIN
    d.B, d.Hin, d.Win, d.stride, d.ntaps = B, H + 4, W + 4, 1, 16
    d.dout, d.gmask, d.ldg, d.ldgm = ptr(g), ptr(gm), Cout, (Cout if gm is not None else 0)
    d.Cout, d.Ho, d.Wo, d.HoG, d.WoG = Cout, H, W, 2 * H, 2 * W
    d.dw, d.dbias, d.algo = ptr(dw), ptr(dbias), algo
    return d


def _splits(B, H, W, Cin, Cout, tw):
    """Tile splits (gridDim.x) of the launch: csrc/conv_wgrad_wino24.hip, launch_wgrad_wino24."""
    ci, co = (64, 32) if Cout % 64 else (32, 64)
    nbatch = -(-(-(-W // tw) * -(-H // 2) * B) // (6 if tw == 3 else 8))
    return max(1, min(256 // ((Cin // ci) * (Cout // co) * 4), nbatch))


# (B, H, W): one batch of tiles = a single split; several splits that meet by atomics; the real scale-2 grid, ragged in the columns
RAW_SHAPES = [(1, 4, 4), (2, 9, 13), (1, 32, 43)]


@pytest.mark.parametrize("gm", [True, False])
@pytest.mark.parametrize("B,H,W", RAW_SHAPES)
@pytest.mark.parametrize("Cin,Cout", [(128, 64), (64, 32)])
def test_du_through_raw_descriptors(Cin, Cout, B, H, W, gm):
    """RAMNET_ALGO_WINOGRAD24_2X3 on a raw ramnet_wgrad_desc: dU [4][30][Cin][Cout] and the bias gradient against the float64 statement.
    The bound is not fixed in advance: the F(2x2) kernel's error against ITS float64 statement on the same inputs is measured, and
    F(2x3) is allowed 4 times that (3.8 was the largest ratio of a float32 emulation of the two transforms over post-ReLU and plain
    inputs of 32 x 42 to 128 x 174) — for dU (max-norm, relative to the largest entry) and for the parity-filter gradient G_r^T dU G_c.
    Measured (max-norm relative errors of dW4, F(2x2) / F(2x3)): see profiles/fold23_wgrad_notes.md."""
    L = Hh.lib()
    torch.manual_seed(11)
    x = torch.relu(torch.randn(B, H, W, Cin, device=dev()))               # (decoder inputs are post-ReLU sums)
    g = torch.randn(B, 2 * H, 2 * W, Cout, device=dev())
    mask = torch.randn(B, 2 * H, 2 * W, Cout, device=dev()) if gm else None
    xpad = torch.empty(B, H + 4, W + 4, Cin, device=dev())
    assert L.ramnet_pad2_sum(ptr(x), None, ptr(xpad), B, H, W, Cin, None) == 0
    geff = (g * (mask > 0)) if gm else g
    x64, g64 = xpad.permute(0, 3, 1, 2).double(), geff.permute(0, 3, 1, 2).double()
    assert _splits(*RAW_SHAPES[0], Cin, Cout, 3) == 1 and _splits(*RAW_SHAPES[1], Cin, Cout, 3) > 1
    err = {}
    for tw, algo, name in ((2, Hh.ALGO_WINOGRAD24, b"conv_wgrad_wino24_kernel<"), (3, Hh.ALGO_WINOGRAD24_2X3, b"conv_wgrad_wino24_kernel_2x3<")):
        dU = torch.zeros(4, 5 * (tw + 3), Cin, Cout, device=dev())
        db = torch.zeros(Cout, device=dev())
        d = _wgrad_desc(xpad, g, mask, dU, db, B, H, W, Cin, Cout, algo)
        assert L.ramnet_wgrad_launch(C.byref(d), None) == 0, L.ramnet_last_error()
        assert L.ramnet_last_kernel().startswith(name), L.ramnet_last_kernel()
        torch.cuda.synchronize()
        ref = fold_wgrad_du(x64, g64, tw)
        w4, w4ref = du_to_parity_filters(dU.double(), tw), du_to_parity_filters(ref, tw)
        err[tw] = (float((dU.double() - ref).abs().max() / ref.abs().max()), float((w4 - w4ref).abs().max() / w4ref.abs().max()))
        assert bool(torch.isfinite(dU).all())
        assert_close(db.cpu().numpy(), g64.sum((0, 2, 3)).cpu().numpy(), TOL, "db")
    print("fold wgrad errors Cin=%d Cout=%d B=%d H=%d W=%d gm=%d: dU 2x2 %.2e 2x3 %.2e | dW4 2x2 %.2e 2x3 %.2e"
          % (Cin, Cout, B, H, W, gm, err[2][0], err[3][0], err[2][1], err[3][1]))
    assert err[3][0] <= 4 * err[2][0], ("dU", err)
    assert err[3][1] <= 4 * err[2][1], ("dW4", err)


def test_raw_descriptor_refusals_and_unpack():
    """The launch refuses channel shapes the kernel does not take; ramnet_fold_unpack_wgrad2x3 equals its torch statement and zeroes what
    it read; ramnet_fold_wgrad_variant answers only RAMNET_ALGO_WINOGRAD24 descriptors."""
    L = Hh.lib()
    torch.manual_seed(12)
    B, H, W, Cin, Cout = 1, 6, 7, 64, 64
    xpad, g = torch.randn(B, H + 4, W + 4, Cin, device=dev()), torch.randn(B, 2 * H, 2 * W, Cout, device=dev())
    dU3 = torch.zeros(4 * 30 * Cin * Cout, device=dev())
    d = _wgrad_desc(xpad, g, None, dU3, None, B, H, W, Cin, Cout, Hh.ALGO_WINOGRAD24)
    assert L.ramnet_fold_wgrad_variant(C.byref(d), 1) == 1
    d.algo = Hh.ALGO_WINOGRAD24_2X3
    assert L.ramnet_fold_wgrad_variant(C.byref(d), 1) == 0
    assert L.ramnet_wgrad_launch(C.byref(d), None) == 0, L.ramnet_last_error()
    d.C0 = 48
    assert L.ramnet_wgrad_launch(C.byref(d), None) == 10001
    d.C0, d.algo = Cin, Hh.ALGO_WINOGRAD24
    d.Cout = 48
    assert L.ramnet_fold_wgrad_variant(C.byref(d), 1) == 0
    w4, dU = torch.randn(64 * Cin * Cout, device=dev()), torch.randn(4 * 25 * Cin * Cout, device=dev())
    wr, wc = torch.randn(2, 5 * Cin, 2 * Cout, device=dev()), torch.randn(2, 5 * Cin, 2 * Cout, device=dev())
    for use_du in (True, False):
        a4, aU, a3, ar, ac = (t.clone() for t in (w4, dU, dU3, wr, wc))
        ref = fold_unpack_torch_2x3(w4, dU if use_du else None, dU3, wr, wc, Cout, Cin, Cin)
        grad = torch.zeros(Cout, Cin, 5, 5, device=dev())
        assert L.ramnet_fold_unpack_wgrad2x3(ptr(a4), ptr(aU) if use_du else None, ptr(a3), ptr(ar), ptr(ac), ptr(grad), Cout, Cin, Cin, None) == 0
        assert_close(grad.cpu().numpy(), ref.cpu().numpy(), 1e-5, "unpack 2x3")
        assert float(a3.abs().max()) == 0.0 and float(a4.abs().max()) == 0.0 and float(ar.abs().max()) == 0.0
        assert (float(aU.abs().max()) == 0.0) == use_du


# the three decoder layers of the flagship workload (256 x 344 input, base 32 channels): (Cin, Cout, low-res H, W)
DECODERS = [(256, 128, 32, 43), (128, 64, 64, 86), (64, 32, 128, 172)]
AUTO = {16: (1, 1, 1), 1: (0, 0, 0)}          # batch -> ramnet_fold_wgrad_variant(force = 0) per decoder: tools/bench_fold23_wgrad.py's sweep


@pytest.mark.parametrize("B", sorted(AUTO))
def test_auto_choice_is_what_the_sweep_found(B):
    L = Hh.lib()
    for (Cin, Cout, H, W), want in zip(DECODERS, AUTO[B]):
        d = _wgrad_desc(None, None, None, None, None, B, H, W, Cin, Cout, Hh.ALGO_WINOGRAD24)
        assert L.ramnet_fold_wgrad_variant(C.byref(d), 0) == want, (Cin, Cout, B)
        assert L.ramnet_fold_wgrad_variant(C.byref(d), 1) == 1
