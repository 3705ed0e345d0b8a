"""GPU: the launches that partial training adds (a frozen prediction layer, a cell behind a frozen encoder), each alone through the C ABI
/ ops.conv_launch, in the manner of tests/test_hip_pointwise.py (the guarded buffers and the `call` of tests/guarded.py).

  ramnet_pred_sigmoid_dgrad / ramnet_pred_linear_dgrad / ramnet_pred_sigmoid_si_dgrad: dx EQUAL, bit for bit, to the dx of the launch
  that also forms the weight and bias gradients, on the same operands — it is the same expression per element.
  The state-half backward-data launch of a cell (ops.StateHalfConvParam: Cout = C into dxh[..., C:] at ld = 2C) against the float64
  statement of the full convolution's adjoint, at the operator bound of DESIGN section 6 (2e-4 max-norm)."""
import ctypes as C

import pytest
import torch

from rpg_ramnet_amd import _hip
from guarded import GUARD, SENT, In, Out, _bits, _dev, call, rn

pytestmark = pytest.mark.gpu

F64 = torch.float64
# pixels: 2 x 8 x 12 (two workgroups, the second half full), a ragged 2 x 7 x 13, and one past 2048 workgroups x 128 pixels, where a
# workgroup's run is 256 pixels and its loop takes a second, ragged trip
SIZES = [2 * 8 * 12, 2 * 7 * 13, 2048 * 128 + 3 * 128 + 5]


def same_bits(a, b, what):
    bad = _bits(a) != _bits(b)
    assert not bool(bad.any()), "%s: %d of %d elements differ, first at %s" % (what, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())


@pytest.mark.parametrize("sig", [False, True])
@pytest.mark.parametrize("npix,lddx", [(SIZES[0], 32), (SIZES[1], 32), (SIZES[1], 40), (SIZES[2], 32)])
def test_pred_dgrad_equals_the_dx_of_the_full_backward(npix, lddx, sig):
    Cc = 32
    x, w, dy = rn(npix, Cc, seed=31), rn(Cc, seed=32, scale=0.5), rn(npix, seed=33)
    y = torch.sigmoid(rn(npix, seed=34, scale=2.0)).float().to(F64) if sig else None
    full, part = Out(npix, Cc, ld=lddx), Out(npix, Cc, ld=lddx)
    dw, db = Out(1, Cc, prefill=torch.zeros(Cc)), Out(1, 1, prefill=torch.zeros(1))
    if sig:
        call("ramnet_pred_sigmoid_bwd", In(x), Cc, Cc, In(w), In(y), In(dy), full, lddx, dw, db, npix)
        call("ramnet_pred_sigmoid_dgrad", Cc, In(w), In(y), In(dy), part, lddx, npix)
    else:
        call("ramnet_pred_linear_bwd", In(x), Cc, Cc, In(w), In(dy), full, lddx, dw, db, npix)
        call("ramnet_pred_linear_dgrad", Cc, In(w), In(dy), part, lddx, npix)
    assert float(full.value().abs().max()) > 0
    same_bits(part.value(), full.value(), "dgrad-only dx")


@pytest.mark.parametrize("seg_pix", [8 * 12, 7 * 13, 1024 * 128 + 3 * 128 + 5])
@pytest.mark.parametrize("mask_x,with_dy,ld", [(0, True, 32), (1, False, 32), (1, True, 40)])
def test_pred_si_dgrad_equals_the_dx_of_the_full_backward(seg_pix, mask_x, with_dy, ld):
    """Two segments (B = 2 maps of seg_pix pixels), 20 % NaN targets, statistics from the forward launch itself; with and without the
    dense gradient dy, with and without the ReLU mask of x, dense and pitched rows."""
    Cc, nseg = 32, 2
    npix = nseg * seg_pix
    L = _hip.lib()
    g = torch.Generator().manual_seed(35)
    x = torch.relu(rn(npix, Cc, seed=36))                # a ReLU output: a third of the mask is zero
    w, b, dy = rn(Cc, seed=37, scale=0.5), rn(1, seed=38), rn(npix, seed=39)
    tg = torch.rand(npix, generator=g)
    tg[torch.rand(npix, generator=g) < 0.2] = float("nan")
    tgd = tg.to(_dev())
    arr = (C.c_void_p * nseg)(*[tgd.data_ptr() + 4 * i * seg_pix for i in range(nseg)])
    xin, win = In(x, ld), In(w)
    y = Out(1, npix)
    scratch = torch.zeros(L.ramnet_pred_si_scratch_doubles(seg_pix, nseg), device=_dev(), dtype=F64)
    stats = torch.empty(nseg, 4, device=_dev(), dtype=F64)
    loss = torch.empty(nseg, device=_dev())
    gs = torch.tensor([0.5, 0.25], device=_dev())
    call("ramnet_pred_sigmoid_si_fwd", xin, ld, Cc, win, In(b), y, seg_pix, nseg, arr, 1.0, 0.85, scratch, stats, loss)
    yin = In(y.value().double().reshape(-1))
    dyin = In(dy) if with_dy else None
    full, part = Out(npix, Cc, ld=ld), Out(npix, Cc, ld=ld)
    dw, db = Out(1, Cc, prefill=torch.zeros(Cc)), Out(1, 1, prefill=torch.zeros(1))
    call("ramnet_pred_sigmoid_si_bwd", xin, ld, Cc, win, yin, dyin, seg_pix, nseg, arr, stats, gs, 1.0, 0.85, full, ld, dw, db, scratch, mask_x)
    call("ramnet_pred_sigmoid_si_dgrad", xin if mask_x else None, ld if mask_x else 0, Cc, win, yin, dyin, seg_pix, nseg, arr, stats, gs, 1.0, 0.85,
         part, ld, mask_x)
    v = full.value()
    assert float(v.abs().max()) > 0 and (not mask_x or bool((v == 0).any()))
    same_bits(part.value(), v, "SI dgrad-only dx")


def test_pred_dgrad_argument_checks():
    i, o = In(torch.zeros(64, 64)), Out(64, 64)
    tg = (C.c_void_p * 1)(i.ptr)
    bad = [("ramnet_pred_sigmoid_dgrad", 6, i, i, i, o, 8, 4), ("ramnet_pred_sigmoid_dgrad", 8, i, i, i, o, 4, 4), ("ramnet_pred_sigmoid_dgrad", 8, i, i, i, o, 10, 4),
           ("ramnet_pred_sigmoid_dgrad", 132, i, i, i, o, 132, 4), ("ramnet_pred_sigmoid_dgrad", 8, i, None, i, o, 8, 4), ("ramnet_pred_sigmoid_dgrad", 8, i, i, i, o, 8, 0),
           ("ramnet_pred_linear_dgrad", 8, i, None, o, 8, 4), ("ramnet_pred_linear_dgrad", 8, None, i, o, 8, 4), ("ramnet_pred_linear_dgrad", 8, i, i, o, 6, 4),
           ("ramnet_pred_sigmoid_si_dgrad", None, 0, 8, i, i, i, 4, 1, tg, i, i, 1.0, 1.0, o, 8, 1),       # the mask without x
           ("ramnet_pred_sigmoid_si_dgrad", i, 4, 8, i, i, i, 4, 1, tg, i, i, 1.0, 1.0, o, 8, 1),
           ("ramnet_pred_sigmoid_si_dgrad", None, 0, 8, i, i, i, 4, 9, tg, i, i, 1.0, 1.0, o, 8, 0),
           ("ramnet_pred_sigmoid_si_dgrad", None, 0, 8, i, i, i, 4, 1, None, i, i, 1.0, 1.0, o, 8, 0)]
    for args in bad:
        call(*args, rc=10001)


# ------------------------------------------------------------------------------------------------ state half of a cell's backward-data
def _guarded(shape, fill=SENT):
    """contiguous device tensor of `shape` between sentinel guards -> (tensor view, whole buffer)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((2 * GUARD + n,), fill, device=_dev(), dtype=torch.float32)
    return buf[GUARD:GUARD + n].view(shape), buf


@pytest.mark.parametrize("wino2x4", ["auto", "force"])
@pytest.mark.parametrize("cout_mult,beta", [(1, 0.0), (2, 1.0), (4, 0.0), (4, 1.0)])
def test_state_half_backward_data_against_float64(cout_mult, beta, wino2x4):
    """The three convolutions a cell differentiates (ConvGRU candidate: C outputs; gates: 2C, accumulating; ConvLSTM gates: 4C, plain and
    accumulating) at C = 64, 2 x 8 x 12 pixels: dxh[..., C:] (+)= the h half of the adjoint; the x half and the guards stay as they were."""
    import torch.nn.functional as F
    from rpg_ramnet_amd import ops
    Cc, B, Hh, W = 64, 2, 8, 12
    co = cout_mult * Cc
    torch.manual_seed(40 + cout_mult)
    w = torch.nn.Parameter((torch.randn(co, 2 * Cc, 3, 3) * 0.05).to(_dev()))
    cp = ops.ConvParam([w], [torch.nn.Parameter(torch.zeros(co, device=_dev()))], gates=4 if cout_mult == 4 else 1)
    g = torch.randn(B, co, Hh, W)
    gd = g.permute(0, 2, 3, 1).contiguous().to(_dev())
    dxh, buf = _guarded((B, Hh, W, 2 * Cc))
    old = torch.randn(B, Hh, W, Cc)
    if beta:
        dxh[..., Cc:] = old.to(_dev())
    before = buf.clone()
    with ops.switches(winograd_2x4=wino2x4):
        ops.conv_launch(gd, ops.Taps.get("dgrad1", 3, 1), cp.state_half().bwd(), dxh, Cc, out_off=Cc, beta=beta)
        torch.cuda.synchronize()
    ref = F.conv_transpose2d(g.double(), w.detach().cpu().double(), padding=1)[:, Cc:].permute(0, 2, 3, 1)
    if beta:
        ref = ref + old.double()
    got = dxh[..., Cc:].cpu().double()
    err = float((got - ref).abs().max() / ref.abs().max())
    print("state half Cout=%d beta=%g %s: max-norm rel err %.3e (%s)" % (co, beta, wino2x4, err, _hip.lib().ramnet_last_kernel().decode()))
    assert err <= 2e-4
    keep = torch.ones_like(before, dtype=torch.bool)
    keep[GUARD:GUARD + dxh.numel()].view(B, Hh, W, 2 * Cc)[..., Cc:] = False
    assert torch.equal(_bits(buf)[keep], _bits(before)[keep]), "the launch wrote outside dxh[..., C:]"


@pytest.mark.parametrize("cell", ["convgru", "convlstm"])
def test_cell_backward_behind_a_frozen_encoder(cell):
    """x without a gradient, h with one: the cell forms dh through the state-half launches ("force") and through the full-width ones ("off");
    both are fp32 evaluations of one float64 value — they agree within twice the operator bound — and the weight gradients too."""
    from rpg_ramnet_amd import ops
    from rpg_ramnet_amd.model.submodules import ConvGRU, ConvLSTM
    Cc, B, Hh, W = 64, 2, 8, 12
    torch.manual_seed(50)
    m = (ConvGRU if cell == "convgru" else ConvLSTM)(Cc, Cc, 3).to(_dev())
    x, h0, c0, gout = (torch.randn(B, Hh, W, Cc, device=_dev()) for _ in range(4))
    res = {}
    for mode in ("off", "force"):
        with ops.switches(cell_state_half=mode):
            h = h0.clone().requires_grad_(True)
            m.zero_grad()
            out = m(x, h) if cell == "convgru" else m(x, (h, c0))[0]
            names = []

            def tracer(name, fn, args):
                names.append((name, args[0]._obj.Cout if name == "ramnet_conv_launch" else 0))
                return fn(*args)
            _hip.set_tracer(tracer)
            try:
                (out * gout).sum().backward()
            finally:
                _hip.set_tracer(None)
            torch.cuda.synchronize()
        widths = [c for n, c in names if n == "ramnet_conv_launch"]
        assert widths and all(c == (Cc if mode == "force" else 2 * Cc) for c in widths), (mode, names)
        res[mode] = [h.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    for a, b in zip(res["force"], res["off"]):
        assert float((a - b).abs().max()) <= 2 * 2e-4 * float(b.abs().max())
