"""GPU: the ConvLSTM state update on the F(2x4,3x3) Winograd kernels (csrc/conv_wino6.hip, ABI 27) — the cell launch (gate-interleaved
pack, cell epilogue, per-sample update masks) and the backward-data launch — from raw launches up to the network: against float64 torch /
the CPU oracle, against the F(2x2,3x3) launches, and at full resolution against tests/golden/fullsize_lstm.npz (oracle outputs on seeded
inputs, tests/golden/make_golden_fullsize_lstm.py).

Reference semantics: RAM_Net/model/submodules.py:303-358 (ConvLSTM), statenet.py:222-229 (the shared (h, c) state).  Tolerances are the
sibling tests' (tests/test_hip_ops.py TOL, tests/test_hip_model.py, tests/test_hip_fullsize.py); none is new."""
import ctypes

import numpy as np
import pytest
import torch

import fullsize_cases as fc
import test_hip_irregular as irr
import test_hip_model as thm
from oracle import ramnet_ref
from test_hip_fullsize import run_pair64
from test_hip_ops import TOL, run_pair
from util import ELEM_FLOOR, assert_close, build_hip_model, load_golden, nchw, nhwc, ref_cfg

pytestmark = pytest.mark.gpu
R6 = "conv_wino_r6_kernel<"


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def last_kernel():
    from rpg_ramnet_amd import _hip as Hh
    return Hh.lib().ramnet_last_kernel().decode()


@pytest.fixture
def forced():
    """Every structurally eligible forward / backward-data launch on F(2x4,3x3), backward-weights on its F(2x4,3x3) kernel."""
    from rpg_ramnet_amd import ops
    with ops.switches(winograd_2x4="force", wgrad_winograd_2x4="force"):
        yield


def _lstm_param(C, seed=11):
    from rpg_ramnet_amd import ops
    torch.manual_seed(seed)
    w = torch.randn(4 * C, 2 * C, 3, 3) * (0.5 / np.sqrt(2 * C))
    b = torch.randn(4 * C) * 0.1
    cp = ops.ConvParam([torch.nn.Parameter(w.to(dev()))], [torch.nn.Parameter(b.to(dev()))], gates=4)
    return w, b, cp


def _cell_ref(x, h, c, w, b):
    """float64 torch: (h', c', activated gates [B, 4C, H, W] in (i, f, o, g) order)."""
    g = torch.nn.functional.conv2d(torch.cat([x, h], 1).double(), w.double(), b.double(), 1, 1)
    gi, gf, go, gc = g.chunk(4, 1)
    gi, gf, go, gc = torch.sigmoid(gi), torch.sigmoid(gf), torch.sigmoid(go), torch.tanh(gc)
    cn = gf * c.double() + gi * gc
    return go * torch.tanh(cn), cn, torch.cat([gi, gf, go, gc], 1)


def _launch(cp, x, h, c, C, gates=True, active=None):
    """One cell launch through ops.conv_launch into NaN-filled outputs; returns (h', c', gates or None, kernel name)."""
    from rpg_ramnet_amd import ops, _hip as Hh
    B, Hh_, W, _ = x.shape
    hn = torch.full((B, Hh_, W, C), float("nan"), device=dev())
    cn = torch.full((B, Hh_, W, C), float("nan"), device=dev())
    gt = torch.full((B, Hh_, W, 4 * C), float("nan"), device=dev()) if gates else None
    kw = dict(x1=h, in_mode=Hh.IN_CAT, C1=C, bias=cp.bias(), epi=Hh.EPI_LSTM, e1=c, o1=cn, o2=gt)
    if active is not None:
        kw.update(e0=h, active=active)
    ops.conv_launch(x, ops.Taps.get("conv", 3, 1), cp.fwd(), hn, C, **kw)
    return hn, cn, gt, last_kernel()


@pytest.mark.parametrize("B,H,W", [(2, 16, 32), (1, 7, 13), (2, 9, 43), (1, 2, 2), (1, 32, 8), (2, 8, 32), (1, 64, 86)])
@pytest.mark.parametrize("C", [16, 64, 128])
def test_lstm_cell_raw(B, H, W, C):
    """Raw cell launches, forced F(2x4) against float64 torch and against the F(2x2) launch ("off"): h', c' and the gates, all three
    workgroup tile shapes, ragged maps; NaN-filled outputs; with and without a previous cell state (e1) and a gate buffer (o2); two
    identical launches are bit-identical."""
    from rpg_ramnet_amd import ops
    w, b, cp = _lstm_param(C)
    torch.manual_seed(3)
    x, h, c = torch.randn(B, C, H, W), torch.tanh(torch.randn(B, C, H, W)), torch.randn(B, C, H, W)
    xg, hg, cg = (nhwc(t).to(dev()) for t in (x, h, c))
    outs = {}
    for mode in ("force", "off"):
        with ops.switches(winograd_2x4=mode):
            outs[mode] = _launch(cp, xg, hg, cg, C)
            if mode == "force":
                again = _launch(cp, xg, hg, cg, C)
                nocell = _launch(cp, xg, hg, None, C)
                infer = _launch(cp, xg, hg, cg, C, gates=False)
    assert outs["force"][3].startswith(R6) and "lstm" in outs["force"][3], outs["force"][3]
    assert outs["off"][3].startswith("conv_wino_r_kernel"), outs["off"][3]
    assert nocell[3].startswith(R6) and infer[3].startswith(R6)
    rh, rc, rg = _cell_ref(x, h, c, w, b)
    err = lambda a, r: float((nchw(a).cpu().double() - r).abs().max() / r.abs().max())
    print("max-norm error vs float64: F(2x4) h' %.2e c' %.2e gates %.2e; F(2x2) h' %.2e c' %.2e gates %.2e" % (
        err(outs["force"][0], rh), err(outs["force"][1], rc), err(outs["force"][2], rg),
        err(outs["off"][0], rh), err(outs["off"][1], rc), err(outs["off"][2], rg)))
    for mode in ("force", "off"):
        for got, ref, what in zip(outs[mode][:3], (rh, rc, rg), ("h'", "c'", "gates")):
            assert bool(torch.isfinite(got).all()), "%s 2x4=%s: an output entry was not written" % (what, mode)
            assert_close(nchw(got).cpu().numpy(), ref.numpy(), TOL, "%s 2x4=%s" % (what, mode))
    for a, o, what in zip(outs["force"][:3], outs["off"][:3], ("h'", "c'", "gates")):
        assert_close(a.cpu().numpy(), o.cpu().numpy(), TOL, "F(2x4) vs F(2x2) " + what)
    for a, o in zip(outs["force"][:3], again[:3]):
        assert torch.equal(bits(a), bits(o)), "two identical launches differ"
    for a, o in zip(outs["force"][:2], infer[:2]):
        assert torch.equal(bits(a), bits(o)), "o2 = NULL changes the state"
    zh, zc, zg = _cell_ref(x, h, torch.zeros_like(c), w, b)
    for got, ref, what in zip(nocell[:3], (zh, zc, zg), ("h'", "c'", "gates")):
        assert_close(nchw(got).cpu().numpy(), ref.numpy(), TOL, "e1 = NULL " + what)


@pytest.mark.parametrize("B,H,W,C,mask", [(3, 8, 16, 64, [1, 0, 1]), (2, 16, 32, 128, [0, 1]), (4, 4, 43, 256, [0, 1, 1, 0]), (2, 9, 13, 16, [0, 1]),
                                          (1, 32, 8, 64, [0])])
def test_lstm_cell_raw_masked(B, H, W, C, mask, forced):
    """Masked launches (ramnet_conv_desc.active): inactive samples leave h' = h and c' = c bit for bit (-0.0 included) and zero gates;
    active samples are bit-equal to the unmasked launch."""
    w, b, cp = _lstm_param(C)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, H, W, C, generator=g).to(dev())
    h = torch.tanh(torch.randn(B, H, W, C, generator=g))
    h[:, ::3, ::2, ::5] = -0.0
    h = h.to(dev())
    c = torch.randn(B, H, W, C, generator=g).to(dev())
    act = torch.tensor(mask, dtype=torch.bool)
    plain = _launch(cp, x, h, c, C)
    masked = _launch(cp, x, h, c, C, active=act.to(torch.int32).to(dev()))
    assert masked[3].startswith(R6) and "masked" in masked[3] and "lstm" in masked[3], masked[3]
    for m_, p_ in zip(masked[:3], plain[:3]):
        assert torch.equal(bits(m_)[act], bits(p_)[act]), "active samples differ from the unmasked launch"
    assert torch.equal(bits(masked[0])[~act], bits(h)[~act]), "inactive h' is not a copy of h"
    assert torch.equal(bits(masked[1])[~act], bits(c)[~act]), "inactive c' is not a copy of c"
    assert bool((bits(masked[2])[~act] == 0).all()), "inactive gates are not zero"


def _pack_restatement(w, C):
    """torch restatement of the gate-interleaved F(2x4,3x3) pack: the index formula of pack_weight_wino_r6_kernel with the column
    permutation — column n of n-block f of block nb = gate n >> 3 of hidden channel nb*16 + f*8 + (n & 7)."""
    N, R = w.shape[0], w.shape[1]
    G2 = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)
    G4 = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
                      dtype=torch.float64)
    U = torch.einsum("wa,ncab,pb->wpcn", G2, w.double(), G4)            # [4][6][R][N]
    nchunks, nblk = R // 8, N // 64
    idx = torch.arange(nchunks * nblk * 24 * 64 * 8)
    j, lane, f = idx & 3, (idx >> 2) & 63, (idx >> 8) & 1
    jj = idx >> 9
    pl, jj = jj % 6, jj // 6
    wv, jj = jj & 3, jj >> 2
    nb, chunk = jj % nblk, jj // nblk
    n = lane & 31
    r = chunk * 8 + 4 * (lane >> 5) + j
    no = (n >> 3) * C + nb * 16 + f * 8 + (n & 7)
    return U[wv, pl, r, no].float()


@pytest.mark.parametrize("C", [16, 64])
def test_gate_interleaved_pack(C):
    from rpg_ramnet_amd import _hip as Hh, ops
    w, b, cp = _lstm_param(C, seed=5)
    got = cp.pack(0, "2x4g")
    want = _pack_restatement(w, C)
    assert got.numel() == want.numel() == Hh.lib().ramnet_packed_weight_elems_wino2x4_gates(4 * C, 2 * C, 0, 4)
    # exact up to the float rounding of the double-precision transform (the summation order of the 9 terms may differ: one ulp)
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=3e-7, atol=1e-9)
    # gates = 1 through the new entry point is the generic pack
    gen = torch.empty_like(got)
    assert Hh.lib().ramnet_pack_weight_wino2x4_gates(ops._p(cp._cat_w()), ops._p(gen), 4 * C, 2 * C, 0, 1, ops._st()) == 0
    assert torch.equal(bits(gen), bits(cp.pack(0, "2x4")))


def test_lstm_cell_through_raw_descriptors():
    """The raw C ABI with ctypes and device pointers: gate-interleaved pack + RAMNET_ALGO_WINOGRAD_2X4 launch of a RAMNET_EPI_LSTM descriptor,
    the kernel the library reports, and the backward-data launch of the same layer (generic transposed pack, LINEAR)."""
    from rpg_ramnet_amd import _hip
    L = _hip.lib()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.manual_seed(4)
    B, H, W, C = 2, 18, 26, 32
    x, h, c = (torch.randn(B, H, W, C, device=dev()) for _ in range(3))
    w = torch.randn(4 * C, 2 * C, 3, 3, device=dev()) * 0.1
    b = torch.randn(4 * C, device=dev()) * 0.1
    wp = torch.empty(L.ramnet_packed_weight_elems_wino2x4_gates(4 * C, 2 * C, 0, 4), device=dev())
    assert L.ramnet_pack_weight_wino2x4_gates(ptr(w), ptr(wp), 4 * C, 2 * C, 0, 4, st) == 0, L.ramnet_last_error()
    hn, cn = (torch.full((B, H, W, C), float("nan"), device=dev()) for _ in range(2))
    gt = torch.full((B, H, W, 4 * C), float("nan"), device=dev())
    d = _hip.ConvDesc()
    d.x0, d.x1, d.ld0, d.ld1, d.C0, d.C1, d.in_mode = ptr(x), ptr(h), C, C, C, C, _hip.IN_CAT
    d.B, d.Hin, d.Win, d.stride, d.ntaps = B, H, W, 1, 9
    for i in range(9):
        d.dy[i], d.dx[i], d.wtap[i] = i // 3 - 1, i % 3 - 1, i
    d.w, d.bias, d.Cout = ptr(wp), ptr(b), C
    d.Ho, d.Wo, d.HoF, d.WoF = H, W, H, W
    d.osy, d.osx = 1, 1
    d.epi, d.out, d.ldo, d.algo = _hip.EPI_LSTM, ptr(hn), C, _hip.ALGO_WINOGRAD
    d.e1, d.lde1, d.o1, d.ldo1, d.o2, d.ldo2 = ptr(c), C, ptr(cn), C, ptr(gt), 4 * C
    assert L.ramnet_conv_wino_variant(ctypes.byref(d), 1) == 1
    assert L.ramnet_conv_wino_split_ok(ctypes.byref(d), 1) == 0
    d.algo = _hip.ALGO_WINOGRAD_2X4
    assert L.ramnet_conv_launch(ctypes.byref(d), st) == 0, L.ramnet_last_error()
    assert L.ramnet_last_kernel().decode().startswith(R6)
    rh, rc, rg = _cell_ref(nchw(x).cpu(), nchw(h).cpu(), nchw(c).cpu(), w.cpu(), b.cpu())
    for got, ref, what in ((hn, rh, "h'"), (cn, rc, "c'"), (gt, rg, "gates")):
        assert_close(nchw(got).cpu().numpy(), ref.numpy(), TOL, "raw ABI " + what)
    d.o2, d.ldo2 = ptr(gt) .value + 4, 4 * C                       # a misaligned gate buffer is refused on the host
    assert L.ramnet_conv_launch(ctypes.byref(d), st) == 10001
    # backward-data: dpre [4C] -> d[x | h] [2C], generic transposed pack
    dpre = torch.randn(B, H, W, 4 * C, device=dev())
    wt = torch.empty(L.ramnet_packed_weight_elems_wino2x4(4 * C, 2 * C, 1), device=dev())
    assert L.ramnet_pack_weight_wino2x4(ptr(w), ptr(wt), 4 * C, 2 * C, 1, st) == 0
    dxh = torch.full((B, H, W, 2 * C), float("nan"), device=dev())
    e = _hip.ConvDesc()
    e.x0, e.ld0, e.C0, e.in_mode = ptr(dpre), 4 * C, 4 * C, _hip.IN_PLAIN
    e.B, e.Hin, e.Win, e.stride, e.ntaps = B, H, W, 1, 9
    for i in range(9):
        e.dy[i], e.dx[i], e.wtap[i] = i // 3 - 1, i % 3 - 1, i
    e.w, e.Cout, e.Ho, e.Wo, e.HoF, e.WoF, e.osy, e.osx = ptr(wt), 2 * C, H, W, H, W, 1, 1
    e.epi, e.out, e.ldo, e.algo = _hip.EPI_LINEAR, ptr(dxh), 2 * C, _hip.ALGO_WINOGRAD_2X4
    assert L.ramnet_conv_launch(ctypes.byref(e), st) == 0, L.ramnet_last_error()
    assert L.ramnet_last_kernel().decode().startswith(R6)
    ref = torch.nn.functional.conv_transpose2d(nchw(dpre).cpu().double(), w.cpu().double(), None, 1, 1)
    assert_close(nchw(dxh).cpu().numpy(), ref.numpy(), TOL, "raw ABI backward-data")


class _Wrap(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        from rpg_ramnet_amd.model.submodules import ConvLSTM
        self.L = ConvLSTM(C, C, 3)
        with torch.no_grad():
            for p in self.L.parameters():
                if p.dim() == 1:
                    p.uniform_(-0.1, 0.1)

    def forward(self, x, h, c):
        return self.L(x, (h, c))


def _spy_kernels():
    """Record the kernel the library reports after every convolution launch (ops.conv_launch)."""
    from rpg_ramnet_amd import ops
    seen, orig = [], ops.conv_launch

    def spy(*a, **kw):
        orig(*a, **kw)
        seen.append((int(kw.get("epi", 0)), last_kernel()))
    return seen, orig, spy


@pytest.mark.parametrize("B,H,W,C", [(2, 8, 16, 64), (1, 7, 13, 32), (2, 4, 43, 256), (2, 9, 20, 16)])
def test_conv_lstm_module_forced(B, H, W, C, forced, monkeypatch):
    """ConvLSTM forward and all gradients (dx, dh, dc, dW, db) against ramnet_ref.conv_lstm (run_pair's scheme); cell and backward-data
    launches report the F(2x4) kernel (backward-data: 2C % 64 == 0, else F(2x2))."""
    from rpg_ramnet_amd import ops, _hip as Hh
    seen, orig, spy = _spy_kernels()
    monkeypatch.setattr(ops, "conv_launch", spy)
    torch.manual_seed(6)
    run_pair(_Wrap(C), lambda sd, a, h, c: ramnet_ref.conv_lstm(sd, "L", a, (h, c)),
             [torch.randn(B, C, H, W), torch.tanh(torch.randn(B, C, H, W)), torch.randn(B, C, H, W)])
    cell = [k for e, k in seen if e == Hh.EPI_LSTM]
    dgrad = [k for e, k in seen if e == Hh.EPI_LINEAR]
    assert cell and all(k.startswith(R6) for k in cell), seen
    assert dgrad and all(k.startswith(R6 if C % 32 == 0 else "conv_wino_r_kernel") for k in dgrad), seen


@pytest.mark.parametrize("B,H,W,C,mask", [(3, 8, 16, 64, [1, 0, 1]), (4, 4, 43, 256, [0, 1, 1, 0])])
def test_conv_lstm_module_forced_masked(B, H, W, C, mask, forced):
    """With an `active` mask: states and gradients of the active sub-batch against the float64 oracle on those samples alone; inactive
    samples pass (h, c) and (dh', dc') through bit for bit, dx = 0 (tests/test_hip_irregular.py::test_masked_cell's scheme)."""
    m = _Wrap(C).to(dev())
    g = torch.Generator().manual_seed(1)
    x, c = (torch.randn(B, H, W, C, generator=g).to(dev()) for _ in range(2))
    h = torch.tanh(torch.randn(B, H, W, C, generator=g)).to(dev())
    act = torch.tensor(mask, dtype=torch.bool)
    ina = ~act
    xg, hg, cg = (t.clone().requires_grad_(True) for t in (x, h, c))
    out = m.L(xg, (hg, cg), active=act.to(dev()))
    assert last_kernel().startswith(R6) and "masked" in last_kernel()
    wts = [torch.randn(B, H, W, C, generator=g) for _ in out]
    sum((o * w_.to(dev())).sum() for o, w_ in zip(out, wts)).backward()
    for o, i in zip(out, (h, c)):
        assert torch.equal(bits(o)[ina], bits(i)[ina])
    assert torch.equal(hg.grad.cpu()[ina], wts[0][ina]) and torch.equal(cg.grad.cpu()[ina], wts[1][ina])
    assert bool((xg.grad.cpu()[ina] == 0).all())
    sd = {"L." + k: v.detach().cpu().double().requires_grad_(True) for k, v in m.L.state_dict().items()}
    sel = act.to(dev())
    xa, ha, ca = (nchw(t[sel].cpu()).double().requires_grad_(True) for t in (x, h, c))
    r64 = ramnet_ref.conv_lstm(sd, "L", xa, (ha, ca))
    sum((r * nchw(w_[act]).double()).sum() for r, w_ in zip(r64, wts)).backward()
    for o, r, what in zip(out, r64, ("h'", "c'")):
        assert_close(nchw(o.detach()[sel]).cpu().numpy(), r.detach().numpy(), TOL, "masked " + what)
    for got, ref, what in ((xg, xa, "dx"), (hg, ha, "dh"), (cg, ca, "dc")):
        assert_close(nchw(got.grad[sel]).cpu().numpy(), ref.grad.numpy(), TOL, "masked " + what)
    gmax = max(float(v.grad.abs().max()) for v in sd.values())
    for k, p in m.L.named_parameters():
        assert_close(p.grad.cpu().numpy(), sd["L." + k].grad.numpy(), TOL, "masked grad " + k, floor=1e-2 * gmax)


@pytest.mark.parametrize("C,div", [(64, 2), (128, 4), (256, 8)])
def test_conv_lstm_full_size_auto(C, div, monkeypatch):
    """The three scales of the network at the training batch (B = 8, 256 x 344) under "auto": forward + gradients against the oracle in
    float64 at the bound of test_conv_gru_full_size; the size rule puts the cell and the backward-data launch on F(2x4)."""
    from rpg_ramnet_amd import ops, _hip as Hh
    from rpg_ramnet_amd.model.submodules import ConvLSTM
    seen, orig, spy = _spy_kernels()
    monkeypatch.setattr(ops, "conv_launch", spy)
    with ops.switches(wgrad_overlap=True):
        torch.manual_seed(30 + div)
        m = ConvLSTM(C, C, 3)
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() == 1:
                    p.uniform_(-0.1, 0.1)
        B, H, W = 8, 256 // div, 344 // div
        x, h, c = torch.randn(B, C, H, W), torch.tanh(torch.randn(B, C, H, W)), torch.randn(B, C, H, W)

        class Both(torch.nn.Module):              # (h' and c' as one tensor: run_pair64 compares a single output)
            def __init__(self):
                super().__init__()
                self.L = m

            def forward(self, a, hh, cc):
                return torch.cat(self.L(a, (hh, cc)), 3)

        run_pair64(Both(), lambda sd, a, hh, cc: torch.cat(ramnet_ref.conv_lstm(sd, "L", a, (hh, cc)), 1), [x, h, c])
    assert [k for e, k in seen if e == Hh.EPI_LSTM] and all(k.startswith(R6) for e, k in seen), seen


@pytest.mark.parametrize("tag", ["seeded_ramnet_lstm", "small_lstm", "small_gru_enclstm"])
def test_reference_golden_forward_lstm_f2x4(tag, monkeypatch):
    """The reference-generated ConvLSTM fixtures with every eligible 3x3 launch forced onto F(2x4,3x3) (tests/test_hip_model.py::
    run_fixture, the tolerances of test_reference_golden_forward_f2x4).  Hidden sizes 8 / 16 / 32 in the narrow variants: the 16- and
    32-channel cells run the F(2x4) kernel, the 8-channel one falls back."""
    from rpg_ramnet_amd import ops, _hip as Hh
    seen, orig, spy = _spy_kernels()
    monkeypatch.setattr(ops, "conv_launch", spy)
    with ops.switches(winograd_2x4="force"):
        thm.run_fixture(tag)
    cells = [k for e, k in seen if e == Hh.EPI_LSTM]
    assert any(k.startswith(R6) for k in cells), sorted(set(cells))
    if tag != "seeded_ramnet_lstm":
        assert any(not k.startswith(R6) for k in cells), "the 8-channel cell cannot run F(2x4)"
    else:
        assert all(k.startswith(R6) for k in cells), sorted(set(cells))


@pytest.mark.parametrize("mode", ["lstm", "enc_lstm", "base_e"])
def test_bptt_gradients_vs_oracle_f2x4(mode, forced):
    """tests/test_hip_model.py::test_bptt_gradients_vs_oracle (loss rtol 1e-4, gradients 2e-3 above 1 % of the largest) with F(2x4)
    forward, backward-data and backward-weights forced."""
    thm.test_bptt_gradients_vs_oracle(mode)


def test_bptt_irregular_batch_f2x4(forced, monkeypatch):
    """An irregular batch (`num_events`) of the ConvLSTM network with F(2x4) forced: masked cell launches inside a differentiated network;
    loss, predictions and every gradient against the float64 per-sample loop (tests/test_hip_irregular.py's scheme and bounds)."""
    from rpg_ramnet_amd import ops, _hip as Hh
    seen, orig, spy = _spy_kernels()
    monkeypatch.setattr(ops, "conv_launch", spy)
    irr.test_irregular_network_vs_oracle("convlstm")
    cells = [k for e, k in seen if e == Hh.EPI_LSTM]
    assert any("masked" in k and k.startswith(R6) for k in cells), sorted(set(cells))


def test_time_batched_stream_lstm_f2x4(forced):
    """The streaming runtime captures graphs: the ConvLSTM layers' F(2x4) packs are built by the eager warm-up (graph._warm) before the
    capture — tests/test_hip_graph.py's ConvLSTM case with F(2x4) forced."""
    import test_hip_graph as thg
    thg.test_time_batched_stream_equals_eager_primitives("net_seeded_ramnet_lstm.npz", 2)


# ------------------------------------------------------------------------------------------------------------ full resolution
# Bound of the two full-resolution runs: the project's own 1e-3 (north star), max-norm and element-wise with ELEM_FLOOR.  The yardstick was
# measured first (profiles/lstm2x4_notes.md): a build of the parent commit, every ConvLSTM launch on F(2x2,3x3), gives worst max-norm /
# element-wise 6.2e-6 / 2.8e-4 over the 48 updates and 5.8e-6 / 2.7e-4 over the 200-update stream — it meets 1e-3, so 1e-3 holds for every
# variant (this tree: off = the parent's figures, auto 6.4e-6 / 2.8e-4 and 5.8e-6 / 2.7e-4, f2x4 6.3e-6 / 2.8e-4 and 6.9e-6 / 3.5e-4,
# f2x4_split 6.9e-6 / 3.4e-4 and 6.9e-6 / 3.5e-4).
LSTM_FULLSIZE_TOL = 1e-3
N_MAP_LSTM = 2048                      # tests/golden/make_golden_fullsize_lstm.py


@pytest.fixture(params=["off", "auto", "f2x4", "f2x4_split"])
def lstm_variant(request):
    """off: every ConvLSTM launch on F(2x2,3x3) (what the tree ran before ABI 27); auto: the library's selection — at batch 1 the two fine
    scales' cell launches (352 and 176 workgroups against the threshold of 150) already run F(2x4); f2x4: every eligible launch forced;
    f2x4_split: the same with split operands (the cell launch stays on the exact-fp32 kernel, the other 3x3 layers split)."""
    from rpg_ramnet_amd import ops
    with ops.switches(winograd_2x4={"off": "off", "auto": "auto"}.get(request.param, "force"), split_operands=request.param == "f2x4_split"):
        yield request.param


class _Worst:
    """Errors of sampled tensors against fullsize_lstm.npz: every figure is printed, the assertion comes at the end."""

    def __init__(self, z):
        self.z, self.lines, self.e, self.ee = z, [], 0.0, 0.0

    def add(self, key, got, what):
        z = self.z
        ref = z[key + ".val"].astype(np.float64)
        g = np.asarray(got, dtype=np.float64).ravel()[fc.sample_idx(key, int(np.asarray(got).size), N_MAP_LSTM)]
        amax = max(float(z[key + ".absmax"]), 1e-30)
        e = float(np.abs(g - ref).max()) / amax
        ee = float((np.abs(g - ref) / np.maximum(np.abs(ref), ELEM_FLOOR * amax)).max())
        self.e, self.ee = max(self.e, e), max(self.ee, ee)
        self.lines.append("%s max-norm %.2e elem %.2e" % (what, e, ee))

    def check(self, what, tol):
        print("\n".join(self.lines))
        print("%s: worst max-norm %.3e, worst element-wise %.3e (bound %.1e)" % (what, self.e, self.ee, tol))
        assert self.e <= tol, "%s: rel err %.3e > %.1e" % (what, self.e, tol)
        assert self.ee <= tol, "%s: element-wise rel err %.3e > %.1e (floor %.0e)" % (what, self.ee, tol, ELEM_FLOOR)


def test_lstm_long_horizon_forward_full_resolution(lstm_variant):
    """48 consecutive ConvLSTM state updates at the real resolution (B = 1, 256 x 344, K = 5, L = 8 packages through
    ERGB2DepthRecurrent.forward) against the float64 oracle: every prediction of every package and the (h, c) pair of the three scales,
    max-norm AND element-wise over the fixture's seeded entries, the last frame prediction over all of its pixels."""
    cfg, _ = ref_cfg("net_seeded_ramnet_lstm.npz", every_x_rgb_frame=5)
    model = build_hip_model("ERGB2DepthRecurrent", cfg).eval()
    wst = _Worst(load_golden("fullsize_lstm.npz"))
    prev, lstm = None, ramnet_ref.empty_states_lstm(5)
    with torch.no_grad():
        for l, item in enumerate(fc.long_horizon_items()):
            preds, supers, lstm = model(item, prev, lstm)
            prev = supers["image"]
            for k in preds:
                wst.add("long.%d.pred.%s" % (l, k), preds[k].cpu().numpy(), "package %d pred %s" % (l, k))
            for i, (h, c) in enumerate(prev):
                wst.add("long.%d.state%d.h" % (l, i), h.cpu().numpy(), "package %d state %d h" % (l, i))
                wst.add("long.%d.state%d.c" % (l, i), c.cpu().numpy(), "package %d state %d c" % (l, i))
    wst.check("48 updates, %s" % lstm_variant, LSTM_FULLSIZE_TOL)
    assert_close(preds["image"].cpu().numpy(), wst.z["long.last_image_full"], LSTM_FULLSIZE_TOL, "last frame prediction, every pixel",
                 elem_tol=LSTM_FULLSIZE_TOL)


def test_lstm_streaming_200_updates_full_resolution(lstm_variant):
    """Batch-1 asynchronous streaming with a persistent (h, c) state: 200 updates at 256 x 344 on the irregular schedule of
    fullsize_cases.stream_200_schedule() through init_states / update_events / update_image / decode, against the float32 oracle:
    predictions at the checkpoints and the final (h, c) of each scale."""
    cfg, _ = ref_cfg("net_seeded_ramnet_lstm.npz")
    model = build_hip_model("ERGB2DepthRecurrent", cfg).eval()
    wst = _Worst(load_golden("fullsize_lstm.npz"))
    states = model.init_states(1, fc.H, fc.W)
    c = 0
    with torch.no_grad():
        for st in fc.stream_200_schedule():
            if st[0] == "events":
                states, _ = model.update_events(st[1], states)
            elif st[0] == "rgb":
                states, _ = model.update_image(st[1], states)
            else:
                wst.add("stream.check%d" % c, model.decode(states).cpu().numpy(), st[1])
                c += 1
    for i, (h, cs) in enumerate(states):
        wst.add("stream.final_state%d.h" % i, h.permute(0, 3, 1, 2).cpu().numpy(), "final state %d h" % i)
        wst.add("stream.final_state%d.c" % i, cs.permute(0, 3, 1, 2).cpu().numpy(), "final state %d c" % i)
    wst.check("200 updates, %s" % lstm_variant, LSTM_FULLSIZE_TOL)
