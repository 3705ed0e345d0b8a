"""No GPU: the float64 statements of the input-gradient launches (tests/input_grad_restatement.py) anchored against torch's own
gradients, the three entry points in the header / binding / library, what they refuse before any launch, and the flag handling of
inference.input_gradients."""
import ctypes as C
import os
import re

import pytest
import torch

import input_grad_restatement as R

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ramnet_head_dgrad", "ramnet_nhwc_unpad_to_nchw", "ramnet_reflect_pad_bwd")
PAD_CASES = R.PAD_CASES


def ri(*shape, seed, m):
    return torch.randint(-m, m + 1, shape, generator=torch.Generator().manual_seed(seed)).to(F64)


def test_crop_split_is_crop_parameters():
    from rpg_ramnet_amd.ops import CropParameters
    for h, w, enc in ((5, 7, 3), (20, 22, 5), (260, 346, 3)):
        cp = CropParameters(w, h, enc)
        assert R.crop_split(h, w, enc) == (cp.height_crop_size, cp.width_crop_size, cp.padding_top, cp.padding_left)
    assert PAD_CASES[0] == (5, 7, 8, 8, 2, 1) and PAD_CASES[2] == (20, 22, 32, 32, 6, 5)


@pytest.mark.parametrize("cin", [1, 3, 5, 10])
@pytest.mark.parametrize("cout,masked", [(32, True), (7, False), (7, True)])
def test_head_dgrad_statement_is_conv2d_input(cin, cout, masked):
    B, H, W = 2, 6, 9
    dy, w = ri(B, H, W, cout, seed=1, m=4), ri(cout, cin, 5, 5, seed=2, m=3)
    y = ri(B, H, W, cout, seed=3, m=2) if masked else None
    g = dy if y is None else dy * (y > 0)
    ref = torch.nn.grad.conv2d_input((B, cin, H, W), w, g.permute(0, 3, 1, 2), stride=1, padding=2)
    got = R.head_dgrad(dy, w, y)
    ld = (cin + 3) // 4 * 4
    assert got.shape == (B, H, W, ld)
    assert torch.equal(got[..., :cin], ref.permute(0, 2, 3, 1)) and float(got[..., cin:].abs().sum()) == 0.0
    # the companion: the same expression on absolute values bounds every partial sum
    top = R.head_dgrad(dy, w, y, absolute=True)
    assert bool((top >= got.abs()).all()) and R.head_dgrad_partial_max(dy, w, y) == float(top.max())
    refa = torch.nn.grad.conv2d_input((B, cin, H, W), w.abs(), g.abs().permute(0, 3, 1, 2), stride=1, padding=2)
    assert torch.equal(top[..., :cin], refa.permute(0, 2, 3, 1))


@pytest.mark.parametrize("nhwc", [0, 1])
@pytest.mark.parametrize("H,W,Hc,Wc,top,left", PAD_CASES)
def test_reflect_pad_bwd_statement_is_the_gradient_of_reflectionpad2d(H, W, Hc, Wc, top, left, nhwc):
    B, Cc, Cpad = 2, 5, 8
    g = ri(B, Cc, Hc, Wc, seed=4, m=9)
    x = torch.zeros(B, Cc, H, W, dtype=F64, requires_grad=True)
    torch.nn.ReflectionPad2d((left, Wc - W - left, top, Hc - H - top))(x).backward(g)
    gin = g
    if nhwc:
        gin = torch.full((B, Hc, Wc, Cpad), float("nan"), dtype=F64)     # the pad lanes are not read
        gin[..., :Cc] = g.permute(0, 2, 3, 1)
    got = R.reflect_pad_bwd(gin, Cc, H, W, top, left, nhwc)
    assert torch.equal(got, x.grad)
    assert torch.equal(R.reflect_pad_bwd(gin, Cc, H, W, top, left, nhwc, absolute=True),
                       R.reflect_pad_bwd(gin.abs(), Cc, H, W, top, left, nhwc))
    most = max(len(R.mirrors(s, H, top, Hc)) for s in range(H)) * max(len(R.mirrors(s, W, left, Wc)) for s in range(W))
    assert most <= 9 and (most == 9) == ((Hc, Wc) == (11, 13))
    # every padded position is summed exactly once
    ones = R.reflect_pad_bwd(torch.ones(1, 1, Hc, Wc, dtype=F64), 1, H, W, top, left, 0)
    assert float(ones.sum()) == Hc * Wc


def test_nhwc_unpad_statement_inverts_the_repack():
    import pointwise_restatement as pr
    src = ri(2, 5, 3, 4, seed=5, m=9)
    assert torch.equal(R.nhwc_unpad(pr.nchw_to_nhwc_pad(src, 8), 5), src)


def test_header_binding_and_library_carry_the_three_entry_points():
    """Fails without the feature: the parent has none of the three."""
    from rpg_ramnet_amd import _hip
    src = open(os.path.join(ROOT, "include", "ramnet_hip.h")).read()
    L = _hip.lib()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, src), name
        assert name in _hip.EXPORTS and getattr(L, name) is not None
        assert _hip._SIGS[name][0] is C.c_int and _hip._SIGS[name][1][-1] is C.c_void_p
    assert len(_hip._SIGS["ramnet_head_dgrad"][1]) == 13 and len(_hip._SIGS["ramnet_reflect_pad_bwd"][1]) == 13
    assert len(_hip._SIGS["ramnet_nhwc_unpad_to_nchw"][1]) == 8
    assert int(re.search(r"#define RAMNET_ABI_VERSION (\d+)", src).group(1)) == 27 and L.ramnet_abi_version() == 27
    assert "padded rows ascending" in src          # the order of the reflect-pad gather is stated where the test restates it


def test_refusals_need_no_device():
    """Every documented precondition, violated once: RAMNET_E_BADARG and the message, before any HIP call (the pointers are never read)."""
    from rpg_ramnet_amd import _hip
    L = _hip.lib()
    p, odd = C.c_void_p(4096), C.c_void_p(4100)
    good = dict(dy=p, ldg=32, y=p, ldgm=32, w=p, dx=p, ld=8, B=1, H=4, W=4, Cin=5, Cout=32)
    order = ("dy", "ldg", "y", "ldgm", "w", "dx", "ld", "B", "H", "W", "Cin", "Cout")
    bad = [dict(dy=None), dict(w=None), dict(dx=None), dict(B=0), dict(H=0), dict(W=0), dict(Cin=2, ld=4), dict(Cin=6), dict(Cout=33, ldg=36),
           dict(Cout=0), dict(ld=12), dict(ld=5), dict(ldg=30), dict(ldg=28), dict(dy=odd), dict(ldgm=30), dict(ldgm=28), dict(y=odd),
           dict(w=C.c_void_p(4097)), dict(dx=C.c_void_p(4098)), dict(B=1 << 30, H=17, W=33)]
    for over in bad:
        a = dict(good, **over)
        assert L.ramnet_head_dgrad(*[a[k] for k in order], None) == 10001, over
        assert b"bad argument" in L.ramnet_last_error(), over
    for args in ((None, p, 1, 5, 2, 2, 8), (p, None, 1, 5, 2, 2, 8), (p, p, 0, 5, 2, 2, 8), (p, p, 1, 5, 2, 2, 4), (p, p, 1, 5, 2, 2, 6)):
        assert L.ramnet_nhwc_unpad_to_nchw(*args, None) == 10001 and b"bad argument" in L.ramnet_last_error()
    for args in ((None, p, 1, 5, 5, 7, 8, 2, 1, 8, 8, 1), (p, p, 1, 5, 5, 7, 6, 2, 1, 8, 8, 1), (p, p, 1, 5, 5, 7, 4, 2, 1, 8, 8, 1),
                 (p, p, 1, 1, 2, 7, 4, 2, 1, 8, 8, 0), (p, p, 1, 1, 5, 7, 4, 2, 1, 6, 8, 0), (p, p, 1, 5, 5, 7, 8, 6, 1, 16, 16, 1)):
        assert L.ramnet_reflect_pad_bwd(*args, None) == 10001 and b"bad argument" in L.ramnet_last_error()


class _Toy(torch.nn.Module):
    gpu, every_x_rgb_frame = "cpu", 1

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.ones(3))
        self.b = torch.nn.Parameter(torch.ones(2), requires_grad=False)


def test_input_gradients_restores_every_flag_also_when_the_loss_raises(monkeypatch):
    from rpg_ramnet_amd import inference, trainer
    m = _Toy()
    seen = {}

    def loss(model, seq, lc, lw, **kw):
        seen["flags"] = [p.requires_grad for p in model.parameters()]
        seen["leaves"] = [(k, v.requires_grad, v.is_leaf) for it in seq for k, v in sorted(it.items()) if torch.is_tensor(v)]
        seen["lw"], seen["kw"] = lw, kw
        if kw.get("grad_loss_weight") == "boom":
            raise RuntimeError("boom")
        total = sum((it["events0"] * 2.0).sum() + (it["image"].double() * 3.0).sum() for it in seq)
        return total, total.detach()
    monkeypatch.setattr(trainer, "sequence_loss", loss)
    seq = [dict(events0=torch.ones(1, 5, 2, 2), image=torch.ones(1, 1, 2, 2, dtype=F64), depth_image=torch.ones(1, 1, 2, 2), num_events=[1])
           for _ in range(2)]
    total, grads = inference.input_gradients(m, seq, ["image"])
    assert [p.requires_grad for p in m.parameters()] == [True, False] and seen["flags"] == [False, False]
    assert seen["leaves"] == [("depth_image", False, True), ("events0", True, True), ("image", True, True)] * 2 and seen["lw"] == [1.0]
    assert float(total) == 2 * (5 * 4 * 2.0 + 4 * 3.0) and not total.requires_grad
    assert len(grads) == 2 and all(set(g) == {"events0", "image"} for g in grads)
    for g, it in zip(grads, seq):
        assert torch.equal(g["events0"], torch.full((1, 5, 2, 2), 2.0)) and g["image"].dtype == F64 and torch.equal(g["image"], torch.full((1, 1, 2, 2), 3.0, dtype=F64))
        assert not it["events0"].requires_grad and it["events0"].grad is None       # the caller's tensors are left alone
    assert m.a.grad is None and m.b.grad is None
    with pytest.raises(RuntimeError, match="boom"):
        inference.input_gradients(m, seq, ["image"], [2.0], grad_loss_weight="boom")
    assert [p.requires_grad for p in m.parameters()] == [True, False] and seen["lw"] == [2.0]


def test_pack_input_without_requires_grad_is_the_bare_launch(monkeypatch):
    """The path that exists today: one launch through _pack_input_launch, no autograd node built."""
    from rpg_ramnet_amd import ops
    calls = []
    monkeypatch.setattr(ops, "_pack_input_launch", lambda x, crop: calls.append((x.requires_grad, crop)) or x)
    monkeypatch.setattr(ops.PackInput, "apply", lambda x, crop: calls.append("function") or x)
    x = torch.ones(1, 5, 2, 2)
    ops.pack_input(x, "cpu")
    with torch.no_grad():
        ops.pack_input(x.clone().requires_grad_(True), "cpu")
    assert calls == [(False, None), (True, None)]
    ops.pack_input(x.double().requires_grad_(True), "cpu")
    assert calls[-1] == "function"
