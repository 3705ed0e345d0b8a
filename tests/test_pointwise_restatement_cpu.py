"""CPU: anchors of tests/pointwise_restatement.py, the float64 reference of tests/test_hip_pointwise.py — its adjoints against their
forwards (dot-product test), its layout maps against torch and the header's index formulas, its cell backward maps against the oracle's
cells differentiated in float64."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ramnet_ref
import pointwise_restatement as pr

F64 = torch.float64


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


def _dot_ok(lhs, rhs):
    assert abs(float(lhs) - float(rhs)) <= 1e-12 * max(abs(float(lhs)), abs(float(rhs))), (float(lhs), float(rhs))


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 3, 4), (1, 2, 2, 4), (2, 2, 7, 4), (1, 5, 11, 8), (2, 8, 16, 4)])
def test_adjoints_pass_the_dot_product_test(B, H, W, C):
    x = _rand(B, H, W, C, seed=1)
    # <pad2_sum x, y> = <x, unpad2_fold y>
    y = _rand(B, H + 4, W + 4, C, seed=2)
    _dot_ok((pr.pad2_sum(x) * y).sum(), (x * pr.unpad2_fold(y)).sum())
    # <up2x x, y> = <x, upsample2x_bwd y>
    y = _rand(B, 2 * H, 2 * W, C, seed=3)
    _dot_ok((pr.up2x(x) * y).sum(), (x * pr.upsample2x_bwd(y)).sum())
    # <im2col x, (r, c)> = <x, col2im(r, c)>, and col2im accumulates into what dx holds
    gr, gc = _rand(2, B, 2 * W, 5, C, seed=4), _rand(2, B, 2 * H, 5, C, seed=5)
    rows, cols = pr.up2x_border_im2col(x)
    dx0 = _rand(B, H, W, C, seed=6)
    got = pr.up2x_border_col2im(gr, gc, dx0) - dx0
    _dot_ok((rows * gr).sum() + (cols * gc).sum(), (x * got).sum())
    # only border pixels receive
    if H > 2 and W > 2:
        assert float(got[:, 1:-1, 1:-1].abs().max()) == 0.0


def test_border_im2col_is_the_unrolled_upsample():
    """entry (o, k): rows clamp the column o + k - 2, cols are zero outside the image — against a plain loop over the upsampled tensor"""
    B, H, W, C = 2, 3, 4, 4
    x, s = _rand(B, H, W, C, seed=7), _rand(B, H, W, C, seed=8)
    u = pr.up2x(x + s)
    rows, cols = pr.up2x_border_im2col(x, s)
    assert rows.shape == (2, B, 2 * W, 5, C) and cols.shape == (2, B, 2 * H, 5, C)
    for side in range(2):
        for o in range(2 * W):
            for k in range(5):
                assert torch.equal(rows[side, :, o, k], u[:, (2 * H - 1) * side, min(max(o + k - 2, 0), 2 * W - 1)])
        for o in range(2 * H):
            for k in range(5):
                r = o + k - 2
                want = u[:, r, (2 * W - 1) * side] if 0 <= r < 2 * H else torch.zeros(B, C, dtype=F64)
                assert torch.equal(cols[side, :, o, k], want)
    p = pr.pad2_sum(x, s)
    assert torch.equal(p[:, 2:-2, 2:-2], x + s) and torch.equal(p[:, 0, 0], (x + s)[:, 0, 0]) and torch.equal(p[:, -1, 3], (x + s)[:, -1, 1])


@pytest.mark.parametrize("H,W,enc,want", [(260, 346, 3, (264, 352, 2, 2, 3, 3)), (5, 7, 3, (8, 8, 2, 1, 1, 0))])
def test_reflect_pad_is_reflectionpad2d_with_crop_parameters(H, W, enc, want):
    Hc, Wc, top, bottom, left, right = pr.crop_parameters(H, W, enc)
    assert (Hc, Wc, top, bottom, left, right) == want
    src = _rand(2, 5, H, W, seed=9)
    ref = torch.nn.ReflectionPad2d((left, right, top, bottom))(src)
    assert torch.equal(pr.reflect_pad(src, top, left, Hc, Wc, 8, 0), ref)
    nhwc = pr.reflect_pad(src, top, left, Hc, Wc, 8, 1)
    assert nhwc.shape == (2, Hc, Wc, 8)
    assert torch.equal(nhwc[..., :5], ref.permute(0, 2, 3, 1)) and float(nhwc[..., 5:].abs().max()) == 0.0
    assert torch.equal(pr.nchw_to_nhwc_pad(src, 8)[..., :5], src.permute(0, 2, 3, 1))


def test_space_to_depth_channel_order_and_round_trip():
    B, H, W, C = 2, 4, 6, 4
    x = _rand(B, H, W, C, seed=10)
    d = pr.space_to_depth2(x)
    assert d.shape == (B, H // 2, W // 2, 4 * C)
    for a in range(2):
        for c in range(2):
            for ch in range(C):
                assert torch.equal(d[..., (a * 2 + c) * C + ch], x[:, a::2, c::2, ch])
    assert torch.equal(pr.space_to_depth2(d, inverse=True), x)


def test_frame_gather_and_concat():
    B, H2, W2, C = 2, 6, 8, 4
    dy, m = _rand(B, H2, W2, C, seed=11), _rand(B, H2, W2, C, seed=12)
    rows, cols = pr.frame_gather(dy, m)
    g = dy * (m > 0)
    for slot in range(2):
        assert torch.equal(rows[0, :, :, slot], g[:, slot]) and torch.equal(rows[1, :, :, slot], g[:, H2 - 2 + slot])
        assert torch.equal(cols[0, :, :, slot], g[:, :, slot]) and torch.equal(cols[1, :, :, slot], g[:, :, W2 - 2 + slot])
    a, b = _rand(5, 4, seed=13), _rand(5, 8, seed=14)
    a2, b2 = pr.split2(pr.concat2(a, b), 4, 8)
    assert torch.equal(a, a2) and torch.equal(b, b2)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("with_h", [True, False])
def test_gru_maps_equal_the_oracle_cell_differentiated(seed, with_h):
    """One pixel, C = 4: the bias gradients of the oracle's three gate convolutions ARE the pre-activation gradients, and the gradient of
    the state is the two point-wise parts plus the convolutions' backward-data (centre taps: the image is one pixel)."""
    C = 4
    g = torch.Generator().manual_seed(100 + seed)
    sd = {}
    for gate in ("update_gate", "reset_gate", "out_gate"):
        sd["cell.%s.weight" % gate] = (torch.randn(C, 2 * C, 3, 3, dtype=F64, generator=g) * 0.5).requires_grad_(True)
        sd["cell.%s.bias" % gate] = (torch.randn(C, dtype=F64, generator=g) * 0.5).requires_grad_(True)
    x = torch.randn(1, C, 1, 1, dtype=F64, generator=g)
    h = torch.randn(1, C, 1, 1, dtype=F64, generator=g).requires_grad_(True) if with_h else None
    dhn = torch.randn(1, C, 1, 1, dtype=F64, generator=g)
    hn = ramnet_ref.conv_gru(sd, "cell", x, h)
    leaves = [sd["cell.update_gate.bias"], sd["cell.reset_gate.bias"], sd["cell.out_gate.bias"]] + ([h] if with_h else [])
    grads = torch.autograd.grad(hn, leaves, dhn)
    # the saved activations, as the kernels see them
    with torch.no_grad():
        hv = h if with_h else torch.zeros_like(x)
        xh = torch.cat([x, hv], 1)
        u = torch.sigmoid(F.conv2d(xh, sd["cell.update_gate.weight"], sd["cell.update_gate.bias"], 1, 1))
        r = torch.sigmoid(F.conv2d(xh, sd["cell.reset_gate.weight"], sd["cell.reset_gate.bias"], 1, 1))
        o = torch.tanh(F.conv2d(torch.cat([x, hv * r], 1), sd["cell.out_gate.weight"], sd["cell.out_gate.bias"], 1, 1))
    flat = lambda t: t.reshape(1, C)
    hk = flat(hv) if with_h else None
    dpo, dpu, dh = pr.gru_bwd_a(flat(dhn), flat(u), flat(o), hk)
    wc = lambda gate: sd["cell.%s.weight" % gate].detach()[:, C:, 1, 1]             # [out][hidden in], centre tap
    dhr = dpo @ wc("out_gate")
    dpr, dh = pr.gru_bwd_b(dhr, flat(r), dh, hk)
    tol = dict(rtol=1e-10, atol=1e-13)
    torch.testing.assert_close(dpu, flat(grads[0]), **tol)
    torch.testing.assert_close(dpr, flat(grads[1]), **tol)
    torch.testing.assert_close(dpo, flat(grads[2]), **tol)
    if with_h:
        torch.testing.assert_close(dh + dpu @ wc("update_gate") + dpr @ wc("reset_gate"), flat(grads[3]), **tol)
    else:
        assert float(dpr.abs().max()) == 0.0


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("with_state", [True, False])
def test_lstm_map_equals_the_oracle_cell_differentiated(seed, with_state):
    C = 4
    g = torch.Generator().manual_seed(200 + seed)
    sd = {"cell.Gates.weight": torch.randn(4 * C, 2 * C, 3, 3, dtype=F64, generator=g) * 0.5,
          "cell.Gates.bias": (torch.randn(4 * C, dtype=F64, generator=g) * 0.5).requires_grad_(True)}
    x = torch.randn(1, C, 1, 1, dtype=F64, generator=g)
    hp = torch.randn(1, C, 1, 1, dtype=F64, generator=g)
    cp = torch.randn(1, C, 1, 1, dtype=F64, generator=g).requires_grad_(True)
    dhn, dcn = torch.randn(1, C, 1, 1, dtype=F64, generator=g), torch.randn(1, C, 1, 1, dtype=F64, generator=g)
    hn, cn = ramnet_ref.conv_lstm(sd, "cell", x, (hp, cp) if with_state else None)
    leaves = [sd["cell.Gates.bias"]] + ([cp] if with_state else [])
    grads = torch.autograd.grad((hn, cn), leaves, (dhn, dcn))
    with torch.no_grad():
        pre = F.conv2d(torch.cat([x, hp if with_state else torch.zeros_like(x)], 1), sd["cell.Gates.weight"], sd["cell.Gates.bias"], 1, 1).reshape(1, 4 * C)
        gates = torch.cat([torch.sigmoid(pre[:, :3 * C]), torch.tanh(pre[:, 3 * C:])], 1)
    flat = lambda t: t.detach().reshape(1, C)
    dpre, dcp = pr.lstm_bwd(gates, flat(cn), flat(cp) if with_state else None, flat(dhn), flat(dcn))
    tol = dict(rtol=1e-10, atol=1e-13)
    torch.testing.assert_close(dpre, grads[0].reshape(1, 4 * C), **tol)
    if with_state:
        torch.testing.assert_close(dcp, flat(grads[1]), **tol)
    # one cotangent at a time = the other one absent
    a, _ = pr.lstm_bwd(gates, flat(cn), flat(cp), flat(dhn), None)
    b, _ = pr.lstm_bwd(gates, flat(cn), flat(cp), None, flat(dcn))
    full, _ = pr.lstm_bwd(gates, flat(cn), flat(cp), flat(dhn), flat(dcn))
    torch.testing.assert_close(a + b, full, **tol)


def test_lstm_masked_rule_and_prediction_head():
    C, hw = 4, 3
    gates = torch.cat([torch.sigmoid(_rand(3 * hw, 3 * C, seed=20)), torch.tanh(_rand(3 * hw, C, seed=21))], 1)
    cn, cp, dh, dc = (_rand(3 * hw, C, seed=s) for s in (22, 23, 24, 25))
    dpre, dcp, dxh = pr.lstm_bwd_masked(gates, cn, [1, 0, 1], hw, cp, dh, dc)
    ref_pre, ref_dcp = pr.lstm_bwd(gates, cn, cp, dh, dc)
    on = torch.tensor([0, 1, 2, 6, 7, 8])
    off = torch.tensor([3, 4, 5])
    assert torch.equal(dpre[on], ref_pre[on]) and torch.equal(dcp[on], ref_dcp[on]) and float(dxh[on].abs().max()) == 0.0
    assert float(dpre[off].abs().max()) == 0.0 and torch.equal(dcp[off], dc[off])
    assert torch.equal(dxh[off, C:], dh[off]) and float(dxh[off, :C].abs().max()) == 0.0
    # prediction head: the documented gradients dz = dy y (1 - y), dx = dz w, dw = sum dz x, db = sum dz
    x, w, b, dy = _rand(7, 8, seed=26), _rand(8, seed=27), _rand(1, seed=28)[0], _rand(7, seed=29)
    y = pr.pred_fwd(x, w, b)
    dx, dw, db = pr.pred_bwd(x, w, dy, y, dw0=torch.ones(8, dtype=F64), db0=torch.tensor(2.0, dtype=F64))
    dz = dy * y * (1 - y)
    tol = dict(rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(dx, dz[:, None] * w[None], **tol)
    torch.testing.assert_close(dw, 1 + (dz[:, None] * x).sum(0), **tol)
    torch.testing.assert_close(db, 2 + dz.sum(), **tol)
    dx, dw, db = pr.pred_bwd(x, w, dy)
    torch.testing.assert_close(dw, (dy[:, None] * x).sum(0), **tol)
    assert torch.equal(pr.bias_grad(x, None, torch.zeros(8, dtype=F64)), x.sum(0))
