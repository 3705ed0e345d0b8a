"""No GPU: the host side of the batched multi-scale gradient loss (ops.multi_scale_grad_loss_batch, csrc/grad_loss.hip) — argument checks that
must fire before the library is touched, the option switch, and float64 checks of the two pieces of algebra the kernels rest on: per-shard
(S_s, C_s) sums reproduce the oracle's loss on the concatenated batch (the data-parallel form), and the transposed clamped Sobel stencil the
backward gathers with equals the oracle's autograd gradient."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import loss_ref


def _blocks(rng, B, H, W):
    """Targets with block-shaped NaN regions (a corner rectangle per sample and, where there is room, an interior block off the 8-grid)."""
    p = torch.from_numpy(rng.random((B, 1, H, W)))
    t = torch.from_numpy(rng.random((B, 1, H, W)))
    t[:, :, :H // 3, :W // 3] = float("nan")
    if H >= 64:
        t[:, :, H // 2 - 4:H // 2 + 5, W // 2 - 5:W // 2 + 6] = float("nan")
    return p, t


def _stats(p, t, ns=4):
    """(S_s, C_s) with the oracle's own spatial_gradient: [ns, 2] float64."""
    out = torch.zeros(ns, 2, dtype=torch.float64)
    d = p - t
    for s in range(ns):
        g = loss_ref.spatial_gradient(F.avg_pool2d(d, 2 ** s, 2 ** s))
        ok = ~torch.isnan(g)
        out[s, 0], out[s, 1] = g[ok].abs().sum(), ok.sum()
    return out


def test_argument_errors_are_raised_before_the_library_is_touched(monkeypatch):
    from rpg_ramnet_amd import _hip, ops

    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_hip, "lib", boom)
    a, b = torch.zeros(2, 1, 16, 16), torch.zeros(2, 1, 16, 16)
    with pytest.raises(ValueError, match="GPU"):
        ops.multi_scale_grad_loss_batch([a], [b])
    with pytest.raises(ValueError, match="no pairs"):
        ops.multi_scale_grad_loss_batch([], [])
    with pytest.raises(ValueError, match="1 predictions, 2 targets"):
        ops.multi_scale_grad_loss_batch([a], [b, b])
    with pytest.raises(ValueError):
        ops.msg_local_stats([a], [b])
    with pytest.raises(ValueError, match="B x 1 x H x W"):
        ops.multi_scale_grad_loss_batch([torch.zeros(2, 16, 16)], [torch.zeros(2, 16, 16)])
    with pytest.raises(ValueError, match="every prediction and target"):
        ops.multi_scale_grad_loss_batch([a, torch.zeros(2, 1, 16, 20)], [b, torch.zeros(2, 1, 16, 20)])
    with pytest.raises(ValueError, match="every prediction and target"):
        ops.multi_scale_grad_loss_batch([a], [torch.zeros(2, 1, 16, 20)])


def test_option_getter_and_setter():
    from rpg_ramnet_amd import ops
    assert ops.grad_loss_batched() is True                     # default: on
    with ops.switches(grad_loss_batched=False):
        assert ops.grad_loss_batched() is False
        ops.set_grad_loss_batched(1)
        assert ops.grad_loss_batched() is True


def test_header_and_ctypes_table_carry_the_entry_points():
    from rpg_ramnet_amd import _hip, build
    names = {"ramnet_grad_loss_workspace", "ramnet_grad_loss_stats", "ramnet_grad_loss_from_stats", "ramnet_grad_loss_bwd",
             "ramnet_fill_pointer_table"}
    assert names <= set(_hip.EXPORTS)
    assert "grad_loss.hip" in build.sources()


@pytest.mark.parametrize("B,H,W", [(4, 35, 53), (3, 77, 141)])
def test_shard_statistics_add_up_to_the_loss_of_the_whole_batch(B, H, W):
    """loss = mean_s (sum_shards S_s / sum_shards C_s * B * 2): what _sequence_loss_dp_exact all-reduces.  The mean of per-shard losses is NOT
    that value (every scale normalises by its own count), which the second assertion records."""
    rng = np.random.default_rng(11)
    p, t = _blocks(rng, B, H, W)
    t[0, :, :H // 3 + 3, :W // 3 + 5] = float("nan")           # shards with different valid counts
    whole = float(loss_ref.multi_scale_grad_loss(p, t))
    assert np.isfinite(whole)
    st = _stats(p[:1], t[:1]) + _stats(p[1:], t[1:])
    from_stats = float((st[:, 0] / st[:, 1] * B * 2).mean())
    np.testing.assert_allclose(from_stats, whole, rtol=1e-12)
    naive = float(loss_ref.multi_scale_grad_loss(p[:1], t[:1])) + float(loss_ref.multi_scale_grad_loss(p[1:], t[1:]))
    assert abs(naive - whole) > 1e-6 * abs(whole)


def _dp8(sx, sy):
    """8 dP of one level from the signs of its Sobel components ([B, h, w] each): the integer gather of gl_bwd_kernel —
    Sy^T Dx^T sx + Dy^T Sx^T sy with the transposes of the clamped operators S = [1 2 1], D = [-1 0 1]."""
    def St(a, dim):
        n = a.shape[dim]
        i = torch.arange(n)
        return a.index_select(dim, (i - 1).clamp(min=0)) + 2 * a + a.index_select(dim, (i + 1).clamp(max=n - 1))

    def Dt(a, dim):
        n = a.shape[dim]
        i = torch.arange(n)
        shape = [1] * a.dim()
        shape[dim] = n
        fl = torch.where(i > 0, 1.0, -1.0).reshape(shape).to(a.dtype)
        fh = torch.where(i < n - 1, 1.0, -1.0).reshape(shape).to(a.dtype)
        return fl * a.index_select(dim, (i - 1).clamp(min=0)) - fh * a.index_select(dim, (i + 1).clamp(max=n - 1))
    return St(Dt(sx, 2), 1) + Dt(St(sy, 2), 1)


@pytest.mark.parametrize("B,H,W,nan", [(2, 35, 53, True), (1, 20, 28, False), (1, 16, 16, False), (2, 77, 141, True), (1, 8, 9, False)])
def test_transposed_stencil_gather_equals_autograd(B, H, W, nan):
    rng = np.random.default_rng(3)
    p, t = _blocks(rng, B, H, W) if nan else (torch.from_numpy(rng.random((B, 1, H, W))), torch.from_numpy(rng.random((B, 1, H, W))))
    pr = p.clone().requires_grad_(True)
    loss_ref.multi_scale_grad_loss(pr, t).backward()
    ns, d = 4, p - t
    grad = torch.zeros(B, H, W, dtype=torch.float64)
    for s in range(ns):
        k = 2 ** s
        g = loss_ref.spatial_gradient(F.avg_pool2d(d, k, k))[:, 0]          # [B, 2, h, w]
        sg = torch.where(torch.isnan(g), torch.zeros_like(g), torch.sign(g))
        cnt = float((~torch.isnan(g)).sum())
        dP = _dp8(sg[:, 0], sg[:, 1]) * (B * 2.0 / cnt / ns / (k * k) / 8.0)
        h, w = dP.shape[1:]
        grad[:, :h * k, :w * k] += dP.repeat_interleave(k, 1).repeat_interleave(k, 2)
    np.testing.assert_allclose(grad.numpy(), pr.grad[:, 0].numpy(), rtol=0, atol=1e-14)
    assert float(grad[torch.isnan(t[:, 0])].abs().max() if nan else 0.0) == 0.0        # pixels under a NaN target get 0
