"""Float64 statement of the batched multi-scale gradient loss (`ramnet_grad_loss_stats`, `ramnet_grad_loss_from_stats`, `ramnet_grad_loss_bwd`),
written from the text of include/ramnet_hip.h and from nothing in csrc/.  Anchored on the CPU by tests/test_grad_loss_restatement_cpu.py.

  diff = f32(pred - target);  P_s = avg_pool2d(diff, 2^s) (trailing rows / columns dropped; a NaN makes its cell NaN)
  g_s  = Sobel / 8 of P_s with replicate padding on P_s's own map; a NaN anywhere in the 3 x 3 window makes both components NaN
  S_s  = sum |g_s| over the non-NaN components, C_s = their count;  loss = w * mean_s (S_s / C_s * Bg * 2)
  dpred = (up + up_sum) * w * gain * sum_s (Bg * 2 / C_s / ns) * d(S_s) / d(pred), sign(0) = 0, C_s given by the caller; a scale with C_s = 0 adds nothing

A pair is a [B][H][W] float64 tensor of fp32 values."""
import torch
import torch.nn.functional as F

F64 = torch.float64
U = 2.0 ** -24
E64 = 2.0 ** -53
TILE = 64
_KX = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype=F64) / 8.0
_K = torch.stack([_KX, _KX.t()])[:, None]
GRAD_ROUNDINGS = 5          # coef_s once from double, coef_s x integer once, three adds over the four scales
SOBEL_ADDS = 5              # six non-zero taps


def f32(t):
    return t.float().to(F64)


def scales_ok(H, W, ns):
    return 1 <= ns <= 4 and (H >> (ns - 1)) >= 1 and (W >> (ns - 1)) >= 1


def workspace_bytes(G, B, H, W):
    """one row of (S_s, C_s) x 4 scales in doubles per 64 x 64 tile, sample and pair"""
    return G * B * (-(-H // TILE)) * (-(-W // TILE)) * 8 * 8


def pool(x, s):
    B, H, W = x.shape
    k, h, w = 1 << s, H >> s, W >> s
    return x[:, :h * k, :w * k].reshape(B, h, k, w, k).mean(dim=(2, 4))


def _conv(P, K):
    return F.conv2d(F.pad(P[:, None], (1, 1, 1, 1), mode="replicate"), K)


def valid(P):
    """[B][h][w] bool: no NaN in the replicate-padded 3 x 3 window"""
    return _conv(torch.isnan(P).to(F64), torch.ones(1, 1, 3, 3, dtype=F64))[:, 0] == 0


def responses(pred, target, ns):
    """per scale (g [B][2][h][w] with 0 where invalid, ok [B][h][w], |K| * |P| [B][2][h][w]: the responses on absolute values)"""
    diff = f32(pred - target)
    out = []
    for s in range(ns):
        P = pool(diff, s)
        ok = valid(P)
        P0 = torch.nan_to_num(P, nan=0.0)
        out.append((_conv(P0, _K) * ok[:, None], ok, _conv(P0.abs(), _K.abs()) * ok[:, None]))
    return out


def stats(pred, target, ns):
    """-> (stats [ns][2] = (S_s, C_s), the same sums on absolute values [ns])"""
    rows, ab = [], []
    for g, ok, ga in responses(pred, target, ns):
        rows.append(torch.stack([g.abs().sum(), 2.0 * ok.sum().to(F64)]))
        ab.append(ga.sum())
    return torch.stack(rows), torch.stack(ab)


def loss_from_stats(st, Bg, weight=1.0):
    """st [ns][2] (or [G][ns][2] with weight [G]); 0 / 0 = NaN"""
    return weight * (st[..., 0] / st[..., 1] * Bg * 2.0).mean(dim=-1)


def backward(pred, target, ns, counts, factor):
    """factor = (up + up_sum) * w * gain * Bg * 2.  -> (dpred, the same adjoint on absolute values), both [B][H][W]"""
    diff = f32(pred - target)
    d0 = torch.nan_to_num(diff, nan=0.0).requires_grad_(True)
    da = d0.detach().abs().requires_grad_(True)
    total, atotal = d0.sum() * 0.0, da.sum() * 0.0
    for s in range(ns):
        if float(counts[s]) <= 0.0:
            continue
        ok = valid(pool(diff, s))[:, None]
        c = factor / float(counts[s]) / ns
        g = _conv(pool(d0, s), _K)
        total = total + c * (g.abs() * ok).sum()
        live = ((g.detach() != 0) & ok).to(F64)
        atotal = atotal + abs(c) * (_conv(pool(da, s), _K.abs()) * live).sum()
    grad, = torch.autograd.grad(total, d0)
    agrad, = torch.autograd.grad(atotal, da)
    return grad, agrad


def grad_bound(agrad):
    """coef_s rounded once from double, the product with the integer once, three adds: 5 x 2^-24 on the absolute-value adjoint (second order
    and the double arithmetic of the coefficient: a factor 1 + 2^-20)"""
    return GRAD_ROUNDINGS * U * (1.0 + 2.0 ** -20) * agrad


def response_bounds(pred, target, ns):
    """fp32 error bound of every response of normal data: 2 roundings per pooling level reach every leaf (the pairs, then their sum; x 0.25 is
    exact), then the 5 adds of the six taps: (2 s + 5) 2^-24 x the response on absolute values"""
    return [(g, ok, (2 * s + SOBEL_ADDS) * U * (1.0 + 2.0 ** -20) * ga) for s, (g, ok, ga) in enumerate(responses(pred, target, ns))]


def unsafe_pixels(pred, target, ns):
    """[B][H][W] bool: a response within reach of the pixel (the 3 x 3 cells around its own cell, at every scale) lies within its own bound
    of zero, so that its sign may differ between fp32 and float64"""
    B, H, W = pred.shape
    bad = torch.zeros(B, H, W, dtype=torch.bool)
    for s, (g, ok, bound) in enumerate(response_bounds(pred, target, ns)):
        near = ((g.abs() <= bound) & (bound > 0)).any(dim=1).to(F64)
        reach = F.max_pool2d(near[:, None], 3, 1, 1)[:, 0] > 0
        k, h, w = 1 << s, H >> s, W >> s
        bad[:, :h * k, :w * k] |= reach.repeat_interleave(k, 1).repeat_interleave(k, 2)
    return bad
