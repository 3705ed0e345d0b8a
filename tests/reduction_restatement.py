"""TEST INFRASTRUCTURE ONLY: float64 statements of the reduction entry points outside the convolutions: the loss / statistics half of
csrc/loss_voxel.hip, csrc/norm.hip and csrc/gemm_skinny.hip, one function per entry point, written from the comments of
include/ramnet_hip.h and the reference's formulas (oracle/loss_ref.py), not from the kernels.  tests/test_reduction_restatement_cpu.py
anchors them on the CPU; tests/test_hip_reductions.py compares the kernels with them.

Steps that the header documents as fp32 (d = pred - target, the pooled mean, the half-resolution cell) are rounded to fp32 here (`f32`);
everything else is float64.  Inputs are float64 tensors holding fp32-representable values; NaN marks an invalid target."""
import torch
import torch.nn.functional as F

F64 = torch.float64


def f32(t):
    """one fp32 rounding of a float64 value"""
    return t.to(torch.float32).to(F64)


# ------------------------------------------------------------------------------------------------ scale-invariant losses
def si_diff(pred, target, log=False):
    """d of model/loss.py:6-9 (fp32 difference) or :12-15 (log(pred) - log(target), left in float64: logf is a measured intrinsic)"""
    return torch.log(pred) - torch.log(target) if log else f32(pred - target)


def si_stats(pred, target, log=False):
    """(sum d, sum d^2, count) over the non-NaN d, as a float64 vector"""
    d = si_diff(pred.reshape(-1), target.reshape(-1), log)
    d = d[~torch.isnan(d)]
    return torch.stack([d.sum(), (d * d).sum(), torch.tensor(float(d.numel()), dtype=F64)])


def si_stats_abs(pred, target, log=False):
    """the same sums on absolute values: what the derived bounds are taken of"""
    d = si_diff(pred.reshape(-1), target.reshape(-1), log)
    d = d[~torch.isnan(d)].abs()
    return torch.stack([d.sum(), (d * d).sum()])


def si_loss_from_stats(stats, weight=1.0, lam=1.0):
    """w (S2 / N - lambda (S1 / N)^2); N = 0 gives NaN"""
    S1, S2, N = stats[0], stats[1], stats[2]
    m = S1 / N
    return weight * (S2 / N - lam * m * m)


def si_bwd(pred, target, stats, weight=1.0, lam=1.0, gscale=1.0, log=False):
    """gscale w (2 d / N - 2 lambda mean / N) on valid pixels (divided by pred for the log form), 0 elsewhere; the statistics are GIVEN"""
    d = si_diff(pred, target, log)
    N, mean = stats[2], stats[0] / stats[2]
    g = gscale * weight * 2.0 / N * (d - lam * mean)
    if log:
        g = g / pred
    return torch.where(torch.isnan(d), torch.zeros_like(g), g)


# ------------------------------------------------------------------------------------------------ mse term
def mse_cell(m, half):
    """[B][H][W] -> the map the loss is taken on: itself, or F.interpolate(scale 0.5, bilinear, align_corners=False) = the mean of the 2 x 2
    block in torch's order of operations (each fp32; the halvings are exact), an odd trailing row / column dropped"""
    if not half:
        return m
    H2, W2 = m.shape[1] // 2, m.shape[2] // 2
    m = m[:, :2 * H2, :2 * W2]
    a, b, c, d = m[:, 0::2, 0::2], m[:, 0::2, 1::2], m[:, 1::2, 0::2], m[:, 1::2, 1::2]
    return f32(0.5 * f32(0.5 * a + 0.5 * b) + 0.5 * f32(0.5 * c + 0.5 * d))


def mse_stats(pred, target, half):
    """(sum d^2, count) over the cells whose TARGET cell is not NaN, d = cell(pred) - cell(target) in fp32"""
    t = mse_cell(target, half)
    d = f32(mse_cell(pred, half) - t)[~torch.isnan(t)]
    return torch.stack([(d * d).sum(), torch.tensor(float(d.numel()), dtype=F64)])


def mse_loss(stats):
    return stats[0] / stats[1]


def mse_bwd(pred, target, half, stats, gscale=1.0):
    """gscale d loss / d pred [B][H][W] with the count GIVEN: 2 d / N per cell, a quarter of it to each pixel of a block under `half`;
    masked cells and the dropped odd row / column get 0"""
    t = mse_cell(target, half)
    d = f32(mse_cell(pred, half) - t)
    g = torch.where(torch.isnan(t), torch.zeros_like(d), gscale * 2.0 / stats[1] * d)
    if not half:
        return g
    out = torch.zeros_like(pred)
    H2, W2 = g.shape[1], g.shape[2]
    out[:, :2 * H2, :2 * W2] = (0.25 * g).repeat_interleave(2, 1).repeat_interleave(2, 2)
    return out


# ------------------------------------------------------------------------------------------------ depth metrics
DEPTH_EPS = 1e-5


def metric_depths(pred, target, clip, reg):
    """evaluation.py:74-96: d = exp(reg (y - 1)) clip, the prediction clipped to [exp(-reg) clip, clip] (float64 throughout)"""
    t = torch.exp(reg * (target - 1.0)) * clip
    p = (torch.exp(reg * (pred - 1.0)) * clip).clamp(float(torch.exp(torch.tensor(-reg, dtype=F64))) * clip, clip)
    return t, p


def depth_metric_terms(t, p):
    """the seven per-pixel terms of out11[2..7] and the ratio of the three thresholds, from metric depths"""
    d = t - p
    ld = torch.log(t + DEPTH_EPS) - torch.log(p + DEPTH_EPS)
    ratio = torch.maximum(t / (p + DEPTH_EPS), p / (t + DEPTH_EPS))
    return [d.abs() / (t + 1e-6), d * d / (t * t + 1e-6), d * d, ld * ld, ld.abs(), d.abs()], ratio


def depth_metrics(pred, target, clip, reg, cutoff):
    """out11: n (non-NaN targets in the mask), n_mask (mask = nan_to_num(metric target) < cutoff), then over the n pixels the six sums
    and the counts of ratio <= 1.25, 1.25^2, 1.25^3"""
    t, p = metric_depths(pred.reshape(-1), target.reshape(-1), clip, reg)
    nan = torch.isnan(target.reshape(-1))
    mask = nan | (t < cutoff)
    ok = mask & ~nan
    terms, ratio = depth_metric_terms(t[ok], p[ok])
    out = [torch.tensor(float(ok.sum()), dtype=F64), torch.tensor(float(mask.sum()), dtype=F64)] + [x.sum() for x in terms]
    out += [(ratio <= 1.25 ** k).sum().to(F64) for k in (1, 2, 3)]
    return torch.stack(out)


# ------------------------------------------------------------------------------------------------ multi-scale gradient loss
_SOBEL_X = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype=F64) / 8.0


def msg_scales(H, W, num_scales):
    """[(k, h, w)] of AvgPool2d(k, k) for k = 1, 2, 4, 8 (truncating); None when a scale would be empty"""
    out = [(1 << s, H >> s, W >> s) for s in range(num_scales)]
    return None if not 1 <= num_scales <= 4 or any(h < 1 or w < 1 for _, h, w in out) else out


def msg_workspace_elems(B, H, W, num_scales):
    sc = msg_scales(H, W, num_scales)
    return 0 if sc is None else sum(B * h * w for _, h, w in sc)


def _msg_pool(diff, k, h, w):
    """[B][H][W] -> [B][h][w]: fp32 sum of the k x k block in row order, times the fp32 1 / k^2 (a NaN in the block makes the cell NaN)"""
    B = diff.shape[0]
    blk = diff[:, :h * k, :w * k].reshape(B, h, k, w, k).permute(0, 1, 3, 2, 4).reshape(B, h, w, k * k)
    acc = torch.zeros(B, h, w, dtype=F64)
    for j in range(k * k):
        acc = f32(acc + blk[..., j])
    return f32(acc * (1.0 / (k * k)))


def _msg_conv(P, kernels):
    """replicate-padded 3 x 3 cross-correlations of [B][h][w] -> [B][len(kernels)][h][w]"""
    xp = F.pad(P[:, None], (1, 1, 1, 1), mode="replicate")
    return F.conv2d(xp, torch.stack(kernels)[:, None])


def msg_forward(pred, target, num_scales):
    """MultiScaleGradient (model/loss.py:22-70, kornia's Sobel / 8 with replicate padding): per scale (sum |g|, count) over the non-NaN
    components of the gradient of the pooled pred - target (a NaN anywhere in the 3 x 3 window makes both components NaN), the loss
    mean_s(sum_s / count_s B 2), and the pooled maps (the workspace, one scale behind the other)"""
    B, H, W = pred.shape
    diff = f32(pred - target)
    stats, ws = [], []
    for k, h, w in msg_scales(H, W, num_scales):
        P = _msg_pool(diff, k, h, w)
        g = _msg_conv(P, [_SOBEL_X, _SOBEL_X.t()])
        ok = ~torch.isnan(g)
        stats += [g[ok].abs().sum(), torch.tensor(float(ok.sum()), dtype=F64)]
        ws.append(P.reshape(-1))
    stats = torch.stack(stats)
    loss = (stats[0::2] / stats[1::2] * B * 2.0).sum() / num_scales
    return stats, loss, torch.cat(ws)


def msg_backward(ws, stats, B, H, W, num_scales, gscale=1.0):
    """gscale d loss / d pred [B][H][W] from the pooled maps and GIVEN per-scale counts: the adjoint of pool and Sobel applied to
    sign(g) B 2 / count_s / num_scales (0 where g is NaN or 0).  Also returns the same adjoint on absolute values (the sum of |term|
    of every pixel's gradient) and the largest number of terms that meet in one cell of a scale."""
    grad, agrad, nterm = torch.zeros(B, H, W, dtype=F64), torch.zeros(B, H, W, dtype=F64), 0
    off = 0
    ring = torch.ones(3, 3, dtype=F64)
    ring[1, 1] = 0.0
    for s, (k, h, w) in enumerate(msg_scales(H, W, num_scales)):
        P = ws[off:off + B * h * w].reshape(B, h, w)
        off += B * h * w
        if float(stats[2 * s + 1]) == 0.0:          # no valid component at this scale: its (NaN) loss term has no gradient
            continue
        nan = torch.isnan(P)
        P0 = torch.where(nan, torch.zeros_like(P), P).requires_grad_(True)
        ok = ~torch.isnan(_msg_conv(P, [_SOBEL_X, _SOBEL_X.t()]))
        coef = gscale * B * 2.0 / stats[2 * s + 1] / num_scales
        g = _msg_conv(P0, [_SOBEL_X, _SOBEL_X.t()])
        dP, = torch.autograd.grad((g.abs() * ok).sum() * coef, P0)
        sgn = (g.detach() != 0) & ok
        ga = _msg_conv(P0, [_SOBEL_X.abs(), _SOBEL_X.t().abs()])
        aP, = torch.autograd.grad((ga * sgn).sum() * abs(float(coef)), P0)
        gn = _msg_conv(P0, [ring])
        nP, = torch.autograd.grad((gn * (sgn[:, :1] | sgn[:, 1:])).sum(), P0)
        nterm = max(nterm, int(nP.max()))
        up = lambda t: (t / (k * k)).repeat_interleave(k, 1).repeat_interleave(k, 2)
        grad[:, :h * k, :w * k] += up(dP)
        agrad[:, :h * k, :w * k] += up(aP)
    return grad, agrad, nterm


# ------------------------------------------------------------------------------------------------ nonzero statistics / normalisation
def nonzero_stats(grid):
    """(sum, sum of squares, count of non-zero entries) of one grid"""
    g = grid.reshape(-1)
    return torch.stack([g.sum(), (g * g).sum(), torch.tensor(float((g != 0).sum()), dtype=F64)])


def normalize_nonzero(grid):
    """event_tensor_utils.py:52-66 / event_dataset.py:150: (v - mean) / stddev over the non-zero entries, zeros stay zero; a grid without
    non-zero entries or with a single distinct non-zero value (stddev 0) is left unchanged"""
    S1, S2, cnt = nonzero_stats(grid)
    if cnt == 0:
        return grid.clone()
    mean = S1 / cnt
    var = S2 / cnt - mean * mean
    nz = grid[grid != 0]
    if bool((nz == nz[0]).all()):
        return grid.clone()
    return torch.where(grid != 0, (grid - mean) / torch.sqrt(var), torch.zeros_like(grid))


# ------------------------------------------------------------------------------------------------ BatchNorm / InstanceNorm
def norm_act_grad(dy, y, act):
    """dy act'(y): 0 none, 1 ReLU (y > 0), 2 sigmoid (y (1 - y)), y = the activated output"""
    if y is None or act == 0:
        return dy
    return torch.where(y > 0, dy, torch.zeros_like(dy)) if act == 1 else dy * y * (1.0 - y)


def norm_partial(a, b, y=None, act=0):
    """[groups][npix][C] -> [groups][C][2]: (sum a', sum a' b) over the pixels of a group, a' = a or a act'(y) (the sum over the slabs)"""
    ap = a if y is None else norm_act_grad(a, y, act)
    return torch.stack([ap.sum(1), (ap * b).sum(1)], -1)


def norm_finalize(sums, npix, eps, gamma=None, beta=None, rmean=None, rvar=None, momentum=0.1, update=False, use_running=False):
    """sums [groups][C][2] = (sum x, sum x^2) -> mean, rstd [groups][C], scale = gamma rstd, shift = beta - mean scale, and torch's
    running-buffer update: running = (1 - m) running + m mean over the groups of (mean, UNBIASED variance).  use_running: mean /
    variance are the running buffers (eval mode, groups = 1)."""
    if use_running:
        mean, var = rmean[None].clone(), rvar[None].clone()
    else:
        mean = sums[..., 0] / npix
        var = (sums[..., 1] / npix - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    ga = torch.ones_like(mean[0]) if gamma is None else gamma
    be = torch.zeros_like(mean[0]) if beta is None else beta
    scale = ga[None] * rstd
    shift = be[None] - mean * scale
    new_rm, new_rv = rmean, rvar
    if update and not use_running and rmean is not None:
        new_rm = (1.0 - momentum) * rmean + momentum * mean.mean(0)
        new_rv = (1.0 - momentum) * rvar + momentum * (var * (npix / (npix - 1.0))).mean(0)
    return mean, rstd, scale, shift, new_rm, new_rv


def norm_apply(x, scale, shift, res=None, act=0):
    """[groups][npix][C]: act(x scale[g][c] + shift[g][c] [+ res])"""
    z = x * scale[:, None] + shift[:, None] + (0.0 if res is None else res)
    return z if act == 0 else z.clamp_min(0.0) if act == 1 else torch.sigmoid(z)


def norm_finalize_bwd(sums, npix, mean, rstd, gamma=None, batch_stats=True):
    """sums [groups][C][2] = (S1 = sum g, sum g x) -> c1 = gamma rstd, c2 = -gamma rstd^2 S2 / N, c3 = -gamma rstd S1 / N - c2 mean with
    S2 = sum g xhat = rstd (sum g x - mean S1) (c2 = c3 = 0 without batch statistics); dgamma = sum_groups S2, dbeta = sum_groups S1"""
    S1, Sx = sums[..., 0], sums[..., 1]
    S2 = rstd * (Sx - mean * S1)
    ga = (torch.ones_like(mean[0]) if gamma is None else gamma)[None]
    c1 = ga * rstd
    c2 = -ga * rstd * rstd * S2 / npix if batch_stats else torch.zeros_like(c1)
    c3 = -ga * rstd * S1 / npix - c2 * mean if batch_stats else torch.zeros_like(c1)
    return c1, c2, c3, S2.sum(0), S1.sum(0)


def norm_bwd(dy, x, c1, c2, c3, y=None, act=0):
    """dx = c1 dy' + c2 x + c3, dres = dy' = dy act'(y)"""
    g = norm_act_grad(dy, y, act)
    return c1[:, None] * g + c2[:, None] * x + c3[:, None], g


# ------------------------------------------------------------------------------------------------ small GEMMs
def gemm(A, B, C0=None, trans_a=False):
    """batched C (=, += onto C0) A B or A^T B: A [batch][M][K] ([batch][K][M] when trans_a), B [batch][K][N]"""
    P = torch.matmul(A.transpose(1, 2) if trans_a else A, B)
    return P if C0 is None else C0 + P
