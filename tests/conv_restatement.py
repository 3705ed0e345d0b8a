"""A float64 interpreter of ramnet_conv_desc and ramnet_wgrad_desc, written from include/ramnet_hip.h (not from the kernels), with the
companions the comparison rules of profiles/conv_launch_tests_notes.md need: the same expression on absolute values, the number of terms
that meet in an element and, for the Winograd families, the absolute-value statement in the transformed domain.  No GPU.

A descriptor is a `types.SimpleNamespace` of float64 tensors and numbers (tests/conv_launch_cases.py builds them):
  x0, x1, xm     NHWC sources ([B][2*Hin][2*Win][C0] for IN_S2D), in_mode, Hin, Win
  W              the weight slices W[s][c][n] ([slices][Cin][N], N = Cout or 4 * Cout gate columns for the ConvLSTM cell)
  taps           [(dy, dx, wtap)], stride, Ho, Wo, HoF, WoF, os = (osy, osx, ooy, oox)
  bias, epi, beta, e0, e1, out_old (what `out` holds before the launch), active, out_s2d, Cout
"""
import types

import torch

IN_PLAIN, IN_CAT, IN_CAT_MUL, IN_RELUMASK, IN_S2D = 0, 1, 2, 5, 6
EPI_LINEAR, EPI_RELU, EPI_SIGMOID, EPI_RES_RELU, EPI_GRU_BLEND, EPI_LSTM, EPI_GRU_BWD, EPI_SIGMOID_HR = range(8)
F64 = torch.float64
U = 2.0 ** -24
# maximum absolute errors of sigmoidf_ / tanhf_ and their argument ranges: the constants of tests/guarded.py (that module needs the
# library's binding, this one must not)
SIGMOID_ERR, TANH_ERR, SIG_RANGE, TANH_RANGE = 1.07e-7, 2.18e-7, 16.0, 8.0

# Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks": F(2,3) and F(4,3)
BT2 = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=F64)
G2 = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=F64)
AT2 = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=F64)
BT4 = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                    [0, 4, 0, -5, 0, 1]], dtype=F64)
G4 = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
                  dtype=F64)
AT4 = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=F64)
WINO = {"2x2": (BT2, G2, AT2, BT2, G2, AT2), "2x4": (BT2, G2, AT2, BT4, G4, AT4)}        # (rows: B^T, G, A^T; columns: B^T, G, A^T)
# Roundings r of the transforms per family, counted from the matrices (profiles/conv_launch_tests_notes.md section 2)
R_TRANSFORMS = {"direct": 0, "2x2": 7, "2x4": 12}


def sigmoid(v):
    return 1.0 / (1.0 + torch.exp(-v))


def logical_input(d, absolute=False):
    """[B][Hin][Win][Cin] of the launch: what ramnet_in_mode says feeds the reduction"""
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    if d.in_mode == IN_PLAIN:
        return f(d.x0)
    if d.in_mode == IN_CAT:
        return torch.cat([f(d.x0), f(d.x1)], 3)
    if d.in_mode == IN_CAT_MUL:
        return torch.cat([f(d.x0), f(d.x1) * f(d.xm)], 3)
    if d.in_mode == IN_RELUMASK:
        return f(d.x0) * (d.xm > 0).to(F64)
    if d.in_mode == IN_S2D:        # channel (a*2 + c)*C0 + ch of pixel (i, j) = x0(2i + a, 2j + c, ch)
        B, H2, W2, C0 = d.x0.shape
        return f(d.x0).view(B, H2 // 2, 2, W2 // 2, 2, C0).permute(0, 1, 3, 2, 4, 5).reshape(B, H2 // 2, W2 // 2, 4 * C0)
    raise ValueError(d.in_mode)


def _gather(x, n, stride, off):
    """x along one axis at i*stride + off for i < n, zero outside: (index, inside)"""
    i = torch.arange(n) * stride + off
    return i.clamp(0, x - 1), ((i >= 0) & (i < x))


def reduction(xin, W, taps, stride, Ho, Wo):
    """acc[b][a][c][n] = sum_t sum_k in(a*stride + dy[t], c*stride + dx[t], k) W[wtap[t]][k][n], and the in-image terms per element"""
    B, Hin, Win, Cin = xin.shape
    acc = torch.zeros(B, Ho, Wo, W.shape[2], dtype=F64)
    terms = torch.zeros(Ho, Wo, dtype=F64)
    for dy, dx, wt in taps:
        iy, oky = _gather(Hin, Ho, stride, dy)
        ix, okx = _gather(Win, Wo, stride, dx)
        ok = (oky[:, None] & okx[None, :]).to(F64)
        acc += (xin[:, iy][:, :, ix] * ok[None, :, :, None]) @ W[wt]
        terms += ok * Cin
    return acc, terms


def wino_abs(xin_abs, W_abs_slices, taps, Ho, Wo, family, absolute=True):
    """|A^T| (sum_c |U| .* |V|) |A| with |U| = |G| |g| |G^T| and |V| = |B^T| |d| |B| on the tiles of the map (zero outside the image):
    the absolute-value statement in the transformed domain of F(2x2,3x3) / F(2x4,3x3); taps = the dense 3x3 window (any order).
    absolute=False: the matrices with their signs, i.e. the Winograd evaluation itself (the CPU anchor checks the matrices with it)"""
    BTr, Gr, ATr, BTc, Gc, ATc = [m.abs() if absolute else m for m in WINO[family]]
    th, tw = ATr.shape[0], ATc.shape[0]
    dy0, dx0 = min(t[0] for t in taps), min(t[1] for t in taps)
    g = torch.zeros(3, 3, *W_abs_slices.shape[1:], dtype=F64)
    for dy, dx, wt in taps:
        g[dy - dy0, dx - dx0] = W_abs_slices[wt]
    Uabs = torch.einsum("ia,abkn,jb->ijkn", Gr, g, Gc)
    B, Hin, Win, Cin = xin_abs.shape
    ty, tx = -(-Ho // th), -(-Wo // tw)
    pad = torch.zeros(B, ty * th + 2, tx * tw + 2, Cin, dtype=F64)                # padded row p = input row p + dy0
    y0, x0, sy, sx = max(0, -dy0), max(0, -dx0), max(0, dy0), max(0, dx0)
    hh, ww = min(Hin - sy, pad.shape[1] - y0), min(Win - sx, pad.shape[2] - x0)
    pad[:, y0:y0 + hh, x0:x0 + ww] = xin_abs[:, sy:sy + hh, sx:sx + ww]
    tiles = pad.unfold(1, th + 2, th).unfold(2, tw + 2, tw)                     # [B][ty][tx][Cin][th+2][tw+2]
    V = torch.einsum("ia,zyxkab,jb->zyxijk", BTr, tiles, BTc)
    M = torch.einsum("zyxijk,ijkn->zyxijn", V, Uabs)
    Y = torch.einsum("pi,zyxijn,qj->zypxqn", ATr, M, ATc).reshape(B, ty * th, tx * tw, -1)
    return Y[:, :Ho, :Wo]


def conv_statement(d, family="direct"):
    """Everything a launch of descriptor d leaves behind, in float64.  Returns a namespace with
       out, o1, o2      full tensors ([B][HoF][WoF][...]; None where the launch has no such output)
       w_out, w_o1, w_o2  boolean masks of the elements the launch writes
       b_out, b_o1, b_o2  the derived / measured error bound of every written element (0 where the rule is bit)
       pre, pre_abs, n  pre-activation [B][Ho][Wo][N], its absolute-value statement (transformed domain for a Winograd family), terms
       kink             written elements of `out` left out of the value comparison (within their bound of a kink)
       sig_arg, tanh_arg  largest |argument| an activation sees (0 if none)"""
    r = types.SimpleNamespace(o1=None, o2=None, w_o1=None, w_o2=None, b_o1=None, b_o2=None, sig_arg=0.0, tanh_arg=0.0)
    xin, xabs = logical_input(d), logical_input(d, True)
    acc, terms = reduction(xin, d.W, d.taps, d.stride, d.Ho, d.Wo)
    spatial_abs, _ = reduction(xabs, d.W.abs(), d.taps, d.stride, d.Ho, d.Wo)
    if family == "direct":
        aabs, n = spatial_abs, terms[None, :, :, None]
    else:
        aabs, n = wino_abs(xabs, d.W.abs(), d.taps, d.Ho, d.Wo, family[:3]), float(xin.shape[3])
    B, Ho, Wo, N = acc.shape
    osy, osx, ooy, oox = d.os
    ys, xs = torch.arange(Ho) * osy + ooy, torch.arange(Wo) * osx + oox

    def sub(t):          # the (a, b) sub-grid of a full-resolution tensor
        return t[:, ys][:, :, xs]

    pre, pabs = acc.clone(), aabs.clone()
    extra = torch.zeros_like(acc)                   # one 2^-24 per further fp32 result, on its magnitude
    if d.bias is not None:
        pre, pabs = pre + d.bias, pabs + d.bias.abs()
        extra = extra + pre.abs()
    if d.beta != 0.0 and d.epi in (EPI_LINEAR, EPI_RELU):
        old = sub(d.out_old)
        pre, pabs = pre + d.beta * old, pabs + abs(d.beta) * old.abs()
        extra = extra + pre.abs() + (abs(d.beta) * old.abs() if d.beta != 1.0 else 0.0)
    split = 3.0 if family.endswith("split") else 0.0
    bpre = (n + R_TRANSFORMS[family[:3] if family != "direct" else "direct"] + 2 + split) * U * pabs + U * extra
    r.pre, r.pre_abs, r.n, r.b_pre = pre, pabs, n, bpre
    Cout, epi = d.Cout, d.epi
    act = torch.ones(B, dtype=torch.bool) if d.active is None else d.active != 0
    am = act[:, None, None, None]
    kink = None
    if epi == EPI_LINEAR:
        val, bnd = pre, bpre
    elif epi in (EPI_RELU, EPI_RES_RELU):
        z, bz = pre, bpre
        if epi == EPI_RES_RELU:
            z = pre + sub(d.e0)
            bz = bpre + U * z.abs()
        val, bnd = z.clamp_min(0), bz
        kink = z.abs() <= bz
    elif epi in (EPI_SIGMOID, EPI_SIGMOID_HR):
        r.sig_arg = float(pre.abs().max())
        val = sigmoid(pre)
        bnd = bpre / 4 + 4 * SIGMOID_ERR
        if epi == EPI_SIGMOID_HR:
            C = Cout // 2
            h = sub(d.e1)
            hr = h * val[..., C:]
            r.o1 = torch.where(am, hr, torch.zeros_like(hr))
            r.b_o1 = torch.where(am, h.abs() * bnd[..., C:] + U * hr.abs(), torch.zeros_like(hr))
        val, bnd = torch.where(am, val, torch.zeros_like(val)), torch.where(am, bnd, torch.zeros_like(bnd))
    elif epi == EPI_GRU_BLEND:
        r.tanh_arg = float(pre.abs().max())
        o, bo = torch.tanh(pre), bpre + 4 * TANH_ERR
        u = sub(d.e0)
        h = sub(d.e1) if d.e1 is not None else torch.zeros_like(o)
        val = h * (1 - u) + o * u
        bnd = u.abs() * bo + 3 * U * (h.abs() * (1 - u).abs() + (o * u).abs())
        r.o1, r.b_o1 = torch.where(am, o, torch.zeros_like(o)), torch.where(am, bo, torch.zeros_like(o))
        val, bnd = torch.where(am, val, h), torch.where(am, bnd, torch.zeros_like(bnd))
    elif epi == EPI_LSTM:
        C = Cout
        gi, gf, go, gg = pre[..., :C], pre[..., C:2 * C], pre[..., 2 * C:3 * C], pre[..., 3 * C:]
        r.sig_arg, r.tanh_arg = float(pre[..., :3 * C].abs().max()), float(gg.abs().max())
        i, f, o, g = sigmoid(gi), sigmoid(gf), sigmoid(go), torch.tanh(gg)
        bs, bg = bpre[..., :3 * C] / 4 + 4 * SIGMOID_ERR, bpre[..., 3 * C:] + 4 * TANH_ERR
        bi, bf, bo = bs[..., :C], bs[..., C:2 * C], bs[..., 2 * C:]
        c = sub(d.e1) if d.e1 is not None else torch.zeros_like(i)
        cn = f * c + i * g
        bcn = bf * c.abs() + bi * g.abs() + bg * i.abs() + 3 * U * ((f * c).abs() + (i * g).abs())
        r.tanh_arg = max(r.tanh_arg, float(cn.abs().max()))
        val = o * torch.tanh(cn)
        bnd = bo * torch.tanh(cn).abs() + o.abs() * (bcn + 4 * TANH_ERR) + 2 * U * val.abs()
        gates, bgates = torch.cat([i, f, o, g], 3), torch.cat([bs, bg], 3)
        z = torch.zeros_like(val)
        r.o1, r.b_o1 = torch.where(am, cn, c), torch.where(am, bcn, z)
        r.o2, r.b_o2 = torch.where(am, gates, torch.zeros_like(gates)), torch.where(am, bgates, torch.zeros_like(gates))
        if d.active is not None:
            val, bnd = torch.where(am, val, sub(d.e0)), torch.where(am, bnd, z)
    elif epi == EPI_GRU_BWD:
        C = Cout // 2
        g = pre[..., C:]
        rr = sub(d.e0)[..., C:2 * C]
        h = sub(d.e1) if d.e1 is not None else torch.zeros_like(g)
        old = sub(d.out_old)[..., C:]
        dpr = g * h * rr * (1 - rr)
        dh = old + g * rr
        r.o1 = torch.cat([torch.zeros_like(dpr), dpr], 3)
        r.b_o1 = torch.cat([torch.zeros_like(dpr), (h * rr * (1 - rr)).abs() * bpre[..., C:] + 4 * U * dpr.abs()], 3)
        val = torch.cat([pre[..., :C], dh], 3)
        bnd = torch.cat([bpre[..., :C], rr.abs() * bpre[..., C:] + U * (g * rr).abs() + U * dh.abs()], 3)
    else:
        raise ValueError(epi)
    kink = torch.zeros_like(val, dtype=torch.bool) if kink is None else kink

    def scatter(v, nch, fill):
        full = torch.full((B, d.HoF, d.WoF, nch), fill, dtype=v.dtype)
        full[:, ys[:, None], xs[None, :]] = v
        return full

    if d.out_s2d:                                    # channel (a*2 + c)*C + ch of pixel (i, j) -> out(2i + a, 2j + c, ch)
        C = d.out_s2d

        def deep(v):
            return v.view(B, Ho, Wo, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Ho, 2 * Wo, C)
        r.out, r.b_out, r.kink = deep(val), deep(bnd), deep(kink)
        r.w_out = torch.ones_like(r.out, dtype=torch.bool)
    else:
        r.out, r.b_out, r.kink = scatter(val, val.shape[3], 0.0), scatter(bnd, val.shape[3], 0.0), scatter(kink, val.shape[3], False)
        r.w_out = scatter(torch.ones_like(val, dtype=torch.bool), val.shape[3], False)
    if epi == EPI_GRU_BWD:                           # o1 is written for the channels n >= C only
        half = torch.cat([torch.zeros_like(dpr, dtype=torch.bool), torch.ones_like(dpr, dtype=torch.bool)], 3)
        r.w_o1 = scatter(half, 2 * C, False)
        r.o1, r.b_o1 = scatter(r.o1, 2 * C, 0.0), scatter(r.b_o1, 2 * C, 0.0)
    elif r.o1 is not None:
        r.w_o1 = scatter(torch.ones_like(r.o1, dtype=torch.bool), r.o1.shape[3], False)
        r.o1, r.b_o1 = scatter(r.o1, r.o1.shape[3], 0.0), scatter(r.b_o1, r.b_o1.shape[3], 0.0)
    if r.o2 is not None:
        r.w_o2 = scatter(torch.ones_like(r.o2, dtype=torch.bool), r.o2.shape[3], False)
        r.o2, r.b_o2 = scatter(r.o2, r.o2.shape[3], 0.0), scatter(r.b_o2, r.b_o2.shape[3], 0.0)
    return r


def exact_ok(st, family):
    """the conditions of the exact rule, on the float64 side: the statement and its absolute-value companion (transformed domain for a
    Winograd family: every intermediate of the transforms is bounded by it) are multiples of 1/16 below 2^24 / 16"""
    vals = [st.pre, st.out] + [t for t in (st.o1, st.o2) if t is not None]
    ints = all(torch.equal(v * 16, (v * 16).round()) for v in vals)
    return ints and float(st.pre_abs.max()) * 16 < 2 ** 24 and all(float(v.abs().max()) * 16 < 2 ** 24 for v in vals)


# ------------------------------------------------------------------------------------------------ backward-weights
def wgrad_statement(d):
    """dW[t][c][n] = sum_{b, a, b'} in(a*stride + dy[t], b'*stride + dx[t], c) g(a, b', n), g = dout (* (gmask > 0)); dbias[n] = sum g; with
    their absolute-value companions and term counts.  d: x0 / x1 / xm / in_mode as above, taps [(dy, dx)], stride, dout, gmask, Ho, Wo;
    several segments (d.segs: a list of such namespaces) add up."""
    segs = getattr(d, "segs", None) or [d]
    out = None
    for s in segs:
        xin, xabs = logical_input(s), logical_input(s, True)
        g = s.dout if s.gmask is None else s.dout * (s.gmask > 0).to(F64)
        B, Hin, Win, Cin = xin.shape
        dW, dWa, cnt = [], [], []
        for dy, dx in d.taps:
            iy, oky = _gather(Hin, d.Ho, d.stride, dy)
            ix, okx = _gather(Win, d.Wo, d.stride, dx)
            ok = (oky[:, None] & okx[None, :]).to(F64)[None, :, :, None]
            dW.append(torch.einsum("bhwc,bhwn->cn", xin[:, iy][:, :, ix] * ok, g))
            dWa.append(torch.einsum("bhwc,bhwn->cn", xabs[:, iy][:, :, ix] * ok, g.abs()))
            cnt.append(float(ok.sum()) * B)
        cur = [torch.stack(dW), torch.stack(dWa), torch.tensor(cnt, dtype=F64), g.sum((0, 1, 2)), g.abs().sum((0, 1, 2)), float(B * d.Ho * d.Wo)]
        out = cur if out is None else [a + b for a, b in zip(out, cur)]
    return types.SimpleNamespace(dW=out[0], dW_abs=out[1], n=out[2], dbias=out[3], dbias_abs=out[4], n_bias=out[5])


# Roundings of the backward-weights transforms besides the n terms of the reduction, counted from the matrices: F(2x2,3x3): input transform
# 2, transform of dout (A g A^T, two non-zeros per column) 2, the fp32 fold G^T dU G over 16 positions 16, the += 1; F(2x4,3x3): input
# transform 5, dout transform (rows 1, columns of up to four non-zeros 3) 4, the fold (in double) and its rounding 1, the += 1; direct: the
# += of the unpack; split operands: + 3 as for the forward family
R_WGRAD = {"direct": 1, "dsplit": 4, "2x2": 21, "2x4": 11}


def wgrad_wino(d, family, absolute=True):
    """the backward-weights statement in the transformed domain: |G_r^T| (sum over tiles and images |B^T d B| (x) |A g A^T|) |G_c| as
    [9][Cin][Cout] (forward tap order), and the number of tiles that meet in an element; absolute=False: the matrices with their signs,
    which must give dW itself (CPU anchor).  Dense 3x3 stride-1 taps, Ho = Hin, Wo = Win."""
    BTr, Gr, ATr, BTc, Gc, ATc = [m.abs() if absolute else m for m in WINO[family]]
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    th, tw = ATr.shape[0], ATc.shape[0]
    dU, tiles_n = None, 0
    for s in getattr(d, "segs", None) or [d]:
        x = logical_input(s, absolute)
        g = f(s.dout) if s.gmask is None else f(s.dout) * (s.gmask > 0).to(F64)
        B, H, W, Cin = x.shape
        ty, tx = -(-H // th), -(-W // tw)
        px = torch.zeros(B, ty * th + 2, tx * tw + 2, Cin, dtype=F64)
        px[:, 1:H + 1, 1:W + 1] = x
        pg = torch.zeros(B, ty * th, tx * tw, g.shape[3], dtype=F64)
        pg[:, :H, :W] = g
        V = torch.einsum("ia,zyxkab,jb->zyxijk", BTr, px.unfold(1, th + 2, th).unfold(2, tw + 2, tw), BTc)
        Y = torch.einsum("pi,zyxnpq,qj->zyxijn", ATr, pg.unfold(1, th, th).unfold(2, tw, tw), ATc)
        cur = torch.einsum("zyxijk,zyxijn->ijkn", V, Y)
        dU = cur if dU is None else dU + cur
        tiles_n += B * ty * tx
    grad = torch.einsum("ia,ijkn,jb->abkn", Gr, dU, Gc)
    return grad.reshape(9, grad.shape[2], grad.shape[3]), tiles_n


def wgrad_bound(d, st, family):
    """(derived bound of the unpacked gradient [9][Cin][Cout], of dbias [Cout]) on normal data"""
    if family in ("direct", "dsplit"):
        a, n = st.dW_abs, st.n[:, None, None]
    else:
        a, n = wgrad_wino(d, family)
    return (n + R_WGRAD[family] + 2) * U * a, (st.n_bias + 2) * U * st.dbias_abs


def unpack_statement(grad_old, dW, Cout, Cin, n_off):
    """ramnet_unpack_wgrad: grad_oihw[n][c][tap] += ws[tap][c][n_off + n] for c < Cin, n < Cout ([T][CinWs][CoutWs] workspace)"""
    T = dW.shape[0]
    return grad_old + dW[:, :Cin, n_off:n_off + Cout].permute(2, 1, 0).reshape(Cout, Cin, T).reshape(grad_old.shape)
