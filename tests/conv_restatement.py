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

IN_PLAIN, IN_CAT, IN_CAT_MUL, IN_UP2X, IN_UP2X_SKIP, IN_RELUMASK, IN_S2D, IN_PARITY4 = range(8)
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
    if d.in_mode == IN_UP2X:       # x0 = [B][Hin / 2][Win / 2][C0]; Hin, Win = the extent after the x2
        return up2x(f(d.x0))
    if d.in_mode == IN_UP2X_SKIP:
        return up2x(f(d.x0) + f(d.x1))
    if d.in_mode in (IN_S2D, IN_PARITY4):      # channel (a*2 + c)*C0 + ch of pixel (i, j) = x0(2i + a, 2j + c, ch); PARITY4: the four parity
        B, H2, W2, C0 = d.x0.shape             # sub-grids of the full-resolution gradient as reduction blocks, class (a, c) major
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
    if getattr(d, "frame", 0):                       # border corrections of the folded upsample-conv, on the FULL output
        add, aabs, both = frame_terms(d, N)
        pre, pabs = pre + sub(add), pabs + sub(aabs)
        extra = extra + sub(both) + pre.abs() * (sub(aabs) != 0).to(F64)
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


# ================================================================================================ head, folded decoders, UP2X loaders
# (profiles/fold_head_launch_tests_notes.md; written from include/ramnet_hip.h like everything above)
# Toom-Cook F(2,4) on the points 0, 1, -1, 2, inf and F(3,4) on 0, 1, -1, 1/2, -1/2, inf; G = G6 / 6 and Gc = GC3 / 3 as in ramnet_hip.h
BT24 = torch.tensor([[2, -1, -2, 1, 0], [0, -2, -1, 1, 0], [0, 2, -3, 1, 0], [0, -1, 0, 1, 0], [0, 2, -1, -2, 1]], dtype=F64)
AT24 = torch.tensor([[1, 1, 1, 1, 0], [0, 1, -1, 2, 1]], dtype=F64)
G6 = torch.tensor([[3, 0, 0, 0], [-3, -3, -3, -3], [-1, 1, -1, 1], [1, 2, 4, 8], [0, 0, 0, 6]], dtype=F64)
BT34 = torch.tensor([[1 / 4, 0, -5 / 4, 0, 1, 0], [0, -1 / 4, -1 / 4, 1, 1, 0], [0, 1 / 4, -1 / 4, -1, 1, 0], [0, -1 / 2, -1, 1 / 2, 1, 0],
                     [0, 1 / 2, -1, -1 / 2, 1, 0], [0, 1 / 4, 0, -5 / 4, 0, 1]], dtype=F64)
AT34 = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 1 / 2, -1 / 2, 0], [0, 1, 1, 1 / 4, 1 / 4, 1]], dtype=F64)
GC3 = torch.tensor([[12, 0, 0, 0], [2, 2, 2, 2], [2, -2, 2, -2], [-8, -4, -2, -1], [-8, 4, -2, 1], [0, 0, 0, 3]], dtype=F64)
WINO["fold2x2"] = (BT24, G6 / 6, AT24, BT24, G6 / 6, AT24)
WINO["fold2x3"] = (BT24, G6 / 6, AT24, BT34, GC3 / 3, AT34)
# Roundings of the folded families, counted from the matrices (notes section 2): input transform 3 per pass (rows of B^T with four
# non-zeros, or three and a factor 3 or 5/4), the pack 1, the output transform 3 per F(2,4) pass (four non-zeros per row of A^T) and 4 for
# F(3,4) (five)
R_TRANSFORMS.update({"fold2x2": 3 + 3 + 1 + 3 + 3, "fold2x3": 3 + 3 + 1 + 3 + 4})
# the dyadic grid 2^-k of the exact rule (weights 9 x integer): U = (6G)(4FA) w (4FA)^T (6G)^T / 576 lies on 2^-6, on 2^-5 with 3Gc (/ 288);
# B^T d B is integral for F(2,4) and on 2^-2 with the quarters of F(3,4); A^T of F(3,4) adds another 2^-2
GRID_BITS = {"fold2x2": 6, "fold2x3": 9}
FOLD_TW = {"fold2x2": 2, "fold2x3": 3}


def up2x(x):
    """bilinear x2, align_corners=False, of [B][h][w][C]: fine sample 2i is 1/4 x(i-1) + 3/4 x(i), 2i+1 is 3/4 x(i) + 1/4 x(i+1), clamped"""
    def axis(t, dim):
        n = t.shape[dim]
        i = torch.arange(n)
        lo, hi = t.index_select(dim, (i - 1).clamp_min(0)), t.index_select(dim, (i + 1).clamp_max(n - 1))
        return torch.stack([0.25 * lo + 0.75 * t, 0.75 * t + 0.25 * hi], dim + 1).flatten(dim, dim + 1)
    return axis(axis(x, 1), 2)


def fold_matrix():
    """FA[p][t][k]: weight of padded low-res row a + p + t (low-res row a + p + t - 2) in fine row 2a + p + k - 2 of the x2 upsample,
    i.e. in tap k of output parity p (t < 4, k < 5); from the bilinear rule above"""
    FA = torch.zeros(2, 4, 5, dtype=F64)
    for p in range(2):
        for k in range(5):
            i, par = divmod(p + k - 2, 2)
            for off, wgt in (((-1, 0.25), (0, 0.75)) if par == 0 else ((0, 0.75), (1, 0.25))):
                FA[p, i + off + 2 - p, k] += wgt
    return FA


def fold_w4(w5, scaled=False):
    """W4[n][c][py][px][t][s] = sum_{k,l} FA[py][t][k] FA[px][s][l] w5[n][c][k][l]; scaled: 16 W4, through the integers 4 FA"""
    FA4 = 4 * fold_matrix()
    w16 = torch.einsum("ptk,qsl,nckl->ncpqts", FA4, FA4, w5)
    return w16 if scaled else w16 / 16


def fold_taps(py, px):
    """the 16 taps of parity class (py, px) on the replicate-padded input, slice t*4 + s"""
    return [(py + t, px + s, t * 4 + s) for t in range(4) for s in range(4)]


def fold_wino(xpad, W4c, py, px, H, W, family, shift=0, absolute=True):
    """The transformed-domain statement of one parity class on the library's tiling: tiles of 2 x TW outputs with origins (2i, TW j - shift)
    (shift = 1: column parity 1 of the pair form), windows of 5 x (TW + 3) padded pixels from (2i + py, TW j - shift + px), rows and columns
    past the padded input clamped; |A^T| (sum_c |U| .* |V|) |A| with |U| = |G| |W4| |Gc^T|, |V| = |B^T| |d| |Bc|.  W4c = [16][C][N] (slice
    t*4 + s).  absolute=False: the matrices with their signs = the class's tap sum (CPU anchor)."""
    BTr, Gr, ATr, BTc, Gc, ATc = [m.abs() if absolute else m for m in WINO[family]]
    tw = ATc.shape[0]
    B, Hp, Wp, C = xpad.shape
    ny, nx = -(-H // 2), -(-(W + shift) // tw)
    ry = (2 * torch.arange(ny)[:, None] + py + torch.arange(5)[None, :]).clamp_max(Hp - 1)               # [ny][5]
    rx = (tw * torch.arange(nx)[:, None] - shift + px + torch.arange(tw + 3)[None, :]).clamp_max(Wp - 1)  # [nx][tw + 3]
    assert int(rx.min()) >= 0
    win = xpad[:, ry][:, :, :, rx]                                                  # [B][ny][5][nx][tw+3][C]
    V = torch.einsum("ar,zyrxck,bc->zyxabk", BTr, win, BTc)
    Uw = torch.einsum("at,tskn,bs->abkn", Gr, W4c.view(4, 4, C, -1), Gc)
    Y = torch.einsum("pa,zyxabn,qb->zypxqn", ATr, torch.einsum("zyxabk,abkn->zyxabn", V, Uw), ATc).reshape(B, 2 * ny, tw * nx, -1)
    return Y[:, :H, shift:shift + W]


def frame_terms(d, Cout):
    """ramnet_conv_desc.frame: what the outermost `frame` rows / columns of the FULL output add to the pre-activation: rows from
    e1 [2 sides][B][WoF][frame * Cout] (side 0 top, 1 bottom; slot = distance into the band from its upper edge), columns from
    e0 [2][B][HoF][frame * Cout]; corners get both.  Returns (sum, sum of absolute values, |e1 + e0| where both meet) as [B][HoF][WoF][Cout]"""
    fr, HoF, WoF = d.frame, d.HoF, d.WoF
    B = d.e1.shape[1]
    rows, cols = torch.zeros(B, HoF, WoF, Cout, dtype=F64), torch.zeros(B, HoF, WoF, Cout, dtype=F64)
    e1, e0 = d.e1.reshape(2, B, WoF, fr, Cout), d.e0.reshape(2, B, HoF, fr, Cout)
    for slot in range(fr):
        rows[:, slot], rows[:, HoF - fr + slot] = e1[0, :, :, slot], e1[1, :, :, slot]
        cols[:, :, slot], cols[:, :, WoF - fr + slot] = e0[0, :, :, slot], e0[1, :, :, slot]
    return rows + cols, rows.abs() + cols.abs(), (rows + cols).abs() * ((rows != 0) & (cols != 0)).to(F64)


def fold_statement(d, family, pair=False):
    """RAMNET_ALGO_WINOGRAD24 (family "fold2x2") / _2X3 ("fold2x3"), forward: Out(2a + py, 2b + px, n) = epi(sum_{t,s<4} sum_c
    xpad(a + py + t, b + px + s, c) W4[n][c][py][px][t][s] + bias + frame) with d.x0 = xpad [B][Ho + 4][Wo + 4][C0], d.w5 the OIHW 5x5
    weights, d.frame / e0 / e1 as in frame_terms.  pair: the tiling of the pair form (column parity 1 shifted by one column) for the
    transformed-domain companion.  Fields as conv_statement."""
    r = types.SimpleNamespace(o1=None, o2=None, w_o1=None, w_o2=None, b_o1=None, b_o2=None, sig_arg=0.0, tanh_arg=0.0)
    B, Hp, Wp, C0 = d.x0.shape
    H, W, N = d.Ho, d.Wo, d.Cout
    W4 = fold_w4(d.w5)
    pre, pabs = torch.zeros(B, 2 * H, 2 * W, N, dtype=F64), torch.zeros(B, 2 * H, 2 * W, N, dtype=F64)
    for py in range(2):
        for px in range(2):
            Wc = W4[:, :, py, px].permute(2, 3, 1, 0).reshape(16, C0, N)
            acc, _ = reduction(d.x0, Wc, fold_taps(py, px), 1, H, W)
            pre[:, py::2, px::2] = acc
            pabs[:, py::2, px::2] = fold_wino(d.x0.abs(), Wc.abs(), py, px, H, W, family, shift=int(pair and px == 1))
    extra = torch.zeros_like(pre)
    if d.bias is not None:
        pre, pabs = pre + d.bias, pabs + d.bias.abs()
        extra = extra + pre.abs()
    if d.frame:
        add, aabs, both = frame_terms(d, N)
        pre, pabs = pre + add, pabs + aabs
        extra = extra + both + pre.abs() * (aabs != 0).to(F64)
    bpre = (C0 + R_TRANSFORMS[family] + 2) * U * pabs + U * extra
    r.pre, r.pre_abs, r.n, r.b_pre = pre, pabs, float(C0), bpre
    if d.epi == EPI_RELU:
        r.out, r.kink = pre.clamp_min(0), pre.abs() <= bpre
    else:
        r.out, r.kink = pre, torch.zeros_like(pre, dtype=torch.bool)
    r.b_out, r.w_out = bpre, torch.ones_like(pre, dtype=torch.bool)
    return r


def fold_exact_ok(st, family):
    """the exact rule of a folded family: every value of the statement on the grid 2^-k of the family's transformed domain, and the
    transformed-domain absolute-value statement (which bounds every intermediate: each column of |A^T| holds an entry >= 1) below 2^24 on it"""
    k = 2.0 ** GRID_BITS[family]
    return torch.equal(st.pre * 16, (st.pre * 16).round()) and float(st.pre_abs.max()) * k < 2 ** 24


# ---------------------------------------------------------------------------------------------------- packs: the rounding of the rational
def fold_u(w5, tw, dgrad=False):
    """U[py][px][a][b][c][n] = sum G[a][t] W4[n][c][py][px][t][s] Gc[b][s] (dgrad: W4 flipped, [3 - t][3 - s]) through the integers 6 G,
    3 Gc (6 G for F(2x2)) and 4 FA, ONE division: exact in float64 for integer weights"""
    W16 = fold_w4(w5, scaled=True)
    if dgrad:
        W16 = W16.flip(4, 5)
    Gc, den = (G6, 16 * 36) if tw == 2 else (GC3, 16 * 18)
    return torch.einsum("at,ncpqts,bs->pqabcn", G6, W16, Gc) / den


def fold_u_abs(w5, tw, dgrad=False):
    W4 = fold_w4(w5.abs())
    return torch.einsum("at,ncpqts,bs->pqabcn", G6.abs() / 6, W4.flip(4, 5) if dgrad else W4, (G6.abs() / 6) if tw == 2 else GC3.abs() / 3)


def _scatter(U4, index, total):
    out = torch.zeros(total, dtype=F64)
    out[index.reshape(-1)] = U4.reshape(-1)
    return out


def pack_fold_statement(w5, tw, pair=False, absolute=False):
    """ramnet_pack_weight_fold_wino / ...2x3 in the layout of ramnet_hip.h (RAMNET_ALGO_WINOGRAD24): (KC, NCQ) = (16, 4) when Cout % 64 == 0
    and C0 % 16 == 0 or in the pair layout, else (8, 2); NP = 5 (tw + 3) positions"""
    Cout, C0 = w5.shape[:2]
    NP = 5 * (tw + 3)
    U4 = (fold_u_abs(w5, tw) if absolute else fold_u(w5, tw)).reshape(2, 2, NP, C0, Cout)
    py, px, pos, k, n = torch.meshgrid(torch.arange(2), torch.arange(2), torch.arange(NP), torch.arange(C0), torch.arange(Cout), indexing="ij")
    if pair:           # [py][C0 / 16][NP][4 column groups of 16][64 lanes][4], column = (px, channel)
        col = px * 32 + n
        idx = (((py * (C0 // 16) + k // 16) * NP + pos) * 4 + col // 16) * 256 + ((k % 16) // 4 * 16 + col % 16) * 4 + k % 4
    else:
        KC, NCQ = (16, 4) if (Cout % 64 == 0 and C0 % 16 == 0) else (8, 2)
        cls = py * 2 + px
        idx = ((((cls * (C0 // KC) + k // KC) * (Cout // (16 * NCQ)) + n // (16 * NCQ)) * NP + pos) * NCQ + (n % (16 * NCQ)) // 16) * 16 * KC \
            + (((k % KC) // (KC // 4)) * 16 + n % 16) * (KC // 4) + k % (KC // 4)
    return _scatter(U4, idx, 4 * NP * C0 * Cout)


def pack_fold_dgrad_statement(w5, tw, absolute=False):
    """ramnet_pack_weight_fold_wino_dgrad / ...2x3_dgrad: the flipped parity filters, reduction index k = (py * 2 + px) * Cout + n over
    4 * Cout, columns = the layer's input channels c: the (16, 4) layout above with one class"""
    Cout, C0 = w5.shape[:2]
    NP = 5 * (tw + 3)
    U4 = (fold_u_abs(w5, tw, dgrad=True) if absolute else fold_u(w5, tw, dgrad=True)).reshape(2, 2, NP, C0, Cout)
    py, px, pos, c, n = torch.meshgrid(torch.arange(2), torch.arange(2), torch.arange(NP), torch.arange(C0), torch.arange(Cout), indexing="ij")
    k = (py * 2 + px) * Cout + n
    idx = ((((k // 16) * (C0 // 64) + c // 64) * NP + pos) * 4 + (c % 64) // 16) * 256 + ((k % 16) // 4 * 16 + c % 16) * 4 + k % 4
    return _scatter(U4, idx, 4 * NP * C0 * Cout)


FOLD_LOST = [[(0, 1), (0,)], [(4,), (3, 4)]]        # [side][slot]: the taps of fine row / column `slot` of the band that leave the image


def border_statement(w5):
    """ramnet_pack_border_weights: rows, cols [2 sides][5 * Cin][2 * Cout] = minus the taps the zero padding removes at the image border
    (rows[side][kx * Cin + ci][slot * Cout + co] = - sum_{a in LOST[side][slot]} w[co][ci][a][kx], cols with the lost direction along kx)
    and their transposes [2][2 * Cout][5 * Cin]; sums of at most two fp32 numbers, one rounding"""
    Cout, Cin = w5.shape[:2]

    def mats(wk):                                   # wk[co][ci][lost direction][kept direction]
        out = []
        for side in range(2):
            slots = [-sum(wk[:, :, a, :] for a in FOLD_LOST[side][slot]) for slot in range(2)]          # [co][ci][kb]
            out.append(torch.stack(slots, 0).permute(3, 2, 0, 1).reshape(5 * Cin, 2 * Cout))
        return torch.stack(out, 0)
    rows, cols = mats(w5), mats(w5.transpose(2, 3))
    return rows, cols, rows.transpose(1, 2).contiguous(), cols.transpose(1, 2).contiguous()


def border_operands(x, w5):
    """float64 e0 / e1 of a folded layer from the definition: the taps that leave the image read, in the replicate-extended form, the clamped
    border line of u = up2x(x): e1[side][b][X][slot * Cout + co] = - sum_{a lost} sum_{kx, ci} w[co][ci][a][kx] u(border row, clamp(X + kx - 2), ci);
    e0 the same along columns, with rows OUTSIDE the image zero (the row correction has already taken those taps out)"""
    u = up2x(x)
    B, H2, W2, Cin = u.shape
    Cout = w5.shape[0]
    rows, cols, _, _ = border_statement(w5)
    ix = (torch.arange(W2)[:, None] + torch.arange(5)[None, :] - 2).clamp(0, W2 - 1)
    iy = torch.arange(H2)[:, None] + torch.arange(5)[None, :] - 2
    oky = ((iy >= 0) & (iy < H2)).to(F64)
    e1 = torch.stack([torch.einsum("bxkc,kcn->bxn", u[:, r][:, ix], rows[s].view(5, Cin, 2 * Cout)) for s, r in ((0, 0), (1, H2 - 1))])
    e0 = torch.stack([torch.einsum("bykc,kcn->byn", u[:, :, c][:, iy.clamp(0, H2 - 1)] * oky[None, :, :, None], cols[s].view(5, Cin, 2 * Cout))
                      for s, c in ((0, 0), (1, W2 - 1))])
    return e0, e1


def pad2(x):
    """ramnet_pad2_sum of an already summed x: replicate-pad [B][H][W][C] by 2"""
    B, H, W, C = x.shape
    iy, ix = (torch.arange(H + 4) - 2).clamp(0, H - 1), (torch.arange(W + 4) - 2).clamp(0, W - 1)
    return x[:, iy][:, :, ix]


def pack_head_statement(w5):
    """ramnet_pack_weight_head: OIHW [Cout <= 32][Cin][5][5] -> [25 * Cin rounded up to even][32], row = tap * Cin + channel, zero beyond"""
    Cout, Cin = w5.shape[:2]
    rows = (25 * Cin + 1) // 2 * 2
    out = torch.zeros(rows, 32, dtype=F64)
    out[:25 * Cin, :Cout] = w5.permute(2, 3, 1, 0).reshape(25 * Cin, Cout)
    return out


# ---------------------------------------------------------------------------------------------------- PARITY4: backward-data of the fold
def parity4_taps_weights(w5):
    """RAMNET_IN_PARITY4 as a tap list over logical_input (the parity sub-grids [B][H][W][4 * C0], C0 = the layer's output channels):
    out(u, v, c) = sum_{py,px} sum_{t,s} g(2 (u - py - t) + py, 2 (v - px - s) + px, n) W4[n][c][py][px][t][s] on the (H + 4) x (W + 4)
    grid of the padded low-res tensor: taps (dy, dx) in -4..0, slice (dy + 4) * 5 + dx + 4 = [4 * C0][Cin] with W4 at t = -dy - py, s = -dx - px"""
    N, C = w5.shape[:2]
    W4 = fold_w4(w5)
    Wt = torch.zeros(25, 4 * N, C, dtype=F64)
    for py in range(2):
        for px in range(2):
            for t in range(4):
                for s in range(4):
                    dy, dx = -py - t, -px - s
                    Wt[(dy + 4) * 5 + dx + 4, (py * 2 + px) * N:(py * 2 + px + 1) * N] = W4[:, :, py, px, t, s]
    return [(dy, dx, (dy + 4) * 5 + dx + 4) for dy in range(-4, 1) for dx in range(-4, 1)], Wt


def parity4_wino(g, w5, family, absolute=True):
    """transformed-domain statement of the backward-data launch: per reduction class (cy, cx) the flipped filter W4[..][3 - t][3 - s] slides
    over the class grid extended by 3 zeros on every side: out(u, v) = sum_{t',s'} gz(u - cy - 3 + t', v - cx - 3 + s') W4f[t'][s'];
    tiles of 2 x TW outputs from (0, 0) on the (H + 4) x (W + 4) grid"""
    BTr, Gr, ATr, BTc, Gc, ATc = [m.abs() if absolute else m for m in WINO[family]]
    tw = ATc.shape[0]
    B, H2, W2, N = g.shape
    H, W, C = H2 // 2, W2 // 2, w5.shape[1]
    Ho, Wo = H + 4, W + 4
    ny, nx = -(-Ho // 2), -(-Wo // tw)
    W4 = fold_w4(w5.abs() if absolute else w5).flip(4, 5)
    out = torch.zeros(B, 2 * ny, tw * nx, C, dtype=F64)
    for cy in range(2):
        for cx in range(2):
            gz = torch.zeros(B, 2 * ny + 4 + 4, tw * nx + 4 + 4, N, dtype=F64)          # class grid with a margin of 4 in front
            gz[:, 4:4 + H, 4:4 + W] = (g.abs() if absolute else g)[:, cy::2, cx::2]
            ry = 2 * torch.arange(ny)[:, None] - cy - 3 + 4 + torch.arange(5)[None, :]
            rx = tw * torch.arange(nx)[:, None] - cx - 3 + 4 + torch.arange(tw + 3)[None, :]
            win = gz[:, ry][:, :, :, rx]
            V = torch.einsum("ar,zyrxck,bc->zyxabk", BTr, win, BTc)
            Uw = torch.einsum("at,nkts,bs->abkn", Gr, W4[:, :, cy, cx], Gc)                 # [a][b][input channel k][reduced n]
            M = torch.einsum("zyxabn,abkn->zyxabk", V, Uw)
            out += torch.einsum("pa,zyxabk,qb->zypxqk", ATr, M, ATc).reshape(B, 2 * ny, tw * nx, C)
    return out[:, :Ho, :Wo]


# ---------------------------------------------------------------------------------------------------- folded backward-weights
# Roundings besides the n tiles that meet in an element: input transform 3 + 3, transform of the gradient tile A g Ac^T (rows of A hold two
# non-zeros: 1 per F(2,4) pass; three with the halves and quarters of F(3,4): 2), the fold in double and its rounding 1, the += 1
R_WGRAD.update({"fold2x2": 6 + 2 + 1 + 1, "fold2x3": 6 + 3 + 1 + 1})
WGRAD_GRID_BITS = {"fold2x2": 0, "fold2x3": 4}      # B^T d B and A g Ac^T are integral for F(2,4) and on 2^-2 each with F(3,4) columns


def fold_class_wgrad(d, py, px):
    """the backward-weights descriptor of parity class (py, px): x0 = the padded input, the class's 16 taps, g = that parity of dout / gmask"""
    return types.SimpleNamespace(in_mode=IN_PLAIN, x0=d.x0, x1=None, xm=None, stride=1, Ho=d.Ho, Wo=d.Wo, taps=[t[:2] for t in fold_taps(py, px)],
                                 dout=d.dout[:, py::2, px::2], gmask=None if d.gmask is None else d.gmask[:, py::2, px::2])


def fold_wgrad_statement(d):
    """RAMNET_ALGO_WINOGRAD24 / _2X3 backward-weights: dW4[class][t*4 + s][c][n] = sum_{b, a, b'} xpad(a + py + t, b' + px + s, c) g(2a + py, 2b' + px, n),
    g = dout (* (gmask > 0)), its absolute-value companion, dbias over the full-resolution gradient"""
    cls = [wgrad_statement(fold_class_wgrad(d, py, px)) for py in range(2) for px in range(2)]
    return types.SimpleNamespace(dW4=torch.stack([s.dW for s in cls]), dW4_abs=torch.stack([s.dW_abs for s in cls]), dbias=sum(s.dbias for s in cls),
                                 dbias_abs=sum(s.dbias_abs for s in cls), n_bias=sum(s.n_bias for s in cls))


def fold_wgrad_wino(d, family, absolute=True):
    """the transformed-domain form: dU[class][a][b][c][n] = sum over tiles and images (B^T d Bc)[a][b][c] (A g Ac^T)[a][b][n] on 2 x TW tiles from
    (0, 0) (windows clamped to the padded input, the gradient zero outside the grid), and its fold G^T dU Gc = dW4 [4][16][C][N]; absolute:
    every matrix and operand by its absolute value.  Returns (dU, folded, tiles per class)"""
    BTr, Gr, ATr, BTc, Gc, ATc = [m.abs() if absolute else m for m in WINO[family]]
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    tw = ATc.shape[0]
    B, Hp, Wp, C = d.x0.shape
    H, W = d.Ho, d.Wo
    ny, nx = -(-H // 2), -(-W // tw)
    g = f(d.dout) if d.gmask is None else f(d.dout) * (d.gmask > 0).to(F64)
    dU = []
    for py in range(2):
        for px in range(2):
            ry = (2 * torch.arange(ny)[:, None] + py + torch.arange(5)[None, :]).clamp_max(Hp - 1)
            rx = (tw * torch.arange(nx)[:, None] + px + torch.arange(tw + 3)[None, :]).clamp_max(Wp - 1)
            V = torch.einsum("ar,zyrxck,bc->zyxabk", BTr, f(d.x0)[:, ry][:, :, :, rx], BTc)
            gp = torch.zeros(B, 2 * ny, tw * nx, g.shape[3], dtype=F64)
            gp[:, :H, :W] = g[:, py::2, px::2]
            Y = torch.einsum("pa,zypxqn,qb->zyxabn", ATr, gp.view(B, ny, 2, nx, tw, -1), ATc)
            dU.append(torch.einsum("zyxabk,zyxabn->abkn", V, Y))
    dU = torch.stack(dU)                                                         # [4][5][tw + 3][C][N]
    folded = torch.einsum("at,zabkn,bs->ztskn", Gr, dU, Gc).reshape(4, 16, C, -1)
    return dU, folded, B * ny * nx


def fold_unpack_statement(gold, dW4, w4, wr, wc):
    """ramnet_fold_unpack_wgrad[2x3]: grad[o][i][k][l] += sum_{p,q,t,s} FA[p][t][k] FA[q][s][l] (dW4 + w4)[p][q][t][s][i][o] - the border-GEMM
    gradients wr / wc [2][5 * Cin][2 * Cout] routed back to the taps they summed (FOLD_LOST); dW4 = what the Winograd-domain workspaces stand
    for ([4][16][Cin][Cout]), w4 = the direct parity launches' workspace in the same layout"""
    Cout, Cin = gold.shape[:2]
    FA = fold_matrix()
    d4 = (dW4 + w4).view(2, 2, 4, 4, Cin, Cout)
    g = gold + torch.einsum("ptk,qsl,pqtsio->oikl", FA, FA, d4)
    r, c = wr.view(2, 5, Cin, 2, Cout), wc.view(2, 5, Cin, 2, Cout)
    for side in range(2):
        for slot in range(2):
            for a in FOLD_LOST[side][slot]:
                g[:, :, a, :] -= r[side, :, :, slot, :].permute(2, 1, 0)
                g[:, :, :, a] -= c[side, :, :, slot, :].permute(2, 1, 0)
    return g
