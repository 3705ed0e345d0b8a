"""Float64 statements of the point-wise and glue entry points of csrc/pointwise.hip, one function per entry point, written from the
comments of include/ramnet_hip.h (test references only: nothing under rpg_ramnet_amd/ imports this module).

Tensors are torch float64, activations NHWC as in the C ABI.  The adjoints (unpad2_fold, up2x_border_col2im, upsample2x_bwd) and the cell /
prediction-head backward maps are torch.autograd.grad of the forward statements: no gather is restated by hand.
tests/test_pointwise_restatement_cpu.py anchors this file without a GPU; tests/test_hip_pointwise.py compares the kernels with it."""
import torch
import torch.nn.functional as F

F64 = torch.float64


def _f64(t):
    return None if t is None else torch.as_tensor(t).to(F64)


# ------------------------------------------------------------------------------------------------ layout maps
def nchw_to_nhwc_pad(src, Cpad):
    """[B, C, H, W] -> [B, H, W, Cpad], channels C.. zero."""
    B, C, H, W = src.shape
    out = src.new_zeros(B, H, W, Cpad)
    out[..., :C] = src.permute(0, 2, 3, 1)
    return out


def _reflect(k, n):
    """ReflectionPad2d index rule (no repeated border pixel): k < 0 -> -k, k >= n -> 2 (n - 1) - k."""
    k = torch.where(k < 0, -k, k)
    return torch.where(k >= n, 2 * (n - 1) - k, k)


def reflect_pad(src, top, left, Hc, Wc, Cpad, nhwc):
    """[B, C, H, W] reflect-padded to [Hc, Wc] with `top` rows above and `left` columns to the left; nhwc = 1: NHWC with the channels
    zero-padded to Cpad, nhwc = 0: NCHW (Cpad ignored)."""
    B, C, H, W = src.shape
    sy = _reflect(torch.arange(Hc) - top, H)
    sx = _reflect(torch.arange(Wc) - left, W)
    out = src[:, :, sy][:, :, :, sx]
    return nchw_to_nhwc_pad(out, Cpad) if nhwc else out.contiguous()


def crop_parameters(H, W, num_encoders):
    """Paddings of CropParameters: the next multiple of 2^num_encoders, top / left = ceil of half the excess.  (Hc, Wc, top, bottom, left, right)"""
    m = 2 ** num_encoders
    Hc, Wc = -(-H // m) * m, -(-W // m) * m
    top, left = -(-(Hc - H) // 2), -(-(Wc - W) // 2)
    return Hc, Wc, top, Hc - H - top, left, Wc - W - left


def space_to_depth2(x, inverse=False):
    """[B, H, W, C] -> [B, H/2, W/2, 4C] with channel (a*2 + c)*C + ch = x[b][2i + a][2j + c][ch]; inverse: the way back."""
    if not inverse:
        B, H, W, C = x.shape
        out = x.new_empty(B, H // 2, W // 2, 4 * C)
        for a in range(2):
            for c in range(2):
                out[..., (a * 2 + c) * C:(a * 2 + c + 1) * C] = x[:, a::2, c::2]
        return out
    B, Ho, Wo, C4 = x.shape
    C = C4 // 4
    out = x.new_empty(B, 2 * Ho, 2 * Wo, C)
    for a in range(2):
        for c in range(2):
            out[:, a::2, c::2] = x[..., (a * 2 + c) * C:(a * 2 + c + 1) * C]
    return out


def concat2(a, b):
    """y[pix] = [a[pix] | b[pix]]"""
    return torch.cat([a, b], -1)


def split2(y, Ca, Cb):
    return y[..., :Ca].contiguous(), y[..., Ca:Ca + Cb].contiguous()


def frame_gather(dy, mask=None):
    """dy [B, H2, W2, C] (* (mask > 0)): rows [2][B][W2][2][C] = image rows (0, 1) and (H2-2, H2-1), cols [2][B][H2][2][C] = image
    columns (0, 1) and (W2-2, W2-1): side 0 = top / left, the two slots of a side in ascending image order."""
    g = dy if mask is None else torch.where(mask > 0, dy, torch.zeros_like(dy))
    B, H2, W2, C = g.shape
    rows = torch.stack([g[:, 0:2].permute(0, 2, 1, 3), g[:, H2 - 2:H2].permute(0, 2, 1, 3)])          # [2][B][W2][2][C]
    cols = torch.stack([g[:, :, 0:2], g[:, :, W2 - 2:W2]])                                             # [2][B][H2][2][C]
    return rows.contiguous(), cols.contiguous()


# ------------------------------------------------------------------------------------------------ decoder glue
def up2x(x):
    """bilinear x2 of an NHWC tensor: F.interpolate(scale_factor=2, mode="bilinear", align_corners=False)"""
    return F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


def pad2_sum(x, skip=None):
    """replicate padding by 2 of x (+ skip): [B, H, W, C] -> [B, H+4, W+4, C]"""
    s = x if skip is None else x + skip
    return F.pad(s.permute(0, 3, 1, 2), (2, 2, 2, 2), mode="replicate").permute(0, 2, 3, 1)


def up2x_border_im2col(x, skip=None):
    """u = up2x(x + skip) [B, 2H, 2W, C].  rows [2][B][2W][5][C]: entry (o, k) of side 0 / 1 = u[top / bottom row][clamp(o + k - 2)];
    cols [2][B][2H][5][C]: entry (o, k) = u[o + k - 2][left / right column], zero where o + k - 2 lies outside the image."""
    u = up2x(x if skip is None else x + skip)
    B, H2, W2, C = u.shape
    k = torch.arange(5)
    ix = (torch.arange(W2)[:, None] + k[None, :] - 2).clamp(0, W2 - 1)                   # [W2][5]
    rows = torch.stack([u[:, 0][:, ix], u[:, H2 - 1][:, ix]])                            # [2][B][W2][5][C]
    iy = torch.arange(H2)[:, None] + k[None, :] - 2                                      # [H2][5]
    inside = ((iy >= 0) & (iy < H2)).to(u.dtype)[None, :, :, None]
    iyc = iy.clamp(0, H2 - 1)
    cols = torch.stack([u[:, :, 0][:, iyc] * inside, u[:, :, W2 - 1][:, iyc] * inside])  # [2][B][H2][5][C]
    return rows, cols


def _adjoint(fwd, shape, *cot):
    """The float64 autograd adjoint of the linear map fwd at an input of `shape`, applied to the cotangents `cot` (one per output)."""
    x = torch.zeros(shape, dtype=F64, requires_grad=True)
    out = fwd(x)
    out = out if isinstance(out, tuple) else (out,)
    return torch.autograd.grad(out, x, [c.to(F64) for c in cot])[0]


def unpad2_fold(dxpad):
    """adjoint of pad2_sum: [B, H+4, W+4, C] -> [B, H, W, C]"""
    B, Hp, Wp, C = dxpad.shape
    return _adjoint(pad2_sum, (B, Hp - 4, Wp - 4, C), dxpad)


def up2x_border_col2im(rows, cols, dx):
    """dx + the adjoint of up2x_border_im2col applied to (rows, cols)"""
    return dx + _adjoint(up2x_border_im2col, dx.shape, rows, cols)


def upsample2x_bwd(dup):
    """adjoint of up2x: [B, 2H, 2W, C] -> [B, H, W, C]"""
    B, H2, W2, C = dup.shape
    return _adjoint(up2x, (B, H2 // 2, W2 // 2, C), dup)


# ------------------------------------------------------------------------------------------------ simple maps, bias
def relu_bwd(dy, y):
    return torch.where(y > 0, dy, torch.zeros_like(dy))


def add(a, b):
    return a + b


def bias_grad(dy, mask, db):
    """db[c] + sum over the pixels of dy[pix][c] * (mask[pix][c] > 0)"""
    g = dy if mask is None else torch.where(mask > 0, dy, torch.zeros_like(dy))
    return db + g.reshape(-1, g.shape[-1]).sum(0)


# ------------------------------------------------------------------------------------------------ prediction head
def pred_fwd(x, w, b=None, sigmoid=True):
    """x [npix, C], w [C], b scalar tensor or None: sigma(x.w + b) or x.w + b"""
    z = x @ w + (0 if b is None else b)
    return torch.sigmoid(z) if sigmoid else z


def pred_bwd(x, w, dy, y=None, dw0=None, db0=None):
    """Gradients of the head with respect to x, w, b for the cotangent dy.  y = the saved sigmoid output (the kernels read it back instead
    of recomputing it) or None for the linear head.  Returns (dx [npix, C], dw0 + dw [C], db0 + db)."""
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    b = torch.zeros((), dtype=F64, requires_grad=True)
    z = x @ w + b
    if y is None:
        dz = dy
    else:                          # the activation seen through its saved output: y = sigma(logit(y))
        zl = torch.logit(y).requires_grad_(True)
        dz = torch.autograd.grad(torch.sigmoid(zl), zl, dy)[0]
    dx, dw, db = torch.autograd.grad(z, (x, w, b), dz)
    return dx, dw + (0 if dw0 is None else dw0), db + (0 if db0 is None else db0)


# ------------------------------------------------------------------------------------------------ recurrent cells
def gru_cell_from_preacts(h, pu, pr, po_of_hr):
    """The documented ConvGRU cell: u = sigma(pu), r = sigma(pr), o = tanh(po) where the candidate sees h.r, h' = h (1 - u) + u o.
    po_of_hr: callable hr -> po (the candidate convolution)."""
    u, r = torch.sigmoid(pu), torch.sigmoid(pr)
    o = torch.tanh(po_of_hr(h * r))
    return h * (1 - u) + u * o


def gru_bwd_a(dhn, u, o, h=None):
    """Stage A of the cell backward from the saved activations: gradients of h' = h (1 - u) + u o, u = sigma(pu), o = tanh(po), with
    respect to po, pu and (directly) h for the cotangent dh'.  Returns (dpo, dpu, dh)."""
    h = torch.zeros_like(u) if h is None else h
    pu, po, hl = torch.logit(u).requires_grad_(True), torch.atanh(o).requires_grad_(True), h.clone().requires_grad_(True)
    uu, oo = torch.sigmoid(pu), torch.tanh(po)
    hn = hl * (1 - uu) + uu * oo
    dpo, dpu, dh = torch.autograd.grad(hn, (po, pu, hl), dhn)
    return dpo, dpu, dh


def gru_bwd_b(dhr, r, dh, h=None):
    """Stage B: the candidate's input h.r with r = sigma(pr); for the cotangent d(h.r): (dpr, dh + the gradient with respect to h)."""
    h = torch.zeros_like(r) if h is None else h
    pr, hl = torch.logit(r).requires_grad_(True), h.clone().requires_grad_(True)
    dpr, dhh = torch.autograd.grad(hl * torch.sigmoid(pr), (pr, hl), dhr)
    return dpr, dh + dhh


def lstm_bwd(gates, cnew, cprev=None, dhn=None, dcn=None):
    """gates [npix, 4C] = activated [i | f | o | g]; the cell c' = f c + i g, h' = o tanh(c') with c' at its saved value `cnew`;
    cotangents dh', dc' (None: 0).  Returns (dpre [npix, 4C] in gate order i, f, o, g; dc_prev)."""
    C = gates.shape[-1] // 4
    gi, gf, go, gc = (gates[..., k * C:(k + 1) * C] for k in range(4))
    cprev = torch.zeros_like(cnew) if cprev is None else cprev
    dhn = torch.zeros_like(cnew) if dhn is None else dhn
    dcn = torch.zeros_like(cnew) if dcn is None else dcn
    pi, pf, po = (torch.logit(t).requires_grad_(True) for t in (gi, gf, go))
    pg, cp = torch.atanh(gc).requires_grad_(True), cprev.clone().requires_grad_(True)
    c = torch.sigmoid(pf) * cp + torch.sigmoid(pi) * torch.tanh(pg)
    c = c + (cnew - c).detach()                     # the saved value, the cell's derivative
    hn = torch.sigmoid(po) * torch.tanh(c)
    di, df, do, dg, dcp = torch.autograd.grad((hn, c), (pi, pf, po, pg, cp), (dhn, dcn))
    return torch.cat([di, df, do, dg], -1), dcp


def lstm_bwd_masked(gates, cnew, active, hw, cprev=None, dhn=None, dcn=None):
    """lstm_bwd with per-sample flags active [B] (pixel p belongs to sample p // hw): inactive pixels get dpre = 0 and dc_prev = dc'
    (None: 0).  dxh [npix, 2C] = 0 except the h half ([C:]) of inactive pixels = dh' (None: 0).  Returns (dpre, dc_prev, dxh)."""
    npix, C = cnew.shape
    dpre, dcp = lstm_bwd(gates, cnew, cprev, dhn, dcn)
    act = (torch.as_tensor(active) != 0).repeat_interleave(hw)[:, None]
    zero = torch.zeros_like(cnew)
    dpre = torch.where(act, dpre, torch.zeros_like(dpre))
    dcp = torch.where(act, dcp, zero if dcn is None else dcn)
    dxh = torch.cat([zero, torch.where(act, zero, zero if dhn is None else dhn)], -1)
    return dpre, dcp, dxh
