"""Float64 statements of the input-gradient launches, written from include/ramnet_hip.h in plain torch indexing (not from the kernels),
each with its absolute-value companion (the same expression on absolute values: S_abs of the summation bounds).  No GPU, no library.

  head_dgrad        ramnet_head_dgrad: backward-data of the 5x5, stride-1, pad-2 head layer, optional ReLU mask operand
  reflect_pad_bwd   ramnet_reflect_pad_bwd: every frame pixel sums the padded positions that mirror onto it, in the header's order
  nhwc_unpad        ramnet_nhwc_unpad_to_nchw: a copy
"""
import torch

F64 = torch.float64
U = 2.0 ** -24


def head_dgrad(dy, w, y=None, ld=None, absolute=False):
    """dy [B][H][W][Cout], w OIHW [Cout][Cin][5][5], y = the mask operand (a term counts where y > 0) or None -> dx [B][H][W][ld]:
    dx[b,y,x,c] = sum_{n,ky,kx} w[n,c,ky,kx] m(b,y+2-ky,x+2-kx,n) dy[b,y+2-ky,x+2-kx,n], zero outside the image; lanes Cin..ld-1 zero."""
    dy, w = dy.to(F64), w.to(F64)
    if absolute:
        dy, w = dy.abs(), w.abs()
    B, H, W, Cout = dy.shape
    Cin = w.shape[1]
    ld = (Cin + 3) // 4 * 4 if ld is None else ld
    g = dy if y is None else dy * (y.to(F64) > 0).to(F64)
    pad = torch.zeros(B, H + 4, W + 4, Cout, dtype=F64)
    pad[:, 2:H + 2, 2:W + 2] = g
    dx = torch.zeros(B, H, W, ld, dtype=F64)
    for ky in range(5):
        for kx in range(5):
            # padded index of (y + 2 - ky, x + 2 - kx) is (y + 4 - ky, x + 4 - kx)
            dx[..., :Cin] += pad[:, 4 - ky:4 - ky + H, 4 - kx:4 - kx + W] @ w[:, :, ky, kx]
    return dx


def head_dgrad_partial_max(dy, w, y=None):
    """An upper limit of every partial sum of the statement in any order: the absolute-value statement's maximum."""
    return float(head_dgrad(dy, w, y, absolute=True).max())


def mirrors(s, n, pad0, nc):
    """Padded positions along one axis (extent n, `pad0` positions in front, nc in all) that reflect onto frame position s, ascending."""
    out = []
    if 1 <= s <= pad0:
        out.append(pad0 - s)
    out.append(pad0 + s)
    if s <= n - 2 and pad0 + 2 * (n - 1) - s < nc:
        out.append(pad0 + 2 * (n - 1) - s)
    return out


def reflect_pad_bwd(g, C, H, W, top, left, nhwc, absolute=False, dtype=F64):
    """g = the gradient of the padded tensor, [B][Hc][Wc][Cpad] (nhwc) or [B][C][Hc][Wc] -> dx [B][C][H][W].  The header's order: padded
    rows ascending, inside a row padded columns ascending, every term added to a sum that starts at zero (dtype=float32 follows the
    kernel's own roundings)."""
    g = g.to(dtype)
    if absolute:
        g = g.abs()
    if nhwc:
        g = g[..., :C].permute(0, 3, 1, 2)
    B, _, Hc, Wc = g.shape
    dx = torch.zeros(B, C, H, W, dtype=dtype)
    for sy in range(H):
        for sx in range(W):
            acc = torch.zeros(B, C, dtype=dtype)
            for py in mirrors(sy, H, top, Hc):
                for px in mirrors(sx, W, left, Wc):
                    acc = acc + g[:, :, py, px]
            dx[:, :, sy, sx] = acc
    return dx


def nhwc_unpad(src, C):
    """[B][H][W][Cpad] -> [B][C][H][W]"""
    return src[..., :C].permute(0, 3, 1, 2).contiguous()


def crop_split(h, w, num_encoders):
    """(Hc, Wc, top, left) of CropParameters (utils/inference_utils.py:278-314): the next multiple of 2^num_encoders, the ceil of half the
    excess above / to the left."""
    f = 2 ** num_encoders
    Hc, Wc = -(-h // f) * f, -(-w // f) * f
    return Hc, Wc, (Hc - h + 1) // 2, (Wc - w + 1) // 2


# (H, W, Hc, Wc, top, left) of the reflect-pad cases: 5 x 7 and 20 x 22 with the CropParameters split of the excess (num_encoders 3 and 5),
# and 5 x 7 padded by 3 on every side, where the middle pixels are met by three positions per axis (nine in all).  Reflection needs
# pad < extent on every side (torch.nn.ReflectionPad2d and ramnet_reflect_pad both refuse more): 16 x 16 cannot be reached from 5 rows.
PAD_CASES = [(5, 7) + crop_split(5, 7, 3), (5, 7, 11, 13, 3, 3), (20, 22) + crop_split(20, 22, 5)]
