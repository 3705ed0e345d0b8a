"""CPU: the F(2x3,4x4) Winograd transform of the folded decoders (csrc/conv_wino24.hip, TW = 3) — the 1-D identities of its row and
column transforms and the 2-D form against conv2d in float64 — and the plain-torch statement of its weight packs (test reference
only; tests/test_hip_fold_wino2x3.py holds the packs against it)."""
import torch
import torch.nn.functional as F

import torch_restatements as tr
from rpg_ramnet_amd.ops import _fold_pair, fold_weights

# columns: F(3,4), points 0, 1, -1, 1/2, -1/2, inf (wincnn convention); rows keep F(2,4) (tr.W24_*)
W23_BT = [[1 / 4, 0, -5 / 4, 0, 1, 0], [0, -1 / 4, -1 / 4, 1, 1, 0], [0, 1 / 4, -1 / 4, -1, 1, 0], [0, -1 / 2, -1, 1 / 2, 1, 0],
          [0, 1 / 2, -1, -1 / 2, 1, 0], [0, 1 / 4, 0, -5 / 4, 0, 1]]
W23_AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 1 / 2, -1 / 2, 0], [0, 1, 1, 1 / 4, 1 / 4, 1]]
W23_G = [[4, 0, 0, 0], [2 / 3, 2 / 3, 2 / 3, 2 / 3], [2 / 3, -2 / 3, 2 / 3, -2 / 3], [-8 / 3, -4 / 3, -2 / 3, -1 / 3], [-8 / 3, 4 / 3, -2 / 3, 1 / 3],
         [0, 0, 0, 1]]


def _t(m, device="cpu"):
    return torch.tensor(m, dtype=torch.float64, device=device)


def fold_weights_wino2x3(w):
    """OIHW 5x5 -> U[class = py*2+px][pos = a*6+b][Cin][Cout] = G W4 Gc^T of the four 4x4 parity filters (float64)."""
    u = torch.einsum("at,bs,oipqts->pqabio", _t(tr.W24_G, w.device), _t(W23_G, w.device), fold_weights(w))
    return u.reshape(4, 30, w.shape[1], w.shape[0])


def pack_fold_wino2x3(w):
    """fold_weights_wino2x3() in the lane order of conv_wino24_kernel<4, .., 3>'s B operand: the 64-column layouts of tr.pack_fold_wino
    with 30 positions."""
    Cout, Cin = w.shape[0], w.shape[1]
    if _fold_pair(Cout, Cin):
        u = fold_weights_wino2x3(w).float().view(2, 2, 30, Cin, 32).permute(0, 2, 3, 1, 4).reshape(2, 30, Cin // 16, 4, 4, 1, 4, 16)
        return u.permute(0, 2, 5, 1, 6, 3, 7, 4).contiguous().view(-1)
    assert Cout % 64 == 0 and Cin % 16 == 0
    u = fold_weights_wino2x3(w).float().view(4, 30, Cin // 16, 4, 4, Cout // 64, 4, 16)        # cls pos chunk ks j nb cq l15
    return u.permute(0, 2, 5, 1, 6, 3, 7, 4).contiguous().view(-1)                         # cls chunk nb pos cq ks l15 j


def pack_fold_wino2x3_dgrad(w):
    """Backward-data (RAMNET_IN_PARITY4) pack: tr.pack_fold_wino_dgrad with the column matrix of F(2x3) and 30 positions."""
    Cout, Cin = w.shape[0], w.shape[1]
    u = torch.einsum("at,bs,ncpqts->abpqnc", _t(tr.W24_G, w.device), _t(W23_G, w.device), fold_weights(w).flip(4, 5))
    u = u.reshape(1, 30, 4 * Cout, Cin).float().view(1, 30, 4 * Cout // 16, 4, 4, Cin // 64, 4, 16)
    return u.permute(0, 2, 5, 1, 6, 3, 7, 4).contiguous().view(-1)


def _corr1d(d, g, m):
    return torch.stack([sum(g[s] * d[i + s] for s in range(4)) for i in range(m)])


def test_one_dimensional_identities_in_float64():
    """A^T [(G g) .* (B^T d)] = the 4-tap correlation of d, for the rows' F(2,4) and the columns' F(3,4)."""
    torch.manual_seed(0)
    for BT, G, AT, m in ((tr.W24_BT, tr.W24_G, tr.W24_AT, 2), (W23_BT, W23_G, W23_AT, 3)):
        for _ in range(20):
            d, g = torch.randn(m + 3, dtype=torch.float64), torch.randn(4, dtype=torch.float64)
            y = _t(AT) @ ((_t(G) @ g) * (_t(BT) @ d))
            assert float((y - _corr1d(d, g, m)).abs().max()) < 1e-13


def test_two_dimensional_form_equals_conv2d():
    """Y = A^T [sum_ci U .* (B^T d Bc)] Ac on 2 x 3 tiles of the four parity grids of the replicate-padded input, with U from the pack
    statement's float64 weights, equals conv5x5(bilinear_x2(x)) away from the border (the border is the folded layer's `frame`)."""
    torch.manual_seed(1)
    B, Cin, Cout, H, W = 2, 3, 4, 6, 9
    x = torch.randn(B, Cin, H, W, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 5, 5, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False), w, None, 1, 2)
    xpad = F.pad(x, (2, 2, 2, 2), mode="replicate")
    U = fold_weights_wino2x3(w).view(2, 2, 5, 6, Cin, Cout)
    got = torch.empty(B, Cout, 2 * H, 2 * W, dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            win = xpad[:, :, py:, px:].unfold(2, 5, 2).unfold(3, 6, 3)[:, :, :H // 2, :W // 3]       # [B][Cin][ty][tx][5][6]
            V = torch.einsum("ar,bc,kiyxrc->kiyxab", _t(tr.W24_BT), _t(W23_BT), win)
            M = torch.einsum("abio,kiyxab->koyxab", U[py, px], V)
            Y = torch.einsum("ma,nb,koyxab->koymxn", _t(tr.W24_AT), _t(W23_AT), M).reshape(B, Cout, H, W)
            got[:, :, py::2, px::2] = Y
    assert float((got - ref)[:, :, 2:-2, 2:-2].abs().max() / ref.abs().max()) < 1e-12
