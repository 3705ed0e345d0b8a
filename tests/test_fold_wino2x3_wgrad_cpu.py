"""CPU, float64: backward-weights of the folded decoders in the F(2x3,4x4) domain (csrc/conv_wgrad_wino24.hip, conv_wgrad_wino24_kernel_2x3)
— G_r^T [sum over tiles (B_r^T d B_c) . (A_r g A_c^T)] G_c equals the directly summed 4x4 parity-filter gradient — and the plain-torch
statements that tests/test_hip_fold_wino2x3_wgrad.py holds the kernel and ramnet_fold_unpack_wgrad2x3 against (test references only)."""
import torch
import torch.nn.functional as F

import torch_restatements as tr
from test_fold_wino2x3_cpu import W23_AT, W23_BT, W23_G, _t

COLS = {2: (tr.W24_BT, tr.W24_AT, tr.W24_G), 3: (W23_BT, W23_AT, W23_G)}         # tile width -> column matrices (rows: F(2,4) always)


def fold_wgrad_du(xpad, g, tw):
    """dU[class = py*2+px][pos = a*(tw+3) + b][Cin][Cout] = sum over 2 x tw tiles of (B_r^T d B_c) . (A_r g A_c^T) in the dtype of the inputs.
    xpad: [B][Cin][H+4][W+4] (replicate-padded low-res input), g: [B][Cout][2H][2W] (gradient, ReLU mask applied).  Gradient tiles are
    zero-padded to whole tiles; the windows that then overhang xpad read zeros (any finite value would do: see the kernel's header)."""
    B, Cin, Hp, Wp = xpad.shape
    H, W = Hp - 4, Wp - 4
    ty, tx = -(-H // 2), -(-W // tw)
    BTc, ATc, _ = (_t(m, xpad.device).to(xpad.dtype) for m in COLS[tw])
    BTr, ATr = _t(tr.W24_BT, xpad.device).to(xpad.dtype), _t(tr.W24_AT, xpad.device).to(xpad.dtype)
    out = []
    for py in range(2):
        for px in range(2):
            need_h, need_w = py + 2 * (ty - 1) + 5, px + tw * (tx - 1) + tw + 3
            xp = F.pad(xpad, (0, max(need_w - Wp, 0), 0, max(need_h - Hp, 0)))
            win = xp[:, :, py:, px:].unfold(2, 5, 2).unfold(3, tw + 3, tw)[:, :, :ty, :tx]                   # [B][Cin][ty][tx][5][tw+3]
            gc = F.pad(g[:, :, py::2, px::2], (0, tx * tw - W, 0, ty * 2 - H))
            gt = gc.unfold(2, 2, 2).unfold(3, tw, tw)                                                          # [B][Cout][ty][tx][2][tw]
            V = torch.einsum("ar,bc,kiyxrc->kiyxab", BTr, BTc, win)
            Z = torch.einsum("ma,nb,koyxmn->koyxab", ATr, ATc, gt)
            out.append(torch.einsum("kiyxab,koyxab->abio", V, Z).reshape(5 * (tw + 3), Cin, g.shape[1]))
    return torch.stack(out, 0)


def parity_filter_grads(xpad, g):
    """dW4[class][t][s][Cin][Cout] = sum_{b,i,j} xpad[b, :, i + py + t, j + px + s] g[b, :, 2i + py, 2j + px], summed directly."""
    B, Cin, Hp, Wp = xpad.shape
    H, W = Hp - 4, Wp - 4
    out = torch.zeros(4, 4, 4, Cin, g.shape[1], dtype=xpad.dtype, device=xpad.device)
    for py in range(2):
        for px in range(2):
            gc = g[:, :, py::2, px::2]
            for t in range(4):
                for s in range(4):
                    out[py * 2 + px, t, s] = torch.einsum("kiyx,koyx->io", xpad[:, :, py + t:py + t + H, px + s:px + s + W], gc)
    return out


def du_to_parity_filters(dU, tw):
    """dW4 = G_r^T dU G_c per class: [4][5*(tw+3)][Cin][Cout] -> [4][4][4][Cin][Cout]."""
    Gc, Gr = _t(COLS[tw][2], dU.device).to(dU.dtype), _t(tr.W24_G, dU.device).to(dU.dtype)
    return torch.einsum("at,bs,pabio->ptsio", Gr, Gc, dU.view(4, 5, tw + 3, dU.shape[2], dU.shape[3]))


def fold_unpack_torch_2x3(w4, dU, dU3, wr, wc, Cout, Cin, CinWs):
    """Plain-torch statement of ramnet_fold_unpack_wgrad2x3: tr.fold_unpack_torch with dW4 += G_r^T dU3 G_c of the [4][30][CinWs][Cout]
    workspace of the F(2x3,4x4) launches."""
    if dU3 is not None:
        w4 = w4 + du_to_parity_filters(dU3.view(4, 30, CinWs, Cout), 3).to(w4.dtype).reshape(-1)
    return tr.fold_unpack_torch(w4, dU, wr, wc, Cout, Cin, CinWs)


def _case(H, W, seed=0, B=2, Cin=3, Cout=2):
    torch.manual_seed(seed)
    x = torch.randn(B, Cin, H, W, dtype=torch.float64)
    g = torch.randn(B, Cout, 2 * H, 2 * W, dtype=torch.float64)
    return F.pad(x, (2, 2, 2, 2), mode="replicate"), g


def test_winograd_domain_sum_equals_the_parity_filter_gradient():
    """All four parity classes on 5 x 11 (odd height, 11 = 3.3 + 2 columns), 4 x 4 (less than one tile column pair), 6 x 9 (whole tiles) and
    7 x 13 (13 = 3.4 + 1: the tile column whose window column 4 overhangs), for F(2x3) and, as the yardstick, F(2x2)."""
    for H, W in ((5, 11), (4, 4), (6, 9), (7, 13)):
        xpad, g = _case(H, W, seed=H)
        ref = parity_filter_grads(xpad, g)
        for tw in (3, 2):
            got = du_to_parity_filters(fold_wgrad_du(xpad, g, tw), tw)
            assert float((got - ref).abs().max() / ref.abs().max()) < 1e-12, (H, W, tw)


def test_overhanging_windows_only_meet_zero_gradients_or_cancel():
    """What a window reads past the padded tensor does not reach the filter gradient: finite garbage there changes nothing (window row 4
    and column 5 meet zero gradient entries; column 4 past the row's end cancels in G_r^T (.) G_c, and the kernel reads it as zeros)."""
    H, W = 5, 13
    xpad, g = _case(H, W, seed=3)
    ref = parity_filter_grads(xpad, g)
    big = torch.randn(xpad.shape[0], xpad.shape[1], H + 4 + 2, W + 4 + 3, dtype=torch.float64) * 3.0
    big[:, :, :H + 4, :W + 4] = xpad

    def du(xp):
        ty, tx = 3, 5
        BTr, ATr, BTc, ATc = _t(tr.W24_BT), _t(tr.W24_AT), _t(W23_BT), _t(W23_AT)
        out = []
        for py in range(2):
            for px in range(2):
                win = xp[:, :, py:, px:].unfold(2, 5, 2).unfold(3, 6, 3)[:, :, :ty, :tx]
                gt = F.pad(g[:, :, py::2, px::2], (0, tx * 3 - W, 0, ty * 2 - H)).unfold(2, 2, 2).unfold(3, 3, 3)
                V = torch.einsum("ar,bc,kiyxrc->kiyxab", BTr, BTc, win)
                Z = torch.einsum("ma,nb,koyxmn->koyxab", ATr, ATc, gt)
                out.append(torch.einsum("kiyxab,koyxab->abio", V, Z).reshape(30, xp.shape[1], g.shape[1]))
        return torch.stack(out, 0)

    got = du_to_parity_filters(du(big), 3)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-12


def test_unpack_statement_adds_the_2x3_workspace():
    """fold_unpack_torch_2x3 on a dU3 workspace alone gives A_py^T dW4 A_px of the parity-filter gradients, i.e. the 5x5 gradient of
    conv5x5(bilinear_x2(x)) away from the border terms (wr = wc = 0), and equals the F(2x2) statement on the same data."""
    H, W, Cin, Cout = 5, 11, 4, 2
    xpad, g = _case(H, W, seed=5, Cin=Cin, Cout=Cout)
    dU3 = fold_wgrad_du(xpad, g, 3).float().reshape(-1)
    dU2 = fold_wgrad_du(xpad, g, 2).float().reshape(-1)
    z4, zr = torch.zeros(64 * Cin * Cout), torch.zeros(2, 5 * Cin, 2 * Cout)
    a = fold_unpack_torch_2x3(z4, None, dU3, zr, zr.clone(), Cout, Cin, Cin)
    b = tr.fold_unpack_torch(z4, dU2, zr, zr.clone(), Cout, Cin, Cin)
    both = fold_unpack_torch_2x3(z4, dU2, dU3, zr, zr.clone(), Cout, Cin, Cin)
    assert float((a - b).abs().max() / b.abs().max()) < 1e-5
    assert float((both - 2 * b).abs().max() / b.abs().max()) < 1e-5
