"""The callers at the addressing limits (profiles/address_limit_tests_notes.md, section 5): whole layers of rpg_ramnet_amd at the smallest real
sizes that cross a limit, shared by tests/test_address_limits_cpu.py (the data rule, without a GPU) and tests/test_hip_address_limits.py.

Pitches inside ops.py are the tensors' own, so these rows need real sizes (2048 x 2048, B = 2).  What keeps them cheap: the input x is a
FUNCTION of its flat index (a 32-bit integer hash: sparse integers), so the device fills gigabytes of it in place and the CPU evaluates it
only where it is needed; and the output gradient dy is zero except at a few hundred SAMPLE pixels (the four corners of the first and the
last image, the last rows of the last image, seeded ones between).  Every gradient is then a sum over the samples' neighbourhoods, which
the float64 reference below forms from a few thousand pixels: ALL of dW and dbias, and dx at every pixel that can be non-zero (the rest
must be zero).  Integer data: the reference is exact in fp32 where its statement on absolute values stays far below 2^24 (asserted on the
CPU)."""
import types

import torch

F64 = torch.float64


def xval(idx, seed, dens):
    """x at the flat indices `idx` (int64 tensor, any device): -1, 0 or 1, non-zero with probability dens / 256"""
    h = (idx * 0x9E3779B1 + seed) & 0xffffffff
    h = h ^ (h >> 15)
    h = (h * 0x85EBCA6B) & 0xffffffff
    h = h ^ (h >> 13)
    return (((h & 255) < dens).to(torch.int64) * (((h >> 8) & 1) * 2 - 1)).to(torch.float32)


def fill_x(c, device):
    """the whole input [B][H][W][Cin] on `device`, filled in chunks of 2^26 elements"""
    n = c.B * c.H * c.W * c.Cin
    x = torch.empty(n, dtype=torch.float32, device=device)
    for a in range(0, n, 1 << 26):
        b = min(a + (1 << 26), n)
        x[a:b] = xval(torch.arange(a, b, dtype=torch.int64, device=device), c.seed, c.xdens)
    return x.view(c.B, c.H, c.W, c.Cin)


def _x_at(c, b, yy, xx):
    """x[b, yy, xx, :] in float64 for index tensors of one shape -> [..., Cin]"""
    pix = (b * c.H + yy) * c.W + xx
    return xval(pix[..., None] * c.Cin + torch.arange(c.Cin), c.seed, c.xdens).to(F64)


def _case(name, layer, B, H, W, Cin, Cout, seed, **kw):
    c = dict(name=name, layer=layer, B=B, H=H, W=W, Cin=Cin, Cout=Cout, seed=seed, xdens=64, nsamples=256)
    c.update(kw)
    return types.SimpleNamespace(**c)


# (H, W: the layer's INPUT map; the decoder's dy is [B][2H][2W][32])
CASES = [
    # UpsampleConvLayer(64, 32): dy = [2][2048][2048][32] is 2^30 bytes — the one-launch folded backward-weights kernel (twice the bytes
    # below WOOB) and the PARITY4 backward-data launch (below 2^30) both cannot address it; one row of dy pairs short both can
    _case("decoder_at", "decoder", 2, 1024, 1024, 64, 32, 11),
    _case("decoder_below", "decoder", 2, 1023, 1024, 64, 32, 12),
    # ResidualBlock(64, 64), wgrad_winograd_2x4 = "force": at [2][2048][2048][64] the whole tensor reaches 2^31 bytes
    _case("resblock_at", "resblock", 2, 2048, 2048, 64, 64, 13, xdens=48, nsamples=96),
    _case("resblock_below", "resblock", 2, 2047, 2048, 64, 64, 14, xdens=48, nsamples=96),
]
CASES += [
    # ConvLayer(64, 64, 3): ONE image of [1][2048][4096][64] reaches 2^31 bytes — beyond the per-image offsets of the Winograd forward and
    # backward-data kernels (and the whole-tensor ones of their backward-weights): the direct kernel takes all three launches
    _case("conv_at", "conv", 1, 2048, 4096, 64, 64, 15, xdens=48, nsamples=96),
    _case("conv_below", "conv", 1, 2047, 4096, 64, 64, 16, xdens=48, nsamples=96),
]
BY_NAME = {c.name: c for c in CASES}


def out_map(c):
    return (2 * c.H, 2 * c.W) if c.layer == "decoder" else (c.H, c.W)


def samples(c):
    """[K][3] (image, row, column) of the output pixels where dy is non-zero, and dy there [K][Cout] (integers in -2..2)"""
    g = torch.Generator().manual_seed(c.seed)
    Ho, Wo = out_map(c)
    pts = {(b, y, x) for b in (0, c.B - 1) for y in (0, Ho - 1) for x in (0, Wo - 1)}
    for x in torch.randint(0, Wo, (24,), generator=g).tolist():                  # the last rows of the last image, the first of the first
        pts |= {(c.B - 1, Ho - 1, x), (c.B - 1, Ho - 2, x), (0, 0, x)}
    for y in torch.randint(0, Ho, (8,), generator=g).tolist():                   # the first and the last column
        pts |= {(c.B - 1, y, Wo - 1), (0, y, 0)}
    while len(pts) < c.nsamples:
        pts.add((int(torch.randint(0, c.B, (1,), generator=g)), int(torch.randint(0, Ho, (1,), generator=g)), int(torch.randint(0, Wo, (1,), generator=g))))
    S = torch.tensor(sorted(pts), dtype=torch.int64)
    dyv = torch.randint(-2, 3, (S.shape[0], c.Cout), generator=g).to(F64)
    return S, dyv


def weights(c):
    """the layer's parameters (OIHW float64 integers): the decoder's 9 x {-1, 0, 1} (the 9 clears the thirds of the folded Winograd
    transforms), the block's 48 x {-1, 0, 1} (G g G^T of F(2x2,3x3) and F(2x4,3x3) integral); biases in -8..8"""
    g = torch.Generator().manual_seed(c.seed + 1000)

    def w(shape, scale, dens):
        return scale * torch.randint(-1, 2, shape, generator=g).to(F64) * (torch.rand(shape, generator=g) < dens).to(F64)

    def b(n):
        return torch.randint(-8, 9, (n,), generator=g).to(F64)
    if c.layer == "decoder":
        return dict(w=w((c.Cout, c.Cin, 5, 5), 9.0, 0.125), b=b(c.Cout))
    if c.layer == "conv":
        return dict(w=w((c.Cout, c.Cin, 3, 3), 48.0, 0.04), b=b(c.Cout))
    return dict(w1=w((c.Cout, c.Cin, 3, 3), 48.0, 0.04), b1=b(c.Cout), w2=w((c.Cout, c.Cout, 3, 3), 48.0, 0.01), b2=b(c.Cout))


def _window(c, S, half, Hm, Wm):
    """(rows [K][n][n], columns, inside-the-map mask) of the (2 half + 1)^2 window around every sample on an Hm x Wm map"""
    k = torch.arange(2 * half + 1) - half
    r = (S[:, 1, None, None] + k[None, :, None]).expand(-1, -1, k.numel())
    s = (S[:, 2, None, None] + k[None, None, :]).expand(-1, k.numel(), -1)
    return r, s, (r >= 0) & (r < Hm) & (s >= 0) & (s < Wm)


def _scatter(pix, val):
    """sum the rows `val` [N][C] by pixel index `pix` [N] -> (unique pixels, their sums)"""
    u, inv = torch.unique(pix, return_inverse=True)
    out = torch.zeros(u.numel(), val.shape[1], dtype=F64)
    out.index_add_(0, inv, val)
    return u, out


def _up2x_coord(d, n):
    """F.interpolate(scale_factor=2, bilinear, align_corners=False): source index pair and the weight of the second one"""
    sf = (0.5 * d.to(F64) - 0.25).clamp_min(0.0)
    i0 = sf.floor().to(torch.int64)
    return i0, i0 + (i0 < n - 1).to(torch.int64), sf - i0.to(F64)


def reference(c):
    """float64: dw / db of every parameter, dx as (flat input pixel indices, [P][Cin] values; zero elsewhere), and the statements on
    absolute values (`top`: the largest of them)"""
    S, dyv = samples(c)
    P = weights(c)
    bidx = S[:, 0, None, None]
    if c.layer == "decoder":
        H2, W2 = out_map(c)
        r, s, ok = _window(c, S, 2, H2, W2)
        rc, sc = r.clamp(0, H2 - 1), s.clamp(0, W2 - 1)
        y0, y1, ly = _up2x_coord(rc, c.H)
        x0, x1, lx = _up2x_coord(sc, c.W)
        corners = [(y0, x0, (1 - ly) * (1 - lx)), (y0, x1, (1 - ly) * lx), (y1, x0, ly * (1 - lx)), (y1, x1, ly * lx)]
        okf = ok.to(F64)
        U = sum((wt * okf)[..., None] * _x_at(c, bidx, yy, xx) for yy, xx, wt in corners)            # [K][5][5][Cin]: the upsampled patch
        pre = torch.einsum("kijc,ocij->ko", U, P["w"]) + P["b"]
        g = dyv * (pre > 0).to(F64)
        out = dict(grads={"conv2d.weight": torch.einsum("kijc,ko->ocij", U, g), "conv2d.bias": g.sum(0)})
        dU = torch.einsum("ocij,ko->kijc", P["w"], g)
        pix = torch.cat([((bidx * c.H + yy) * c.W + xx).reshape(-1) for yy, xx, _ in corners])
        val = torch.cat([((wt * okf)[..., None] * dU).reshape(-1, c.Cin) for _, _, wt in corners])
        out["dx_pix"], out["dx"] = _scatter(pix, val)
        out["top"] = max(float((torch.einsum("kijc,ocij->ko", U.abs(), P["w"].abs()) + P["b"].abs()).max()),
                         float(torch.einsum("kijc,ko->ocij", U.abs(), g.abs()).max()), float(g.abs().sum(0).max()),
                         float(_scatter(pix, val.abs())[1].max()))
        return types.SimpleNamespace(S=S, dyv=dyv, **out)
    if c.layer == "conv":           # y = relu(conv3x3(x) + b)
        r, s, ok = _window(c, S, 1, c.H, c.W)
        xw = _x_at(c, bidx, r.clamp(0, c.H - 1), s.clamp(0, c.W - 1)) * ok.to(F64)[..., None]
        pre = torch.einsum("kijc,ocij->ko", xw, P["w"]) + P["b"]
        g = dyv * (pre > 0).to(F64)
        dxw = torch.einsum("ocij,ko->kijc", P["w"], g)
        keep = ok.reshape(-1)
        pix = ((bidx * c.H + r) * c.W + s).reshape(-1)[keep]
        dx_pix, dx = _scatter(pix, dxw.reshape(-1, c.Cin)[keep])
        top = max(float((torch.einsum("kijc,ocij->ko", xw.abs(), P["w"].abs()) + P["b"].abs()).max()), float(torch.einsum("kijc,ko->ocij", xw.abs(), g.abs()).max()),
                  float(g.abs().sum(0).max()), float(_scatter(pix, torch.einsum("ocij,ko->kijc", P["w"].abs(), g.abs()).reshape(-1, c.Cin)[keep])[1].max()))
        grads = {"conv2d.weight": torch.einsum("kijc,ko->ocij", xw, g), "conv2d.bias": g.sum(0)}
        return types.SimpleNamespace(S=S, dyv=dyv, grads=grads, dx_pix=dx_pix, dx=dx, top=top)
    # ---- residual block: y = relu(conv2(t) + b2 + x), t = relu(conv1(x) + b1)
    r, s, ok = _window(c, S, 2, c.H, c.W)
    xw = _x_at(c, bidx, r.clamp(0, c.H - 1), s.clamp(0, c.W - 1)) * ok.to(F64)[..., None]          # [K][5][5][C], zero padding
    inner = ok[:, 1:4, 1:4].to(F64)                                                                # is t's pixel inside the map?
    K = S.shape[0]
    t, tabs = torch.zeros(K, 3, 3, c.Cout, dtype=F64), torch.zeros(K, 3, 3, c.Cout, dtype=F64)
    for a in range(3):
        for b in range(3):
            t[:, a, b] = torch.relu(torch.einsum("kijc,ocij->ko", xw[:, a:a + 3, b:b + 3], P["w1"]) + P["b1"]) * inner[:, a, b, None]
            tabs[:, a, b] = torch.einsum("kijc,ocij->ko", xw[:, a:a + 3, b:b + 3].abs(), P["w1"].abs()) + P["b1"].abs()
    pre = torch.einsum("kijc,ocij->ko", t, P["w2"]) + P["b2"] + xw[:, 2, 2]
    dpre = dyv * (pre > 0).to(F64)
    dt = torch.einsum("ocij,ko->kijc", P["w2"], dpre)
    d1 = dt * (t > 0).to(F64)
    dw1, dxw = torch.zeros_like(P["w1"]), torch.zeros_like(xw)
    dw1a, dxa = torch.zeros_like(P["w1"]), torch.zeros_like(xw)
    for a in range(3):
        for b in range(3):
            dw1 += torch.einsum("kijc,ko->ocij", xw[:, a:a + 3, b:b + 3], d1[:, a, b])
            dw1a += torch.einsum("kijc,ko->ocij", xw[:, a:a + 3, b:b + 3].abs(), d1[:, a, b].abs())
            dxw[:, a:a + 3, b:b + 3] += torch.einsum("ocij,ko->kijc", P["w1"], d1[:, a, b])
            dxa[:, a:a + 3, b:b + 3] += torch.einsum("ocij,ko->kijc", P["w1"].abs(), d1[:, a, b].abs())
    dxw[:, 2, 2] += dpre
    dxa[:, 2, 2] += dpre.abs()
    keep = ok.reshape(-1)
    pix = ((bidx * c.H + r) * c.W + s).reshape(-1)[keep]
    dx_pix, dx = _scatter(pix, dxw.reshape(-1, c.Cin)[keep])
    top = max(float(tabs.max()), float((torch.einsum("kijc,ocij->ko", t.abs(), P["w2"].abs()) + P["b2"].abs() + xw[:, 2, 2].abs()).max()),
              float(torch.einsum("kijc,ko->ocij", t, dpre.abs()).max()), float(dw1a.max()), float(dt.abs().max()),
              float(_scatter(pix, dxa.reshape(-1, c.Cin)[keep])[1].max()), float(d1.abs().sum((0, 1, 2)).max()))
    grads = {"conv1.weight": dw1, "conv1.bias": d1.sum((0, 1, 2)), "conv2.weight": torch.einsum("kijc,ko->ocij", t, dpre), "conv2.bias": dpre.sum(0)}
    return types.SimpleNamespace(S=S, dyv=dyv, grads=grads, dx_pix=dx_pix, dx=dx, top=top)


_REF = {}


def reference_once(c):
    if c.name not in _REF:
        _REF[c.name] = reference(c)
    return _REF[c.name]
