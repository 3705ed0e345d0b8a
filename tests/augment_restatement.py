"""Float64 statement of `ramnet_augment_batch`, written from the text of include/ramnet_hip.h and from nothing in csrc/.  Anchored on the CPU
by tests/test_augment_restatement_cpu.py.

  window   output pixel (y, x) is pixel (Y, X) = (y + top, x + left) of the flipped / rotated image;
  exact    the flipped image: src(rows mirrored ? H - 1 - Y : Y, columns mirrored ? W - 1 - X : X), bit for bit;
  general  affine_grid + grid_sample(bilinear, zeros, align_corners=False): x_n = bx[X], y_n = by[Y] (the caller's fp32 tables),
           gx = t00 x_n + t01 y_n + t02, ix = ((gx + 1) W - 1) / 2 (rows likewise), the four taps around (ix, iy), taps outside the image
           skipped, taps inside always multiplied (0 x NaN = NaN);
  stats    every source value v is read as v != 0 ? (v - mean) / std : 0 with the statistics of the full grid; degenerate statistics (no
           non-zero value, a single distinct one) leave the values unchanged;
  layout   [C][th][tw], or [th][tw][Cpad] with zeros in the channels from C on.

Sources are [C][H][W] float64 tensors of fp32 values; theta, bx, by float64 tensors of fp32 values."""
import torch

F64 = torch.float64
U = 2.0 ** -24


def base_coords(n):
    """torch's linspace(-1, 1, n) * (n - 1) / n in fp32, as float64"""
    return ((torch.linspace(-1, 1, n) * (n - 1) / n) if n > 1 else torch.zeros(1)).to(F64)


def nonzero_stats(src):
    g = src.reshape(-1)
    return torch.stack([g.sum(), (g * g).sum(), torch.tensor(float((g != 0).sum()), dtype=F64)])


def normalized(src):
    """-> (the source as the transform reads it, the fp32 error bound of every value; None where nothing is computed)"""
    S1, S2, cnt = nonzero_stats(src)
    nz = src[src != 0]
    if cnt == 0 or bool((nz == nz[0]).all()):
        return src.clone(), None
    mean, ms = S1 / cnt, S2 / cnt
    var = ms - mean * mean
    # mean, mean square and their difference in fp32: the variance carries 4 x 2^-24 (ms + mean^2), the standard deviation half of that
    # relative to the variance + 1 rounding; (v - mean) / sd: the rounded mean, the difference, the quotient
    assert float(var) >= 0.1 * float(ms), "the case cancels too much for a derived bound"
    sd = torch.sqrt(var)
    out = torch.where(src != 0, (src - mean) / sd, torch.zeros_like(src))
    esd = 0.5 * 4 * U * (ms + mean * mean) / var + 2 * U
    bound = torch.where(src != 0, (U * mean.abs() + U * (src - mean).abs()) / sd + out.abs() * (esd + 2 * U), torch.zeros_like(src))
    return out, bound


def window_coords(H, W, th, tw, top, left):
    Y = torch.arange(th)[:, None].expand(th, tw) + top
    X = torch.arange(tw)[None, :].expand(th, tw) + left
    return Y, X


def exact(src, H, W, th, tw, top, left, flips):
    Y, X = window_coords(H, W, th, tw, top, left)
    return src[:, (H - 1 - Y) if flips & 2 else Y, (W - 1 - X) if flips & 1 else X]


def sample_points(theta, bx, by, H, W, th, tw, top, left):
    """-> (ix, iy, dix, diy) [th][tw]: the float64 sample point and the fp32 error bound of each coordinate.
    gx: each of the three terms passes at most 3 roundings (its product, two adds; a contracted multiply-add rounds less): 3 u A with
    A = |t00 x_n| + |t01 y_n| + |t02|, which ix sees times W / 2; then gx + 1, the product with W, the - 1 (the halving is exact)."""
    Y, X = window_coords(H, W, th, tw, top, left)
    xn, yn = bx[X], by[Y]
    out = []
    for (a, b, c), n in ((theta[0:3], W), (theta[3:6], H)):
        g = a * xn + b * yn + c
        A = (a * xn).abs() + (b * yn).abs() + abs(c)
        i = ((g + 1.0) * n - 1.0) / 2.0
        d = 0.5 * U * (3.0 * A * n + 2.0 * (g + 1.0).abs() * n + ((g + 1.0) * n - 1.0).abs()) * (1.0 + 2.0 ** -20)
        out.append((i, d))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def _at(src, r, c):
    """src [C][H][W] at integer rows r, columns c [th][tw], 0 outside (and whether inside)"""
    Cn, H, W = src.shape
    inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)
    v = src[:, r.clamp(0, H - 1), c.clamp(0, W - 1)]
    return torch.where(inside[None], v, torch.zeros_like(v)), inside


def bilinear(src, ix, iy, value_bound=None):
    """-> (value [C][th][tw], the fp32 rounding bound of the four products and three adds on absolute values)
    Rounding count per tap term: the weights wx, wy are exact or carry one rounding of a number <= 1 (2^-24 absolute each), their product
    one, the product with the value one, the adds three."""
    x0, y0 = torch.floor(ix), torch.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    x0, y0 = x0.clamp(-4, 2.0 ** 30).long(), y0.clamp(-4, 2.0 ** 30).long()
    val, rnd = 0.0, 0.0
    for dy, wy in ((0, wy0), (1, wy1)):
        for dx, wx in ((0, wx0), (1, wx1)):
            v, inside = _at(src, y0 + dy, x0 + dx)
            val = val + v * (wx * wy)                  # NaN inside the image: 0 x NaN = NaN; outside: the tap is skipped
            a = torch.nan_to_num(v.abs(), nan=0.0)
            rnd = rnd + 5.0 * U * a * (wx * wy) + U * a * (wx + wy)
            if value_bound is not None:
                rnd = rnd + _at(value_bound, y0 + dy, x0 + dx)[0] * (wx * wy) * (1.0 + 8 * U)
    return val, rnd


def lipschitz(src, ix, iy):
    """-> (Lx, Ly) [C][th][tw]: the largest difference between horizontal (vertical) neighbours of the zero-padded source around the sample
    point: rows y0 - 1 .. y0 + 2, column steps x0 - 1 .. x0 + 2 (the cell of the point and the eight around it)"""
    x0, y0 = torch.floor(ix).clamp(-4, 2.0 ** 30).long(), torch.floor(iy).clamp(-4, 2.0 ** 30).long()
    Lx = Ly = 0.0
    for a in range(-1, 3):
        for b in range(-1, 2):
            Lx = torch.maximum((_at(src, y0 + a, x0 + b + 1)[0] - _at(src, y0 + a, x0 + b)[0]).abs(), torch.as_tensor(Lx, dtype=F64))
            Ly = torch.maximum((_at(src, y0 + b + 1, x0 + a)[0] - _at(src, y0 + b, x0 + a)[0]).abs(), torch.as_tensor(Ly, dtype=F64))
    return Lx, Ly


def general(src, theta, bx, by, th, tw, top, left, value_bound=None):
    """-> (value, bound, near) [C][th][tw]: bound = coordinate error x the largest neighbouring difference, per axis, + the roundings (NaN
    where the neighbourhood holds a NaN); near [th][tw]: a coordinate lies within its error of an integer (the taps may differ)"""
    Cn, H, W = src.shape
    ix, iy, dix, diy = sample_points(theta, bx, by, H, W, th, tw, top, left)
    val, rnd = bilinear(src, ix, iy, value_bound)
    Lx, Ly = lipschitz(src, ix, iy)
    bound = (dix * Lx + diy * Ly) * 1.001 + rnd
    near = ((ix - torch.round(ix)).abs() <= dix) | ((iy - torch.round(iy)).abs() <= diy)
    return val, bound, near


def to_layout(out, nhwc, Cpad):
    """[C][th][tw] -> the destination as a flat tensor"""
    if not nhwc:
        return out.reshape(-1)
    Cn, th, tw = out.shape
    full = torch.zeros(th, tw, Cpad, dtype=out.dtype)
    full[:, :, :Cn] = out.permute(1, 2, 0)
    return full.reshape(-1)


def clamp_window(top, left, H, W, th, tw):
    return min(max(top, 0), H - th), min(max(left, 0), W - tw)
