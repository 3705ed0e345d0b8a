"""Float64 statement of `ramnet_augment_scale_batch`, written from the text of include/ramnet_hip.h: the window of `ramnet_augment_batch`
(tests/augment_restatement.py: `exact`, `general`, `normalized`) followed by the bilinear resize of the datasets' scale_factor
(tests/eval_rescale_restatement.py: `resize_bilinear`, the float64 statement of F.interpolate(scale_factor=s, mode='bilinear',
align_corners=False, recompute_scale_factor=False)).  Anchored on the CPU by tests/test_augment_scale_cpu.py.

Tolerance per output value (the entry evaluates coordinates, weights and blend in double and rounds once to fp32):
  exact    2 x 2^-24 |ref|: the one rounding, and one ulp of slack;
  general  the largest of the tolerances augment_restatement assigns to the four window values (its Lipschitz and value-bound rule; the
           blend is a convex combination, so tap errors do not grow) + 2 x 2^-24 |ref|;
  stats    the window values carry the fp32 bound of `normalized`, through the taps in the same way.

Sources are [C][H][W] float64 tensors of fp32 values."""
import numpy as np
import torch

import augment_restatement as ar
from eval_rescale_restatement import resize_bilinear

F64 = torch.float64
U = ar.U


def out_shape(th, tw, s):
    return int(np.floor(th * s)), int(np.floor(tw * s))


def resize(win, s):
    """[C][th][tw] float64 -> [C][oh][ow] float64"""
    return torch.from_numpy(np.stack([resize_bilinear(p.numpy(), s) for p in win]))


def largest_tap(x, s):
    """[C][th][tw] (bounds: >= 0) -> [C][oh][ow]: the largest of the four taps of every output pixel (NaN where one of them is NaN)"""
    Cn, th, tw = x.shape
    oh, ow = out_shape(th, tw, s)
    sy = np.maximum((np.arange(oh) + 0.5) * (1.0 / s) - 0.5, 0.0)
    sx = np.maximum((np.arange(ow) + 0.5) * (1.0 / s) - 0.5, 0.0)
    y0, x0 = np.minimum(sy.astype(np.int64), th - 1), np.minimum(sx.astype(np.int64), tw - 1)
    y1, x1 = y0 + (y0 < th - 1), x0 + (x0 < tw - 1)
    taps = torch.stack([x[:, r][:, :, c] for r in (torch.from_numpy(y0), torch.from_numpy(y1)) for c in (torch.from_numpy(x0), torch.from_numpy(x1))])
    worst = taps.max(dim=0).values
    return torch.where(torch.isnan(taps).any(dim=0), torch.full_like(worst, float("nan")), worst)


def exact(src, H, W, th, tw, top, left, flips, s, value_bound=None):
    """-> (ref, tol) [C][oh][ow]; value_bound [C][H][W]: the bound of every source value (the normalisation's), None: the sources are exact"""
    ref = resize(ar.exact(src, H, W, th, tw, top, left, flips), s)
    tol = 2 * U * ref.abs()
    if value_bound is not None:
        tol = tol + largest_tap(ar.exact(value_bound, H, W, th, tw, top, left, flips), s) * (1.0 + 8 * U)
    return ref, tol


def general(src, theta, bx, by, th, tw, top, left, s, value_bound=None):
    """-> (ref, tol) [C][oh][ow]"""
    val, bound, _ = ar.general(src, theta, bx, by, th, tw, top, left, value_bound)
    ref = resize(val, s)
    return ref, largest_tap(bound, s) + 2 * U * ref.abs()


def check(got, ref, tol, what):
    """got fp32 [..], ref / tol float64: equal NaN masks, |got - ref| <= tol elsewhere; prints the worst ratio before it asserts"""
    ref, tol = ref.reshape(got.shape), tol.reshape(got.shape)
    nan_g, nan_r = torch.isnan(got), torch.isnan(ref)
    fin = ~nan_r & ~nan_g
    err = (got.double() - ref)[fin].abs()
    ratio = float((err / tol[fin].clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s: max |err| %.3e, max err / tol %.3f, NaN %d" % (what, float(err.max()) if err.numel() else 0.0, ratio, int(nan_r.sum())))
    assert torch.equal(nan_g, nan_r), "%s: %d NaN of one side are numbers on the other" % (what, int((nan_g != nan_r).sum()))
    assert bool((err <= tol[fin]).all()), "%s: error %.3f x its tolerance" % (what, ratio)
