// Training augmentation on the device (utils/data_augmentation.py: RandomRotationFlip + RandomCrop / CenterCrop, train.py:149-150):
// G tensors [C][H][W] -> G windows [C][th][tw] (NCHW) or [th][tw][Cpad] (the model's NHWC input), one launch for all of them.
// The tensors are separate allocations: a device table holds their source / destination pointers, a parameter-index array maps tensor g
// to its parameter set (one per sample: 2x3 theta, window top / left, host-decided exact flag and flip bits).
//
// exact   (theta = diag(+-1, +-1), no translation — angle 0): out(y, x) = src(vflip ? H-1-Y : Y, hflip ? W-1-X : X), Y = y + top,
//         X = x + left; values are copied bit for bit (NaN included), no interpolation arithmetic.
// general affine_grid(align_corners=False) + grid_sample(bilinear, zeros, align_corners=False) in fp32: x_n = bx[X], y_n = by[Y] (the
//         caller's tables, torch's own linspace(-1, 1, n) (n - 1) / n), gx = t00 x_n + t01 y_n + t02, ix = ((gx + 1) W - 1) / 2; four
//         taps, taps outside the image skipped, taps inside always multiplied (0 x NaN = NaN).
// stats   optional [G][3] doubles (sum, sum of squares, nonzero count: nonzero_stats_batch_kernel): every SOURCE value v becomes
//         v != 0 ? (v - mean) / sd : 0 — the expression of normalize_nonzero_batch_kernel — before it is copied or interpolated.
//
// HBM-bound gather.  NCHW exact path: one thread per 4 output pixels, a 16-byte store and ONE 16-byte load of the 4 source pixels (reversed
// in registers for a horizontal flip), so that a wave reads its row segments in 1 KiB runs in either direction; only the window is read.
#include "common.hpp"

namespace ramnet {

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));      // 16-byte load from a 4-byte aligned address (W = 346: rows are not 16-byte aligned)
typedef float f4a __attribute__((ext_vector_type(4)));
// Pointers that come out of a device table carry no address space; declared global they load / store with global_* instructions, and an
// under-aligned 16-byte load stays ONE instruction (a flat one is taken apart: it might point into scratch).
typedef const float __attribute__((address_space(1))) *gsrc_t;
typedef float __attribute__((address_space(1))) *gdst_t;

struct aug_norm {
    int on;
    float mean, sd;
};

// The variance is formed as in normalize_nonzero_batch_kernel, product and difference each rounded: a fused ms - mean * mean leaves the
// rounding error of mean^2 behind as the "variance" of a grid with a single distinct nonzero value (0.2f: positive), and such a grid
// would be normalised to zeros here while the stand-alone kernel leaves it unchanged.
__device__ __forceinline__ aug_norm aug_norm_of(const double *stats, int g) {
#pragma clang fp contract(off)
    aug_norm n = {0, 0.f, 1.f};
    if (stats == nullptr) return n;
    const double cnt = stats[3 * g + 2];
    if (cnt == 0.0) return n;
    n.mean = (float)(stats[3 * g] / cnt);
    n.sd = sqrtf((float)(stats[3 * g + 1] / cnt) - n.mean * n.mean);
    n.on = n.sd > 0.f;
    return n;
}

__device__ __forceinline__ float aug_val(float v, const aug_norm &n) { return n.on ? (v != 0.f ? (v - n.mean) / n.sd : 0.f) : v; }

// bilinear sample of one plane at (ix, iy) (grid_sample: zeros padding, align_corners=False already folded into ix / iy)
__device__ __forceinline__ float aug_bilinear(gsrc_t plane, int H, int W, float ix, float iy, const aug_norm &n) {
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float wx1 = ix - fx, wy1 = iy - fy, wx0 = (fx + 1.f) - ix, wy0 = (fy + 1.f) - iy;
    float acc = 0.f;
    const bool xa = x0 >= 0 && x0 < W, xb = x0 + 1 >= 0 && x0 + 1 < W, ya = y0 >= 0 && y0 < H, yb = y0 + 1 >= 0 && y0 + 1 < H;
    if (ya && xa) acc += aug_val(plane[(size_t)y0 * W + x0], n) * (wx0 * wy0);
    if (ya && xb) acc += aug_val(plane[(size_t)y0 * W + x0 + 1], n) * (wx1 * wy0);
    if (yb && xa) acc += aug_val(plane[(size_t)(y0 + 1) * W + x0], n) * (wx0 * wy1);
    if (yb && xb) acc += aug_val(plane[(size_t)(y0 + 1) * W + x0 + 1], n) * (wx1 * wy1);
    return acc;
}

struct aug_params {
    float t[6];
    int top, left, exact, hflip, vflip;
};

// win = [P][4] int32: top, left, exact, flips (bit 0: columns mirrored, bit 1: rows mirrored).  top / left are clamped into the image here
// as well (the host checks them wherever it has them): a table that was overwritten must not turn into a read outside the source.
__device__ __forceinline__ aug_params aug_load(const float *__restrict__ theta, const int *__restrict__ win, int p, int H, int W, int th, int tw) {
    aug_params a;
#pragma unroll
    for (int i = 0; i < 6; ++i) a.t[i] = theta[6 * p + i];
    a.top = min(max(win[4 * p + 0], 0), H - th);
    a.left = min(max(win[4 * p + 1], 0), W - tw);
    a.exact = win[4 * p + 2] != 0;
    a.hflip = win[4 * p + 3] & 1, a.vflip = (win[4 * p + 3] >> 1) & 1;
    return a;
}

// blockIdx.y = tensor.  VEC: NCHW, exact, tw % 4 == 0 and a 16-byte aligned destination are decided per tensor (uniform per workgroup);
// everything else takes the per-pixel path below.
template <bool NHWC>
__global__ void __launch_bounds__(256) augment_kernel(const float *const *__restrict__ srcs, float *const *__restrict__ dsts, const int *__restrict__ pidx,
                                                      const float *__restrict__ theta, const int *__restrict__ win, const double *__restrict__ stats,
                                                      const float *__restrict__ bx, const float *__restrict__ by, int n_params, int C, int H, int W,
                                                      int th, int tw, int Cpad) {
    const int g = blockIdx.y;
    int p = pidx ? pidx[g] : g;
    p = min(max(p, 0), n_params - 1);
    const gsrc_t src = (gsrc_t)srcs[g];
    const gdst_t dst = (gdst_t)dsts[g];
    const aug_params a = aug_load(theta, win, p, H, W, th, tw);
    const aug_norm nrm = aug_norm_of(stats, g);
    const size_t plane = (size_t)H * W;
    const unsigned stride = gridDim.x * blockDim.x, first = blockIdx.x * blockDim.x + threadIdx.x;

    if (!NHWC && a.exact && (tw & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const unsigned tw4 = tw >> 2, total = (unsigned)C * th * tw4;
        for (unsigned i = first; i < total; i += stride) {
            const unsigned r = i / tw4, x4 = i - r * tw4;        // r = c * th + y
            const unsigned c = r / th, y = r - c * th;
            const int Y = (int)y + a.top, X = (int)(x4 * 4) + a.left;
            const int sy = a.vflip ? H - 1 - Y : Y, sx = a.hflip ? W - 4 - X : X;       // the 4 source pixels are columns sx .. sx + 3 either way
            const f4u q = *(const f4u __attribute__((address_space(1))) *)(src + c * plane + (size_t)sy * W + sx);
            float4 v;
            if (a.hflip) v = make_float4(q.w, q.z, q.y, q.x);
            else v = make_float4(q.x, q.y, q.z, q.w);
            v.x = aug_val(v.x, nrm), v.y = aug_val(v.y, nrm), v.z = aug_val(v.z, nrm), v.w = aug_val(v.w, nrm);
            *(f4a __attribute__((address_space(1))) *)(dst + (size_t)i * 4) = (f4a){v.x, v.y, v.z, v.w};
        }
        return;
    }

    const unsigned npix = (unsigned)th * tw;
    for (unsigned i = first; i < npix; i += stride) {
        const unsigned y = i / tw, x = i - y * tw;
        const int Y = (int)y + a.top, X = (int)x + a.left;
        float ix = 0.f, iy = 0.f;
        size_t off = 0;
        if (a.exact) {
            off = (size_t)(a.vflip ? H - 1 - Y : Y) * W + (a.hflip ? W - 1 - X : X);
        } else {
            const float xn = bx[X], yn = by[Y];
            const float gx = a.t[0] * xn + a.t[1] * yn + a.t[2], gy = a.t[3] * xn + a.t[4] * yn + a.t[5];
            ix = ((gx + 1.f) * W - 1.f) / 2.f, iy = ((gy + 1.f) * H - 1.f) / 2.f;
        }
        if (NHWC) {
            const gdst_t out = dst + (size_t)i * Cpad;
            for (int c = 0; c < Cpad; c += 4) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[j] = 0.f;
                    if (c + j < C) v[j] = a.exact ? aug_val(src[(c + j) * plane + off], nrm) : aug_bilinear(src + (c + j) * plane, H, W, ix, iy, nrm);
                }
                *(f4a __attribute__((address_space(1))) *)(out + c) = (f4a){v[0], v[1], v[2], v[3]};
            }
        } else {
            for (int c = 0; c < C; ++c)
                dst[(size_t)c * npix + i] = a.exact ? aug_val(src[c * plane + off], nrm) : aug_bilinear(src + c * plane, H, W, ix, iy, nrm);
        }
    }
}

// ---- the window, then the datasets' scale_factor resize (dataset.py:127-140: F.interpolate(scale_factor = s, mode = 'bilinear',
// align_corners = False, recompute_scale_factor = False) AFTER the flip and crop), in one launch: th x tw window -> oh x ow output,
// oh = floor(th s), ow = floor(tw s), 0 < s < 1.  The four taps of an output pixel are WINDOW values — fp32, exactly what augment_kernel
// would have written there (aug_val of a direct load, or aug_bilinear) — and source coordinate, weights and blend are evaluated in double
// without contraction and rounded once (the rule of resize_metric_target_kernel): src = max((dst + 0.5) (1 / s) - 0.5, 0) from the GIVEN
// factor, i0 = min(int(src), n - 1), i1 = i0 + (i0 < n - 1).  All four taps are always multiplied: a NaN tap gives NaN at weight zero too.
// Only the window is read, only the scaled output is written; no LDS, no atomics: the same bits on every launch.
struct aug_axis {
    int i0, i1;
    double l;
};

__device__ __forceinline__ aug_axis aug_scale_axis(unsigned d, int n, double rs) {
#pragma clang fp contract(off)
    aug_axis a;
    const double s = fmax(((double)d + 0.5) * rs - 0.5, 0.0);
    a.i0 = min((int)s, n - 1);
    a.i1 = a.i0 + (a.i0 < n - 1);
    a.l = s - (double)a.i0;
    return a;
}

__device__ __forceinline__ float aug_scale_blend(float a, float b, float c, float d, double lx, double ly) {
#pragma clang fp contract(off)
    return (float)((1.0 - ly) * ((1.0 - lx) * (double)a + lx * (double)b) + ly * ((1.0 - lx) * (double)c + lx * (double)d));
}

// where window pixel (wy, wx) is read: the source offset (exact) or the sample point (general), the expressions of augment_kernel
struct aug_tap {
    size_t off;
    float ix, iy;
};

template <bool EXACT>
__device__ __forceinline__ aug_tap aug_scale_tap(const aug_params &a, const float *__restrict__ bx, const float *__restrict__ by, int wy, int wx, int H,
                                                 int W) {
    const int Y = wy + a.top, X = wx + a.left;
    aug_tap t = {0, 0.f, 0.f};
    if (EXACT) {
        t.off = (size_t)(a.vflip ? H - 1 - Y : Y) * W + (a.hflip ? W - 1 - X : X);
    } else {
        const float xn = bx[X], yn = by[Y];
        const float gx = a.t[0] * xn + a.t[1] * yn + a.t[2], gy = a.t[3] * xn + a.t[4] * yn + a.t[5];
        t.ix = ((gx + 1.f) * W - 1.f) / 2.f, t.iy = ((gy + 1.f) * H - 1.f) / 2.f;
    }
    return t;
}

// one output pixel of one channel plane: the four window values and their blend
template <bool EXACT>
__device__ __forceinline__ float aug_scale_val(gsrc_t pl, const aug_tap (&t)[4], int H, int W, const aug_norm &n, double lx, double ly) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = EXACT ? aug_val(pl[t[k].off], n) : aug_bilinear(pl, H, W, t[k].ix, t[k].iy, n);
    return aug_scale_blend(v[0], v[1], v[2], v[3], lx, ly);
}

// output pixel i of every channel.  The general mode (16 source loads per value) goes one channel at a time, in the NHWC layout with 4-byte
// stores, so that the registers of the kernel stay those of the exact mode (four channels x four taps unrolled: 208 VGPRs, 2 waves per SIMD).
template <bool NHWC, bool EXACT>
__device__ __forceinline__ void aug_scale_pixel(gsrc_t src, gdst_t dst, const aug_params &a, const aug_norm &nrm, const float *__restrict__ bx,
                                                const float *__restrict__ by, unsigned i, unsigned npix, int C, int H, int W, int th, int tw, int ow,
                                                double rs, int Cpad) {
    const size_t plane = (size_t)H * W;
    const unsigned y = i / ow, x = i - y * ow;
    const aug_axis ay = aug_scale_axis(y, th, rs), ax = aug_scale_axis(x, tw, rs);
    const aug_tap t[4] = {aug_scale_tap<EXACT>(a, bx, by, ay.i0, ax.i0, H, W), aug_scale_tap<EXACT>(a, bx, by, ay.i0, ax.i1, H, W),
                          aug_scale_tap<EXACT>(a, bx, by, ay.i1, ax.i0, H, W), aug_scale_tap<EXACT>(a, bx, by, ay.i1, ax.i1, H, W)};
    if (NHWC && !EXACT) {
        const gdst_t out = dst + (size_t)i * Cpad;
#pragma unroll 1
        for (int c = 0; c < Cpad; ++c) out[c] = c < C ? aug_scale_val<EXACT>(src + c * plane, t, H, W, nrm, ax.l, ay.l) : 0.f;
    } else if (NHWC) {
        const gdst_t out = dst + (size_t)i * Cpad;
        for (int c = 0; c < Cpad; c += 4) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = c + j < C ? aug_scale_val<EXACT>(src + (c + j) * plane, t, H, W, nrm, ax.l, ay.l) : 0.f;
            *(f4a __attribute__((address_space(1))) *)(out + c) = (f4a){v[0], v[1], v[2], v[3]};
        }
    } else {
#pragma unroll 1
        for (int c = 0; c < C; ++c) dst[(size_t)c * npix + i] = aug_scale_val<EXACT>(src + c * plane, t, H, W, nrm, ax.l, ay.l);
    }
}

// blockIdx.y = tensor.  HALF: NCHW, exact, s = 0.5 (1 / s == 2: window rows 2y, 2y + 1 and columns 2x, 2x + 1 at weights 0.5), ow % 4 == 0 and
// a 16-byte aligned destination, decided per tensor (uniform per workgroup): one thread per 4 output pixels = 2 rows x 8 columns of the
// window in four under-aligned 16-byte loads (reversed in registers for a horizontal flip, rows mirrored for a vertical one) and one
// 16-byte store, through the same blend as the per-pixel path below: the same bits.
template <bool NHWC>
__global__ void __launch_bounds__(256) augment_scale_kernel(const float *const *__restrict__ srcs, float *const *__restrict__ dsts, const int *__restrict__ pidx,
                                                            const float *__restrict__ theta, const int *__restrict__ win, const double *__restrict__ stats,
                                                            const float *__restrict__ bx, const float *__restrict__ by, int n_params, int C, int H, int W,
                                                            int th, int tw, int oh, int ow, double rs, int Cpad) {
    const int g = blockIdx.y;
    int p = pidx ? pidx[g] : g;
    p = min(max(p, 0), n_params - 1);
    const gsrc_t src = (gsrc_t)srcs[g];
    const gdst_t dst = (gdst_t)dsts[g];
    const aug_params a = aug_load(theta, win, p, H, W, th, tw);
    const aug_norm nrm = aug_norm_of(stats, g);
    const size_t plane = (size_t)H * W;
    const unsigned stride = gridDim.x * blockDim.x, first = blockIdx.x * blockDim.x + threadIdx.x;

    if (!NHWC && a.exact && rs == 2.0 && (ow & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const unsigned ow4 = ow >> 2, total = (unsigned)C * oh * ow4;
        for (unsigned i = first; i < total; i += stride) {
            const unsigned r = i / ow4, x4 = i - r * ow4;        // r = c * oh + y
            const unsigned c = r / oh, y = r - c * oh;
            const int Y = (int)(y * 2) + a.top, X = (int)(x4 * 8) + a.left;
            const int r0 = a.vflip ? H - 1 - Y : Y, r1 = a.vflip ? r0 - 1 : r0 + 1;
            const int sx = a.hflip ? W - 8 - X : X;               // the 8 source pixels are columns sx .. sx + 7 either way
            const gsrc_t p0 = src + c * plane + (size_t)r0 * W + sx, p1 = src + c * plane + (size_t)r1 * W + sx;
            const f4u q00 = *(const f4u __attribute__((address_space(1))) *)p0, q01 = *(const f4u __attribute__((address_space(1))) *)(p0 + 4);
            const f4u q10 = *(const f4u __attribute__((address_space(1))) *)p1, q11 = *(const f4u __attribute__((address_space(1))) *)(p1 + 4);
            float u[8], l[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                u[j] = a.hflip ? q01[3 - j] : q00[j], u[4 + j] = a.hflip ? q00[3 - j] : q01[j];
                l[j] = a.hflip ? q11[3 - j] : q10[j], l[4 + j] = a.hflip ? q10[3 - j] : q11[j];
            }
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                v[j] = aug_scale_blend(aug_val(u[2 * j], nrm), aug_val(u[2 * j + 1], nrm), aug_val(l[2 * j], nrm), aug_val(l[2 * j + 1], nrm), 0.5, 0.5);
            *(f4a __attribute__((address_space(1))) *)(dst + (size_t)i * 4) = (f4a){v[0], v[1], v[2], v[3]};
        }
        return;
    }

    const unsigned npix = (unsigned)oh * ow;
    if (a.exact)
        for (unsigned i = first; i < npix; i += stride) aug_scale_pixel<NHWC, true>(src, dst, a, nrm, bx, by, i, npix, C, H, W, th, tw, ow, rs, Cpad);
    else
        for (unsigned i = first; i < npix; i += stride) aug_scale_pixel<NHWC, false>(src, dst, a, nrm, bx, by, i, npix, C, H, W, th, tw, ow, rs, Cpad);
}

}  // namespace ramnet

using namespace ramnet;

/* win_host: optional HOST copy of `win` ([n_params][4]); when given, every window is checked against the image before any HIP call. */
extern "C" int ramnet_augment_batch(const float *const *src, float *const *dst, const int *pidx, const float *theta, const int *win,
                                    const int *win_host, const double *stats, const float *bx, const float *by, int G, int n_params, int C,
                                    int H, int W, int th, int tw, int Cpad, int nhwc, void *stream) {
    RAMNET_CHECK_ARG(G >= 0 && G <= 65535 && n_params > 0 && C > 0 && H > 0 && W > 0);
    RAMNET_CHECK_ARG(th > 0 && tw > 0 && th <= H && tw <= W);                       // the window fits the image
    RAMNET_CHECK_ARG(!nhwc || (Cpad >= C && Cpad % 4 == 0));
    RAMNET_CHECK_ARG((size_t)C * H * W < ((size_t)1 << 31) && (size_t)(nhwc ? Cpad : C) * th * tw < ((size_t)1 << 31));
    if (G == 0) return 0;
    RAMNET_CHECK_ARG(src && dst && theta && win && bx && by);
    if (win_host)
        for (int p = 0; p < n_params; ++p) {
            const int top = win_host[4 * p], left = win_host[4 * p + 1];
            RAMNET_CHECK_ARG(top >= 0 && left >= 0 && top + th <= H && left + tw <= W);
        }
    const size_t items = nhwc ? (size_t)th * tw : (size_t)C * th * (tw % 4 == 0 ? tw / 4 : tw);
    int gx = (int)((items + 255) / 256);
    const int cap = (2048 * 4 + G - 1) / G;                                          // ~32 workgroups per CU over the whole launch
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    if (nhwc)
        hipLaunchKernelGGL(augment_kernel<true>, dim3(gx, G), dim3(256), 0, (hipStream_t)stream, src, dst, pidx, theta, win, stats, bx, by, n_params, C,
                           H, W, th, tw, Cpad);
    else
        hipLaunchKernelGGL(augment_kernel<false>, dim3(gx, G), dim3(256), 0, (hipStream_t)stream, src, dst, pidx, theta, win, stats, bx, by, n_params, C,
                           H, W, th, tw, Cpad);
    RAMNET_LAUNCH_CHECK();
    note_kernel(nhwc ? "augment_kernel<nhwc>" : "augment_kernel<nchw>");
    return 0;
}

/* ramnet_augment_batch followed by the datasets' scale_factor resize of every window (th x tw -> oh x ow), in one launch. */
extern "C" int ramnet_augment_scale_batch(const float *const *src, float *const *dst, const int *pidx, const float *theta, const int *win,
                                          const int *win_host, const double *stats, const float *bx, const float *by, int G, int n_params, int C,
                                          int H, int W, int th, int tw, int oh, int ow, double scale_factor, int Cpad, int nhwc, void *stream) {
    RAMNET_CHECK_ARG(G >= 0 && G <= 65535 && n_params > 0 && C > 0 && H > 0 && W > 0);
    RAMNET_CHECK_ARG(th > 0 && tw > 0 && th <= H && tw <= W);                       // the window fits the image
    RAMNET_CHECK_ARG(scale_factor > 0.0 && scale_factor < 1.0);                     // (NaN fails both)
    RAMNET_CHECK_ARG(oh >= 1 && ow >= 1 && oh == (int)floor((double)th * scale_factor) && ow == (int)floor((double)tw * scale_factor));
    RAMNET_CHECK_ARG(!nhwc || (Cpad >= C && Cpad % 4 == 0));
    RAMNET_CHECK_ARG((size_t)C * H * W < ((size_t)1 << 31) && (size_t)(nhwc ? Cpad : C) * oh * ow < ((size_t)1 << 31));
    if (G == 0) return 0;
    RAMNET_CHECK_ARG(src && dst && theta && win && bx && by);
    if (win_host)
        for (int p = 0; p < n_params; ++p) {
            const int top = win_host[4 * p], left = win_host[4 * p + 1];
            RAMNET_CHECK_ARG(top >= 0 && left >= 0 && top + th <= H && left + tw <= W);
        }
    const double rs = 1.0 / scale_factor;
    size_t items = (size_t)oh * ow;                                                  // per-pixel path: one thread per output pixel
    if (!nhwc && rs == 2.0 && ow % 4 == 0 && (size_t)C * oh * (ow / 4) > items) items = (size_t)C * oh * (ow / 4);
    int gx = (int)((items + 255) / 256);
    const int cap = (2048 * 4 + G - 1) / G;                                          // ~32 workgroups per CU over the whole launch
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    if (nhwc)
        hipLaunchKernelGGL(augment_scale_kernel<true>, dim3(gx, G), dim3(256), 0, (hipStream_t)stream, src, dst, pidx, theta, win, stats, bx, by, n_params,
                           C, H, W, th, tw, oh, ow, rs, Cpad);
    else
        hipLaunchKernelGGL(augment_scale_kernel<false>, dim3(gx, G), dim3(256), 0, (hipStream_t)stream, src, dst, pidx, theta, win, stats, bx, by, n_params,
                           C, H, W, th, tw, oh, ow, rs, Cpad);
    RAMNET_LAUNCH_CHECK();
    note_kernel(nhwc ? "augment_scale_kernel<nhwc>" : "augment_scale_kernel<nchw>");
    return 0;
}
