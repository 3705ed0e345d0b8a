// The images RAM_Net/test.py writes for a saved data package (test.py:36-43, 259-360) and its least-squares scale (test.py:365-378), for
// all maps of the package together: uint8 planes in FILE order (RGBA / RGB; make_colormap swaps to BGR only because cv2.imwrite swaps back).
//
// Depth maps, two launches whatever G is.  Per map, as numpy and matplotlib 3.10 compute it on float32 arrays:
//   a = amax(map) (NaN propagates), inv = nan_to_num(a - map, nan=1), b = amax(inv), q = nan_to_num(inv / b)        make_colormap
//   x = float32(float64(q) - vmin), x = float32(float64(x) / (vmax - vmin)), or zeros when vmin == vmax              Normalize.__call__
//   xa = x * 256; xa == 256 -> 255, xa < 0 -> under, xa >= 256 -> over, else truncation; the row of the LUT          Colormap.__call__
// (Normalize keeps vmin / vmax as Python floats and works in place on the float32 array: NumPy 2 evaluates both steps in float64 and rounds
// each to float32.)  A map with a NaN has a = NaN, so inv is the constant 1 and q = 1 everywhere; a map without one has b = a - min(map)
// exactly, because rounding is monotone.  So the first launch only needs min, max and a NaN flag per map: grid = (Ws, cells), workgroup
// (w, c) reduces its part of map c to one row of two doubles {min, max or NaN}, stores it and takes the ticket of the cell; the last arrival
// joins the rows in index order (the join of metrics.hip).  The second launch maps four pixels per thread: 16 bytes in, 4 bytes of grey
// (rint(v * 255), half to even, saturated, NaN -> 0: OpenCV's saturate_cast) and 16 bytes of colour out, the LUT in LDS.
//
// The scale rides in the first launch: cells G .. G + n_scale - 1 are (prediction, target) pairs, the row is {sum p t, sum p p} over the
// unclamped metric depths of et_metric_depth, products rounded to float32, sums in double, the rows of a pair added in index order: the
// same bits on every call.  NaN propagates.
//
// Inputs, one launch: s = the channels added in order in float32 (np.sum(axis=0)); events: R = 255 (s > 0.9), G = 0, B = 255 (s <= -0.5),
// the thresholds being doubles; a frame: rint(s * 255) saturated in all three channels.
//
// Workspace: [64 Ki tickets][cells x 2 doubles of results][cells x Ws rows].  Rows and results are written before they are read in every call
// and the last arrival sets its ticket back to 0: ONE zero-fill of the first RAMNET_RENDER_TICKET_BYTES at allocation is all a caller owes.
#include "common.hpp"
#include "metrics_common.hpp"

namespace ramnet {

constexpr int RD_MAX_PER_MAP = 32;         // workgroups per cell at most
constexpr unsigned RD_SPAN = 8192;         // pixels a workgroup should at least have
constexpr int RD_ROW = 2;                  // doubles of a partial row and of a cell's result
constexpr int RD_LUT = 258;                // 256 colours, under, over
constexpr int RD_MAX_INPUTS = 256;         // inputs of one launch of the input kernel (channel counts and kinds travel as kernel arguments)

typedef unsigned char rd_b4 __attribute__((ext_vector_type(4), aligned(1)));
typedef unsigned rd_u4 __attribute__((ext_vector_type(4), aligned(4)));
typedef const bm_f4u __attribute__((address_space(1))) *rd_v4_t;

struct rd_plan_t {
    int Ws;
    size_t off_stat, off_part, total;
};

static rd_plan_t rd_plan(size_t cells, size_t npix) {
    rd_plan_t p;
    size_t ws = (npix + RD_SPAN - 1) / RD_SPAN;
    if (ws > RD_MAX_PER_MAP) ws = RD_MAX_PER_MAP;
    if (ws < 1) ws = 1;
    p.Ws = (int)ws;
    p.off_stat = RAMNET_RENDER_TICKET_BYTES;
    p.off_part = p.off_stat + ((cells * RD_ROW * sizeof(double) + 255) & ~(size_t)255);
    p.total = p.off_part + cells * p.Ws * RD_ROW * sizeof(double);
    return p;
}

static bool rd_sizes_ok(int G, int n_scale, size_t npix) {
    return G >= 0 && n_scale >= 0 && G <= 65535 && n_scale <= 65535 && G + n_scale >= 1 && G + n_scale <= 65535 && npix > 0 &&
           npix < ((size_t)1 << 31);
}

struct rd_meta_t {
    unsigned short c[RD_MAX_INPUTS];
    unsigned char kind[RD_MAX_INPUTS];
};

// The part of a map that workgroup w of Ws reads: [lo, hi) in pixels, lo a multiple of 4.
__device__ __forceinline__ void rd_range(unsigned npix, int Ws, int w, unsigned &lo, unsigned &hi) {
    const unsigned chunk = ((npix + Ws - 1) / Ws + 3u) & ~3u;
    const unsigned long long a = (unsigned long long)w * chunk;
    lo = a < npix ? (unsigned)a : npix;
    hi = npix - lo < chunk ? npix : lo + chunk;
}

// f(values of the NM maps at one pixel) over the pixels [lo, hi): 16 bytes per lane and map, then the tail of fewer than 4 pixels.
template <int NM, class F>
__device__ __forceinline__ void rd_sweep(const bm_src_t (&src)[NM], unsigned lo, unsigned hi, F f) {
    const unsigned nv = (hi - lo) >> 2;
#pragma unroll 4
    for (unsigned i = threadIdx.x; i < nv; i += BM_T) {
        bm_f4u a[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) a[m] = *(rd_v4_t)(src[m] + lo + 4 * (size_t)i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float x[NM];
#pragma unroll
            for (int m = 0; m < NM; ++m) x[m] = a[m][e];
            f(x);
        }
    }
    for (unsigned k = lo + 4 * nv + threadIdx.x; k < hi; k += BM_T) {
        float x[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) x[m] = src[m][k];
        f(x);
    }
}

// max that keeps a NaN of either side (np.amax); min and sum need no such care here
__device__ __forceinline__ double rd_nanmax(double a, double b) { return (a != a || b != b) ? (double)__uint_as_float(0x7fc00000u) : fmax(a, b); }

__global__ void __launch_bounds__(BM_T) rd_stats_kernel(const float *const *__restrict__ maps, int G, const float *const *__restrict__ spred,
                                                        const float *const *__restrict__ starget, unsigned npix, int Ws, float clip, float reg,
                                                        unsigned *tickets, double *stat, double *part, double *__restrict__ scale) {
    __shared__ double red[RD_ROW][BM_T / 64];
    __shared__ int flag;
    const int w = blockIdx.x, P = Ws;
    const size_t cell = blockIdx.y;
    const bool is_map = cell < (size_t)G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned lo, hi;
    rd_range(npix, Ws, w, lo, hi);
    if (is_map) {
        const bm_src_t src[1] = {(bm_src_t)maps[cell]};
        float mn = __uint_as_float(0x7f800000u), mx = __uint_as_float(0xff800000u), nan = 0.f;
        rd_sweep<1>(src, lo, hi, [&](const float (&x)[1]) {
            mn = fminf(mn, x[0]), mx = fmaxf(mx, x[0]);
            if (x[0] != x[0]) nan = 1.f;
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_down(mn, o)), mx = fmaxf(mx, __shfl_down(mx, o)), nan = fmaxf(nan, __shfl_down(nan, o));
        if (lane == 0) red[0][wave] = (double)mn, red[1][wave] = nan != 0.f ? (double)__uint_as_float(0x7fc00000u) : (double)mx;
    } else {
        const bm_src_t src[2] = {(bm_src_t)spred[cell - G], (bm_src_t)starget[cell - G]};
        double spt = 0.0, spp = 0.0;
        rd_sweep<2>(src, lo, hi, [&](const float (&x)[2]) {
            const float p = et_metric_depth(x[0], reg, clip, 0.f, false), t = et_metric_depth(x[1], reg, clip, 0.f, false);
            spt += (double)(p * t), spp += (double)(p * p);
        });
        spt = bm_wave_sum(spt), spp = bm_wave_sum(spp);
        if (lane == 0) red[0][wave] = spt, red[1][wave] = spp;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r0 = red[0][0], r1 = red[1][0];
        for (int i = 1; i < BM_T / 64; ++i) {
            if (is_map) r0 = fmin(r0, red[0][i]), r1 = rd_nanmax(r1, red[1][i]);
            else r0 += red[0][i], r1 += red[1][i];
        }
        part[(cell * P + w) * RD_ROW] = r0, part[(cell * P + w) * RD_ROW + 1] = r1;
    }
    if (!bm_ticket(cell, P, tickets, &flag)) return;

    // last arrival of the cell: its P <= 32 rows in index order
    if (threadIdx.x == 0) {
        const double *rows = part + cell * P * RD_ROW;
        double r0 = bm_ld(rows), r1 = bm_ld(rows + 1);
        for (int r = 1; r < P; ++r) {
            const double a = bm_ld(rows + r * RD_ROW), b = bm_ld(rows + r * RD_ROW + 1);
            if (is_map) r0 = fmin(r0, a), r1 = rd_nanmax(r1, b);
            else r0 += a, r1 += b;
        }
        stat[cell * RD_ROW] = r0, stat[cell * RD_ROW + 1] = r1;
        if (!is_map) scale[cell - G] = r0 / r1;
        atomicExch(tickets + cell, 0u);                           // ready for the next call
    }
}

// cv::saturate_cast<uchar>(float): round half to even, saturate; NaN -> 0
__device__ __forceinline__ unsigned rd_sat_u8(float y) {
    y = rintf(y);
    return y != y ? 0u : (y < 0.f ? 0u : (y > 255.f ? 255u : (unsigned)y));
}

__global__ void __launch_bounds__(256) rd_map_kernel(const float *const *__restrict__ maps, unsigned npix, double vmin, double vrange,
                                                     const unsigned char *__restrict__ lut, const double *__restrict__ stat,
                                                     unsigned char *__restrict__ grey, unsigned char *__restrict__ color) {
    __shared__ unsigned slut[RD_LUT];
    for (int i = threadIdx.x; i < RD_LUT; i += 256)
        slut[i] = (unsigned)lut[4 * i] | ((unsigned)lut[4 * i + 1] << 8) | ((unsigned)lut[4 * i + 2] << 16) | ((unsigned)lut[4 * i + 3] << 24);
    __syncthreads();
    const size_t g = blockIdx.y;
    const unsigned i0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (i0 >= npix) return;
    const unsigned n = npix - i0 < 4u ? npix - i0 : 4u;
    const float a = (float)stat[g * RD_ROW + 1], mn = (float)stat[g * RD_ROW];
    const bool nan = a != a;
    const float b = a - mn;
    const bm_src_t src = (bm_src_t)maps[g] + i0;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (n == 4u) {
        const bm_f4u t = *(rd_v4_t)src;
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (unsigned e = 0; e < 3; ++e)
            if (e < n) v[e] = src[e];
    }
    unsigned gy[4], c[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        gy[e] = rd_sat_u8(v[e] * 255.0f);
        float q = nan ? 1.0f : __fdiv_rn(a - v[e], b);
        if (q != q) q = 0.f;                                      // a constant map: 0 / 0
        float x = 0.f;
        if (vrange != 0.0) {
            x = (float)((double)q - vmin);
            x = (float)((double)x / vrange);
        }
        const float xa = x * 256.0f;
        c[e] = slut[xa == 256.0f ? 255 : (xa < 0.f ? 256 : (xa >= 256.0f ? 257 : (int)xa))];
    }
    unsigned char *gd = grey + g * npix + i0;
    unsigned *cd = reinterpret_cast<unsigned *>(color) + g * npix + i0;
    if (n == 4u) {
        rd_b4 gb;
        gb.x = (unsigned char)gy[0], gb.y = (unsigned char)gy[1], gb.z = (unsigned char)gy[2], gb.w = (unsigned char)gy[3];
        *reinterpret_cast<rd_b4 *>(gd) = gb;
        rd_u4 cw;
        cw.x = c[0], cw.y = c[1], cw.z = c[2], cw.w = c[3];
        *reinterpret_cast<rd_u4 *>(cd) = cw;
    } else {
#pragma unroll
        for (unsigned e = 0; e < 3; ++e)
            if (e < n) gd[e] = (unsigned char)gy[e], cd[e] = c[e];
    }
}

__global__ void __launch_bounds__(256) rd_inputs_kernel(const float *const *__restrict__ inputs, rd_meta_t meta, unsigned npix,
                                                        unsigned char *__restrict__ rgb) {
    const size_t g = blockIdx.y;
    const unsigned i0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (i0 >= npix) return;
    const unsigned n = npix - i0 < 4u ? npix - i0 : 4u;
    const int C = meta.c[g];
    const bool events = meta.kind[g] == RAMNET_RENDER_EVENTS;
    const bm_src_t src = (bm_src_t)inputs[g] + i0;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < C; ++ch) {
        const bm_src_t p = src + (size_t)ch * npix;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (n == 4u) {
            const bm_f4u t = *(rd_v4_t)p;
            v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
        } else {
#pragma unroll
            for (unsigned e = 0; e < 3; ++e)
                if (e < n) v[e] = p[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = ch ? s[e] + v[e] : v[e];
    }
    unsigned char o[12];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (events) {
            o[3 * e] = (double)s[e] > 0.9 ? 255 : 0, o[3 * e + 1] = 0, o[3 * e + 2] = (double)s[e] <= -0.5 ? 255 : 0;
        } else {
            o[3 * e] = o[3 * e + 1] = o[3 * e + 2] = (unsigned char)rd_sat_u8(s[e] * 255.0f);
        }
    }
    unsigned char *d = rgb + 3 * (g * npix + i0);
    if (n == 4u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            rd_b4 w;
            w.x = o[4 * k], w.y = o[4 * k + 1], w.z = o[4 * k + 2], w.w = o[4 * k + 3];
            *reinterpret_cast<rd_b4 *>(d + 4 * k) = w;
        }
    } else {
#pragma unroll
        for (unsigned e = 0; e < 9; ++e)
            if (e < 3 * n) d[e] = o[e];
    }
}

static int rd_launch_stats(const float *const *maps, int G, const float *const *spred, const float *const *starget, int n_scale, size_t npix,
                           float clip, float reg, void *workspace, double *scale, const double **stat, hipStream_t st) {
    const rd_plan_t pl = rd_plan((size_t)G + n_scale, npix);
    char *ws = static_cast<char *>(workspace);
    double *res = reinterpret_cast<double *>(ws + pl.off_stat);
    hipLaunchKernelGGL(rd_stats_kernel, dim3(pl.Ws, G + n_scale), dim3(BM_T), 0, st, maps, G, spred, starget, (unsigned)npix, pl.Ws, clip, reg,
                       reinterpret_cast<unsigned *>(ws), res, reinterpret_cast<double *>(ws + pl.off_part), scale);
    RAMNET_LAUNCH_CHECK();
    *stat = res;
    return 0;
}

}  // namespace ramnet

using namespace ramnet;

extern "C" size_t ramnet_render_depth_workspace(int G, int n_scale, size_t npix) {
    return rd_sizes_ok(G, n_scale, npix) ? rd_plan((size_t)G + n_scale, npix).total : 0;
}

extern "C" int ramnet_render_depth(const float *const *maps, int G, int H, int W, double vmin, double vmax, const unsigned char *lut,
                                   const float *const *scale_pred, const float *const *scale_target, int n_scale, float clip_distance,
                                   float reg_factor, void *workspace, unsigned char *grey, unsigned char *color, double *scale, void *stream) {
    RAMNET_CHECK_ARG(G >= 1 && H >= 1 && W >= 1 && rd_sizes_ok(G, n_scale, (size_t)H * W));
    RAMNET_CHECK_ARG(maps && lut && workspace && grey && color);
    RAMNET_CHECK_ARG(vmin <= vmax && vmax - vmin < __builtin_inf());          // (a NaN fails the comparison)
    RAMNET_CHECK_ARG(n_scale == 0 || (scale_pred && scale_target && scale && clip_distance > 0.f));
    RAMNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0 && (reinterpret_cast<uintptr_t>(color) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(scale) & 7) == 0);
    const size_t npix = (size_t)H * W;
    const double *stat = nullptr;
    hipStream_t st = (hipStream_t)stream;
    const int e = rd_launch_stats(maps, G, scale_pred, scale_target, n_scale, npix, clip_distance, reg_factor, workspace, scale, &stat, st);
    if (e) return e;
    hipLaunchKernelGGL(rd_map_kernel, dim3((unsigned)((npix + 1023) / 1024), G), dim3(256), 0, st, maps, (unsigned)npix, vmin, vmax - vmin, lut, stat,
                       grey, color);
    RAMNET_LAUNCH_CHECK();
    return 0;
}

extern "C" int ramnet_least_squares_scale(const float *const *pred, const float *const *target, int G, size_t npix, float clip_distance,
                                          float reg_factor, void *workspace, double *scale, void *stream) {
    RAMNET_CHECK_ARG(G >= 1 && rd_sizes_ok(0, G, npix));
    RAMNET_CHECK_ARG(pred && target && workspace && scale && clip_distance > 0.f);
    RAMNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0 && (reinterpret_cast<uintptr_t>(scale) & 7) == 0);
    const double *stat = nullptr;
    return rd_launch_stats(nullptr, 0, pred, target, G, npix, clip_distance, reg_factor, workspace, scale, &stat, (hipStream_t)stream);
}

extern "C" int ramnet_render_inputs(const float *const *inputs, const int *channels, const int *kinds, int G, int H, int W, unsigned char *rgb,
                                    void *stream) {
    RAMNET_CHECK_ARG(G >= 1 && G <= 65535 && H >= 1 && W >= 1 && (size_t)H * W < ((size_t)1 << 31));
    RAMNET_CHECK_ARG(inputs && channels && kinds && rgb);
    for (int g = 0; g < G; ++g)
        RAMNET_CHECK_ARG(channels[g] >= 1 && channels[g] <= 65535 && (kinds[g] == RAMNET_RENDER_EVENTS || kinds[g] == RAMNET_RENDER_FRAME));
    const size_t npix = (size_t)H * W;
    for (int g0 = 0; g0 < G; g0 += RD_MAX_INPUTS) {
        const int m = G - g0 < RD_MAX_INPUTS ? G - g0 : RD_MAX_INPUTS;
        rd_meta_t meta;
        for (int k = 0; k < RD_MAX_INPUTS; ++k) meta.c[k] = k < m ? (unsigned short)channels[g0 + k] : 0, meta.kind[k] = k < m ? (unsigned char)kinds[g0 + k] : 0;
        hipLaunchKernelGGL(rd_inputs_kernel, dim3((unsigned)((npix + 1023) / 1024), m), dim3(256), 0, (hipStream_t)stream, inputs + g0, meta,
                           (unsigned)npix, rgb + 3 * npix * (size_t)g0);
    }
    RAMNET_LAUNCH_CHECK();
    return 0;
}
