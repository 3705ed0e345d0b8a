// Multi-scale gradient loss (model/loss.py:22-70, restated in oracle/loss_ref.py; kornia parity unpinned) of G (prediction, target)
// pairs together: statistics, loss and gradient of a whole sequence in a fixed number of launches, with no saved pyramid, no zero-fill
// and no floating-point atomics — the same input gives the same bits on every call.
//
//   diff = pred - target;  P_s = AvgPool2d(2^s)(diff) (H >> s x W >> s: trailing rows / columns dropped, a NaN makes its cell NaN)
//   g_s  = Sobel / 8 of P_s with replicate padding at the edge of P_s (a NaN anywhere in the 3 x 3 window makes both components NaN)
//   S_s  = sum |g_s| over the non-NaN components, C_s = their count;  loss = mean_s (S_s / C_s * Bg * 2)
//
// grid = (tiles, B, G).  A workgroup owns a 64 x 64 tile of one sample whose origin is a multiple of 8 = 2^(4 - 1): it stages diff of
// the tile and a halo in LDS (16-byte loads where the rows allow them) and builds the coarser levels there by 2 x 2 means, so a cell
// of every level lies in exactly one tile.  The halo is zero outside the image; such values are never used, because a Sobel window
// clamps its indices into the level's own map first.
//
// statistics: halo 8 (one cell of the coarsest level).  Every workgroup stores its (S_s, C_s) row to its own slot; gl_join_kernel adds
//             the slots of a pair in a fixed order (thread t: column t % 8 of rows t / 8, t / 8 + 32, ...; then the 32 lanes in order).
// backward:   a gather, halo 16.  dP_s(v, u) needs the signs of g_s at (v +- 1, u +- 1), and those need P_s at +- 2.  The workgroup
//             rebuilds the pyramid, keeps sign(gx), sign(gy) of every cell it needs as one byte, and forms
//               8 dP_s = Sy^T Dx^T sign(gx) + Dy^T Sx^T sign(gy)
//             in INTEGER arithmetic, with the transposes of the clamped 1-D operators S = [1 2 1] and D = [-1 0 1]:
//               S^T a (v) = a(clamp(v - 1)) + 2 a(v) + a(clamp(v + 1))                       (S with replicate padding is symmetric)
//               D^T a (v) = (v > 0 ? a(v - 1) : -a(0)) - (v < n - 1 ? a(v + 1) : -a(n - 1))  (a clamped tap lands on the edge cell)
//             dpred[Y, X] = sum_s coef_s * 8 dP_s[Y >> s, X >> s],  coef_s = up_g w_g gain Bg 2 / (C_s ns 4^s 8), every element
//             written once.  A scale with C_s = 0 has no valid component: coefficient 0.  A cell that holds a NaN has only NaN windows
//             around it, so pixels under a NaN target get 0 without a test.
#include "common.hpp"

namespace ramnet {

constexpr int GL_T = 64;              // tile side, full-resolution pixels
constexpr int GL_NT = 256;            // threads of a workgroup
constexpr int GL_MAXS = 4;            // scales
constexpr int GL_ROW = 2 * GL_MAXS;   // doubles of a partial row: (S_s, C_s) of the four scales
constexpr int GL_HF = 8, GL_HB = 16;  // halo of the statistics / backward kernels

template <int HALO>
struct gl_geom {
    static constexpr int PS = GL_T + 2 * HALO;                                   // side of the level-0 patch
    static constexpr int side(int s) { return PS >> s; }
    static constexpr int off(int s) { return s == 0 ? 0 : off(s - 1) + side(s - 1) * side(s - 1); }
    static constexpr int total = off(GL_MAXS);
};

__device__ __forceinline__ double gl_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// diff of rows [ty0 - HALO, ty0 + 64 + HALO) x columns [tx0 - HALO, ..) of one sample into L (level 0), 0 outside the image, then the
// levels 1 .. ns - 1 by 2 x 2 means.  vec: W % 4 == 0 and both maps 16-byte aligned (then a float4 is inside or outside as a whole).
template <int HALO>
__device__ __forceinline__ void gl_build(float *__restrict__ L, const float *__restrict__ p, const float *__restrict__ t, int H, int W, int ty0,
                                         int tx0, int ns, bool vec) {
    typedef gl_geom<HALO> G;
    constexpr int PS = G::PS;
    const int Y0 = ty0 - HALO, X0 = tx0 - HALO;
    if (vec) {
        constexpr int Q = PS / 4;
#pragma unroll 4
        for (int i = threadIdx.x; i < PS * Q; i += GL_NT) {
            const int r = i / Q, q = i - r * Q, Y = Y0 + r, X = X0 + 4 * q;
            const bool ok = (unsigned)Y < (unsigned)H && (unsigned)X < (unsigned)W;
            const size_t o = ok ? (size_t)Y * W + X : 0;
            const float4 a = ld4(p + o), b = ld4(t + o);
            st4(L + r * PS + 4 * q, ok ? make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w) : f4zero());
        }
    } else {
#pragma unroll 4
        for (int i = threadIdx.x; i < PS * PS; i += GL_NT) {
            const int r = i / PS, c = i - r * PS, Y = Y0 + r, X = X0 + c;
            const bool ok = (unsigned)Y < (unsigned)H && (unsigned)X < (unsigned)W;
            const size_t o = ok ? (size_t)Y * W + X : 0;
            const float a = p[o], b = t[o];
            L[i] = ok ? a - b : 0.f;
        }
    }
    __syncthreads();
    int lo = 0;
    for (int s = 1; s < ns; ++s) {
        const int n = PS >> s, m = n * 2;
        const float *src = L + lo;
        float *dst = L + lo + m * m;
        lo += m * m;
        for (int i = threadIdx.x; i < n * n; i += GL_NT) {
            const int y = i / n, x = i - y * n;
            const float2 a = *reinterpret_cast<const float2 *>(src + (2 * y) * m + 2 * x);
            const float2 b = *reinterpret_cast<const float2 *>(src + (2 * y + 1) * m + 2 * x);
            dst[i] = ((a.x + a.y) + (b.x + b.y)) * 0.25f;
        }
        __syncthreads();
    }
}

// Sobel / 8 at cell (yc, xc) of a level whose map is hs x ws; P: the level's patch (row stride n), whose cell (0, 0) is map cell (py0, px0).
__device__ __forceinline__ void gl_sobel(const float *__restrict__ P, int n, int py0, int px0, int hs, int ws, int yc, int xc, float &gx, float &gy) {
    const int ym = (yc > 0 ? yc - 1 : 0) - py0, yp = (yc < hs - 1 ? yc + 1 : hs - 1) - py0, y = yc - py0;
    const int xm = (xc > 0 ? xc - 1 : 0) - px0, xp = (xc < ws - 1 ? xc + 1 : ws - 1) - px0, x = xc - px0;
    const float a = P[ym * n + xm], b = P[ym * n + x], c = P[ym * n + xp];
    const float d = P[y * n + xm], e = P[y * n + x], f = P[y * n + xp];
    const float g = P[yp * n + xm], hh = P[yp * n + x], i = P[yp * n + xp];
    // the reference convolves with the full 3 x 3 kernel: a NaN under a zero tap (0 * NaN) makes both components NaN
    const float nanprop = 0.f * (a + b + c + d + e + f + g + hh + i);
    gx = (-a + c - 2.f * d + 2.f * f - g + i) * 0.125f + nanprop;
    gy = (-a - 2.f * b - c + g + 2.f * hh + i) * 0.125f + nanprop;
}

__global__ void __launch_bounds__(GL_NT) gl_stats_kernel(const float *const *__restrict__ preds, const float *const *__restrict__ targets, int H,
                                                         int W, int ns, int tilesX, double *__restrict__ part) {
    typedef gl_geom<GL_HF> G;
    __shared__ __attribute__((aligned(16))) float L[G::total];
    __shared__ double red[GL_ROW][GL_NT / 64];
    const int tile = blockIdx.x, b = blockIdx.y;
    const size_t g = blockIdx.z;
    const int ty0 = (tile / tilesX) * GL_T, tx0 = (tile % tilesX) * GL_T;
    const float *p = preds[g] + (size_t)b * H * W, *t = targets[g] + (size_t)b * H * W;
    const bool vec = (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(preds[g]) | reinterpret_cast<uintptr_t>(targets[g])) & 15) == 0;
    gl_build<GL_HF>(L, p, t, H, W, ty0, tx0, ns, vec);

    double acc[GL_ROW] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < GL_MAXS; ++s) {
        if (s >= ns) break;
        const int hs = H >> s, ws = W >> s, n = G::PS >> s, cy0 = ty0 >> s, cx0 = tx0 >> s;
        const int ny = min(GL_T >> s, hs - cy0), nx = min(GL_T >> s, ws - cx0);
        if (ny <= 0 || nx <= 0) continue;
        const float *P = L + G::off(s);
        double sum = 0.0;
        unsigned cnt = 0;
        for (int i = threadIdx.x; i < ny * nx; i += GL_NT) {
            const int ly = i / nx, lx = i - ly * nx;
            float gx, gy;
            gl_sobel(P, n, cy0 - (GL_HF >> s), cx0 - (GL_HF >> s), hs, ws, cy0 + ly, cx0 + lx, gx, gy);
            if (gx == gx) sum += (double)fabsf(gx), ++cnt;
            if (gy == gy) sum += (double)fabsf(gy), ++cnt;
        }
        acc[2 * s] = sum, acc[2 * s + 1] = (double)cnt;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < GL_ROW; ++k) {
        const double v = gl_wave_sum(acc[k]);
        if (lane == 0) red[k][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < GL_ROW) {
        double v = 0.0;
        for (int i = 0; i < GL_NT / 64; ++i) v += red[threadIdx.x][i];
        const size_t wg = (size_t)b * gridDim.x + tile, nwg = (size_t)gridDim.x * gridDim.y;
        part[(g * nwg + wg) * GL_ROW + threadIdx.x] = v;
    }
}

// stats[g][ns][2] = the nwg partial rows of pair g added in a fixed order.
__global__ void __launch_bounds__(GL_NT) gl_join_kernel(const double *__restrict__ part, int nwg, int ns, double *__restrict__ stats) {
    __shared__ double red[GL_NT / GL_ROW][GL_ROW];
    const size_t g = blockIdx.x;
    const int col = threadIdx.x % GL_ROW, r = threadIdx.x / GL_ROW;
    double v = 0.0;
    for (int row = r; row < nwg; row += GL_NT / GL_ROW) v += part[(g * nwg + row) * GL_ROW + col];
    red[r][col] = v;
    __syncthreads();
    if (threadIdx.x < 2 * ns) {
        double s = 0.0;
        for (int i = 0; i < GL_NT / GL_ROW; ++i) s += red[i][threadIdx.x];
        stats[g * 2 * ns + threadIdx.x] = s;
    }
}

// loss[g] = w_g * mean_s (S_s / C_s * Bg * 2) (0 / 0 = NaN for a scale without a valid component, as the reference); wsum = their sum in
// index order.
__global__ void __launch_bounds__(64) gl_loss_kernel(const double *__restrict__ stats, int G, int ns, double Bg, const double *__restrict__ Bg_dev,
                                                     const float *__restrict__ weights, float *__restrict__ loss, float *__restrict__ wsum) {
    if (Bg_dev) Bg = *Bg_dev;
    for (int g = threadIdx.x; g < G; g += 64) {
        double t = 0.0;
        for (int s = 0; s < ns; ++s) t += stats[((size_t)g * ns + s) * 2] / stats[((size_t)g * ns + s) * 2 + 1] * Bg * 2.0;
        loss[g] = (float)((weights ? (double)weights[g] : 1.0) * (t / ns));
    }
    __syncthreads();
    if (wsum && threadIdx.x == 0) {
        double t = 0.0;
        for (int g = 0; g < G; ++g) t += (double)loss[g];
        *wsum = (float)t;
    }
}

// sign(gx), sign(gy) of a cell in one byte; 5 = (0, 0)
__device__ __forceinline__ int gl_sx(int c) { return (c & 3) - 1; }
__device__ __forceinline__ int gl_sy(int c) { return (c >> 2) - 1; }

// 8 dP(v, u) of a level with an hs x ws map from the sign bytes; code: row stride cs, entry (0, 0) = map cell (cy0 - 1, cx0 - 1).
__device__ __forceinline__ int gl_dp8(const unsigned char *__restrict__ code, int cs, int cy0, int cx0, int hs, int ws, int v, int u) {
    const int r[3] = {(v > 0 ? v - 1 : 0) - cy0 + 1, v - cy0 + 1, (v < hs - 1 ? v + 1 : hs - 1) - cy0 + 1};
    const int c[3] = {(u > 0 ? u - 1 : 0) - cx0 + 1, u - cx0 + 1, (u < ws - 1 ? u + 1 : ws - 1) - cx0 + 1};
    const int fl = u > 0 ? 1 : -1, fh = u < ws - 1 ? 1 : -1;
    int A = 0, tr[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int k0 = code[r[i] * cs + c[0]], k1 = code[r[i] * cs + c[1]], k2 = code[r[i] * cs + c[2]];
        A += (i == 1 ? 2 : 1) * (fl * gl_sx(k0) - fh * gl_sx(k2));
        tr[i] = gl_sy(k0) + 2 * gl_sy(k1) + gl_sy(k2);
    }
    return A + (v > 0 ? tr[0] : -tr[0]) - (v < hs - 1 ? tr[2] : -tr[2]);
}

__global__ void __launch_bounds__(GL_NT) gl_bwd_kernel(const float *const *__restrict__ preds, const float *const *__restrict__ targets,
                                                       const double *__restrict__ stats, const float *__restrict__ up, const float *__restrict__ up_sum,
                                                       const float *__restrict__ weights, double scale, const double *__restrict__ Bg_dev, int H, int W,
                                                       int ns, int tilesX, float *__restrict__ dpred, size_t pair_stride) {
    typedef gl_geom<GL_HB> G;
    constexpr int CS0 = GL_T + 2, CS1 = (GL_T >> 1) + 2, CS2 = (GL_T >> 2) + 2, CS3 = (GL_T >> 3) + 2;
    constexpr int COFF[GL_MAXS] = {0, CS0 * CS0, CS0 * CS0 + CS1 * CS1, CS0 * CS0 + CS1 * CS1 + CS2 * CS2};
    constexpr int CTOT = CS0 * CS0 + CS1 * CS1 + CS2 * CS2 + CS3 * CS3;
    constexpr int DOFF[GL_MAXS] = {0, 0, 32 * 32, 32 * 32 + 16 * 16};          // coef_s * 8 dP_s of the levels 1..3, in the level-0 patch
    __shared__ __attribute__((aligned(16))) float L[G::total];
    __shared__ unsigned char code[CTOT];
    const int tile = blockIdx.x, b = blockIdx.y;
    const size_t g = blockIdx.z;
    const int ty0 = (tile / tilesX) * GL_T, tx0 = (tile % tilesX) * GL_T;
    const float *p = preds[g] + (size_t)b * H * W, *t = targets[g] + (size_t)b * H * W;
    float *out = dpred + g * pair_stride + (size_t)b * H * W;
    const bool vin = (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(preds[g]) | reinterpret_cast<uintptr_t>(targets[g])) & 15) == 0;
    const bool vout = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(dpred + g * pair_stride) & 15) == 0;
    gl_build<GL_HB>(L, p, t, H, W, ty0, tx0, ns, vin);

    // coefficient of 8 dP_s
    float coef[GL_MAXS];
    const double upw = ((up ? (double)up[g] : 0.0) + (up_sum ? (double)*up_sum : 0.0)) * (weights ? (double)weights[g] : 1.0) * scale *
                       (Bg_dev ? *Bg_dev : 1.0);
#pragma unroll
    for (int s = 0; s < GL_MAXS; ++s) {
        const double cnt = s < ns ? stats[(g * ns + s) * 2 + 1] : 0.0;
        coef[s] = cnt > 0.0 ? (float)(upw / cnt / (double)(ns * 8 * (1 << (2 * s)))) : 0.f;
    }

    // sign bytes of the cells [cy0 - 1, cy0 + (64 >> s) + 1) x [cx0 - 1, ..) of every level; (0, 0) outside the level's map
#pragma unroll
    for (int s = 0; s < GL_MAXS; ++s) {
        if (s >= ns) break;
        const int hs = H >> s, ws = W >> s, n = G::PS >> s, cy0 = ty0 >> s, cx0 = tx0 >> s, cs = (GL_T >> s) + 2;
        const float *P = L + G::off(s);
        unsigned char *cd = code + COFF[s];
        for (int i = threadIdx.x; i < cs * cs; i += GL_NT) {
            const int ly = i / cs, lx = i - ly * cs, yc = cy0 - 1 + ly, xc = cx0 - 1 + lx;
            int k = 5;
            if ((unsigned)yc < (unsigned)hs && (unsigned)xc < (unsigned)ws) {
                float gx, gy;
                gl_sobel(P, n, cy0 - (GL_HB >> s), cx0 - (GL_HB >> s), hs, ws, yc, xc, gx, gy);
                k = (gx > 0.f ? 2 : gx < 0.f ? 0 : 1) + 4 * (gy > 0.f ? 2 : gy < 0.f ? 0 : 1);          // NaN: (0, 0)
            }
            cd[i] = (unsigned char)k;
        }
    }
    __syncthreads();

    // coef_s * 8 dP_s of the tile's cells of the levels 1 .. ns - 1 (the pyramid is no longer needed: they go where level 0 was)
    float *D = L;
    for (int i = threadIdx.x; i < 32 * 32 + 16 * 16 + 8 * 8; i += GL_NT) {
        const int s = i < 32 * 32 ? 1 : i < 32 * 32 + 16 * 16 ? 2 : 3;
        const int j = i - DOFF[s], m = GL_T >> s, ly = j / m, lx = j - ly * m;
        const int hs = H >> s, ws = W >> s, cy0 = ty0 >> s, cx0 = tx0 >> s, v = cy0 + ly, u = cx0 + lx;
        float d = 0.f;
        if (s < ns && v < hs && u < ws) d = coef[s] * (float)gl_dp8(code + COFF[s], m + 2, cy0, cx0, hs, ws, v, u);
        D[i] = d;
    }
    __syncthreads();

    // every pixel of the tile: level 0 from the sign bytes, the coarser levels from D
    for (int i = threadIdx.x; i < GL_T * GL_T / 4; i += GL_NT) {
        const int ly = i / (GL_T / 4), lx = (i - ly * (GL_T / 4)) * 4, Y = ty0 + ly, X = tx0 + lx;
        if (Y >= H || X >= W) continue;
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = lx + j;
            float d = 0.f;
            if (X + j < W) d = coef[0] * (float)gl_dp8(code, CS0, ty0, tx0, H, W, Y, X + j);
            d += D[DOFF[1] + (ly >> 1) * 32 + (x >> 1)];
            d += D[DOFF[2] + (ly >> 2) * 16 + (x >> 2)];
            d += D[DOFF[3] + (ly >> 3) * 8 + (x >> 3)];
            r[j] = d + 0.f;           // a negative coefficient times 0 is -0 at every scale: a pixel that nothing reaches gets +0 whatever the sign of `up`
        }
        float *o = out + (size_t)Y * W + X;
        if (vout) {
            st4(o, make_float4(r[0], r[1], r[2], r[3]));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (X + j < W) o[j] = r[j];
        }
    }
}

struct gl_ptrs_t {
    const void *p[128];
};

__global__ void gl_fill_table_kernel(const void **table, gl_ptrs_t v, int n) {
    if ((int)threadIdx.x < n) table[threadIdx.x] = v.p[threadIdx.x];
}

static int gl_check_dims(int G, int B, int H, int W, int ns) {
    RAMNET_CHECK_ARG(G >= 0 && G <= 65535 && B > 0 && B <= 65535 && H > 0 && W > 0);
    RAMNET_CHECK_ARG(ns >= 1 && ns <= GL_MAXS && (H >> (ns - 1)) >= 1 && (W >> (ns - 1)) >= 1);
    RAMNET_CHECK_ARG((size_t)B * H * W < ((size_t)1 << 31));
    RAMNET_CHECK_ARG((size_t)cdiv(H, GL_T) * cdiv(W, GL_T) * B < ((size_t)1 << 24));
    return 0;
}

}  // namespace ramnet

using namespace ramnet;

extern "C" int ramnet_fill_pointer_table(const void **table, const void *const *host_ptrs, int n, void *stream) {
    RAMNET_CHECK_ARG(n >= 0);
    if (n == 0) return 0;
    RAMNET_CHECK_ARG(table && host_ptrs);
    for (int i = 0; i < n; i += 128) {
        gl_ptrs_t v;
        const int m = n - i < 128 ? n - i : 128;
        for (int k = 0; k < 128; ++k) v.p[k] = k < m ? host_ptrs[i + k] : nullptr;
        hipLaunchKernelGGL(gl_fill_table_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, table + i, v, m);
    }
    RAMNET_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t ramnet_grad_loss_workspace(int G, int B, int H, int W) {
    if (G <= 0 || B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)G * B * cdiv(H, GL_T) * cdiv(W, GL_T) * GL_ROW * sizeof(double);
}

extern "C" int ramnet_grad_loss_from_stats(const double *stats, int G, int num_scales, double Bg, const double *Bg_dev, const float *weights,
                                           float *loss, float *wsum, void *stream) {
    RAMNET_CHECK_ARG(G >= 0 && G <= 65535 && num_scales >= 1 && num_scales <= GL_MAXS && (Bg_dev || Bg > 0.0));
    if (G == 0) return 0;
    RAMNET_CHECK_ARG(stats && loss);
    hipLaunchKernelGGL(gl_loss_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stats, G, num_scales, Bg, Bg_dev, weights, loss, wsum);
    RAMNET_LAUNCH_CHECK();
    return 0;
}

extern "C" int ramnet_grad_loss_stats(const float *const *pred, const float *const *target, int G, int B, int H, int W, int num_scales,
                                      void *workspace, double *stats, const float *weights, float *loss, float *wsum, void *stream) {
    if (int e = gl_check_dims(G, B, H, W, num_scales)) return e;
    if (G == 0) return 0;
    RAMNET_CHECK_ARG(pred && target && workspace && stats);
    RAMNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(stats) & 7) == 0);
    const int tilesX = cdiv(W, GL_T), tiles = tilesX * cdiv(H, GL_T);
    hipStream_t st = (hipStream_t)stream;
    double *part = static_cast<double *>(workspace);
    hipLaunchKernelGGL(gl_stats_kernel, dim3(tiles, B, G), dim3(GL_NT), 0, st, pred, target, H, W, num_scales, tilesX, part);
    hipLaunchKernelGGL(gl_join_kernel, dim3(G), dim3(GL_NT), 0, st, part, tiles * B, num_scales, stats);
    if (loss) hipLaunchKernelGGL(gl_loss_kernel, dim3(1), dim3(64), 0, st, stats, G, num_scales, (double)B, (const double *)nullptr, weights, loss,
                                 wsum);
    RAMNET_LAUNCH_CHECK();
    note_kernel("gl_stats_kernel + gl_join_kernel");
    return 0;
}

extern "C" int ramnet_grad_loss_bwd(const float *const *pred, const float *const *target, int G, int B, int H, int W, int num_scales,
                                    const double *stats, double Bg, const double *Bg_dev, double gain, const float *weights, const float *up,
                                    const float *up_sum, float *dpred, void *stream) {
    if (int e = gl_check_dims(G, B, H, W, num_scales)) return e;
    if (G == 0) return 0;
    RAMNET_CHECK_ARG(pred && target && stats && dpred && (up || up_sum) && (Bg_dev || Bg > 0.0));
    RAMNET_CHECK_ARG((reinterpret_cast<uintptr_t>(dpred) & 3) == 0);
    const int tilesX = cdiv(W, GL_T), tiles = tilesX * cdiv(H, GL_T);
    hipLaunchKernelGGL(gl_bwd_kernel, dim3(tiles, B, G), dim3(GL_NT), 0, (hipStream_t)stream, pred, target, stats, up, up_sum, weights,
                       gain * 2.0 * (Bg_dev ? 1.0 : Bg), (const double *)Bg_dev, H, W, num_scales, tilesX, dpred, (size_t)B * H * W);
    RAMNET_LAUNCH_CHECK();
    note_kernel("gl_bwd_kernel");
    return 0;
}
