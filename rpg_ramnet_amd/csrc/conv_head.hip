// The two head layers of the RAM-Net path (5x5, stride 1, 5 event bins / 1 frame channel -> 32 feature maps at full
// resolution; statenet.py:160-175, submodules.py:8-35) for gfx950 (MI355X), forward, backward-weights and backward-data (the
// gradient of the model's event grids and frames: conv_head_dgrad_kernel below).
//
// With 1-8 input channels the generic implicit-GEMM kernel has nothing to amortise its patch staging and operand traffic
// over (one 8-channel chunk, N = 32): it runs at ~16 % of the fp32 MFMA peak.  Here the reduction index is the dense
// (tap, channel) pair, K = 25*CR (125 for the event head instead of 25*8 = 200), and
//   forward:  the whole weight matrix [K][32] lives in REGISTERS (lane = output channel, 63 VGPRs for CR = 5); a wave owns
//             4 rows x 32 pixels, the A operand of v_mfma_f32_32x32x2_f32 is one 4-byte LDS read per MFMA from a
//             channel-planar input patch (conflict-free: lanes = consecutive pixels), addressed as lane base + a
//             compile-time (tap, channel) constant;
//   backward-weights: dW[(tap,c)][n] = sum_pixels in(pixel + tap, c) * g(pixel, n): M = (tap, c) in 4 blocks of 32, N = 32,
//             K = pixels; both operands from LDS (planar patch, gradient tile [pixel][32]), 5 reads per 4 MFMAs; the
//             [128][32] partial of a workgroup is folded into the OIHW gradient (and the bias gradient) by atomics.
// Exact fp32 like the rest of the path.
#include <stdlib.h>
#include "common.hpp"

namespace ramnet {

constexpr int HT_W = 32;                            // output pixels per workgroup: TH rows (TH/4 per wave) x 32
constexpr int HP_W = HT_W + 4;                      // input patch width
constexpr int HP_LD = HP_W + 1;                     // padded patch row (floats)
constexpr int HF_H = 16, HG_H = 8;                  // tile height of the forward / backward-weights kernel

template <int CR, int TH>
struct HeadGeom {
    static constexpr int KT = 25 * CR;              // dense reduction length
    static constexpr int NS = (KT + 1) / 2;         // MFMA steps (K = 2 each)
    static constexpr int PLANE = (TH + 4) * HP_LD;  // one channel plane of the input patch
    // LDS offset of reduction index k inside the planar patch, relative to the output pixel's own position
    static constexpr int koff(int k) {
        return k >= KT ? 0 : (k % CR) * PLANE + ((k / CR) / 5) * HP_LD + (k / CR) % 5;
    }
};

// stage the (TH+4 x HP_W) input patch of the tile at (b, oy0, ox0) as CR channel planes; zero outside the image
template <int CR, int TH>
__device__ __forceinline__ void head_stage_patch(float *__restrict__ P, const float *__restrict__ x, int ld, int b, int oy0, int ox0, int H,
                                                 int W, int tid) {
    constexpr int HP_PLANE = HeadGeom<CR, TH>::PLANE;
#pragma unroll
    for (int i = tid; i < (TH + 4) * HP_W; i += 256) {
        const int py = i / HP_W, px = i - py * HP_W;
        const int iy = oy0 - 2 + py, ix = ox0 - 2 + px;
        float v[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
            const float *src = x + ((size_t)(b * H + iy) * W + ix) * ld;
            const float4 a = ld4(src);
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
            if (CR > 4) {
                const float4 c = ld4(src + 4);
                v[4] = c.x, v[5] = c.y, v[6] = c.z, v[7] = c.w;
            }
            if (CR > 8) {
                const float4 c = ld4(src + 8);
                v[8] = c.x, v[9] = c.y, v[10] = c.z, v[11] = c.w;
            }
        }
#pragma unroll
        for (int c = 0; c < CR; ++c) P[c * HP_PLANE + py * HP_LD + px] = v[c];
    }
}

static bool head_channels_ok(int c) { return c == 1 || c == 3 || c == 5 || c == 10; }      // (10: the configs[4] voxel grids)

struct HeadFwdParams {
    const float *x, *wp, *bias;
    float *out;
    int ld, ldo, B, H, W, Cout, relu, tiles_x, tiles_y;
};

template <int CR>
__global__ void __launch_bounds__(256, 2) conv_head_fwd_kernel(const HeadFwdParams p) {
    using G = HeadGeom<CR, HF_H>;
    constexpr int HT_H = HF_H;
    __shared__ float P[CR * G::PLANE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, h = lane >> 5;
    int bid = blockIdx.x;
    const int tx = bid % p.tiles_x;
    bid /= p.tiles_x;
    const int ty = bid % p.tiles_y, b = bid / p.tiles_y;
    const int oy0 = ty * HT_H, ox0 = tx * HT_W;

    // the lane's column of the weight matrix: k = 2s + h
    float wreg[G::NS];
#pragma unroll
    for (int s = 0; s < G::NS; ++s) wreg[s] = p.wp[(2 * s + h) * 32 + n];
    // (loaded HERE, in front of the patch staging that waits for all its loads: a bias load still pending at the epilogue makes the
    // compiler wait for ALL memory operations — i.e. for the previous STORE — in front of each of the 64 conditional stores)
    const float bv = (p.bias && n < p.Cout) ? p.bias[n] : 0.f;

    head_stage_patch<CR, HF_H>(P, p.x, p.ld, b, oy0, ox0, p.H, p.W, tid);
    __syncthreads();

    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const float *pa = P + (wave * 4) * HP_LD + n;      // A row = pixel (lane & 31) of patch row 4*wave + t (+ tap offsets)
#pragma unroll
    for (int s = 0; s < G::NS; ++s) {
        const int off = h ? G::koff(2 * s + 1) : G::koff(2 * s);
        float a[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] = pa[off + t * HP_LD];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], wreg[s], acc[t], 0, 0, 0);
    }

    if (n >= p.Cout) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int oy = oy0 + wave * 4 + t;
        if (oy >= p.H) continue;
        float *orow = p.out + ((size_t)(b * p.H + oy) * p.W) * p.ldo + n;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ox = ox0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (ox >= p.W) continue;
            float v = acc[t][r] + bv;
            if (p.relu) v = fmaxf(v, 0.f);
            orow[(size_t)ox * p.ldo] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward-weights
struct HeadWgradParams {
    const float *x, *g, *gm;
    float *dw, *dbias;
    int ld, ldg, ldgm, B, H, W, Cin, Cout, tiles_x, tiles_y, ntiles;
};

constexpr int HG_LD = 32;                           // gradient tile [HG_H * 32 pixels][32 channels]

#define HEADWG_SLAB 0
#define HEADWG_KERNEL(name) name
#include "conv_head_wgrad_kernel.hpp"
#undef HEADWG_SLAB
#undef HEADWG_KERNEL
#define HEADWG_SLAB 1
#define HEADWG_KERNEL(name) name##_slab
#include "conv_head_wgrad_kernel.hpp"
#undef HEADWG_SLAB
#undef HEADWG_KERNEL

// workgroups (= slabs) of the slab form: one per pixel tile up to the cap; 0 when the head kernel does not take the descriptor
int head_wgrad_slabs(const ramnet_wgrad_desc &d) {
    if (!head_channels_ok(d.head_cin) || d.Cout < 1 || d.Cout > 32 || d.B < 1 || d.Ho < 1 || d.Wo < 1) return 0;
    const long ntiles = (long)cdiv(d.Wo, HT_W) * cdiv(d.Ho, HG_H) * d.B;
    return ntiles < RAMNET_WGRAD_SLAB_CAP ? (int)ntiles : RAMNET_WGRAD_SLAB_CAP;
}

int launch_head_wgrad(const ramnet_wgrad_desc &d, hipStream_t st) {
    RAMNET_CHECK_ARG(d.ntaps == 25 && d.stride == 1 && d.in_mode == RAMNET_IN_PLAIN);
    for (int t = 0; t < 25; ++t) RAMNET_CHECK_ARG(d.dy[t] == t / 5 - 2 && d.dx[t] == t % 5 - 2);
    RAMNET_CHECK_ARG(d.head_cin >= 1 && d.head_cin <= d.C0 && head_channels_ok(d.head_cin) && d.Cout <= 32);
    RAMNET_CHECK_ARG(d.Ho == d.Hin && d.Wo == d.Win && ((uintptr_t)d.x0 & 15) == 0 && ((uintptr_t)d.dout & 15) == 0 &&
                     (d.gmask == nullptr || ((uintptr_t)d.gmask & 15) == 0) && (d.head_cin <= 4 || d.C0 >= 8) && (d.head_cin <= 8 || d.C0 >= 12));
    HeadWgradParams q;
    q.x = d.x0, q.g = d.dout, q.gm = d.gmask, q.dw = d.dw, q.dbias = d.dbias;
    q.ld = d.ld0, q.ldg = d.ldg, q.ldgm = d.ldgm, q.B = d.B, q.H = d.Hin, q.W = d.Win, q.Cin = d.C0, q.Cout = d.Cout;
    q.tiles_x = cdiv(d.Wo, HT_W), q.tiles_y = cdiv(d.Ho, HG_H), q.ntiles = q.tiles_x * q.tiles_y * d.B;
    const bool slab = d.dw_slabs > 0;
    int blocks = 512;                               // persistent workgroups (256 measured the same)
    if (slab) blocks = d.dw_slabs < RAMNET_WGRAD_SLAB_CAP ? d.dw_slabs : RAMNET_WGRAD_SLAB_CAP;
    if (blocks > q.ntiles) blocks = q.ntiles;
    if (blocks < 1) blocks = 1;
    auto go = [&](auto kern, int cr) -> int {
        const size_t lds = (size_t)(((cr * (HG_H + 4) * HP_LD + 3) & ~3) + HG_H * HT_W * HG_LD) * sizeof(float);
        RAMNET_FULL_LDS((kern));
        note_kernel(slab ? "conv_head_wgrad_kernel_slab<%d>" : "conv_head_wgrad_kernel<%d>", cr);
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, st, q);
        return 0;
    };
    int rc;
    if (slab) {
        if (d.head_cin == 1) rc = go(conv_head_wgrad_kernel_slab<1>, 1);
        else if (d.head_cin == 3) rc = go(conv_head_wgrad_kernel_slab<3>, 3);
        else if (d.head_cin == 10) rc = go(conv_head_wgrad_kernel_slab<10>, 10);
        else rc = go(conv_head_wgrad_kernel_slab<5>, 5);
    } else if (d.head_cin == 1) rc = go(conv_head_wgrad_kernel<1>, 1);
    else if (d.head_cin == 3) rc = go(conv_head_wgrad_kernel<3>, 3);
    else if (d.head_cin == 10) rc = go(conv_head_wgrad_kernel<10>, 10);
    else rc = go(conv_head_wgrad_kernel<5>, 5);
    if (rc) return rc;
    RAMNET_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- backward-data
// dx[b,y,x,c] = sum_{n,ky,kx} w[n,c,ky,kx] * m(b,y+2-ky,x+2-kx,n) * dy[b,y+2-ky,x+2-kx,n]: the forward kernel with the operand roles
// swapped.  The reduction index is the dense (tap, feature map) pair, K = 25*32 = 800 in 200 steps of v_mfma_f32_16x16x4_f32; M = 16
// consecutive pixels of a row, N = the input channel padded to 16 (the 32-wide form would pad 1-10 channels to 32).  The lane's column
// of the weight matrix lives in REGISTERS (lane = (channel, k), 200 VGPRs, read straight from the OIHW tensor: no pack); the A operand
// is one 4-byte LDS read per MFMA from a feature-map-planar patch of the masked gradient (lanes = consecutive pixels of 4 planes; the
// plane stride 720 = 16 mod 64 puts the four planes of a read on different banks), addressed as lane base + a compile-time (tap, map)
// constant.  A workgroup owns HD_H x HT_W = 16 x 32 pixels (a wave 4 rows x 2 halves = 8 accumulators) and stages its (16+4) x (32+4)
// patch in two passes of 16 feature maps (46 KB of LDS).  A gather: no atomics, no zero-fill, the same bits on every launch.
constexpr int HD_H = 16;                            // tile height of the backward-data kernel (tile = HD_H x HT_W)
constexpr int HD_NC = 16;                           // feature maps staged per pass
constexpr int HD_PLANE = (HD_H + 4) * HP_W;         // one feature-map plane of the gradient patch

struct HeadDgradParams {
    const float *g, *gm, *w;
    float *dx;
    int ldg, ldgm, ld, B, H, W, Cin, Cout, tiles_x, tiles_y;
};

__global__ void __launch_bounds__(256) conv_head_dgrad_kernel(const HeadDgradParams p) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    __shared__ float P[HD_NC * HD_PLANE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, k = lane >> 4;         // B operand: (k, channel c); A operand: (pixel c, k); D: (pixel 4k + r, channel c)
    int bid = blockIdx.x;
    const int tx = bid % p.tiles_x;
    bid /= p.tiles_x;
    const int ty = bid % p.tiles_y, b = bid / p.tiles_y;
    const int oy0 = ty * HD_H, ox0 = tx * HT_W;

    // the lane's column of the weight matrix: step s = tap*8 + j holds feature map n = 4j + k
    float wreg[200];
#pragma unroll
    for (int s = 0; s < 200; ++s) {
        const int n = 4 * (s & 7) + k;
        wreg[s] = (n < p.Cout && c < p.Cin) ? p.w[((size_t)n * p.Cin + c) * 25 + (s >> 3)] : 0.f;
    }

    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *pa = P + k * HD_PLANE + (wave * 4) * HP_W + c;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (half * HD_NC >= p.Cout) break;          // (uniform: nothing but zeros in the second 16 feature maps)
        if (half) __syncthreads();
        // stage feature maps [16 half, 16 half + 16) of the masked gradient patch as planes; zero outside the image and beyond Cout
        for (int i = tid; i < (HD_H + 4) * HP_W * 4; i += 256) {
            const int quad = i & 3, pix = i >> 2;
            const int py = pix / HP_W, px = pix - py * HP_W;
            const int iy = oy0 - 2 + py, ix = ox0 - 2 + px, n0 = half * HD_NC + quad * 4;
            float4 v = f4zero();
            if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W && n0 < p.Cout) {
                const size_t gp = ((size_t)b * p.H + iy) * p.W + ix;
                v = ld4(p.g + gp * p.ldg + n0);
                if (p.gm) {
                    const float4 m = ld4(p.gm + gp * p.ldgm + n0);
                    v = make_float4(m.x > 0.f ? v.x : 0.f, m.y > 0.f ? v.y : 0.f, m.z > 0.f ? v.z : 0.f, m.w > 0.f ? v.w : 0.f);
                }
                if (n0 + 1 >= p.Cout) v.y = 0.f;    // (the lanes between Cout and the pitch hold whatever the caller left there)
                if (n0 + 2 >= p.Cout) v.z = 0.f;
                if (n0 + 3 >= p.Cout) v.w = 0.f;
            }
            float *d = P + (quad * 4) * HD_PLANE + pix;
            d[0] = v.x, d[HD_PLANE] = v.y, d[2 * HD_PLANE] = v.z, d[3 * HD_PLANE] = v.w;
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 25; ++tap) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int off = q * 4 * HD_PLANE + (4 - tap / 5) * HP_W + 4 - tap % 5;
                float a[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) a[t] = pa[off + (t >> 1) * HP_W + 16 * (t & 1)];
#pragma unroll
                for (int t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], wreg[tap * 8 + half * 4 + q], acc[t], 0, 0, 0);
            }
        }
    }

    if (c >= p.ld) return;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int oy = oy0 + wave * 4 + (t >> 1);
        if (oy >= p.H) continue;
        float *orow = p.dx + ((size_t)b * p.H + oy) * p.W * p.ld + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ox = ox0 + 16 * (t & 1) + 4 * k + r;
            if (ox < p.W) orow[(size_t)ox * p.ld] = c < p.Cin ? acc[t][r] : 0.f;       // lanes Cin..ld-1: zero
        }
    }
}

// OIHW [Cout][Cin][5][5] -> [K pad][32]: row k = tap*Cin + c, zero rows / columns beyond
__global__ void pack_weight_head_kernel(const float *__restrict__ w, float *__restrict__ wp, int Cout, int Cin, int rows) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * 32) return;
    const int n = i & 31, k = i >> 5;
    const int tap = k / Cin, c = k - tap * Cin;
    wp[i] = (tap < 25 && n < Cout) ? w[((size_t)n * Cin + c) * 25 + tap] : 0.f;
}

int launch_head(const ramnet_conv_desc &d, hipStream_t st) {
    RAMNET_CHECK_ARG(d.ntaps == 25 && d.stride == 1 && d.in_mode == RAMNET_IN_PLAIN);
    for (int t = 0; t < 25; ++t) RAMNET_CHECK_ARG(d.dy[t] == t / 5 - 2 && d.dx[t] == t % 5 - 2 && d.wtap[t] == t);   // dense padded 5x5
    RAMNET_CHECK_ARG(d.head_cin >= 1 && d.head_cin <= d.C0 && head_channels_ok(d.head_cin) && d.Cout <= 32);
    RAMNET_CHECK_ARG(d.Ho == d.Hin && d.Wo == d.Win && d.HoF == d.Ho && d.WoF == d.Wo && d.osy == 1 && d.osx == 1 && d.ooy == 0 && d.oox == 0);
    RAMNET_CHECK_ARG((d.epi == RAMNET_EPI_RELU || d.epi == RAMNET_EPI_LINEAR) && d.beta == 0.f && d.frame == 0 && d.out_s2d == 0);
    RAMNET_CHECK_ARG(((uintptr_t)d.x0 & 15) == 0 && d.ld0 % 4 == 0 && (d.head_cin <= 4 || d.C0 >= 8) && (d.head_cin <= 8 || d.C0 >= 12));
    HeadFwdParams q;
    q.x = d.x0, q.wp = d.w, q.bias = d.bias, q.out = d.out;
    q.ld = d.ld0, q.ldo = d.ldo, q.B = d.B, q.H = d.Hin, q.W = d.Win, q.Cout = d.Cout, q.relu = d.epi == RAMNET_EPI_RELU;
    q.tiles_x = cdiv(d.Wo, HT_W), q.tiles_y = cdiv(d.Ho, HF_H);
    const dim3 grid(q.tiles_x * q.tiles_y * d.B);
    note_kernel("conv_head_fwd_kernel<%d>", d.head_cin);      // (head_channels_ok: 1, 3, 5 or 10, one instantiation each)
    if (d.head_cin == 1) hipLaunchKernelGGL(conv_head_fwd_kernel<1>, grid, dim3(256), 0, st, q);
    else if (d.head_cin == 3) hipLaunchKernelGGL(conv_head_fwd_kernel<3>, grid, dim3(256), 0, st, q);
    else if (d.head_cin == 10) hipLaunchKernelGGL(conv_head_fwd_kernel<10>, grid, dim3(256), 0, st, q);
    else hipLaunchKernelGGL(conv_head_fwd_kernel<5>, grid, dim3(256), 0, st, q);
    RAMNET_LAUNCH_CHECK();
    return 0;
}

}  // namespace ramnet

using namespace ramnet;

extern "C" size_t ramnet_packed_weight_elems_head(int Cin) { return (size_t)((25 * Cin + 1) / 2 * 2) * 32; }

extern "C" int ramnet_head_supported(int Cin, int Cout) { return head_channels_ok(Cin) && Cout >= 1 && Cout <= 32; }

extern "C" int ramnet_head_dgrad(const float *dy, int ldg, const float *y, int ldgm, const float *w, float *dx, int ld, int B, int H, int W, int Cin,
                                 int Cout, void *stream) {
    RAMNET_CHECK_ARG(dy && w && dx && B >= 1 && H >= 1 && W >= 1);
    RAMNET_CHECK_ARG(ramnet_head_supported(Cin, Cout) && ld == roundup(Cin, 4));
    RAMNET_CHECK_ARG(ldg % 4 == 0 && ldg >= roundup(Cout, 4) && ((uintptr_t)dy & 15) == 0);
    RAMNET_CHECK_ARG(y == nullptr || (ldgm % 4 == 0 && ldgm >= roundup(Cout, 4) && ((uintptr_t)y & 15) == 0));
    RAMNET_CHECK_ARG(((uintptr_t)w & 3) == 0 && ((uintptr_t)dx & 3) == 0);
    const long tiles = (long)cdiv(W, HT_W) * cdiv(H, HD_H) * B;      // (pixel indices are 64-bit in the kernel: the grid is the one limit)
    RAMNET_CHECK_ARG(tiles <= 0x7fffffffL);
    HeadDgradParams q;
    q.g = dy, q.gm = y, q.w = w, q.dx = dx;
    q.ldg = ldg, q.ldgm = y ? ldgm : 0, q.ld = ld, q.B = B, q.H = H, q.W = W, q.Cin = Cin, q.Cout = Cout;
    q.tiles_x = cdiv(W, HT_W), q.tiles_y = cdiv(H, HD_H);
    note_kernel("conv_head_dgrad_kernel");
    hipLaunchKernelGGL(conv_head_dgrad_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, q);
    RAMNET_LAUNCH_CHECK();
    return 0;
}

extern "C" int ramnet_pack_weight_head(const float *w, float *wp, int Cout, int Cin, void *stream) {
    RAMNET_CHECK_ARG(w && wp && ramnet_head_supported(Cin, Cout));
    const int rows = (25 * Cin + 1) / 2 * 2;
    hipLaunchKernelGGL(pack_weight_head_kernel, dim3(cdiv(rows * 32, 256)), dim3(256), 0, (hipStream_t)stream, w, wp, Cout, Cin, rows);
    RAMNET_LAUNCH_CHECK();
    return 0;
}
