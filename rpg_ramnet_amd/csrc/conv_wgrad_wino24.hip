// Backward-weights of the folded upsample-conv (decoders, statenet.py:305-308) in the Winograd F(2x2,4x4) domain on gfx950:
//     dU_cls[pos][ci][co] = sum_tiles V_cls[pos][tile][ci] * Z_cls[pos][tile][co],   V = B^T d B,   Z = A g A^T
// with d the 5x5 window of the replicate-padded low-res input of parity class cls = (py, px) and g the 2x2 tile of that
// parity's sub-grid of dy (* ReLU mask); the 4x4 parity-filter gradient is dW4 = G^T dU G (ops.ConvParam._finalize_fold).
// 25 GEMMs per class with M = input channel, N = output channel, K = tiles on v_mfma_f32_32x32x2_f32: 25 instead of 64
// multiplies per tile and channel pair (csrc/conv_wino24.hip has the forward and the matrices).
//
// A workgroup (8 waves) owns 32 x 64 channels of one class and walks batches of 8 tiles: every thread loads the window of one
// (tile, input channel) and the 2x2 gradients of one (tile, output channel) straight from global memory (lanes along channels:
// coalesced), transforms them in registers and writes V[25][8][32] / Z[25][8][64] to LDS (double-buffered, one barrier per
// batch).  Wave (position group of 7/6/6/6, channel half) accumulates 32 x 32 per position (112 VGPRs) over its whole tile range;
// loads and transforms of the next batches are issued between the MFMAs; tile splits meet by atomics in the [4][25][Cin][Cout]
// workspace; the bias gradient rides along.  conv_wgrad_wino24_kernel_2x3 below is the F(2x3,4x4) form of the same launch
// (RAMNET_ALGO_WINOGRAD24_2X3, picked by wgrad_wino24_variant).
#include <stdlib.h>
#include "common.hpp"
#include "conv_plan.hpp"

namespace ramnet {

constexpr int G24_T = 8;                          // tiles per batch
// channels per workgroup: 32 input x 64 output, or (WCI, for 32-output-channel layers) 64 input x 32 output

struct Wgrad24Params {
    const float *x, *g, *gm;
    float *dw, *dbias;
    int ldx, ldg, ldgm, Hp, Wp, H2, W2, Hc, Wc, Cin, Cout, tiles_x, tiles_y, ntiles, nbatch, ncob;
    size_t xbytes, gbytes, gmbytes;       // extents of x / g / gm (buffer addressing: < WOOB, checked on the host)
};

constexpr int G23_T = 6, G23_NP = 30;             // F(2x3,4x4): tiles per batch, positions

#define WG24_SLAB 0
#define WG24_KERNEL(name) name
#include "conv_wgrad_wino24_kernels.hpp"
#undef WG24_SLAB
#undef WG24_KERNEL
#define WG24_SLAB 1
#define WG24_KERNEL(name) name##_slab
#include "conv_wgrad_wino24_kernels.hpp"
#undef WG24_SLAB
#undef WG24_KERNEL

// Bias gradient of the slab form: dbias[s][n] += sum of g (* (gm > 0)) over rows [s * rows / S, (s + 1) * rows / S) of the `rows` = B * 2H
// full-resolution gradient rows of `W2` pixels.  Workgroup (s, 32-channel block) alone touches its 32 floats; thread (pixel lane, channel)
// adds its pixels in index order into four interleaved sums, the eight pixel lanes meet in LDS in lane order: the same bits on every launch.
__global__ void __launch_bounds__(256) wgrad24_dbias_slab_kernel(const float *__restrict__ g, const float *__restrict__ gm, float *dbias, int ldg,
                                                                 int ldgm, int Cout, long rows, int W2) {
    __shared__ float red[8][32];
    const int c = threadIdx.x & 31, pl = threadIdx.x >> 5, n = blockIdx.y * 32 + c;
    const long S = gridDim.x, s = blockIdx.x;
    const long p0 = s * rows / S * W2, p1 = (s + 1) * rows / S * W2;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (n < Cout) {
        for (long pix = p0 + pl; pix < p1; pix += 32) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long q = pix + 8 * i;
                if (q < p1) {
                    float v = g[q * ldg + n];
                    if (gm != nullptr) v = gm[q * ldgm + n] > 0.f ? v : 0.f;
                    a[i] += v;
                }
            }
        }
    }
    red[pl][c] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    if (pl == 0 && n < Cout) {
        float t = 0.f;
        for (int i = 0; i < 8; ++i) t += red[i][c];
        dbias[s * Cout + n] += t;
    }
}

// tile splits of a launch (the slabs its slab form uses: ramnet_wgrad_slabs); 0 when the kernel does not take the descriptor
int wgrad_wino24_splits(const ramnet_wgrad_desc &d) {
    const bool f23 = d.algo == RAMNET_ALGO_WINOGRAD24_2X3;
    const bool wci = d.Cout % 64 != 0;
    const int ci = wci ? 64 : 32, co = wci ? 32 : 64;
    if (d.C0 <= 0 || d.C0 % ci != 0 || d.Cout <= 0 || d.Cout % 32 != 0 || d.Ho < 2 || d.Wo < 2 || d.B < 1) return 0;
    const int ntiles = cdiv(d.Wo, f23 ? 3 : 2) * cdiv(d.Ho, 2) * d.B, nbatch = cdiv(ntiles, f23 ? G23_T : G24_T);
    int splits = 256 / ((d.C0 / ci) * cdiv(d.Cout, co) * 4);                   // (128 / 384 workgroups measured the same training step)
    if (splits > nbatch) splits = nbatch;
    return splits < 1 ? 1 : splits;
}

int launch_wgrad_wino24(const ramnet_wgrad_desc &d, hipStream_t st) {
    // x0 = replicate-padded low-res input [B][Hin = H+4][Win = W+4][C0]; dout / gmask = [B][HoG = 2H][WoG = 2W][Cout]; Ho, Wo = H, W
    const bool f23 = d.algo == RAMNET_ALGO_WINOGRAD24_2X3;       // 2 x 3 tiles in batches of 6, dw = [4][30][C0][Cout]
    const bool wci = d.Cout % 64 != 0;           // 32-output-channel layers: 64 x 32 channels per workgroup
    const int G24_CI = wci ? 64 : 32, G24_CO = wci ? 32 : 64;
    RAMNET_CHECK_ARG(d.in_mode == RAMNET_IN_PLAIN && d.stride == 1 && d.C0 % G24_CI == 0 && d.Cout % 32 == 0);
    RAMNET_CHECK_ARG(d.Hin == d.Ho + 4 && d.Win == d.Wo + 4 && d.HoG == 2 * d.Ho && d.WoG == 2 * d.Wo && d.Ho >= 2 && d.Wo >= 2);
    Wgrad24Params q;
    q.x = d.x0, q.g = d.dout, q.gm = d.gmask, q.dw = d.dw, q.dbias = d.dbias;
    q.ldx = d.ld0, q.ldg = d.ldg, q.ldgm = d.ldgm, q.Hp = d.Hin, q.Wp = d.Win, q.H2 = d.HoG, q.W2 = d.WoG, q.Hc = d.Ho, q.Wc = d.Wo;
    q.Cin = d.C0, q.Cout = d.Cout;
    q.xbytes = fold_wgrad_x_bytes(d), q.gbytes = fold_wgrad_g_bytes(d, d.ldg);
    q.gmbytes = d.gmask ? fold_wgrad_g_bytes(d, d.ldgm) : 0;
    // per-lane 32-bit byte offsets; a tile past the last one may stand up to one grid stride of images beyond the tensor
    RAMNET_CHECK_ARG(2 * q.xbytes < WOOB && 2 * q.gbytes < WOOB && 2 * q.gmbytes < WOOB);
    const int tiles_per_batch = f23 ? G23_T : G24_T;
    q.tiles_x = cdiv(d.Wo, f23 ? 3 : 2), q.tiles_y = cdiv(d.Ho, 2), q.ntiles = q.tiles_x * q.tiles_y * d.B, q.nbatch = cdiv(q.ntiles, tiles_per_batch);
    q.ncob = cdiv(d.Cout, G24_CO);
    const int gy = d.C0 / G24_CI, gz = q.ncob * 4;
    const bool slab = d.dw_slabs > 0;                // split s owns slab s of dw [S][4][25 | 30][C0][Cout] and of dbias [S][Cout]
    int splits = wgrad_wino24_splits(d);
    if (slab && splits > d.dw_slabs) splits = d.dw_slabs;
    const size_t lds = (size_t)2 * (f23 ? G23_NP : 25) * tiles_per_batch * (32 + 64) * sizeof(float);
    const dim3 grid(splits, gy, gz);
    auto go = [&](auto kern) -> int {
        RAMNET_FULL_LDS((kern));
        note_kernel(slab ? (f23 ? "conv_wgrad_wino24_kernel_2x3_slab<%d,%d>" : "conv_wgrad_wino24_kernel_slab<%d,%d>")
                         : (f23 ? "conv_wgrad_wino24_kernel_2x3<%d,%d>" : "conv_wgrad_wino24_kernel<%d,%d>"), d.gmask ? 1 : 0, (int)wci);
        hipLaunchKernelGGL(kern, grid, dim3(512), lds, st, q);
        return 0;
    };
    if (slab) {
        const int rc = f23 ? (wci ? (d.gmask ? go(conv_wgrad_wino24_kernel_2x3_slab<true, true>) : go(conv_wgrad_wino24_kernel_2x3_slab<false, true>))
                                  : (d.gmask ? go(conv_wgrad_wino24_kernel_2x3_slab<true, false>) : go(conv_wgrad_wino24_kernel_2x3_slab<false, false>)))
                     : wci ? (d.gmask ? go(conv_wgrad_wino24_kernel_slab<true, true>) : go(conv_wgrad_wino24_kernel_slab<false, true>))
                           : (d.gmask ? go(conv_wgrad_wino24_kernel_slab<true, false>) : go(conv_wgrad_wino24_kernel_slab<false, false>));
        if (rc) return rc;
        if (d.dbias != nullptr)
            hipLaunchKernelGGL(wgrad24_dbias_slab_kernel, dim3(splits, cdiv(d.Cout, 32)), dim3(256), 0, st, d.dout, d.gmask, d.dbias, d.ldg, d.ldgm,
                               d.Cout, (long)d.B * d.HoG, d.WoG);
        RAMNET_LAUNCH_CHECK();
        return 0;
    }
    const int rc = f23 ? (wci ? (d.gmask ? go(conv_wgrad_wino24_kernel_2x3<true, true>) : go(conv_wgrad_wino24_kernel_2x3<false, true>))
                              : (d.gmask ? go(conv_wgrad_wino24_kernel_2x3<true, false>) : go(conv_wgrad_wino24_kernel_2x3<false, false>)))
                 : wci ? (d.gmask ? go(conv_wgrad_wino24_kernel<true, true>) : go(conv_wgrad_wino24_kernel<false, true>))
                       : (d.gmask ? go(conv_wgrad_wino24_kernel<true, false>) : go(conv_wgrad_wino24_kernel<false, false>));
    if (rc) return rc;
    RAMNET_LAUNCH_CHECK();
    return 0;
}

// Does this RAMNET_ALGO_WINOGRAD24 backward-weights launch run F(2x3,4x4) (RAMNET_ALGO_WINOGRAD24_2X3)?  force: every launch the kernel takes.
// Otherwise the launches whose workgroups walk at least 24 batches of 6 tiles each: the fixed part of a launch (accumulator set-up, prologue,
// 30 instead of 25 positions of atomic joins) is larger on F(2x3) and the part per batch smaller.  In the isolated sweep of the three decoder
// layers over batch 1-32 (tools/bench_fold23_wgrad.py, profiles/fold23_wgrad_sweep.jsonl: about 10 batches per workgroup and image on all
// three) F(2x3) is 2-5 % slower at batch 1, 1-3 % faster at batch 2 (left on F(2x2): a tie), 6-7 % faster at batch 3 and 18-33 % at batch 16.
int wgrad_wino24_variant(const ramnet_wgrad_desc &d, int force) {
    if (d.algo != RAMNET_ALGO_WINOGRAD24 || d.in_mode != RAMNET_IN_PLAIN || d.stride != 1 || d.Ho < 2 || d.Wo < 2 || d.B < 1) return 0;
    const bool wci = d.Cout % 64 != 0;
    const int ci = wci ? 64 : 32, co = wci ? 32 : 64;
    if (d.C0 % ci != 0 || d.Cout % 32 != 0) return 0;
    if (force) return 1;
    const long nbatch = ((long)cdiv(d.Wo, 3) * cdiv(d.Ho, 2) * d.B + G23_T - 1) / G23_T;
    const int per_split = 256 / ((d.C0 / ci) * cdiv(d.Cout, co) * 4);                       // (launch_wgrad_wino24)
    return nbatch >= 24L * (per_split < 1 ? 1 : per_split) ? 1 : 0;
}

}  // namespace ramnet

extern "C" int ramnet_fold_wgrad_variant(const ramnet_wgrad_desc *d, int force) { return d ? ramnet::wgrad_wino24_variant(*d, force) : 0; }
