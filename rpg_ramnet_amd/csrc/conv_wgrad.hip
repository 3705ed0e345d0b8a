// Backward-weights (+bias) of every convolution on the RAM-Net path, gfx950 fp32 MFMA.
//
//   dW[t][c][n] += sum_{b,oy,ox} in(b, oy*s+dy[t], ox*s+dx[t], c) * g(b, oy, ox, n)
//
// GEMM view: M = input channel (32 per workgroup), N = output channel (64 per workgroup), K = pixels.
// A workgroup walks TH x 16 pixel tiles; per tile it stages the input patch (tile + halo, 32
// channels; same fused loaders as the forward kernel: concat, h*r, bilinear x2 (+skip), ReLU mask)
// and the 128 x 64 gradient tile in LDS, then every filter tap is one 32x32 accumulator whose A
// operand is the patch shifted by the tap offset.  The taps x 2 N-halves accumulators are spread
// over the 4 waves (wave w: N-half w&1, taps (w>>1), (w>>1)+2, ...) and stay in registers for the
// whole pixel range of the workgroup; partial sums of the pixel splits meet in a [tap][Cin][Cout]
// fp32 workspace through coalesced atomic adds.  The bias gradient (column sums of g) rides along.
#include <stdlib.h>
#include "common.hpp"
#include "conv_plan.hpp"

namespace ramnet {

struct WgradDerived {
    InSrc src;
    int PH, PW, dymin, dxmin;
    int TH;                         // pixel tile = TH x 16: 8, or 4 when two workgroups would not fit a CU's LDS (stride-2 5x5)
    int tiles_x, tiles_y, ntiles;   // pixel tiles per image / total
    int tpm, ntt;                   // taps per 32-row accumulator tile (Cin < 32 packs several taps), number of tap tiles
    int toff[25];
    int gsy, gsx, goy, gox, HoG, WoG;   // addressing of dout / gmask (ramnet_wgrad_desc)
};

#define WGRAD_SLAB 0
#define WGRAD_KERNEL(name) name
#include "conv_wgrad_kernel.hpp"
#undef WGRAD_SLAB
#undef WGRAD_KERNEL
#define WGRAD_SLAB 1
#define WGRAD_KERNEL(name) name##_slab
#include "conv_wgrad_kernel.hpp"
#undef WGRAD_SLAB
#undef WGRAD_KERNEL

// Host-only shape of a RAMNET_ALGO_DIRECT launch: which kernel takes it (wide: conv_wgrad_kernel<9,2,2>, 64 x 64 channels per workgroup;
// narrow: 32 x 32; else 32 x 64), its channel-block grid, and the splits its slab form uses at most (conv_plan.hpp)
struct WgradShape {
    bool wide, narrow;
    int wck, wbn, gy, gz, cap;
};

template <int MAXT, int NSUB, int CSUB = 1, bool SLAB = false>
static int launch_wgrad(const ramnet_wgrad_desc &d, const WgradDerived &q, const WgradShape &s, hipStream_t st) {
    if (!SLAB && d.dw_slabs > 0) return launch_wgrad<MAXT, NSUB, CSUB, true>(d, q, s, st);
    auto kern = SLAB ? conv_wgrad_kernel_slab<MAXT, NSUB, CSUB> : conv_wgrad_kernel<MAXT, NSUB, CSUB>;
    size_t lds = ((size_t)q.PH * q.PW * s.wck + q.TH * TWID * s.wbn) * sizeof(float);
    RAMNET_FULL_LDS((kern));
    if (lds > 160 * 1024) {
        set_error("wgrad patch does not fit LDS (%zu bytes)", lds);
        return RAMNET_E_UNSUPPORTED;
    }
    // one resident wave of workgroups (256 CUs x blocks/CU the register budget admits): fewer pixel splits = fewer
    // atomic partial-sum merges, and every CU still gets an equal share
    const int splits = SLAB ? wgrad_splits(s.cap, q.ntiles, d.dw_slabs) : wgrad_splits(wgrad_direct_own(s.gy * s.gz), q.ntiles, 0);
    note_kernel(SLAB ? "conv_wgrad_kernel_slab<%d,%d,%d>" : "conv_wgrad_kernel<%d,%d,%d>", MAXT, NSUB, CSUB);
    hipLaunchKernelGGL(kern, dim3(splits, s.gy, s.gz), dim3(256), lds, st, d, q);
    RAMNET_LAUNCH_CHECK();
    return 0;
}

}  // namespace ramnet

using namespace ramnet;

static WgradShape wgrad_derive(const ramnet_wgrad_desc &d, WgradDerived &q);

extern "C" int ramnet_wgrad_launch(const ramnet_wgrad_desc *dp, void *stream) {
    RAMNET_CHECK_ARG(dp != nullptr);
    const ramnet_wgrad_desc &d = *dp;
    RAMNET_CHECK_ARG(d.x0 && d.dout && d.dw);
    RAMNET_CHECK_ARG(d.ntaps >= 1 && d.ntaps <= 25 && (d.stride == 1 || d.stride == 2));
    RAMNET_CHECK_ARG(d.B > 0 && d.Ho > 0 && d.Wo > 0 && d.Cout > 0 && d.Cout % 4 == 0 && d.ldg % 4 == 0);
    RAMNET_CHECK_ARG(d.C0 > 0 && d.C0 % 4 == 0 && d.ld0 % 4 == 0);
    const bool cat = d.in_mode == RAMNET_IN_CAT || d.in_mode == RAMNET_IN_CAT_MUL;
    if (cat) RAMNET_CHECK_ARG(d.x1 && d.C1 > 0 && d.C1 % 4 == 0 && d.ld1 % 4 == 0);
    if (d.in_mode == RAMNET_IN_CAT_MUL || d.in_mode == RAMNET_IN_RELUMASK) RAMNET_CHECK_ARG(d.xm && d.ldm % 4 == 0);
    if (d.in_mode == RAMNET_IN_UP2X_SKIP) RAMNET_CHECK_ARG(d.x1 && d.ld1 % 4 == 0);
    if (d.gmask) RAMNET_CHECK_ARG(d.ldgm % 4 == 0);
    // every leading dimension covers the channels the loaders read through it (ramnet_hip.h)
    RAMNET_CHECK_ARG(d.ld0 >= d.C0 && d.ldg >= d.Cout && (!d.gmask || d.ldgm >= d.Cout));
    if (cat) RAMNET_CHECK_ARG(d.ld1 >= d.C1);
    if (d.in_mode == RAMNET_IN_CAT_MUL) RAMNET_CHECK_ARG(d.ldm >= d.C1);
    if (d.in_mode == RAMNET_IN_RELUMASK) RAMNET_CHECK_ARG(d.ldm >= d.C0);
    RAMNET_CHECK_ARG(d.nseg >= 0 && (d.nseg == 0 || d.algo == RAMNET_ALGO_WINOGRAD_2X4));       // multi-segment launches: F(2x4,3x3) only
    if (d.algo == RAMNET_ALGO_WINOGRAD24 || d.algo == RAMNET_ALGO_WINOGRAD24_2X3) return launch_wgrad_wino24(d, (hipStream_t)stream);
    const bool gdense = d.gsy == 0 && d.gsx == 0 && d.goy == 0 && d.gox == 0 && d.HoG == 0 && d.WoG == 0;
    if (!gdense) RAMNET_CHECK_ARG(d.gsy >= 1 && d.gsx >= 1 && d.goy >= 0 && d.gox >= 0 && (d.Ho - 1) * d.gsy + d.goy < d.HoG &&
                                  (d.Wo - 1) * d.gsx + d.gox < d.WoG && d.algo == RAMNET_ALGO_DIRECT);
    if (d.algo == RAMNET_ALGO_WINOGRAD) return launch_wgrad_wino(d, (hipStream_t)stream);
    if (d.algo == RAMNET_ALGO_WINOGRAD_2X4) return launch_wgrad_wino6(d, (hipStream_t)stream);
    if (d.algo == RAMNET_ALGO_DIRECT_SPLIT) {
        RAMNET_CHECK_ARG(gdense);
        return launch_wgrad_dsplit(d, (hipStream_t)stream);
    }
    if (d.algo == RAMNET_ALGO_HEAD) {
        RAMNET_CHECK_ARG(gdense);
        return launch_head_wgrad(d, (hipStream_t)stream);
    }
    RAMNET_CHECK_ARG(d.algo == RAMNET_ALGO_DIRECT && d.in_mode != RAMNET_IN_S2D);

    WgradDerived q;
    const WgradShape s = wgrad_derive(d, q);
    hipStream_t st = (hipStream_t)stream;
    if (s.narrow) {                                 // WBN = 32: tap tiles spread over 4 waves
        const int per_wave = cdiv(q.ntt, 4);
        if (per_wave <= 1) return launch_wgrad<1, 1>(d, q, s, st);
        if (per_wave <= 3) return launch_wgrad<3, 1>(d, q, s, st);
        if (per_wave <= 4) return launch_wgrad<4, 1>(d, q, s, st);     // 16 taps: one parity of the folded upsample-conv
        return launch_wgrad<7, 1>(d, q, s, st);
    }
    if (s.wide) return launch_wgrad<9, 2, 2>(d, q, s, st);
    const int per_wave = cdiv(q.ntt, 2);            // WBN = 64: tap tiles spread over 2 wave pairs
    if (per_wave <= 1) return launch_wgrad<1, 2>(d, q, s, st);
    if (per_wave <= 5) return launch_wgrad<5, 2>(d, q, s, st);
    return launch_wgrad<13, 2>(d, q, s, st);
}

// Geometry of a RAMNET_ALGO_DIRECT launch (host arithmetic only): pixel tiles, patch, tap tiles, and the shape of the kernel that takes it
static WgradShape wgrad_derive(const ramnet_wgrad_desc &d, WgradDerived &q) {
    const bool gdense = d.gsy == 0 && d.gsx == 0 && d.goy == 0 && d.gox == 0 && d.HoG == 0 && d.WoG == 0;
    fill_in_src(d, q.src);
    int dymin = 127, dymax = -127, dxmin = 127, dxmax = -127;
    for (int t = 0; t < d.ntaps; ++t) {
        dymin = d.dy[t] < dymin ? d.dy[t] : dymin, dymax = d.dy[t] > dymax ? d.dy[t] : dymax;
        dxmin = d.dx[t] < dxmin ? d.dx[t] : dxmin, dxmax = d.dx[t] > dxmax ? d.dx[t] : dxmax;
    }
    q.dymin = dymin, q.dxmin = dxmin;
    q.gsy = gdense ? 1 : d.gsy, q.gsx = gdense ? 1 : d.gsx, q.goy = d.goy, q.gox = d.gox;
    q.HoG = gdense ? d.Ho : d.HoG, q.WoG = gdense ? d.Wo : d.WoG;
    // two co-resident workgroups per CU hide each other's staging: halve the pixel tile when a full one needs > 80 KB
    q.TH = 8;
    // -> conv_wgrad_kernel<9,2,2>; needs >= 4 pixel tiles per workgroup to amortise its 9 x 64 x 64 atomic epilogue
    const long tiles8 = (long)cdiv(d.Wo, TWID) * cdiv(d.Ho, 8) * d.B;
    const bool wide = d.ntaps <= 9 && d.ntaps > 1 && q.src.Cin >= 64 && d.Cout > 32 &&
                      tiles8 * cdiv(q.src.Cin, 64) * cdiv(d.Cout, 64) >= 2048;
    const int wck = wide ? 64 : WCK;
    if (((7 * d.stride + (dymax - dymin) + 1) * ((TWID - 1) * d.stride + (dxmax - dxmin) + 1) * wck + 128 * 32) * 4 > 80 * 1024) q.TH = 4;
    q.PH = (q.TH - 1) * d.stride + (dymax - dymin) + 1;
    q.PW = (TWID - 1) * d.stride + (dxmax - dxmin) + 1;
    q.tiles_x = cdiv(d.Wo, TWID), q.tiles_y = cdiv(d.Ho, q.TH);
    q.ntiles = q.tiles_x * q.tiles_y * d.B;
    for (int t = 0; t < d.ntaps; ++t) q.toff[t] = ((d.dy[t] - dymin) * q.PW + (d.dx[t] - dxmin)) * wck;
    // Cin < 32: several taps share one 32-row accumulator tile (head convs: 5 or 1 input channels)
    q.tpm = 1;
    if (q.src.Cin <= 16) q.tpm = q.src.Cin <= 4 ? 8 : q.src.Cin <= 8 ? 4 : 2;
    q.ntt = cdiv(d.ntaps, q.tpm);
    // measured (profiles/r01_*layers*): 5x5 layers run 1.5x faster with WBN = 32 (7 tiles/wave, 2 workgroups/CU) than with
    // WBN = 64 (13 tiles/wave, 1 workgroup/CU); 3x3 layers prefer WBN = 64 (5 tiles/wave)
    WgradShape s{wide, d.Cout <= 32 || d.ntaps > 9};
    s.wck = wck, s.wbn = s.narrow ? 32 : 64;
    s.gy = cdiv(q.src.Cin, s.wck), s.gz = cdiv(d.Cout, s.wbn), s.cap = wgrad_direct_cap(s.gy * s.gz);
    return s;
}

// Can the launch of d->algo address its operands (the size guards of that launch alone, nothing structural)?  Quiet.
extern "C" int ramnet_wgrad_addressable(const ramnet_wgrad_desc *dp) {
    if (dp == nullptr || dp->B < 1 || dp->Hin < 1 || dp->Win < 1) return 0;
    switch (dp->algo) {
    case RAMNET_ALGO_WINOGRAD:
    case RAMNET_ALGO_WINOGRAD_2X4: return wgrad_offsets32(*dp, true) == 0;
    case RAMNET_ALGO_WINOGRAD24:
    case RAMNET_ALGO_WINOGRAD24_2X3: return fold_wgrad_addressable(*dp) ? 1 : 0;
    default: return 1;          // direct, direct-split, head: 64-bit pixel indices
    }
}

// Largest number of splits a launch of this descriptor's algorithm and shape can use in its slab form (ramnet_hip.h)
extern "C" int ramnet_wgrad_slabs(const ramnet_wgrad_desc *dp) {
    if (dp == nullptr) return 0;
    const ramnet_wgrad_desc &d = *dp;
    if (d.B < 1 || d.Ho < 1 || d.Wo < 1 || d.Cout < 1 || d.C0 < 1) return 0;
    InSrc in;
    fill_in_src(d, in);
    const int Cin = in.Cin;
    switch (d.algo) {
    case RAMNET_ALGO_WINOGRAD24:
    case RAMNET_ALGO_WINOGRAD24_2X3: return wgrad_wino24_splits(d);
    case RAMNET_ALGO_HEAD: return head_wgrad_slabs(d);
    case RAMNET_ALGO_WINOGRAD: return ramnet_wgrad_wino_slabs(Cin, d.Cout);
    case RAMNET_ALGO_WINOGRAD_2X4: return ramnet_wgrad_wino2x4_slabs(Cin, d.Cout);
    case RAMNET_ALGO_DIRECT_SPLIT: return ramnet_wgrad_dsplit_slabs(Cin, d.Cout);
    case RAMNET_ALGO_DIRECT: break;
    default: return 0;
    }
    if (d.ntaps < 1 || d.ntaps > 25 || (d.stride != 1 && d.stride != 2) || d.in_mode == RAMNET_IN_S2D) return 0;
    WgradDerived q;
    const WgradShape s = wgrad_derive(d, q);
    return wgrad_splits(s.cap, q.ntiles, 0);
}
