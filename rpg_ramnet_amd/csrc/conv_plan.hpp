// Host side of the 3x3 launchers (conv_wino.hip, conv_wino6.hip, conv_wino6s.hip, conv_wgrad_wino.hip, conv_wgrad_wino6.hip,
// conv_wgrad_dsplit.hip): what a launcher reads off its descriptor before it picks a template instantiation — the logical input, the tap
// window, the conditions of the channel-quad epilogues, the XCD groups, the 32-bit offsets — and the ONE plan of an F(2x4,3x3) launch,
// which launch_wino6 / launch_wino6s execute and wino6_eligible asks without launching.  For the backward-weights launchers (those three
// and conv_wgrad.hip): the one structural check of the 3x3 families, and the split rule — per family the own figure and the cap its
// ramnet_wgrad_*_slabs query answers, the clamp chain (wgrad_splits) and the XCD step (wgrad_xcd_splits) that launcher and query both
// call —, the (XMK, GM) dispatch and the unpack entry.  No device code besides the blocked-workspace address of the two unpack kernels;
// nothing here allocates or formats a string unless a check fails.
#pragma once
#include <stdlib.h>
#include <type_traits>
#include "conv_wino_common.hpp"

namespace ramnet {

// RAMNET_CHECK_ARG for plans that eligibility also asks: `quiet` (a bool in scope) = refuse without touching ramnet_last_error()
#define RAMNET_PLAN_CHECK(cond)                                                                       \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            if (!quiet) ramnet::set_error("%s:%d: bad argument: %s", __FILE__, __LINE__, #cond);      \
            return RAMNET_E_BADARG;                                                                   \
        }                                                                                             \
    } while (0)

constexpr int WKS = 16;                              // conv_wino6s.hip: input channels per chunk = K of one v_mfma_f32_32x32x16_bf16
constexpr int W6_BN = 64;                            // F(2x4,3x3): output channels per block of the packed weights (both kernels)
constexpr int W6_U_FLOATS = 24 * W6_BN * WK;         // conv_wino6.hip: weights of one (chunk, 64-channel block): 24 positions x 64 x 8 = 48 KB
constexpr int W6S_POS_BYTES = 2 * 3 * 1024;          // conv_wino6s.hip: B operands of one (row, position): [32-channel half 2][plane 3][lane 64][8 bf16]
constexpr int W6S_BLK_BYTES = 4 * 6 * W6S_POS_BYTES; // one (chunk, 64-channel block): 144 KB

inline int log2_exact(int v) {                       // log2 of a power of two, -1 for anything else
    int sh = 0;
    while ((1 << sh) < v) ++sh;
    return (1 << sh) == v ? sh : -1;
}

inline bool al16(const void *ptr) { return ptr == nullptr || ((uintptr_t)ptr & 15) == 0; }

// The logical input of a launch (ramnet_conv_desc / ramnet_wgrad_desc).  Space-to-depth view: Cin = the four parity groups, ld1 carries
// log2 C0 (the caller has checked that C0 is a power of two).
template <class Desc>
inline void fill_in_src(const Desc &d, InSrc &s) {
    const bool cat = d.in_mode == RAMNET_IN_CAT || d.in_mode == RAMNET_IN_CAT_MUL;
    s.x0 = d.x0, s.x1 = d.x1, s.xm = d.xm;
    s.ld0 = d.ld0, s.ld1 = d.ld1, s.ldm = d.ldm;
    s.C0 = d.C0, s.Cin = d.C0 + (cat ? d.C1 : 0);
    s.mode = d.in_mode, s.Hin = d.Hin, s.Win = d.Win;
    if (d.in_mode == RAMNET_IN_S2D) s.Cin = 4 * d.C0, s.ld1 = log2_exact(d.C0);
}

// Are the nine taps the dense 3x3 window — in any order (forward and backward-data: which weight slice each one reads is baked into the
// Winograd pack), or exactly in the forward order kh*3 + kw (backward-weights: the workspace rows follow it)?  (dy0, dx0) = its first tap.
inline bool taps_3x3(const int8_t *dy, const int8_t *dx, bool forward_order, int &dy0, int &dx0) {
    dy0 = 127, dx0 = 127;
    for (int t = 0; t < 9; ++t) {
        dy0 = dy[t] < dy0 ? dy[t] : dy0;
        dx0 = dx[t] < dx0 ? dx[t] : dx0;
    }
    unsigned seen = 0;
    for (int t = 0; t < 9; ++t) {
        const int a = dy[t] - dy0, c = dx[t] - dx0;
        if (a < 0 || a >= 3 || c < 0 || c >= 3 || (forward_order && a * 3 + c != t)) return false;
        seen |= 1u << (a * 3 + c);
    }
    return seen == 0x1ffu;
}

// Do all epilogue operands allow 16-byte channel-quad accesses?  o2 (the gates of a ConvLSTM cell) counts for F(2x2,3x3); the F(2x4,3x3)
// cell checks it in wino6_lstm_ok.
inline bool conv_vec4(const ramnet_conv_desc &d, bool with_o2) {
    return d.Cout % 4 == 0 && d.ldo % 4 == 0 && al16(d.out) && al16(d.bias) && (!d.o1 || (d.ldo1 % 4 == 0 && al16(d.o1))) &&
           (!d.e0 || (d.lde0 % 4 == 0 && al16(d.e0))) && (!d.e1 || (d.lde1 % 4 == 0 && al16(d.e1))) &&
           (!with_o2 || !d.o2 || (d.ldo2 % 4 == 0 && al16(d.o2)));
}

// out_s2d (backward-data of a stride-2 5x5 encoder over its space-to-depth view): what the epilogues need besides vec4
inline bool out_s2d_ok(const ramnet_conv_desc &d) {
    return d.out_s2d >= 8 && log2_exact(d.out_s2d) > 0 && d.Cout == 4 * d.out_s2d && d.epi == RAMNET_EPI_LINEAR && !d.bias && d.beta == 0.f &&
           d.HoF == 2 * d.Ho && d.WoF == 2 * d.Wo;
}

// log2 of the number of XCD-pinned channel-block groups, for weights that do not fit an L2: 2 groups above 3 MB, 4 above 12 MB (when
// nblk divides)
inline int xcd_groups(size_t wbytes, int nblk) {
    int xg = wbytes > (12u << 20) ? 2 : wbytes > (3u << 20) ? 1 : 0;
    while (xg > 0 && (nblk % (1 << xg)) != 0) --xg;
    return xg;
}

// The kernels address every tensor inside ONE image with 32-bit byte offsets below WOOB: the sources, and the epilogue's tensors
// (with_o2: the gates of a ConvLSTM cell too)
inline int check_offsets32(const ramnet_conv_desc &d, bool with_o2, bool quiet) {
    const unsigned long long px = (unsigned long long)d.Hin * d.Win * (d.in_mode == RAMNET_IN_S2D ? 4 : 1);
    int ldmax = d.ld0 > d.ld1 ? d.ld0 : d.ld1;
    ldmax = ldmax > d.ldm ? ldmax : d.ldm;
    RAMNET_PLAN_CHECK(px * ldmax * 4ull < (unsigned long long)WOOB);
    int lo = d.ldo > d.ldo1 ? d.ldo : d.ldo1;
    lo = lo > d.lde0 ? lo : d.lde0;
    lo = lo > d.lde1 ? lo : d.lde1;
    if (with_o2) lo = lo > d.ldo2 ? lo : d.ldo2;
    RAMNET_PLAN_CHECK((unsigned long long)d.HoF * d.WoF * lo * 4ull < (unsigned long long)WOOB);
    return 0;
}

// What the folded families (conv_wino24.hip, conv_wgrad_wino24.hip) address with 32-bit byte offsets into one buffer resource per tensor:
// the WHOLE x0 of a forward launch, of a PARITY4 backward-data launch below 2^30 (window elements outside the tensor are given offsets from
// 2^30 up), the packed weights; backward-weights: twice the bytes of x0 / dout / gmask below WOOB (a tile past the last one may stand up
// to one grid stride of images beyond the tensor).  One statement for the launchers and for ramnet_conv_addressable / ramnet_wgrad_addressable.
constexpr unsigned long long FOLD_X_LIMIT = 0xffffffffull, FOLD_DGRAD_X_LIMIT = 0x40000000ull, FOLD_W_LIMIT = 0x7fffffffull;
inline unsigned long long fold_x_bytes(const ramnet_conv_desc &d) { return (unsigned long long)d.B * d.Hin * d.Win * d.ld0 * sizeof(float); }
inline unsigned long long fold_w_bytes(const ramnet_conv_desc &d) {
    return (d.algo == RAMNET_ALGO_WINOGRAD24_2X3 ? 120ull : 100ull) * d.C0 * d.Cout * sizeof(float);
}
inline bool fold_conv_addressable(const ramnet_conv_desc &d) {
    return fold_x_bytes(d) < (d.in_mode == RAMNET_IN_PARITY4 ? FOLD_DGRAD_X_LIMIT : FOLD_X_LIMIT) && fold_w_bytes(d) < FOLD_W_LIMIT;
}
inline unsigned long long fold_wgrad_x_bytes(const ramnet_wgrad_desc &d) { return (unsigned long long)d.B * d.Hin * d.Win * d.ld0 * 4ull; }
inline unsigned long long fold_wgrad_g_bytes(const ramnet_wgrad_desc &d, int ld) { return (unsigned long long)d.B * d.HoG * d.WoG * ld * 4ull; }
inline bool fold_wgrad_addressable(const ramnet_wgrad_desc &d) {
    return 2 * fold_wgrad_x_bytes(d) < WOOB && 2 * fold_wgrad_g_bytes(d, d.ldg) < WOOB && (!d.gmask || 2 * fold_wgrad_g_bytes(d, d.ldgm) < WOOB);
}

// Workgroup tile of F(2x4,3x3) for an Ho x Wo map: 32 tiles of 2 x 4 pixels as 16 x 16 (TXG 4), 32 x 8 (TXG 2) or 8 x 32 (TXG 8),
// whichever pads the map least; returns the padded area.
inline long wino6_tile(int Ho, int Wo, int &txg) {
    const int shapes[3] = {4, 2, 8};
    long best = -1;
    for (int s = 0; s < 3; ++s) {
        const int t = shapes[s], th = 2 * (32 / t), tw = 4 * t;
        const long a = (long)cdiv(Ho, th) * th * cdiv(Wo, tw) * tw;
        if (best < 0 || a < best) best = a, txg = t;
    }
    return best;
}

// What the ConvLSTM cell epilogue of conv_wino_r6_kernel needs beyond conv_vec4: concatenated input on a chunk boundary, hidden size a
// multiple of 16 (4C gate columns = whole 64-column blocks), bias and o1 present, 16-byte-accessible gates, dense output
inline bool wino6_lstm_ok(const ramnet_conv_desc &d) {
    return d.in_mode == RAMNET_IN_CAT && d.C0 % WK == 0 && d.Cout > 0 && d.Cout % 16 == 0 && d.o1 && d.bias && !d.out_s2d && !d.frame &&
           d.osy == 1 && d.osx == 1 && d.ooy == 0 && d.oox == 0 &&
           (!d.o2 || (d.ldo2 % 4 == 0 && d.ldo2 >= 4 * d.Cout && ((uintptr_t)d.o2 & 15) == 0));
}

// An F(2x4,3x3) launch: every structural condition of the kernel, its parameters, tile shape, grid and exchange buffer.
// chunk = WK: conv_wino_r6_kernel (exact fp32; 32-channel workgroups, two per 64-column weight block; the ConvLSTM cell),
// chunk = WKS: conv_wino_r6s_kernel (split bf16 operands; 64-channel workgroups; no cell epilogue).
// (d.w is not looked at: a caller that asks ramnet_conv_wino_variant sets the pack of the variant afterwards.)
struct Wino6Plan {
    WinoParams q;
    int txg;                // tiles per workgroup row: the TXG of the instantiation
    unsigned grid;
    size_t exchange;        // bytes of the exchange buffer [wave 4][column 4][tile 32][channels + 4]: the least dynamic LDS of the launch
};

inline int wino6_plan(const ramnet_conv_desc &d, int chunk, Wino6Plan &out, bool quiet = false) {
    const bool split = chunk == WKS;
    RAMNET_PLAN_CHECK(d.ntaps == 9 && d.stride == 1 && !d.frame);
    const bool lstm = d.epi == RAMNET_EPI_LSTM;
    if (lstm) RAMNET_PLAN_CHECK(!split && wino6_lstm_ok(d) && (!d.active || d.e0));
    const int ncol = lstm ? 4 * d.Cout : d.Cout;                    // (ConvLSTM: Cout = hidden size, the weights hold 4C gate columns)
    RAMNET_PLAN_CHECK(ncol % W6_BN == 0);
    RAMNET_PLAN_CHECK(d.in_mode == RAMNET_IN_PLAIN || d.in_mode == RAMNET_IN_CAT || d.in_mode == RAMNET_IN_CAT_MUL || d.in_mode == RAMNET_IN_RELUMASK ||
                      d.in_mode == RAMNET_IN_S2D);
    if (d.in_mode == RAMNET_IN_S2D) RAMNET_PLAN_CHECK(d.C0 >= chunk && log2_exact(d.C0) > 0);                 // a chunk lies in one parity group
    if (d.in_mode == RAMNET_IN_CAT || d.in_mode == RAMNET_IN_CAT_MUL) RAMNET_PLAN_CHECK(d.C0 % chunk == 0);   // chunks do not straddle the concatenation
    RAMNET_PLAN_CHECK(conv_vec4(d, false) && d.osy == 1 && d.osx == 1 && d.ooy == 0 && d.oox == 0);
    if (d.out_s2d) RAMNET_PLAN_CHECK(out_s2d_ok(d));
    if (d.epi == RAMNET_EPI_GRU_BWD) RAMNET_PLAN_CHECK(d.Cout % 128 == 0);      // a 64-channel block lies in one half of [dx | d(h.r)]
    int dy0, dx0;
    RAMNET_PLAN_CHECK(taps_3x3(d.dy, d.dx, false, dy0, dx0));
    if (int rc = check_offsets32(d, lstm && d.o2, quiet)) return rc;
    WinoParams &q = out.q;
    q = WinoParams{};                                               // (ksplit / ws / cnt / sparse: F(2x2,3x3) only)
    fill_in_src(d, q.src);
    q.nchunks = cdiv(q.src.Cin, chunk), q.nblk = cdiv(ncol, W6_BN);
    wino6_tile(d.Ho, d.Wo, out.txg);
    q.tiles_x = cdiv(d.Wo, 4 * out.txg), q.tiles_y = cdiv(d.Ho, 2 * (32 / out.txg));
    q.dy0 = dy0, q.dx0 = dx0;
    q.vec4 = 1, q.s2d_shift = d.out_s2d ? log2_exact(d.out_s2d) : 0, q.ksplit = 1;
    // XCD-pinned channel groups for weights that do not fit an L2 (conv_wino.hip)
    q.xg = xcd_groups((size_t)q.nchunks * q.nblk * (split ? (size_t)W6S_BLK_BYTES : W6_U_FLOATS * sizeof(float)), q.nblk);
    const int wgcols = split ? 64 : 32;                             // output channels per workgroup
    const int nbl = (q.nblk * (W6_BN / wgcols)) >> q.xg;            // channel blocks of one XCD group
    q.inv_nbl = 1.0f / (float)nbl, q.inv_tx = 1.0f / (float)q.tiles_x, q.inv_ty = 1.0f / (float)q.tiles_y;
    out.grid = (unsigned)(cdiv(q.tiles_x * q.tiles_y * d.B, 8 >> q.xg) * 8 * nbl);
    out.exchange = (size_t)4 * 4 * 32 * (wgcols + 4) * sizeof(float);
    return 0;
}

// ---- backward-weights (conv_wgrad.hip, conv_wgrad_wino.hip, conv_wgrad_wino6.hip, conv_wgrad_dsplit.hip) --------------------------

// What the three 3x3 families require of a descriptor: nine taps in the forward order kh*3 + kw (the workspace rows follow it; (dy0, dx0)
// = the first one), stride 1, a same-size map, an input mode their loaders know, the 32 (dsplit: 4) input channels a workgroup (a
// staging quad) loads together inside one tensor of a concatenation / one parity group of a space-to-depth view (`group`), and
// several segments only where the kernel walks them (F(2x4)).
inline int wgrad3x3_check(const ramnet_wgrad_desc &d, int group, bool segments, int &dy0, int &dx0, bool quiet = false) {
    RAMNET_PLAN_CHECK(d.ntaps == 9 && d.stride == 1 && d.Ho == d.Hin && d.Wo == d.Win && (segments || d.nseg == 0));
    RAMNET_PLAN_CHECK(d.in_mode == RAMNET_IN_PLAIN || d.in_mode == RAMNET_IN_CAT || d.in_mode == RAMNET_IN_CAT_MUL || d.in_mode == RAMNET_IN_RELUMASK ||
                      d.in_mode == RAMNET_IN_S2D);
    if (d.in_mode == RAMNET_IN_CAT || d.in_mode == RAMNET_IN_CAT_MUL) RAMNET_PLAN_CHECK(d.C0 % group == 0);
    if (d.in_mode == RAMNET_IN_S2D) RAMNET_PLAN_CHECK(d.C0 >= group && log2_exact(d.C0) > 0);
    RAMNET_PLAN_CHECK(taps_3x3(d.dy, d.dx, true, dy0, dx0));
    return 0;
}

// The Winograd backward-weights kernels (F(2x2) and F(2x4) alike) address every tensor (of a segment) through ONE buffer resource of WOOB
// bytes with two 32-bit byte offsets: a per-lane one, the slot inside the strip of a batch, and a scalar one, the strip's corner, which
// carries the image.  The hardware checks their SUM against the resource's extent (measured: profiles/address_limit_tests_notes.md), so the
// WHOLE tensor of B images must end below WOOB — for the sources together with the halo in front of them: their resource begins one row
// and one pixel before the tensor (the first strip's corner), and the last pixel's offset is longer by that much.  Beyond it a load of a
// pixel INSIDE the tensor returns zero.  dsplit addresses with 64-bit pixel indices: no check.
inline int wgrad_offsets32(const ramnet_wgrad_desc &d, bool quiet = false) {
    const bool s2d = d.in_mode == RAMNET_IN_S2D;
    const unsigned long long n = d.B, px = n * d.Hin * d.Win * (s2d ? 4 : 1) + (s2d ? 4ull * d.Win + 2 : d.Win + 1ull);
    const unsigned long long mpx = n * d.Hin * d.Win + d.Win + 1ull, gpx = n * d.Ho * d.Wo;
    const unsigned long long ldx = d.ld0 > d.ld1 ? d.ld0 : d.ld1;
    RAMNET_PLAN_CHECK(px * ldx * 4ull < WOOB && mpx * d.ldm * 4ull < WOOB && gpx * d.ldg * 4ull < WOOB && gpx * d.ldgm * 4ull < WOOB);
    return 0;
}

// How a launch splits its pixel tiles.  Every family has an OWN figure — the workgroups a launch aims at (an option or a constant),
// divided by its channel blocks — and a CAP, a function of the channels alone, which is what ramnet_wgrad_*_slabs answers and a caller
// sizes the [S][...] workspace of the slab form by.  Own figure and cap are NOT ordered: F(2x2) runs 32 x 32-channel workgroups by
// default (nf = 1: twice the target at half the block) while its cap counts 64-channel blocks, so with an odd number of 32-channel
// output blocks own > cap (Cin 64, Cout 96: 128 against 96; Cin 32, Cout 32: 768 against 384); "wgrad_wino_blocks" / RAMNET_DS_TARGET
// move the own figure and leave the cap.  What bounds a launch by its workspace is the dw_slabs term of wgrad_splits, nothing else.
constexpr int WGRAD_WINO_TARGET = 384;      // F(2x2): workgroups per launch the tile splits aim at
constexpr int WG6_TARGET = 384;             // F(2x4): the same
constexpr int DS_TARGET = 512;              // dsplit: the same

inline int wgrad_chan_blocks(int Cin, int ci, int Cout, int co) { return cdiv(Cin, ci) * cdiv(Cout, co); }
inline int at_least_1(int v) { return v < 1 ? 1 : v; }

inline int wgrad_direct_own(int blocks) { return g_opt_wgrad_blocks / blocks; }                 // (ramnet_set_option("wgrad_blocks"): default 512)
inline int wgrad_direct_cap(int blocks) { const int o = wgrad_direct_own(blocks); return o < RAMNET_WGRAD_SLAB_CAP ? o : RAMNET_WGRAD_SLAB_CAP; }     // slab form only
inline int wgrad_wino_own(int Cin, int Cout, int nf) { return g_opt_wgrad_wino_blocks * (2 / nf) / wgrad_chan_blocks(Cin, 32, Cout, 32 * nf); }
inline int wgrad_wino_cap(int Cin, int Cout) { return at_least_1(WGRAD_WINO_TARGET / wgrad_chan_blocks(Cin, 32, Cout, 64)); }
inline int wgrad_wino6_own(int Cin, int Cout) { return g_opt_wgrad_wino_blocks / wgrad_chan_blocks(Cin, 32, Cout, 32); }
inline int wgrad_wino6_cap(int Cin, int Cout) { return at_least_1(WG6_TARGET / wgrad_chan_blocks(Cin, 32, Cout, 32)); }
inline int wgrad_dsplit_own(int Cin, int Cout) {
    static const int target = getenv("RAMNET_DS_TARGET") ? atoi(getenv("RAMNET_DS_TARGET")) : DS_TARGET;      // (tuning runs)
    return target / wgrad_chan_blocks(Cin, 64, Cout, 64);
}
inline int wgrad_dsplit_cap(int Cin, int Cout) { return at_least_1(wgrad_dsplit_own(Cin, Cout)); }

// The clamp chain: the own figure (slab form of the direct family: its cap), at most the units the launch can divide (pixel tiles or
// batches of them), at most the slabs the caller gave (dw_slabs > 0), at least 1.
inline int wgrad_splits(int own, int units, int dw_slabs) {
    int s = own < units ? own : units;
    if (dw_slabs > 0 && s > dw_slabs) s = dw_slabs;
    return at_least_1(s);
}

// 1-D grids that deal their splits to the 8 XCDs (the workgroups that share a split's strips then share an L2) need a multiple of 8:
// from 8 splits up the count moves to one and *xcd_map is set.  F(2x4) rounds to the NEAREST multiple that units and dw_slabs still
// allow, else down: its target of 384 workgroups leaves room below the 512 that the 256 CUs hold at two per CU, and the at most 4
// splits added stay within it ((own + 4) x channel blocks <= 512 from own = 12 up, the first figure that rounds up), so nearest keeps
// the launch closest to the measured target.  dsplit rounds DOWN: its target IS those 512, a step up would leave workgroups waiting
// for a second wave.
inline int wgrad_xcd_splits(int splits, int units, int dw_slabs, bool nearest, int *xcd_map) {
    *xcd_map = splits >= 8;
    if (splits < 8) return splits;
    const int up = (splits + 4) / 8 * 8;
    return nearest && up <= units && (dw_slabs <= 0 || up <= dw_slabs) ? up : splits / 8 * 8;
}

// Second operand of the input loader (XMK: 0 none, 1 ReLU mask, 2 the product of a CAT_MUL input) and mask on dy (GM) -> the template
// instantiation: f(std::integral_constant<int, XMK>, std::bool_constant<GM>), whose int is returned
template <class F>
inline int wgrad_dispatch(const ramnet_wgrad_desc &d, F &&f) {
    const auto on_gm = [&](auto xmk) { return d.gmask != nullptr ? f(xmk, std::true_type{}) : f(xmk, std::false_type{}); };
    if (d.in_mode == RAMNET_IN_RELUMASK) return on_gm(std::integral_constant<int, 1>{});
    if (d.in_mode == RAMNET_IN_CAT_MUL) return on_gm(std::integral_constant<int, 2>{});
    return on_gm(std::integral_constant<int, 0>{});
}

// Address of (input channel c, output channel n) inside one position of a blocked workspace [Cin / 32][Cout / 32][64][16] (the join of
// conv_wgrad_wino_r6_kernel / conv_wgrad_dsplit_kernel: 32 x 32 accumulator tiles as the MFMA leaves them); nCoB = output blocks
__device__ __forceinline__ size_t wgrad_blocked_at(int c, int n, int nCoB) {
    const int c32 = c & 31;
    return ((size_t)(c >> 5) * nCoB + (n >> 5)) * 1024 + ((n & 31) + 32 * ((c32 >> 2) & 1)) * 16 + (c32 & 3) + 4 * (c32 >> 3);
}

#undef RAMNET_PLAN_CHECK

// Grid-stride launch of a pack / unpack kernel over `total` elements in blocks of BLOCK threads (args: ALL of the kernel's parameters)
template <int BLOCK = 256, class K, class... A>
inline int launch_1d(K kernel, size_t total, void *stream, A... args) {
    size_t blocks = (total + BLOCK - 1) / BLOCK;
    if (blocks > 65535) blocks = 65535;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream, args...);
    RAMNET_LAUNCH_CHECK();
    return 0;
}

// ramnet_unpack_wgrad_wino / _wino2x4 / _dsplit: the window [n_off, n_off + Cout) x [0, Cin) of a [.][CinWs][CoutWs] workspace -> grad (+=)
template <class K>
inline int launch_wgrad_unpack(K kernel, const float *ws, float *grad, int Cout, int Cin, int CinWs, int CoutWs, int n_off, void *stream) {
    RAMNET_CHECK_ARG(ws && grad && Cout > 0 && Cin > 0 && CinWs >= Cin && n_off >= 0 && CoutWs >= n_off + Cout);
    return launch_1d(kernel, (size_t)Cout * Cin, stream, ws, grad, Cout, Cin, CinWs, CoutWs, n_off, (size_t)Cout * Cin);
}

}  // namespace ramnet
