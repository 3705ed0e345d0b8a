// Winograd F(2x2, 4x4) for the folded upsample-conv of the decoders (statenet.py:305-308, submodules.py:69-97) on gfx950.
//
// conv5x5(bilinear_x2(x + skip)) is, per output parity (py, px), a 4x4 stride-1 convolution of the replicate-padded low-res
// sum.  Each of those four convolutions is evaluated here as
//     Y = A^T [ sum_ci (G g G^T) .* (B^T d B) ] A,     5x5 input tile -> 2x2 outputs, 25 instead of 64 multiplies
// (Toom-Cook points 0, 1, -1, 2, inf), i.e. 6.25 multiplies per output and input channel instead of 16 (25 for the plain 5x5).
//
// Workgroup = 8 waves: 32 tiles (8 x 4 tiles = 16 x 8 pixels of one parity grid) x 64 output channels (NCQ = 4; for 32-channel
// layers NCQ = 2: 64 tiles x 32 channels, chunks of 8 input channels, 8-byte operand reads).  Per chunk of 16
// input channels every thread loads the 5x5 window of ONE (tile, channel) straight from global memory (the padded input needs
// no bounds logic), transforms it in registers and writes the 25 values to V[25][32 tiles][16] in LDS (double-buffered, one
// barrier per chunk).  Wave (tile half, channel quarter) accumulates all 25 positions of its 16 tiles x 16 channels on
// v_mfma_f32_16x16x4_f32 (100 accumulator VGPRs): A = one 16-byte LDS read per position (swizzled: 2-way, tools/check_fold23_lds_swizzle.py), B = one
// 16-byte global (L2) read per position from weights packed in exactly that lane order.  Loads and the transform of chunk
// i+1 are issued between the MFMAs of chunk i.  The output transform is register-local; bias / ReLU and the border
// corrections of the folded layer (ramnet_conv_desc.frame) are applied by the shared epilogue.
//
// TW = 3 (RAMNET_ALGO_WINOGRAD24_2X3): F(2x3, 4x4), the same structure on 2 x 3 output tiles.  Rows keep the 5-point F(2,4)
// transform, columns take the 6-point F(3,4) one (points 0, 1, -1, 1/2, -1/2, inf): a 5 x 6 window, 30 positions (15 pairs,
// 120 accumulator VGPRs), 5.0 multiplies per output instead of 6.25 — 20 % fewer MFMAs and window loads per output.  V holds 30
// positions (2 x 61.4 KB).  Training-batch launches only (ramnet_fold_wino_variant): no split reduction.
// HALF: the F(2x3) launches as workgroups of ONE 16-tile group (4 waves, 2 x 30.7 KB, two per CU; ramnet_fold_halfwg_variant).
#include <stdlib.h>
#include "common.hpp"
#include "conv_plan.hpp"
#include "conv_epilogue.hpp"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace ramnet {

// tiles per workgroup (2x2 outputs each): 8 x 4 or 4 x 8 (rows x columns, TXW = columns) for 32 tiles, 8 x 8 for 64
constexpr int W24_PS = 512;                       // floats per position in V: tiles x chunk channels (32 x 16 or 64 x 8)
constexpr int W24_V = 25 * W24_PS;                // floats per V buffer (51.2 KB)
constexpr int W23_V = 30 * W24_PS;                // the same for F(2x3, 4x4) (61.4 KB)

__device__ __forceinline__ float2 ld2f(const float *p) { return *reinterpret_cast<const float2 *>(p); }

// Buffer resource over [p, p + bytes): loads then take a 32-bit per-lane byte offset plus a scalar one, so the window and
// weight streams of the main loop need no 64-bit address arithmetic.  The pointer goes through readfirstlane so that the
// compiler knows the descriptor is wave-uniform (cdna_hip_programming.md, buffer addressing).
__device__ __forceinline__ auto make_rsrc(const void *p, unsigned bytes) {
    const unsigned long long a = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)hi << 32) | lo), (short)0, (int)bytes, 0x00020000);
}

#ifdef W24_TRACE   // tools/wino24_trace.hip: per-wave timestamps (s_memtime, 100 MHz): [block][wave][16 chunks][6 slots] + 4 kernel slots
__device__ unsigned long long *g_w24_trace;
#define W24_STAMP(chunk_, slot)                                                                                          \
    do {                                                                                                                 \
        if (lane == 0 && (chunk_) <= 16) g_w24_trace[(((size_t)blockIdx.x * 8 + wave) * 17 + (chunk_)) * 6 + (slot)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define W24_STAMP(chunk_, slot)
#endif

struct Wino24Params {
    const float *x;          // replicate-padded low-res input [B][Hp][Wp][Cin]
    const float *wp;         // [4 classes][Cin/16][Cout/64][25][4][64 lanes][4]
    int Hp, Wp, ldx, nchunks, nblk, tiles_x, tiles_y, Hc, Wc;
    int cpc;                  // backward-data (DG): chunks per parity class = Cout_fwd / chunk size
    unsigned xbytes, wbytes;  // extents of x and wp (buffer addressing: both below 4 GB)
    int ksplit;               // forward: gridDim.y = splits of the channel reduction (1 = none; an even number of chunks each)
    float *ws;                // ksplit > 1: partial outputs [gridDim.x][ksplit][512 threads x 16]
    int *cnt;                 //             arrival counters [gridDim.x], zero between launches
};

// NCQ = 16-channel groups of output channels per workgroup: 4 (32 tiles, chunks of 16) or 2 (64 tiles, chunks of 8)
// DG = backward-data of the folded layer (RAMNET_IN_PARITY4): the input is the full-resolution gradient [B][2*Hc][2*Wc][C]
// (Hp, Wp = its extent), whose four parity sub-grids are the reduction blocks (class = chunk / cpc: window origin and pixel
// stride 2, zero outside — a buffer load past the tensor returns 0); the output is the dense (Hc+4) x (Wc+4) grid of the padded
// low-resolution tensor.
// PAIR (32-channel layers: the last decoder): the two column parities px = 0 / 1 of a row parity share ONE transformed input — the
// class-(py, 1) grid is tiled with its tile origins shifted by one column, so that both classes read the same 5 x 5 windows — and
// the workgroup's 64 columns are (px, 32 channels): the input transform (25 loads + ~160 VALU per tile and channel, the cost that
// bounds this kernel at 32 output channels: 35 % MFMA-busy) feeds twice the MFMAs.  NCQ = 4 geometry, chunks of 16.
// TW = output columns per tile: 2 = F(2x2, 4x4), 3 = F(2x3, 4x4) (NCQ = 4 only; window 5 x (TW + 3), NP = 5 (TW + 3) positions).
// HALF (F(2x3) only): ONE 16-tile group per workgroup — 4 waves (one per channel quarter) on 256 threads, V planes of 256 floats per position
// (2 x 30.7 KB), two workgroups per CU.  Per wave the instruction stream is the 8-wave kernel's: the same tiles' arithmetic, chunk order and
// MFMA order (bit-identical outputs); a 61 KB workgroup can share a CU with a workgroup of another kernel where the 123 KB one holds it alone.
template <int NCQ, bool DG, int TXW, bool PAIR = false, int TW = 2, bool HALF = false>
__global__ void __launch_bounds__(HALF ? 256 : 512, HALF ? 2 : 1) conv_wino24_kernel(const ramnet_conv_desc p, const Wino24Params q) {
    static_assert(!PAIR || (NCQ == 4 && !DG), "pair mode: forward, 64-column workgroups");
    static_assert(TW == 2 || (TW == 3 && NCQ == 4), "F(2x3): 64-column workgroups");
    static_assert(!HALF || TW == 3, "half workgroups: F(2x3) only");
    constexpr int NTG = HALF ? 1 : 2;                 // 16-tile groups per workgroup (NCQ = 4)
    constexpr int PS = HALF ? W24_PS / 2 : W24_PS;    // floats per position in V
    constexpr int WC = TW + 3, NP = 5 * WC;           // window columns, Winograd positions
    constexpr int VSZ = NP * PS;                      // floats per V buffer
    constexpr int W24_K = NCQ == 4 ? 16 : 8;          // input channels per chunk
    constexpr int W24_TX = TXW, W24_TY = (NCQ == 4 ? 16 * NTG : 64) / TXW;      // tile columns / rows per workgroup
    constexpr int VEC = W24_K / 4;                    // floats per lane and operand read (k = VEC*ks + j)
    constexpr int W24_U = NP * NCQ * 64 * VEC;        // packed weights of one (class, chunk, channel block)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *V = smem;                               // [2][NP][32 (HALF: 16)][16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, ks = lane >> 4;
    const int th = HALF ? 0 : NCQ == 4 ? wave & 1 : wave & 3, cq = HALF ? wave : NCQ == 4 ? wave >> 1 : wave >> 2;       // 16-tile group, 16-channel group

    // blockIdx.x = ((tile block * nblk + channel block) * 4 + class): the four parities of a tile block read the same input
    int bid = blockIdx.x;
    const int cls = DG ? 0 : PAIR ? bid & 1 : bid & 3;          // PAIR: the row parity; both column parities in this workgroup
    if (!DG) bid >>= PAIR ? 1 : 2;
    const int nb = bid % q.nblk;
    bid /= q.nblk;
    const int tbx = bid % q.tiles_x;
    bid /= q.tiles_x;
    const int tby = bid % q.tiles_y, b = bid / q.tiles_y;
    const int py = PAIR ? cls : cls >> 1, px = PAIR ? 0 : cls & 1;
    const int n0 = nb * 16 * NCQ;

    // ---- input transform item of this thread: (tile, channel of the chunk)
    const int it = tid / W24_K, ik = tid % W24_K;
    // window rows / columns past the padded input only feed outputs past the grid: clamp them one by one
    const int iy0 = 2 * (tby * W24_TY + it / W24_TX) + py, ix0 = TW * (tbx * W24_TX + it % W24_TX) + px;
    // byte offsets: lane part (image + row, column + channel: one add per load) + scalar part (chunk)
    unsigned rowo[5], colo[WC];
    int cur_cls = -1;
    auto set_class = [&](int c) {                   // DG: window of parity class c = (c >> 1, c & 1); invalid -> offset past the tensor
        cur_cls = c;
        const int cy = c >> 1, cx = c & 1;
        const int u0 = 2 * (tby * W24_TY + it / W24_TX), v0 = TW * (tbx * W24_TX + it % W24_TX);
#pragma unroll
        for (int r = 0; r < WC; ++r) {
            const int i = u0 - cy - 3 + r, j = v0 - cx - 3 + r;           // class-grid row / column
            if (r < 5) rowo[r] = (unsigned)i < (unsigned)q.Hc ? 4u * (unsigned)((b * q.Hp + 2 * i + cy) * q.Wp * q.ldx) : 0x40000000u;
            colo[r] = (unsigned)j < (unsigned)q.Wc ? 4u * (unsigned)((2 * j + cx) * q.ldx + ik) : 0x40000000u;
        }
    };
    if (!DG) {
#pragma unroll
        for (int r = 0; r < WC; ++r) {
            if (r < 5) rowo[r] = 4u * (unsigned)((b * q.Hp + min(iy0 + r, q.Hp - 1)) * q.Wp * q.ldx);
            colo[r] = 4u * (unsigned)(min(ix0 + r, q.Wp - 1) * q.ldx + ik);
        }
    }
    // Split reduction (forward launches far below one workgroup per CU: the first decoders at batch 1): workgroup blockIdx.y reduces
    // chunks [cbeg, cbeg + nch) and the partial outputs are joined in front of the epilogue (as in conv_wino.hip).  F(2x3): never split.
    const int ksp = (DG || TW != 2) ? 1 : q.ksplit;
    const int cps = ((q.nchunks / 2 + ksp - 1) / ksp) * 2, cbeg = DG ? 0 : (int)blockIdx.y * cps;
    const auto xrs = make_rsrc(q.x + cbeg * W24_K, q.xbytes - (unsigned)cbeg * W24_K * 4u);
    // operand reads are VEC floats per lane; the XOR swizzle spreads the 16 tiles of a read over all banks
    const int vdst = NCQ == 4 ? it * 16 + (((ik >> 2) ^ ((it >> 2) & 3)) << 2) + (ik & 3) : it * 8 + (((ik >> 1) ^ ((it >> 3) & 1)) << 1) + (ik & 1);
    float raw[5 * WC];
    auto load_raw = [&](int chunk) {
        int soff = chunk * (W24_K * 4);                 // uniform
        if (DG) {
            const int c = chunk / q.cpc;
            if (c != cur_cls) set_class(c);
            soff = (chunk - c * q.cpc) * (W24_K * 4);
        }
#pragma unroll
        for (int r = 0; r < 5; ++r)
#pragma unroll
            for (int c = 0; c < WC; ++c)
                raw[r * WC + c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, (int)(rowo[r] + colo[c]), soff, 0));
    };
    // one window row at a time (the main loop requests row i as soon as tr_row(i) has consumed the previous window's row i: five loads per
    // slot instead of 25 in one)
    int lr_soff = 0;
    auto load_row_begin = [&](int chunk) {
        lr_soff = chunk * (W24_K * 4);
        if (DG) {
            const int c = chunk / q.cpc;
            if (c != cur_cls) set_class(c);
            lr_soff = (chunk - c * q.cpc) * (W24_K * 4);
        }
    };
    auto load_row = [&](int r) {
#pragma unroll
        for (int c = 0; c < WC; ++c)
            raw[r * WC + c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, (int)(rowo[r] + colo[c]), lr_soff, 0));
    };
    // B^T = [2 -1 -2 1 0; 0 -2 -1 1 0; 0 2 -3 1 0; 0 -1 0 1 0; 0 2 -1 -2 1]
    auto tr_col = [&](int c) {
        const float d0 = raw[c], d1 = raw[WC + c], d2 = raw[2 * WC + c], d3 = raw[3 * WC + c], d4 = raw[4 * WC + c];
        raw[c] = 2.f * (d0 - d2) - d1 + d3;
        raw[WC + c] = d3 - d2 - 2.f * d1;
        raw[2 * WC + c] = 2.f * d1 - 3.f * d2 + d3;
        raw[3 * WC + c] = d3 - d1;
        raw[4 * WC + c] = 2.f * (d1 - d3) - d2 + d4;
    };
    // F(2x3): vbuf = the lane's first element of the buffer (V + vdst or V + dbuf1 below)
    auto tr_row = [&](float *vbuf, int i) {
        float *dst = TW == 2 ? vbuf + (i * WC) * PS + vdst : vbuf + (i * WC) * PS;
        if constexpr (TW == 2) {
            const float d0 = raw[i * 5], d1 = raw[i * 5 + 1], d2 = raw[i * 5 + 2], d3 = raw[i * 5 + 3], d4 = raw[i * 5 + 4];
            dst[0 * PS] = 2.f * (d0 - d2) - d1 + d3;
            dst[1 * PS] = d3 - d2 - 2.f * d1;
            dst[2 * PS] = 2.f * d1 - 3.f * d2 + d3;
            dst[3 * PS] = d3 - d1;
            dst[4 * PS] = 2.f * (d1 - d3) - d2 + d4;
        } else {
            // F(3,4) columns, B^T = [1/4 0 -5/4 0 1 0; 0 -1/4 -1/4 1 1 0; 0 1/4 -1/4 -1 1 0; 0 -1/2 -1 1/2 1 0; 0 1/2 -1 -1/2 1 0; 0 1/4 0 -5/4 0 1]
            const float d0 = raw[i * 6], d1 = raw[i * 6 + 1], d2 = raw[i * 6 + 2], d3 = raw[i * 6 + 3], d4 = raw[i * 6 + 4], d5 = raw[i * 6 + 5];
            const float u = d3 - d1, v = d4 - d2;
            dst[0 * PS] = fmaf(-1.25f, d2, fmaf(0.25f, d0, d4));
            dst[1 * PS] = fmaf(-0.25f, d1 + d2, d3 + d4);
            dst[2 * PS] = fmaf(0.25f, d1 - d2, d4 - d3);
            dst[3 * PS] = fmaf(0.5f, u, v);
            dst[4 * PS] = fmaf(-0.5f, u, v);
            dst[5 * PS] = fmaf(-1.25f, d3, fmaf(0.25f, d1, d5));
        }
    };

    // ---- MFMA operands
    const int tile = th * 16 + l15;
    const int aoff = NCQ == 4 ? tile * 16 + ((ks ^ ((tile >> 2) & 3)) << 2) : tile * 8 + ((ks ^ ((tile >> 3) & 1)) << 1);
    constexpr int WPOS = NCQ * 64 * VEC;              // packed floats per position
    const auto wrs = make_rsrc(q.wp, q.wbytes);
    const int wsrc = (((cls * q.nchunks + cbeg) * q.nblk + nb) * W24_U + cq * (64 * VEC)) * 4;     // uniform byte offset; lane part below
    const int wlane = lane * VEC * 4;
    auto ldv = [&](const float *ptr) {                // VEC floats -> float4 (upper half unused for VEC = 2)
        if (VEC == 4) return ld4(ptr);
        const float2 t = ld2f(ptr);
        return make_float4(t.x, t.y, 0.f, 0.f);
    };
    auto ldw = [&](int soff) {                       // weights: scalar byte offset + lane offset
        if constexpr (VEC == 4) {
            return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wrs, wlane, soff, 0));
        } else {
            const float2 t = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(wrs, wlane, soff, 0));
            return make_float4(t.x, t.y, 0.f, 0.f);
        }
    };
    const int wchunk = q.nblk * W24_U * 4;
    // F(2x3): V is 2 x 61.4 KB.  The lane's offsets into buffer 1 are made opaque, so that every A-operand read and V store of a buffer is
    // ONE base VGPR + an immediate offset (30 positions x 2 KB < 64 KB); left to itself the compiler keeps a base per group of positions
    // and spills them (reloads behind s_waitcnt vmcnt(0) in the main loop).
    int abuf1 = VSZ + aoff, dbuf1 = VSZ + vdst;
    if constexpr (TW == 3) asm volatile("" : "+v"(abuf1), "+v"(dbuf1));

    f32x4 acc[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nch = DG ? q.nchunks : min(cps, q.nchunks - cbeg);
    W24_STAMP(16, 0);
    load_raw(0);
    // Weight ring: 10 slots, prefetch distance 9 positions.  Vector loads return in order, so a weight load issued after the
    // 25 window loads of a chunk can only be consumed once those have landed: the ring is deep enough to give them ~9 positions
    // (~1 us) of MFMA work, and the chunk loop is unrolled by two so that the slot of a position is a compile-time constant
    // (RING divides 2 NP).  F(2x3) forward: 6 slots, prefetch distance 4 — with 10 its 120 accumulators spill (backward-data keeps 10).
    constexpr int RING = TW == 2 || DG ? 10 : 6, DIST = RING - 2;
    static_assert((2 * NP) % RING == 0, "ring slots repeat every chunk pair");
    float4 bq[RING];
#pragma unroll
    for (int i = 0; i < DIST; ++i) bq[i] = ldw(wsrc + i * (WPOS * 4));
#pragma unroll
    for (int c = 0; c < WC; ++c) tr_col(c);
#pragma unroll
    for (int i = 0; i < 5; ++i) tr_row(TW == 2 ? V : V + vdst, i);
    load_raw(min(1, nch - 1));
    __syncthreads();

    W24_STAMP(16, 1);
    for (int chunk0 = 0; chunk0 < nch; chunk0 += 2) {             // nch is even (checked on the host)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int chunk = chunk0 + half;
            const float *vb = V + half * VSZ;
            float *vn = TW == 2 ? V + (half ^ 1) * VSZ : V + (half ? vdst : dbuf1);
            auto lda = [&](int pos) {
                if constexpr (TW == 2) return ldv(vb + pos * PS + aoff);
                else return ldv(V + (half ? abuf1 : aoff) + pos * PS);
            };
            // The window of chunk+1 is already in registers (loaded at the end of the previous phase: a weight load issued
            // after it can only be consumed once it has landed, and there it has a barrier and four position pairs to do so);
            // it is transformed into the other V buffer during this phase and the window of chunk+2 requested right after.
            const int cnext = min(chunk + 1, nch - 1), cnext2 = min(chunk + 2, nch - 1);     // past the end: re-stage the last chunk
            const int wcur = wsrc + chunk * wchunk, wnext = wsrc + cnext * wchunk;
            W24_STAMP(chunk, 0);
            // positions go in pairs (two independent accumulator chains: a 16x16x4 MFMA can be issued every 32 cycles but its
            // result is only available to a dependent one after 40); F(2x2): the last position runs alone
            float4 aq[2][2];                                   // A operands of the current / next pair (ping-pong, no copies)
            aq[0][0] = lda(0), aq[0][1] = lda(1);
#pragma unroll
            for (int pp = 0; pp < (NP + 1) / 2; ++pp) {
                const int pos = 2 * pp, g = half * NP + pos;
                const bool two = pos + 1 < NP;
                if (pos + 2 < NP) aq[(pp + 1) & 1][0] = lda(pos + 2);
                if (pos + 3 < NP) aq[(pp + 1) & 1][1] = lda(pos + 3);
                const float4 a0 = aq[pp & 1][0], a1 = aq[pp & 1][1];
#if !defined(W24_ABLATE) || !(W24_ABLATE & 2)
                bq[(g + DIST) % RING] = pos + DIST < NP ? ldw(wcur + (pos + DIST) * (WPOS * 4)) : ldw(wnext + (pos + DIST - NP) * (WPOS * 4));
                if (two) bq[(g + 1 + DIST) % RING] = pos + 1 + DIST < NP ? ldw(wcur + (pos + 1 + DIST) * (WPOS * 4)) : ldw(wnext + (pos + 1 + DIST - NP) * (WPOS * 4));
#endif
                const float4 b0 = bq[g % RING], b1 = bq[(g + 1) % RING];
                __builtin_amdgcn_sched_barrier(0);
                acc[pos] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0.x, acc[pos], 0, 0, 0);
                if (two) acc[pos + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b1.x, acc[pos + 1], 0, 0, 0);
                acc[pos] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0.y, acc[pos], 0, 0, 0);
                if (two) acc[pos + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b1.y, acc[pos + 1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                // The side work of the chunk in SLOTS (slot = 2 pp + side), one piece behind every group of four MFMAs instead of blocks of
                // 24-34 VALU in three gaps and 25 loads in one: column transform c in slots 4..8, row transform i (+ its 5 LDS stores) in
                // slots 9, 11, .., 17, and the five window loads of row i of chunk + 2 right behind it (slots 10, 12, .., 18: the row's
                // registers are free, and the loads have six position pairs + the barrier to land before the next chunk's slot 4).
                // F(2x3) (30 slots): column transforms in slots 4..9, rows in 10, 12, .., 18, their six loads in 11, 13, .., 19.
                constexpr int R0 = 4 + WC;                     // slot of the first row transform
                auto slot = [&](int sl) {
                    if (sl == 4) W24_STAMP(chunk, 1);
                    if (sl >= 4 && sl < R0) tr_col(sl - 4);
                    if (sl == R0) W24_STAMP(chunk, 2);
                    if (sl >= R0 && sl <= R0 + 8 && !((sl - R0) & 1)) tr_row(vn, (sl - R0) >> 1);
#if !defined(W24_ABLATE) || !(W24_ABLATE & 1)      // timing experiments (tools/wino24_trace.hip): 1 = no window loads, 2 = no weight loads
                    if (sl == R0 + 1) load_row_begin(cnext2);
                    if (sl > R0 && sl <= R0 + 9 && ((sl - R0) & 1)) load_row((sl - R0 - 1) >> 1);
#endif
                    if (sl == R0 + 9) W24_STAMP(chunk, 3);
                };
                slot(2 * pp);
                __builtin_amdgcn_sched_barrier(0);
                if (VEC == 4) {
                    acc[pos] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b0.z, acc[pos], 0, 0, 0);
                    if (two) acc[pos + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b1.z, acc[pos + 1], 0, 0, 0);
                    acc[pos] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b0.w, acc[pos], 0, 0, 0);
                    if (two) acc[pos + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b1.w, acc[pos + 1], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                slot(2 * pp + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            W24_STAMP(chunk, 4);
            __syncthreads();
            W24_STAMP(chunk, 5);
        }
    }
    W24_STAMP(16, 2);

    // ---- output transform A^T M A (A^T = [1 1 1 1 0; 0 1 -1 2 1]) of the lane's 4 tiles x 1 channel, fused epilogue.
    // All 16 outputs of the lane are finished in registers (bias — ONE load —, border corrections, ReLU) and stored at the end: with the
    // stores interleaved, every border-correction block (a conditional load) was followed by a wait for ALL memory operations, i.e. for
    // the previous output's store (stores count in vmcnt on gfx9): 16 serialized write latencies per workgroup, which holds its CU alone.
    const int ncol = n0 + cq * 16 + l15;
    const int pxc = PAIR ? ncol >> 5 : px, n = PAIR ? ncol & 31 : ncol;      // PAIR: column = (column parity, channel)
    if (n >= p.Cout) return;
    const int epi = p.epi;
    const float bias_n = (!DG && p.bias) ? p.bias[n] : 0.f;
    const bool relu = epi == RAMNET_EPI_RELU;
    constexpr int NOUT = 8 * TW;                      // 4 tiles x 2 x TW outputs
    float ov[NOUT];
    size_t op[NOUT];
    bool oo[NOUT];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float s[2][WC];
#pragma unroll
        for (int j = 0; j < WC; ++j) {
            const float m0 = acc[j][r], m1 = acc[WC + j][r], m2 = acc[2 * WC + j][r], m3 = acc[3 * WC + j][r], m4 = acc[4 * WC + j][r];
            s[0][j] = m0 + m1 + m2 + m3;
            s[1][j] = m1 - m2 + 2.f * m3 + m4;
        }
#pragma unroll
        for (int a2 = 0; a2 < 2; ++a2) {
            if constexpr (TW == 2) {
                ov[(r * 2 + a2) * 2] = s[a2][0] + s[a2][1] + s[a2][2] + s[a2][3];
                ov[(r * 2 + a2) * 2 + 1] = s[a2][1] - s[a2][2] + 2.f * s[a2][3] + s[a2][4];
            } else {                                // A^T = [1 1 1 1 1 0; 0 1 -1 1/2 -1/2 0; 0 1 1 1/4 1/4 1]
                ov[(r * 2 + a2) * 3] = s[a2][0] + s[a2][1] + s[a2][2] + s[a2][3] + s[a2][4];
                ov[(r * 2 + a2) * 3 + 1] = fmaf(0.5f, s[a2][3] - s[a2][4], s[a2][1] - s[a2][2]);
                ov[(r * 2 + a2) * 3 + 2] = fmaf(0.25f, s[a2][3] + s[a2][4], s[a2][1] + s[a2][2]) + s[a2][5];
            }
        }
    }
    if (!DG && ksp > 1) {
        // join of the split reduction: partial outputs -> slab blockIdx.y of this tile's workspace, the last arrival adds the slabs in
        // split order (device-scope 16-byte accesses, no fences: see conv_wino.hip) and goes on; no lane has left (Cout fills the block)
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        constexpr int AUX_SC1 = 16;
        const auto wr = make_rsrc(q.ws + (size_t)blockIdx.x * ksp * 8192, (unsigned)(ksp * 8192 * 4));
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, make_float4(ov[4 * i], ov[4 * i + 1], ov[4 * i + 2], ov[4 * i + 3])), wr,
                                                   (i * 512 + tid) * 16, (int)blockIdx.y * 32768, AUX_SC1);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        if (tid == 0) {
            const int arrived = __hip_atomic_fetch_add(q.cnt + blockIdx.x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (arrived == ksp - 1) __hip_atomic_store(q.cnt + blockIdx.x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            reinterpret_cast<int *>(smem)[0] = arrived == ksp - 1;
        }
        __syncthreads();
        if (!reinterpret_cast<int *>(smem)[0]) return;
#pragma unroll
        for (int i = 0; i < 16; ++i) ov[i] = 0.f;
        for (int sp = 0; sp < ksp; ++sp)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 t = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wr, (i * 512 + tid) * 16, sp * 32768, AUX_SC1));
                ov[4 * i] += t.x, ov[4 * i + 1] += t.y, ov[4 * i + 2] += t.z, ov[4 * i + 3] += t.w;
            }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = th * 16 + 4 * ks + r;
        const int oy0 = 2 * (tby * W24_TY + t / W24_TX), ox0 = TW * (tbx * W24_TX + t % W24_TX) - (PAIR ? pxc : 0);
#pragma unroll
        for (int a2 = 0; a2 < 2; ++a2) {
#pragma unroll
            for (int c2 = 0; c2 < TW; ++c2) {
                const int oy = oy0 + a2, ox = ox0 + c2, idx = (r * 2 + a2) * TW + c2;
                if (DG) {                           // dense output grid, plain store
                    oo[idx] = oy < p.Ho && ox < p.Wo;
                    op[idx] = (((size_t)b * p.Ho + oy) * p.Wo + ox) * p.ldo + n;
                    continue;
                }
                oo[idx] = !(oy >= q.Hc || ox >= q.Wc || (PAIR && ox < 0));
                const int oyF = 2 * oy + py, oxF = 2 * ox + pxc;
                op[idx] = (((size_t)b * p.HoF + oyF) * p.WoF + oxF) * p.ldo + n;
                float v = ov[idx] + bias_n;
                if (oo[idx]) v += epilogue_side(p, epi, b, oyF, oxF, n);
                ov[idx] = relu ? fmaxf(v, 0.f) : v;
            }
        }
    }
#pragma unroll
    for (int idx = 0; idx < NOUT; ++idx)
        if (oo[idx]) p.out[op[idx]] = ov[idx];
    W24_STAMP(16, 3);
}

// OIHW 5x5 weights of an UpsampleConvLayer -> U = G W4 G^T of the four 4x4 parity filters W4 = A_py w A_px^T (the bilinear x2
// upsample folded into the filter) in the lane order of the kernel's B operand; integer matrices, double sums, one division.
// TW = 3: F(2x3, 4x4), U = G W4 Gc^T with the 6 x 4 column matrix Gc (30 positions, pos = a*6 + b).
// The packs evaluate U through the INTEGER matrices 6 G, 3 Gc and 4 FA and divide once: U = (6 G)(4 FA) w (4 FA)^T (6 G | 3 Gc)^T / (16 x 36 | 16 x 18)
// is then the rounding of the rational (a transformed weight that cancels comes out as 0, not as a 2^-5x residue of the double 1.0 / 6).
__device__ __forceinline__ int fold_wino_g6(int a, int t) {            // 6 G of F(2,4), points 0, 1, -1, 2, inf
    const int G6[5][4] = {{3, 0, 0, 0}, {-3, -3, -3, -3}, {-1, 1, -1, 1}, {1, 2, 4, 8}, {0, 0, 0, 6}};
    return G6[a][t];
}
__device__ __forceinline__ int fold_wino_gc3(int b, int s) {           // 3 Gc of F(3,4), points 0, 1, -1, 1/2, -1/2, inf
    const int G3[6][4] = {{12, 0, 0, 0}, {2, 2, 2, 2}, {2, -2, 2, -2}, {-8, -4, -2, -1}, {-8, 4, -2, 1}, {0, 0, 0, 3}};
    return G3[b][s];
}
__device__ __forceinline__ int fold_fa4(int p, int t, int k) {         // 4 FA: the bilinear fold (ops.FOLD_A)
    const int FA4[2][4][5] = {{{1, 0, 0, 0, 0}, {3, 3, 1, 0, 0}, {0, 1, 3, 3, 1}, {0, 0, 0, 1, 3}}, {{3, 1, 0, 0, 0}, {1, 3, 3, 1, 0}, {0, 0, 1, 3, 3}, {0, 0, 0, 0, 1}}};
    return FA4[p][t][k];
}
// column matrix of a TW-wide tile times its denominator (6 for F(2,4), 3 for F(3,4))
__device__ __forceinline__ int fold_wino_gci(int tw, int b, int s) { return tw == 2 ? fold_wino_g6(b, s) : fold_wino_gc3(b, s); }
// U of one (position (a, b), parities (py, px), flipped or not) from the 25 taps wk of one (output, input) channel pair
__device__ __forceinline__ float fold_wino_u(int tw, int a, int b, int py, int px, bool flip, const float *__restrict__ wk) {
    int ga[5], gb[5];                               // ga[kh] = sum_t (6 G)[a][t] (4 FA)[py][t][kh], gb the same along the columns
    for (int kh = 0; kh < 5; ++kh) {
        ga[kh] = 0, gb[kh] = 0;
        for (int t = 0; t < 4; ++t) {
            const int tt = flip ? 3 - t : t;
            ga[kh] += fold_wino_g6(a, t) * fold_fa4(py, tt, kh), gb[kh] += fold_wino_gci(tw, b, t) * fold_fa4(px, tt, kh);
        }
    }
    double u = 0;                                   // (integer x fp32 products: exact in double)
    for (int kh = 0; kh < 5; ++kh)
        for (int kw = 0; kw < 5; ++kw) u += (double)(ga[kh] * gb[kw]) * (double)wk[kh * 5 + kw];
    return (float)(u / (tw == 2 ? 576.0 : 288.0));
}

template <int TW>
__global__ void pack_weight_fold_wino_kernel(const float *__restrict__ w, float *__restrict__ wp, int Cout, int Cin, int kc, int ncq,
                                             int pair, size_t total) {
    constexpr int WC = TW + 3, NP = 5 * WC;
    const int vec = kc / 4, nblk = pair ? 1 : Cout / (16 * ncq), nch = Cin / kc;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        // i = ((((cls*nch + chunk)*nblk + nb)*NP + pos)*ncq + cq)*64*vec + (ks*16 + l15)*vec + j
        size_t r = i;
        const int j = (int)(r % vec);
        r /= vec;
        const int l15 = (int)(r % 16);
        r /= 16;
        const int ks = (int)(r % 4);
        r /= 4;
        const int cq = (int)(r % ncq);
        r /= ncq;
        const int pos = (int)(r % NP);
        r /= NP;
        const int nb = (int)(r % nblk);
        r /= nblk;
        const int chunk = (int)(r % nch), cls = (int)(r / nch);
        const int k = chunk * kc + ks * vec + j, col = (nb * ncq + cq) * 16 + l15;
        // pair layout (32-channel layers): class = row parity, column = (column parity, channel)
        const int n = pair ? col & 31 : col;
        const int py = pair ? cls : cls >> 1, px = pair ? col >> 5 : cls & 1, a = pos / WC, b = pos % WC;
        // U[a][b] = sum_{t,s} G[a][t] G[b][s] sum_{kh,kw} FA[py][t][kh] FA[px][s][kw] w[n][k][kh][kw]
        wp[i] = fold_wino_u(TW, a, b, py, px, false, w + ((size_t)n * Cin + k) * 25);
    }
}

static bool fold_wino_pair(int Cout, int Cin) {
    return Cout == 32 && Cin % 32 == 0 && g_opt_fold_pair;      // (ramnet_set_option("fold_pair", 0): the 32-channel form, 64 tiles x 32 channels, chunks of 8)
}

static bool fold_wino_geometry(int Cout, int Cin, int &kc, int &ncq) {
    kc = ((Cout % 64 == 0 && Cin % 16 == 0) || fold_wino_pair(Cout, Cin)) ? 16 : 8, ncq = kc == 16 ? 4 : 2;
    return Cout % 32 == 0 && Cin % (2 * kc) == 0;
}

// Backward-data of the folded layer: x0 = g = dy * mask [B][Hin = 2H][Win = 2W][C0 = Cout_fwd], out = gradient of the padded
// low-res tensor [B][Ho = H+4][Wo = W+4][Cout = Cin_fwd]; w = Winograd weights of the flipped parity filters over 4*C0 reduction
// channels (ops.pack_fold_wino_dgrad).
// F(2x3) workgroup tile: 32 tiles of 2 x 3 outputs as 16 x 12 (TX 4), 32 x 6 (TX 2) or 4 x 48 (TX 16) outputs, whichever pads the
// Ho x Wt grid least (as wino6_tile in conv_wino6.hip); returns the padded area.  Parity grids 32x43 / 64x86 / 128x172 (+1 column for
// the pair form) and backward-data outputs 36x47 / 68x90 / 132x176: tile-level edge waste <= 4.7 %.
static long wino23_tile(int Ho, int Wt, int &tx) {
    const int shapes[3] = {4, 2, 16};
    long best = -1;
    for (int s = 0; s < 3; ++s) {
        const int t = shapes[s], th = 2 * (32 / t), tw = 3 * t;
        const long a = (long)cdiv(Ho, th) * th * cdiv(Wt, tw) * tw;
        if (best < 0 || a < best) best = a, tx = t;
    }
    return best;
}

// The same for the half-workgroup form (conv_wino24_kernel<.., HALF = true>): 16 tiles as 8 x 12 (TX 4), 16 x 6 (TX 2), 4 x 24 (TX 8) or
// 2 x 48 (TX 16) outputs.  Every 32-tile block above is two of these side by side or on top of each other, so the padded area is never
// larger than wino23_tile's on the same map.
static long wino23_tile_half(int Ho, int Wt, int &tx) {
    const int shapes[4] = {4, 2, 8, 16};
    long best = -1;
    for (int s = 0; s < 4; ++s) {
        const int t = shapes[s], th = 2 * (16 / t), tw = 3 * t;
        const long a = (long)cdiv(Ho, th) * th * cdiv(Wt, tw) * tw;
        if (best < 0 || a < best) best = a, tx = t;
    }
    return best;
}

// Does this RAMNET_ALGO_WINOGRAD24_2X3 launch run as half workgroups (4 waves, 16 tiles, two per CU)?  Structurally: every launch the
// F(2x3) launcher accepts (64-column workgroups — NCQ = 4, the pair form included —, no split reduction).  force = 0 follows
// ramnet_set_option("fold_half_wg"): 0 = never, 1 = every eligible launch, 2 = auto (fold_halfwg_auto below).
static bool fold_halfwg_auto(const ramnet_conv_desc &d);
static int fold_halfwg_variant(const ramnet_conv_desc &d, int force) {
    if (d.algo != RAMNET_ALGO_WINOGRAD24_2X3 || d.stride != 1 || d.splitk_ws != nullptr) return 0;
    if (d.in_mode == RAMNET_IN_PARITY4) {
        if (d.C0 % 16 != 0 || d.Cout % 64 != 0) return 0;
    } else if (d.in_mode == RAMNET_IN_PLAIN) {
        const bool wide = fold_wino_pair(d.Cout, d.C0) || (d.Cout % 64 == 0 && d.C0 % 16 == 0);
        if (!wide || d.C0 % 32 != 0 || d.Ho < 2 || d.Wo < 2) return 0;
    } else {
        return 0;
    }
    const int mode = force ? 1 : g_opt_fold_half_wg;
    return mode == 1 ? 1 : mode == 2 ? (int)fold_halfwg_auto(d) : 0;
}

// Tile block and grid of an F(2x3) launch (the launchers below and ramnet_fold_halfwg_grid): tx = tile columns of a block, 16 or 32 tiles
struct Wino23Grid {
    int tx, rows, cols, tiles_x, tiles_y;           // block = rows x cols outputs; blocks over the (Ho, Wt) map
    long wgs;                                       // workgroups = blocks x batch x 64-column channel blocks x parity classes
};
static Wino23Grid wino23_grid(const ramnet_conv_desc &d, bool half) {
    const bool dg = d.in_mode == RAMNET_IN_PARITY4, pair = !dg && fold_wino_pair(d.Cout, d.C0);
    // pair: column parity 1 is tiled with its origins one column to the left, so the tiles cover Wo + 1 columns
    const int Wt = pair ? d.Wo + 1 : d.Wo, ntiles = half ? 16 : 32;
    Wino23Grid g;
    if (half) wino23_tile_half(d.Ho, Wt, g.tx);
    else wino23_tile(d.Ho, Wt, g.tx);
    g.rows = 2 * (ntiles / g.tx), g.cols = 3 * g.tx;
    g.tiles_x = cdiv(Wt, g.cols), g.tiles_y = cdiv(d.Ho, g.rows);
    g.wgs = (long)g.tiles_x * g.tiles_y * d.B * (pair ? 1 : d.Cout / 64) * (dg ? 1 : pair ? 2 : 4);
    return g;
}

// auto: batch >= 2 and more half workgroups than the 512 that are resident at once (two on each of 256 CUs).  Isolated sweep of the three
// decoder layers, forward / pair / backward-data, batch 1-32 (tools/bench_fold23_halfwg.py, profiles/fold23_halfwg_sweep.jsonl): every such
// launch measured as fast or faster (forward 1.00-1.11, backward-data 1.04-1.46); the five launches that measured slower (0.97-0.995) all have
// 257-512 half workgroups — one resident round either way, the CUs' MFMA pipes shared by two workgroups instead of held by one.  Launches of
// at most 256 half workgroups measured 1.5-1.8 x faster (twice the CUs busy); they are batch 1-2 launches, which the callers run on F(2x2)
// with a split reduction, and stay on the 8-wave kernels.
static bool fold_halfwg_auto(const ramnet_conv_desc &d) { return d.B >= 2 && wino23_grid(d, true).wgs > 512; }

template <bool DG, bool PAIR, bool HALF = false>
static int launch_wino23(int tx, dim3 grid, size_t lds, const ramnet_conv_desc &d, const Wino24Params &q, hipStream_t st) {
#define W23_GO(T)                                                                                                         \
    if (tx == T) {                                                                                                        \
        RAMNET_FULL_LDS((conv_wino24_kernel<4, DG, T, PAIR, 3, HALF>));                                                     \
        if (HALF) note_kernel("conv_wino24_kernel<4,%d,%d,%d,3,1>", (int)DG, T, (int)PAIR);                                \
        else note_kernel("conv_wino24_kernel<4,%d,%d,%d,3>", (int)DG, T, (int)PAIR);                                       \
        hipLaunchKernelGGL((conv_wino24_kernel<4, DG, T, PAIR, 3, HALF>), grid, dim3(HALF ? 256 : 512), lds, st, d, q);     \
    }
    W23_GO(2) W23_GO(4) W23_GO(16)
    if constexpr (HALF) W23_GO(8)
#undef W23_GO
    RAMNET_LAUNCH_CHECK();
    return 0;
}

static int launch_wino24_dgrad(const ramnet_conv_desc &d, hipStream_t st) {
    RAMNET_CHECK_ARG(d.stride == 1 && d.C0 % 16 == 0 && d.Cout % 64 == 0);
    RAMNET_CHECK_ARG(d.Hin % 2 == 0 && d.Win % 2 == 0 && d.Ho == d.Hin / 2 + 4 && d.Wo == d.Win / 2 + 4 && d.HoF == d.Ho && d.WoF == d.Wo);
    RAMNET_CHECK_ARG(d.epi == RAMNET_EPI_LINEAR && !d.bias && d.beta == 0.f && d.frame == 0 && d.out_s2d == 0);
    Wino24Params q;
    q.x = d.x0, q.wp = d.w, q.Hp = d.Hin, q.Wp = d.Win, q.ldx = d.ld0;
    q.cpc = d.C0 / 16, q.nchunks = 4 * q.cpc, q.nblk = d.Cout / 64;
    q.ksplit = 1, q.ws = nullptr, q.cnt = nullptr;
    q.Hc = d.Hin / 2, q.Wc = d.Win / 2;
    const bool w23 = d.algo == RAMNET_ALGO_WINOGRAD24_2X3;
    const size_t xb = fold_x_bytes(d), wb = fold_w_bytes(d);
    RAMNET_CHECK_ARG(xb < FOLD_DGRAD_X_LIMIT && wb < FOLD_W_LIMIT);      // invalid window elements use offsets >= 2^30 (conv_plan.hpp)
    q.xbytes = (unsigned)xb, q.wbytes = (unsigned)wb;
    if (w23) {
        const bool half = fold_halfwg_variant(d, 0);
        const Wino23Grid g = wino23_grid(d, half);
        q.tiles_x = g.tiles_x, q.tiles_y = g.tiles_y;
        if (half) return launch_wino23<true, false, true>(g.tx, dim3((unsigned)g.wgs), (size_t)W23_V * sizeof(float), d, q, st);
        return launch_wino23<true, false>(g.tx, dim3((unsigned)g.wgs), (size_t)2 * W23_V * sizeof(float), d, q, st);
    }
    // 16 x 8 or 8 x 16 output pixels per workgroup: whichever covers the grid with fewer workgroups
    const bool flat = cdiv(d.Wo, 16) * cdiv(d.Ho, 8) < cdiv(d.Wo, 8) * cdiv(d.Ho, 16);
    q.tiles_x = cdiv(d.Wo, flat ? 16 : 8), q.tiles_y = cdiv(d.Ho, flat ? 8 : 16);
    const size_t lds = (size_t)2 * W24_V * sizeof(float);
    const dim3 grid((unsigned)(q.tiles_x * q.tiles_y * d.B * q.nblk));
    if (flat) {
        RAMNET_FULL_LDS((conv_wino24_kernel<4, true, 8>));
        note_kernel("conv_wino24_kernel<4,1,8,0>");
        hipLaunchKernelGGL((conv_wino24_kernel<4, true, 8>), grid, dim3(512), lds, st, d, q);
    } else {
        RAMNET_FULL_LDS((conv_wino24_kernel<4, true, 4>));
        note_kernel("conv_wino24_kernel<4,1,4,0>");
        hipLaunchKernelGGL((conv_wino24_kernel<4, true, 4>), grid, dim3(512), lds, st, d, q);
    }
    RAMNET_LAUNCH_CHECK();
    return 0;
}

// Split of the channel reduction a forward launch wants (1 = none): workgroups of 512 threads, one per CU — a launch that leaves more than
// half of the CUs empty (decoder 0 at batch 1: 96 workgroups of 16 chunks) splits towards one full round of 256 workgroups, at least four
// chunks (an even number) per split; every lane of a workgroup must own an output channel (the join has barriers).  Measured
// (tools/bench_split.py, whole layer): decoder 0 87.0 -> 65.8 us with 2 splits (4: 67.5); decoder 1 (176 workgroups) 63.9 -> 64.8 with 2: a
// second round of workgroups costs what the shorter chains save — not split.
static int wino24_ksplit(const ramnet_conv_desc &d, int gridx, int nchunks) {
    if (!g_opt_wino_ksplit || d.in_mode != RAMNET_IN_PLAIN) return 1;
    const bool pair = fold_wino_pair(d.Cout, d.C0), wide = pair || (d.Cout % 64 == 0 && d.C0 % 16 == 0);
    if (!pair && d.Cout % (wide ? 64 : 32) != 0) return 1;
    int ks = 256 / gridx < 4 ? 256 / gridx : 4;
    if (nchunks / 4 < ks) ks = nchunks / 4;
    if (g_opt_wino_ksplit > 1) ks = g_opt_wino_ksplit < nchunks / 2 ? g_opt_wino_ksplit : nchunks / 2;
    if (ks < 1) ks = 1;
    while (ks > 1 && (ks - 1) * (cdiv(nchunks / 2, ks) * 2) >= nchunks) --ks;        // every split owns chunks
    return ks;
}
static size_t wino24_ksplit_floats(unsigned gridx, int ks) { return (size_t)cdiv((int)gridx, 64) * 64 + (size_t)gridx * ks * 8192; }

// ramnet_conv_splitk_floats() for RAMNET_ALGO_WINOGRAD24 descriptors (same geometry as launch_wino24 below)
size_t wino24_splitk_floats(const ramnet_conv_desc &d) {
    if (d.in_mode != RAMNET_IN_PLAIN || d.C0 % 16 != 0 || d.Cout % 32 != 0) return 0;
    const bool pair = fold_wino_pair(d.Cout, d.C0), wide = pair || (d.Cout % 64 == 0 && d.C0 % 16 == 0);
    if (d.C0 % (wide ? 32 : 16) != 0) return 0;
    const int nchunks = d.C0 / (wide ? 16 : 8), nblk = pair ? 1 : d.Cout / (wide ? 64 : 32);
    const int Wt = pair ? d.Wo + 2 : d.Wo;
    const bool flat = wide && cdiv(Wt, 16) * cdiv(d.Ho, 8) < cdiv(Wt, 8) * cdiv(d.Ho, 16);
    const int tiles_x = cdiv(Wt, wide && !flat ? 8 : 16), tiles_y = cdiv(d.Ho, flat ? 8 : 16);
    const unsigned gridx = (unsigned)(tiles_x * tiles_y * d.B * nblk * (pair ? 2 : 4));
    const int ks = wino24_ksplit(d, (int)gridx, nchunks);
    return ks > 1 ? wino24_ksplit_floats(gridx, ks) : 0;
}

// Does this RAMNET_ALGO_WINOGRAD24 launch run F(2x3, 4x4) (RAMNET_ALGO_WINOGRAD24_2X3)?  Forward launches with 64-column workgroups
// (chunks of 16, the pair form included) and backward-data launches, not split, of at least one full round of workgroups (256: one
// per CU), where the F(2x3) launch is estimated faster: its workgroups run 30 positions where F(2x2) ones run 25, so the launch takes
// 30 x ceil(wgs23 / 256) against 25 x ceil(wgs22 / 256) position-times.  The isolated sweep of the three decoder layers over batch 1-32,
// forward and backward-data (tools/bench_fold23.py, profiles/fold23_sweep.jsonl), never picks a launch that measured slower (those are
// backward-data launches at batch <= 8, whose last, partial round of longer workgroups costs more than the 20 % fewer MFMAs save, and
// the launches below one round); ties go to F(2x2), and so do two forward launches below one round that F(2x3) would speed up (batch <= 2).
static int fold_wino_variant(const ramnet_conv_desc &d, int force) {
    if (d.algo != RAMNET_ALGO_WINOGRAD24 || d.stride != 1) return 0;
    long wgs22, wgs23;
    int tx;
    if (d.in_mode == RAMNET_IN_PARITY4) {
        if (d.C0 % 16 != 0 || d.Cout % 64 != 0) return 0;
        const bool flat = cdiv(d.Wo, 16) * cdiv(d.Ho, 8) < cdiv(d.Wo, 8) * cdiv(d.Ho, 16);
        wgs22 = (long)cdiv(d.Wo, flat ? 16 : 8) * cdiv(d.Ho, flat ? 8 : 16) * d.B * (d.Cout / 64);
        wgs23 = wino23_tile(d.Ho, d.Wo, tx) / 192 * d.B * (d.Cout / 64);
    } else if (d.in_mode == RAMNET_IN_PLAIN) {
        const bool pair = fold_wino_pair(d.Cout, d.C0), wide = pair || (d.Cout % 64 == 0 && d.C0 % 16 == 0);
        if (!wide || d.C0 % 32 != 0 || d.Ho < 2 || d.Wo < 2) return 0;
        const int Wt = pair ? d.Wo + 2 : d.Wo, nblk = pair ? 1 : d.Cout / 64, ncls = pair ? 2 : 4;
        const bool flat = cdiv(Wt, 16) * cdiv(d.Ho, 8) < cdiv(Wt, 8) * cdiv(d.Ho, 16);
        wgs22 = (long)cdiv(Wt, flat ? 16 : 8) * cdiv(d.Ho, flat ? 8 : 16) * d.B * nblk * ncls;
        wgs23 = wino23_tile(d.Ho, pair ? d.Wo + 1 : d.Wo, tx) / 192 * d.B * nblk * ncls;
        if (!force && wino24_ksplit(d, (int)wgs22, d.C0 / 16) > 1) return 0;          // split launches stay on F(2x2)
    } else {
        return 0;
    }
    if (force) return 1;                                            // (tests: every structurally eligible launch)
    return wgs23 >= 256 && 6 * ((wgs23 + 255) / 256) < 5 * ((wgs22 + 255) / 256) ? 1 : 0;
}

int launch_wino24(const ramnet_conv_desc &d, hipStream_t st) {
    if (d.in_mode == RAMNET_IN_PARITY4) return launch_wino24_dgrad(d, st);
    // d.x0 = replicate-padded low-res input [B][Hin = H+4][Win = W+4][C0]; Ho, Wo = the parity grid (H, W); HoF = 2H, WoF = 2W
    RAMNET_CHECK_ARG(d.in_mode == RAMNET_IN_PLAIN && d.stride == 1);
    const bool pair = fold_wino_pair(d.Cout, d.C0);            // both column parities of a 32-channel layer in one workgroup
    const bool wide = pair || (d.Cout % 64 == 0 && d.C0 % 16 == 0);      // 64-column workgroups, chunks of 16; else 32 channels, chunks of 8
    RAMNET_CHECK_ARG(d.C0 % (wide ? 32 : 16) == 0);            // an even number of chunks (the chunk loop is unrolled by two)
    RAMNET_CHECK_ARG(d.C0 % 8 == 0 && d.Cout % 32 == 0 && d.Hin == d.Ho + 4 && d.Win == d.Wo + 4 && d.HoF == 2 * d.Ho && d.WoF == 2 * d.Wo);
    RAMNET_CHECK_ARG((d.epi == RAMNET_EPI_RELU || d.epi == RAMNET_EPI_LINEAR) && d.beta == 0.f && d.out_s2d == 0 && d.Ho >= 2 && d.Wo >= 2);
    const bool w23 = d.algo == RAMNET_ALGO_WINOGRAD24_2X3;
    if (w23) RAMNET_CHECK_ARG(wide && d.splitk_ws == nullptr);     // F(2x3): 64-column workgroups, no split reduction
    Wino24Params q;
    q.x = d.x0, q.wp = d.w, q.Hp = d.Hin, q.Wp = d.Win, q.ldx = d.ld0;
    q.nchunks = d.C0 / (wide ? 16 : 8), q.nblk = pair ? 1 : d.Cout / (wide ? 64 : 32);
    q.Hc = d.Ho, q.Wc = d.Wo, q.cpc = 1;
    const size_t xb = fold_x_bytes(d), wb = fold_w_bytes(d);
    RAMNET_CHECK_ARG(xb < FOLD_X_LIMIT && wb < FOLD_W_LIMIT);
    q.xbytes = (unsigned)xb, q.wbytes = (unsigned)wb;
    if (w23) {
        q.ksplit = 1, q.ws = nullptr, q.cnt = nullptr;
        const bool half = fold_halfwg_variant(d, 0);
        const Wino23Grid g = wino23_grid(d, half);
        q.tiles_x = g.tiles_x, q.tiles_y = g.tiles_y;
        const dim3 grid((unsigned)g.wgs);
        if (half) {
            const size_t lds = (size_t)W23_V * sizeof(float);
            return pair ? launch_wino23<false, true, true>(g.tx, grid, lds, d, q, st) : launch_wino23<false, false, true>(g.tx, grid, lds, d, q, st);
        }
        const size_t lds = (size_t)2 * W23_V * sizeof(float);
        return pair ? launch_wino23<false, true>(g.tx, grid, lds, d, q, st) : launch_wino23<false, false>(g.tx, grid, lds, d, q, st);
    }
    const int Wt = pair ? d.Wo + 2 : d.Wo;                     // pair: one more tile column (the shifted tiling of column parity 1)
    const bool flat = wide && cdiv(Wt, 16) * cdiv(d.Ho, 8) < cdiv(Wt, 8) * cdiv(d.Ho, 16);      // 8 x 16 instead of 16 x 8 pixels
    q.tiles_x = cdiv(Wt, wide && !flat ? 8 : 16), q.tiles_y = cdiv(d.Ho, flat ? 8 : 16);
    const size_t lds = (size_t)2 * W24_V * sizeof(float);
    const unsigned gridx = (unsigned)(q.tiles_x * q.tiles_y * d.B * q.nblk * (pair ? 2 : 4));
    const int want = wino24_ksplit(d, (int)gridx, q.nchunks);
    q.ksplit = d.splitk_ws ? want : 1;
    q.cnt = reinterpret_cast<int *>(d.splitk_ws);
    q.ws = d.splitk_ws ? d.splitk_ws + cdiv((int)gridx, 64) * 64 : nullptr;
    if (q.ksplit > 1) RAMNET_CHECK_ARG(d.splitk_floats >= wino24_ksplit_floats(gridx, want) && ((uintptr_t)d.splitk_ws & 15) == 0);
    const dim3 grid(gridx, q.ksplit);
    if (pair && flat) {
        RAMNET_FULL_LDS((conv_wino24_kernel<4, false, 8, true>));
        note_kernel("conv_wino24_kernel<4,0,8,1>");
        hipLaunchKernelGGL((conv_wino24_kernel<4, false, 8, true>), grid, dim3(512), lds, st, d, q);
    } else if (pair) {
        RAMNET_FULL_LDS((conv_wino24_kernel<4, false, 4, true>));
        note_kernel("conv_wino24_kernel<4,0,4,1>");
        hipLaunchKernelGGL((conv_wino24_kernel<4, false, 4, true>), grid, dim3(512), lds, st, d, q);
    } else if (wide && flat) {
        RAMNET_FULL_LDS((conv_wino24_kernel<4, false, 8>));
        note_kernel("conv_wino24_kernel<4,0,8,0>");
        hipLaunchKernelGGL((conv_wino24_kernel<4, false, 8>), grid, dim3(512), lds, st, d, q);
    } else if (wide) {
        RAMNET_FULL_LDS((conv_wino24_kernel<4, false, 4>));
        note_kernel("conv_wino24_kernel<4,0,4,0>");
        hipLaunchKernelGGL((conv_wino24_kernel<4, false, 4>), grid, dim3(512), lds, st, d, q);
    } else {
        RAMNET_FULL_LDS((conv_wino24_kernel<2, false, 8>));
        note_kernel("conv_wino24_kernel<2,0,8,0>");
        hipLaunchKernelGGL((conv_wino24_kernel<2, false, 8>), grid, dim3(512), lds, st, d, q);
    }
    RAMNET_LAUNCH_CHECK();
    return 0;
}

// Backward-data of the folded layer on conv_wino24_kernel (RAMNET_IN_PARITY4): Winograd weights of the FLIPPED parity filters with the roles
// of the channels swapped — reduce over k = (parity class (p, q), output channel n), produce input channels c.  Layout = the forward pack's
// with one class, chunks of 16 and 64-column blocks: i = ((((chunk*NB + nb)*25 + pos)*4 + cq)*4 + ks)*64 + l15*4 + j,
// k = chunk*16 + ks*4 + j = (p*2 + q)*Cout + n, c = nb*64 + cq*16 + l15;
// U[a][b][k][c] = sum_{t,s} G[a][t] G[b][s] W4[n][c][p][q][3-t][3-s],  W4 = FA_p w FA_q^T (integer matrices and one division, like the forward pack)
template <int TW>
__global__ void pack_weight_fold_wino_dgrad_kernel(const float *__restrict__ w, float *__restrict__ wp, int Cout, int Cin, size_t total) {
    constexpr int WC = TW + 3, NP = 5 * WC;
    const int NB = Cin / 64;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t r = i;
        const int j = (int)(r & 3), l15 = (int)((r >> 2) & 15), ks = (int)((r >> 6) & 3), cq = (int)((r >> 8) & 3);
        r >>= 10;
        const int pos = (int)(r % NP);
        r /= NP;
        const int nb = (int)(r % NB), chunk = (int)(r / NB);
        const int k = chunk * 16 + ks * 4 + j, c = nb * 64 + cq * 16 + l15;
        const int pq = k / Cout, n = k - pq * Cout, pp = pq >> 1, qq = pq & 1, a = pos / WC, b = pos % WC;
        wp[i] = fold_wino_u(TW, a, b, pp, qq, true, w + ((size_t)n * Cin + c) * 25);
    }
}

// Border matrices of the folded layer (ops._folded_upsample_conv): the layer zero-pads where the folded form replicate-extends, so the taps
// that fall outside the image are taken out again through two small GEMMs per border.  rows[side][kx*Cin + ci][slot*Cout + co] =
// -sum_{a in LOST[side][slot]} w[co][ci][a][kx]; cols the same with the lost direction along kx; *_t = their transposes (backward-data).
__global__ void pack_border_weights_kernel(const float *__restrict__ w, float *__restrict__ rows, float *__restrict__ cols, float *__restrict__ rows_t,
                                           float *__restrict__ cols_t, int Cout, int Cin, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t r = i;
        const int co = (int)(r % Cout);
        r /= Cout;
        const int slot = (int)(r & 1);
        r >>= 1;
        const int ci = (int)(r % Cin);
        r /= Cin;
        const int kb = (int)(r % 5), side = (int)(r / 5);
        // LOST = [[(0, 1), (0,)], [(4,), (3, 4)]]
        const int a0 = side == 0 ? 0 : (slot == 0 ? 4 : 3), na = side == 0 ? (slot == 0 ? 2 : 1) : (slot == 0 ? 1 : 2);
        const float *wk = w + ((size_t)co * Cin + ci) * 25;
        float sr = 0.f, sc = 0.f;
        for (int e = 0; e < na; ++e) sr += wk[(a0 + e) * 5 + kb], sc += wk[kb * 5 + (a0 + e)];
        const size_t K = (size_t)kb * Cin + ci, N = (size_t)slot * Cout + co;
        rows[((size_t)side * 5 * Cin + K) * 2 * Cout + N] = -sr;
        cols[((size_t)side * 5 * Cin + K) * 2 * Cout + N] = -sc;
        rows_t[((size_t)side * 2 * Cout + N) * 5 * Cin + K] = -sr;
        cols_t[((size_t)side * 2 * Cout + N) * 5 * Cin + K] = -sc;
    }
}

// End of a backward pass of a folded decoder: dW5[o][i][k][l] += sum_{p,q,t,s} FA[p][t][k] FA[q][s][l] dW4[p][q][t][s][i][o]
//   - (border-GEMM gradients routed back to the taps they summed),   dW4 = w4 (direct parity launches) + G^T dU G (Winograd-domain launches)
//   + G^T dU3 Gc (F(2x3,4x4) launches, csrc/conv_wgrad_wino24.hip: [4][30][CinWs][Cout], Gc = fold_wino_gc3 / 3).
// One thread per (o, i); the workspaces it reads are zeroed for the next pass.
__global__ void fold_unpack_wgrad_kernel(float *__restrict__ w4, float *__restrict__ dU, float *__restrict__ dU3, float *__restrict__ wr,
                                         float *__restrict__ wc, float *__restrict__ grad, int Cout, int Cin, int CinWs) {
    // Folded in double through the integer matrices 4 FA, 6 G and 3 Gc with ONE division (as the packs above and unpack_wgrad_wino2x4_kernel):
    // 576 dW5 = sum (4 FA)(4 FA) [36 w4 + (6 G)^T dU (6 G) + 2 (6 G)^T dU3 (3 Gc)] — a gradient that is an fp32 number comes out as that number.
    const size_t total = (size_t)Cout * Cin;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int o = (int)(idx % Cout), i = (int)(idx / Cout);        // (consecutive threads: consecutive o = the workspaces' fastest index)
        double g5[25];
        for (int e = 0; e < 25; ++e) g5[e] = 0.0;
        for (int pq = 0; pq < 4; ++pq) {
            const int pp = pq >> 1, qq = pq & 1;
            double d4[16];                          // 36 dW4 of the class
            for (int ts = 0; ts < 16; ++ts) {
                float *cell = w4 + ((size_t)(pq * 16 + ts) * CinWs + i) * Cout + o;
                d4[ts] = 36.0 * (double)*cell;
                *cell = 0.f;
            }
            if (dU != nullptr) {
                for (int ab = 0; ab < 25; ++ab) {
                    float *cell = dU + ((size_t)(pq * 25 + ab) * CinWs + i) * Cout + o;
                    const double u = (double)*cell;
                    *cell = 0.f;
                    const int a = ab / 5, b = ab % 5;
                    for (int t = 0; t < 4; ++t)
                        for (int s = 0; s < 4; ++s) d4[t * 4 + s] += (double)(fold_wino_g6(a, t) * fold_wino_g6(b, s)) * u;
                }
            }
            if (dU3 != nullptr) {
                for (int ab = 0; ab < 30; ++ab) {
                    float *cell = dU3 + ((size_t)(pq * 30 + ab) * CinWs + i) * Cout + o;
                    const double u = (double)*cell;
                    *cell = 0.f;
                    const int a = ab / 6, b = ab % 6;
                    for (int t = 0; t < 4; ++t)
                        for (int s = 0; s < 4; ++s) d4[t * 4 + s] += (double)(2 * fold_wino_g6(a, t) * fold_wino_gc3(b, s)) * u;
                }
            }
            for (int t = 0; t < 4; ++t)
                for (int s = 0; s < 4; ++s) {
                    const double v = d4[t * 4 + s];
                    for (int k = 0; k < 5; ++k) {
                        const int fk = fold_fa4(pp, t, k);
                        if (fk == 0) continue;
                        for (int l = 0; l < 5; ++l) g5[k * 5 + l] += (double)(fk * fold_fa4(qq, s, l)) * v;
                    }
                }
        }
        for (int e = 0; e < 25; ++e) g5[e] /= 576.0;        // 16 from the two 4 FA, 36 from 6 G x 6 G (= 2 x 6 G x 3 Gc)
        for (int side = 0; side < 2; ++side)
            for (int slot = 0; slot < 2; ++slot) {
                const int a0 = side == 0 ? 0 : (slot == 0 ? 4 : 3), na = side == 0 ? (slot == 0 ? 2 : 1) : (slot == 0 ? 1 : 2);
                for (int kb = 0; kb < 5; ++kb) {
                    float *rc = wr + (((size_t)side * 5 + kb) * Cin + i) * 2 * Cout + (size_t)slot * Cout + o;
                    float *cc = wc + (((size_t)side * 5 + kb) * Cin + i) * 2 * Cout + (size_t)slot * Cout + o;
                    const double r = (double)*rc, c = (double)*cc;
                    *rc = 0.f, *cc = 0.f;
                    for (int e = 0; e < na; ++e) g5[(a0 + e) * 5 + kb] -= r, g5[kb * 5 + (a0 + e)] -= c;
                }
            }
        float *g = grad + ((size_t)o * Cin + i) * 25;
        for (int e = 0; e < 25; ++e) g[e] = (float)((double)g[e] + g5[e]);
    }
}

}  // namespace ramnet

using namespace ramnet;

extern "C" int ramnet_fold_wino_supported(int Cout, int Cin) {
    int kc, ncq;
    return fold_wino_geometry(Cout, Cin, kc, ncq) ? 1 : 0;
}

extern "C" size_t ramnet_packed_weight_elems_fold_wino(int Cout, int Cin) { return (size_t)100 * Cout * Cin; }

extern "C" int ramnet_pack_weight_fold_wino(const float *w, float *wp, int Cout, int Cin, void *stream) {
    int kc, ncq;
    RAMNET_CHECK_ARG(w && wp && Cout > 0 && Cin > 0 && fold_wino_geometry(Cout, Cin, kc, ncq));
    const size_t total = (size_t)100 * Cout * Cin;
    return launch_1d(pack_weight_fold_wino_kernel<2>, total, stream, w, wp, Cout, Cin, kc, ncq, (int)fold_wino_pair(Cout, Cin), total);
}

extern "C" int ramnet_pack_weight_fold_wino_dgrad(const float *w, float *wp, int Cout, int Cin, void *stream) {
    RAMNET_CHECK_ARG(w && wp && Cout > 0 && Cin > 0 && Cin % 64 == 0 && (4 * Cout) % 16 == 0);
    const size_t total = (size_t)100 * Cout * Cin;
    return launch_1d(pack_weight_fold_wino_dgrad_kernel<2>, total, stream, w, wp, Cout, Cin, total);
}

extern "C" size_t ramnet_packed_weight_elems_fold_wino2x3(int Cout, int Cin) { return (size_t)120 * Cout * Cin; }

extern "C" int ramnet_pack_weight_fold_wino2x3(const float *w, float *wp, int Cout, int Cin, void *stream) {
    int kc, ncq;
    RAMNET_CHECK_ARG(w && wp && Cout > 0 && Cin > 0 && fold_wino_geometry(Cout, Cin, kc, ncq) && kc == 16);
    const size_t total = (size_t)120 * Cout * Cin;
    return launch_1d(pack_weight_fold_wino_kernel<3>, total, stream, w, wp, Cout, Cin, kc, ncq, (int)fold_wino_pair(Cout, Cin), total);
}

extern "C" int ramnet_pack_weight_fold_wino2x3_dgrad(const float *w, float *wp, int Cout, int Cin, void *stream) {
    RAMNET_CHECK_ARG(w && wp && Cout > 0 && Cin > 0 && Cin % 64 == 0 && (4 * Cout) % 16 == 0);
    const size_t total = (size_t)120 * Cout * Cin;
    return launch_1d(pack_weight_fold_wino_dgrad_kernel<3>, total, stream, w, wp, Cout, Cin, total);
}

extern "C" int ramnet_fold_wino_variant(const ramnet_conv_desc *d, int force) { return d ? fold_wino_variant(*d, force) : 0; }

extern "C" int ramnet_fold_halfwg_variant(const ramnet_conv_desc *d, int force) { return d ? fold_halfwg_variant(*d, force) : 0; }

extern "C" int ramnet_fold_halfwg_grid(const ramnet_conv_desc *d, int half, int *block_rows, int *block_cols, long *workgroups) {
    RAMNET_CHECK_ARG(d && block_rows && block_cols && workgroups && fold_halfwg_variant(*d, 1));
    const Wino23Grid g = wino23_grid(*d, half != 0);
    *block_rows = g.rows, *block_cols = g.cols, *workgroups = g.wgs;
    return 0;
}

extern "C" int ramnet_pack_border_weights(const float *w, float *rows, float *cols, float *rows_t, float *cols_t, int Cout, int Cin, void *stream) {
    RAMNET_CHECK_ARG(w && rows && cols && rows_t && cols_t && Cout > 0 && Cin > 0);
    const size_t total = (size_t)2 * 5 * Cin * 2 * Cout;
    return launch_1d(pack_border_weights_kernel, total, stream, w, rows, cols, rows_t, cols_t, Cout, Cin, total);
}

extern "C" int ramnet_fold_unpack_wgrad(float *w4, float *dU, float *wr, float *wc, float *grad, int Cout, int Cin, int CinWs, void *stream) {
    RAMNET_CHECK_ARG(w4 && wr && wc && grad && Cout > 0 && Cin > 0 && CinWs >= Cin);
    const size_t total = (size_t)Cout * Cin;
    return launch_1d<128>(fold_unpack_wgrad_kernel, total, stream, w4, dU, (float *)nullptr, wr, wc, grad, Cout, Cin, CinWs);
}

extern "C" int ramnet_fold_unpack_wgrad2x3(float *w4, float *dU, float *dU3, float *wr, float *wc, float *grad, int Cout, int Cin, int CinWs,
                                           void *stream) {
    RAMNET_CHECK_ARG(w4 && wr && wc && grad && Cout > 0 && Cin > 0 && CinWs >= Cin);
    const size_t total = (size_t)Cout * Cin;
    return launch_1d<128>(fold_unpack_wgrad_kernel, total, stream, w4, dU, dU3, wr, wc, grad, Cout, Cin, CinWs);
}
