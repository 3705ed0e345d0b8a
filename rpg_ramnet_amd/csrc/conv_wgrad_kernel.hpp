// The direct backward-weights kernel, included twice by conv_wgrad.hip: WGRAD_SLAB 0 = the kernel whose pixel splits meet by atomics in one
// workspace (WGRAD_KERNEL(name) = name: the text and the symbol it always had), WGRAD_SLAB 1 = its slab form conv_wgrad_kernel_slab
// (ramnet_wgrad_desc.dw_slabs > 0): split blockIdx.x owns slab blockIdx.x of dw [S][ntaps][Cin][Cout] and of dbias [S][Cout] and joins them by
// plain read-modify-write.  A preprocessor switch and not a template parameter: the default instantiations keep their symbols and their
// register allocation (several of them spill scalars, one vectors: a folded-away branch in the epilogue moved the spill counts).
// MAXT: accumulator tiles per wave; NSUB: 32-wide output-channel sub-tiles per workgroup (WBN = 32*NSUB).
// Accumulator tile (jt, ns): rows = (tap jt*tpm + row/cinp, channel row%cinp), cols = output channel ns*32 + col.
// Wave w owns ns = w % NSUB and tap tiles w/NSUB, w/NSUB + 4/NSUB, ...; waves with fewer real tiles run the same MAXT
// MFMAs on a valid dummy address (they would wait at the barrier anyway) so the K loop has no branches.
// CSUB = 2 (3x3 layers with >= 64 input channels): the workgroup owns 64 input x 64 output channels and wave w owns ALL taps
// of quadrant (input half w>>1, output half w&1): 9 tiles per wave, perfectly balanced, and the gradient tile is staged
// once per 64 input channels instead of once per 32.
template <int MAXT, int NSUB, int CSUB = 1>
__global__ void __launch_bounds__(256, CSUB == 2 ? 2 : 1) WGRAD_KERNEL(conv_wgrad_kernel)(const ramnet_wgrad_desc p, const WgradDerived q) {
    constexpr int WBN = 32 * NSUB, GQ = WBN / 4;   // GQ: channel quads per gradient-tile pixel
    constexpr int WCK = 32 * CSUB;                 // input channels per workgroup (shadows the namespace default)
    constexpr int TSTEP = CSUB == 2 ? 1 : 4 / NSUB;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *patch = smem;                         // [PH*PW][32]
    float *gsm = smem + q.PH * q.PW * WCK;       // [128][WBN]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kk = lane >> 5;
    const int ns = wave % NSUB, csub = CSUB == 2 ? wave / NSUB : 0, tap0 = CSUB == 2 ? 0 : wave / NSUB;
    const int ntw = (q.ntt - tap0 + TSTEP - 1) / TSTEP;
    const int c0 = blockIdx.y * WCK, n0 = blockIdx.z * WBN;
    const int cinp = 32 / q.tpm, sub = l31 / cinp, cl = l31 - sub * cinp;

    f32x16 acc[MAXT];
#pragma unroll
    for (int j = 0; j < MAXT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    int toffw[MAXT];                             // per-lane LDS offset of this lane's (tap, channel) row
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
        const int tap = (tap0 + TSTEP * j) * q.tpm + sub;
        toffw[j] = ((j < ntw && tap < p.ntaps) ? q.toff[tap] + cl : cl) + csub * 32;
    }

    float4 bsum = f4zero();                      // bias gradient partial: fixed channel quad (tid % GQ)
    const bool do_bias = p.dbias != nullptr && blockIdx.y == 0;

    for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
        int tt = tile;
        const int tx_i = tt % q.tiles_x;
        tt /= q.tiles_x;
        const int ty_i = tt % q.tiles_y;
        const int b = tt / q.tiles_y;
        const int oy0 = ty_i * q.TH, ox0 = tx_i * TWID;
        const int iy0 = oy0 * p.stride + q.dymin, ix0 = ox0 * p.stride + q.dxmin;
        __syncthreads();
        {   // gradient tile: TH*16 pixels x GQ channel quads, 4 loads (x2 with mask) in flight per batch
            constexpr int NG = 128 * GQ / 256;
            const int nsl = q.TH * TWID * GQ;
            stage_patch<WCK / 4, WCK, 4, 256>(patch, q.src, b, iy0, ix0, c0, q.PH, q.PW, tid);
#pragma unroll
            for (int h = 0; h < NG; h += 4) {
                float4 g[4], y[4];
                bool ok[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int s = tid + (h + i) * 256;
                    const int m = s / GQ, qd = s % GQ;
                    const int oy = oy0 + (m >> 4), ox = ox0 + (m & 15), n = n0 + qd * 4;
                    ok[i] = s < nsl && oy < p.Ho && ox < p.Wo && n < p.Cout;
                    const size_t pix = ((size_t)b * q.HoG + (oy * q.gsy + q.goy)) * q.WoG + (ox * q.gsx + q.gox);
                    g[i] = ld4(ok[i] ? p.dout + pix * p.ldg + n : p.dout);
                    if (p.gmask) y[i] = ld4(ok[i] ? p.gmask + pix * p.ldgm + n : p.gmask);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int s = tid + (h + i) * 256;
                    float4 r = g[i];
                    if (p.gmask) r = make_float4(y[i].x > 0.f ? r.x : 0.f, y[i].y > 0.f ? r.y : 0.f, y[i].z > 0.f ? r.z : 0.f, y[i].w > 0.f ? r.w : 0.f);
                    if (!ok[i]) r = f4zero();
                    if (s < nsl) st4(gsm + (s / GQ) * WBN + (s % GQ) * 4, r);
                    bsum = f4add(bsum, r);
                }
            }
        }
        __syncthreads();
        {   // K step = 2 pixels (lanes 0-31: pixel 2i, lanes 32-63: pixel 2i+1).  Two-stage operand pipeline pinned with
            // sched_barrier: the LDS reads of step i+1 are issued BEFORE the MFMAs of step i (left alone, hipcc sinks the
            // reads next to their use and every step eats a full LDS latency whenever the wave is alone on its SIMD).
            float a0[MAXT], a1[MAXT], b0, b1;
            auto fetch = [&](int i, float (&a)[MAXT], float &bv) {
                const int m = 2 * i + kk;
                bv = gsm[m * WBN + ns * 32 + l31];
                const float *pa = patch + (((m >> 4) * p.stride) * q.PW + (m & 15) * p.stride) * WCK;
#pragma unroll
                for (int j = 0; j < MAXT; ++j) a[j] = pa[toffw[j]];
            };
            auto mma = [&](const float (&a)[MAXT], float bv) {
#pragma unroll
                for (int j = 0; j < MAXT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], bv, acc[j], 0, 0, 0);
            };
            fetch(0, a0, b0);
            const int ksteps = q.TH * TWID / 2;
            for (int i = 0; i < ksteps; i += 2) {
                fetch(i + 1, a1, b1);
                __builtin_amdgcn_sched_barrier(0);
                mma(a0, b0);
                __builtin_amdgcn_sched_barrier(0);
                fetch(i + 2 < ksteps ? i + 2 : i, a0, b0);
                __builtin_amdgcn_sched_barrier(0);
                mma(a1, b1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    // D[row = (tap, input channel)][col = output channel] -> ws[(tap*Cin + c)*Cout + n]
    const int Cin = q.src.Cin;
    const int n = n0 + ns * 32 + l31;
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
        if (j >= ntw) continue;
#if WGRAD_SLAB      // split blockIdx.x owns slab blockIdx.x: the 16 old values are requested together, then stored (no atomics)
        float *dwb = p.dw + (size_t)blockIdx.x * p.ntaps * Cin * p.Cout;
        float old[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * kk;
            const int t = (tap0 + TSTEP * j) * q.tpm + row / cinp, c = c0 + csub * 32 + row % cinp;
            old[r] = (t < p.ntaps && c < Cin && n < p.Cout) ? dwb[((size_t)t * Cin + c) * p.Cout + n] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * kk;
            const int t = (tap0 + TSTEP * j) * q.tpm + row / cinp, c = c0 + csub * 32 + row % cinp;
            if (t < p.ntaps && c < Cin && n < p.Cout) dwb[((size_t)t * Cin + c) * p.Cout + n] = old[r] + acc[j][r];
        }
#else
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * kk;
            const int t = (tap0 + TSTEP * j) * q.tpm + row / cinp, c = c0 + csub * 32 + row % cinp;
            if (t < p.ntaps && c < Cin && n < p.Cout) atomicAdd(p.dw + ((size_t)t * Cin + c) * p.Cout + n, acc[j][r]);
        }
#endif
    }
    if (do_bias) {
        __syncthreads();
        float *red = smem;                        // [256 / GQ][WBN]
        st4(red + (tid / GQ) * WBN + (tid % GQ) * 4, bsum);
        __syncthreads();
        if (tid < WBN) {
            float s = 0.f;
            for (int g = 0; g < 256 / GQ; ++g) s += red[g * WBN + tid];
#if WGRAD_SLAB      // (one workgroup per (slab, channel block): blockIdx.y == 0)
            if (n0 + tid < p.Cout) p.dbias[(size_t)blockIdx.x * p.Cout + n0 + tid] += s;
#else
            if (n0 + tid < p.Cout) atomicAdd(p.dbias + n0 + tid, s);
#endif
        }
    }
}

