// The head layers' backward-weights kernel, included twice by conv_head.hip: HEADWG_SLAB 0 = the kernel whose workgroups meet by atomics in one
// workspace (HEADWG_KERNEL(name) = name: the text and the symbol it always had), HEADWG_SLAB 1 = its slab form conv_head_wgrad_kernel_slab
// (ramnet_wgrad_desc.dw_slabs > 0; at most RAMNET_WGRAD_SLAB_CAP workgroups walk the tiles).  A preprocessor switch and not a template
// parameter: the default instantiations keep their symbols and their register allocation.
template <int CR>
__global__ void __launch_bounds__(256, 2) HEADWG_KERNEL(conv_head_wgrad_kernel)(const HeadWgradParams p) {
    using G = HeadGeom<CR, HG_H>;
    constexpr int HT_H = HG_H, HP_PLANE = G::PLANE, WR = HG_H / 4;     // WR rows of 32 pixels per wave
    constexpr int MT = (G::KT + 31) / 32;           // 32-row blocks of the (tap, channel) index
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *P = smem;                                // [CR][HG_H + 4][HP_LD]
    float *Gt = smem + ((CR * HP_PLANE + 3) & ~3);  // [HG_H * 32][32]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;

    f32x16 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    // A row m = (tap, channel) mt*32 + l31 at pixel 2j + h of the wave's WR x 32 strip; B row = the same pixel, column l31
    int aoff[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int m = t * 32 + l31;
        const int tap = m / CR, c = m - tap * CR;
        aoff[t] = (m < G::KT ? c * HP_PLANE + (tap / 5) * HP_LD + tap % 5 : 0) + wave * WR * HP_LD + h;
    }
    const int boff = (wave * WR * 32 + h) * HG_LD + l31;
    float4 bsum = f4zero();                         // bias gradient partial of channel quad (tid & 7)

    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        int bid = tile;
        const int tx = bid % p.tiles_x;
        bid /= p.tiles_x;
        const int ty = bid % p.tiles_y, b = bid / p.tiles_y;
        const int oy0 = ty * HT_H, ox0 = tx * HT_W;
        __syncthreads();                            // the previous tile's readers are done
        head_stage_patch<CR, HG_H>(P, p.x, p.ld, b, oy0, ox0, p.H, p.W, tid);
#pragma unroll
        for (int i = 0; i < HT_H * HT_W * 8 / 256; ++i) {      // gradient tile: pixels x 8 channel quads
            const int sl = tid + i * 256, pix = sl >> 3, qd = sl & 7;
            const int oy = oy0 + (pix >> 5), ox = ox0 + (pix & 31);
            float4 r = f4zero();
            if (oy < p.H && ox < p.W && qd * 4 < p.Cout) {
                const size_t gp = (size_t)(b * p.H + oy) * p.W + ox;
                r = ld4(p.g + gp * p.ldg + qd * 4);
                if (p.gm) {
                    const float4 mk = ld4(p.gm + gp * p.ldgm + qd * 4);
                    r = make_float4(mk.x > 0.f ? r.x : 0.f, mk.y > 0.f ? r.y : 0.f, mk.z > 0.f ? r.z : 0.f, mk.w > 0.f ? r.w : 0.f);
                }
            }
            st4(Gt + pix * HG_LD + qd * 4, r);
            bsum = f4add(bsum, r);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < WR * 16; ++j) {         // the wave's pixels, two per MFMA
            const int po = ((2 * j) >> 5) * HP_LD + ((2 * j) & 31);
            const float bv = Gt[boff + 2 * j * HG_LD];
            float a[MT];
#pragma unroll
            for (int t = 0; t < MT; ++t) a[t] = P[aoff[t] + po];
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], bv, acc[t], 0, 0, 0);
        }
    }

    // fold the four waves' partials in LDS, then one atomic per element into ws[tap][Cin][Cout].  The waves take turns (plain
    // read-add-write: the lanes of ONE wave own distinct elements) — fp32 LDS atomics run at ~0.4 per clock and CU on gfx950
    // (profiles/r03_h_tuning_notes.md, voxelizer), MT * 4096 of them per workgroup were ~20 us of every workgroup's tail
    __syncthreads();
    float *red = smem;                              // [MT*32][32]  (red + bred = 5120 floats fit below the gradient tile's end)
    float *bred = smem + MT * 1024;                 // [32][32], behind red
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float *q = red + (t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * 32 + l31;
                    *q = (w == 0 ? 0.f : *q) + acc[t][r];
                }
        }
        if (w == 0) st4(bred + (tid >> 3) * 32 + (tid & 7) * 4, bsum);
        __syncthreads();
    }
    for (int i = tid; i < G::KT * 32; i += 256) {
        const int n = i & 31, m = i >> 5;
        const int tap = m / CR, c = m - tap * CR;
#if HEADWG_SLAB     // workgroup blockIdx.x owns slab blockIdx.x of dw [S][25][Cin][Cout] and of dbias [S][Cout] (no atomics)
        if (n < p.Cout) p.dw[(((size_t)blockIdx.x * 25 + tap) * p.Cin + c) * p.Cout + n] += red[i];
#else
        if (n < p.Cout) atomicAdd(p.dw + ((size_t)tap * p.Cin + c) * p.Cout + n, red[i]);
#endif
    }
    if (p.dbias != nullptr && tid < 32 && tid < p.Cout) {
        float t = 0.f;
        for (int g = 0; g < 32; ++g) t += bred[g * 32 + tid];
#if HEADWG_SLAB
        p.dbias[(size_t)blockIdx.x * p.Cout + tid] += t;
#else
        atomicAdd(p.dbias + tid, t);
#endif
    }
}

