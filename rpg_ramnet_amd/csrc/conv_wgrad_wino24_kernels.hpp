// The two backward-weights kernels of the folded upsample-conv, included twice by conv_wgrad_wino24.hip: WG24_SLAB 0 = the kernels whose tile
// splits meet by atomics in one workspace (WG24_KERNEL(name) = name: the text and the symbols they always had), WG24_SLAB 1 = their slab forms
// name_slab (ramnet_wgrad_desc.dw_slabs > 0): split blockIdx.x owns slab blockIdx.x of a [S][4][25 | 30][Cin][Cout] workspace and joins it by a
// plain read-modify-write; the bias gradient is left to wgrad24_dbias_slab_kernel (the four classes of a split would meet in one row).  A
// preprocessor switch and not a template parameter: the default kernels keep their symbols, and they hold 112-128 accumulator registers at one
// workgroup per CU — anything in their epilogue, a folded-away branch included, moved their register allocation.
template <bool GM, bool WCI>
__global__ void __launch_bounds__(512, 1) WG24_KERNEL(conv_wgrad_wino24_kernel)(const Wgrad24Params p) {
    constexpr int G24_CI = WCI ? 64 : 32, G24_CO = WCI ? 32 : 64;
    constexpr int G24_V = 25 * G24_T * G24_CI, G24_Z = 25 * G24_T * G24_CO;      // 6400 / 12800 floats (or swapped)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *V = smem;                   // [2][25][8][CI]
    float *Z = smem + 2 * G24_V;       // [2][25][8][CO]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kk = lane >> 5;
    const int pg = wave >> 1, ch = wave & 1;                  // position group, half of the wider channel dimension
    const int p0 = pg == 0 ? 0 : 1 + 6 * pg;                  // positions p0 .. p0 + (pg == 0 ? 7 : 6) - 1
    const int cls = blockIdx.z / p.ncob, cob = blockIdx.z % p.ncob;
    const int py = cls >> 1, px = cls & 1;
    const int c0 = blockIdx.y * G24_CI, n0 = cob * G24_CO;
    const bool vrole = WCI || wave < 4, zrole = !WCI || wave < 4;      // the narrower operand has 256 items per batch, the wider 512
    const int vt = (tid / G24_CI) & 7, vc = tid % G24_CI;      // input item: (tile of the batch, input channel)
    const int zt = (tid / G24_CO) & 7, zc = tid % G24_CO;      // gradient item: (tile, output channel)

    f32x16 acc[7];
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    float vraw[25], zraw[4];
    float bsum = 0.f;
    // Loaders (round 4: 670 -> see the header; two run-time integer divisions, 64-bit pointer arithmetic, ten clamps and a select per value
    // before): the (image, tile row, tile column) of the thread's tile is divided out ONCE and then walks by the pre-divided grid stride
    // with carries; a value is one buffer load at lane offset + scalar offset.  The window of a tile that overhangs the grid, or lies past
    // the last tile, reads whatever finite data (or the zeros past the tensor) the offset finds: it only meets gradient entries that are
    // zero — the Winograd row / column that contains window line 4 multiplies A g's last line, which is the out-of-grid gradient itself.
    struct Walk { int tx, ty, b, T; };
    const int dT = G24_T * (int)gridDim.x;
    const int d_tx = dT % p.tiles_x, d_ty = (dT / p.tiles_x) % p.tiles_y, d_b = (dT / p.tiles_x) / p.tiles_y;
    auto walk_init = [&](Walk &w, int batch, int tile) {
        w.T = batch * G24_T + tile;
        int t = w.T;
        w.tx = t % p.tiles_x;
        t /= p.tiles_x;
        w.ty = t % p.tiles_y, w.b = t / p.tiles_y;
    };
    auto walk_step = [&](Walk &w, int adv) {            // adv = 1: the next batch of this workgroup, 0: the same one again (clamped tail)
        w.T += adv * dT;
        w.tx += adv * d_tx;
        const int cx = w.tx >= p.tiles_x ? 1 : 0;
        w.tx -= cx * p.tiles_x;
        w.ty += adv * d_ty + cx;
        const int cy = w.ty >= p.tiles_y ? 1 : 0;
        w.ty -= cy * p.tiles_y;
        w.b += adv * d_b + cy;
    };
    Walk wv, wz;
    int lbv = 0, lbz = 0;                               // batch the walks stand at
    const auto rx = wino_rsrc(p.x, (unsigned)min((size_t)p.xbytes, (size_t)WOOB));
    const auto rg = wino_rsrc(p.g, (unsigned)min((size_t)p.gbytes, (size_t)WOOB));
    const auto rgm = GM ? wino_rsrc(p.gm, (unsigned)min((size_t)p.gmbytes, (size_t)WOOB)) : rg;
    const bool vch_ok = c0 + vc < p.Cin, zch_ok = n0 + zc < p.Cout;
    const unsigned zch = (unsigned)(n0 + zc);
    const int rowB = p.Wp * p.ldx * 4, colB = p.ldx * 4;                              // bytes per window row / column
    auto load_v = [&](int batch) {
        walk_step(wv, batch != lbv ? 1 : 0);
        lbv = batch;
        const unsigned base = (unsigned)(((wv.b * p.Hp + 2 * wv.ty + py) * p.Wp + 2 * wv.tx + px) * p.ldx + c0 + vc) * 4u;
        const unsigned lane_off = ((wv.T < p.ntiles) & vch_ok) ? base : WOOB;
#pragma unroll
        for (int r = 0; r < 5; ++r)
#pragma unroll
            for (int c = 0; c < 5; ++c)
                vraw[r * 5 + c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, (int)(lane_off + (unsigned)(r * rowB)), c * colB, 0));
    };
    auto load_z = [&](int batch, bool count) {
        walk_step(wz, batch != lbz ? 1 : 0);
        lbz = batch;
        const bool tok = (wz.T < p.ntiles) & zch_ok;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int oy = 2 * wz.ty + a, ox = 2 * wz.tx + c;
                const bool ok = tok & (oy < p.Hc) & (ox < p.Wc);
                const unsigned pix = (unsigned)((wz.b * p.H2 + 2 * oy + py) * p.W2 + 2 * ox + px);
                float v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, (int)(ok ? (pix * p.ldg + zch) * 4u : WOOB), 0, 0));
                if (GM) {
                    const float m = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rgm, (int)(ok ? (pix * p.ldgm + zch) * 4u : WOOB), 0, 0));
                    v = m > 0.f ? v : 0.f;
                }
                zraw[a * 2 + c] = v;
                if (count) bsum += v;
            }
    };
    // B^T = [2 -1 -2 1 0; 0 -2 -1 1 0; 0 2 -3 1 0; 0 -1 0 1 0; 0 2 -1 -2 1]
    auto v_cols = [&]() {
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const float d0 = vraw[c], d1 = vraw[5 + c], d2 = vraw[10 + c], d3 = vraw[15 + c], d4 = vraw[20 + c];
            vraw[c] = 2.f * (d0 - d2) - d1 + d3;
            vraw[5 + c] = d3 - d2 - 2.f * d1;
            vraw[10 + c] = 2.f * d1 - 3.f * d2 + d3;
            vraw[15 + c] = d3 - d1;
            vraw[20 + c] = 2.f * (d1 - d3) - d2 + d4;
        }
    };
    auto v_row = [&](float *vbuf, int i) {
        const float d0 = vraw[i * 5], d1 = vraw[i * 5 + 1], d2 = vraw[i * 5 + 2], d3 = vraw[i * 5 + 3], d4 = vraw[i * 5 + 4];
        float *dst = vbuf + ((i * 5) * G24_T + vt) * G24_CI + vc;
        dst[0 * G24_T * G24_CI] = 2.f * (d0 - d2) - d1 + d3;
        dst[1 * G24_T * G24_CI] = d3 - d2 - 2.f * d1;
        dst[2 * G24_T * G24_CI] = 2.f * d1 - 3.f * d2 + d3;
        dst[3 * G24_T * G24_CI] = d3 - d1;
        dst[4 * G24_T * G24_CI] = 2.f * (d1 - d3) - d2 + d4;
    };
    // Z = A g A^T, A = [1 0; 1 1; 1 -1; 1 2; 0 1]: row i of Z from w_i = (g0*, g0*+g1*, g0*-g1*, g0*+2 g1*, g1*)
    auto z_row = [&](float *zbuf, int i) {
        float w0, w1;                                   // (A g)[i][0], (A g)[i][1]
        if (i == 0) w0 = zraw[0], w1 = zraw[1];
        if (i == 1) w0 = zraw[0] + zraw[2], w1 = zraw[1] + zraw[3];
        if (i == 2) w0 = zraw[0] - zraw[2], w1 = zraw[1] - zraw[3];
        if (i == 3) w0 = zraw[0] + 2.f * zraw[2], w1 = zraw[1] + 2.f * zraw[3];
        if (i == 4) w0 = zraw[2], w1 = zraw[3];
        float *dst = zbuf + ((i * 5) * G24_T + zt) * G24_CO + zc;
        dst[0 * G24_T * G24_CO] = w0;
        dst[1 * G24_T * G24_CO] = w0 + w1;
        dst[2 * G24_T * G24_CO] = w0 - w1;
        dst[3 * G24_T * G24_CO] = w0 + 2.f * w1;
        dst[4 * G24_T * G24_CO] = w1;
    };

    const int step = gridDim.x;
    int batch = blockIdx.x;
    if (batch < p.nbatch) {
        const int last = batch + ((p.nbatch - 1 - batch) / step) * step;
        // prologue: batch -> buffer 0; raw data of the next batch in registers
        walk_init(wv, batch, vt), walk_init(wz, batch, zt);
        lbv = lbz = batch;
        if (zrole) load_z(batch, true);
        if (vrole) load_v(batch);
        if (zrole) {
#pragma unroll
            for (int i = 0; i < 5; ++i) z_row(Z, i);
        }
        if (vrole) {
            v_cols();
#pragma unroll
            for (int i = 0; i < 5; ++i) v_row(V, i);
        }
        {
            const bool more = batch + step <= last;
            if (zrole) load_z(min(batch + step, last), more);
            if (vrole) load_v(min(batch + step, last));
        }
        __syncthreads();
        const int aoff = (kk * 4) * G24_CI + (WCI ? ch * 32 : 0) + l31, boff = (kk * 4) * G24_CO + (WCI ? 0 : ch * 32) + l31;
        int buf = 0;
        for (; batch <= last; batch += step, buf ^= 1) {
            const float *vb = V + buf * G24_V, *zb = Z + buf * G24_Z;
            float *vn = V + (buf ^ 1) * G24_V, *zn = Z + (buf ^ 1) * G24_Z;
            const int b2 = min(batch + 2 * step, last);
            const bool more2 = batch + 2 * step <= last;
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                if (q < 6 || pg == 0) {
                    const int pos = p0 + q;
                    const float *ap = vb + pos * (G24_T * G24_CI) + aoff, *bp = zb + pos * (G24_T * G24_CO) + boff;
                    const float a0 = ap[0], a1 = ap[G24_CI], a2 = ap[2 * G24_CI], a3 = ap[3 * G24_CI];
                    const float b0 = bp[0], b1 = bp[G24_CO], b2v = bp[2 * G24_CO], b3 = bp[3 * G24_CO];
                    __builtin_amdgcn_sched_barrier(0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[q], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    // raw data of the next batch (in registers) -> the other LDS buffer; then the loads of the batch after it
                    if (q == 0 && zrole) z_row(zn, 0), z_row(zn, 1), z_row(zn, 2);
                    if (q == 1 && zrole) z_row(zn, 3), z_row(zn, 4);
                    if (q == 2 && vrole) v_cols();
                    if (q == 3 && vrole) v_row(vn, 0), v_row(vn, 1), v_row(vn, 2);
                    if (q == 4 && vrole) v_row(vn, 3), v_row(vn, 4);
                    if (q == 4) {
                        if (zrole) load_z(b2, more2);
                        if (vrole) load_v(b2);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b2v, acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b3, acc[q], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __syncthreads();
        }
    }

    // D[row = input channel][col = output channel] of position p0 + q -> dw[((cls*25 + pos)*Cin + c)*Cout + n]
    const int n = n0 + (WCI ? 0 : ch * 32) + l31;
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        if (q < 6 || pg == 0) {
#if WG24_SLAB       // split blockIdx.x owns slab blockIdx.x: the 16 old values are requested together, then stored (no atomics)
            float *col = p.dw + (((size_t)blockIdx.x * 4 + cls) * 25 + p0 + q) * p.Cin * p.Cout + n;
            float old[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = c0 + (WCI ? ch * 32 : 0) + (r & 3) + 8 * (r >> 2) + 4 * kk;
                old[r] = (c < p.Cin && n < p.Cout) ? col[(size_t)c * p.Cout] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = c0 + (WCI ? ch * 32 : 0) + (r & 3) + 8 * (r >> 2) + 4 * kk;
                if (c < p.Cin && n < p.Cout) col[(size_t)c * p.Cout] = old[r] + acc[q][r];
            }
#else
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = c0 + (WCI ? ch * 32 : 0) + (r & 3) + 8 * (r >> 2) + 4 * kk;
                if (c < p.Cin && n < p.Cout) atomicAdd(p.dw + (((size_t)cls * 25 + p0 + q) * p.Cin + c) * p.Cout + n, acc[q][r]);
            }
#endif
        }
    }
    if (!WG24_SLAB && p.dbias != nullptr && blockIdx.y == 0) {      // (slab form: wgrad24_dbias_slab_kernel)
        __syncthreads();
        float *red = smem;                        // [8][CO]
        if (zrole) red[zt * G24_CO + zc] = bsum;
        __syncthreads();
        if (tid < G24_CO) {
            float t = 0.f;
            for (int g = 0; g < 8; ++g) t += red[g * G24_CO + tid];
            if (n0 + tid < p.Cout) atomicAdd(p.dbias + n0 + tid, t);
        }
    }
}

// ---- F(2x3,4x4): 2 x 3 gradient tiles, 30 positions per 6 outputs (5.0 products per output instead of 6.25) ---------------------------
//     dU_cls[pos = a*6 + b][ci][co] = sum_tiles V * Z,   V = B^T d Bc over the 5 x 6 window,   Z = A g Ac^T of the 2 x 3 tile,
// rows as above, columns on the 6-point F(3,4) of csrc/conv_wino24.hip (TW = 3; points 0, 1, -1, 1/2, -1/2, inf):
//     Bc^T = [1/4 0 -5/4 0 1 0; 0 -1/4 -1/4 1 1 0; 0 1/4 -1/4 -1 1 0; 0 -1/2 -1 1/2 1 0; 0 1/2 -1 -1/2 1 0; 0 1/4 0 -5/4 0 1]
//     Ac^T = [1 1 1 1 1 0; 0 1 -1 1/2 -1/2 0; 0 1 1 1/4 1/4 1];   dW4 = G^T dU Gc (ramnet_fold_unpack_wgrad2x3).
// Two buffers of 30 positions x 8 tiles do not fit the 160 KB of a CU: a batch is 6 tiles (3 MFMAs of K = 2 per position; 2 x 30 x 6 x 96 x 4 B
// = 138 KB).  A batch has 192 input and 384 gradient items (or 384 and 192, WCI), one per lane: three (six) waves load and transform inputs,
// the other five (two) gradients, one of them two items per lane — no wave loads both operands.  Wave (position group of 8/8/7/7, channel
// half) accumulates 32 x 32 per position (128 VGPRs).  What differs from the F(2x2) loop above besides the tile (isolated launches at batch 16,
// profiles/fold23_wgrad_notes.md): the ReLU mask and the bias sum are applied when the transform reads the gradients, not next to their
// loads, and each operand's loads are issued as soon as its registers are free (-6 %); loaders apart per wave (a further -3 to -15 %).
//
// Overhang.  Rows are those of the F(2x2) kernel: window row 4 of a tile whose second gradient row lies outside the grid enters Winograd
// row 4 only, which multiplies (A g)'s last row, the out-of-grid gradient itself: zero.  Columns: a window that starts at 3 tx + px reaches
// column 3 tx + px + 5 of the Wo + 4 padded ones.  Window column 5 enters position b = 5 only (Bc^T's last row), whose Z is g's third column
// alone; it lies past the row's end only where that gradient column is outside the grid (Wo % 3 != 0): it meets zeros.  Window column 4 enters
// positions 0-4, which also carry g's FIRST column; it lies past the row's end exactly for px = 1 in the last tile column when Wo % 3 == 1
// (one valid gradient column) — in exact arithmetic G^T (.) Gc annihilates that product (it belongs to filter tap 4 of 0..3), in fp32 only
// up to rounding, so the loader reads that column as zeros (one select per batch on its lane offset).  Everything else a window reads past
// a row's end is finite data of the next row (or the zeros past the tensor) times a zero gradient.

template <bool GM, bool WCI>
__global__ void __launch_bounds__(512, 1) WG24_KERNEL(conv_wgrad_wino24_kernel_2x3)(const Wgrad24Params p) {
    constexpr int CI = WCI ? 64 : 32, CO = WCI ? 32 : 64;
    constexpr int NV = G23_NP * G23_T * CI, NZ = G23_NP * G23_T * CO;            // 5760 / 11520 floats (or swapped)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *V = smem;                   // [2][30][6][CI]
    float *Z = smem + 2 * NV;          // [2][30][6][CO]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kk = lane >> 5;
    const int pg = wave >> 1, ch = wave & 1;                  // position group, half of the wider channel dimension
    const int p0 = pg < 2 ? 8 * pg : 2 + 7 * pg;              // positions p0 .. p0 + (pg < 2 ? 8 : 7) - 1
    const int cls = blockIdx.z / p.ncob, cob = blockIdx.z % p.ncob;
    const int py = cls >> 1, px = cls & 1;
    const int c0 = blockIdx.y * CI, n0 = cob * CO;
    // 192 or 384 input items (three or six waves, one item per lane) and 384 or 192 gradient items per batch: no wave loads both operands
    // (its waits for the older loads of one would also wait for the younger loads of the other), so one gradient wave carries two items per lane
    const bool vrole = WCI ? wave < 6 : wave >= 5, zrole = WCI ? wave >= 6 : wave < 5;
    const bool z2 = wave == (WCI ? 6 : 4);
    const int vi = WCI ? tid : max(tid - 320, 0), zi = WCI ? (wave == 7 ? 128 + lane : lane) : tid;
    const int vt = vi / CI, vc = vi % CI;                     // input item: (tile of the batch, input channel)
    const int zt = zi / CO, zc = zi % CO;                     // gradient item: (tile, output channel)

    f32x16 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    float vraw[30], zraw[12], zmraw[GM ? 12 : 1];          // (gradient items: the second one of a z2 wave at 6..11)
    float bsum = 0.f;
    bool zcnt = false;                                  // do the gradients in zraw enter the bias sum (not a repeat of the clamped tail)?
    // the walks of the F(2x2) kernel over the grid of 2 x 3 tiles
    struct Walk { int tx, ty, b, T; };
    const int dT = G23_T * (int)gridDim.x;
    const int d_tx = dT % p.tiles_x, d_ty = (dT / p.tiles_x) % p.tiles_y, d_b = (dT / p.tiles_x) / p.tiles_y;
    auto walk_init = [&](Walk &w, int batch, int tile) {
        w.T = batch * G23_T + tile;
        int t = w.T;
        w.tx = t % p.tiles_x;
        t /= p.tiles_x;
        w.ty = t % p.tiles_y, w.b = t / p.tiles_y;
    };
    auto walk_step = [&](Walk &w, int adv) {            // adv = 1: the next batch of this workgroup, 0: the same one again (clamped tail)
        w.T += adv * dT;
        w.tx += adv * d_tx;
        const int cx = w.tx >= p.tiles_x ? 1 : 0;
        w.tx -= cx * p.tiles_x;
        w.ty += adv * d_ty + cx;
        const int cy = w.ty >= p.tiles_y ? 1 : 0;
        w.ty -= cy * p.tiles_y;
        w.b += adv * d_b + cy;
    };
    Walk wv, wz, wz2;
    int lbv = 0, lbz = 0;                               // batch the walks stand at
    const auto rx = wino_rsrc(p.x, (unsigned)min((size_t)p.xbytes, (size_t)WOOB));
    const auto rg = wino_rsrc(p.g, (unsigned)min((size_t)p.gbytes, (size_t)WOOB));
    const auto rgm = GM ? wino_rsrc(p.gm, (unsigned)min((size_t)p.gmbytes, (size_t)WOOB)) : rg;
    const bool vch_ok = c0 + vc < p.Cin, zch_ok = n0 + zc < p.Cout;
    const unsigned zch = (unsigned)(n0 + zc);
    const int rowB = p.Wp * p.ldx * 4, colB = p.ldx * 4;                              // bytes per window row / column
    auto load_v = [&](int batch) {
        walk_step(wv, batch != lbv ? 1 : 0);
        lbv = batch;
        const int wx = 3 * wv.tx + px;
        const unsigned base = (unsigned)(((wv.b * p.Hp + 2 * wv.ty + py) * p.Wp + wx) * p.ldx + c0 + vc) * 4u;
        const bool ok = (wv.T < p.ntiles) & vch_ok;
        const unsigned lane_off = ok ? base : WOOB;
        const unsigned lane_off4 = (ok & (wx + 4 < p.Wp)) ? base : WOOB;          // window column 4 past the row's end: zeros (header)
#pragma unroll
        for (int r = 0; r < 5; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c)
                vraw[r * 6 + c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, (int)((c == 4 ? lane_off4 : lane_off) + (unsigned)(r * rowB)), c * colB, 0));
    };
    auto load_z1 = [&](Walk &wz, int o, int adv) {
        walk_step(wz, adv);
        const bool tok = (wz.T < p.ntiles) & zch_ok;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int oy = 2 * wz.ty + a, ox = 3 * wz.tx + c;
                const bool ok = tok & (oy < p.Hc) & (ox < p.Wc);
                const unsigned pix = (unsigned)((wz.b * p.H2 + 2 * oy + py) * p.W2 + 2 * ox + px);
                // (the top bit instead of a select between the offset and WOOB: the compiler turns that select into two loads of one register
                //  under complementary masks, the second behind a wait for the first — six memory latencies in a row)
                const unsigned oob = ok ? 0u : 0x80000000u;
                zraw[o + a * 3 + c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, (int)(((pix * p.ldg + zch) * 4u) | oob), 0, 0));
                if (GM) zmraw[o + a * 3 + c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rgm, (int)(((pix * p.ldgm + zch) * 4u) | oob), 0, 0));
            }
    };
    auto load_z = [&](int batch, bool count) {
        const int adv = batch != lbz ? 1 : 0;
        lbz = batch;
        load_z1(wz, 0, adv);
        if (z2) load_z1(wz2, 6, adv);
        zcnt = count;
    };
    // The ReLU mask and the bias sum wait until the transform reads the values: a use next to the loads would hold the wave (and its MFMAs)
    // for the whole memory latency once per batch.
    auto z_mask = [&]() {
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            if (i < 6 || z2) {
                if (GM) zraw[i] = zmraw[i] > 0.f ? zraw[i] : 0.f;
                bsum += zcnt ? zraw[i] : 0.f;
            }
        }
    };
    // rows: B^T of F(2,4) down the 5 window rows, for each of the 6 window columns
    auto v_cols = [&]() {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float d0 = vraw[c], d1 = vraw[6 + c], d2 = vraw[12 + c], d3 = vraw[18 + c], d4 = vraw[24 + c];
            vraw[c] = 2.f * (d0 - d2) - d1 + d3;
            vraw[6 + c] = d3 - d2 - 2.f * d1;
            vraw[12 + c] = 2.f * d1 - 3.f * d2 + d3;
            vraw[18 + c] = d3 - d1;
            vraw[24 + c] = 2.f * (d1 - d3) - d2 + d4;
        }
    };
    // columns: Bc^T of F(3,4) along the 6 window columns of Winograd row i
    auto v_row = [&](float *vbuf, int i) {
        const float d0 = vraw[i * 6], d1 = vraw[i * 6 + 1], d2 = vraw[i * 6 + 2], d3 = vraw[i * 6 + 3], d4 = vraw[i * 6 + 4], d5 = vraw[i * 6 + 5];
        float *dst = vbuf + ((i * 6) * G23_T + vt) * CI + vc;
        const float e = d4 - 0.25f * d2, o = d3 - 0.25f * d1;            // even / odd parts of the +-1 pair
        const float f = d4 - d2, h = 0.5f * (d3 - d1);                   // ... and of the +-1/2 pair
        dst[0 * G23_T * CI] = 0.25f * d0 - 1.25f * d2 + d4;
        dst[1 * G23_T * CI] = e + o;
        dst[2 * G23_T * CI] = e - o;
        dst[3 * G23_T * CI] = f + h;
        dst[4 * G23_T * CI] = f - h;
        dst[5 * G23_T * CI] = 0.25f * d1 - 1.25f * d3 + d5;
    };
    // Z = A g Ac^T: row i of (A g) = (g0*, g0*+g1*, g0*-g1*, g0*+2 g1*, g1*), then its three entries through Ac^T
    auto z_row1 = [&](float *zbuf, int i, const float *zraw, int zt) {
        float w0, w1, w2;
        if (i == 0) w0 = zraw[0], w1 = zraw[1], w2 = zraw[2];
        if (i == 1) w0 = zraw[0] + zraw[3], w1 = zraw[1] + zraw[4], w2 = zraw[2] + zraw[5];
        if (i == 2) w0 = zraw[0] - zraw[3], w1 = zraw[1] - zraw[4], w2 = zraw[2] - zraw[5];
        if (i == 3) w0 = zraw[0] + 2.f * zraw[3], w1 = zraw[1] + 2.f * zraw[4], w2 = zraw[2] + 2.f * zraw[5];
        if (i == 4) w0 = zraw[3], w1 = zraw[4], w2 = zraw[5];
        float *dst = zbuf + ((i * 6) * G23_T + zt) * CO + zc;
        const float s = w0 + w2, q = w0 + 0.25f * w2;
        dst[0 * G23_T * CO] = w0;
        dst[1 * G23_T * CO] = s + w1;
        dst[2 * G23_T * CO] = s - w1;
        dst[3 * G23_T * CO] = q + 0.5f * w1;
        dst[4 * G23_T * CO] = q - 0.5f * w1;
        dst[5 * G23_T * CO] = w2;
    };
    auto z_row = [&](float *zbuf, int i) {
        z_row1(zbuf, i, zraw, zt);
        if (z2) z_row1(zbuf, i, zraw + 6, zt + 64 / CO);
    };

    const int step = gridDim.x;
    int batch = blockIdx.x;
    if (batch < p.nbatch) {
        const int last = batch + ((p.nbatch - 1 - batch) / step) * step;
        // prologue: batch -> buffer 0; raw data of the next batch in registers
        walk_init(wv, batch, vt), walk_init(wz, batch, zt), walk_init(wz2, batch, zt + 64 / CO);
        lbv = lbz = batch;
        if (zrole) load_z(batch, true);
        if (vrole) load_v(batch);
        if (zrole) {
            z_mask();
#pragma unroll
            for (int i = 0; i < 5; ++i) z_row(Z, i);
        }
        if (vrole) {
            v_cols();
#pragma unroll
            for (int i = 0; i < 5; ++i) v_row(V, i);
        }
        {
            const bool more = batch + step <= last;
            if (zrole) load_z(min(batch + step, last), more);
            if (vrole) load_v(min(batch + step, last));
        }
        __syncthreads();
        const int aoff = (kk * 3) * CI + (WCI ? ch * 32 : 0) + l31, boff = (kk * 3) * CO + (WCI ? 0 : ch * 32) + l31;
        int buf = 0;
        for (; batch <= last; batch += step, buf ^= 1) {
            const float *vb = V + buf * NV, *zb = Z + buf * NZ;
            float *vn = V + (buf ^ 1) * NV, *zn = Z + (buf ^ 1) * NZ;
            const int b2 = min(batch + 2 * step, last);
            const bool more2 = batch + 2 * step <= last;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (q < 7 || pg < 2) {
                    const int pos = p0 + q;
                    const float *ap = vb + pos * (G23_T * CI) + aoff, *bp = zb + pos * (G23_T * CO) + boff;
                    const float a0 = ap[0], a1 = ap[CI], a2 = ap[2 * CI];
                    const float b0 = bp[0], b1 = bp[CO], b2v = bp[2 * CO];
                    __builtin_amdgcn_sched_barrier(0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[q], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    // raw data of the next batch (in registers) -> the other LDS buffer; the loads of the batch after it are issued as soon as
                    // their registers are free and stay in flight for 5-6 positions
                    if (q == 0 && zrole) z_mask(), z_row(zn, 0), z_row(zn, 1), z_row(zn, 2);
                    if (q == 1 && zrole) z_row(zn, 3), z_row(zn, 4), load_z(b2, more2);
                    if (q == 2 && vrole) v_cols();
                    if (q == 3 && vrole) v_row(vn, 0), v_row(vn, 1), v_row(vn, 2);
                    if (q == 4 && vrole) v_row(vn, 3), v_row(vn, 4), load_v(b2);
                    __builtin_amdgcn_sched_barrier(0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b2v, acc[q], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __syncthreads();
        }
    }

    // D[row = input channel][col = output channel] of position p0 + q -> dw[((cls*30 + pos)*Cin + c)*Cout + n]
    const int n = n0 + (WCI ? 0 : ch * 32) + l31;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        if (q < 7 || pg < 2) {
#if WG24_SLAB       // split blockIdx.x owns slab blockIdx.x: the 16 old values are requested together, then stored (no atomics)
            float *col = p.dw + (((size_t)blockIdx.x * 4 + cls) * G23_NP + p0 + q) * p.Cin * p.Cout + n;
            float old[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = c0 + (WCI ? ch * 32 : 0) + (r & 3) + 8 * (r >> 2) + 4 * kk;
                old[r] = (c < p.Cin && n < p.Cout) ? col[(size_t)c * p.Cout] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = c0 + (WCI ? ch * 32 : 0) + (r & 3) + 8 * (r >> 2) + 4 * kk;
                if (c < p.Cin && n < p.Cout) col[(size_t)c * p.Cout] = old[r] + acc[q][r];
            }
#else
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = c0 + (WCI ? ch * 32 : 0) + (r & 3) + 8 * (r >> 2) + 4 * kk;
                if (c < p.Cin && n < p.Cout) atomicAdd(p.dw + (((size_t)cls * G23_NP + p0 + q) * p.Cin + c) * p.Cout + n, acc[q][r]);
            }
#endif
        }
    }
    if (!WG24_SLAB && p.dbias != nullptr && blockIdx.y == 0) {      // (slab form: wgrad24_dbias_slab_kernel)
        __syncthreads();
        float *red = smem;                        // [6][CO]
        if (zrole) red[zt * CO + zc] = bsum;              // (a z2 wave summed both of its items, of the same channel)
        if (z2) red[(zt + 64 / CO) * CO + zc] = 0.f;
        __syncthreads();
        if (tid < CO) {
            float t = 0.f;
            for (int g = 0; g < G23_T; ++g) t += red[g * CO + tid];
            if (n0 + tid < p.Cout) atomicAdd(p.dbias + n0 + tid, t);
        }
    }
}

