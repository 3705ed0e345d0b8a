// The skinny-GEMM kernel, included twice by gemm_skinny.hip: GEMM32_ORDERED 0 = gemm32_kernel as it always was (GEMM32_KERNEL(name) = name,
// GEMM32_PART empty), GEMM32_ORDERED 1 = gemm32_kernel_ordered (ramnet_gemm_ordered / ramnet_gemm2_ordered: the accumulating forms without
// atomics; one more argument `part`): reduction slice ks of batch entry bi stores its block to part[(bi * ksplit + ks)][Mp][Np] (Mp, Np = the
// taller problem's M, and N, rounded up to 32) and gemm_join_kernel adds the slices to C in slice order.  A preprocessor switch and not a
// template parameter: the default instantiations keep their symbols and their register allocation.
template <bool TA>
__global__ void __launch_bounds__(256) GEMM32_KERNEL(gemm32_kernel)(const float *__restrict__ A, const float *__restrict__ B, float *__restrict__ C,
                                                     int M, int N, int K, int lda, int ldb, int ldc, int ksplit, int atomic,
                                                     int intra, long sa, long sb, long sc, const Gemm2nd two GEMM32_PART) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    // accumulating forms: the 4 waves of a workgroup own 4 neighbouring blocks (they share the A rows through the L1) and the
    // reduction is split over gridDim.z; plain product (intra): the 4 waves split the reduction of ONE block and join through LDS
    // in a fixed order — four times the waves in flight, still bit-reproducible
    const int nb = intra ? blockIdx.x : blockIdx.x * 4 + wave, mb = blockIdx.y;
    if (nb * 32 >= N) return;                                           // (uniform over the workgroup when intra)
    int bi = blockIdx.z / ksplit;                                        // batch entry (independent products)
    const int ks = intra ? wave : blockIdx.z - bi * ksplit;             // reduction slice
    if (bi >= two.nb1) {
        bi -= two.nb1;
        A = two.A, B = two.B, C = two.C, M = two.M, K = two.K, sa = two.sa, sb = two.sb, sc = two.sc;
    }
    if (mb * 32 >= M) return;                                           // (uniform over the workgroup: the other problem is taller)
    A += bi * sa, B += bi * sb, C += bi * sc;
    const int m = mb * 32 + l31, n = nb * 32 + l31;
    const int nsl = intra ? 4 : ksplit;
    const int kper = ((K + nsl - 1) / nsl + 31) / 32 * 32;
    const int kbeg = ks * kper, kend = min(K, kbeg + kper);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const bool mok = m < M, nok = n < N;
    // Operands through buffer loads: the per-lane byte offsets of a K step are computed once (rows / columns past M, N get an
    // out-of-range offset and read as 0), the step moves the descriptor, whose extent ends with this slice of the reduction —
    // so the loads of the main loop carry no mask, no branch and no per-lane address arithmetic.
    // one K step = 32 values: half 0 of the wave takes k0 .. k0+15, half 1 k0+16 .. k0+31 (MFMA i pairs k0+i with k0+16+i), so a
    // row of A is read as one full 128-byte line by its two lanes (4 x 16 bytes each) — no reliance on the L1 keeping it
    unsigned ao[TA ? 16 : 4], bo[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        bo[j] = nok ? (unsigned)(((16 * kh + j) * ldb + n) * 4) : WOOB;
        if (TA) ao[j] = mok ? (unsigned)(((16 * kh + j) * lda + m) * 4) : WOOB;
    }
    if (!TA) {
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) ao[qd] = mok ? (unsigned)((m * lda + 16 * kh + 4 * qd) * 4) : WOOB;
    }
    auto load = [&](int k0, float (&a)[16], float (&b)[16]) {
        // descriptors from row k0 to the end of the slice (the range check looks at the per-lane offset only): rows past kend read 0
        const auto rb = wino_rsrc(B + (size_t)k0 * ldb, (unsigned)min((size_t)(kend - k0) * ldb * 4, (size_t)WOOB));
        const auto ra = TA ? wino_rsrc(A + (size_t)k0 * lda, (unsigned)min((size_t)(kend - k0) * lda * 4, (size_t)WOOB)) : wino_rsrc(A + k0, WOOB);
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            if (!TA) {      // K % 4 == 0 and 16-byte aligned rows (host): a quad never straddles kend
                const unsigned o = k0 + 16 * kh + 4 * qd < kend ? ao[qd] : WOOB;
                const float4 v = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(ra, (int)o, 0, 0));
                a[4 * qd] = v.x, a[4 * qd + 1] = v.y, a[4 * qd + 2] = v.z, a[4 * qd + 3] = v.w;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (TA) a[4 * qd + j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, (int)ao[4 * qd + j], 0, 0));
                b[4 * qd + j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, (int)bo[4 * qd + j], 0, 0));
            }
        }
    };
    auto mm = [&](const float (&a)[16], const float (&b)[16]) {
#pragma unroll
        for (int j = 0; j < 16; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
    };
    float a0[16], b0[16], a1[16], b1[16];       // loads run one step (1024 MFMA cycles) ahead
    if (kbeg < kend) load(kbeg, a0, b0);
    for (int k0 = kbeg; k0 < kend; k0 += 64) {
        if (k0 + 32 < kend) load(k0 + 32, a1, b1);
        mm(a0, b0);
        if (k0 + 32 >= kend) break;
        if (k0 + 64 < kend) load(k0 + 64, a0, b0);
        mm(a1, b1);
    }
    if (intra) {
        __shared__ float red[3][16][64];
        if (wave > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) red[wave - 1][r][lane] = acc[r];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = ((acc[r] + red[0][r][lane]) + red[1][r][lane]) + red[2][r][lane];
    }
    if (!nok) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (row >= M) continue;
#if GEMM32_ORDERED  // slice ks of entry bi -> part[bi * ksplit + ks][Mp][Np]; a launch that does not split adds to C itself (one writer per element)
        if (ksplit > 1) part[((size_t)blockIdx.z * gridDim.y * 32 + row) * ((N + 31) / 32 * 32) + n] = acc[r];
        else C[(size_t)row * ldc + n] += acc[r];
#else
        if (atomic) atomicAdd(C + (size_t)row * ldc + n, acc[r]);
        else C[(size_t)row * ldc + n] = acc[r];
#endif
    }
}

