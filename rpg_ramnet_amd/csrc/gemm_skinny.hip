// Small fp32 GEMMs of the path — the border corrections of the folded upsample-conv ([border pixels x 5*Cin] x
// [5*Cin x 2*Cout], their backward-data and backward-weights forms) — on v_mfma_f32_32x32x2_f32, without LDS and without
// barriers: every WAVE owns one 32 x 32 block of C and reads its operands from global memory directly in MFMA lane layout
// (the matrices are a few MB and were written by the previous kernel: L2 / Infinity-Cache hits).
//
//   NN:  C[M][N]  = A[M][K] * B[K][N]          lane (row m = lane & 31, half = lane >> 5) loads A[m][k0 + 16*half .. +15] as four
//                                              16-byte loads (the MFMA's K index 0 / 1 = the two halves: a row's 128-byte line
//                                              is consumed whole), B[k][n = lane & 31] as 128-byte-coalesced 4-byte loads
//   TN:  C[K][N] += A[R][K]^T * B[R][N]        (weight gradient: reduction over the R pixel rows, split over gridDim.z and
//                                              joined by atomics) — both operands coalesced along their channel index
// Loads run one K step (32 values, 1024 MFMA cycles) ahead of the MFMAs.  The accumulating forms (backward pass) split the
// reduction over workgroups until ~8 waves per SIMD are in flight (partial sums meet by atomics): the operand loads are
// latency-bound, occupancy is what hides them.  The plain product (forward pass) splits the reduction over the four waves of the
// block's workgroup, which join through LDS in a fixed order: bit-reproducible.
#include <stdlib.h>
#include "common.hpp"

namespace ramnet {

// A launch may carry TWO problems of the same N, leading dimensions and mode (the row and the column border of a decoder layer differ in
// M — forward / backward-data — or in the reduction length K — weight gradient): batch entries [0, nb1) belong to (A, B, C, M), the rest to the second set.
struct Gemm2nd {
    const float *A, *B;
    float *C;
    int M, K, nb1;
    long sa, sb, sc;
};

#define GEMM32_ORDERED 0
#define GEMM32_KERNEL(name) name
#define GEMM32_PART
#include "gemm_skinny_kernel.hpp"
#undef GEMM32_ORDERED
#undef GEMM32_KERNEL
#undef GEMM32_PART
#define GEMM32_ORDERED 1
#define GEMM32_KERNEL(name) name##_ordered
#define GEMM32_PART , float *__restrict__ part
#include "gemm_skinny_kernel.hpp"
#undef GEMM32_ORDERED
#undef GEMM32_KERNEL
#undef GEMM32_PART

// C[bi] += part[bi][0] + part[bi][1] + ... + part[bi][ksplit - 1], added one after the other in that order; grid (blocks over Mp * Np, batch entries)
__global__ void __launch_bounds__(256) gemm_join_kernel(const float *__restrict__ part, float *__restrict__ C, int M, int N, int ldc, long sc,
                                                        int ksplit, int Mp, int Np, const Gemm2nd two) {
    int bi = blockIdx.y;
    const float *pp = part + (size_t)bi * ksplit * Mp * Np;
    if (bi >= two.nb1) bi -= two.nb1, C = two.C, M = two.M, sc = two.sc;
    const int idx = blockIdx.x * 256 + threadIdx.x, row = idx / Np, n = idx - row * Np;
    if (row >= M || n >= N) return;
    float *c = C + bi * sc + (size_t)row * ldc + n;
    float v = *c;
    for (int ks = 0; ks < ksplit; ++ks) v += pp[((size_t)ks * Mp + row) * Np + n];
    *c = v;
}

}  // namespace ramnet

using namespace ramnet;

// reduction slices of an accumulating launch (backward pass): the operand loads are latency-bound and occupancy is what hides them, so the
// reduction is split over gridDim.z until a few thousand waves are in flight
static int gemm_ksplit(int nb, int Mmax, int N, int Kmax) {
    const int blocks = nb * cdiv(Mmax, 32) * cdiv(N, 32);
    int ksplit = 1;             // (splitting less — 512 ... 2048 blocks — measured the same training step: 198.2 - 199.2 samples/s)
    while (blocks * ksplit < 8192 && Kmax / (ksplit * 2) >= 128) ksplit *= 2;
    return ksplit;
}

static int launch_gemm(const float *A, const float *B, float *C, int M, int N, int K, int lda, int ldb, int ldc, int trans_a, int accumulate,
                       int batch, long stride_a, long stride_b, long stride_c, const float *A2, const float *B2, float *C2, int M2, int K2, int batch2,
                       long stride_a2, long stride_b2, long stride_c2, void *stream, bool ordered = false, float *partial = nullptr) {
    const int Mmax = M > M2 ? M : M2, Kmax = K > K2 ? K : K2;
    RAMNET_CHECK_ARG(A && B && C && M > 0 && N > 0 && K > 0 && ldb >= N && ldc >= N && batch >= 1 && batch2 >= 0);
    if (batch2 > 0) RAMNET_CHECK_ARG(A2 && B2 && C2 && M2 > 0 && K2 > 0 && ((uintptr_t)A2 & 15) == 0 && stride_a2 % 4 == 0 && (trans_a || K2 % 4 == 0));
    if (trans_a) RAMNET_CHECK_ARG(lda >= Mmax);
    else RAMNET_CHECK_ARG(lda >= Kmax && K % 4 == 0 && lda % 4 == 0 && ((uintptr_t)A & 15) == 0 && stride_a % 4 == 0);
    // operands are addressed through 32-bit per-lane byte offsets and buffer extents clamped to WOOB (like the conv launchers)
    RAMNET_CHECK_ARG((unsigned long long)(trans_a ? Kmax : Mmax) * lda * 4ull < WOOB && (unsigned long long)Kmax * ldb * 4ull < WOOB &&
                     (unsigned long long)Mmax * ldc * 4ull < WOOB);
    // accumulate (backward pass): the operand loads are latency-bound and occupancy is what hides them, so the reduction is split
    // over gridDim.z until a few thousand waves are in flight; partial sums meet by atomics in C.  A plain product (forward pass)
    // splits it over the waves of one workgroup per block instead (fixed-order LDS join): bit-reproducible, as every forward kernel.
    const int nb = batch + batch2;
    const int ksplit = accumulate ? gemm_ksplit(nb, Mmax, N, Kmax) : 1;
    const int intra = !accumulate && Kmax >= 128;
    const dim3 grid(intra ? cdiv(N, 32) : cdiv(cdiv(N, 32), 4), cdiv(Mmax, 32), ksplit * nb);
    const Gemm2nd two = {A2, B2, C2, M2, K2, batch, stride_a2, stride_b2, stride_c2};
    if (ordered) {
        RAMNET_CHECK_ARG(accumulate && (ksplit == 1 || partial != nullptr));
        if (trans_a)
            hipLaunchKernelGGL(gemm32_kernel_ordered<true>, grid, dim3(256), 0, (hipStream_t)stream, A, B, C, M, N, K, lda, ldb, ldc, ksplit, 0, 0,
                               stride_a, stride_b, stride_c, two, partial);
        else
            hipLaunchKernelGGL(gemm32_kernel_ordered<false>, grid, dim3(256), 0, (hipStream_t)stream, A, B, C, M, N, K, lda, ldb, ldc, ksplit, 0, 0,
                               stride_a, stride_b, stride_c, two, partial);
        if (ksplit > 1) {
            const int Mp = roundup(Mmax, 32), Np = roundup(N, 32);
            hipLaunchKernelGGL(gemm_join_kernel, dim3(cdiv(Mp * Np, 256), nb), dim3(256), 0, (hipStream_t)stream, partial, C, M, N, ldc, stride_c,
                               ksplit, Mp, Np, two);
        }
        RAMNET_LAUNCH_CHECK();
        return 0;
    }
    if (trans_a)
        hipLaunchKernelGGL(gemm32_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, A, B, C, M, N, K, lda, ldb, ldc, ksplit, accumulate,
                           intra, stride_a, stride_b, stride_c, two);
    else
        hipLaunchKernelGGL(gemm32_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, A, B, C, M, N, K, lda, ldb, ldc, ksplit, accumulate,
                           intra, stride_a, stride_b, stride_c, two);
    RAMNET_LAUNCH_CHECK();
    return 0;
}

extern "C" int ramnet_gemm(const float *A, const float *B, float *C, int M, int N, int K, int lda, int ldb, int ldc, int trans_a,
                           int accumulate, int batch, long stride_a, long stride_b, long stride_c, void *stream) {
    return launch_gemm(A, B, C, M, N, K, lda, ldb, ldc, trans_a, accumulate, batch, stride_a, stride_b, stride_c, nullptr, nullptr, nullptr, 0, 0, 0, 0,
                       0, 0, stream);
}

extern "C" int ramnet_gemm2(const float *A, const float *B, float *C, int M, long stride_a, long stride_b, long stride_c, int batch, const float *A2,
                            const float *B2, float *C2, int M2, long stride_a2, long stride_b2, long stride_c2, int batch2, int N, int K, int K2, int lda,
                            int ldb, int ldc, int trans_a, int accumulate, void *stream) {
    RAMNET_CHECK_ARG(batch2 >= 1);
    return launch_gemm(A, B, C, M, N, K, lda, ldb, ldc, trans_a, accumulate, batch, stride_a, stride_b, stride_c, A2, B2, C2, M2, K2, batch2, stride_a2,
                       stride_b2, stride_c2, stream);
}

// ---- the accumulating forms with a fixed order of the sums (no atomics): C += the products of the reduction slices, added in slice order ----
extern "C" size_t ramnet_gemm_partial_floats(int M, int N, int K, int batch, int M2, int K2, int batch2) {
    if (M <= 0 || N <= 0 || K <= 0 || batch < 1 || batch2 < 0 || (batch2 > 0 && (M2 <= 0 || K2 <= 0))) return 0;
    const int Mmax = batch2 > 0 && M2 > M ? M2 : M, Kmax = batch2 > 0 && K2 > K ? K2 : K;
    const int ksplit = gemm_ksplit(batch + batch2, Mmax, N, Kmax);
    return ksplit > 1 ? (size_t)(batch + batch2) * ksplit * roundup(Mmax, 32) * roundup(N, 32) : 0;
}

extern "C" int ramnet_gemm_ordered(const float *A, const float *B, float *C, int M, int N, int K, int lda, int ldb, int ldc, int trans_a, int batch,
                                   long stride_a, long stride_b, long stride_c, float *partial, void *stream) {
    return launch_gemm(A, B, C, M, N, K, lda, ldb, ldc, trans_a, 1, batch, stride_a, stride_b, stride_c, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0,
                       stream, true, partial);
}

extern "C" int ramnet_gemm2_ordered(const float *A, const float *B, float *C, int M, long stride_a, long stride_b, long stride_c, int batch,
                                    const float *A2, const float *B2, float *C2, int M2, long stride_a2, long stride_b2, long stride_c2, int batch2,
                                    int N, int K, int K2, int lda, int ldb, int ldc, int trans_a, float *partial, void *stream) {
    RAMNET_CHECK_ARG(batch2 >= 1);
    return launch_gemm(A, B, C, M, N, K, lda, ldb, ldc, trans_a, 1, batch, stride_a, stride_b, stride_c, A2, B2, C2, M2, K2, batch2, stride_a2,
                       stride_b2, stride_c2, stream, true, partial);
}
