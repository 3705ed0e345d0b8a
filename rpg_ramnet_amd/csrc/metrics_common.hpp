// What the reductions of metrics.hip and render.hip share: the streaming load types, the wave sum, the ticket / last-arrival join and the
// ONE conversion of normalised log depth to metric depth.
#pragma once
#include "common.hpp"

namespace ramnet {

typedef float bm_f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef const float __attribute__((address_space(1))) *bm_src_t;

constexpr int BM_T = 256;                  // threads of a workgroup

__device__ __forceinline__ double bm_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

__device__ __forceinline__ unsigned bm_ld(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double bm_ld(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Takes the pair's ticket after the workgroup's stores; true in every thread of the last arrival of the pair.
__device__ __forceinline__ bool bm_ticket(size_t g, int P, unsigned *tickets, int *flag) {
    // Release ONCE per workgroup (a __threadfence() in each of the 6144 waves of a G = 48 launch writes the L2 back 6144 times): every wave
    // waits until its own stores have reached the L2 (the barrier alone does not), then thread 0 fences at device scope and takes the ticket.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        *flag = atomicAdd(tickets + g, 1u) == (unsigned)P - 1u;
    }
    __syncthreads();
    const bool last = *flag != 0;
    if (last) __threadfence();
    return last;
}

// Normalised log depth -> metric depth (evaluation.py:76-85), the ONE conversion of ramnet_metric_depth and of the table kernels.
// lo = expf(-reg) * clip.  The clamp keeps a NaN (both comparisons are false); on numbers it is fminf(fmaxf(d, lo), clip).
__device__ __forceinline__ float et_metric_depth(float y, float reg, float clip, float lo, bool clamp) {
    float d = expf(reg * (y - 1.0f)) * clip;
    if (clamp) d = d < lo ? lo : (d > clip ? clip : d);
    return d;
}

}  // namespace ramnet
