// Training metrics (model/metric.py:8-54) of G (prediction, target) pairs without the host: the six means, the per-sample mse and the
// EXACT median of d = |t - p| of every pair, three launches for all pairs together.
//
// grid = (Ws, N, G): workgroup (w, s, g) reads a contiguous quarter-or-so of sample s of pair g, 16 bytes per lane and map (the loads are
// 4-byte aligned global loads: a sample need not start on a 16-byte boundary), so a pass reads 8 B per element and writes nothing but its
// partials.  P = N * Ws workgroups work on one pair.
//
// pass 1  sums + histogram of bits 30..20 of d   (d >= +0: the uint32 pattern of a non-NaN d orders like its value, bit 31 is 0)
// pass 2  histogram of bits 19..10 of the d whose bits 30..20 equal the bin that holds the wanted rank
// pass 3  histogram of bits  9..0  of the d whose bits 30..10 equal the 21-bit prefix     -> the element of that rank, bit for bit
// An even count needs the elements of ranks n/2 - 1 and n/2: both are carried through the passes, with a histogram each from the pass after
// the one where they part (np.median: (a + b) * 0.5 rounded in fp32).
//
// Joins.  Every workgroup counts in an LDS histogram (ds_add_u32) and STORES it whole to its own slab, stores its eight double partial sums
// to its own row, releases both with one device-scope fence and takes a ticket of its pair; the last arrival of a pair adds the P rows
// and the P slabs in index order (integer sums and a fixed order of the double sums: the same bits on every launch), picks the bin
// that holds each rank and leaves the (prefix, rank inside it) of the pair in the workspace for the next pass.  No value crosses to
// the host between the passes.
//
// Workspace: [64 Ki tickets][G states][G x P partial rows][G x P x 2 slabs].  Slabs, rows and states are written in full before they are
// read in every call; the tickets are set back to 0 by the last arrival.  So ONE zero-fill of the first RAMNET_BATCH_METRICS_TICKET_BYTES
// at allocation is all a caller owes, and calls of any shape that fit the allocation can follow each other without a memset
// (one call at a time per workspace: calls on the same workspace are ordered on one stream).
//
// Element arithmetic is numpy's on float32 arrays: fabsf(t - p), d / (t + 1e-6f), d * d / (t * t + 1e-6f) with IEEE division and no
// contraction (this file is built with -ffp-contract=off; the divisions are __fdiv_rn), accumulated in double.
#include "common.hpp"
#include "metrics_common.hpp"

namespace ramnet {


constexpr int BM_BINS = 2048;              // bins of pass 1 (11 bits); passes 2 and 3 use the first 1024 of a slab
constexpr int BM_ROW = 8;                  // doubles of a partial row: n, n_target, sum d/(t+eps), sum d^2/(t^2+eps), sum d^2, sum d, sum (p-t)^2 | t valid, (unused)
constexpr int BM_STATE = 8;                // uint32 of a pair's state: prefix0, rank0, prefix1, rank1, n
constexpr int BM_MAX_PER_PAIR = 32;        // workgroups per pair when N allows it (N > 32: one per sample)
constexpr int BM_STAGE = 64;                // partial rows the last arrival stages through LDS at a time
constexpr unsigned BM_SPAN = 8192;         // elements a workgroup should at least have

struct bm_plan_t {
    int Ws, P;
    size_t off_state, off_part, off_slab, total;
};

static bm_plan_t bm_plan(int G, int N, size_t npix) {
    bm_plan_t p;
    size_t ws = (npix + BM_SPAN - 1) / BM_SPAN;
    const size_t cap = N >= BM_MAX_PER_PAIR ? 1 : BM_MAX_PER_PAIR / N;
    if (ws > cap) ws = cap;
    if (ws < 1) ws = 1;
    p.Ws = (int)ws;
    p.P = N * p.Ws;
    p.off_state = RAMNET_BATCH_METRICS_TICKET_BYTES;
    p.off_part = p.off_state + (((size_t)G * BM_STATE * sizeof(unsigned) + 255) & ~(size_t)255);
    p.off_slab = p.off_part + (((size_t)G * p.P * BM_ROW * sizeof(double) + 255) & ~(size_t)255);
    p.total = p.off_slab + (size_t)G * p.P * 2 * BM_BINS * sizeof(unsigned);
    return p;
}

// The part of sample s that workgroup w of Ws reads: [lo, hi) in elements of the sample, lo a multiple of 4.
__device__ __forceinline__ void bm_range(unsigned npix, int Ws, int w, unsigned &lo, unsigned &hi) {
    const unsigned chunk = ((npix + Ws - 1) / Ws + 3u) & ~3u;
    const unsigned long long a = (unsigned long long)w * chunk;
    lo = a < npix ? (unsigned)a : npix;
    hi = npix - lo < chunk ? npix : lo + chunk;
}

// f(p, t) over the elements [lo, hi) of one sample: 16 bytes per lane and map, then the tail of fewer than 4 elements.
template <class F>
__device__ __forceinline__ void bm_sweep(bm_src_t p, bm_src_t t, unsigned lo, unsigned hi, F f) {
    typedef const bm_f4u __attribute__((address_space(1))) *v4_t;
    const unsigned nv = (hi - lo) >> 2;
    unsigned i = threadIdx.x;
    for (; i + 3 * BM_T < nv; i += 4 * BM_T) {                   // eight loads in flight per lane
        bm_f4u a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = *(v4_t)(p + lo + 4 * (size_t)(i + j * BM_T)), b[j] = *(v4_t)(t + lo + 4 * (size_t)(i + j * BM_T));
#pragma unroll
        for (int j = 0; j < 4; ++j) f(a[j].x, b[j].x), f(a[j].y, b[j].y), f(a[j].z, b[j].z), f(a[j].w, b[j].w);
    }
    for (; i < nv; i += BM_T) {
        const bm_f4u a = *(v4_t)(p + lo + 4 * (size_t)i), b = *(v4_t)(t + lo + 4 * (size_t)i);
        f(a.x, b.x), f(a.y, b.y), f(a.z, b.z), f(a.w, b.w);
    }
    for (unsigned k = lo + 4 * nv + threadIdx.x; k < hi; k += BM_T) f(p[k], t[k]);
}

// Adds the P slabs `h` of pair g into the LDS histogram (index order), all threads.  The loads of four slabs are in flight together: one
// after the other, the P x NBINS / BM_T coherent loads of a thread were most of a launch (profiles/epoch_metrics_notes.md).
// WGS / HS: words between the slabs of two workgroups / of two histograms of one workgroup (the evaluation table below packs four).
template <int NBINS, int WGS = 2 * BM_BINS, int HS = BM_BINS>
__device__ __forceinline__ void bm_join_slabs(const unsigned *slab, size_t g, int P, int h, unsigned *lds) {
    constexpr int PER = NBINS / BM_T;
    unsigned v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) v[j] = 0;
    for (int k0 = 0; k0 < P; k0 += 4) {
        unsigned x[4][PER];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int j = 0; j < PER; ++j)
                x[kk][j] = k0 + kk < P ? bm_ld(slab + ((size_t)g * P + k0 + kk) * WGS + (size_t)h * HS + threadIdx.x + j * BM_T) : 0u;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int j = 0; j < PER; ++j) v[j] += x[kk][j];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) lds[threadIdx.x + j * BM_T] = v[j];
    __syncthreads();
}

// The bin of the joined LDS histogram that holds the element of rank `rank` (0-based) and the rank inside that bin -> res[0], res[1]
// (LDS; {0, 0} when the histogram holds no such rank).  scan: a word of LDS per wave.  All threads; ends with a barrier.
__device__ __forceinline__ void bm_select(const unsigned *lds, int nbins, unsigned rank, unsigned *scan, unsigned *res) {
    const int per = nbins / BM_T;
    unsigned tot = 0;
    for (int j = 0; j < per; ++j) tot += lds[threadIdx.x * per + j];
    // exclusive scan of the 256 totals: inside each wave by shuffles, the four wave totals through LDS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) scan[wave] = inc;
    if (threadIdx.x == 0) res[0] = 0, res[1] = 0;
    __syncthreads();
    unsigned before = inc - tot;
    for (int w = 0; w < wave; ++w) before += scan[w];
    if (rank >= before && rank - before < tot) {                  // exactly one thread
        unsigned r = rank - before;
        for (int j = 0; j < per; ++j) {
            const unsigned c = lds[threadIdx.x * per + j];
            if (r < c) {
                res[0] = threadIdx.x * per + j, res[1] = r;
                break;
            }
            r -= c;
        }
    }
    __syncthreads();
}

// Stores the workgroup's histogram(s) to its slab(s), takes the pair's ticket; true in every thread of the last arrival of the pair.
__device__ __forceinline__ bool bm_arrive(unsigned (*hist)[BM_BINS], int nh, int nbins, unsigned *slab, size_t g, int P, int wg, unsigned *tickets,
                                          int *flag) {
    for (int h = 0; h < nh; ++h)
        for (int b = threadIdx.x; b < nbins; b += BM_T) slab[(((size_t)g * P + wg) * 2 + h) * BM_BINS + b] = hist[h][b];
    return bm_ticket(g, P, tickets, flag);
}

__global__ void __launch_bounds__(BM_T) bm_sums_kernel(const float *const *__restrict__ preds, const float *const *__restrict__ targets, int N,
                                                       unsigned npix, int Ws, unsigned *tickets, unsigned *state, double *part, unsigned *slab,
                                                       double *__restrict__ out) {
    __shared__ unsigned hist[2][BM_BINS];
    __shared__ double red[BM_ROW][BM_T / 64], stage[BM_STAGE * BM_ROW];
    __shared__ unsigned scan[BM_T / 64], res[2];
    __shared__ int flag;
    const int w = blockIdx.x, s = blockIdx.y, P = N * Ws, wg = s * Ws + w;
    const size_t g = blockIdx.z;
    for (int b = threadIdx.x; b < BM_BINS; b += BM_T) hist[0][b] = 0;
    __syncthreads();
    unsigned lo, hi;
    bm_range(npix, Ws, w, lo, hi);
    const bm_src_t p = (bm_src_t)preds[g] + (size_t)s * npix, t = (bm_src_t)targets[g] + (size_t)s * npix;
    double acc[BM_ROW] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    unsigned n = 0, nt = 0;
    bm_sweep(p, t, lo, hi, [&](float pv, float tv) {
        const float d = fabsf(tv - pv);
        if (tv == tv) {
            const float e = pv - tv;
            ++nt;
            acc[6] += (double)(e * e);                            // NaN for a non-finite prediction, as sklearn's mean would be
        }
        if (d == d) {
            const float d2 = d * d;
            ++n;
            acc[2] += (double)__fdiv_rn(d, tv + 1e-6f);
            acc[3] += (double)__fdiv_rn(d2, tv * tv + 1e-6f);
            acc[4] += (double)d2;
            acc[5] += (double)d;
            atomicAdd(&hist[0][__float_as_uint(d) >> 20], 1u);
        }
    });
    acc[0] = (double)n, acc[1] = (double)nt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < BM_ROW; ++k) {
        const double v = bm_wave_sum(acc[k]);
        if (lane == 0) red[k][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < BM_ROW) {
        double v = 0.0;
        for (int i = 0; i < BM_T / 64; ++i) v += red[threadIdx.x][i];
        part[((size_t)g * P + wg) * BM_ROW + threadIdx.x] = v;
    }
    if (!bm_arrive(hist, 1, BM_BINS, slab, g, P, wg, tickets, &flag)) return;

    // last arrival of the pair: the rows come through LDS 64 at a time (all loads of a chunk in flight), one thread per column adds them in
    // index order; column 6 becomes the per-sample mse (thread 6 closes a sample after its Ws rows)
    const double *rows = part + (size_t)g * P * BM_ROW;
    double v = 0.0, sq = 0.0, c = 0.0;
    for (int r0 = 0; r0 < P; r0 += BM_STAGE) {
        const int nr = P - r0 < BM_STAGE ? P - r0 : BM_STAGE;
        for (int i = threadIdx.x; i < nr * BM_ROW; i += BM_T) stage[i] = bm_ld(rows + (size_t)r0 * BM_ROW + i);
        __syncthreads();
        if (threadIdx.x < 6) {
            for (int r = 0; r < nr; ++r) v += stage[r * BM_ROW + threadIdx.x];
        } else if (threadIdx.x == 6) {
            for (int r = 0; r < nr; ++r) {
                sq += stage[r * BM_ROW + 6], c += stage[r * BM_ROW + 1];
                if ((r0 + r + 1) % Ws == 0) v += sq / c, sq = 0.0, c = 0.0;          // 0 / 0: a sample without a valid target makes the pair's mse NaN
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) red[threadIdx.x][0] = v;
    else if (threadIdx.x == 6) red[6][0] = v / (double)N;
    bm_join_slabs<BM_BINS>(slab, g, P, 0, hist[0]);               // (barrier: red is complete as well)
    const double cnt = red[0][0];
    const unsigned total = (unsigned)cnt;
    if (threadIdx.x == 0) {
        double *o = out + g * 10;
        const double md = red[5][0] / cnt, md2 = red[4][0] / cnt;
        o[0] = cnt, o[1] = red[1][0], o[2] = red[6][0];
        o[3] = red[2][0] / cnt, o[4] = red[3][0] / cnt, o[5] = sqrt(md2), o[6] = md2 - md * md, o[7] = md;
        o[9] = 0.0;
    }
    unsigned *st = state + g * BM_STATE;
    const unsigned r0 = total ? (total - 1) / 2 : 0, r1 = total / 2;
    bm_select(hist[0], BM_BINS, r0, scan, res);
    if (threadIdx.x == 0) st[0] = res[0], st[1] = res[1], st[4] = total;
    bm_select(hist[0], BM_BINS, r1, scan, res);
    if (threadIdx.x == 0) {
        st[2] = res[0], st[3] = res[1];
        atomicExch(tickets + g, 0u);                              // ready for the next pass
    }
}

// SHIFT = 10: bits 19..10 of the d whose bits 30..20 equal the pair's prefix; SHIFT = 0: bits 9..0 under the 21-bit prefix, and the median.
template <int SHIFT>
__global__ void __launch_bounds__(BM_T) bm_select_kernel(const float *const *__restrict__ preds, const float *const *__restrict__ targets, int N,
                                                         unsigned npix, int Ws, unsigned *tickets, unsigned *state, unsigned *slab,
                                                         double *__restrict__ out) {
    constexpr int NB = 1024;
    __shared__ unsigned hist[2][BM_BINS];
    __shared__ unsigned scan[BM_T / 64], res[2];
    __shared__ int flag;
    const int w = blockIdx.x, s = blockIdx.y, P = N * Ws, wg = s * Ws + w;
    const size_t g = blockIdx.z;
    unsigned *st = state + g * BM_STATE;
    const unsigned pre0 = st[0], rank0 = st[1], pre1 = st[2], rank1 = st[3], total = st[4];
    const bool two = pre0 != pre1;
    for (int b = threadIdx.x; b < NB; b += BM_T) hist[0][b] = 0, hist[1][b] = 0;
    __syncthreads();
    unsigned lo, hi;
    bm_range(npix, Ws, w, lo, hi);
    const bm_src_t p = (bm_src_t)preds[g] + (size_t)s * npix, t = (bm_src_t)targets[g] + (size_t)s * npix;
    bm_sweep(p, t, lo, hi, [&](float pv, float tv) {
        const float d = fabsf(tv - pv);
        if (d == d) {
            const unsigned key = __float_as_uint(d), top = key >> (SHIFT + 10), bin = (key >> SHIFT) & (NB - 1);
            if (top == pre0) atomicAdd(&hist[0][bin], 1u);
            else if (top == pre1) atomicAdd(&hist[1][bin], 1u);
        }
    });
    __syncthreads();
    if (!bm_arrive(hist, two ? 2 : 1, NB, slab, g, P, wg, tickets, &flag)) return;

    bm_join_slabs<NB>(slab, g, P, 0, hist[0]);
    bm_select(hist[0], NB, rank0, scan, res);
    const unsigned a = (pre0 << 10) | res[0], ra = res[1];
    __syncthreads();
    if (two) bm_join_slabs<NB>(slab, g, P, 1, hist[0]);
    bm_select(hist[0], NB, rank1, scan, res);
    const unsigned b = (pre1 << 10) | res[0], rb = res[1];
    if (threadIdx.x == 0) {
        if (SHIFT) {
            st[0] = a, st[1] = ra, st[2] = b, st[3] = rb;
        } else {
            const float fa = __uint_as_float(a), fb = __uint_as_float(b);
            const float med = (total & 1u) ? fa : (fa + fb) * 0.5f;
            out[g * 10 + 8] = total ? (double)med : (double)__uint_as_float(0x7fc00000u);
        }
        atomicExch(tickets + g, 0u);
    }
}

}  // namespace ramnet

using namespace ramnet;

extern "C" size_t ramnet_batch_metrics_workspace(int G, int N, size_t npix) {
    if (G <= 0 || N <= 0 || npix == 0 || G > 65535 || N > 65535 || (size_t)N * npix >= ((size_t)1 << 31)) return 0;
    return bm_plan(G, N, npix).total;
}

extern "C" int ramnet_batch_metrics(const float *const *pred, const float *const *target, int G, int N, size_t npix, void *workspace, double *out,
                                    void *stream) {
    RAMNET_CHECK_ARG(G >= 0 && G <= 65535 && N > 0 && N <= 65535 && npix > 0);
    RAMNET_CHECK_ARG((size_t)N * npix < ((size_t)1 << 31));
    if (G == 0) return 0;
    RAMNET_CHECK_ARG(pred && target && workspace && out);
    RAMNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0);
    const bm_plan_t pl = bm_plan(G, N, npix);
    char *ws = static_cast<char *>(workspace);
    unsigned *tickets = reinterpret_cast<unsigned *>(ws), *state = reinterpret_cast<unsigned *>(ws + pl.off_state);
    double *part = reinterpret_cast<double *>(ws + pl.off_part);
    unsigned *slab = reinterpret_cast<unsigned *>(ws + pl.off_slab);
    const dim3 grid(pl.Ws, N, G);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bm_sums_kernel, grid, dim3(BM_T), 0, st, pred, target, N, (unsigned)npix, pl.Ws, tickets, state, part, slab, out);
    hipLaunchKernelGGL(bm_select_kernel<10>, grid, dim3(BM_T), 0, st, pred, target, N, (unsigned)npix, pl.Ws, tickets, state, slab, out);
    hipLaunchKernelGGL(bm_select_kernel<0>, grid, dim3(BM_T), 0, st, pred, target, N, (unsigned)npix, pl.Ws, tickets, state, slab, out);
    RAMNET_LAUNCH_CHECK();
    note_kernel("bm_sums_kernel + bm_select_kernel<10> + bm_select_kernel<0>");
    return 0;
}

// ================================================================================================ depth evaluation table
namespace ramnet {

// The table of evaluation.py:295-397 for G (prediction, target) pairs of normalised log depth, every variant of it together: all pixels and
// each depth cut-off, and the same again under an event mask.  grid = (Ws, V, G): workgroup (w, v, g) reads its part of map g for variant v;
// every variant re-reads the maps (they stay in L2: 8 B per pixel and pair), which keeps one histogram set per workgroup and the joins of
// the training metrics above: partial rows and slabs in index order, tickets that reset themselves, the same bits on every call.
//
// pass 1  the sums of depth_metrics_kernel (loss_voxel.hip: same expressions, epsilons and types) + histograms of bits 30..20 of the metric
//         target and of the metric prediction (positive floats: the pattern orders like the value)
// pass 2  bits 19..10 under the prefixes of the wanted ranks (two per stream for an even count), pass 3  bits 9..0 -> both medians
// A variant whose mask holds a NaN target, or nothing, has NaN medians (np.median over such a mask is NaN): passes 2 and 3 skip it.
//
// Workspace: [64 Ki tickets][G V states][G V x P partial rows][G V x P slabs of 4096 words: 2 x 2048 bins in pass 1, 4 x 1024 after it].
//
// RESCALED rows (evaluation.py:99-154, rescale_by_the_median before the metrics are formed; template argument RS): the sums are taken on
//   t' = T_t(t) [+ md], p' = T_p(p) [+ md],  T_x(v) = (v - med_x) / std_x + |(min_x - med_x) / std_x|,  md = |T_t-median - T_p-median|
// added to the side with the smaller median, all in double on the float32 depths.  The constants of a (pair, variant) have to exist before the
// first term: pass 1 adds the sums (-> means) and the minima of t and p, pass 2 the sums of squared deviations from those means (np.std's
// two passes), pass 3 leaves the two middle values of each map in the state, and a FOURTH pass, et_rescale_kernel, forms the sums and writes
// columns 2..12.  T_x is monotone: minimum and median of a transformed map are the transforms of the minimum and of the middle values.
// A variant with a NaN target, or empty, takes no part in passes 2..4 (pass 1 writes its row: NaN sums, zero threshold counts); zero spread
// is not special-cased: 0 / 0 makes the sums NaN and the comparisons false.  Partial rows are 16 doubles here and the constants live behind
// the slabs: [...][G V x P slabs][G V x 8 doubles].
constexpr int ET_ROW = 12;                 // doubles of a partial row: n_mask, n, six sums, three threshold counts, (unused)
constexpr int ET_ROWX = 16;                // ... of a rescaled call: the same, then sum t, sum p, min t, min p, (unused)
constexpr int ET_CST = 8;                  // doubles per (pair, variant) of a rescaled call: mean t, mean p, min t, min p, std t, std p, (unused)
constexpr int ET_COLS = 11;
constexpr int ET_OUT = 16;                 // doubles of an output row
constexpr int ET_STATE = 12;               // uint32 per (pair, variant): target prefix0, rank0, prefix1, rank1; the same of the prediction; n; medians wanted
constexpr int ET_MAX_PER_MAP = 32;         // workgroups per (pair, variant) at most
constexpr unsigned ET_SPAN = 16384;        // pixels a workgroup should at least have (its slab is 16 KB: an eighth of what it reads)
constexpr int ET_SLAB = 2 * BM_BINS;       // words of a workgroup's slab
constexpr int ET_MAXCUT = 8;

typedef const unsigned char __attribute__((address_space(1))) *et_msk_t;
typedef unsigned char et_b4 __attribute__((ext_vector_type(4), aligned(1)));

struct et_args_t {
    float clip, reg, cut[ET_MAXCUT];
    int ncut, V, Ws;
    unsigned npix;
    int tmetric;                           // the target tables hold float32 metric depth already
};

struct et_plan_t {
    int V, Ws;
    size_t off_state, off_part, off_slab, off_cst, total;
};

static et_plan_t et_plan(int G, size_t npix, int ncut, int has_mask, bool rescale = false) {
    et_plan_t p;
    size_t ws = (npix + ET_SPAN - 1) / ET_SPAN;
    if (ws > ET_MAX_PER_MAP) ws = ET_MAX_PER_MAP;
    p.Ws = (int)ws;
    p.V = (1 + ncut) * (has_mask ? 2 : 1);
    const size_t cells = (size_t)G * p.V;
    p.off_state = RAMNET_EVAL_TABLE_TICKET_BYTES;
    p.off_part = p.off_state + ((cells * ET_STATE * sizeof(unsigned) + 255) & ~(size_t)255);
    p.off_slab = p.off_part + ((cells * p.Ws * (rescale ? ET_ROWX : ET_ROW) * sizeof(double) + 255) & ~(size_t)255);
    p.off_cst = p.off_slab + cells * p.Ws * ET_SLAB * sizeof(unsigned);
    p.total = p.off_cst + (rescale ? cells * ET_CST * sizeof(double) : 0);
    return p;
}

static bool et_sizes_ok(int G, size_t npix, int ncut, int has_mask) {
    if (G < 1 || G > 65535 || npix == 0 || npix >= ((size_t)1 << 32) || ncut < 0 || ncut > ET_MAXCUT) return false;
    return (size_t)G * (1 + ncut) * (has_mask ? 2 : 1) <= RAMNET_EVAL_TABLE_TICKET_BYTES / sizeof(unsigned);
}

// bm_range for a map of up to 2^32 - 1 pixels
__device__ __forceinline__ void et_range(unsigned npix, int Ws, int w, unsigned &lo, unsigned &hi) {
    const unsigned chunk = (unsigned)((((unsigned long long)npix + Ws - 1) / Ws + 3u) & ~3ull);
    const unsigned long long a = (unsigned long long)w * chunk;
    lo = a < npix ? (unsigned)a : npix;
    hi = npix - lo < chunk ? npix : lo + chunk;
}

// f(p, t, inside mask) over the pixels [lo, hi) of one map: 16 bytes per lane and map (and 4 of the mask), then the tail.  m == NULL: all inside.
template <class F>
__device__ __forceinline__ void et_sweep(bm_src_t p, bm_src_t t, et_msk_t m, unsigned lo, unsigned hi, F f) {
    typedef const bm_f4u __attribute__((address_space(1))) *v4_t;
    typedef const et_b4 __attribute__((address_space(1))) *b4_t;
    const unsigned nv = (hi - lo) >> 2;
    unsigned i = threadIdx.x;
    for (; i + BM_T < nv; i += 2 * BM_T) {                        // four (six) loads in flight per lane
        bm_f4u a[2], b[2];
        et_b4 c[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const size_t o = lo + 4 * (size_t)(i + j * BM_T);
            a[j] = *(v4_t)(p + o), b[j] = *(v4_t)(t + o);
            c[j] = m ? *(b4_t)(m + o) : (et_b4)(unsigned char)1;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) f(a[j].x, b[j].x, c[j].x), f(a[j].y, b[j].y, c[j].y), f(a[j].z, b[j].z, c[j].z), f(a[j].w, b[j].w, c[j].w);
    }
    for (; i < nv; i += BM_T) {
        const size_t o = lo + 4 * (size_t)i;
        const bm_f4u a = *(v4_t)(p + o), b = *(v4_t)(t + o);
        const et_b4 c = m ? *(b4_t)(m + o) : (et_b4)(unsigned char)1;
        f(a.x, b.x, c.x), f(a.y, b.y, c.y), f(a.z, b.z, c.z), f(a.w, b.w, c.w);
    }
    for (size_t k = (size_t)lo + 4 * (size_t)nv + threadIdx.x; k < hi; k += BM_T) f(p[k], t[k], m ? m[k] : (unsigned char)1);
}

// What a workgroup of variant v of pair g sweeps, and which pixels are inside: (mask byte != 0 or unmasked variant) and
// (target NaN or metric target < cutoff) — np.nan_to_num(target) < cutoff, strict; variant 0 of each half applies no cut-off test.
struct et_view_t {
    bm_src_t p, t;
    et_msk_t m;
    unsigned lo, hi;
    float reg, clip, lo_d, cutoff;
    bool cut, tmetric;
    __device__ __forceinline__ et_view_t(const float *const *preds, const float *const *targets, const unsigned char *const *masks, const et_args_t &a,
                                         int w, int v, size_t g) {
        const int c = v % (a.ncut + 1);
        p = (bm_src_t)preds[g], t = (bm_src_t)targets[g];
        m = v > a.ncut && masks ? (et_msk_t)masks[g] : (et_msk_t) nullptr;
        et_range(a.npix, a.Ws, w, lo, hi);
        reg = a.reg, clip = a.clip, lo_d = expf(-a.reg) * a.clip;
        cut = c != 0, cutoff = c ? a.cut[c - 1] : 0.f;
        tmetric = a.tmetric != 0;
    }
    // metric target of a pixel that is inside -> tm; nan: it has no ground truth
    __device__ __forceinline__ bool inside(float tn, unsigned char mv, float &tm, bool &nan) const {
        nan = !(tn == tn);
        tm = tmetric ? tn : et_metric_depth(tn, reg, clip, lo_d, false);
        return mv != 0 && (!cut || nan || tm < cutoff);
    }
    __device__ __forceinline__ float pred(float pn) const { return et_metric_depth(pn, reg, clip, lo_d, true); }
};

__device__ __forceinline__ unsigned et_key(float x) { return __float_as_uint(x) & 0x7fffffffu; }     // (a sign bit cannot leave the histogram)

// Stores the marked histograms of the workgroup to its slab (histogram h at h * nbins) and takes the ticket of (pair, variant).
__device__ __forceinline__ bool et_arrive(unsigned (*hist)[BM_BINS / 2], unsigned hmask, unsigned *slab, size_t cell, int P, int wg,
                                          unsigned *tickets, int *flag) {
    constexpr int NB = BM_BINS / 2;
    for (int h = 0; h < 4; ++h)
        if ((hmask >> h) & 1u)
            for (int b = threadIdx.x; b < NB; b += BM_T) slab[(cell * P + wg) * ET_SLAB + h * NB + b] = hist[h][b];
    return bm_ticket(cell, P, tickets, flag);
}

__device__ __forceinline__ float et_wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_down(v, o));
    return v;
}

// RS: a rescaled call (rows of ET_ROWX doubles; cst = the constants of the (pair, variant) cells)
template <bool RS>
__global__ void __launch_bounds__(BM_T) et_sums_kernel(const float *const *__restrict__ preds, const float *const *__restrict__ targets,
                                                       const unsigned char *const *__restrict__ masks, et_args_t a, unsigned *tickets, unsigned *state,
                                                       double *part, unsigned *slab, double *cst, double *__restrict__ out) {
    constexpr int ROW = RS ? ET_ROWX : ET_ROW;
    __shared__ unsigned hist[2][BM_BINS];
    __shared__ double red[ET_OUT][BM_T / 64], stage[ET_MAX_PER_MAP * ROW];
    __shared__ unsigned scan[BM_T / 64], res[2];
    __shared__ int flag;
    const int w = blockIdx.x, v = blockIdx.y, P = a.Ws;
    const size_t g = blockIdx.z, cell = g * a.V + v;
    unsigned *const both = &hist[0][0];
    for (int b = threadIdx.x; b < 2 * BM_BINS; b += BM_T) both[b] = 0;
    __syncthreads();
    const et_view_t vw(preds, targets, masks, a, w, v, g);
    double acc[ET_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double sum_t = 0.0, sum_p = 0.0;
    float min_t = __uint_as_float(0x7f800000u), min_p = __uint_as_float(0x7f800000u);
    unsigned nmask = 0, n = 0;
    const double eps = 1e-5;
    et_sweep(vw.p, vw.t, vw.m, vw.lo, vw.hi, [&](float pn, float tn, unsigned char mv) {
        float t;
        bool nan;
        if (!vw.inside(tn, mv, t, nan)) return;
        ++nmask;
        if (nan) return;
        const float p = vw.pred(pn);
        const double d = (double)t - (double)p, ld = log((double)t + eps) - log((double)p + eps);
        ++n;
        acc[2] += fabs(d) / ((double)t + 1e-6), acc[3] += d * d / ((double)t * t + 1e-6), acc[4] += d * d;
        acc[5] += ld * ld, acc[6] += fabs(ld), acc[7] += fabs(d);
        const double r = fmax((double)t / ((double)p + eps), (double)p / ((double)t + eps));
        acc[8] += r <= 1.25, acc[9] += r <= 1.5625, acc[10] += r <= 1.953125;
        atomicAdd(&hist[0][et_key(t) >> 20], 1u);
        atomicAdd(&hist[1][et_key(p) >> 20], 1u);
        if (RS) sum_t += (double)t, sum_p += (double)p, min_t = fminf(min_t, t), min_p = fminf(min_p, p);
    });
    acc[0] = (double)nmask, acc[1] = (double)n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < ET_COLS; ++k) {
        const double s = bm_wave_sum(acc[k]);
        if (lane == 0) red[k][wave] = s;
    }
    if (RS) {
        const double st = bm_wave_sum(sum_t), sp = bm_wave_sum(sum_p);
        const float mt = et_wave_min(min_t), mp = et_wave_min(min_p);
        if (lane == 0) red[11][wave] = st, red[12][wave] = sp, red[13][wave] = (double)mt, red[14][wave] = (double)mp;
    }
    __syncthreads();
    if (threadIdx.x < (RS ? 13 : ET_COLS)) {
        double s = 0.0;
        for (int i = 0; i < BM_T / 64; ++i) s += red[threadIdx.x][i];
        part[(cell * P + w) * ROW + threadIdx.x] = s;
    } else if (RS && threadIdx.x < 15) {
        double s = red[threadIdx.x][0];
        for (int i = 1; i < BM_T / 64; ++i) s = fmin(s, red[threadIdx.x][i]);
        part[(cell * P + w) * ROW + threadIdx.x] = s;
    }
    for (int b = threadIdx.x; b < 2 * BM_BINS; b += BM_T) slab[(cell * P + w) * ET_SLAB + b] = both[b];
    if (!bm_ticket(cell, P, tickets, &flag)) return;

    // last arrival of (pair, variant): the P <= 32 rows through LDS, one thread per column adds them in index order
    const double *rows = part + cell * P * ROW;
    for (int i = threadIdx.x; i < P * ROW; i += BM_T) stage[i] = bm_ld(rows + i);
    __syncthreads();
    if (threadIdx.x < (RS ? 13 : ET_COLS)) {
        double s = 0.0;
        for (int r = 0; r < P; ++r) s += stage[r * ROW + threadIdx.x];
        red[threadIdx.x][0] = s;
        if (!RS) out[cell * ET_OUT + threadIdx.x] = s;
    } else if (RS && threadIdx.x < 15) {
        double s = stage[threadIdx.x];
        for (int r = 1; r < P; ++r) s = fmin(s, stage[r * ROW + threadIdx.x]);
        red[threadIdx.x][0] = s;
    } else if (!RS && threadIdx.x < ET_OUT) {
        out[cell * ET_OUT + threadIdx.x] = threadIdx.x < 13 ? (double)__uint_as_float(0x7fc00000u) : 0.0;      // (pass 3 writes the medians it finds)
    }
    __syncthreads();
    const unsigned total = (unsigned)red[1][0];
    const bool wanted = total != 0 && red[0][0] == red[1][0];
    unsigned *st = state + cell * ET_STATE;
    if (RS) {
        // the row of a variant that takes no part in the later passes, and what pass 4 leaves alone; it overwrites columns 2..12 of the others
        if (threadIdx.x < ET_OUT) {
            const int c = threadIdx.x;
            out[cell * ET_OUT + c] = c < 2 ? red[c][0] : ((c < 8 || c == 11 || c == 12) ? (double)__uint_as_float(0x7fc00000u) : 0.0);
        }
        if (threadIdx.x < 2) cst[cell * ET_CST + threadIdx.x] = red[11 + threadIdx.x][0] / red[1][0];
        else if (threadIdx.x < 4) cst[cell * ET_CST + threadIdx.x] = red[11 + threadIdx.x][0];
    }
    if (wanted) {
        const unsigned r0 = (total - 1) / 2, r1 = total / 2;
        for (int s = 0; s < 2; ++s) {
            bm_join_slabs<BM_BINS, ET_SLAB, BM_BINS>(slab, cell, P, s, hist[0]);
            bm_select(hist[0], BM_BINS, r0, scan, res);
            if (threadIdx.x == 0) st[4 * s] = res[0], st[4 * s + 1] = res[1];
            bm_select(hist[0], BM_BINS, r1, scan, res);
            if (threadIdx.x == 0) st[4 * s + 2] = res[0], st[4 * s + 3] = res[1];
        }
    }
    if (threadIdx.x == 0) {
        st[8] = total, st[9] = wanted ? 1u : 0u;
        atomicExch(tickets + cell, 0u);                           // ready for the next pass
    }
}

// RS, SHIFT = 10: the sums of (t - mean t)^2 and (p - mean p)^2 ride along (rows of ET_ROWX doubles, columns 0 and 1) and the last arrival
// leaves both standard deviations in cst.  RS, SHIFT = 0: the middle values stay in the state for pass 4, which writes the medians.
template <int SHIFT, bool RS>
__global__ void __launch_bounds__(BM_T) et_select_kernel(const float *const *__restrict__ preds, const float *const *__restrict__ targets,
                                                         const unsigned char *const *__restrict__ masks, et_args_t a, unsigned *tickets, unsigned *state,
                                                         double *part, unsigned *slab, double *cst, double *__restrict__ out) {
    constexpr int NB = BM_BINS / 2;
    constexpr bool DEV = RS && SHIFT == 10;
    __shared__ unsigned hist[4][NB];
    __shared__ double red[2][BM_T / 64];
    __shared__ unsigned scan[BM_T / 64], res[2];
    __shared__ int flag;
    const int w = blockIdx.x, v = blockIdx.y, P = a.Ws;
    const size_t g = blockIdx.z, cell = g * a.V + v;
    unsigned *st = state + cell * ET_STATE;
    if (st[9] == 0) return;                                       // NaN medians: written by pass 1, no ticket is taken
    unsigned pre[4], rank[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) pre[k] = st[2 * k], rank[k] = st[2 * k + 1];
    const unsigned total = st[8];
    const bool two_t = pre[0] != pre[1], two_p = pre[2] != pre[3];
    for (int h = 0; h < 4; ++h)
        for (int b = threadIdx.x; b < NB; b += BM_T) hist[h][b] = 0;
    __syncthreads();
    const et_view_t vw(preds, targets, masks, a, w, v, g);
    const double mean_t = DEV ? cst[cell * ET_CST] : 0.0, mean_p = DEV ? cst[cell * ET_CST + 1] : 0.0;
    double dev_t = 0.0, dev_p = 0.0;
    et_sweep(vw.p, vw.t, vw.m, vw.lo, vw.hi, [&](float pn, float tn, unsigned char mv) {
        float t;
        bool nan;
        if (!vw.inside(tn, mv, t, nan) || nan) return;
        const float p = vw.pred(pn);
        if (DEV) {
            const double et = (double)t - mean_t, ep = (double)p - mean_p;
            dev_t += et * et, dev_p += ep * ep;
        }
        const unsigned kt = et_key(t), kp = et_key(p);
        const unsigned tt = kt >> (SHIFT + 10), tp = kp >> (SHIFT + 10);
        if (tt == pre[0]) atomicAdd(&hist[0][(kt >> SHIFT) & (NB - 1)], 1u);
        else if (tt == pre[1]) atomicAdd(&hist[1][(kt >> SHIFT) & (NB - 1)], 1u);
        if (tp == pre[2]) atomicAdd(&hist[2][(kp >> SHIFT) & (NB - 1)], 1u);
        else if (tp == pre[3]) atomicAdd(&hist[3][(kp >> SHIFT) & (NB - 1)], 1u);
    });
    if (DEV) {
        const double st_ = bm_wave_sum(dev_t), sp_ = bm_wave_sum(dev_p);
        if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = st_, red[1][threadIdx.x >> 6] = sp_;
    }
    __syncthreads();
    if (DEV && threadIdx.x < 2) {
        double s = 0.0;
        for (int i = 0; i < BM_T / 64; ++i) s += red[threadIdx.x][i];
        part[(cell * P + w) * ET_ROWX + threadIdx.x] = s;
    }
    if (!et_arrive(hist, 1u | (two_t ? 2u : 0u) | 4u | (two_p ? 8u : 0u), slab, cell, P, w, tickets, &flag)) return;

    if (DEV && threadIdx.x < 2) {                                 // np.std: sqrt(mean((x - mean(x))^2)), the rows in index order
        double s = 0.0;
        for (int r = 0; r < P; ++r) s += bm_ld(part + (cell * P + r) * ET_ROWX + threadIdx.x);
        cst[cell * ET_CST + 4 + threadIdx.x] = sqrt(s / (double)total);
    }
    unsigned found[4], inside[4];
    for (int s = 0; s < 2; ++s) {
        const bool two = s ? two_p : two_t;
        bm_join_slabs<NB, ET_SLAB, NB>(slab, cell, P, 2 * s, hist[0]);
        bm_select(hist[0], NB, rank[2 * s], scan, res);
        found[2 * s] = (pre[2 * s] << 10) | res[0], inside[2 * s] = res[1];
        __syncthreads();
        if (two) bm_join_slabs<NB, ET_SLAB, NB>(slab, cell, P, 2 * s + 1, hist[0]);
        bm_select(hist[0], NB, rank[2 * s + 1], scan, res);
        found[2 * s + 1] = (pre[2 * s + 1] << 10) | res[0], inside[2 * s + 1] = res[1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (SHIFT || RS) {
#pragma unroll
            for (int k = 0; k < 4; ++k) st[2 * k] = found[k], st[2 * k + 1] = inside[k];
        } else {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float fa = __uint_as_float(found[2 * s]), fb = __uint_as_float(found[2 * s + 1]);
                out[cell * ET_OUT + 11 + s] = (double)((total & 1u) ? fa : (fa + fb) * 0.5f);
            }
        }
        atomicExch(tickets + cell, 0u);
    }
}

// Pass 4 of a rescaled call: columns 2..12 of the row on the transformed pair (the header of this section; include/ramnet_hip.h).
__global__ void __launch_bounds__(BM_T) et_rescale_kernel(const float *const *__restrict__ preds, const float *const *__restrict__ targets,
                                                          const unsigned char *const *__restrict__ masks, et_args_t a, unsigned *tickets,
                                                          const unsigned *state, double *part, const double *cst, double *__restrict__ out) {
    __shared__ double red[ET_COLS][BM_T / 64], stage[ET_MAX_PER_MAP * ET_ROWX];
    __shared__ int flag;
    const int w = blockIdx.x, v = blockIdx.y, P = a.Ws;
    const size_t g = blockIdx.z, cell = g * a.V + v;
    const unsigned *st = state + cell * ET_STATE;
    if (st[9] == 0) return;                                       // its row was written by pass 1, no ticket is taken
    const bool odd = (st[8] & 1u) != 0;
    const double *c = cst + cell * ET_CST;
    double med[2], sd[2], off[2], m[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float fa = __uint_as_float(st[4 * s]), fb = __uint_as_float(st[4 * s + 2]);
        med[s] = (double)(odd ? fa : (fa + fb) * 0.5f);           // np.median of the float32 values
        sd[s] = c[4 + s];
        off[s] = fabs((c[2 + s] - med[s]) / sd[s]);
        const double ta = ((double)fa - med[s]) / sd[s] + off[s], tb = ((double)fb - med[s]) / sd[s] + off[s];
        m[s] = odd ? ta : (ta + tb) * 0.5;
    }
    const double md = fabs(m[0] - m[1]);
    const bool up_t = m[0] < m[1];                                // the side with the smaller median is lifted (a NaN: the prediction)
    const et_view_t vw(preds, targets, masks, a, w, v, g);
    double acc[ET_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double eps = 1e-5;
    et_sweep(vw.p, vw.t, vw.m, vw.lo, vw.hi, [&](float pn, float tn, unsigned char mv) {
        float tf;
        bool nan;
        if (!vw.inside(tn, mv, tf, nan) || nan) return;
        double t = ((double)tf - med[0]) / sd[0] + off[0], p = ((double)vw.pred(pn) - med[1]) / sd[1] + off[1];
        if (up_t) t += md;
        else p += md;
        const double d = t - p, ld = log(t + eps) - log(p + eps);
        acc[2] += fabs(d) / (t + 1e-6), acc[3] += d * d / (t * t + 1e-6), acc[4] += d * d;
        acc[5] += ld * ld, acc[6] += fabs(ld), acc[7] += fabs(d);
        const double r = fmax(t / (p + eps), p / (t + eps));
        acc[8] += r <= 1.25, acc[9] += r <= 1.5625, acc[10] += r <= 1.953125;
    });
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 2; k < ET_COLS; ++k) {
        const double s = bm_wave_sum(acc[k]);
        if (lane == 0) red[k][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x >= 2 && threadIdx.x < ET_COLS) {
        double s = 0.0;
        for (int i = 0; i < BM_T / 64; ++i) s += red[threadIdx.x][i];
        part[(cell * P + w) * ET_ROWX + threadIdx.x] = s;
    }
    if (!bm_ticket(cell, P, tickets, &flag)) return;

    const double *rows = part + cell * P * ET_ROWX;
    for (int i = threadIdx.x; i < P * ET_ROWX; i += BM_T) stage[i] = bm_ld(rows + i);
    __syncthreads();
    if (threadIdx.x >= 2 && threadIdx.x < ET_COLS) {
        double s = 0.0;
        for (int r = 0; r < P; ++r) s += stage[r * ET_ROWX + threadIdx.x];
        out[cell * ET_OUT + threadIdx.x] = s;
    } else if (threadIdx.x == 11) {
        out[cell * ET_OUT + 11] = up_t ? m[0] + md : m[0];
    } else if (threadIdx.x == 12) {
        out[cell * ET_OUT + 12] = up_t ? m[1] : m[1] + md;
    }
    if (threadIdx.x == 0) atomicExch(tickets + cell, 0u);
}

// Metric targets at reduced resolution (evaluation.py:87-94): F.interpolate(metric target, scale_factor = s, mode = 'bilinear') at its
// defaults — align_corners = False, source coordinate (dst + 0.5) / s - 0.5 from the GIVEN factor, clamped at 0 — on the metric depths of
// et_metric_depth (no clamp), the four products in double, rounded once to float32.  A NaN tap makes the output NaN, at weight zero too.
__global__ void __launch_bounds__(256) resize_metric_target_kernel(const float *const *__restrict__ targets, int H, int W, int Ho, int Wo, double rs,
                                                                   float clip, float reg, float *__restrict__ out) {
    const size_t g = blockIdx.y, n = (size_t)Ho * Wo;
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int oy = (int)(i / Wo), ox = (int)(i % Wo);
    const double sy = fmax(rs * ((double)oy + 0.5) - 0.5, 0.0), sx = fmax(rs * ((double)ox + 0.5) - 0.5, 0.0);
    const int y0 = min((int)sy, H - 1), x0 = min((int)sx, W - 1);
    const int y1 = y0 + (y0 < H - 1), x1 = x0 + (x0 < W - 1);
    const double ly = sy - (double)y0, lx = sx - (double)x0;
    const float *t = targets[g];
    const double t00 = (double)et_metric_depth(t[(size_t)y0 * W + x0], reg, clip, 0.f, false);
    const double t01 = (double)et_metric_depth(t[(size_t)y0 * W + x1], reg, clip, 0.f, false);
    const double t10 = (double)et_metric_depth(t[(size_t)y1 * W + x0], reg, clip, 0.f, false);
    const double t11 = (double)et_metric_depth(t[(size_t)y1 * W + x1], reg, clip, 0.f, false);
    out[g * n + i] = (float)((1.0 - ly) * ((1.0 - lx) * t00 + lx * t01) + ly * ((1.0 - lx) * t10 + lx * t11));
}

__global__ void __launch_bounds__(256) metric_depth_kernel(const float *__restrict__ y, size_t n, float clip, float reg, int clamp, float *__restrict__ out) {
    const float lo = expf(-reg) * clip;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = et_metric_depth(y[i], reg, clip, lo, clamp != 0);
}

}  // namespace ramnet

extern "C" int ramnet_metric_depth(const float *y, size_t n, float clip_distance, float reg_factor, int clamp, float *out, void *stream) {
    RAMNET_CHECK_ARG(y && out && n > 0 && clip_distance > 0.f);
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(metric_depth_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, y, n, clip_distance,
                       reg_factor, clamp, out);
    RAMNET_LAUNCH_CHECK();
    return 0;
}

static int et_launch(const float *const *pred, const float *const *target, const unsigned char *const *mask, int G, size_t npix, float clip_distance,
                     float reg_factor, const float *cutoffs, int ncut, int flags, void *workspace, double *out, void *stream) {
    RAMNET_CHECK_ARG(pred && target && workspace && out && clip_distance > 0.f);
    RAMNET_CHECK_ARG(et_sizes_ok(G, npix, ncut, mask != nullptr));
    RAMNET_CHECK_ARG(ncut == 0 || cutoffs);
    for (int i = 0; i < ncut; ++i) RAMNET_CHECK_ARG(cutoffs[i] > (i ? cutoffs[i - 1] : 0.f));
    RAMNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0);
    RAMNET_CHECK_ARG((flags & ~(RAMNET_EVAL_RESCALE | RAMNET_EVAL_TARGET_METRIC)) == 0);
    const bool rescale = (flags & RAMNET_EVAL_RESCALE) != 0;
    const et_plan_t pl = et_plan(G, npix, ncut, mask != nullptr, rescale);
    et_args_t a;
    a.clip = clip_distance, a.reg = reg_factor, a.ncut = ncut, a.V = pl.V, a.Ws = pl.Ws, a.npix = (unsigned)npix;
    a.tmetric = (flags & RAMNET_EVAL_TARGET_METRIC) != 0;
    for (int i = 0; i < ET_MAXCUT; ++i) a.cut[i] = i < ncut ? cutoffs[i] : 0.f;
    char *ws = static_cast<char *>(workspace);
    unsigned *tickets = reinterpret_cast<unsigned *>(ws), *state = reinterpret_cast<unsigned *>(ws + pl.off_state);
    double *part = reinterpret_cast<double *>(ws + pl.off_part), *cst = reinterpret_cast<double *>(ws + pl.off_cst);
    unsigned *slab = reinterpret_cast<unsigned *>(ws + pl.off_slab);
    const dim3 grid(pl.Ws, pl.V, G);
    hipStream_t st = (hipStream_t)stream;
    if (rescale) {
        hipLaunchKernelGGL(et_sums_kernel<true>, grid, dim3(BM_T), 0, st, pred, target, mask, a, tickets, state, part, slab, cst, out);
        hipLaunchKernelGGL((et_select_kernel<10, true>), grid, dim3(BM_T), 0, st, pred, target, mask, a, tickets, state, part, slab, cst, out);
        hipLaunchKernelGGL((et_select_kernel<0, true>), grid, dim3(BM_T), 0, st, pred, target, mask, a, tickets, state, part, slab, cst, out);
        hipLaunchKernelGGL(et_rescale_kernel, grid, dim3(BM_T), 0, st, pred, target, mask, a, tickets, state, part, cst, out);
        RAMNET_LAUNCH_CHECK();
        note_kernel("et_sums_kernel<rescale> + et_select_kernel<10> + et_select_kernel<0> + et_rescale_kernel");
        return 0;
    }
    hipLaunchKernelGGL(et_sums_kernel<false>, grid, dim3(BM_T), 0, st, pred, target, mask, a, tickets, state, part, slab, cst, out);
    hipLaunchKernelGGL((et_select_kernel<10, false>), grid, dim3(BM_T), 0, st, pred, target, mask, a, tickets, state, part, slab, cst, out);
    hipLaunchKernelGGL((et_select_kernel<0, false>), grid, dim3(BM_T), 0, st, pred, target, mask, a, tickets, state, part, slab, cst, out);
    RAMNET_LAUNCH_CHECK();
    note_kernel("et_sums_kernel + et_select_kernel<10> + et_select_kernel<0>");
    return 0;
}

extern "C" size_t ramnet_eval_table_workspace(int G, size_t npix, int ncut, int has_mask) {
    return et_sizes_ok(G, npix, ncut, has_mask) ? et_plan(G, npix, ncut, has_mask).total : 0;
}

extern "C" int ramnet_eval_table(const float *const *pred, const float *const *target, const unsigned char *const *mask, int G, size_t npix,
                                 float clip_distance, float reg_factor, const float *cutoffs, int ncut, void *workspace, double *out, void *stream) {
    return et_launch(pred, target, mask, G, npix, clip_distance, reg_factor, cutoffs, ncut, 0, workspace, out, stream);
}

extern "C" size_t ramnet_eval_table_ex_workspace(int G, size_t npix, int ncut, int has_mask, int flags) {
    if ((flags & ~(RAMNET_EVAL_RESCALE | RAMNET_EVAL_TARGET_METRIC)) != 0 || !et_sizes_ok(G, npix, ncut, has_mask)) return 0;
    return et_plan(G, npix, ncut, has_mask, (flags & RAMNET_EVAL_RESCALE) != 0).total;
}

extern "C" int ramnet_eval_table_ex(const float *const *pred, const float *const *target, const unsigned char *const *mask, int G, size_t npix,
                                    float clip_distance, float reg_factor, const float *cutoffs, int ncut, int flags, void *workspace, double *out,
                                    void *stream) {
    return et_launch(pred, target, mask, G, npix, clip_distance, reg_factor, cutoffs, ncut, flags, workspace, out, stream);
}

extern "C" int ramnet_resize_metric_target(const float *const *target, int G, int H, int W, double scale_factor, float clip_distance, float reg_factor,
                                           float *out, void *stream) {
    RAMNET_CHECK_ARG(target && out && clip_distance > 0.f);
    RAMNET_CHECK_ARG(G >= 1 && G <= 65535 && H >= 1 && W >= 1 && (size_t)H * W < ((size_t)1 << 31));
    RAMNET_CHECK_ARG(scale_factor > 0.0 && scale_factor <= 1.0);
    const int Ho = (int)floor((double)H * scale_factor), Wo = (int)floor((double)W * scale_factor);
    RAMNET_CHECK_ARG(Ho >= 1 && Wo >= 1);
    const size_t n = (size_t)Ho * Wo;
    hipLaunchKernelGGL(resize_metric_target_kernel, dim3((unsigned)((n + 255) / 256), G), dim3(256), 0, (hipStream_t)stream, target, H, W, Ho, Wo,
                       1.0 / scale_factor, clip_distance, reg_factor, out);
    RAMNET_LAUNCH_CHECK();
    return 0;
}
