// The fixed-tree reduction layer of the length-n kernels: wavefront shuffles, then the waves of a block in wave
// order, then the blocks in block order.  Every sum of vec_kernels.hip, shannon_kernels.hip, quartic_kernels.hip and
// inexact_kernels.hip runs over this one tree, so repeated calls are bit-identical and the parity tests can hold a
// result to the rounding of one summation order.  Sets no compile flag: the including translation unit decides
// about -ffp-contract.
#pragma once
#include "internal.h"

namespace accbpg {

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}
// minimum that keeps a NaN (np.min does; fmin would drop it and a NaN would slip through the reference's
// `x.min() > 0` assertions, functions.py:252)
__device__ __forceinline__ double min_nan(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min_nan(v, __shfl_down(v, off));
    return v;
}

// Block stage.  The NS per-thread values of a block of NT threads (sums; the last one a minimum when MIN_LAST), each
// reduced over wave shuffles (in place) and then the waves in wave order, written to a record of OUT slots at dst: the
// sums in front, the minimum in the last slot, the slots between (OUT > NS) as 0.0.
// Thread k folds slot k starting from wave 0's value.  Starting from 0.0 instead, or one thread folding every slot,
// is the same arithmetic: each slot's waves are added in wave order by one thread, and 0.0 + v has the bits of v for
// every v that a sum started at +0.0 can reach (round-to-nearest never turns it into -0.0).
template <int NT, int NS, bool MIN_LAST, int OUT = NS>
__device__ __forceinline__ void block_reduce_store(double (&v)[NS], double* __restrict__ dst) {
    static_assert(NT % 64 == 0 && OUT >= NS && OUT <= NT, "block_reduce_store: bad shape");
    __shared__ double sh[NS][NT / 64];
    constexpr int NSUM = MIN_LAST ? NS - 1 : NS;
#pragma unroll
    for (int k = 0; k < NSUM; ++k) v[k] = wave_sum(v[k]);
    const double mn = MIN_LAST ? wave_min(v[NS - 1]) : 0.0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NSUM; ++k) sh[k][w] = v[k];
        if (MIN_LAST) sh[NS - 1][w] = mn;
    }
    __syncthreads();
    if (threadIdx.x < OUT) {
        const int k = threadIdx.x;
        const bool is_min = MIN_LAST && k == OUT - 1;
        const int src = (OUT > NS && is_min) ? NS - 1 : k;      // the slot of sh behind dst[k]
        double a = 0.0;
        if (OUT == NS || is_min || k < NSUM) {
            a = sh[src][0];
            for (int j = 1; j < NT / 64; ++j) a = is_min ? min_nan(a, sh[src][j]) : a + sh[src][j];
        }
        dst[k] = a;
    }
}

// Final stage: one workgroup adds the records part[b*NS + k] of nb blocks in block order, out[0..NS) as the slots
template <int NT, int NS, bool MIN_LAST>
__device__ __forceinline__ void reduce_final_body(const double* __restrict__ part, int nb, double* __restrict__ out) {
    constexpr int NSUM = MIN_LAST ? NS - 1 : NS;
    double s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = (k < NSUM) ? 0.0 : __builtin_inf();
    for (int b = threadIdx.x; b < nb; b += NT) {
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = (k < NSUM) ? s[k] + part[b * NS + k] : min_nan(s[k], part[b * NS + k]);
    }
    block_reduce_store<NT, NS, MIN_LAST>(s, out);
}
template <int NT, int NS, bool MIN_LAST>
__global__ __launch_bounds__(NT) void reduce_final_kernel(const double* __restrict__ part, int nb,
                                                          double* __restrict__ out) {
    reduce_final_body<NT, NS, MIN_LAST>(part, nb, out);
}

constexpr int RED_THREADS = 256;     // threads of the streaming reductions and of the elementwise passes

// blocks of a streaming reduction over n entries: four entries per thread, at most max_blocks.  The count fixes the
// summation order, and NS * max_blocks partials must fit behind the n doubles of the workspace (vec_ws_doubles).
inline int red_blocks(int64_t n, int max_blocks) {
    int64_t b = (n + (int64_t)RED_THREADS * 4 - 1) / ((int64_t)RED_THREADS * 4);
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (int)b;
}
// blocks of an elementwise pass over n entries
inline int ew_blocks(int64_t n) {
    const int64_t b = (n + RED_THREADS - 1) / RED_THREADS;
    return (int)(b > 2048 ? 2048 : b);
}

// First-index arg-minimum and arg-maximum over RED_THREADS-wide blocks (accbpg_vec_argminmax and the Kumar-Yildirim
// start).  An arg-extremum is exact in any merge order, so these follow the tree's shape without being part of it.
struct MinMaxRec {
    double vmin, vmax;
    int64_t imin, imax;
};
__device__ __forceinline__ MinMaxRec mm_merge(MinMaxRec a, MinMaxRec b) {
    // np.argmin / np.argmax: a NaN is the extremum; among equals (or among NaNs) the first index wins
    MinMaxRec r = a;
    const bool an = a.vmin != a.vmin, bn = b.vmin != b.vmin;
    if ((bn && !an) || (!an && b.vmin < a.vmin) || ((b.vmin == a.vmin || (an && bn)) && b.imin < a.imin)) {
        r.vmin = b.vmin; r.imin = b.imin;
    }
    const bool ax = a.vmax != a.vmax, bx = b.vmax != b.vmax;
    if ((bx && !ax) || (!ax && b.vmax > a.vmax) || ((b.vmax == a.vmax || (ax && bx)) && b.imax < a.imax)) {
        r.vmax = b.vmax; r.imax = b.imax;
    }
    return r;
}
// the records of a block's RED_THREADS threads merged; every thread returns the block's record
__device__ __forceinline__ MinMaxRec mm_block(MinMaxRec a, MinMaxRec* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        MinMaxRec o;
        o.vmin = __shfl_down(a.vmin, off); o.vmax = __shfl_down(a.vmax, off);
        o.imin = __shfl_down((long long)a.imin, off); o.imax = __shfl_down((long long)a.imax, off);
        a = mm_merge(a, o);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = a;
    __syncthreads();
    MinMaxRec r = sh[0];
    for (int i = 1; i < RED_THREADS / 64; ++i) r = mm_merge(r, sh[i]);
    return r;
}
// stage 1: block b's record of the entries b*RED_THREADS + t + k*gridDim.x*RED_THREADS, into part[b]
__device__ __forceinline__ void minmax_partial_body(const double* __restrict__ x, int64_t n,
                                                    MinMaxRec* __restrict__ part) {
    __shared__ MinMaxRec sh[RED_THREADS / 64];
    const double inf = __builtin_inf();
    MinMaxRec a{inf, -inf, INT64_MAX, INT64_MAX};
    const int64_t stride = (int64_t)gridDim.x * RED_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += stride) {
        const double v = x[i];
        a = mm_merge(a, MinMaxRec{v, v, i, i});
    }
    a = mm_block(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}
// stage 2 (one block): the nblk stage-1 records merged; every thread returns the result
__device__ __forceinline__ MinMaxRec minmax_final_body(const MinMaxRec* __restrict__ part, int nblk) {
    __shared__ MinMaxRec sh[RED_THREADS / 64];
    const double inf = __builtin_inf();
    MinMaxRec a{inf, -inf, INT64_MAX, INT64_MAX};
    for (int b = threadIdx.x; b < nblk; b += RED_THREADS) a = mm_merge(a, part[b]);
    return mm_block(a, sh);
}

// Host tail of a reduction on stream s.  Launches `final_kernel` over the nb block records at part into red_out --
// unless it is null: a pass of a single block has written its result itself -- checks the launches, copies `count`
// doubles from dout (the device scratch of vec_scratch) to pin + 8, waits, and returns pin + 8; null after a HIP error
// (the message is set).
typedef void (*reduce_final_fn)(const double*, int, double*);
inline const double* reduce_finish(reduce_final_fn final_kernel, const double* part, int nb, double* red_out,
                                   const double* dout, int count, double* pin, hipStream_t s) {
    auto tail = [&]() -> int {
        if (final_kernel) final_kernel<<<1, RED_THREADS, 0, s>>>(part, nb, red_out);
        ACC_HIP(hipGetLastError());
        ACC_HIP(hipMemcpyAsync(pin + 8, dout, count * sizeof(double), hipMemcpyDeviceToHost, s));
        ACC_HIP(hipStreamSynchronize(s));
        return ACCBPG_OK;
    };
    return tail() == ACCBPG_OK ? pin + 8 : nullptr;
}

}  // namespace accbpg
