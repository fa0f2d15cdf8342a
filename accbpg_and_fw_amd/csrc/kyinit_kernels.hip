// Kumar-Yildirim starting point of the D-optimal design solvers (accbpg/applications.py:59-95) with every step decided on
// the device: the Gram-Schmidt recurrences, the pass over V, the arg-extrema and the column difference are enqueued for
// all m steps on the handle's stream, and the host waits once, at the end.  accbpg_dopt_batch_kyinit runs the K
// instances of a batch through the same bodies in lock-step: every launch carries an instance dimension on its grid.
//
// Q is stored column-contiguous: column j at Q + j*m.
//
// THE SUMMATION ORDER of every dot <Q[:,j], s> and of every sum of squares over m entries -- the same for every j, every
// step and every grid size, because one workgroup of 256 threads owns the whole sum:
//   1. thread t folds the terms t, t + 256, t + 512, ... in that order into an accumulator started at +0.0;
//   2. inside each wavefront of 64 lanes, wave_sum: v[l] += v[l + off] for off = 32, 16, 8, 4, 2, 1;
//   3. the four wavefronts are added in wave order, starting from wave 0's value.
// (reduce.hpp's block stage on strided per-thread partial sums, with no stage across blocks.)  Each term is one rounded
// product; this file is compiled with -ffp-contract=off, so no product is fused into the addition that follows it.
#include "internal.h"
#include "reduce.hpp"

namespace accbpg {

constexpr int KB = RED_THREADS;     // threads of the one-workgroup sums and of the arg-extremum stages
constexpr int KROWS = 64;           // rows (= threads) per workgroup of the deflation: one wavefront, so that even m = 2048
                                    // spreads over 32 CUs
constexpr int KY_MAXREC = 128;      // stage-1 records of the arg-extremum, as accbpg_vec_argminmax

// the sum over r < m of term(r) in the order above; every thread returns it
template <class F>
__device__ __forceinline__ double ky_tree_sum(int64_t m, F term) {
    __shared__ double total;
    double s = 0.0;
    for (int64_t r = threadIdx.x; r < m; r += KB) s += term(r);
    double v[1] = {s};
    block_reduce_store<KB, 1, false>(v, &total);
    __syncthreads();
    return total;
}

// col <- col / sqrt(sum col^2)  (q / np.linalg.norm(q), :89): a true division; a zero norm gives NaN as it does there
__device__ __forceinline__ void ky_normalize_body(double* col, int64_t m) {
    const double nrm = sqrt(ky_tree_sum(m, [&](int64_t r) { return col[r] * col[r]; }));
    for (int64_t r = threadIdx.x; r < m; r += KB) col[r] = col[r] / nrm;
    __syncthreads();        // the workgroup reads the column back right away (ky_dots_kernel)
}

// c[j] = <Q[:,j], src> for j = blockIdx.x (Rij of :77 and :87; the coefficients of one vector are independent of each
// other because each is taken from the un-deflated vector).  norm_last: column gridDim.x - 1 still holds the raw
// deflated vector of the step before; its workgroup normalises it first (:89), before anything reads it -- the
// deflation that uses it runs behind this kernel.
__device__ __forceinline__ void ky_dots_body(double* Q, const double* __restrict__ src, int64_t m, int norm_last,
                                             double* __restrict__ c) {
    double* col = Q + (size_t)blockIdx.x * (size_t)m;
    if (norm_last && blockIdx.x == gridDim.x - 1) ky_normalize_body(col, m);
    const double d = ky_tree_sum(m, [&](int64_t r) { return col[r] * src[r]; });
    if (threadIdx.x == 0) c[blockIdx.x] = d;
}

// out[r] = src[r] - c[0]*Q[r,0] - c[1]*Q[r,1] - ... - c[ncoef-1]*Q[r,ncoef-1], subtracted in that order with a rounded
// product each (q = q - Rij * Q[:,j], :78 and :88); one thread per row, so the reads of a column are coalesced
__device__ __forceinline__ void ky_deflate_body(const double* __restrict__ Q, const double* __restrict__ src,
                                                const double* __restrict__ c, int ncoef, int64_t m,
                                                double* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * KROWS + threadIdx.x;
    if (r >= m) return;
    double a = src[r];
    const double* qr = Q + r;
#pragma unroll 16
    for (int j = 0; j < ncoef; ++j) {
        const double p = c[j] * qr[(size_t)j * (size_t)m];
        a = a - p;
    }
    out[r] = a;
}

// kmax = argmax w, kmin = argmin w from the stage-1 records (np.argmax / np.argmin, :80-81: first index on ties, a NaN
// is the extremum), then v = V[:,kmin] - V[:,kmax] (:84).  Every workgroup merges the (at most 128) records itself and
// takes a block of rows; workgroup 0 records the pair.  Both indices are clamped to [0, n): whatever w holds, the
// column reads stay inside V.
__device__ __forceinline__ void ky_pick_coldiff_body(const MinMaxRec* __restrict__ part, int nblk,
                                                     const double* __restrict__ V, int64_t ldv, int64_t m, int64_t n,
                                                     int64_t* __restrict__ picked, double* __restrict__ v) {
    const MinMaxRec a = minmax_final_body(part, nblk);
    int64_t kmax = a.imax, kmin = a.imin;
    kmax = kmax < 0 ? 0 : (kmax >= n ? n - 1 : kmax);
    kmin = kmin < 0 ? 0 : (kmin >= n ? n - 1 : kmin);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        picked[0] = kmax;       // I.append(kmax); I.append(kmin)  (:82-83)
        picked[1] = kmin;
    }
    const int64_t r = (int64_t)blockIdx.x * KB + threadIdx.x;
    if (r < m) v[r] = V[r * ldv + kmin] - V[r * ldv + kmax];
}

// ---- one instance: the call's pointers as arguments --------------------------------------------------------------
__global__ __launch_bounds__(KB) void ky_normalize_kernel(double* col, int64_t m) { ky_normalize_body(col, m); }
__global__ __launch_bounds__(KB) void ky_dots_kernel(double* Q, const double* __restrict__ src, int64_t m,
                                                     int norm_last, double* __restrict__ c) {
    ky_dots_body(Q, src, m, norm_last, c);
}
__global__ __launch_bounds__(KROWS) void ky_deflate_kernel(const double* __restrict__ Q, const double* __restrict__ src,
                                                           const double* __restrict__ c, int ncoef, int64_t m,
                                                           double* __restrict__ out) {
    ky_deflate_body(Q, src, c, ncoef, m, out);
}
__global__ __launch_bounds__(KB) void ky_minmax_partial_kernel(const double* __restrict__ w, int64_t n,
                                                              MinMaxRec* __restrict__ part) {
    minmax_partial_body(w, n, part);
}
__global__ __launch_bounds__(KB) void ky_pick_coldiff_kernel(const MinMaxRec* __restrict__ part, int nblk,
                                                            const double* __restrict__ V, int64_t ldv, int64_t m,
                                                            int64_t n, int64_t* __restrict__ picked,
                                                            double* __restrict__ v) {
    ky_pick_coldiff_body(part, nblk, V, ldv, m, n, picked, v);
}

// ---- the instances of a batch in lock-step -------------------------------------------------------------------------
// The instance is blockIdx.y and its pointers come from the call's device table (KyInst); blockIdx.x and gridDim.x are
// what the single launch has, so the bodies partition, sum and round as they do there.  `step` selects the row of B
// and the column of Q.  `second` selects the half of a step: 0 deflates the direction b into q, 1 deflates the column
// difference v into Q[:,step].
__global__ __launch_bounds__(KB) void ky_normalize_batch_kernel(const KyInst* __restrict__ tab, int64_t m, int64_t col) {
    const KyInst t = tab[blockIdx.y];
    ky_normalize_body(t.Q + (size_t)col * (size_t)m, m);
}
__global__ __launch_bounds__(KB) void ky_dots_batch_kernel(const KyInst* __restrict__ tab, int64_t m, int64_t step,
                                                           int second) {
    const KyInst t = tab[blockIdx.y];
    ky_dots_body(t.Q, second ? t.v : t.B + (size_t)step * (size_t)m, m, second ? 0 : 1, t.c);
}
__global__ __launch_bounds__(KROWS) void ky_deflate_batch_kernel(const KyInst* __restrict__ tab, int64_t m,
                                                                 int64_t step, int second) {
    const KyInst t = tab[blockIdx.y];
    ky_deflate_body(t.Q, second ? t.v : t.B + (size_t)step * (size_t)m, t.c, (int)step, m,
                    second ? t.Q + (size_t)step * (size_t)m : t.q);
}
__global__ __launch_bounds__(KB) void ky_minmax_partial_batch_kernel(const KyInst* __restrict__ tab, int64_t n) {
    const KyInst t = tab[blockIdx.y];
    minmax_partial_body(t.w, n, t.part);
}
__global__ __launch_bounds__(KB) void ky_pick_coldiff_batch_kernel(const KyInst* __restrict__ tab, int nblk, int64_t ldv,
                                                                   int64_t m, int64_t n, int64_t step) {
    const KyInst t = tab[blockIdx.y];
    ky_pick_coldiff_body(t.part, nblk, t.V, ldv, m, n, t.picked + 2 * step, step > 0 ? t.v : t.Q);
}

// the m steps on h's stream; Q, w, q, v, c, part and picked are the call's own device buffers
static int ky_enqueue(accbpg_dopt* h, const double* B, double* Q, double* w, double* q, double* v, double* c,
                      MinMaxRec* part, int64_t* picked) {
    const int64_t m = h->m, n = h->n;
    hipStream_t s = h->stream;
    const int nsplit = vt_nsplit(m, n, h->num_cu);              // the partition of accbpg_dopt_vt_times
    const int nrec = red_blocks(n, KY_MAXREC);
    const int rowblocks = (int)((m + KROWS - 1) / KROWS);
    const int pickblocks = (int)((m + KB - 1) / KB);
    for (int64_t i = 0; i < m; ++i) {
        const double* b = B + (size_t)i * (size_t)m;
        double* col = Q + (size_t)i * (size_t)m;
        const double* dir = b;                                  // step 0 has no coefficients: q = b, and v goes to Q[:,0]
        if (i > 0) {
            ky_dots_kernel<<<(unsigned)i, KB, 0, s>>>(Q, b, m, 1, c);
            ky_deflate_kernel<<<rowblocks, KROWS, 0, s>>>(Q, b, c, (int)i, m, q);
            dir = q;
        }
        ACC_HIP(hipGetLastError());
        ACC_TRY(launch_vt_times(h->V, h->ldv, m, n, dir, h->vws, nsplit, w, h->vec_ok, s));
        ky_minmax_partial_kernel<<<nrec, KB, 0, s>>>(w, n, part);
        ky_pick_coldiff_kernel<<<pickblocks, KB, 0, s>>>(part, nrec, h->V, h->ldv, m, n, picked + 2 * i, i > 0 ? v : col);
        if (i > 0) {
            ky_dots_kernel<<<(unsigned)i, KB, 0, s>>>(Q, v, m, 0, c);
            ky_deflate_kernel<<<rowblocks, KROWS, 0, s>>>(Q, v, c, (int)i, m, col);
        }
        ACC_HIP(hipGetLastError());
    }
    ky_normalize_kernel<<<1, KB, 0, s>>>(Q + (size_t)(m - 1) * (size_t)m, m);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

// the same m steps for the K instances of tab on stream s: the launch sequence above with an instance dimension on every
// grid, so 8 launches per step (4 at step 0) whatever K is.  nsplit is instance 0's: one shape, one device.
static int ky_enqueue_batch(const KyInst* tab, int K, int64_t m, int64_t n, int64_t ldv, int nsplit, hipStream_t s) {
    const unsigned k = (unsigned)K;
    const int nrec = red_blocks(n, KY_MAXREC);
    const unsigned rowblocks = (unsigned)((m + KROWS - 1) / KROWS);
    const unsigned pickblocks = (unsigned)((m + KB - 1) / KB);
    for (int64_t i = 0; i < m; ++i) {
        if (i > 0) {
            ky_dots_batch_kernel<<<dim3((unsigned)i, k), KB, 0, s>>>(tab, m, i, 0);
            ky_deflate_batch_kernel<<<dim3(rowblocks, k), KROWS, 0, s>>>(tab, m, i, 0);
        }
        ACC_HIP(hipGetLastError());
        ACC_TRY(launch_vt_times_batch(tab, K, ldv, m, n, i == 0, nsplit, s));
        ky_minmax_partial_batch_kernel<<<dim3((unsigned)nrec, k), KB, 0, s>>>(tab, n);
        ky_pick_coldiff_batch_kernel<<<dim3(pickblocks, k), KB, 0, s>>>(tab, nrec, ldv, m, n, i);
        if (i > 0) {
            ky_dots_batch_kernel<<<dim3((unsigned)i, k), KB, 0, s>>>(tab, m, i, 1);
            ky_deflate_batch_kernel<<<dim3(rowblocks, k), KROWS, 0, s>>>(tab, m, i, 1);
        }
        ACC_HIP(hipGetLastError());
    }
    ky_normalize_batch_kernel<<<dim3(1, k), KB, 0, s>>>(tab, m, m - 1);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

}  // namespace accbpg

using namespace accbpg;

extern "C" int accbpg_dopt_kyinit(accbpg_dopt* h, const double* B_dev, int64_t* picked_host, double* Q_dev) {
    if (!h || !B_dev || !picked_host) return ACCBPG_ERR_ARG;
    const size_t m = (size_t)h->m, n = (size_t)h->n;
    // one allocation: [Q m*m when the caller gave none] w n | q m | v m | c m | 128 records | picked 2m
    const size_t qd = Q_dev ? 0 : m * m;
    const size_t doubles = qd + n + 3 * m + KY_MAXREC * sizeof(MinMaxRec) / sizeof(double) + 2 * m;
    double* buf = nullptr;
    ACC_HIP(acc_malloc(&buf, doubles * sizeof(double), "kyinit scratch"));
    double* Q = Q_dev ? Q_dev : buf;
    double* w = buf + qd;
    double* q = w + n;
    double* v = q + m;
    double* c = v + m;
    MinMaxRec* part = reinterpret_cast<MinMaxRec*>(c + m);
    int64_t* picked = reinterpret_cast<int64_t*>(part + KY_MAXREC);
    auto run = [&]() -> int {
        ACC_TRY(ky_enqueue(h, B_dev, Q, w, q, v, c, part, picked));
        ACC_HIP(hipMemcpyAsync(picked_host, picked, 2 * m * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        return ACCBPG_OK;
    };
    const int rc = run();
    const hipError_t waited = hipStreamSynchronize(h->stream);  // (also behind an error: nothing stays in flight)
    acc_free(buf);
    if (rc != ACCBPG_OK) return rc;
    ACC_HIP(waited);
    return ACCBPG_OK;
}

// The K starts of a batch in lock-step on the batch's stream.  One allocation, freed before the call returns -- per
// instance [Q m*m when the caller gave none] w n | q m | v m | c m | 128 records, then the K*2m indices of all
// instances in one piece (one copy to the host), then the K table entries.  Of the instances' handles only the
// vt_times workspace is written.
extern "C" int accbpg_dopt_batch_kyinit(accbpg_dopt_batch* b, const double* B_dev, int64_t* picked_host, double* Q_dev) {
    if (!b || !B_dev || !picked_host) return ACCBPG_ERR_ARG;
    const accbpg_dopt* h0 = b->inst[0];
    const size_t m = (size_t)h0->m, n = (size_t)h0->n, K = (size_t)b->K;
    const size_t qd = Q_dev ? 0 : m * m;
    const size_t per = qd + n + 3 * m + KY_MAXREC * sizeof(MinMaxRec) / sizeof(double);
    const size_t bytes = (K * per + K * 2 * m) * sizeof(double) + K * sizeof(KyInst);
    double* buf = nullptr;
    ACC_HIP(acc_malloc(&buf, bytes, "batch kyinit scratch"));
    int64_t* picked = reinterpret_cast<int64_t*>(buf + K * per);
    KyInst* tab_dev = reinterpret_cast<KyInst*>(picked + K * 2 * m);
    std::vector<KyInst> tab(K);                                 // (alive until the stream has been waited for)
    for (size_t i = 0; i < K; ++i) {
        const accbpg_dopt* h = b->inst[i];
        double* base = buf + i * per;
        double* w = base + qd;
        double* c = w + n + 2 * m;
        tab[i] = KyInst{h->V, h->vws, h->vec_ok ? 1 : 0, B_dev + i * m * m, Q_dev ? Q_dev + i * m * m : base, w, w + n,
                        w + n + m, c, reinterpret_cast<MinMaxRec*>(c + m), picked + i * 2 * m};
    }
    hipStream_t s = b->stream;
    auto run = [&]() -> int {
        ACC_HIP(hipMemcpyAsync(tab_dev, tab.data(), K * sizeof(KyInst), hipMemcpyHostToDevice, s));
        ACC_TRY(ky_enqueue_batch(tab_dev, b->K, h0->m, h0->n, h0->ldv, vt_nsplit(h0->m, h0->n, h0->num_cu), s));
        ACC_HIP(hipMemcpyAsync(picked_host, picked, K * 2 * m * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        return ACCBPG_OK;
    };
    const int rc = run();
    const hipError_t waited = hipStreamSynchronize(s);          // (also behind an error: nothing stays in flight)
    acc_free(buf);
    if (rc != ACCBPG_OK) return rc;
    ACC_HIP(waited);
    return ACCBPG_OK;
}
