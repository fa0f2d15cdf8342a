// Logistic regression f(x) = (1/m) sum_i log(1 + exp(-y_i (A x)_i)) (accbpg/ex_LR_L2L1Linf.py:19-54, the class
// LogisticRegression of accbpg/functions.py:1068-1104) on gfx950.
//
// Two passes over the row-major m x n matrix A per func_grad, both HBM-bound, in the forms of svm_kernels.hip:
//   pass 1  z = A x, one wavefront (or one workgroup for few, long rows) per row, 16-byte loads, with the per-row
//           epilogue of the logistic loss fused in, one rounding per operation:
//             s = y_i*z,   a = |s|,   e = exp(-a)                       (e in [0, 1]: nothing overflows)
//             t_i = max(-s, 0) + log1p(e)                               = log(1 + exp(-s)) without cancellation
//             q   = (s >= 0) ? e/(1 + e) : 1/(1 + e)                    = sigma(-s)
//             r_i = -(y_i*q)
//           A NaN s gives NaN t_i and r_i; s = +inf gives t = 0, q = 0; s = -inf gives t = +inf, q = 1; |s| > 745
//           underflows e to 0 and the formulas give t = max(-s, 0), q = 0 or 1 by themselves.
//   pass 2  s = A^T r on the split-row kernel shared with the Frank-Wolfe update (fw_kernels.hip); every row enters,
//           so 0*NaN propagates; then g_j = s_j/m elementwise.
// The value needs sum_i t_i: it runs on the fixed tree of reduce.hpp with the block cap of vec_kernels.hip; one final
// launch, one readback of one double, and the caller forms sum_t/m.  Algorithmic traffic: 2 * 8 * m * n bytes per
// func_grad, 8*m*n for a value-only call.
// Along a segment x + a d the margins are z + a (A d): accbpg_logistic_line_begin keeps w = A d (pass 1 with a plain
// store), after which a value at any a (line_value) and the rows of the accepted point (line_accept) cost O(m) from
// fma(a, w_i, z_i), and func_grad_carried returns the value and A^T r / m of the rows the handle holds.
// Compiled with -ffp-contract=off: one rounding per operation, no fused
// multiply-add unless written as fma().
#include "internal.h"
#include "reduce.hpp"

struct accbpg_logistic {
    const double* A = nullptr;
    const double* y = nullptr;
    int64_t m = 0, n = 0, lda = 0;
    hipStream_t stream = nullptr;
    int device = 0, num_cu = 256;
    bool vec_ok = false;
    double* Ax = nullptr;      // m
    double* t = nullptr;       // m
    double* r = nullptr;       // m
    double* upart = nullptr;   // VT_MAXSPLIT * n
    double* part = nullptr;    // LG_MAXBLK block sums of t
    double* dout = nullptr;    // device scalar {sum t}
    double* hpin = nullptr;    // pinned host scalar
    double* w = nullptr;       // m: A d of the segment x + a d (accbpg_logistic_line_begin)
    bool z_cur = false;        // Ax, t, r are those of the caller's current point
    bool w_cur = false;        // w belongs to those margins
    unsigned hold_lds = 0;     // dynamic-LDS request that holds the A x kernel to two workgroups per CU
};

namespace accbpg {

namespace {

constexpr int LB = 256;            // threads of the A x kernel
constexpr int LR = RED_THREADS;    // threads of the sum and of the elementwise pass
constexpr int LG_MAXBLK = 1024;    // block cap of the sum (RMAXBLK of vec_kernels.hip)

// the terms of one row from its z = (A x)_i: t_i and r_i
__device__ __forceinline__ void logistic_terms(double z, double yi, double& ti, double& ri) {
    const double s = yi * z;
    const double a = fabs(s);
    const double e = exp(-a);
    const double ns = -s;
    const double hi = (ns > 0.0) ? ns : 0.0;          // a NaN s: 0 here, the NaN comes in with log1p(e)
    const double den = 1.0 + e;
    const double q = (s >= 0.0) ? e / den : 1.0 / den;
    const double yq = yi * q;
    ti = hi + log1p(e);
    ri = -yq;
}

__device__ __forceinline__ void logistic_epilogue(double z, double yi, int64_t row, double* __restrict__ Ax,
                                                  double* __restrict__ t, double* __restrict__ r) {
    double ti, ri;
    logistic_terms(z, yi, ti, ri);
    Ax[row] = z;
    t[row] = ti;
    r[row] = ri;
}

// TPR threads cooperate on one row (64: a wavefront per row, LB: a workgroup per row).  PLAIN: the row sum is stored to
// Ax and nothing else is touched (w = A d of accbpg_logistic_line_begin; y, t and r are not read or written).
template <int TPR, bool PLAIN = false>
__global__ __launch_bounds__(LB) void logistic_ax_kernel(const double* __restrict__ A, int64_t lda, int64_t m,
                                                        int64_t n, const double* __restrict__ x,
                                                        const double* __restrict__ y, double* __restrict__ Ax,
                                                        double* __restrict__ t, double* __restrict__ r, bool vec_ok) {
    __shared__ double sh[LB / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int sub = (TPR == 64) ? lane : (int)threadIdx.x;
    const int64_t row = (TPR == 64) ? (int64_t)blockIdx.x * (LB / 64) + w : (int64_t)blockIdx.x;
    const bool live = row < m;
    double s0 = 0.0, s1 = 0.0;
    if (live) {
        const double* ar = A + row * lda;
        if (vec_ok) {
            const int64_t n2 = n >> 1;
            const double2* a2 = reinterpret_cast<const double2*>(ar);
            const double2* x2 = reinterpret_cast<const double2*>(x);
#pragma unroll 4
            for (int64_t c = sub; c < n2; c += TPR) {
                // A is streamed once per pass: non-temporal loads keep it out of the caches (x stays cached)
                const double* ap = reinterpret_cast<const double*>(a2 + c);
                const double2 av = double2{__builtin_nontemporal_load(ap), __builtin_nontemporal_load(ap + 1)};
                const double2 xv = x2[c];
                s0 = fma(av.x, xv.x, s0);
                s1 = fma(av.y, xv.y, s1);
            }
            if ((n & 1) && sub == 0) s0 = fma(ar[n - 1], x[n - 1], s0);
        } else {
            for (int64_t c = sub; c < n; c += TPR) s0 = fma(ar[c], x[c], s0);
        }
    }
    double s = wave_sum(s0 + s1);
    if (TPR == 64) {
        if (live && lane == 0) {
            if constexpr (PLAIN) Ax[row] = s;
            else logistic_epilogue(s, y[row], row, Ax, t, r);
        }
    } else {
        if (lane == 0) sh[w] = s;
        __syncthreads();
        if (threadIdx.x == 0 && live) {
            double a = 0.0;
            for (int i = 0; i < LB / 64; ++i) a += sh[i];
            if constexpr (PLAIN) Ax[row] = a;
            else logistic_epilogue(a, y[row], row, Ax, t, r);
        }
    }
}

// stage 1 of sum t: block b adds the entries b*LR + thread + k*gridDim.x*LR in that order
__global__ __launch_bounds__(LR) void logistic_sum_partial_kernel(const double* __restrict__ t, int64_t m,
                                                                 double* __restrict__ part) {
    double s = 0.0;
    const int64_t stride = (int64_t)gridDim.x * LR;
    for (int64_t i = (int64_t)blockIdx.x * LR + threadIdx.x; i < m; i += stride) s += t[i];
    double v[1] = {s};
    block_reduce_store<LR, 1, false>(v, part + blockIdx.x);
}

// stage 1 of the value at x + a d: the t of fma(a, w_i, z_i) in the place of t_i, the same entries in the same order;
// nothing is stored but the block sum
__global__ __launch_bounds__(LR) void logistic_line_sum_partial_kernel(const double* __restrict__ z,
                                                                      const double* __restrict__ w,
                                                                      const double* __restrict__ y, double a, int64_t m,
                                                                      double* __restrict__ part) {
    double s = 0.0;
    const int64_t stride = (int64_t)gridDim.x * LR;
    for (int64_t i = (int64_t)blockIdx.x * LR + threadIdx.x; i < m; i += stride) {
        double ti, ri;
        logistic_terms(fma(a, w[i], z[i]), y[i], ti, ri);
        s += ti;
    }
    double v[1] = {s};
    block_reduce_store<LR, 1, false>(v, part + blockIdx.x);
}

// the accepted step: z_i <- fma(a, w_i, z_i) with its t_i and r_i
__global__ __launch_bounds__(LR) void logistic_line_accept_kernel(const double* __restrict__ w,
                                                                 const double* __restrict__ y, double a, int64_t m,
                                                                 double* __restrict__ Ax, double* __restrict__ t,
                                                                 double* __restrict__ r) {
    const int64_t stride = (int64_t)gridDim.x * LR;
    for (int64_t i = (int64_t)blockIdx.x * LR + threadIdx.x; i < m; i += stride)
        logistic_epilogue(fma(a, w[i], Ax[i]), y[i], i, Ax, t, r);
}

// stage 2: one workgroup adds the block sums in block order
__global__ __launch_bounds__(LR) void logistic_sum_final_kernel(const double* __restrict__ part, int nb,
                                                               double* __restrict__ out) {
    reduce_final_body<LR, 1, false>(part, nb, out);
}

// g = s/m in place of s: np.mean is the sum divided by the count
__global__ __launch_bounds__(LR) void logistic_grad_kernel(double dm, int64_t n, double* __restrict__ g) {
    const int64_t stride = (int64_t)gridDim.x * LR;
    for (int64_t i = (int64_t)blockIdx.x * LR + threadIdx.x; i < n; i += stride) g[i] = g[i] / dm;
}

}  // namespace

}  // namespace accbpg

using namespace accbpg;

static int logistic_init(accbpg_logistic* h) {
    ACC_HIP(hipGetDevice(&h->device));
    hipDeviceProp_t prop;
    ACC_HIP(hipGetDeviceProperties(&prop, h->device));
    h->num_cu = prop.multiProcessorCount;
    // the LDS request of the Poisson and SVM A x kernels: two workgroups per CU on long rows
    const size_t per_cu = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : 65536;
    size_t hold = per_cu * 3 / 8;
    if (hold > prop.sharedMemPerBlock) hold = prop.sharedMemPerBlock;
    h->hold_lds = (unsigned)(hold & ~(size_t)255);
    h->vec_ok = ((reinterpret_cast<uintptr_t>(h->A) & 15) == 0) && ((h->lda & 1) == 0);
    ACC_HIP(acc_malloc(&h->Ax, sizeof(double) * (size_t)h->m, "logistic Ax"));
    ACC_HIP(acc_malloc(&h->t, sizeof(double) * (size_t)h->m, "logistic t"));
    ACC_HIP(acc_malloc(&h->r, sizeof(double) * (size_t)h->m, "logistic r"));
    ACC_HIP(acc_malloc(&h->w, sizeof(double) * (size_t)h->m, "logistic w"));
    ACC_HIP(acc_malloc(&h->upart, sizeof(double) * (size_t)VT_MAXSPLIT * (size_t)h->n, "logistic upart"));
    ACC_HIP(acc_malloc(&h->part, sizeof(double) * LG_MAXBLK, "logistic part"));
    ACC_HIP(acc_malloc(&h->dout, sizeof(double) * 4, "logistic dout"));
    ACC_HIP(hipHostMalloc(&h->hpin, sizeof(double) * 4, hipHostMallocDefault));
    return ACCBPG_OK;
}

static void logistic_free(accbpg_logistic* h) {
    acc_free(h->Ax); acc_free(h->t); acc_free(h->r); acc_free(h->w); acc_free(h->upart); acc_free(h->part); acc_free(h->dout);
    if (h->hpin) hipHostFree(h->hpin);
}

extern "C" int accbpg_logistic_create(const double* A_dev, int64_t m, int64_t n, int64_t lda, const double* y_dev,
                                      void* stream, accbpg_logistic** out) {
    if (!A_dev || !y_dev || !out || m <= 0 || n <= 0 || lda < n) return ACCBPG_ERR_ARG;
    accbpg_logistic* h = new accbpg_logistic();
    h->A = A_dev; h->y = y_dev; h->m = m; h->n = n; h->lda = lda;
    h->stream = (hipStream_t)stream;
    const int rc = logistic_init(h);
    if (rc != ACCBPG_OK) {                  // nothing of a half-built handle stays behind
        logistic_free(h);
        delete h;
        return rc;
    }
    *out = h;
    return ACCBPG_OK;
}

extern "C" int accbpg_logistic_destroy(accbpg_logistic* h) {
    if (!h) return ACCBPG_OK;
    logistic_free(h);
    delete h;
    return ACCBPG_OK;
}

extern "C" int accbpg_logistic_set_stream(accbpg_logistic* h, void* stream) {
    if (!h) return ACCBPG_ERR_ARG;
    h->stream = (hipStream_t)stream;
    return ACCBPG_OK;
}

// pass 1 at v in the launch form of the shape: z = A v with the logistic epilogue, or (PLAIN) the plain store to `out`
template <bool PLAIN>
static int logistic_launch_ax(accbpg_logistic* h, const double* v_dev, double* out) {
    hipStream_t s = h->stream;
    const bool xvec = h->vec_ok && ((reinterpret_cast<uintptr_t>(v_dev) & 15) == 0);
    // few long rows: a workgroup per row keeps more of the chip busy than a wavefront per row
    if (h->m < 8 * (int64_t)h->num_cu && h->n >= 4096)
        logistic_ax_kernel<LB, PLAIN><<<(unsigned)h->m, LB, 0, s>>>(h->A, h->lda, h->m, h->n, v_dev, h->y, out, h->t,
                                                                    h->r, xvec);
    else {
        // long rows: two workgroups (eight row streams) per CU, as the Poisson and SVM passes do
        const unsigned hold = (h->n >= 32768) ? h->hold_lds : 0;
        logistic_ax_kernel<64, PLAIN><<<(unsigned)((h->m + LB / 64 - 1) / (LB / 64)), LB, hold, s>>>(
            h->A, h->lda, h->m, h->n, v_dev, h->y, out, h->t, h->r, xvec);
    }
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

// the final stage of a value over nb block sums, and A^T r / m: what follows pass 1 in every entry that returns them
static int logistic_tail(accbpg_logistic* h, int nb, bool want_f, bool want_g, double* f_host, double* g_dev) {
    hipStream_t s = h->stream;
    if (want_f) {
        logistic_sum_final_kernel<<<1, LR, 0, s>>>(h->part, nb, h->dout);
        ACC_HIP(hipGetLastError());
    }
    if (want_g) {
        ACC_TRY(launch_vt_times(h->A, h->lda, h->m, h->n, h->r, h->upart, vt_nsplit(h->m, h->n, h->num_cu), g_dev,
                                h->vec_ok, s));
        logistic_grad_kernel<<<ew_blocks(h->n), LR, 0, s>>>((double)h->m, h->n, g_dev);
        ACC_HIP(hipGetLastError());
    }
    if (want_f) {
        ACC_HIP(hipMemcpyAsync(h->hpin, h->dout, sizeof(double), hipMemcpyDeviceToHost, s));
        ACC_HIP(hipStreamSynchronize(s));
        f_host[0] = h->hpin[0];
    }
    return ACCBPG_OK;
}

static int logistic_check_flag(const accbpg_logistic* h, int flag, const double* f_host, const double* g_dev) {
    if (!h || flag < 0 || flag > 2) return ACCBPG_ERR_ARG;
    if (flag != 1 && !f_host) return ACCBPG_ERR_ARG;
    if (flag != 0 && !g_dev) return ACCBPG_ERR_ARG;
    return ACCBPG_OK;
}

extern "C" int accbpg_logistic_func_grad(accbpg_logistic* h, const double* x_dev, int flag, double* f_host,
                                         double* g_dev) {
    if (!x_dev) return ACCBPG_ERR_ARG;
    ACC_TRY(logistic_check_flag(h, flag, f_host, g_dev));
    if (flag != 0 && g_dev == x_dev) return ACCBPG_ERR_ARG;
    const bool want_f = flag != 1;
    h->z_cur = false; h->w_cur = false;                       // (a failed launch leaves nothing to carry)
    ACC_TRY(logistic_launch_ax<false>(h, x_dev, h->Ax));
    const int nb = red_blocks(h->m, LG_MAXBLK);
    if (want_f) {
        logistic_sum_partial_kernel<<<nb, LR, 0, h->stream>>>(h->t, h->m, h->part);
        ACC_HIP(hipGetLastError());
    }
    ACC_TRY(logistic_tail(h, nb, want_f, flag != 0, f_host, g_dev));
    h->z_cur = true;                                          // the margins are those of x_dev from here on
    return ACCBPG_OK;
}

static int logistic_stale(const char* what) {
    set_last_error(what);
    return ACCBPG_ERR_ARG;
}

extern "C" int accbpg_logistic_line_begin(accbpg_logistic* h, const double* d_dev) {
    if (!h || !d_dev) return ACCBPG_ERR_ARG;
    if (!h->z_cur) return logistic_stale("accbpg_logistic_line_begin: no func_grad has set the margins");
    h->w_cur = false;
    ACC_TRY(logistic_launch_ax<true>(h, d_dev, h->w));
    h->w_cur = true;
    return ACCBPG_OK;
}

extern "C" int accbpg_logistic_line_value(accbpg_logistic* h, double a, double* f_host) {
    if (!h || !f_host) return ACCBPG_ERR_ARG;
    if (!h->z_cur || !h->w_cur) return logistic_stale("accbpg_logistic_line_value: no line has begun at these margins");
    const int nb = red_blocks(h->m, LG_MAXBLK);
    logistic_line_sum_partial_kernel<<<nb, LR, 0, h->stream>>>(h->Ax, h->w, h->y, a, h->m, h->part);
    ACC_HIP(hipGetLastError());
    return logistic_tail(h, nb, true, false, f_host, nullptr);
}

extern "C" int accbpg_logistic_line_accept(accbpg_logistic* h, double a) {
    if (!h) return ACCBPG_ERR_ARG;
    if (!h->z_cur || !h->w_cur) return logistic_stale("accbpg_logistic_line_accept: no line has begun at these margins");
    h->w_cur = false;                                         // the next direction starts from the new margins
    logistic_line_accept_kernel<<<ew_blocks(h->m), LR, 0, h->stream>>>(h->w, h->y, a, h->m, h->Ax, h->t, h->r);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

extern "C" int accbpg_logistic_func_grad_carried(accbpg_logistic* h, int flag, double* f_host, double* g_dev) {
    ACC_TRY(logistic_check_flag(h, flag, f_host, g_dev));
    if (!h->z_cur) return logistic_stale("accbpg_logistic_func_grad_carried: no func_grad has set the margins");
    const bool want_f = flag != 1;
    const int nb = red_blocks(h->m, LG_MAXBLK);
    if (want_f) {
        logistic_sum_partial_kernel<<<nb, LR, 0, h->stream>>>(h->t, h->m, h->part);
        ACC_HIP(hipGetLastError());
    }
    return logistic_tail(h, nb, want_f, flag != 0, f_host, g_dev);
}

extern "C" int accbpg_logistic_get(accbpg_logistic* h, int which, double* out_dev) {
    if (!h || !out_dev || which < 0 || which > 2) return ACCBPG_ERR_ARG;
    const double* src = which == 0 ? h->Ax : (which == 1 ? h->t : h->r);
    ACC_TRY(device_copy(out_dev, src, (size_t)h->m, h->stream));
    return ACCBPG_OK;
}
