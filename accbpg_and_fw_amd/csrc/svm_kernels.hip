// Soft-margin SVM objective f(x) = mean_i max(0, 1 - y_i (A x)_i) + (lamda/2) <x,x> (accbpg/functions.py:161-194) on
// gfx950.
//
// Two passes over the row-major m x n matrix A per func_grad, both HBM-bound, in the forms of poisson_kernels.hip:
//   pass 1  z = A x, one wavefront (or one workgroup for few, long rows) per row, 16-byte loads, with the per-row
//           epilogue of the hinge fused in:
//             marg = y_i*z_i,   t_i = max(0, 1 - marg) (a NaN stays, as np.maximum keeps it),
//             r_i = (marg < 1) ? y_i : 0               (a NaN margin gives 0, as NumPy's < does)
//   pass 2  s = A^T r on the split-row kernel shared with the Frank-Wolfe update (fw_kernels.hip); every row enters,
//           also those with r_i = 0, so 0*NaN propagates as in indicator[:, None] * y[:, None] * A;
//           then g_j = lamda*x_j - s_j/m elementwise: product, quotient, difference, each rounded once.
// The value needs sum_i t_i and <x,x>: both run on the fixed tree of reduce.hpp with the block counts of
// vec_kernels.hip, so <x,x> has the bits of accbpg_vec_dot(x, x); one final launch, one readback of two doubles, and
// the caller forms sum_t/m + lamda/2*xx.  Algorithmic traffic: 2 * 8 * m * n bytes per func_grad, 8*m*n for a
// value-only call.  Compiled with -ffp-contract=off: one rounding per NumPy ufunc, no fused multiply-add unless
// written as fma().
#include "internal.h"
#include "reduce.hpp"

struct accbpg_svm {
    const double* A = nullptr;
    const double* y = nullptr;
    int64_t m = 0, n = 0, lda = 0;
    hipStream_t stream = nullptr;
    int device = 0, num_cu = 256;
    bool vec_ok = false;
    double* Ax = nullptr;      // m
    double* r = nullptr;       // m
    double* t = nullptr;       // m
    double* upart = nullptr;   // VT_MAXSPLIT * n
    double* part = nullptr;    // 2 * SVM_MAXBLK block sums: those of t, then those of x*x
    double* dout = nullptr;    // device scalars {sum t, <x,x>}
    double* hpin = nullptr;    // pinned host scalars
    unsigned hold_lds = 0;     // dynamic-LDS request that holds the A x kernel to two workgroups per CU
};

namespace accbpg {

namespace {

constexpr int SB = 256;            // threads of the A x kernel
constexpr int SR = RED_THREADS;    // threads of the sums and of the elementwise pass
constexpr int SVM_MAXBLK = 1024;   // block cap of the sums (RMAXBLK of vec_kernels.hip)

__device__ __forceinline__ void hinge_epilogue(double z, double yi, int64_t row, double* __restrict__ Ax,
                                               double* __restrict__ r, double* __restrict__ t) {
    const double marg = yi * z;                       // y * np.dot(A, x)          functions.py:171,180
    const double d = 1.0 - marg;
    Ax[row] = z;
    t[row] = (d > 0.0 || d != d) ? d : 0.0;           // np.maximum(0, 1 - marg)
    r[row] = (marg < 1.0) ? yi : 0.0;                 // indicator * y
}

// TPR threads cooperate on one row (64: a wavefront per row, SB: a workgroup per row)
template <int TPR>
__global__ __launch_bounds__(SB) void svm_ax_kernel(const double* __restrict__ A, int64_t lda, int64_t m, int64_t n,
                                                   const double* __restrict__ x, const double* __restrict__ y,
                                                   double* __restrict__ Ax, double* __restrict__ r,
                                                   double* __restrict__ t, bool vec_ok) {
    __shared__ double sh[SB / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int sub = (TPR == 64) ? lane : (int)threadIdx.x;
    const int64_t row = (TPR == 64) ? (int64_t)blockIdx.x * (SB / 64) + w : (int64_t)blockIdx.x;
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
        if (live && lane == 0) hinge_epilogue(s, y[row], row, Ax, r, t);
    } else {
        if (lane == 0) sh[w] = s;
        __syncthreads();
        if (threadIdx.x == 0 && live) {
            double a = 0.0;
            for (int i = 0; i < SB / 64; ++i) a += sh[i];
            hinge_epilogue(a, y[row], row, Ax, r, t);
        }
    }
}

// stage 1 of both sums in one launch: blocks [0, nbt) add t over m entries, blocks [nbt, nbt + nbx) add x*x over n;
// each group partitions its vector as a launch of its own block count would (dot_partial_kernel for x)
__global__ __launch_bounds__(SR) void svm_sums_partial_kernel(const double* __restrict__ t, int64_t m, int nbt,
                                                             const double* __restrict__ x, int64_t n, int nbx,
                                                             double* __restrict__ part) {
    const bool is_t = (int)blockIdx.x < nbt;
    const int blk = is_t ? (int)blockIdx.x : (int)blockIdx.x - nbt;
    const int64_t len = is_t ? m : n;
    const int64_t stride = (int64_t)(is_t ? nbt : nbx) * SR;
    double s = 0.0;
    if (is_t) {
        for (int64_t i = (int64_t)blk * SR + threadIdx.x; i < len; i += stride) s += t[i];
    } else {
        for (int64_t i = (int64_t)blk * SR + threadIdx.x; i < len; i += stride) s += x[i] * x[i];
    }
    double v[1] = {s};
    block_reduce_store<SR, 1, false>(v, part + (is_t ? 0 : SVM_MAXBLK) + blk);
}

// stage 2: workgroup 0 adds the block sums of t in block order into out[0], workgroup 1 those of x*x into out[1]
__global__ __launch_bounds__(SR) void svm_sums_final_kernel(const double* __restrict__ part, int nbt, int nbx,
                                                           double* __restrict__ out) {
    if (blockIdx.x == 0)
        reduce_final_body<SR, 1, false>(part, nbt, out);
    else
        reduce_final_body<SR, 1, false>(part + SVM_MAXBLK, nbx, out + 1);
}

// g = lamda*x - s/m in place of s (functions.py:181,189): np.mean is the sum divided by the count.  x null: g = s/m,
// the subgradient of the loss alone (:181)
__global__ __launch_bounds__(SR) void svm_grad_kernel(double lamda, const double* __restrict__ x, double dm, int64_t n,
                                                     double* __restrict__ g) {
    const int64_t stride = (int64_t)gridDim.x * SR;
    for (int64_t i = (int64_t)blockIdx.x * SR + threadIdx.x; i < n; i += stride) {
        const double q = g[i] / dm;
        if (x == nullptr) {
            g[i] = q;
        } else {
            const double p = lamda * x[i];
            g[i] = p - q;
        }
    }
}

}  // namespace

}  // namespace accbpg

using namespace accbpg;

static int svm_init(accbpg_svm* h) {
    ACC_HIP(hipGetDevice(&h->device));
    hipDeviceProp_t prop;
    ACC_HIP(hipGetDeviceProperties(&prop, h->device));
    h->num_cu = prop.multiProcessorCount;
    // the LDS request of the Poisson A x kernel (poisson_kernels.hip): two workgroups per CU on long rows
    const size_t per_cu = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : 65536;
    size_t hold = per_cu * 3 / 8;
    if (hold > prop.sharedMemPerBlock) hold = prop.sharedMemPerBlock;
    h->hold_lds = (unsigned)(hold & ~(size_t)255);
    h->vec_ok = ((reinterpret_cast<uintptr_t>(h->A) & 15) == 0) && ((h->lda & 1) == 0);
    ACC_HIP(acc_malloc(&h->Ax, sizeof(double) * (size_t)h->m, "svm Ax"));
    ACC_HIP(acc_malloc(&h->r, sizeof(double) * (size_t)h->m, "svm r"));
    ACC_HIP(acc_malloc(&h->t, sizeof(double) * (size_t)h->m, "svm t"));
    ACC_HIP(acc_malloc(&h->upart, sizeof(double) * (size_t)VT_MAXSPLIT * (size_t)h->n, "svm upart"));
    ACC_HIP(acc_malloc(&h->part, sizeof(double) * 2 * SVM_MAXBLK, "svm part"));
    ACC_HIP(acc_malloc(&h->dout, sizeof(double) * 4, "svm dout"));
    ACC_HIP(hipHostMalloc(&h->hpin, sizeof(double) * 4, hipHostMallocDefault));
    return ACCBPG_OK;
}

static void svm_free(accbpg_svm* h) {
    acc_free(h->Ax); acc_free(h->r); acc_free(h->t); acc_free(h->upart); acc_free(h->part); acc_free(h->dout);
    if (h->hpin) hipHostFree(h->hpin);
}

extern "C" int accbpg_svm_create(const double* A_dev, int64_t m, int64_t n, int64_t lda, const double* y_dev,
                                 void* stream, accbpg_svm** out) {
    if (!A_dev || !y_dev || !out || m <= 0 || n <= 0 || lda < n) return ACCBPG_ERR_ARG;
    accbpg_svm* h = new accbpg_svm();
    h->A = A_dev; h->y = y_dev; h->m = m; h->n = n; h->lda = lda;
    h->stream = (hipStream_t)stream;
    const int rc = svm_init(h);
    if (rc != ACCBPG_OK) {                  // nothing of a half-built handle stays behind
        svm_free(h);
        delete h;
        return rc;
    }
    *out = h;
    return ACCBPG_OK;
}

extern "C" int accbpg_svm_destroy(accbpg_svm* h) {
    if (!h) return ACCBPG_OK;
    svm_free(h);
    delete h;
    return ACCBPG_OK;
}

extern "C" int accbpg_svm_set_stream(accbpg_svm* h, void* stream) {
    if (!h) return ACCBPG_ERR_ARG;
    h->stream = (hipStream_t)stream;
    return ACCBPG_OK;
}

extern "C" int accbpg_svm_func_grad(accbpg_svm* h, const double* x_dev, double lamda, int flag, double* f_host,
                                    double* g_dev) {
    if (!h || !x_dev || flag < 0 || flag > 3) return ACCBPG_ERR_ARG;
    const bool want_f = flag == 0 || flag == 2;
    if (want_f && !f_host) return ACCBPG_ERR_ARG;
    if (flag != 0 && (!g_dev || g_dev == x_dev)) return ACCBPG_ERR_ARG;
    hipStream_t s = h->stream;
    const bool xvec = h->vec_ok && ((reinterpret_cast<uintptr_t>(x_dev) & 15) == 0);
    // few long rows: a workgroup per row keeps more of the chip busy than a wavefront per row
    if (h->m < 8 * (int64_t)h->num_cu && h->n >= 4096)
        svm_ax_kernel<SB><<<(unsigned)h->m, SB, 0, s>>>(h->A, h->lda, h->m, h->n, x_dev, h->y, h->Ax, h->r, h->t, xvec);
    else {
        // long rows: two workgroups (eight row streams) per CU, as the Poisson pass does
        const unsigned hold = (h->n >= 32768) ? h->hold_lds : 0;
        svm_ax_kernel<64><<<(unsigned)((h->m + SB / 64 - 1) / (SB / 64)), SB, hold, s>>>(
            h->A, h->lda, h->m, h->n, x_dev, h->y, h->Ax, h->r, h->t, xvec);
    }
    if (want_f) {
        const int nbt = red_blocks(h->m, SVM_MAXBLK), nbx = red_blocks(h->n, SVM_MAXBLK);
        svm_sums_partial_kernel<<<nbt + nbx, SR, 0, s>>>(h->t, h->m, nbt, x_dev, h->n, nbx, h->part);
        svm_sums_final_kernel<<<2, SR, 0, s>>>(h->part, nbt, nbx, h->dout);
    }
    ACC_HIP(hipGetLastError());
    if (flag != 0) {
        ACC_TRY(launch_vt_times(h->A, h->lda, h->m, h->n, h->r, h->upart, vt_nsplit(h->m, h->n, h->num_cu), g_dev,
                                h->vec_ok, s));
        svm_grad_kernel<<<ew_blocks(h->n), SR, 0, s>>>(lamda, flag == 3 ? nullptr : x_dev, (double)h->m, h->n, g_dev);
        ACC_HIP(hipGetLastError());
    }
    if (want_f) {
        ACC_HIP(hipMemcpyAsync(h->hpin, h->dout, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
        ACC_HIP(hipStreamSynchronize(s));
        f_host[0] = h->hpin[0];
        f_host[1] = h->hpin[1];
    }
    return ACCBPG_OK;
}

extern "C" int accbpg_svm_get_ax(accbpg_svm* h, double* out_dev) {
    if (!h || !out_dev) return ACCBPG_ERR_ARG;
    ACC_TRY(device_copy(out_dev, h->Ax, (size_t)h->m, h->stream));
    return ACCBPG_OK;
}
