// Symmetric NMF objective f(X) = 0.5*||M - X X^T||_F^2 on gfx950 (FrobeniusSymLoss, accbpg/functions.py:908-976).
// M is n x n symmetric (row-major, leading dimension ldm >= n), X is n x r row-major.
//
// One func_grad is four launches, all on the handle's stream:
//   1  MX = M X on the fp64 MFMA tile engine (mfma_tile.hpp), register-staged and double-buffered.  A workgroup owns a
//      BM = 256-row panel of M and a BN-column block of X; when the panels and column blocks do not fill the chip the
//      k range is split into `nsplit` pieces whose partial products land in separate slabs (no atomics).  BM = 256
//      keeps the bytes of X streamed per workgroup at BN/BM = 1/4 of the bytes of M (a 64-row panel would read as
//      much X as M, and X -- 8 MiB at (16384,64) -- does not fit an XCD's 4 MiB L2).
//   2  S = X^T X (r x r): partial sums over fixed row chunks, then one pass that adds the chunks in order and writes
//      the per-block partials of ||S||_F^2.
//   3  the epilogue over the n x r elements: MX = sum of the slabs in split order; the per-block partials of
//      <X, MX>; and for a gradient G = 2*(X S) - 2*MX, with X S summed over l in order (np.subtract(2*G, 2*XM)).
//   4  one workgroup adds the partials of ||S||^2 and <X, MX> in block order (value only).
// The host then forms f = 0.5*(M_norm^2 + sqrt(||S||^2)^2) - <X, MX> as the reference's frobenius_sym_loss does.
// Every sum runs in a fixed order, so results are reproducible run to run.  Compiled with -ffp-contract=off: the
// epilogue rounds like the NumPy ufunc chain (the MFMA products are unaffected).
#include "internal.h"
#include "mfma_tile.hpp"
#include "reduce.hpp"

#include <math.h>
#include <algorithm>

struct accbpg_symnmf {
    const double* M = nullptr;
    int64_t n = 0, ldm = 0, r = 0;
    double m_norm = 0.0;
    hipStream_t stream = nullptr;
    int num_cu = 256;
    int wide = 0;              // 0: 256 x 64 tile (r <= 64), 1: 256 x 128 tile
    int nsplit = 1;            // k pieces of the product
    int64_t kchunk = 0;        // rows of X per k piece (multiple of BK)
    int gchunks = 1;           // row chunks of S = X^T X
    int cblocks = 1;           // blocks of the epilogue
    int sblocks = 1;           // blocks of the chunk sum of S
    double* P = nullptr;       // nsplit * n * r partial products
    double* S = nullptr;       // r * r
    double* spart = nullptr;   // gchunks * r * r
    double* red = nullptr;     // sblocks + cblocks partials
    double* dout = nullptr;    // 2 device scalars
    double* hpin = nullptr;    // 2 pinned host scalars
};

namespace accbpg {

namespace {

constexpr int YB = 256;              // threads of the non-MFMA kernels
constexpr int Y_MAXSPLIT = 16;
constexpr int Y_MAXCB = 1024;
using TileR64 = Tile<256, 64, 64, 64, true>;
using TileR128 = TileBig<true>;

// block sum in a fixed order (wave shuffles, then the four waves in order); valid in thread 0
__device__ __forceinline__ double y_block_sum(double v, double* sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double a = 0.0;
    if (threadIdx.x == 0) {
        a = sh[0];
        for (int j = 1; j < YB / 64; ++j) a += sh[j];
    }
    __syncthreads();
    return a;
}

// P[split] (n x r) = M[:, kpiece] X[kpiece, :] for the BM x BN tile (blockIdx.x, blockIdx.y) of piece blockIdx.z
template <class T>
__global__ __launch_bounds__(NTHREADS, 1) void symnmf_mx_kernel(const double* __restrict__ M, int64_t ldm,
                                                                const double* __restrict__ X, int64_t n, int64_t r,
                                                                int64_t kchunk, double* __restrict__ P, bool va,
                                                                bool vb) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int64_t row0 = (int64_t)blockIdx.x * T::BM, col0 = (int64_t)blockIdx.y * T::BN;
    const int64_t kb = (int64_t)blockIdx.z * kchunk;
    const int64_t ke = min(n, kb + kchunk);
    T t;
    t.zero();
    const int64_t ksteps = (ke - kb + BK - 1) / BK;
    auto gload = [&](int64_t ks) {
        t.gload_A(M, ldm, row0, n, kb + ks * BK, ke, va);
        t.gload_B_km(X, r, col0, r, kb + ks * BK, ke, vb);
    };
    gload(0);
    t.sstore(lds);
    __syncthreads();
    int cur = 0;
    for (int64_t ks = 0; ks < ksteps; ++ks) {
        const bool more = ks + 1 < ksteps;
        if (more) gload(ks + 1);
        t.compute(lds + cur * T::STAGE_ELEMS);
        if (more) t.sstore(lds + (cur ^ 1) * T::STAGE_ELEMS);
        __syncthreads();
        cur ^= 1;
    }
    t.store_C(P + (int64_t)blockIdx.z * n * r, r, row0, col0, n, r, 1.0, 0.0, false);
}

// spart[c][i*r+j] = sum over the rows of chunk c (in order) of X[k][i] * X[k][j]
__global__ __launch_bounds__(YB) void symnmf_gram_partial_kernel(const double* __restrict__ X, int64_t n, int64_t r,
                                                                 int64_t rows_per, double* __restrict__ spart) {
    const int64_t k0 = (int64_t)blockIdx.y * rows_per;
    const int64_t k1 = min(n, k0 + rows_per);
    const int64_t rr = r * r;
    const int64_t e = (int64_t)blockIdx.x * YB + threadIdx.x;
    if (e >= rr) return;
    const int64_t i = e / r, j = e - i * r;
    double a = 0.0;
    for (int64_t k = k0; k < k1; ++k) a += X[k * r + i] * X[k * r + j];
    spart[(int64_t)blockIdx.y * rr + e] = a;
}

// S = sum of the chunks in chunk order; red[block] = the block's partial of ||S||_F^2
__global__ __launch_bounds__(YB) void symnmf_gram_final_kernel(const double* __restrict__ spart, int nchunks,
                                                               int64_t rr, double* __restrict__ S,
                                                               double* __restrict__ red) {
    __shared__ double sh[YB / 64];
    const int64_t e = (int64_t)blockIdx.x * YB + threadIdx.x;
    double sq = 0.0;
    if (e < rr) {
        double a = spart[e];
        for (int c = 1; c < nchunks; ++c) a += spart[(int64_t)c * rr + e];
        S[e] = a;
        sq = a * a;
    }
    const double b = y_block_sum(sq, sh);
    if (threadIdx.x == 0) red[blockIdx.x] = b;
}

// the epilogue: mx = sum of the nsplit slabs; red[b] = partial of <X, MX>; G = 2*(X S) - 2*mx when G != NULL
__global__ __launch_bounds__(YB) void symnmf_combine_kernel(const double* __restrict__ P, int nsplit,
                                                            const double* __restrict__ X,
                                                            const double* __restrict__ S, int64_t n, int64_t r,
                                                            double* __restrict__ G, double* __restrict__ red) {
    __shared__ double sh[YB / 64];
    const int64_t total = n * r;
    const int64_t stride = (int64_t)gridDim.x * YB;
    double d = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * YB + threadIdx.x; e < total; e += stride) {
        double mx = P[e];
        for (int s = 1; s < nsplit; ++s) mx += P[(int64_t)s * total + e];
        d += X[e] * mx;
        if (G != nullptr) {
            const int64_t i = e / r, j = e - i * r;
            const double* xr = X + i * r;
            double xs = 0.0;
            for (int64_t l = 0; l < r; ++l) xs += xr[l] * S[l * r + j];
            const double a = 2.0 * xs;
            const double b = 2.0 * mx;
            G[e] = a - b;
        }
    }
    const double b = y_block_sum(d, sh);
    if (threadIdx.x == 0) red[blockIdx.x] = b;
}

// out[0] = ||S||_F^2 (sum of the first ns partials in order), out[1] = <X, MX> (the next nc, in order)
__global__ __launch_bounds__(YB) void symnmf_scalars_kernel(const double* __restrict__ red, int ns, int nc,
                                                            double* __restrict__ out) {
    __shared__ double sh[YB / 64];
    double a = 0.0, b = 0.0;
    for (int k = threadIdx.x; k < ns; k += YB) a += red[k];
    for (int k = threadIdx.x; k < nc; k += YB) b += red[ns + k];
    a = y_block_sum(a, sh);
    b = y_block_sum(b, sh);
    if (threadIdx.x == 0) {
        out[0] = a;
        out[1] = b;
    }
}

template <class T>
int launch_mx(accbpg_symnmf* h, const double* X, hipStream_t s) {
    int dev = 0;
    ACC_HIP(hipGetDevice(&dev));
    const bool va = ((reinterpret_cast<uintptr_t>(h->M) & 15) == 0) && ((h->ldm & 1) == 0);
    const bool vb = ((reinterpret_cast<uintptr_t>(X) & 15) == 0) && ((h->r & 1) == 0);
    dim3 grid((unsigned)((h->n + T::BM - 1) / T::BM), (unsigned)((h->r + T::BN - 1) / T::BN), (unsigned)h->nsplit);
    ACC_LAUNCH_LDS(dev, symnmf_mx_kernel<T>, grid, NTHREADS, T::LDS_BYTES, s, h->M,h->ldm, X, h->n, h->r, h->kchunk, h->P, va, vb);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

// the launch plan depends on (n, r) and the number of compute units only
void symnmf_plan(accbpg_symnmf* h) {
    const int64_t n = h->n, r = h->r;
    h->wide = r > 64 ? 1 : 0;
    const int64_t bm = 256, bn = h->wide ? 128 : 64;
    const int64_t tiles = ((n + bm - 1) / bm) * ((r + bn - 1) / bn);
    const int64_t ksteps = (n + BK - 1) / BK;
    int64_t ns = (h->num_cu + tiles - 1) / tiles;                 // fill the chip ...
    ns = std::min<int64_t>(ns, std::max<int64_t>(1, ksteps / 16)); // ... with pieces at least 256 deep
    ns = std::min<int64_t>(ns, Y_MAXSPLIT);
    if (ns < 1) ns = 1;
    h->kchunk = ((ksteps + ns - 1) / ns) * BK;
    h->nsplit = (int)((n + h->kchunk - 1) / h->kchunk);
    h->gchunks = (int)std::min<int64_t>(h->num_cu, std::max<int64_t>(1, (n + 63) / 64));
    h->sblocks = (int)((r * r + YB - 1) / YB);
    h->cblocks = (int)std::min<int64_t>(Y_MAXCB, (n * r + YB - 1) / YB);
}

}  // namespace

}  // namespace accbpg

using namespace accbpg;

static void symnmf_free(accbpg_symnmf* h) {
    acc_free(h->P); acc_free(h->S); acc_free(h->spart); acc_free(h->red); acc_free(h->dout);
    if (h->hpin) hipHostFree(h->hpin);
}

extern "C" int accbpg_symnmf_create(const double* M_dev, int64_t n, int64_t ldm, int64_t r, double m_norm,
                                    void* stream, accbpg_symnmf** out) {
    if (!M_dev || !out || n <= 0 || r <= 0 || ldm < n) return ACCBPG_ERR_ARG;
    accbpg_symnmf* h = new accbpg_symnmf();
    h->M = M_dev; h->n = n; h->ldm = ldm; h->r = r; h->m_norm = m_norm;
    h->stream = (hipStream_t)stream;
    int rc = ACCBPG_OK;
    do {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) { rc = ACCBPG_ERR_HIP; break; }
        h->num_cu = prop.multiProcessorCount;
        symnmf_plan(h);
        const size_t nr = (size_t)n * (size_t)r, rr = (size_t)r * (size_t)r;
        if (acc_malloc(&h->P, sizeof(double) * nr * (size_t)h->nsplit, "P") != hipSuccess ||
            acc_malloc(&h->S, sizeof(double) * rr, "S") != hipSuccess ||
            acc_malloc(&h->spart, sizeof(double) * rr * (size_t)h->gchunks, "spart") != hipSuccess ||
            acc_malloc(&h->red, sizeof(double) * (size_t)(h->sblocks + h->cblocks), "red") != hipSuccess ||
            acc_malloc(&h->dout, sizeof(double) * 2, "dout") != hipSuccess ||
            hipHostMalloc(&h->hpin, sizeof(double) * 2, hipHostMallocDefault) != hipSuccess) {
            set_last_error("accbpg_symnmf_create: out of memory");
            rc = ACCBPG_ERR_HIP;
        }
    } while (0);
    if (rc != ACCBPG_OK) {                  // nothing of a half-built handle stays behind
        symnmf_free(h);
        delete h;
        return rc;
    }
    *out = h;
    return ACCBPG_OK;
}

extern "C" int accbpg_symnmf_destroy(accbpg_symnmf* h) {
    if (!h) return ACCBPG_OK;
    symnmf_free(h);
    delete h;
    return ACCBPG_OK;
}

extern "C" int accbpg_symnmf_set_stream(accbpg_symnmf* h, void* stream) {
    if (!h) return ACCBPG_ERR_ARG;
    h->stream = (hipStream_t)stream;
    return ACCBPG_OK;
}

extern "C" int accbpg_symnmf_func_grad(accbpg_symnmf* h, const double* X_dev, int flag, double* f_host,
                                       double* g_dev) {
    if (!h || !X_dev || flag < 0 || flag > 2) return ACCBPG_ERR_ARG;
    if (flag != 1 && !f_host) return ACCBPG_ERR_ARG;
    if (flag != 0 && !g_dev) return ACCBPG_ERR_ARG;
    hipStream_t s = h->stream;
    if (h->wide)
        ACC_TRY(launch_mx<TileR128>(h, X_dev, s));
    else
        ACC_TRY(launch_mx<TileR64>(h, X_dev, s));
    const int64_t rr = h->r * h->r;
    const int64_t rows_per = (h->n + h->gchunks - 1) / h->gchunks;
    symnmf_gram_partial_kernel<<<dim3((unsigned)h->sblocks, (unsigned)h->gchunks), YB, 0, s>>>(X_dev, h->n, h->r,
                                                                                               rows_per, h->spart);
    symnmf_gram_final_kernel<<<h->sblocks, YB, 0, s>>>(h->spart, h->gchunks, rr, h->S, h->red);
    symnmf_combine_kernel<<<h->cblocks, YB, 0, s>>>(h->P, h->nsplit, X_dev, h->S, h->n, h->r,
                                                    flag != 0 ? g_dev : nullptr, h->red + h->sblocks);
    ACC_HIP(hipGetLastError());
    if (flag != 1) {
        symnmf_scalars_kernel<<<1, YB, 0, s>>>(h->red, h->sblocks, h->cblocks, h->dout);
        ACC_HIP(hipGetLastError());
        ACC_HIP(hipMemcpyAsync(h->hpin, h->dout, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
        ACC_HIP(hipStreamSynchronize(s));
        // t1 = 0.5*(M_norm**2 + norm(X.T @ X)**2); f = t1 - <X, MX>  (functions.py:936-938)
        const double sn = sqrt(h->hpin[0]);
        const double t1 = 0.5 * (h->m_norm * h->m_norm + sn * sn);
        f_host[0] = t1 - h->hpin[1];
    }
    return ACCBPG_OK;
}

/* launch plan of a handle: {nsplit, kchunk, wide, gchunks} (tests and the rate tool) */
extern "C" int accbpg_symnmf_plan(accbpg_symnmf* h, int64_t* out4) {
    if (!h || !out4) return ACCBPG_ERR_ARG;
    out4[0] = h->nsplit; out4[1] = h->kchunk; out4[2] = h->wide; out4[3] = h->gchunks;
    return ACCBPG_OK;
}
