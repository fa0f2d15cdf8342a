// Length-n kernels of the Shannon-entropy Legendre kernel h(x) = sum x log x on gfx950 (accbpg/functions.py:398-490):
// the closed-form prox maps of ShannonEntropy / ShannonEntropyL1 (one elementwise launch), the simplex-normalised
// prox maps of ShannonEntropySimplex (elementwise pass with per-block sums, then a scaling pass), the divergence and
// the fused line-search terms (<g,x-y>, D(x,y), D(z,z1)) in one streaming pass and one readback.
//
// Every sum is reduced over a fixed tree (a fixed number of blocks, wavefront shuffles, block order), so results
// are reproducible run to run.  The divergence keeps the reference's structure S1 + (Sy - Sx) with its three sums
// reduced separately: late in a run D is ~1e-13 and pure cancellation, and only this structure keeps the result
// inside the reference's own rounding band there.  Compiled with -ffp-contract=off: the reference evaluates these
// expressions with separate NumPy ufuncs (one rounding per operation), so no multiply-add may be fused.
#include "internal.h"
#include "reduce.hpp"

namespace accbpg {

namespace {

constexpr int SB = RED_THREADS;  // threads of the Shannon kernels
constexpr int SNS = 8;           // partial-sum slots per block of the streaming reductions
constexpr int SMAXBLK = 512;     // blocks of a reduction: SNS * SMAXBLK partials fit behind the n doubles of the
                                 // vector workspace (vec_ws_doubles)

// argument of the exponential: the L1 kind adds lamda to g first (functions.py:456-466), then -g/L
__device__ __forceinline__ double neg_g_over_L(int kind, double gi, double L, double lamda) {
    const double gl = (kind == 1) ? lamda + gi : gi;
    return -gl / L;
}

// kind 0 / 1: y == NULL -> exp(-g/L - 1) (ShannonEntropy.prox_map, functions.py:423-429);
//             y != NULL -> y * exp(-g/L) (div_prox_map, :431-438; asserts y >= 0)
__global__ __launch_bounds__(SB) void shannon_prox_kernel(int kind, const double* __restrict__ y,
                                                         const double* __restrict__ g, double L, double lamda,
                                                         int64_t n, double* __restrict__ out, int* __restrict__ flags) {
    const int64_t stride = (int64_t)gridDim.x * SB;
    bool bad_y = false;
    for (int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x; i < n; i += stride) {
        const double q = neg_g_over_L(kind, g[i], L, lamda);
        if (y != nullptr) {
            const double yi = y[i];
            bad_y |= !(yi >= 0.0);
            out[i] = yi * exp(q);
        } else {
            out[i] = exp(q - 1.0);
        }
    }
    if (bad_y) flags[FLAG_NONPOS] = 1;
}

// simplex, pass 1: x = exp(-g/L - 1) or y * exp(-g/L) (functions.py:475-490; the div form asserts y > 0), written to
// out, with the block's partial sum of x in part[blockIdx.x]
__global__ __launch_bounds__(SB) void shannon_simplex_partial_kernel(const double* __restrict__ y,
                                                                    const double* __restrict__ g, double L, int64_t n,
                                                                    double* __restrict__ out,
                                                                    double* __restrict__ part,
                                                                    int* __restrict__ flags) {
    const int64_t stride = (int64_t)gridDim.x * SB;
    bool bad_y = false;
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x; i < n; i += stride) {
        const double q = -g[i] / L;
        double xi;
        if (y != nullptr) {
            const double yi = y[i];
            bad_y |= !(yi > 0.0);
            xi = yi * exp(q);
        } else {
            xi = exp(q - 1.0);
        }
        out[i] = xi;
        s += xi;
    }
    if (bad_y) flags[FLAG_NONPOS] = 1;
    double v[1] = {s};
    block_reduce_store<SB, 1, false>(v, part + blockIdx.x);
}

// sum of the nb partials in a fixed order (every block obtains the same total), broadcast to the block
__device__ __forceinline__ double block_total(const double* __restrict__ part, int nb, double* sh) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += SB) s += part[b];
    s = wave_sum(s);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = s;
    __syncthreads();
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < SB / 64; ++k) a += sh[k];
    return a;
}

// simplex, pass 2: x / sum(x)
__global__ __launch_bounds__(SB) void shannon_simplex_scale_kernel(const double* __restrict__ part, int nb, int64_t n,
                                                                  double* __restrict__ out) {
    __shared__ double sh[SB / 64];
    const double tot = block_total(part, nb, sh);
    const int64_t stride = (int64_t)gridDim.x * SB;
    for (int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x; i < n; i += stride) out[i] = out[i] / tot;
}

// Streaming reduction, stage 1.  Slots of part[blockIdx.x * SNS + k]:
//   0  sum g*(x-y)                           (np.dot(g, x1-x), algorithms.py:53)
//   1  sum x*log((x+delta)/(y+delta))        (functions.py:421)
//   2  sum x          3  sum y
//   4  sum z*log((z+delta)/(z1+delta))
//   5  sum z          6  sum z1
//   7  min over every vector that enters a divergence (x >= 0 and y >= 0, functions.py:418)
__global__ __launch_bounds__(SB) void shannon_ls_partial_kernel(const double* __restrict__ g,
                                                               const double* __restrict__ x,
                                                               const double* __restrict__ y,
                                                               const double* __restrict__ z,
                                                               const double* __restrict__ z1, int64_t n, double delta,
                                                               double* __restrict__ part) {
    double s[SNS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, __builtin_inf()};
    double& mn = s[SNS - 1];
    const int64_t stride = (int64_t)gridDim.x * SB;
    for (int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x; i < n; i += stride) {
        const double xi = x[i], yi = y[i];
        if (g != nullptr) {
            const double d = xi - yi;
            s[0] += g[i] * d;
        }
        {
            const double a = xi + delta;
            const double b = yi + delta;
            const double lg = log(a / b);
            s[1] += xi * lg;
            s[2] += xi;
            s[3] += yi;
            mn = min_nan(mn, min_nan(xi, yi));
        }
        if (z != nullptr) {
            const double zi = z[i], wi = z1[i];
            const double a = zi + delta;
            const double b = wi + delta;
            const double lg = log(a / b);
            s[4] += zi * lg;
            s[5] += zi;
            s[6] += wi;
            mn = min_nan(mn, min_nan(zi, wi));
        }
    }
    block_reduce_store<SB, SNS, true>(s, part + blockIdx.x * SNS);
}

}  // namespace

}  // namespace accbpg

using namespace accbpg;

extern "C" int accbpg_shannon_div_prox(int kind, const double* y_dev, const double* g_dev, double L, double lamda,
                                       int64_t n, double* x_out_dev, double* ws_dev, void* stream) {
    if (!g_dev || !x_out_dev || n <= 0 || kind < 0 || kind > 2) return ACCBPG_ERR_ARG;
    if (kind == 2 && !ws_dev) return ACCBPG_ERR_ARG;
    if (!(L > 0.0)) {                                           // functions.py:428, :437, :483, :489
        set_last_error("ShannonEntropy prox_map require L > 0.");
        return ACCBPG_ERR_ASSERT;
    }
    double* pin = nullptr; int* flags = nullptr; double* dout = nullptr;
    ACC_TRY(vec_scratch(&pin, &flags, &dout));
    hipStream_t s = (hipStream_t)stream;
    ACC_HIP(hipMemsetAsync(flags, 0, 8 * sizeof(int), s));
    if (kind == 2) {
        const int nb = red_blocks(n, SMAXBLK);
        double* part = ws_dev + n;
        shannon_simplex_partial_kernel<<<nb, SB, 0, s>>>(y_dev, g_dev, L, n, x_out_dev, part, flags);
        shannon_simplex_scale_kernel<<<ew_blocks(n), SB, 0, s>>>(part, nb, n, x_out_dev);
    } else {
        shannon_prox_kernel<<<ew_blocks(n), SB, 0, s>>>(kind, y_dev, g_dev, L, lamda, n, x_out_dev, flags);
    }
    ACC_HIP(hipGetLastError());
    int* pin_i = reinterpret_cast<int*>(pin);
    ACC_HIP(hipMemcpyAsync(pin_i, flags, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    ACC_HIP(hipStreamSynchronize(s));
    if (pin_i[FLAG_NONPOS]) {                                   // functions.py:437 / :488
        set_last_error(kind == 2 ? "prox_map needs positive arguments." : "Some entries of y are negavie.");
        return ACCBPG_ERR_ASSERT;
    }
    return ACCBPG_OK;
}

extern "C" int accbpg_shannon_ls_terms(const double* g_dev, const double* x_dev, const double* y_dev,
                                       const double* z_dev, const double* z1_dev, int64_t n, double delta,
                                       double* out_host, double* ws_dev, void* stream) {
    if (!x_dev || !y_dev || n <= 0 || !out_host || !ws_dev) return ACCBPG_ERR_ARG;
    if ((z_dev == nullptr) != (z1_dev == nullptr)) return ACCBPG_ERR_ARG;
    double* pin = nullptr; int* flags = nullptr; double* dout = nullptr;
    ACC_TRY(vec_scratch(&pin, &flags, &dout));
    hipStream_t s = (hipStream_t)stream;
    const int nb = red_blocks(n, SMAXBLK);
    double* part = ws_dev + n;
    shannon_ls_partial_kernel<<<nb, SB, 0, s>>>(g_dev, x_dev, y_dev, z_dev, z1_dev, n, delta, part);
    // stage 2: one workgroup adds the partials of each slot in block order; o[0..7] as the slots
    const double* o = reduce_finish(reduce_final_kernel<SB, SNS, true>, part, nb, dout, dout, SNS, pin, s);
    if (!o) return ACCBPG_ERR_HIP;
    out_host[0] = o[0];
    out_host[1] = o[1] + (o[3] - o[2]);                         // sum(x log(..)) + (sum(y) - sum(x)), functions.py:421
    out_host[2] = o[4] + (o[6] - o[5]);
    if (!(o[7] >= 0.0)) {                                       // functions.py:418
        set_last_error("Some entries are negative.");
        return ACCBPG_ERR_ASSERT;
    }
    return ACCBPG_OK;
}

extern "C" int accbpg_shannon_divergence(const double* x_dev, const double* y_dev, int64_t n, double delta,
                                         double* out_host, double* ws_dev, void* stream) {
    if (!x_dev || !y_dev || !out_host) return ACCBPG_ERR_ARG;
    double o[3] = {0.0, 0.0, 0.0};
    const int rc = accbpg_shannon_ls_terms(nullptr, x_dev, y_dev, nullptr, nullptr, n, delta, o, ws_dev, stream);
    out_host[0] = o[1];
    return rc;
}
