// Length-n kernels of the quartic Legendre kernel h(x) = (sigma/2)||x||^2 + (alpha/4)||x||^4 (SumOf2nd4thPowers and
// SumOf2nd4thPowersPositiveOrthant, accbpg/functions.py:493-577) and the Frank-Wolfe linear minimisation oracles of
// the l2 and l-infinity balls (accbpg/functions_lmo.py:16-51, 106-134), on gfx950.  Vectors are flat views of any
// shape (n x r iterates included).
//
//   prox stage   y' = z*y - (1/L)*g, optionally clipped to [0, ub], written out together with ||y'||^2: the host then
//                solves the cubic of div_prox_map in float64 and scales by 1/z' (accbpg_vec_div_scalar);
//   ls terms     (<g,x-y>, ||x||^2, ||y||^2, <y,x-y>, ||z||^2, ||z1||^2, <z1,z-z1>) in one streaming pass and one
//                readback: D(x,y) = h(x) - (h(y) + c_y <y, x-y>) with c_y = sigma + alpha ||y||^2 on the host;
//   lmo l2       s = c - (R*g)/||g||, with ||s - c||^2 of the same launch for the boundary assertion;
//   lmo linf     s = c - R*sign(g), sign(0) = 0.
// Every sum is reduced over a fixed tree (a fixed number of blocks, wavefront shuffles, block order), so results are
// reproducible run to run.  Compiled with -ffp-contract=off: one rounding per NumPy ufunc, no fused multiply-add.
#include "internal.h"
#include "reduce.hpp"

namespace accbpg {

namespace {

constexpr int QK = RED_THREADS;  // threads per block
constexpr int QNS = 8;           // partial-sum slots per block
constexpr int QMAXBLK = 512;     // QNS * QMAXBLK partials fit behind the n doubles of the vector workspace

// the QNS sums of a block to part[block*QNS + k]
__device__ __forceinline__ void q_block_store(double (&s)[QNS], double* __restrict__ part) {
    block_reduce_store<QK, QNS, false>(s, part + blockIdx.x * QNS);
}

// y' = z*y - invL*g (functions.py:553-554), clipped to [0, ub] when clip (np.clip(y, 0, upper_bound), :573);
// slot 0 = sum y'^2
__global__ __launch_bounds__(QK) void quartic_prox_kernel(const double* __restrict__ y, const double* __restrict__ g,
                                                          double z, double invL, int clip, double ub, int64_t n,
                                                          double* __restrict__ out, double* __restrict__ part) {
    double s[QNS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * QK;
    for (int64_t i = (int64_t)blockIdx.x * QK + threadIdx.x; i < n; i += stride) {
        const double a = z * y[i];
        const double b = invL * g[i];
        double v = a - b;
        if (clip) {
            v = (v < 0.0) ? 0.0 : v;            // NaN passes through, as in np.clip
            v = (v > ub) ? ub : v;
        }
        out[i] = v;
        s[0] += v * v;
    }
    q_block_store(s, part);
}

// slots: 0 <g,x-y>, 1 ||x||^2, 2 ||y||^2, 3 <y,x-y>, 4 ||z||^2, 5 ||z1||^2, 6 <z1,z-z1>
__global__ __launch_bounds__(QK) void quartic_ls_kernel(const double* __restrict__ g, const double* __restrict__ x,
                                                        const double* __restrict__ y, const double* __restrict__ z,
                                                        const double* __restrict__ z1, int64_t n,
                                                        double* __restrict__ part) {
    double s[QNS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * QK;
    for (int64_t i = (int64_t)blockIdx.x * QK + threadIdx.x; i < n; i += stride) {
        const double xi = x[i], yi = y[i];
        const double d = xi - yi;
        if (g != nullptr) s[0] += g[i] * d;
        s[1] += xi * xi;
        s[2] += yi * yi;
        s[3] += yi * d;
        if (z != nullptr) {
            const double zi = z[i], wi = z1[i];
            s[4] += zi * zi;
            s[5] += wi * wi;
            s[6] += wi * (zi - wi);
        }
    }
    q_block_store(s, part);
}

// centre of a ball: kind 0 = the scalar cval (0 for no centre), kind 1 = the array c (same shape as g)
__device__ __forceinline__ double q_center(int kind, const double* __restrict__ c, double cval, int64_t i) {
    return kind == 1 ? c[i] : cval;
}

// s = c - (R*g)/gnorm (functions_lmo.py:43); slot 0 = sum (s - c)^2 (:45)
__global__ __launch_bounds__(QK) void lmo_l2_kernel(const double* __restrict__ g, int kind,
                                                    const double* __restrict__ c, double cval, double radius,
                                                    double gnorm, int64_t n, double* __restrict__ out,
                                                    double* __restrict__ part) {
    double s[QNS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * QK;
    for (int64_t i = (int64_t)blockIdx.x * QK + threadIdx.x; i < n; i += stride) {
        const double ci = q_center(kind, c, cval, i);
        const double t = (radius * g[i]) / gnorm;
        const double si = ci - t;
        out[i] = si;
        const double d = si - ci;
        s[0] += d * d;
    }
    q_block_store(s, part);
}

// s = c - R*sign(g) (functions_lmo.py:131); np.sign: 0 for 0, NaN for NaN
__global__ __launch_bounds__(QK) void lmo_linf_kernel(const double* __restrict__ g, int kind,
                                                      const double* __restrict__ c, double cval, double radius,
                                                      int64_t n, double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * QK;
    for (int64_t i = (int64_t)blockIdx.x * QK + threadIdx.x; i < n; i += stride) {
        const double gi = g[i];
        const double sg = gi > 0.0 ? 1.0 : (gi < 0.0 ? -1.0 : gi);   // +-0 stays +-0 (R*(-0) then c - (-0) = c)
        out[i] = q_center(kind, c, cval, i) - radius * sg;
    }
}

// the partials of each slot added in block order and read back: *o = the QNS slots on the host
int q_finish(const double* part, int nb, hipStream_t s, const double** o) {
    double* pin = nullptr; int* flags = nullptr; double* dout = nullptr;
    ACC_TRY(vec_scratch(&pin, &flags, &dout));
    *o = reduce_finish(reduce_final_kernel<QK, QNS, false>, part, nb, dout, dout, QNS, pin, s);
    return *o ? ACCBPG_OK : ACCBPG_ERR_HIP;
}

}  // namespace

}  // namespace accbpg

using namespace accbpg;

extern "C" int accbpg_quartic_prox_stage(const double* y_dev, const double* g_dev, double z, double invL, int clip,
                                         double upper_bound, int64_t n, double* out_dev, double* ssq_host,
                                         double* ws_dev, void* stream) {
    if (!y_dev || !g_dev || !out_dev || !ssq_host || !ws_dev || n <= 0 || clip < 0 || clip > 1) return ACCBPG_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int nb = red_blocks(n, QMAXBLK);
    double* part = ws_dev + n;
    quartic_prox_kernel<<<nb, QK, 0, s>>>(y_dev, g_dev, z, invL, clip, upper_bound, n, out_dev, part);
    const double* o = nullptr;
    ACC_TRY(q_finish(part, nb, s, &o));
    ssq_host[0] = o[0];
    return ACCBPG_OK;
}

extern "C" int accbpg_quartic_ls_terms(const double* g_dev, const double* x_dev, const double* y_dev,
                                       const double* z_dev, const double* z1_dev, int64_t n, double* out7_host,
                                       double* ws_dev, void* stream) {
    if (!x_dev || !y_dev || n <= 0 || !out7_host || !ws_dev) return ACCBPG_ERR_ARG;
    if ((z_dev == nullptr) != (z1_dev == nullptr)) return ACCBPG_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int nb = red_blocks(n, QMAXBLK);
    double* part = ws_dev + n;
    quartic_ls_kernel<<<nb, QK, 0, s>>>(g_dev, x_dev, y_dev, z_dev, z1_dev, n, part);
    const double* o = nullptr;
    ACC_TRY(q_finish(part, nb, s, &o));
    for (int k = 0; k < 7; ++k) out7_host[k] = o[k];
    return ACCBPG_OK;
}

extern "C" int accbpg_lmo_l2_ball(const double* g_dev, int center_kind, const double* center_dev, double center_val,
                                  double radius, double gnorm, int64_t n, double* out_dev, double* dist_host,
                                  double* ws_dev, void* stream) {
    if (!g_dev || !out_dev || !dist_host || !ws_dev || n <= 0 || center_kind < 0 || center_kind > 1) return ACCBPG_ERR_ARG;
    if (center_kind == 1 && !center_dev) return ACCBPG_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int nb = red_blocks(n, QMAXBLK);
    double* part = ws_dev + n;
    lmo_l2_kernel<<<nb, QK, 0, s>>>(g_dev, center_kind, center_dev, center_val, radius, gnorm, n, out_dev, part);
    const double* o = nullptr;
    ACC_TRY(q_finish(part, nb, s, &o));
    dist_host[0] = sqrt(o[0]);
    if (!(fabs(dist_host[0] - radius) <= 1e-10)) {                // functions_lmo.py:45-46
        set_last_error("Solution does not lie on ball boundary");
        return ACCBPG_ERR_ASSERT;
    }
    return ACCBPG_OK;
}

extern "C" int accbpg_lmo_linf_ball(const double* g_dev, int center_kind, const double* center_dev, double center_val,
                                    double radius, int64_t n, double* out_dev, void* stream) {
    if (!g_dev || !out_dev || n <= 0 || center_kind < 0 || center_kind > 1) return ACCBPG_ERR_ARG;
    if (center_kind == 1 && !center_dev) return ACCBPG_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    lmo_linf_kernel<<<ew_blocks(n), QK, 0, s>>>(g_dev, center_kind, center_dev, center_val, radius, n, out_dev);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}
