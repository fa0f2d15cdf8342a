// Length-n kernels of the inexact-oracle accelerated methods AIBM, AdaptFGM and UniversalGM
// (accbpg/algorithms.py:593-777) and of lmo_l2_ball_positive_orthant (accbpg/functions_lmo.py:54-102) on gfx950.
//
//   combine_ls:  w = (a*u + b*v)/c written out, with <g, w - x> and D_h(w, x) reduced in the same pass
//                (h = Burg entropy or (1/2)||.||^2): the extrapolated point of a line-search try and the two
//                numbers its test needs, one read-back.  c = 1 gives AIBM's alpha/B*z + (1-alpha/B)*y (:628, :632),
//                c = A gives (alpha*u + A_k*x_k)/A of AdaptFGM / UniversalGM (:686-689, :744-748).
//   lmo_pos:     masked sum of squares over g < 0, then max(c + R*(-g/||g_neg||)*[g<0], eps) with ||s - c||^2 and
//                min(s) for the reference's two assertions.
//
// HBM/latency-bound streams of 8-byte loads (no alignment beyond that of a double is assumed), wavefront shuffle
// reductions and a fixed tree: block partials are added in block order, so results are reproducible run to run.  A
// vector that fits one block (n <= 1024) is reduced by the pass itself; longer ones take a second, one-block launch.
// Compiled with -ffp-contract=off: every product, sum and quotient rounds once, as the NumPy ufuncs do.
#include "internal.h"
#include "reduce.hpp"

namespace accbpg {

namespace {

constexpr int IK = RED_THREADS;  // threads per block
constexpr int IMAXBLK = 1024;    // 4 * IMAXBLK partials fit behind the n doubles of the vector workspace

// three sums and a minimum of a block -> dst[0..3]
__device__ __forceinline__ void i_block_store(double s0, double s1, double s2, double mn, double* __restrict__ dst) {
    double v[4] = {s0, s1, s2, mn};
    block_reduce_store<IK, 4, true>(v, dst);
}
// a one-block grid is the whole reduction: it writes the result; otherwise block b writes its partials
__device__ __forceinline__ double* i_dst(double* __restrict__ part, double* __restrict__ out) {
    return gridDim.x == 1 ? out : part + 4 * (int64_t)blockIdx.x;
}

// KIND 0: D = sum w/x - log(w/x) - 1 (functions.py:253), slot 3 = min over w and x (its assertion, :252)
// KIND 1: slot 1 = sum (w-x)^2, D = half of it (functions.py:749-750)
// x NULL: w only (nothing is reduced)
template <int KIND>
__global__ __launch_bounds__(IK) void combine_ls_kernel(double a, const double* __restrict__ u, double b,
                                                        const double* __restrict__ v, double c,
                                                        const double* __restrict__ g, const double* __restrict__ x,
                                                        int64_t n, double* __restrict__ w, double* __restrict__ part,
                                                        double* __restrict__ out) {
    double s0 = 0.0, s1 = 0.0, mn = __builtin_inf();
    const int64_t stride = (int64_t)gridDim.x * IK;
    for (int64_t i = (int64_t)blockIdx.x * IK + threadIdx.x; i < n; i += stride) {
        const double p = a * u[i];
        const double q = b * v[i];
        const double wi = (p + q) / c;
        w[i] = wi;
        if (x != nullptr) {
            const double xi = x[i];
            const double d = wi - xi;
            if (g != nullptr) s0 += g[i] * d;
            if (KIND == 0) {
                const double r = wi / xi;
                s1 += r - log(r) - 1.0;
                mn = min_nan(mn, min_nan(wi, xi));
            } else {
                s1 += d * d;
            }
        }
    }
    if (x != nullptr) i_block_store(s0, s1, 0.0, mn, i_dst(part, out));
}

// slot 0 = sum of g^2 over g < 0 (np.linalg.norm(g[g < 0])^2, functions_lmo.py:86-88), slot 2 = how many
__global__ __launch_bounds__(IK) void lmo_pos_norm_kernel(const double* __restrict__ g, int64_t n,
                                                          double* __restrict__ part, double* __restrict__ out) {
    double s0 = 0.0, cnt = 0.0;
    const int64_t stride = (int64_t)gridDim.x * IK;
    for (int64_t i = (int64_t)blockIdx.x * IK + threadIdx.x; i < n; i += stride) {
        const double gi = g[i];
        if (gi < 0.0) { s0 += gi * gi; cnt += 1.0; }
    }
    i_block_store(s0, 0.0, cnt, 0.0, i_dst(part, out));
}

// s = max(c + R*direction, eps) with direction = -g/||g_neg|| where g < 0, else 0 (functions_lmo.py:87-94); with no
// negative entry s = max(c, eps) (:83-84).  red = the result of lmo_pos_norm_kernel.  slot 0 = sum (s - c)^2, slot 3 =
// min s.  np.maximum keeps a NaN.
__global__ __launch_bounds__(IK) void lmo_pos_apply_kernel(const double* __restrict__ g, const double* __restrict__ c,
                                                           double radius, double eps, const double* __restrict__ red,
                                                           int64_t n, double* __restrict__ sout,
                                                           double* __restrict__ part, double* __restrict__ out) {
    const double gnorm = sqrt(red[0]);
    const bool any = red[2] > 0.0;
    double s0 = 0.0, mn = __builtin_inf();
    const int64_t stride = (int64_t)gridDim.x * IK;
    for (int64_t i = (int64_t)blockIdx.x * IK + threadIdx.x; i < n; i += stride) {
        const double ci = c != nullptr ? c[i] : 0.0;
        double si = ci;
        if (any) {
            const double gi = g[i];
            const double dir = gi < 0.0 ? (-gi) / gnorm : 0.0;
            const double t = radius * dir;
            si = ci + t;
        }
        si = (si >= eps || si != si) ? si : eps;
        sout[i] = si;
        const double d = si - ci;
        s0 += d * d;
        mn = min_nan(mn, si);
    }
    i_block_store(s0, 0.0, 0.0, mn, i_dst(part, out));
}

// the partials of each slot in block order
constexpr reduce_final_fn inexact_final_kernel = reduce_final_kernel<IK, 4, true>;

}  // namespace

}  // namespace accbpg

using namespace accbpg;

extern "C" int accbpg_combine_ls_terms(int kind, double a, const double* u_dev, double b, const double* v_dev, double c,
                                       const double* g_dev, const double* x_dev, int64_t n, double* w_dev,
                                       double* out2_host, double* ws_dev, void* stream) {
    if (!u_dev || !v_dev || !w_dev || n <= 0 || kind < 0 || kind > 1) return ACCBPG_ERR_ARG;
    if (w_dev == u_dev || w_dev == v_dev || w_dev == g_dev || w_dev == x_dev) return ACCBPG_ERR_ARG;
    if (x_dev && (!out2_host || !ws_dev)) return ACCBPG_ERR_ARG;
    if (g_dev && !x_dev) return ACCBPG_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    double* pin = nullptr; int* flags = nullptr; double* dout = nullptr;
    ACC_TRY(vec_scratch(&pin, &flags, &dout));
    int nb = red_blocks(n, IMAXBLK);
    if (!x_dev) nb = ew_blocks(n);                              // elementwise only: a block per 256 entries
    double* part = ws_dev ? ws_dev + n : nullptr;
    if (kind == 0)
        combine_ls_kernel<0><<<nb, IK, 0, s>>>(a, u_dev, b, v_dev, c, g_dev, x_dev, n, w_dev, part, dout);
    else
        combine_ls_kernel<1><<<nb, IK, 0, s>>>(a, u_dev, b, v_dev, c, g_dev, x_dev, n, w_dev, part, dout);
    ACC_HIP(hipGetLastError());
    if (!x_dev) return ACCBPG_OK;
    const double* o = reduce_finish(nb > 1 ? inexact_final_kernel : nullptr, part, nb, dout, dout, 4, pin, s);
    if (!o) return ACCBPG_ERR_HIP;
    out2_host[0] = o[0];
    out2_host[1] = kind == 0 ? o[1] : 0.5 * o[1];
    if (kind == 0 && !(o[3] > 0.0)) {                           // functions.py:252
        set_last_error("Entries of x or y not positive.");
        return ACCBPG_ERR_ASSERT;
    }
    return ACCBPG_OK;
}

extern "C" int accbpg_lmo_l2_ball_pos(const double* g_dev, const double* center_dev, double radius, double epsilon,
                                      int64_t n, double* out_dev, double* info3_host, double* ws_dev, void* stream) {
    if (!g_dev || !out_dev || !info3_host || !ws_dev || n <= 0 || out_dev == g_dev || out_dev == center_dev)
        return ACCBPG_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    double* pin = nullptr; int* flags = nullptr; double* dout = nullptr;
    ACC_TRY(vec_scratch(&pin, &flags, &dout));
    const int nb = red_blocks(n, IMAXBLK);
    double* part = ws_dev + n;
    lmo_pos_norm_kernel<<<nb, IK, 0, s>>>(g_dev, n, part, dout);
    if (nb > 1) inexact_final_kernel<<<1, IK, 0, s>>>(part, nb, dout);
    lmo_pos_apply_kernel<<<nb, IK, 0, s>>>(g_dev, center_dev, radius, epsilon, dout, n, out_dev, part, dout + 4);
    // both records (norm pass, apply pass) in one copy
    const double* o = reduce_finish(nb > 1 ? inexact_final_kernel : nullptr, part, nb, dout + 4, dout, 8, pin, s);
    if (!o) return ACCBPG_ERR_HIP;
    info3_host[0] = o[2];                                       // entries with g < 0
    info3_host[1] = sqrt(o[4]);                                 // ||s - c||
    info3_host[2] = o[7];                                       // min s
    if (!(o[2] > 0.0)) return ACCBPG_OK;                        // early return of :83-84: nothing is asserted
    if (!(o[7] >= epsilon)) {                                   // :97
        set_last_error("Output violates epsilon-nonnegativity");
        return ACCBPG_ERR_ASSERT;
    }
    if (!(info3_host[1] <= radius + 1e-8)) {                    // :98
        set_last_error("Output outside L2 ball");
        return ACCBPG_ERR_ASSERT;
    }
    return ACCBPG_OK;
}
