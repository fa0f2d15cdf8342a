// Length-n kernels of the Bregman proximal gradient loop on gfx950: Burg-entropy simplex prox
// (the whole bisection + Newton scalar solve in one launch), Bregman divergences, the line-search
// inner product, and the a*x + b*z combination.  HBM/latency-bound: coalesced 8-byte-per-lane
// streams, wavefront (64-lane) shuffle reductions, a fixed reduction tree so that results are
// reproducible run to run.
//
// This translation unit is compiled with -ffp-contract=off: the reference evaluates these
// expressions with separate NumPy ufuncs (one rounding per operation), so no multiply-add here
// may be fused.  Replaces accbpg/functions.py:246-271 and 336-356.
#include <atomic>
#include <cstring>
#include <mutex>

#include "internal.h"
#include "reduce.hpp"

namespace accbpg {

constexpr int PB = 1024;   // threads of the single-workgroup prox kernel
constexpr int RB = RED_THREADS;    // threads of the streaming reductions
constexpr int RMAXBLK = 1024;

// sum over the PB threads of the prox workgroup, result broadcast to every thread
__device__ __forceinline__ double block_sum_bcast(double v, double* sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < PB / 64; ++i) s += sh[i];
    return s;
}
__device__ __forceinline__ double block_min_bcast(double v, double* sh) {
    v = wave_min(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double s = sh[0];
#pragma unroll
    for (int i = 1; i < PB / 64; ++i) s = min_nan(s, sh[i]);
    return s;
}

// Burg simplex prox, functions.py:336-356 (and :264-271 when y != NULL).
// EPT > 0: gg lives in registers (n <= PB*EPT); EPT == 0: gg is kept in `ggbuf` and re-read.
// LOAD_ACC: the argument is xi + alpha*g, formed on load (one product, one sum) and stored to xi_out -- the
// accumulated gradient of AIBM (algorithms.py:630-631); everything behind the load is the same code.
// LOAD_AVG: the argument is (xi + alpha*g) / csum, the sum stored to xi_out and then divided (one more rounding) -- the
// weighted gradient average of ABDA and its quotient (algorithms.py:483-485).
constexpr int LOAD_PLAIN = 0, LOAD_ACC = 1, LOAD_AVG = 2;
template <int EPT, int LOAD = LOAD_PLAIN>
__device__ __forceinline__ void burg_prox_body(const double* __restrict__ y, const double* __restrict__ g,
                                               double L, double eps, int64_t n, double* __restrict__ xout,
                                               double* __restrict__ ggbuf, int* __restrict__ info,
                                               int* __restrict__ flags, const double* __restrict__ xi = nullptr,
                                               double alpha = 0.0, double* __restrict__ xi_out = nullptr,
                                               double csum = 1.0) {
    __shared__ double sh[PB / 64];
    const int tid = threadIdx.x;
    constexpr int R = EPT > 0 ? EPT : 1;
    double gg[R];
    const double inf = __builtin_inf();
    double lmin = inf;
    bool bad = false;

    auto make_gg = [&](int64_t i) -> double {
        double a = g[i];
        if constexpr (LOAD != LOAD_PLAIN) {
            const double t = alpha * a;       // alpha * grad_x     algorithms.py:630 (theta^(1-gamma) * g, :483)
            a = xi[i] + t;                    // xi_grad += ...
            xi_out[i] = a;
        }
        if constexpr (LOAD == LOAD_AVG) a = a / csum;      // gavg / csum      algorithms.py:485
        if (y != nullptr) {
            const double yi = y[i];
            if (!(yi > 0.0)) bad = true;
            const double t = -1.0 / yi;       // h.gradient(y)      functions.py:248
            a = a - L * t;                    // g - L*grad         functions.py:271
        }
        return a / L;                         // gg = g / L         functions.py:341
    };
    if constexpr (EPT > 0) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int64_t i = tid + (int64_t)PB * e;
            gg[e] = (i < n) ? make_gg(i) : inf;
            lmin = min_nan(lmin, gg[e]);
        }
    } else {
        for (int64_t i = tid; i < n; i += PB) {
            const double v = make_gg(i);
            ggbuf[i] = v;
            lmin = min_nan(lmin, v);
        }
    }
    const double cmin = -block_min_bcast(lmin, sh);       // functions.py:342

    auto phi = [&](double c) -> double {                   // sum(1/(gg+c)) - 1
        double s = 0.0;
        if constexpr (EPT > 0) {
#pragma unroll
            for (int e = 0; e < EPT; ++e) s += 1.0 / (gg[e] + c);
        } else {
            for (int64_t i = tid; i < n; i += PB) s += 1.0 / (ggbuf[i] + c);
        }
        return block_sum_bcast(s, sh) - 1.0;
    };
    auto dphi = [&](double c) -> double {                  // sum(-1/(gg+c)^2)
        double s = 0.0;
        if constexpr (EPT > 0) {
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const double r = gg[e] + c;
                s += -1.0 / (r * r);
            }
        } else {
            for (int64_t i = tid; i < n; i += PB) {
                const double r = ggbuf[i] + c;
                s += -1.0 / (r * r);
            }
        }
        return block_sum_bcast(s, sh);
    };

    double c = cmin + 1.0;                                 // functions.py:344
    int nb = 0, nn = 0;
    double fc = phi(c);
    while (fc < 0.0 && nb < 4096) {                        // functions.py:345-346
        c = (cmin + c) / 2.0;
        fc = phi(c);
        ++nb;
    }
    while (fabs(fc) > eps && nn < 4096) {                  // functions.py:349
        const double fpc = dphi(c);                        // :350
        const double step = fc / fpc;
        if ((c - (c - step)) == 0.0) break;                // :351-352
        c = c - step;                                      // :353
        fc = phi(c);                                       // :354
        ++nn;
    }
    if constexpr (EPT > 0) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int64_t i = tid + (int64_t)PB * e;
            if (i < n) xout[i] = 1.0 / (gg[e] + c);        // :355
        }
    } else {
        for (int64_t i = tid; i < n; i += PB) xout[i] = 1.0 / (ggbuf[i] + c);
    }
    // the status is written unconditionally (no memset in front of the launch)
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (tid == 0) {
        flags[FLAG_NOT_PD] = 0; flags[FLAG_NEG_X] = 0; flags[FLAG_NONPOS] = any_bad; flags[FLAG_BAD_G] = 0;
        info[0] = nb;
        info[1] = nn;
    }
}

template <int EPT>
__global__ __launch_bounds__(PB) void burg_prox_kernel(const double* __restrict__ y, const double* __restrict__ g,
                                                      double L, double eps, int64_t n, double* __restrict__ xout,
                                                      double* __restrict__ ggbuf, int* __restrict__ info,
                                                      int* __restrict__ flags) {
    burg_prox_body<EPT>(y, g, L, eps, n, xout, ggbuf, info, flags);
}
// BurgEntropySimplex.prox_map(xi + alpha*g, L) with the sum stored to xi_out (n <= PB*EPT)
template <int EPT>
__global__ __launch_bounds__(PB) void burg_prox_acc_kernel(const double* __restrict__ xi, double alpha,
                                                          const double* __restrict__ g, double L, double eps, int64_t n,
                                                          double* __restrict__ xi_out, double* __restrict__ xout,
                                                          int* __restrict__ info, int* __restrict__ flags) {
    burg_prox_body<EPT, LOAD_ACC>(nullptr, g, L, eps, n, xout, nullptr, info, flags, xi, alpha, xi_out);
}
// the prox of every active instance of a batch in one launch: a workgroup per instance (row `instance` of the K x n
// arrays), its own constant L, its own status words
template <int EPT>
__global__ __launch_bounds__(PB) void burg_prox_batch_kernel(BatchAct act, const double* __restrict__ ybase,
                                                            const double* __restrict__ gbase, int64_t ld, BatchVals Ls,
                                                            double eps, int64_t n, double* __restrict__ obase,
                                                            double* __restrict__ ggbase, int* __restrict__ flags) {
    const int inst = act.idx[blockIdx.x];
    burg_prox_body<EPT>(ybase ? ybase + (int64_t)inst * ld : nullptr, gbase + (int64_t)inst * ld, Ls.v[inst], eps, n,
                        obase + (int64_t)inst * ld, ggbase ? ggbase + (int64_t)inst * n : nullptr, flags + 8 * inst + 4,
                        flags + 8 * inst);
}
// ABDA's step of every active instance in one launch: row i of avg_out = avg_i + wgt_i * g_i, row i of obase =
// prox_map(avg_out_i / csum_i, Lc_i) (n <= PB*EPT)
template <int EPT>
__global__ __launch_bounds__(PB) void burg_avg_prox_batch_kernel(BatchAct act, const double* __restrict__ avgbase,
                                                                const double* __restrict__ gbase, int64_t ld,
                                                                BatchVals wgt, BatchVals csum, BatchVals Lc, double eps,
                                                                int64_t n, double* __restrict__ avg_out,
                                                                double* __restrict__ obase, int* __restrict__ flags) {
    const int inst = act.idx[blockIdx.x];
    const int64_t row = (int64_t)inst * ld;
    burg_prox_body<EPT, LOAD_AVG>(nullptr, gbase + row, Lc.v[inst], eps, n, obase + row, nullptr, flags + 8 * inst + 4,
                                  flags + 8 * inst, avgbase + row, wgt.v[inst], avg_out + row, csum.v[inst]);
}

// ---------------------------------------------------------------------------------------------------------------
// The same prox over SEVERAL workgroups for long vectors (n > 32768: BASELINE config 5 has n = 262144, replicated on
// every rank): each workgroup keeps its slice of gg in registers and runs the scalar loop itself; the two sums of a
// Newton step (phi and phi' at the same c: the reference evaluates phi at the new c and then phi' at that c) travel in
// ONE exchange: every workgroup publishes its two partial sums (write-through stores, then an epoch flag), waits for the
// flags of all others, and adds the partials in workgroup order -- so every workgroup obtains bit-identical totals and
// takes identical decisions, with no further communication.  Exchange r uses slot set r & 1 (a workgroup can only be
// one exchange ahead of the slowest).  Every wait is bounded: on a timeout the launch raises flags[4] and the host
// reruns the single-workgroup kernel.  All workgroups must be resident together (at most 128 of 1024 threads).
// ---------------------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(1))) double pm_gdouble;
typedef __attribute__((address_space(1))) int pm_gint;
struct ProxMultiShared {
    double* part;      // [2][G][2] partial sums
    int* epoch;        // [G] last exchange each workgroup has published (1-based)
    int* abortw;
};
template <int OP>      // 0: sums of both values, 1: minimum of the first
__device__ __forceinline__ bool pm_exchange(const ProxMultiShared sh, int G, int round, double& a, double& b, double* lds,
                                            long long limit) {
    const int w = blockIdx.x;
    double* slot = sh.part + ((size_t)(round & 1) * G + w) * 2;
    if (threadIdx.x == 0) {
        __hip_atomic_store((pm_gdouble*)slot, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store((pm_gdouble*)(slot + 1), b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store((pm_gint*)(sh.epoch + w), round + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    int ok = 1;
    if (threadIdx.x < 64) {
        // lane l waits for the workgroups l, l + 64, ...
        const long long t0 = wall_clock64();
        unsigned spins = 0;
        for (int v = threadIdx.x; v < G; v += 64) {
            while (__hip_atomic_load((const pm_gint*)(sh.epoch + v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < round + 1) {
                __builtin_amdgcn_s_sleep(1);
                if ((++spins & 31u) == 0u) {
                    if (__hip_atomic_load((const pm_gint*)sh.abortw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) { ok = 0; break; }
                    if (wall_clock64() - t0 > limit) {
                        __hip_atomic_store((pm_gint*)sh.abortw, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        ok = 0;
                        break;
                    }
                }
            }
            if (!ok) break;
        }
        ok = __all(ok);
        if (ok && threadIdx.x == 0) {
            // one lane adds the partials in workgroup order (every workgroup does the same sum)
            const double* base = sh.part + (size_t)(round & 1) * G * 2;
            double sa = __hip_atomic_load((const pm_gdouble*)base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            double sb = __hip_atomic_load((const pm_gdouble*)(base + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int v = 1; v < G; ++v) {
                const double pa = __hip_atomic_load((const pm_gdouble*)(base + 2 * v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const double pb = __hip_atomic_load((const pm_gdouble*)(base + 2 * v + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (OP == 0) { sa += pa; sb += pb; }
                else { sa = min_nan(sa, pa); }
            }
            lds[0] = sa; lds[1] = sb;
        }
        if (threadIdx.x == 0) lds[2] = ok ? 1.0 : 0.0;
    }
    __syncthreads();
    a = lds[0]; b = lds[1];
    const bool good = lds[2] != 0.0;
    __syncthreads();
    return good;
}

template <int EPT>
__global__ __launch_bounds__(PB) void burg_prox_multi_kernel(const double* __restrict__ y, const double* __restrict__ g,
                                                            double L, double eps, int64_t n, double* __restrict__ xout,
                                                            ProxMultiShared shm, int G, int* __restrict__ info,
                                                            int* __restrict__ flags, long long limit) {
    __shared__ double sh[PB / 64];
    __shared__ double xch[4];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * PB * EPT;
    double gg[EPT];
    const double inf = __builtin_inf();
    double lmin = inf;
    bool bad = false;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int64_t i = base + tid + (int64_t)PB * e;
        double v = inf;
        if (i < n) {
            double a = g[i];
            if (y != nullptr) {
                const double yi = y[i];
                if (!(yi > 0.0)) bad = true;
                const double t = -1.0 / yi;       // h.gradient(y)      functions.py:248
                a = a - L * t;                    // g - L*grad         functions.py:271
            }
            v = a / L;                            // gg = g / L         functions.py:341
        }
        gg[e] = v;
        lmin = min_nan(lmin, v);
    }
    int round = 0;
    double m0 = block_min_bcast(lmin, sh), m1 = 0.0;
    if (!pm_exchange<1>(shm, G, round++, m0, m1, xch, limit)) return;
    const double cmin = -m0;                                   // functions.py:342
    // phi(c) = sum 1/(gg+c) - 1 and phi'(c) = sum -1/(gg+c)^2, both at the same c, in one exchange
    auto both = [&](double c, double& fc, double& fpc) -> bool {
        double s = 0.0, d = 0.0;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const double r = gg[e] + c;
            s += 1.0 / r;
            d += -1.0 / (r * r);
        }
        s = block_sum_bcast(s, sh);
        d = block_sum_bcast(d, sh);
        if (!pm_exchange<0>(shm, G, round++, s, d, xch, limit)) return false;
        fc = s - 1.0;
        fpc = d;
        return true;
    };
    double c = cmin + 1.0;                                     // functions.py:344
    int nb = 0, nn = 0;
    double fc, fpc;
    if (!both(c, fc, fpc)) return;
    while (fc < 0.0 && nb < 4096) {                            // functions.py:345-346
        c = (cmin + c) / 2.0;
        if (!both(c, fc, fpc)) return;
        ++nb;
    }
    while (fabs(fc) > eps && nn < 4096) {                      // functions.py:349
        const double step = fc / fpc;                          // :350 (phi' at the current c came with phi)
        if ((c - (c - step)) == 0.0) break;                    // :351-352
        c = c - step;                                          // :353
        if (!both(c, fc, fpc)) return;                         // :354
        ++nn;
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int64_t i = base + tid + (int64_t)PB * e;
        if (i < n) xout[i] = 1.0 / (gg[e] + c);                // :355
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (tid == 0) {
        if (any_bad) atomicOr(flags + FLAG_NONPOS, 1);
        if (blockIdx.x == 0) { info[0] = nb; info[1] = nn; }
    }
}

// Streaming reduction, stage 1.  Up to four sums / minima per pass:
//   q0 = sum g*(x-y)                                  (np.dot(g, x1-x), algorithms.py:53)
//   q1 = sum x/y - log(x/y) - 1                       (functions.py:253)
//   q2 = sum z/z1 - log(z/z1) - 1
//   q3 = min over every vector that enters a divergence (positivity assert, functions.py:252)
__device__ __forceinline__ void ls_terms_partial_body(const double* __restrict__ g,
                                                      const double* __restrict__ x,
                                                      const double* __restrict__ y,
                                                      const double* __restrict__ z,
                                                      const double* __restrict__ z1, int64_t n,
                                                      int want_div_xy, double* __restrict__ part) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, mn = __builtin_inf();
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < n; i += stride) {
        if (x != nullptr && y != nullptr) {
            const double xi = x[i], yi = y[i];
            if (g != nullptr) {
                const double d = xi - yi;
                s0 += g[i] * d;
            }
            if (want_div_xy) {
                const double r = xi / yi;
                s1 += r - log(r) - 1.0;
                mn = min_nan(mn, min_nan(xi, yi));
            }
        }
        if (z != nullptr) {
            const double zi = z[i], wi = z1[i];
            const double r = zi / wi;
            s2 += r - log(r) - 1.0;
            mn = min_nan(mn, min_nan(zi, wi));
        }
    }
    double v[4] = {s0, s1, s2, mn};
    block_reduce_store<RB, 4, true>(v, part + blockIdx.x * 4);
}

__global__ __launch_bounds__(RB) void ls_terms_partial_kernel(const double* __restrict__ g,
                                                             const double* __restrict__ x,
                                                             const double* __restrict__ y,
                                                             const double* __restrict__ z,
                                                             const double* __restrict__ z1, int64_t n,
                                                             int want_div_xy, double* __restrict__ part) {
    ls_terms_partial_body(g, x, y, z, z1, n, want_div_xy, part);
}
// the same pass for every active instance of a batch (blockIdx.y); partials of instance i at part + i * pstride
__global__ __launch_bounds__(RB) void ls_terms_partial_batch_kernel(BatchAct act, const double* __restrict__ g,
                                                                   const double* __restrict__ x,
                                                                   const double* __restrict__ y,
                                                                   const double* __restrict__ z,
                                                                   const double* __restrict__ z1, int64_t ld, int64_t n,
                                                                   double* __restrict__ part, int64_t pstride) {
    const int64_t o = (int64_t)act.idx[blockIdx.y] * ld;
    ls_terms_partial_body(g ? g + o : nullptr, x + o, y + o, z ? z + o : nullptr, z1 ? z1 + o : nullptr, n, 1,
                          part + (int64_t)act.idx[blockIdx.y] * pstride);
}

// stage 2: one workgroup adds the partials in block order
__global__ __launch_bounds__(RB) void ls_terms_final_kernel(const double* __restrict__ part, int nblk,
                                                           double* __restrict__ out) {
    reduce_final_body<RB, 4, true>(part, nblk, out);
}
__global__ __launch_bounds__(RB) void ls_terms_final_batch_kernel(BatchAct act, const double* __restrict__ part,
                                                                 int64_t pstride, int nblk, double* __restrict__ out) {
    const int inst = act.idx[blockIdx.x];
    reduce_final_body<RB, 4, true>(part + (int64_t)inst * pstride, nblk, out + 4 * inst);
}

// out = a*x + b*z for every active instance of a batch (its own a and b), NumPy's rounding as in axpby_kernel
__global__ __launch_bounds__(RB) void axpby_batch_kernel(BatchAct act, BatchVals a, const double* __restrict__ x, BatchVals b,
                                                        const double* __restrict__ z, int64_t ld, int64_t n,
                                                        double* __restrict__ out) {
    const int inst = act.idx[blockIdx.y];
    const double ai = a.v[inst], bi = b.v[inst];
    const int64_t o = (int64_t)inst * ld;
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < n; i += stride) {
        const double p = ai * x[o + i];
        const double q = bi * z[o + i];
        out[o + i] = p + q;
    }
}

__global__ __launch_bounds__(RB) void min_sum_partial_kernel(const double* __restrict__ x, int64_t n,
                                                            double* __restrict__ part) {
    double s = 0.0, mn = __builtin_inf();
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < n; i += stride) {
        const double v = x[i];
        s += v;
        mn = min_nan(mn, v);
    }
    double v[2] = {s, mn};
    block_reduce_store<RB, 2, true, 4>(v, part + blockIdx.x * 4);
}

// out = a*x + b*z with NumPy's rounding of (1-theta)*x + theta*z   (algorithms.py:147,150,369,374)
__global__ __launch_bounds__(RB) void axpby_kernel(double a, const double* __restrict__ x, double b,
                                                  const double* __restrict__ z, int64_t n,
                                                  double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < n; i += stride) {
        const double p = a * x[i];
        const double q = b * z[i];
        out[i] = p + q;
    }
}

// out = x / d elementwise (NumPy true division: gavg/csum, algorithms.py:485)
__global__ __launch_bounds__(RB) void div_scalar_kernel(const double* __restrict__ x, double d, int64_t n,
                                                       double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < n; i += stride) out[i] = x[i] / d;
}

// out[i] = fill, out[idx] = value  (lmo_simplex vertex, functions_lmo.py:152-157)
__global__ __launch_bounds__(RB) void vertex_kernel(int64_t idx, double value, double fill, int64_t n,
                                                   double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < n; i += stride) out[i] = (i == idx) ? value : fill;
}

// sum x*y  (np.dot(x, x) of BurgEntropyL2.extra_Psi, functions.py:314)
__global__ __launch_bounds__(RB) void dot_partial_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                        int64_t n, double* __restrict__ part) {
    double s = 0.0;
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < n; i += stride) s += x[i] * y[i];
    double v[1] = {s};
    block_reduce_store<RB, 1, false, 4>(v, part + blockIdx.x * 4);
}

// sum |x|  (np.sum(abs(x)) of L2L1Linf.extra_Psi, functions.py:801)
__global__ __launch_bounds__(RB) void l1_partial_kernel(const double* __restrict__ x, int64_t n,
                                                       double* __restrict__ part) {
    double s = 0.0;
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < n; i += stride) s += fabs(x[i]);
    double v[1] = {s};
    block_reduce_store<RB, 1, false, 4>(v, part + blockIdx.x * 4);
}

// slots: 0 <g,x-y>, 1 sum (x-y)^2, 2 sum (z-z1)^2 -- the line-search terms of h = (1/2)||.||^2 (functions.py:809-815)
__global__ __launch_bounds__(RB) void sq_ls_partial_kernel(const double* __restrict__ g, const double* __restrict__ x,
                                                          const double* __restrict__ y, const double* __restrict__ z,
                                                          const double* __restrict__ z1, int64_t n,
                                                          double* __restrict__ part) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < n; i += stride) {
        const double d = x[i] - y[i];
        if (g != nullptr) s0 += g[i] * d;
        s1 += d * d;
        if (z != nullptr) {
            const double dz = z[i] - z1[i];
            s2 += dz * dz;
        }
    }
    double v[3] = {s0, s1, s2};
    block_reduce_store<RB, 3, false, 4>(v, part + blockIdx.x * 4);
}

// L2L1Linf.prox_map / div_prox_map (functions.py:817-835) in the reference's operation order:
//   w = g - L*y (y given), v = -(invL*w), soft threshold at thr, clip to [-B, B] with a NaN kept as np.clip keeps it
__global__ __launch_bounds__(RB) void l2l1linf_prox_kernel(const double* __restrict__ y, const double* __restrict__ g,
                                                          double L, double invL, double thr, double B, int64_t n,
                                                          double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < n; i += stride) {
        double w = g[i];
        if (y != nullptr) {
            const double ly = L * y[i];
            w = w - ly;
        }
        const double p = invL * w;
        double v = -p;
        if (fabs(v) <= thr) v = 0.0;                  // x[abs(x) <= threshold] = 0
        if (v > thr) v = v - thr;                     // x[x > threshold] -= threshold
        if (v < -thr) v = v + thr;                    // x[x < -threshold] += threshold
        v = (v < -B) ? -B : v;                        // np.clip: a NaN passes both comparisons
        v = (v > B) ? B : v;
        out[i] = v;
    }
}

// Closed-form Burg-entropy prox maps on x > 0 with NumPy's operation order:
//   gt = g - L*(-1/y)  when y != NULL (BurgEntropy.div_prox_map, functions.py:264-271), else gt = g
//   kind 0: L / gt                                     (BurgEntropy.prox_map,   :255-262, needs gt > 0)
//   kind 1: L / (lamda + gt)                           (BurgEntropyL1.prox_map, :290-298, needs gt > -lamda)
//   kind 2: (sqrt(gg*gg + 4*lamda_L) - gg)/(2*lamda_L) (BurgEntropyL2.prox_map, :316-323), gg = gt/L, lamda_L = lamda/L
__global__ __launch_bounds__(RB) void burg_reg_prox_kernel(int kind, const double* __restrict__ y,
                                                          const double* __restrict__ g, double L, double lamda,
                                                          int64_t n, double* __restrict__ out,
                                                          int* __restrict__ flags) {
    const int64_t stride = (int64_t)gridDim.x * RB;
    const double lamda_L = lamda / L;
    const double four_l = 4 * lamda_L, two_l = 2 * lamda_L;
    bool bad_y = false, bad_g = false;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < n; i += stride) {
        double gt = g[i];
        if (y != nullptr) {
            const double yi = y[i];
            bad_y |= !(yi > 0.0);
            const double hy = -1.0 / yi;
            const double t = L * hy;
            gt = gt - t;
        }
        double r;
        if (kind == 0) {
            bad_g |= !(gt > 0.0);
            r = L / gt;
        } else if (kind == 1) {
            bad_g |= !(gt > -lamda);
            r = L / (lamda + gt);
        } else {
            const double gg = gt / L;
            const double sq = gg * gg;
            r = (sqrt(sq + four_l) - gg) / two_l;
        }
        out[i] = r;
    }
    if (bad_y) flags[FLAG_NONPOS] = 1;
    if (bad_g) flags[FLAG_BAD_G] = 1;
}

// first-index argmin and argmax (np.argmin / np.argmax / np.where(g == g.min())[0][0])
__global__ __launch_bounds__(RB) void minmax_partial_kernel(const double* __restrict__ x, int64_t n,
                                                           MinMaxRec* __restrict__ part) {
    minmax_partial_body(x, n, part);
}
__global__ __launch_bounds__(RB) void minmax_final_kernel(const MinMaxRec* __restrict__ part, int nblk,
                                                         MinMaxRec* __restrict__ out) {
    const MinMaxRec a = minmax_final_body(part, nblk);
    if (threadIdx.x == 0) *out = a;
}

// -----------------------------------------------------------------------------------------
// The Frank-Wolfe direction of a gradient g at x in two phases (accbpg_fw_direction): what lmo(g), s - x, <g, g>,
// <g, s - x> and <s - x, s - x> compute in five launches with a read-back each.
//   phase 1  sum g^2 (the terms and the tree of dot_partial_kernel) and the first-index argmin of g; the final stage
//            leaves {sum g^2, min g, argmin as int64 bits, 1.0 when sqrt(sum g^2) < 1e-10} in four device doubles
//   phase 2  s from those scalars, d = s - x, and the sums <g, d>, sum d^2, sum (s - c)^2
// Every elementwise operation is the one of the kernel it replaces: lmo_l2_kernel / lmo_linf_kernel
// (quartic_kernels.hip), vertex_kernel, axpby_kernel with a = 1, b = -1 (1*s and -1*x are exact, so p + q is s - x).
constexpr int FWD_L2 = 0, FWD_LINF = 1, FWD_SIMPLEX = 2;
constexpr double FWD_FILL = 1e-15;         // the simplex vertex's other entries (functions_lmo.py:152)
constexpr double FWD_TINY = 1e-10;         // ||g|| below this: the l2 ball's centre (functions_lmo.py:37)

// part: nb block sums of g^2, then (from part + RMAXBLK) nb pairs {min g, argmin bits}
__global__ __launch_bounds__(RB) void fw_dir_scan_kernel(const double* __restrict__ g, int64_t n,
                                                        double* __restrict__ part) {
    __shared__ MinMaxRec sh[RB / 64];
    const double inf = __builtin_inf();
    MinMaxRec a{inf, -inf, INT64_MAX, INT64_MAX};
    double s = 0.0;
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < n; i += stride) {
        const double v = g[i];
        s += v * v;
        a = mm_merge(a, MinMaxRec{v, v, i, i});
    }
    a = mm_block(a, sh);
    double v[1] = {s};
    block_reduce_store<RB, 1, false>(v, part + blockIdx.x);
    if (threadIdx.x == 0) {
        part[RMAXBLK + 2 * blockIdx.x] = a.vmin;
        part[RMAXBLK + 2 * blockIdx.x + 1] = __longlong_as_double((long long)a.imin);
    }
}
__global__ __launch_bounds__(RB) void fw_dir_scan_final_kernel(const double* __restrict__ part, int nb,
                                                              double* __restrict__ scal) {
    __shared__ MinMaxRec sh[RB / 64];
    const double inf = __builtin_inf();
    MinMaxRec a{inf, -inf, INT64_MAX, INT64_MAX};
    for (int b = threadIdx.x; b < nb; b += RB) {
        const double v = part[RMAXBLK + 2 * b];
        const int64_t i = (int64_t)__double_as_longlong(part[RMAXBLK + 2 * b + 1]);
        a = mm_merge(a, MinMaxRec{v, v, i, i});
    }
    a = mm_block(a, sh);
    __shared__ double tot[1];
    reduce_final_body<RB, 1, false>(part, nb, tot);
    __syncthreads();
    if (threadIdx.x == 0) {
        scal[0] = tot[0];
        scal[1] = a.vmin;
        scal[2] = __longlong_as_double((long long)a.imin);
        scal[3] = (sqrt(tot[0]) < FWD_TINY) ? 1.0 : 0.0;     // a NaN norm is not small: NaN goes through, as on the host
    }
}
// slots: 0 <g, d>, 1 sum d^2, 2 sum (s - c)^2 (l2 ball away from the centre, else 0)
__global__ __launch_bounds__(RB) void fw_dir_form_kernel(int lmo, const double* __restrict__ g,
                                                        const double* __restrict__ x, int kind,
                                                        const double* __restrict__ c, double cval, double radius,
                                                        const double* __restrict__ scal, int64_t n,
                                                        double* __restrict__ s_out, double* __restrict__ d_out,
                                                        double* __restrict__ part) {
    const double gnorm = sqrt(scal[0]);
    const int64_t imin = (int64_t)__double_as_longlong(scal[2]);
    const bool centre = scal[3] != 0.0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const int64_t stride = (int64_t)gridDim.x * RB;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < n; i += stride) {
        const double gi = g[i];
        double si;
        if (lmo == FWD_SIMPLEX) {
            si = (i == imin) ? radius : FWD_FILL;
        } else {
            const double ci = kind == 1 ? c[i] : cval;
            if (lmo == FWD_LINF) {
                const double sg = gi > 0.0 ? 1.0 : (gi < 0.0 ? -1.0 : gi);
                si = ci - radius * sg;
            } else if (centre) {
                si = ci;
            } else {
                const double t = (radius * gi) / gnorm;
                si = ci - t;
                const double e = si - ci;
                s2 += e * e;
            }
        }
        const double di = si - x[i];
        s_out[i] = si;
        d_out[i] = di;
        s0 += gi * di;
        s1 += di * di;
    }
    double v[3] = {s0, s1, s2};
    block_reduce_store<RB, 3, false, 4>(v, part + blockIdx.x * 4);
}

// -----------------------------------------------------------------------------------------
// Scratch of the handle-free entry points: one block per (host thread, device) -- instances of a batch are
// driven from separate threads on separate streams, and one thread may drive several GPUs.  A block goes back
// to a per-device pool when its thread ends and is handed to the next thread that asks, so generations of
// worker threads do not grow the allocation; the pool itself lives as long as the process.
struct ScratchBlock {
    double* pin = nullptr;       // pinned host scratch (32 doubles)
    int* flags = nullptr;        // device flags (8 ints)
    double* out = nullptr;       // device result scalars (16 doubles)
};
constexpr int MAX_DEV = 64;
static std::mutex g_pool_mu;
static std::vector<ScratchBlock> g_pool[MAX_DEV];
struct ThreadScratch {
    ScratchBlock blk[MAX_DEV];
    ~ThreadScratch() {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (int d = 0; d < MAX_DEV; ++d)
            if (blk[d].pin) g_pool[d].push_back(blk[d]);
    }
};
static thread_local ThreadScratch g_tls;
static thread_local double* g_pin = nullptr;       // the block of the device current at the last ensure_scratch()
static thread_local int* g_flags = nullptr;
static thread_local double* g_out = nullptr;

static int ensure_scratch() {
    int dev = 0;
    ACC_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEV) return ACCBPG_ERR_ARG;
    ScratchBlock& b = g_tls.blk[dev];
    if (!b.pin) {
        {
            std::lock_guard<std::mutex> lk(g_pool_mu);
            if (!g_pool[dev].empty()) { b = g_pool[dev].back(); g_pool[dev].pop_back(); }
        }
        if (!b.pin) {
            ScratchBlock nb;
            ACC_HIP(hipHostMalloc(&nb.pin, 32 * sizeof(double), hipHostMallocDefault));
            if (acc_malloc(&nb.flags, 8 * sizeof(int), "vec scratch flags") != hipSuccess || acc_malloc(&nb.out, 16 * sizeof(double), "vec scratch out") != hipSuccess) {
                hipHostFree(nb.pin); acc_free(nb.flags); acc_free(nb.out);
                set_last_error("accbpg: out of device memory for the vector-kernel scratch");
                return ACCBPG_ERR_HIP;
            }
            b = nb;
        }
    }
    g_pin = b.pin; g_flags = b.flags; g_out = b.out;
    return ACCBPG_OK;
}

int vec_scratch(double** pin, int** flags, double** out) {
    ACC_TRY(ensure_scratch());
    *pin = g_pin; *flags = g_flags; *out = g_out;
    return ACCBPG_OK;
}

static bool g_prox_multi_off = false;    // set when the multi-workgroup prox had to give up a wait (then: one workgroup)
static std::atomic<int> g_prox_variant{0};          // accbpg_debug_prox_variant
static thread_local int g_prox_last[2] = {0, 0};    // {variant, workgroups} of this thread's last prox launch

int64_t vec_ws_doubles(int64_t n) { return n + 4 * RMAXBLK + 64; }

// the tail of the 4-slot reductions: final stage over nb block records behind the n doubles of ws, result on the host
static const double* finish4(const double* part, int nb, hipStream_t s) {
    return reduce_finish(ls_terms_final_kernel, part, nb, g_out, g_out, 4, g_pin, s);
}

}  // namespace accbpg

using namespace accbpg;

extern "C" int64_t accbpg_vec_workspace_doubles(int64_t n) { return vec_ws_doubles(n); }

namespace accbpg {
// The launch forms of the Burg simplex prox.  prox_plan picks the form of a call: by size, or the one
// accbpg_debug_prox_variant names.  prox_enqueue makes the launches of that form on s and waits for nothing: the
// status goes to `flags` (8 device ints: flags 0..3, then {bisection, newton}); the multi-workgroup form raises
// `gave_up` (a device int its launch zeroes through `flags` or the workspace) when it abandons a wait.
struct ProxPlan {
    bool multi, wide;
    int forced, G;
};
static int prox_plan(int64_t n, ProxPlan* p) {
    // the form of this call: by size, or the one accbpg_debug_prox_variant names
    const int forced = g_prox_variant.load(std::memory_order_relaxed);
    bool multi, wide;
    if (forced == 2 || forced == 3) { multi = true; wide = forced == 3; }
    else if (forced == 1) { multi = false; wide = false; }
    else {
        multi = n > (int64_t)PB * 32 && n <= (int64_t)PB * 32 * 128 && !g_prox_multi_off;
        wide = n > (int64_t)PB * 8 * 128;
    }
    const int ept = wide ? 32 : 8;
    const int64_t G64 = (n + (int64_t)PB * ept - 1) / ((int64_t)PB * ept);
    if (multi && G64 > 128) {                                   // only a forced form can get here
        set_last_error("accbpg_burg_simplex_div_prox: the forced multi-workgroup form needs more than 128 workgroups");
        return ACCBPG_ERR_ARG;
    }
    p->multi = multi; p->wide = wide; p->forced = forced; p->G = (int)G64;
    return ACCBPG_OK;
}
// long vectors: several workgroups, each with its slice in registers (ws_dev: exchange slots, then the epoch flags and,
// unless the caller keeps the give-up word elsewhere -- inside `flags`, which is zeroed here --, that word)
static int prox_enqueue_multi(const ProxPlan& p, const double* y_dev, const double* g_dev, double L, double eps, int64_t n,
                              double* x_out_dev, double* ws_dev, int* flags, int* gave_up, hipStream_t s,
                              int** gave_up_at) {
    const int G = p.G;
    int* g_info = flags + 4;
    ProxMultiShared shm;
    shm.part = ws_dev;
    shm.epoch = reinterpret_cast<int*>(ws_dev + 4 * G);
    shm.abortw = gave_up ? gave_up : shm.epoch + G;
    ACC_HIP(hipMemsetAsync(ws_dev, 0, sizeof(double) * 4 * G + sizeof(int) * (G + 4), s));
    ACC_HIP(hipMemsetAsync(flags, 0, 8 * sizeof(int), s));
    if (p.wide)
        burg_prox_multi_kernel<32><<<G, PB, 0, s>>>(y_dev, g_dev, L, eps, n, x_out_dev, shm, G, g_info, flags, 20000000LL);
    else
        burg_prox_multi_kernel<8><<<G, PB, 0, s>>>(y_dev, g_dev, L, eps, n, x_out_dev, shm, G, g_info, flags, 20000000LL);
    ACC_HIP(hipGetLastError());
    g_prox_last[0] = p.wide ? 3 : 2; g_prox_last[1] = G;
    if (gave_up_at) *gave_up_at = shm.abortw;
    return ACCBPG_OK;
}
static int prox_enqueue_single(int forced, const double* y_dev, const double* g_dev, double L, double eps, int64_t n,
                               double* x_out_dev, double* ws_dev, int* flags, hipStream_t s) {
    int* g_info = flags + 4;                                    // {bisection, newton} right behind the flags
    int ran;
    if (forced != 1 && n <= (int64_t)PB * 2) {
        burg_prox_kernel<2><<<1, PB, 0, s>>>(y_dev, g_dev, L, eps, n, x_out_dev, ws_dev, g_info, flags);
        ran = 10;
    } else if (forced != 1 && n <= (int64_t)PB * 8) {
        burg_prox_kernel<8><<<1, PB, 0, s>>>(y_dev, g_dev, L, eps, n, x_out_dev, ws_dev, g_info, flags);
        ran = 11;
    } else if (forced != 1 && n <= (int64_t)PB * 32) {
        burg_prox_kernel<32><<<1, PB, 0, s>>>(y_dev, g_dev, L, eps, n, x_out_dev, ws_dev, g_info, flags);
        ran = 12;
    } else {
        burg_prox_kernel<0><<<1, PB, 0, s>>>(y_dev, g_dev, L, eps, n, x_out_dev, ws_dev, g_info, flags);
        ran = 1;
    }
    g_prox_last[0] = ran; g_prox_last[1] = 1;
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

// The length-n stages of accbpg_dopt_burg_trial (capi.hip): the same launches as accbpg_burg_simplex_div_prox and
// accbpg_ls_terms make, with their status words at addresses of the caller's and no wait.
int trial_prox_enqueue(const double* y_dev, const double* g_dev, double L, double eps, int64_t n, double* x_out_dev,
                       double* ws_dev, int* flags8, int gave_up_idx, hipStream_t s, bool* multi) {
    ProxPlan p;
    ACC_TRY(prox_plan(n, &p));
    *multi = p.multi;
    if (p.multi)
        return prox_enqueue_multi(p, y_dev, g_dev, L, eps, n, x_out_dev, ws_dev, flags8, flags8 + gave_up_idx, s, nullptr);
    return prox_enqueue_single(p.forced, y_dev, g_dev, L, eps, n, x_out_dev, ws_dev, flags8, s);
}
void trial_prox_gave_up() { g_prox_multi_off = true; }         // a wait timed out: one workgroup from here on
int trial_ls_terms_enqueue(const double* g_dev, const double* x_dev, const double* y_dev, const double* z_dev,
                           const double* z1_dev, int64_t n, double* ws_dev, double* out4_dev, hipStream_t s) {
    const int nb = red_blocks(n, RMAXBLK);
    double* part = ws_dev + n;
    ls_terms_partial_kernel<<<nb, RB, 0, s>>>(g_dev, x_dev, y_dev, z_dev, z1_dev, n, 1, part);
    ls_terms_final_kernel<<<1, RB, 0, s>>>(part, nb, out4_dev);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}
}  // namespace accbpg

extern "C" int accbpg_burg_simplex_div_prox(const double* y_dev, const double* g_dev, double L, double eps,
                                            int64_t n, double* x_out_dev, double* ws_dev, int* info_host,
                                            void* stream) {
    if (!g_dev || !x_out_dev || n <= 0 || !ws_dev) return ACCBPG_ERR_ARG;
    if (!(L > 0.0)) return ACCBPG_ERR_ASSERT;                 // functions.py:270 / :340
    ProxPlan p;
    ACC_TRY(prox_plan(n, &p));
    ACC_TRY(ensure_scratch());
    hipStream_t s = (hipStream_t)stream;
    if (p.multi) {
        int* gave_up = nullptr;
        ACC_TRY(prox_enqueue_multi(p, y_dev, g_dev, L, eps, n, x_out_dev, ws_dev, g_flags, nullptr, s, &gave_up));
        int* pin_m = reinterpret_cast<int*>(g_pin);
        ACC_HIP(hipMemcpyAsync(pin_m, g_flags, 6 * sizeof(int), hipMemcpyDeviceToHost, s));
        ACC_HIP(hipMemcpyAsync(pin_m + 8, gave_up, sizeof(int), hipMemcpyDeviceToHost, s));
        ACC_HIP(hipStreamSynchronize(s));
        if (pin_m[8] == 0) {
            if (info_host) { info_host[0] = pin_m[4]; info_host[1] = pin_m[5]; }
            if (pin_m[FLAG_NONPOS]) return ACCBPG_ERR_ASSERT;     // y.min() > 0, functions.py:270
            return ACCBPG_OK;
        }
        g_prox_multi_off = true;                                // a wait timed out: one workgroup from here on
    }
    ACC_TRY(prox_enqueue_single(p.forced, y_dev, g_dev, L, eps, n, x_out_dev, ws_dev, g_flags, s));
    int* pin_i = reinterpret_cast<int*>(g_pin);
    ACC_HIP(hipMemcpyAsync(pin_i, g_flags, 6 * sizeof(int), hipMemcpyDeviceToHost, s));   // flags + info, one copy
    ACC_HIP(hipStreamSynchronize(s));
    if (info_host) { info_host[0] = pin_i[4]; info_host[1] = pin_i[5]; }
    if (pin_i[FLAG_NONPOS]) return ACCBPG_ERR_ASSERT;         // y.min() > 0, functions.py:270
    return ACCBPG_OK;
}

extern "C" int accbpg_debug_prox_variant(int variant) {
    if (variant < 0 || variant > 3) return ACCBPG_ERR_ARG;
    g_prox_variant.store(variant, std::memory_order_relaxed);
    return ACCBPG_OK;
}

extern "C" int accbpg_debug_prox_state(int* out3_host) {
    if (!out3_host) return ACCBPG_ERR_ARG;
    out3_host[0] = g_prox_last[0];
    out3_host[1] = g_prox_last[1];
    out3_host[2] = g_prox_multi_off ? 1 : 0;
    return ACCBPG_OK;
}

extern "C" int accbpg_burg_simplex_prox_acc(const double* xi_dev, double alpha, const double* g_dev, double L, double eps,
                                            int64_t n, double* xi_out_dev, double* x_out_dev, double* ws_dev,
                                            int* info_host, void* stream) {
    if (!xi_dev || !g_dev || !xi_out_dev || !x_out_dev || n <= 0 || !ws_dev) return ACCBPG_ERR_ARG;
    if (xi_out_dev == xi_dev || xi_out_dev == g_dev || x_out_dev == xi_out_dev) return ACCBPG_ERR_ARG;
    if (!(L > 0.0)) return ACCBPG_ERR_ASSERT;                 // functions.py:340
    hipStream_t s = (hipStream_t)stream;
    if (n > (int64_t)PB * 32) {
        // long vectors: the sum in a pass of its own (1.0*xi is exact), then the multi-workgroup prox as it is
        ACC_TRY(accbpg_vec_axpby(1.0, xi_dev, alpha, g_dev, n, xi_out_dev, stream));
        return accbpg_burg_simplex_div_prox(nullptr, xi_out_dev, L, eps, n, x_out_dev, ws_dev, info_host, stream);
    }
    ACC_TRY(ensure_scratch());
    int* g_info = g_flags + 4;
    if (n <= (int64_t)PB * 2)
        burg_prox_acc_kernel<2><<<1, PB, 0, s>>>(xi_dev, alpha, g_dev, L, eps, n, xi_out_dev, x_out_dev, g_info, g_flags);
    else if (n <= (int64_t)PB * 8)
        burg_prox_acc_kernel<8><<<1, PB, 0, s>>>(xi_dev, alpha, g_dev, L, eps, n, xi_out_dev, x_out_dev, g_info, g_flags);
    else
        burg_prox_acc_kernel<32><<<1, PB, 0, s>>>(xi_dev, alpha, g_dev, L, eps, n, xi_out_dev, x_out_dev, g_info, g_flags);
    ACC_HIP(hipGetLastError());
    if (!info_host) return ACCBPG_OK;                         // no y, so no flag can be raised: nothing to wait for
    int* pin_i = reinterpret_cast<int*>(g_pin);
    ACC_HIP(hipMemcpyAsync(pin_i, g_flags, 6 * sizeof(int), hipMemcpyDeviceToHost, s));
    ACC_HIP(hipStreamSynchronize(s));
    info_host[0] = pin_i[4]; info_host[1] = pin_i[5];
    return ACCBPG_OK;
}

extern "C" int accbpg_ls_terms(const double* g_dev, const double* x_dev, const double* y_dev, const double* z_dev,
                               const double* z1_dev, int64_t n, double* out_host, double* ws_dev, void* stream) {
    if (n <= 0 || !out_host || !ws_dev) return ACCBPG_ERR_ARG;
    if ((z_dev == nullptr) != (z1_dev == nullptr)) return ACCBPG_ERR_ARG;
    ACC_TRY(ensure_scratch());
    hipStream_t s = (hipStream_t)stream;
    const int nb = red_blocks(n, RMAXBLK);
    double* part = ws_dev + n;
    ls_terms_partial_kernel<<<nb, RB, 0, s>>>(g_dev, x_dev, y_dev, z_dev, z1_dev, n, 1, part);
    const double* o = finish4(part, nb, s);
    if (!o) return ACCBPG_ERR_HIP;
    out_host[0] = o[0]; out_host[1] = o[1]; out_host[2] = o[2];
    if (!(o[3] > 0.0)) return ACCBPG_ERR_ASSERT;              // functions.py:252
    return ACCBPG_OK;
}

extern "C" int accbpg_burg_divergence(const double* x_dev, const double* y_dev, int64_t n, double* out_host,
                                      double* ws_dev, void* stream) {
    if (!x_dev || !y_dev) return ACCBPG_ERR_ARG;
    double o[3];
    int rc = accbpg_ls_terms(nullptr, x_dev, y_dev, nullptr, nullptr, n, o, ws_dev, stream);
    if (out_host) out_host[0] = o[1];
    return rc;
}

extern "C" int accbpg_vec_dot_diff(const double* g_dev, const double* x_dev, const double* y_dev, int64_t n,
                                   double* out_host, double* ws_dev, void* stream) {
    if (!g_dev || !x_dev || !y_dev || n <= 0 || !out_host || !ws_dev) return ACCBPG_ERR_ARG;
    ACC_TRY(ensure_scratch());
    hipStream_t s = (hipStream_t)stream;
    const int nb = red_blocks(n, RMAXBLK);
    double* part = ws_dev + n;
    ls_terms_partial_kernel<<<nb, RB, 0, s>>>(g_dev, x_dev, y_dev, nullptr, nullptr, n, 0, part);
    const double* o = finish4(part, nb, s);
    if (!o) return ACCBPG_ERR_HIP;
    out_host[0] = o[0];
    return ACCBPG_OK;
}

extern "C" int accbpg_vec_min_sum(const double* x_dev, int64_t n, double* out_host, double* ws_dev, void* stream) {
    if (!x_dev || n <= 0 || !out_host || !ws_dev) return ACCBPG_ERR_ARG;
    ACC_TRY(ensure_scratch());
    hipStream_t s = (hipStream_t)stream;
    const int nb = red_blocks(n, RMAXBLK);
    double* part = ws_dev + n;
    min_sum_partial_kernel<<<nb, RB, 0, s>>>(x_dev, n, part);
    const double* o = finish4(part, nb, s);
    if (!o) return ACCBPG_ERR_HIP;
    out_host[0] = o[3];
    out_host[1] = o[0];
    return ACCBPG_OK;
}

extern "C" int accbpg_vec_axpby(double a, const double* x_dev, double b, const double* z_dev, int64_t n,
                                double* out_dev, void* stream) {
    if (!x_dev || !z_dev || !out_dev || n <= 0) return ACCBPG_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    axpby_kernel<<<ew_blocks(n), RB, 0, s>>>(a, x_dev, b, z_dev, n, out_dev);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

extern "C" int accbpg_vec_div_scalar(const double* x_dev, double d, int64_t n, double* out_dev, void* stream) {
    if (!x_dev || !out_dev || n <= 0) return ACCBPG_ERR_ARG;
    div_scalar_kernel<<<ew_blocks(n), RB, 0, (hipStream_t)stream>>>(x_dev, d, n, out_dev);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

extern "C" int accbpg_vec_vertex(int64_t idx, double value, double fill, int64_t n, double* out_dev, void* stream) {
    if (!out_dev || n <= 0 || idx < 0 || idx >= n) return ACCBPG_ERR_ARG;
    vertex_kernel<<<ew_blocks(n), RB, 0, (hipStream_t)stream>>>(idx, value, fill, n, out_dev);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

extern "C" int accbpg_vec_argminmax(const double* x_dev, int64_t n, int64_t* idx_host, double* val_host,
                                    double* ws_dev, void* stream) {
    if (!x_dev || n <= 0 || !idx_host || !ws_dev) return ACCBPG_ERR_ARG;
    ACC_TRY(ensure_scratch());
    hipStream_t s = (hipStream_t)stream;
    int nb = red_blocks(n, RMAXBLK);
    if (nb > 128) nb = 128;                                     // 128 records of 32 B = the 4096-double tail of ws
    MinMaxRec* part = reinterpret_cast<MinMaxRec*>(ws_dev + n + (n & 1));
    MinMaxRec* out = reinterpret_cast<MinMaxRec*>(g_out + 8);
    minmax_partial_kernel<<<nb, RB, 0, s>>>(x_dev, n, part);
    minmax_final_kernel<<<1, RB, 0, s>>>(part, nb, out);
    ACC_HIP(hipGetLastError());
    ACC_HIP(hipMemcpyAsync(g_pin + 16, out, sizeof(MinMaxRec), hipMemcpyDeviceToHost, s));
    ACC_HIP(hipStreamSynchronize(s));
    const MinMaxRec* r = reinterpret_cast<const MinMaxRec*>(g_pin + 16);
    idx_host[0] = r->imin;
    idx_host[1] = r->imax;
    if (val_host) { val_host[0] = r->vmin; val_host[1] = r->vmax; }
    return ACCBPG_OK;
}

extern "C" int accbpg_fw_direction(const double* g_dev, const double* x_dev, int lmo_kind, int center_kind,
                                   const double* center_dev, double center_val, double radius, int64_t n,
                                   double* s_out_dev, double* d_out_dev, double* out5_host, int64_t* idx_host,
                                   double* ws_dev, void* stream) {
    if (!g_dev || !x_dev || !s_out_dev || !d_out_dev || !out5_host || !idx_host || !ws_dev || n <= 0) return ACCBPG_ERR_ARG;
    if (lmo_kind < FWD_L2 || lmo_kind > FWD_SIMPLEX || center_kind < 0 || center_kind > 1) return ACCBPG_ERR_ARG;
    if (lmo_kind != FWD_SIMPLEX && center_kind == 1 && !center_dev) return ACCBPG_ERR_ARG;
    if (s_out_dev == d_out_dev || s_out_dev == g_dev || s_out_dev == x_dev || d_out_dev == g_dev || d_out_dev == x_dev)
        return ACCBPG_ERR_ARG;
    ACC_TRY(ensure_scratch());
    hipStream_t s = (hipStream_t)stream;
    const int nb = red_blocks(n, RMAXBLK);
    double* part = ws_dev + n;                                  // 3 * RMAXBLK doubles of phase 1, then 4 * nb of phase 2
    double* scal = g_out + 4;
    fw_dir_scan_kernel<<<nb, RB, 0, s>>>(g_dev, n, part);
    fw_dir_scan_final_kernel<<<1, RB, 0, s>>>(part, nb, scal);
    fw_dir_form_kernel<<<nb, RB, 0, s>>>(lmo_kind, g_dev, x_dev, center_kind, center_dev, center_val, radius, scal, n,
                                         s_out_dev, d_out_dev, part);
    // one final stage, one copy of {<g,d>, sum d^2, sum (s-c)^2, -, sum g^2, min g, argmin, centre} and one wait
    const double* o = reduce_finish(ls_terms_final_kernel, part, nb, g_out, g_out, 8, g_pin, s);
    if (!o) return ACCBPG_ERR_HIP;
    const bool centre = o[7] != 0.0;
    out5_host[0] = o[4];
    out5_host[1] = o[0];
    out5_host[2] = o[1];
    out5_host[3] = (lmo_kind == FWD_L2 && !centre) ? sqrt(o[2]) : 0.0;
    out5_host[4] = centre ? 1.0 : 0.0;
    int64_t imin;
    memcpy(&imin, &o[6], sizeof(imin));
    idx_host[0] = imin;
    if (lmo_kind == FWD_L2 && !centre && !(fabs(out5_host[3] - radius) <= 1e-10)) {    // functions_lmo.py:45-46
        set_last_error("Solution does not lie on ball boundary");
        return ACCBPG_ERR_ASSERT;
    }
    return ACCBPG_OK;
}

extern "C" int accbpg_vec_dot(const double* x_dev, const double* y_dev, int64_t n, double* out_host, double* ws_dev,
                              void* stream) {
    if (!x_dev || !y_dev || n <= 0 || !out_host || !ws_dev) return ACCBPG_ERR_ARG;
    ACC_TRY(ensure_scratch());
    hipStream_t s = (hipStream_t)stream;
    const int nb = red_blocks(n, RMAXBLK);
    double* part = ws_dev + n;
    dot_partial_kernel<<<nb, RB, 0, s>>>(x_dev, y_dev, n, part);
    const double* o = finish4(part, nb, s);
    if (!o) return ACCBPG_ERR_HIP;
    out_host[0] = o[0];
    return ACCBPG_OK;
}

extern "C" int accbpg_l1_norm(const double* x_dev, int64_t n, double* out_host, double* ws_dev, void* stream) {
    if (!x_dev || n <= 0 || !out_host || !ws_dev) return ACCBPG_ERR_ARG;
    ACC_TRY(ensure_scratch());
    hipStream_t s = (hipStream_t)stream;
    const int nb = red_blocks(n, RMAXBLK);
    double* part = ws_dev + n;
    l1_partial_kernel<<<nb, RB, 0, s>>>(x_dev, n, part);
    const double* o = finish4(part, nb, s);
    if (!o) return ACCBPG_ERR_HIP;
    out_host[0] = o[0];
    return ACCBPG_OK;
}

extern "C" int accbpg_sq_ls_terms(const double* g_dev, const double* x_dev, const double* y_dev, const double* z_dev,
                                  const double* z1_dev, int64_t n, double* out_host, double* ws_dev, void* stream) {
    if (!x_dev || !y_dev || n <= 0 || !out_host || !ws_dev) return ACCBPG_ERR_ARG;
    if ((z_dev == nullptr) != (z1_dev == nullptr)) return ACCBPG_ERR_ARG;
    ACC_TRY(ensure_scratch());
    hipStream_t s = (hipStream_t)stream;
    const int nb = red_blocks(n, RMAXBLK);
    double* part = ws_dev + n;
    sq_ls_partial_kernel<<<nb, RB, 0, s>>>(g_dev, x_dev, y_dev, z_dev, z1_dev, n, part);
    const double* o = finish4(part, nb, s);
    if (!o) return ACCBPG_ERR_HIP;
    out_host[0] = o[0];
    out_host[1] = 0.5 * o[1];
    out_host[2] = 0.5 * o[2];
    return ACCBPG_OK;
}

extern "C" int accbpg_l2l1linf_prox(const double* y_dev, const double* g_dev, double L, double lamda, double B,
                                    int64_t n, double* out_dev, void* stream) {
    if (!g_dev || !out_dev || n <= 0) return ACCBPG_ERR_ARG;
    if (!(L > 0.0)) {                                           // functions.py:821, :834
        set_last_error("L2L1Linf: L should be positive.");
        return ACCBPG_ERR_ASSERT;
    }
    const double invL = 1.0 / L, thr = lamda / L;
    l2l1linf_prox_kernel<<<ew_blocks(n), RB, 0, (hipStream_t)stream>>>(y_dev, g_dev, L, invL, thr, B, n, out_dev);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

extern "C" int accbpg_burg_reg_div_prox(int kind, const double* y_dev, const double* g_dev, double L, double lamda,
                                        int64_t n, double* x_out_dev, void* stream) {
    if (!g_dev || !x_out_dev || n <= 0 || kind < 0 || kind > 2) return ACCBPG_ERR_ARG;
    if (!(L > 0.0)) {                                           // functions.py:260, :270, :295, :320
        set_last_error("prox_map only takes positive L");
        return ACCBPG_ERR_ASSERT;
    }
    if (kind != 0 && !(lamda >= 0.0)) return ACCBPG_ERR_ARG;
    ACC_TRY(ensure_scratch());
    hipStream_t s = (hipStream_t)stream;
    ACC_HIP(hipMemsetAsync(g_flags, 0, 8 * sizeof(int), s));
    burg_reg_prox_kernel<<<ew_blocks(n), RB, 0, s>>>(kind, y_dev, g_dev, L, lamda, n, x_out_dev, g_flags);
    ACC_HIP(hipGetLastError());
    int* pin_i = reinterpret_cast<int*>(g_pin);
    ACC_HIP(hipMemcpyAsync(pin_i, g_flags, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    ACC_HIP(hipStreamSynchronize(s));
    if (pin_i[FLAG_NONPOS]) {                                   // y.min() > 0, functions.py:270
        set_last_error("Either y or L is not positive.");
        return ACCBPG_ERR_ASSERT;
    }
    if (pin_i[FLAG_BAD_G]) {                                    // functions.py:261 / :296
        set_last_error(kind == 1 ? "Not getting positive solution." : "BurgEntropy prox_map only takes positive value.");
        return ACCBPG_ERR_ASSERT;
    }
    return ACCBPG_OK;
}


// ------------------------------------------------------------------------------------------------------------
// Length-n kernels over the active instances of a batch (accbpg_dopt_batch_*): K x n arrays, row i = instance i.
// ------------------------------------------------------------------------------------------------------------
static int batch_vec_scratch(accbpg_dopt_batch* b) {
    if (b->vflags) return ACCBPG_OK;
    ACC_HIP(acc_malloc(&b->vflags, sizeof(int) * 8 * (size_t)b->K, "vflags"));
    ACC_HIP(hipMemsetAsync(b->vflags, 0, sizeof(int) * 8 * (size_t)b->K, b->stream));   // the stream of the launches that follow
    ACC_HIP(acc_malloc(&b->vout, sizeof(double) * 4 * (size_t)b->K, "vout"));
    ACC_HIP(acc_malloc(&b->vpart, sizeof(double) * 4 * RMAXBLK * (size_t)b->K, "vpart"));
    ACC_HIP(hipHostMalloc(&b->vpin, sizeof(double) * 8 * (size_t)b->K, hipHostMallocDefault));
    return ACCBPG_OK;
}

static BatchAct batch_active(const accbpg_dopt_batch* b, const int* active_host) {
    BatchAct act;
    for (int i = 0; i < b->K && i < BATCH_MAX; ++i)
        if (!active_host || active_host[i]) act.idx[act.n++] = i;
    return act;
}

/* x_out[i] <- BurgEntropySimplex.div_prox_map(y[i], g[i], L_host[i]) for the active instances (y_dev NULL: prox_map).
 * status_host[i]: ACCBPG_OK or ACCBPG_ERR_ASSERT (L <= 0, or min(y) <= 0).  info_host (optional, 2 ints per instance)
 * receives {bisection steps, Newton steps}. */
extern "C" int accbpg_dopt_batch_burg_simplex_div_prox(accbpg_dopt_batch* b, const double* y_dev, const double* g_dev,
                                                       int64_t ld, const double* L_host, double eps, double* x_out_dev,
                                                       const int* active_host, int* status_host, int* info_host) {
    if (!b || !g_dev || !x_out_dev || !L_host || !status_host || b->K > BATCH_MAX) return ACCBPG_ERR_ARG;
    const int64_t n = b->inst[0]->n;
    if (ld < n) return ACCBPG_ERR_ARG;
    ACC_TRY(batch_vec_scratch(b));
    BatchAct all = batch_active(b, active_host), act;
    BatchVals Ls;
    for (int a = 0; a < all.n; ++a) {                           // functions.py:270 / :340: L > 0 is checked before anything runs
        const int i = all.idx[a];
        Ls.v[i] = L_host[i];
        if (!(L_host[i] > 0.0)) status_host[i] = ACCBPG_ERR_ASSERT;
        else { status_host[i] = ACCBPG_OK; act.idx[act.n++] = i; }
    }
    if (act.n == 0) return ACCBPG_OK;
    hipStream_t s = b->stream;
    if (n > (int64_t)PB * 32) {
        // Long vectors: the single-instance prox spreads one instance over several workgroups with an order of
        // summation of its own (burg_prox_multi_kernel), which the one-workgroup-per-instance kernel below does not
        // reproduce.  Run the single-instance prox itself, instance by instance, so that a batch stays bit for bit
        // equal to its instances evaluated on their own.
        if (!b->vws) ACC_HIP(acc_malloc(&b->vws, sizeof(double) * (size_t)vec_ws_doubles(n), "vws"));
        for (int a = 0; a < act.n; ++a) {
            const int i = act.idx[a];
            int info[2] = {0, 0};
            const int rc = accbpg_burg_simplex_div_prox(y_dev ? y_dev + (size_t)i * ld : nullptr, g_dev + (size_t)i * ld,
                                                        L_host[i], eps, n, x_out_dev + (size_t)i * ld, b->vws, info, s);
            if (rc == ACCBPG_ERR_ASSERT) status_host[i] = ACCBPG_ERR_ASSERT;   // y.min() > 0, functions.py:270
            else if (rc != ACCBPG_OK) return rc;
            if (info_host) { info_host[2 * i] = info[0]; info_host[2 * i + 1] = info[1]; }
        }
        return ACCBPG_OK;
    }
    if (n <= (int64_t)PB * 2)
        burg_prox_batch_kernel<2><<<act.n, PB, 0, s>>>(act, y_dev, g_dev, ld, Ls, eps, n, x_out_dev, nullptr, b->vflags);
    else if (n <= (int64_t)PB * 8)
        burg_prox_batch_kernel<8><<<act.n, PB, 0, s>>>(act, y_dev, g_dev, ld, Ls, eps, n, x_out_dev, nullptr, b->vflags);
    else                                                        // n <= PB * 32: longer rows returned above
        burg_prox_batch_kernel<32><<<act.n, PB, 0, s>>>(act, y_dev, g_dev, ld, Ls, eps, n, x_out_dev, nullptr, b->vflags);
    ACC_HIP(hipGetLastError());
    int* pin_i = reinterpret_cast<int*>(b->vpin);
    ACC_HIP(hipMemcpyAsync(pin_i, b->vflags, sizeof(int) * 8 * (size_t)b->K, hipMemcpyDeviceToHost, s));
    ACC_HIP(hipStreamSynchronize(s));
    for (int a = 0; a < act.n; ++a) {
        const int i = act.idx[a];
        if (pin_i[8 * i + FLAG_NONPOS]) status_host[i] = ACCBPG_ERR_ASSERT;     // y.min() > 0, functions.py:270
        if (info_host) { info_host[2 * i] = pin_i[8 * i + 4]; info_host[2 * i + 1] = pin_i[8 * i + 5]; }
    }
    return ACCBPG_OK;
}

/* ABDA's dual-averaging step for the active instances (algorithms.py:483-485): gavg_out[i] <- gavg[i] + wgt_host[i] * g[i],
 * z_out[i] <- BurgEntropySimplex.prox_map(gavg_out[i] / csum_host[i], Lc_host[i]), one launch.  status_host[i]:
 * ACCBPG_OK or ACCBPG_ERR_ASSERT (Lc <= 0; nothing is written for that instance).  info_host (optional, 2 ints per
 * instance) receives {bisection steps, Newton steps}. */
extern "C" int accbpg_dopt_batch_burg_simplex_avg_prox(accbpg_dopt_batch* b, const double* gavg_dev, const double* g_dev,
                                                       int64_t ld, const double* wgt_host, const double* csum_host,
                                                       const double* Lc_host, double eps, double* gavg_out_dev,
                                                       double* z_out_dev, const int* active_host, int* status_host,
                                                       int* info_host) {
    if (!b || !gavg_dev || !g_dev || !wgt_host || !csum_host || !Lc_host || !gavg_out_dev || !z_out_dev || !status_host ||
        b->K > BATCH_MAX)
        return ACCBPG_ERR_ARG;
    if (gavg_out_dev == gavg_dev || gavg_out_dev == g_dev || z_out_dev == gavg_out_dev || z_out_dev == gavg_dev ||
        z_out_dev == g_dev)
        return ACCBPG_ERR_ARG;
    const int64_t n = b->inst[0]->n;
    if (ld < n) return ACCBPG_ERR_ARG;
    ACC_TRY(batch_vec_scratch(b));
    BatchAct all = batch_active(b, active_host), act;
    BatchVals wgt, csum, Lc;
    for (int a = 0; a < all.n; ++a) {                           // functions.py:340: L > 0 is checked before anything runs
        const int i = all.idx[a];
        wgt.v[i] = wgt_host[i]; csum.v[i] = csum_host[i]; Lc.v[i] = Lc_host[i];
        if (!(Lc_host[i] > 0.0)) status_host[i] = ACCBPG_ERR_ASSERT;
        else { status_host[i] = ACCBPG_OK; act.idx[act.n++] = i; }
    }
    if (act.n == 0) return ACCBPG_OK;
    hipStream_t s = b->stream;
    if (n > (int64_t)PB * 32) {
        // Long vectors: as in accbpg_dopt_batch_burg_simplex_div_prox, the multi-workgroup prox of the single instance
        // has its own order of summation.  Run what the sequential solver runs, instance by instance: the sum, the
        // quotient (into a scratch row), the prox.
        if (!b->vws) ACC_HIP(acc_malloc(&b->vws, sizeof(double) * (size_t)vec_ws_doubles(n), "vws"));
        if (!b->vquot) ACC_HIP(acc_malloc(&b->vquot, sizeof(double) * (size_t)n, "vquot"));
        for (int a = 0; a < act.n; ++a) {
            const int i = act.idx[a];
            const size_t row = (size_t)i * ld;
            int info[2] = {0, 0};
            ACC_TRY(accbpg_vec_axpby(1.0, gavg_dev + row, wgt_host[i], g_dev + row, n, gavg_out_dev + row, s));
            ACC_TRY(accbpg_vec_div_scalar(gavg_out_dev + row, csum_host[i], n, b->vquot, s));
            ACC_TRY(accbpg_burg_simplex_div_prox(nullptr, b->vquot, Lc_host[i], eps, n, z_out_dev + row, b->vws, info, s));
            if (info_host) { info_host[2 * i] = info[0]; info_host[2 * i + 1] = info[1]; }
        }
        return ACCBPG_OK;
    }
    if (n <= (int64_t)PB * 2)
        burg_avg_prox_batch_kernel<2><<<act.n, PB, 0, s>>>(act, gavg_dev, g_dev, ld, wgt, csum, Lc, eps, n, gavg_out_dev,
                                                           z_out_dev, b->vflags);
    else if (n <= (int64_t)PB * 8)
        burg_avg_prox_batch_kernel<8><<<act.n, PB, 0, s>>>(act, gavg_dev, g_dev, ld, wgt, csum, Lc, eps, n, gavg_out_dev,
                                                           z_out_dev, b->vflags);
    else                                                        // n <= PB * 32: longer rows returned above
        burg_avg_prox_batch_kernel<32><<<act.n, PB, 0, s>>>(act, gavg_dev, g_dev, ld, wgt, csum, Lc, eps, n, gavg_out_dev,
                                                            z_out_dev, b->vflags);
    ACC_HIP(hipGetLastError());
    if (!info_host) return ACCBPG_OK;                           // no y, so no flag can be raised: nothing to wait for
    int* pin_i = reinterpret_cast<int*>(b->vpin);
    ACC_HIP(hipMemcpyAsync(pin_i, b->vflags, sizeof(int) * 8 * (size_t)b->K, hipMemcpyDeviceToHost, s));
    ACC_HIP(hipStreamSynchronize(s));
    for (int a = 0; a < act.n; ++a) {
        const int i = act.idx[a];
        info_host[2 * i] = pin_i[8 * i + 4]; info_host[2 * i + 1] = pin_i[8 * i + 5];
    }
    return ACCBPG_OK;
}

/* out_host[3 i ..] <- { <g_i, x_i - y_i>, D_h(x_i, y_i), D_h(z_i, z1_i) } for the active instances (g, and z with z1,
 * may be NULL); status_host[i] = ACCBPG_ERR_ASSERT where an entry that enters a divergence is not positive. */
extern "C" int accbpg_dopt_batch_ls_terms(accbpg_dopt_batch* b, const double* g_dev, const double* x_dev, const double* y_dev,
                                          const double* z_dev, const double* z1_dev, int64_t ld, const int* active_host,
                                          double* out_host, int* status_host) {
    if (!b || !x_dev || !y_dev || !out_host || !status_host || b->K > BATCH_MAX) return ACCBPG_ERR_ARG;
    if ((z_dev == nullptr) != (z1_dev == nullptr)) return ACCBPG_ERR_ARG;
    const int64_t n = b->inst[0]->n;
    if (ld < n) return ACCBPG_ERR_ARG;
    ACC_TRY(batch_vec_scratch(b));
    const BatchAct act = batch_active(b, active_host);
    if (act.n == 0) return ACCBPG_OK;
    hipStream_t s = b->stream;
    const int nb = red_blocks(n, RMAXBLK);
    ls_terms_partial_batch_kernel<<<dim3(nb, act.n), RB, 0, s>>>(act, g_dev, x_dev, y_dev, z_dev, z1_dev, ld, n, b->vpart,
                                                                4 * RMAXBLK);
    ls_terms_final_batch_kernel<<<act.n, RB, 0, s>>>(act, b->vpart, 4 * RMAXBLK, nb, b->vout);
    ACC_HIP(hipGetLastError());
    ACC_HIP(hipMemcpyAsync(b->vpin, b->vout, sizeof(double) * 4 * (size_t)b->K, hipMemcpyDeviceToHost, s));
    ACC_HIP(hipStreamSynchronize(s));
    for (int a = 0; a < act.n; ++a) {
        const int i = act.idx[a];
        out_host[3 * i] = b->vpin[4 * i]; out_host[3 * i + 1] = b->vpin[4 * i + 1]; out_host[3 * i + 2] = b->vpin[4 * i + 2];
        status_host[i] = (b->vpin[4 * i + 3] > 0.0) ? ACCBPG_OK : ACCBPG_ERR_ASSERT;     // functions.py:252
    }
    return ACCBPG_OK;
}

/* out[i] <- a_host[i] * x[i] + b_host[i] * z[i] for the active instances, NumPy's rounding (algorithms.py:147,150). */
extern "C" int accbpg_dopt_batch_axpby(accbpg_dopt_batch* b, const double* a_host, const double* x_dev, const double* b_host,
                                       const double* z_dev, int64_t ld, const int* active_host, double* out_dev) {
    if (!b || !a_host || !b_host || !x_dev || !z_dev || !out_dev || b->K > BATCH_MAX) return ACCBPG_ERR_ARG;
    const int64_t n = b->inst[0]->n;
    if (ld < n) return ACCBPG_ERR_ARG;
    const BatchAct act = batch_active(b, active_host);
    if (act.n == 0) return ACCBPG_OK;
    BatchVals av, bv;
    for (int i = 0; i < b->K; ++i) { av.v[i] = a_host[i]; bv.v[i] = b_host[i]; }
    int64_t nb = (n + RB - 1) / RB;
    if (nb > 256) nb = 256;
    axpby_batch_kernel<<<dim3((unsigned)nb, act.n), RB, 0, b->stream>>>(act, av, x_dev, bv, z_dev, ld, n, out_dev);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}
