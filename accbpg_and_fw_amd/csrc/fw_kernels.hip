// Frank-Wolfe / Wolfe-Atwood step kernels for D-optimal design on gfx950.
// Replaces the loop bodies of D_opt_FW and D_opt_FW_away (accbpg/D_opt_alg.py:51-82, 135-179).
// Every kernel here is HBM- or latency-bound: the step reads V once (8*m*n bytes) for
// u = Hv^T V, reads and rewrites the m x m inverse H for the rank-one update, and makes a few
// passes over the length-n vectors.  Compiled with -ffp-contract=off (NumPy ufunc rounding).
#include "internal.h"
#include "reduce.hpp"
#include "fw_div_decide.hpp"
#include "fw_div_replay.hpp"

namespace accbpg {

constexpr int FB = 256;
constexpr int VG_COLS = 2 * FB;      // columns of V per workgroup in the V^T Hv pass
constexpr int VG_MAXSPLIT = 64;

// first-index-on-ties argmax / argmin, the NumPy convention (D_opt_alg.py:59,61,145,147); a NaN is the
// extremum for both (np.argmax / np.argmin return the first NaN)
__device__ __forceinline__ ValIdx better_max(ValIdx a, ValIdx b) {
    const bool an = a.v != a.v, bn = b.v != b.v;
    const bool take = (bn && !an) || (!an && b.v > a.v) || ((b.v == a.v || (an && bn)) && b.i < a.i);
    return take ? b : a;
}
__device__ __forceinline__ ValIdx better_min(ValIdx a, ValIdx b) {
    const bool an = a.v != a.v, bn = b.v != b.v;
    const bool take = (bn && !an) || (!an && b.v < a.v) || ((b.v == a.v || (an && bn)) && b.i < a.i);
    return take ? b : a;
}
__device__ __forceinline__ ValIdx shfl_down_vi(ValIdx a, int off) {
    ValIdx r;
    r.v = __shfl_down(a.v, off);
    r.i = __shfl_down((long long)a.i, off);
    return r;
}

template <bool IS_MAX, int NT>
__device__ __forceinline__ ValIdx block_reduce_vi_n(ValIdx a, ValIdx* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ValIdx o = shfl_down_vi(a, off);
        a = IS_MAX ? better_max(a, o) : better_min(a, o);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = a;
    __syncthreads();
    ValIdx r = sh[0];
    for (int i = 1; i < NT / 64; ++i) r = IS_MAX ? better_max(r, sh[i]) : better_min(r, sh[i]);
    return r;
}

// Probe, stage 1 (one pass over w and x, many workgroups): per-block first-index argmax of w and
// first-index argmin of w over the support mask (away: x > 1e-8, D_opt_alg.py:147; FW: x > 0, :60).
//
// For the Frank-Wolfe variant the masked minimum of w is all that is needed (only w_j enters eps_neg).  The
// away index j = argmin((w - w_i) * [x > 1e-8]) (:146-147) is taken on the ROUNDED differences, and two
// masked entries with different w can round to the same difference from a much larger w_i, in which case
// NumPy returns the first of them: stage 2 therefore evaluates that expression itself once w_i is known.
__device__ __forceinline__ void fw_probe_partial_body(const double* __restrict__ w,
                                                             const double* __restrict__ x, int64_t n, int away,
                                                             ValIdx* __restrict__ part) {
    __shared__ ValIdx sh[FB / 64];
    const double inf = __builtin_inf();
    const double thr = away ? 1.0e-8 : 0.0;
    ValIdx best{-inf, INT64_MAX}, lo{inf, INT64_MAX};
    const int64_t stride = (int64_t)gridDim.x * FB;
    for (int64_t k = (int64_t)blockIdx.x * FB + threadIdx.x; k < n; k += stride) {
        const double wk = w[k];
        best = better_max(best, ValIdx{wk, k});
        if (x[k] > thr) lo = better_min(lo, ValIdx{wk, k});
    }
    const ValIdx mx = block_reduce_vi_n<true, FB>(best, sh);
    const ValIdx mn = block_reduce_vi_n<false, FB>(lo, sh);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = mx;
        part[2 * blockIdx.x + 1] = mn;
    }
}

// stage 2: combine the partials (block order), resolve the all-zero case, fetch w_j and x_j
__device__ __forceinline__ void fw_probe_final_body(const ValIdx* __restrict__ part, int nblk,
                                                           const double* __restrict__ w,
                                                           const double* __restrict__ x, int64_t n, int away,
                                                           double* __restrict__ dout, int64_t* __restrict__ iout,
                                                           const double* __restrict__ qsrc) {
    // (dout / iout point into the handle's PINNED HOST record: the results -- and q of the last update, qsrc -- are
    //  written where the host reads them, no copy operation behind the kernel)
    __shared__ ValIdx sh[FB / 64];
    const double inf = __builtin_inf();
    ValIdx best{-inf, INT64_MAX}, lo{inf, INT64_MAX};
    for (int b = threadIdx.x; b < nblk; b += FB) {
        best = better_max(best, part[2 * b]);
        lo = better_min(lo, part[2 * b + 1]);
    }
    const ValIdx mx = block_reduce_vi_n<true, FB>(best, sh);
    ValIdx mn = block_reduce_vi_n<false, FB>(lo, sh);
    if (away) {
        // d_k = (w_k - w_i) * [x_k > 1e-8] exactly as the reference forms it (one subtraction, one product with
        // 1.0 or 0.0), first index of its minimum.  One workgroup over 2n doubles: a few microseconds at the
        // sizes the away variant runs at, next to a factorisation of H per iteration.
        ValIdx dm{inf, INT64_MAX};
        for (int64_t k = threadIdx.x; k < n; k += FB) {
            const double diff = w[k] - mx.v;
            const double dk = diff * ((x[k] > 1.0e-8) ? 1.0 : 0.0);
            dm = better_min(dm, ValIdx{dk, k});
        }
        mn = block_reduce_vi_n<false, FB>(dm, sh);
    }
    if (threadIdx.x == 0) {
        const int64_t j = mn.i;
        iout[0] = mx.i;
        iout[1] = j;
        dout[0] = mx.v;
        const bool ok = j >= 0 && j < n;
        dout[1] = ok ? w[j] : inf;
        dout[2] = ok ? x[j] : 0.0;
        dout[6] = *qsrc;
    }
}

// Away variant, stage 2 on many workgroups (one workgroup scanning 2n doubles took 40 us of a 170 us step at n = 32768):
// every workgroup combines the stage-1 maxima itself (at most 512 records: the same w_i everywhere), then takes the
// first-index minimum of d_k = (w_k - w_i) * [x_k > 1e-8] -- formed exactly as the reference forms it, D_opt_alg.py:146-147
// -- over its slice; workgroup 0 leaves (w_i, i) for the final stage.
__device__ __forceinline__ void fw_probe_away_partial_body(const ValIdx* __restrict__ part, int nblk,
                                                                  const double* __restrict__ w,
                                                                  const double* __restrict__ x, int64_t n,
                                                                  ValIdx* __restrict__ part2, ValIdx* __restrict__ mxslot) {
    __shared__ ValIdx sh[FB / 64];
    const double inf = __builtin_inf();
    ValIdx best{-inf, INT64_MAX};
    for (int b = threadIdx.x; b < nblk; b += FB) best = better_max(best, part[2 * b]);
    const ValIdx mx = block_reduce_vi_n<true, FB>(best, sh);
    ValIdx dm{inf, INT64_MAX};
    const int64_t per = (n + gridDim.x - 1) / gridDim.x;
    const int64_t k0 = (int64_t)blockIdx.x * per, k1 = min(n, k0 + per);
    for (int64_t k = k0 + threadIdx.x; k < k1; k += FB) {
        const double diff = w[k] - mx.v;
        const double dk = diff * ((x[k] > 1.0e-8) ? 1.0 : 0.0);
        dm = better_min(dm, ValIdx{dk, k});
    }
    const ValIdx mn = block_reduce_vi_n<false, FB>(dm, sh);
    if (threadIdx.x == 0) {
        part2[blockIdx.x] = mn;
        if (blockIdx.x == 0) *mxslot = mx;
    }
}
__device__ __forceinline__ void fw_probe_away_final_body(const ValIdx* __restrict__ part2, int nb2,
                                                                const ValIdx* __restrict__ mxslot,
                                                                const double* __restrict__ w,
                                                                const double* __restrict__ x, int64_t n,
                                                                double* __restrict__ dout, int64_t* __restrict__ iout,
                                                                const double* __restrict__ qsrc) {
    __shared__ ValIdx sh[FB / 64];
    const double inf = __builtin_inf();
    ValIdx dm{inf, INT64_MAX};
    for (int b = threadIdx.x; b < nb2; b += FB) dm = better_min(dm, part2[b]);
    const ValIdx mn = block_reduce_vi_n<false, FB>(dm, sh);
    if (threadIdx.x == 0) {
        const ValIdx mx = *mxslot;
        const int64_t j = mn.i;
        iout[0] = mx.i;
        iout[1] = j;
        dout[0] = mx.v;
        const bool ok = j >= 0 && j < n;
        dout[1] = ok ? w[j] : inf;
        dout[2] = ok ? x[j] : 0.0;
        dout[6] = *qsrc;
    }
}

// x <- x*xscale; x[p] += xadd   (D_opt_alg.py:76-77,164-165,173-174); vp <- V[:,p]
__device__ __forceinline__ void fw_xupdate_gather_body(double* __restrict__ x, int64_t n, int64_t p,
                                                              double xscale, double xadd,
                                                              const double* __restrict__ V, int64_t ldv, int64_t m,
                                                              double* __restrict__ vp) {
    const int64_t stride = (int64_t)gridDim.x * FB;
    for (int64_t k = (int64_t)blockIdx.x * FB + threadIdx.x; k < n; k += stride) {
        double v = x[k] * xscale;
        if (k == p) v += xadd;
        x[k] = v;
    }
    for (int64_t r = (int64_t)blockIdx.x * FB + threadIdx.x; r < m; r += stride) vp[r] = V[r * ldv + p];
}

// hv = H vp, one wave per row of H          (np.dot(H, V[:,i]), D_opt_alg.py:78,166,175)
__device__ __forceinline__ void fw_gemv_h_body(const double* __restrict__ H, int64_t m,
                                                      const double* __restrict__ vp, double* __restrict__ hv) {
    // one wave per PAIR of rows (twice the loads in flight per wave; the per-row summation order is that of one
    // row per wave)
    const int lane = threadIdx.x & 63;
    const int64_t row = 2 * ((int64_t)blockIdx.x * (FB / 64) + (threadIdx.x >> 6));
    if (row >= m) return;
    const bool two = row + 1 < m;
    const double* hr = H + row * m;
    const double* hq = two ? hr + m : hr;
    double s = 0.0, t = 0.0;
    if ((m & 1) == 0) {
        // 16-byte loads, four independent accumulators per row (H rows are 16-byte aligned when m is even)
        const double2* h2 = reinterpret_cast<const double2*>(hr);
        const double2* q2 = reinterpret_cast<const double2*>(hq);
        const double2* v2 = reinterpret_cast<const double2*>(vp);
        const int64_t n2 = m >> 1;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
        int64_t c = lane;
        for (; c + 64 < n2; c += 128) {
            const double2 a = h2[c], b = h2[c + 64], p = q2[c], q = q2[c + 64], x = v2[c], y = v2[c + 64];
            s0 = fma(a.x, x.x, s0); s1 = fma(a.y, x.y, s1);
            s2 = fma(b.x, y.x, s2); s3 = fma(b.y, y.y, s3);
            t0 = fma(p.x, x.x, t0); t1 = fma(p.y, x.y, t1);
            t2 = fma(q.x, y.x, t2); t3 = fma(q.y, y.y, t3);
        }
        for (; c < n2; c += 64) {
            const double2 a = h2[c], p = q2[c], x = v2[c];
            s0 = fma(a.x, x.x, s0); s1 = fma(a.y, x.y, s1);
            t0 = fma(p.x, x.x, t0); t1 = fma(p.y, x.y, t1);
        }
        s = (s0 + s1) + (s2 + s3);
        t = (t0 + t1) + (t2 + t3);
    } else {
        for (int64_t c = lane; c < m; c += 64) {
            s = fma(hr[c], vp[c], s);
            t = fma(hq[c], vp[c], t);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off);
        t += __shfl_down(t, off);
    }
    if (lane == 0) {
        hv[row] = s;
        if (two) hv[row + 1] = t;
    }
}

// H <- (H + hcoef*outer(hv,hv)) / hdiv       (D_opt_alg.py:79,167,176); a row per workgroup pass
// Workgroup 0 also leaves q = v_p^T (H v_p), the quadratic form of the pivot column in the inverse AS MAINTAINED (the
// tracked w_p drifts away from it: w is never refreshed, D_opt_alg.py:82): by the matrix determinant lemma
// det(H+) = det(H) (1 + hcoef q) / hdiv^m holds for exactly this q, which is what the log-space advance of log det(H)
// between two factorisations uses (accbpg_fw_probe: q_prev).
__device__ __forceinline__ void fw_rank1_body(double* __restrict__ H, int64_t m,
                                                     const double* __restrict__ hv, double hcoef, double hdiv,
                                                     const double* __restrict__ vp, double* __restrict__ qout) {
    if (blockIdx.x == 0) {
        __shared__ double qs[FB / 64];
        double q = 0.0;
        for (int64_t c = threadIdx.x; c < m; c += FB) q = fma(vp[c], hv[c], q);
        q = wave_sum(q);
        if ((threadIdx.x & 63) == 0) qs[threadIdx.x >> 6] = q;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = qs[0];
            for (int i = 1; i < FB / 64; ++i) t += qs[i];
            *qout = t;
        }
    }
    for (int64_t r = blockIdx.x; r < m; r += gridDim.x) {
        const double hr = hv[r];
        double* row = H + r * m;
        if ((m & 1) == 0) {
            double2* row2 = reinterpret_cast<double2*>(row);
            const double2* hv2 = reinterpret_cast<const double2*>(hv);
            for (int64_t c = threadIdx.x; c < (m >> 1); c += FB) {
                double2 a = row2[c];
                const double2 b = hv2[c];
                const double o0 = hr * b.x, o1 = hr * b.y;
                const double t0 = hcoef * o0, t1 = hcoef * o1;
                a.x = (a.x + t0) / hdiv;
                a.y = (a.y + t1) / hdiv;
                row2[c] = a;
            }
        } else {
            for (int64_t c = threadIdx.x; c < m; c += FB) {
                const double o = hr * hv[c];
                const double t = hcoef * o;
                row[c] = (row[c] + t) / hdiv;
            }
        }
    }
}

// partial u[s][k] = sum over the rows of split s of hv[r]*V[r][k]; two columns per thread
__device__ __forceinline__ void fw_vgemv_partial_body(const double* __restrict__ V, int64_t ldv, int64_t m,
                                                             int64_t n, const double* __restrict__ hv, int nsplit,
                                                             double* __restrict__ upart, bool vec_ok) {
    const int64_t k = (int64_t)blockIdx.x * VG_COLS + 2 * threadIdx.x;
    const int s = blockIdx.y;
    const int64_t rows_per = (m + nsplit - 1) / nsplit;
    const int64_t r0 = (int64_t)s * rows_per, r1 = min(m, r0 + rows_per);
    if (k >= n) return;
    double a0 = 0.0, a1 = 0.0;
    const bool pair = vec_ok && (k + 1 < n);
    if (pair) {
        const double* vp = V + r0 * ldv + k;
#pragma unroll 8
        for (int64_t r = r0; r < r1; ++r) {
            // V is streamed once per pass (512 MiB at config 3): non-temporal loads keep it out of the caches
            const double2 v = double2{__builtin_nontemporal_load(vp), __builtin_nontemporal_load(vp + 1)};
            const double h = hv[r];
            a0 = fma(h, v.x, a0);
            a1 = fma(h, v.y, a1);
            vp += ldv;
        }
    } else {
        for (int64_t r = r0; r < r1; ++r) {
            const double h = hv[r];
            a0 = fma(h, V[r * ldv + k], a0);
            if (k + 1 < n) a1 = fma(h, V[r * ldv + k + 1], a1);
        }
    }
    upart[(int64_t)s * n + k] = a0;
    if (k + 1 < n) upart[(int64_t)s * n + k + 1] = a1;
}

// w <- (w + hcoef * u^2) / hdiv with u = sum of the partials     (D_opt_alg.py:82,170,179)
__global__ __launch_bounds__(FB) void fw_wupdate_kernel(double* __restrict__ w, int64_t n,
                                                       const double* __restrict__ upart, int nsplit, double hcoef,
                                                       double hdiv) {
    const int64_t stride = (int64_t)gridDim.x * FB;
    for (int64_t k = (int64_t)blockIdx.x * FB + threadIdx.x; k < n; k += stride) {
        double u = 0.0;
        for (int s = 0; s < nsplit; ++s) u += upart[(int64_t)s * n + k];
        const double sq = u * u;
        const double t = hcoef * sq;
        w[k] = (w[k] + t) / hdiv;
    }
}

// The same update fused with stage 1 of the NEXT iteration's probe (fw_probe_partial_kernel): the new w
// is in registers anyway, x was updated earlier in this step.
__device__ __forceinline__ void fw_wupdate_probe_body(double* __restrict__ w, int64_t n,
                                                             const double* __restrict__ upart, int nsplit,
                                                             double hcoef, double hdiv,
                                                             const double* __restrict__ x, int away,
                                                             ValIdx* __restrict__ part) {
    __shared__ ValIdx sh[FB / 64];
    const double inf = __builtin_inf();
    const double thr = away ? 1.0e-8 : 0.0;
    ValIdx best{-inf, INT64_MAX}, lo{inf, INT64_MAX};
    const int64_t stride = (int64_t)gridDim.x * FB;
    for (int64_t k = (int64_t)blockIdx.x * FB + threadIdx.x; k < n; k += stride) {
        double u = 0.0;
        for (int s = 0; s < nsplit; ++s) u += upart[(int64_t)s * n + k];
        const double sq = u * u;
        const double t = hcoef * sq;
        const double wk = (w[k] + t) / hdiv;
        w[k] = wk;
        best = better_max(best, ValIdx{wk, k});
        if (x[k] > thr) lo = better_min(lo, ValIdx{wk, k});
    }
    const ValIdx mx = block_reduce_vi_n<true, FB>(best, sh);
    const ValIdx mn = block_reduce_vi_n<false, FB>(lo, sh);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = mx;
        part[2 * blockIdx.x + 1] = mn;
    }
}

// ---- the step kernels: one instance (the handle's pointers as arguments) ----------------------------------------
// Each is a thin wrapper round the body above; the lock-step forms below wrap the SAME bodies, so an instance of a
// batch goes through the very arithmetic, partition and summation order of the single handle.
__global__ __launch_bounds__(FB) void fw_probe_partial_kernel(const double* __restrict__ w,
                                                             const double* __restrict__ x, int64_t n, int away,
                                                             ValIdx* __restrict__ part) {
    fw_probe_partial_body(w, x, n, away, part);
}
__global__ __launch_bounds__(FB) void fw_probe_final_kernel(const ValIdx* __restrict__ part, int nblk,
                                                           const double* __restrict__ w,
                                                           const double* __restrict__ x, int64_t n, int away,
                                                           double* __restrict__ dout, int64_t* __restrict__ iout,
                                                           const double* __restrict__ qsrc) {
    fw_probe_final_body(part, nblk, w, x, n, away, dout, iout, qsrc);
}
__global__ __launch_bounds__(FB) void fw_probe_away_partial_kernel(const ValIdx* __restrict__ part, int nblk,
                                                                  const double* __restrict__ w,
                                                                  const double* __restrict__ x, int64_t n,
                                                                  ValIdx* __restrict__ part2, ValIdx* __restrict__ mxslot) {
    fw_probe_away_partial_body(part, nblk, w, x, n, part2, mxslot);
}
__global__ __launch_bounds__(FB) void fw_probe_away_final_kernel(const ValIdx* __restrict__ part2, int nb2,
                                                                const ValIdx* __restrict__ mxslot,
                                                                const double* __restrict__ w,
                                                                const double* __restrict__ x, int64_t n,
                                                                double* __restrict__ dout, int64_t* __restrict__ iout,
                                                                const double* __restrict__ qsrc) {
    fw_probe_away_final_body(part2, nb2, mxslot, w, x, n, dout, iout, qsrc);
}
__global__ __launch_bounds__(FB) void fw_xupdate_gather_kernel(double* __restrict__ x, int64_t n, int64_t p,
                                                              double xscale, double xadd,
                                                              const double* __restrict__ V, int64_t ldv, int64_t m,
                                                              double* __restrict__ vp) {
    fw_xupdate_gather_body(x, n, p, xscale, xadd, V, ldv, m, vp);
}
__global__ __launch_bounds__(FB) void fw_gemv_h_kernel(const double* __restrict__ H, int64_t m,
                                                      const double* __restrict__ vp, double* __restrict__ hv) {
    fw_gemv_h_body(H, m, vp, hv);
}
__global__ __launch_bounds__(FB) void fw_rank1_kernel(double* __restrict__ H, int64_t m,
                                                     const double* __restrict__ hv, double hcoef, double hdiv,
                                                     const double* __restrict__ vp, double* __restrict__ qout) {
    fw_rank1_body(H, m, hv, hcoef, hdiv, vp, qout);
}
__global__ __launch_bounds__(FB) void fw_vgemv_partial_kernel(const double* __restrict__ V, int64_t ldv, int64_t m,
                                                             int64_t n, const double* __restrict__ hv, int nsplit,
                                                             double* __restrict__ upart, bool vec_ok) {
    fw_vgemv_partial_body(V, ldv, m, n, hv, nsplit, upart, vec_ok);
}
__global__ __launch_bounds__(FB) void fw_wupdate_probe_kernel(double* __restrict__ w, int64_t n,
                                                             const double* __restrict__ upart, int nsplit,
                                                             double hcoef, double hdiv,
                                                             const double* __restrict__ x, int away,
                                                             ValIdx* __restrict__ part) {
    fw_wupdate_probe_body(w, n, upart, nsplit, hcoef, hdiv, x, away, part);
}

// ---- the step kernels: the active instances of a batch in lock-step ----------------------------------------------
// The instance is a grid dimension (blockIdx.z for the pass over V, whose blockIdx.y is the row split; blockIdx.y
// elsewhere); blockIdx.x and gridDim.x are what the single launch of that instance has, so the bodies partition and
// sum as they do there.  Pointers come from the batch's device table (FwInst), the active set and the per-instance
// scalars travel by value in the kernel arguments: no second synchronisation per step.  What lies behind t.hv and the
// layout of a probe record are the accessors next to FwInst (internal.h), here and on the host.
__global__ __launch_bounds__(FB) void fw_probe_partial_batch_kernel(const FwInst* __restrict__ tab, BatchAct act,
                                                                   int64_t m, int64_t n, int away) {
    const FwInst t = tab[act.idx[blockIdx.y]];
    fw_probe_partial_body(t.w, t.x, n, away, fw_part_of(t, m));
}
__global__ __launch_bounds__(FB) void fw_probe_final_batch_kernel(const FwInst* __restrict__ tab, FwProbeArgs pa,
                                                                 int64_t m, int64_t n, int away) {
    const FwInst t = tab[pa.idx[blockIdx.y]];
    fw_probe_final_body(fw_part_of(t, m), pa.nblk[blockIdx.y], t.w, t.x, n, away, fw_rec_d(t.rec),
                        fw_rec_i(t.rec), t.q);
}
__global__ __launch_bounds__(FB) void fw_probe_away_partial_batch_kernel(const FwInst* __restrict__ tab, FwProbeArgs pa,
                                                                        int64_t m, int64_t n) {
    const FwInst t = tab[pa.idx[blockIdx.y]];
    fw_probe_away_partial_body(fw_part_of(t, m), pa.nblk[blockIdx.y], t.w, t.x, n, fw_part2_of(t, m), fw_mxslot_of(t, m));
}
__global__ __launch_bounds__(FB) void fw_probe_away_final_batch_kernel(const FwInst* __restrict__ tab, FwProbeArgs pa,
                                                                      int nb2, int64_t m, int64_t n) {
    const FwInst t = tab[pa.idx[blockIdx.y]];
    fw_probe_away_final_body(fw_part2_of(t, m), nb2, fw_mxslot_of(t, m), t.w, t.x, n, fw_rec_d(t.rec), fw_rec_i(t.rec),
                             t.q);
}
__global__ __launch_bounds__(FB) void fw_xupdate_gather_batch_kernel(const FwInst* __restrict__ tab, FwUpdArgs ua,
                                                                    int64_t m, int64_t n, int64_t ldv) {
    const int a = blockIdx.y;
    const FwInst t = tab[ua.idx[a]];
    fw_xupdate_gather_body(t.x, n, ua.p[a], ua.xscale[a], ua.xadd[a], t.V, ldv, m, fw_vp_of(t, m));
}
__global__ __launch_bounds__(FB) void fw_gemv_h_batch_kernel(const FwInst* __restrict__ tab, BatchAct act, int64_t m) {
    const FwInst t = tab[act.idx[blockIdx.y]];
    fw_gemv_h_body(t.H, m, fw_vp_of(t, m), t.hv);
}
__global__ __launch_bounds__(FB) void fw_rank1_batch_kernel(const FwInst* __restrict__ tab, FwUpdArgs ua, int64_t m) {
    const int a = blockIdx.y;
    const FwInst t = tab[ua.idx[a]];
    fw_rank1_body(t.H, m, t.hv, ua.hcoef[a], ua.hdiv[a], fw_vp_of(t, m), t.q);
}
__global__ __launch_bounds__(FB) void fw_vgemv_partial_batch_kernel(const FwInst* __restrict__ tab, BatchAct act,
                                                                   int64_t ldv, int64_t m, int64_t n, int nsplit) {
    const FwInst t = tab[act.idx[blockIdx.z]];
    fw_vgemv_partial_body(t.V, ldv, m, n, t.hv, nsplit, t.vws, t.vec_ok != 0);
}
__global__ __launch_bounds__(FB) void fw_wupdate_probe_batch_kernel(const FwInst* __restrict__ tab, FwUpdArgs ua,
                                                                   int64_t m, int64_t n, int nsplit) {
    const int a = blockIdx.y;
    const FwInst t = tab[ua.idx[a]];
    fw_wupdate_probe_body(t.w, n, t.vws, nsplit, ua.hcoef[a], ua.hdiv[a], t.x, (int)((ua.awaymask >> a) & 1ull),
                          fw_part_of(t, m));
}

// ---- the step kernels: several iterations per host round trip (accbpg_fw_run) -----------------------------------
// The "run" forms wrap the SAME bodies on the single handle's grids.  The scalars of the step come from the handle's
// FwRun in device memory instead of the kernel arguments, and every kernel returns at once when that record says the
// run has stopped (the load is the same for every thread of the grid: the branch is uniform).  Thread 0 of the probe's
// final stage takes the decisions of the iteration -- D_opt_alg.py:63-82 and :150-179, operation for operation as
// _fw_decide and _AwayRun.iterate of the Python package write them; this file is compiled with -ffp-contract=off --
// writes FwRun for the update kernels behind it and the record of the step straight into the pinned host array.
__device__ __forceinline__ int fw_run_stop(const FwRun* run) {
    return *reinterpret_cast<const volatile int32_t*>(&run->stop);
}
__device__ __forceinline__ void fw_run_decide(FwRun* run, const double* rec, int64_t m, int64_t n, int away, double eps,
                                              accbpg_fw_step* __restrict__ out) {
    // rec: the scratch record the body has just written (this thread wrote it), laid out as the pinned record is
    const int64_t* irec = reinterpret_cast<const int64_t*>(rec + 8);
    const int64_t i = irec[0], j = irec[1];
    const double w_i = rec[4], w_j = rec[5], x_j = rec[6], q_prev = rec[10];
    const double md = (double)m;
    const double eps_pos = w_i / md - 1.0;                      // :63, :150
    const double eps_neg = 1.0 - w_j / md;                      // :64, :151
    accbpg_fw_step st;
    st.i = i; st.j = j; st.w_i = w_i; st.w_j = w_j; st.x_j = x_j; st.q_prev = q_prev;
    st.p = -1; st.xscale = 0.0; st.xadd = 0.0; st.hcoef = 0.0; st.hdiv = 0.0;
    st.kind = -1; st.status = 1;
    if (!(eps_pos <= eps && eps_neg <= eps)) {                  // :72, :159 (a NaN does not stop)
        int64_t p;
        double xscale, xadd, hcoef, hdiv;
        int kind;
        if (!away || eps_pos >= eps_neg) {                      // :162 (a NaN takes the away branch)
            const double t = (w_i / md - 1.0) / (w_i - 1.0);    // :75, :163
            const double coef = away ? t / (1.0 - t + t * w_i)  // :167
                                     : t / (1.0 + t * (w_i - 1.0));   // :79
            p = i; xscale = 1.0 - t; xadd = t; hcoef = -coef; hdiv = 1.0 - t; kind = 0;
        } else {
            const double a = (1.0 - w_j / md) / (w_j - 1.0);    // :172
            const double b = x_j / (1.0 - x_j);
            const double t = (b < a) ? b : a;                   // Python's min(a, b)
            const double coef = t / (1.0 + t - t * w_j);        // :176
            p = j; xscale = 1.0 + t; xadd = -t; hcoef = coef; hdiv = 1.0 + t; kind = 1;
        }
        st.p = p; st.xscale = xscale; st.xadd = xadd; st.hcoef = hcoef; st.hdiv = hdiv; st.kind = kind;
        st.status = (p >= 0 && p < n) ? 0 : 2;
        if (st.status == 0) {
            run->p = p; run->xscale = xscale; run->xadd = xadd; run->hcoef = hcoef; run->hdiv = hdiv;
        }
    }
    if (st.status != 0) *reinterpret_cast<volatile int32_t*>(&run->stop) = st.status;
    *out = st;
}
__global__ __launch_bounds__(FB) void fw_probe_final_run_kernel(FwRun* run, const ValIdx* __restrict__ part, int nblk,
                                                               const double* __restrict__ w,
                                                               const double* __restrict__ x, int64_t m, int64_t n,
                                                               int away, double eps, double* rec,
                                                               const double* __restrict__ qsrc,
                                                               accbpg_fw_step* __restrict__ out) {
    if (fw_run_stop(run)) return;
    fw_probe_final_body(part, nblk, w, x, n, away, fw_rec_d(rec), fw_rec_i(rec), qsrc);
    if (threadIdx.x == 0) fw_run_decide(run, rec, m, n, away, eps, out);
}
__global__ __launch_bounds__(FB) void fw_probe_away_partial_run_kernel(const FwRun* run, const ValIdx* __restrict__ part,
                                                                      int nblk, const double* __restrict__ w,
                                                                      const double* __restrict__ x, int64_t n,
                                                                      ValIdx* __restrict__ part2,
                                                                      ValIdx* __restrict__ mxslot) {
    if (fw_run_stop(run)) return;
    fw_probe_away_partial_body(part, nblk, w, x, n, part2, mxslot);
}
__global__ __launch_bounds__(FB) void fw_probe_away_final_run_kernel(FwRun* run, const ValIdx* __restrict__ part2, int nb2,
                                                                    const ValIdx* __restrict__ mxslot,
                                                                    const double* __restrict__ w,
                                                                    const double* __restrict__ x, int64_t m, int64_t n,
                                                                    double eps, double* rec,
                                                                    const double* __restrict__ qsrc,
                                                                    accbpg_fw_step* __restrict__ out) {
    if (fw_run_stop(run)) return;
    fw_probe_away_final_body(part2, nb2, mxslot, w, x, n, fw_rec_d(rec), fw_rec_i(rec), qsrc);
    if (threadIdx.x == 0) fw_run_decide(run, rec, m, n, 1, eps, out);
}
__global__ __launch_bounds__(FB) void fw_xupdate_gather_run_kernel(const FwRun* __restrict__ run, double* __restrict__ x,
                                                                  int64_t n, const double* __restrict__ V, int64_t ldv,
                                                                  int64_t m, double* __restrict__ vp) {
    const FwRun r = *run;
    if (r.stop) return;
    fw_xupdate_gather_body(x, n, r.p, r.xscale, r.xadd, V, ldv, m, vp);
}
__global__ __launch_bounds__(FB) void fw_gemv_h_run_kernel(const FwRun* __restrict__ run, const double* __restrict__ H,
                                                          int64_t m, const double* __restrict__ vp,
                                                          double* __restrict__ hv) {
    if (run->stop) return;
    fw_gemv_h_body(H, m, vp, hv);
}
__global__ __launch_bounds__(FB) void fw_rank1_run_kernel(const FwRun* __restrict__ run, double* __restrict__ H, int64_t m,
                                                         const double* __restrict__ hv, const double* __restrict__ vp,
                                                         double* __restrict__ qout) {
    const FwRun r = *run;
    if (r.stop) return;
    fw_rank1_body(H, m, hv, r.hcoef, r.hdiv, vp, qout);
}
__global__ __launch_bounds__(FB) void fw_vgemv_partial_run_kernel(const FwRun* __restrict__ run,
                                                                 const double* __restrict__ V, int64_t ldv, int64_t m,
                                                                 int64_t n, const double* __restrict__ hv, int nsplit,
                                                                 double* __restrict__ upart, bool vec_ok) {
    if (run->stop) return;
    fw_vgemv_partial_body(V, ldv, m, n, hv, nsplit, upart, vec_ok);
}
__global__ __launch_bounds__(FB) void fw_wupdate_probe_run_kernel(const FwRun* __restrict__ run, double* __restrict__ w,
                                                                 int64_t n, const double* __restrict__ upart, int nsplit,
                                                                 const double* __restrict__ x, int away,
                                                                 ValIdx* __restrict__ part) {
    const FwRun r = *run;
    if (r.stop) return;
    fw_wupdate_probe_body(w, n, upart, nsplit, r.hcoef, r.hdiv, x, away, part);
}

// ---- the step kernels: several iterations per host round trip for the active instances of a batch ---------------
// (accbpg_dopt_batch_fw_run)  The "batch-run" forms are the two families above at once: the instance is the grid
// dimension of the lock-step forms and its pointers come from the batch's table; the scalars of its step come from its
// own FwRunSlot, and a workgroup returns at once when ITS instance has stopped (one load per workgroup, the same for
// all its threads) while the workgroups of the other instances go on.  blockIdx.x / gridDim.x, the row split, vec_ok,
// the stage-1 area and AWAY_NB are the single launch's; thread 0 of an instance's final stage calls fw_run_decide with
// that instance's eps and writes record k of that instance's row of the pinned array.
__global__ __launch_bounds__(FB) void fw_probe_final_brun_kernel(const FwInst* __restrict__ tab, FwRunSlot* runs,
                                                                FwProbeArgs pa, ::BatchVals eps, int64_t m, int64_t n,
                                                                int away, accbpg_fw_step* steps, int k) {
    const int a = blockIdx.y, i = pa.idx[a];
    FwRunSlot* sl = runs + i;
    if (fw_run_stop(&sl->run)) return;
    const FwInst t = tab[i];
    fw_probe_final_body(fw_part_of(t, m), pa.nblk[a], t.w, t.x, n, away, fw_rec_d(sl->rec),
                        fw_rec_i(sl->rec), t.q);
    if (threadIdx.x == 0)
        fw_run_decide(&sl->run, sl->rec, m, n, away, eps.v[a], steps + (size_t)i * ACCBPG_FW_RUN_MAX + k);
}
__global__ __launch_bounds__(FB) void fw_probe_away_partial_brun_kernel(const FwInst* __restrict__ tab,
                                                                       const FwRunSlot* runs, FwProbeArgs pa, int64_t m,
                                                                       int64_t n) {
    const int a = blockIdx.y, i = pa.idx[a];
    if (fw_run_stop(&runs[i].run)) return;
    const FwInst t = tab[i];
    fw_probe_away_partial_body(fw_part_of(t, m), pa.nblk[a], t.w, t.x, n, fw_part2_of(t, m), fw_mxslot_of(t, m));
}
__global__ __launch_bounds__(FB) void fw_probe_away_final_brun_kernel(const FwInst* __restrict__ tab, FwRunSlot* runs,
                                                                     BatchAct act, ::BatchVals eps, int nb2, int64_t m,
                                                                     int64_t n, accbpg_fw_step* steps, int k) {
    const int a = blockIdx.y, i = act.idx[a];
    FwRunSlot* sl = runs + i;
    if (fw_run_stop(&sl->run)) return;
    const FwInst t = tab[i];
    fw_probe_away_final_body(fw_part2_of(t, m), nb2, fw_mxslot_of(t, m), t.w, t.x, n, fw_rec_d(sl->rec),
                             fw_rec_i(sl->rec), t.q);
    if (threadIdx.x == 0)
        fw_run_decide(&sl->run, sl->rec, m, n, 1, eps.v[a], steps + (size_t)i * ACCBPG_FW_RUN_MAX + k);
}
__global__ __launch_bounds__(FB) void fw_xupdate_gather_brun_kernel(const FwInst* __restrict__ tab,
                                                                   const FwRunSlot* __restrict__ runs, BatchAct act,
                                                                   int64_t m, int64_t n, int64_t ldv) {
    const int i = act.idx[blockIdx.y];
    const FwRun r = runs[i].run;
    if (r.stop) return;
    const FwInst t = tab[i];
    fw_xupdate_gather_body(t.x, n, r.p, r.xscale, r.xadd, t.V, ldv, m, fw_vp_of(t, m));
}
// (Hv, the pass over V and the rank-one update take the slot type of the caller: FwRunSlot here, FwDivRunSlot in the
//  Bregman-step family below -- both begin with the FwRun these kernels read)
template <class Slot>
__global__ __launch_bounds__(FB) void fw_gemv_h_brun_kernel(const FwInst* __restrict__ tab,
                                                           const Slot* __restrict__ runs, BatchAct act, int64_t m) {
    const int i = act.idx[blockIdx.y];
    if (runs[i].run.stop) return;
    const FwInst t = tab[i];
    fw_gemv_h_body(t.H, m, fw_vp_of(t, m), t.hv);
}
template <class Slot>
__global__ __launch_bounds__(FB) void fw_rank1_brun_kernel(const FwInst* __restrict__ tab,
                                                          const Slot* __restrict__ runs, BatchAct act, int64_t m) {
    const int i = act.idx[blockIdx.y];
    const FwRun r = runs[i].run;
    if (r.stop) return;
    const FwInst t = tab[i];
    fw_rank1_body(t.H, m, t.hv, r.hcoef, r.hdiv, fw_vp_of(t, m), t.q);
}
template <class Slot>
__global__ __launch_bounds__(FB) void fw_vgemv_partial_brun_kernel(const FwInst* __restrict__ tab,
                                                                  const Slot* __restrict__ runs, BatchAct act,
                                                                  int64_t ldv, int64_t m, int64_t n, int nsplit) {
    const int i = act.idx[blockIdx.z];
    if (runs[i].run.stop) return;
    const FwInst t = tab[i];
    fw_vgemv_partial_body(t.V, ldv, m, n, t.hv, nsplit, t.vws, t.vec_ok != 0);
}
__global__ __launch_bounds__(FB) void fw_wupdate_probe_brun_kernel(const FwInst* __restrict__ tab,
                                                                  const FwRunSlot* __restrict__ runs, BatchAct act,
                                                                  int64_t m, int64_t n, int nsplit, int away) {
    const int i = act.idx[blockIdx.y];
    const FwRun r = runs[i].run;
    if (r.stop) return;
    const FwInst t = tab[i];
    fw_wupdate_probe_body(t.w, n, t.vws, nsplit, r.hcoef, r.hdiv, t.x, away, fw_part_of(t, m));
}
// what a launch of the family carries by value at most: the active set, the stage-1 records of the first iteration
// and eps, far inside the 4 KiB of kernel arguments at K = ACCBPG_BATCH_MAX
static_assert(sizeof(FwProbeArgs) + sizeof(::BatchVals) + 64 <= 4096, "batch-run kernel arguments");

// u = sum of the row-split partials (u = V^T q)
__device__ __forceinline__ void fw_usum_body(const double* __restrict__ upart, int nsplit, int64_t n,
                                             double* __restrict__ u) {
    const int64_t stride = (int64_t)gridDim.x * FB;
    for (int64_t k = (int64_t)blockIdx.x * FB + threadIdx.x; k < n; k += stride) {
        double a = 0.0;
        for (int s = 0; s < nsplit; ++s) a += upart[(int64_t)s * n + k];
        u[k] = a;
    }
}
__global__ __launch_bounds__(FB) void fw_usum_kernel(const double* __restrict__ upart, int nsplit, int64_t n,
                                                    double* __restrict__ u) {
    fw_usum_body(upart, nsplit, n, u);
}
// u = V^T q of the instances of a Kumar-Yildirim table in lock-step (launch_vt_times_batch): the instance is
// blockIdx.z of the pass over V and blockIdx.y of the sum, the other grid dimensions are the single launch's
__global__ __launch_bounds__(FB) void vt_partial_batch_kernel(const KyInst* __restrict__ tab, int64_t ldv, int64_t m,
                                                             int64_t n, int first, int nsplit) {
    const KyInst t = tab[blockIdx.z];
    fw_vgemv_partial_body(t.V, ldv, m, n, first ? t.B : t.q, nsplit, t.vws, t.vec_ok != 0);
}
__global__ __launch_bounds__(FB) void vt_usum_batch_kernel(const KyInst* __restrict__ tab, int nsplit, int64_t n) {
    const KyInst t = tab[blockIdx.y];
    fw_usum_body(t.vws, nsplit, n, t.w);
}
// ---- the Bregman-step Frank-Wolfe probe (accbpg_fw_div_probe_step / accbpg_fw_div_apply) --------------------------
// FW_alg_div_step / FW_alg_descent_step on the D-optimal objective with the simplex LMO (algorithms_fw.py:6-75,
// :210-247; functions_lmo.py:137-160): the gradient is -w, the vertex is s = fill everywhere and `value` at the first
// argmax of w, and everything the host needs for an iteration is a handful of sums over w and x.  The sums and the
// minimum run over the fixed tree of reduce.hpp on red_blocks(n, FW_DIV_CAP) workgroups.
//
// Stage 2 of the probe (stage 1 is the first-index argmax records of fw_probe_partial / fw_wupdate_probe): every
// workgroup combines the stage-1 maxima itself (at most FW_PART_MAX records: the same i everywhere), then folds its
// entries.  Per entry, each operation rounded once, written as the generic path writes them (vec_kernels.hip,
// ls_terms_partial_body with g = -w, x = s, y = x):
//   sum_w += w;  sum_w2 += w*w;  slope += (-w) * (s - x);  div += s/x - log(s/x) - 1;  min_x = min_nan(min_x, x)
__device__ __forceinline__ void fw_div_probe_partial_body(const ValIdx* __restrict__ part, int nblk,
                                                          const double* __restrict__ w,
                                                          const double* __restrict__ x, int64_t n, double fill,
                                                          double value, double* __restrict__ rec,
                                                          ValIdx* __restrict__ mxslot) {
    __shared__ ValIdx sh[FB / 64];
    const double inf = __builtin_inf();
    ValIdx best{-inf, INT64_MAX};
    for (int b = threadIdx.x; b < nblk; b += FB) best = better_max(best, part[2 * b]);
    const ValIdx mx = block_reduce_vi_n<true, FB>(best, sh);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, mn = inf;
    const int64_t stride = (int64_t)gridDim.x * FB;
    for (int64_t k = (int64_t)blockIdx.x * FB + threadIdx.x; k < n; k += stride) {
        const double wk = w[k], xk = x[k];
        const double sk = (k == mx.i) ? value : fill;
        s0 += wk;
        s1 += wk * wk;
        const double d = sk - xk;
        s2 += (-wk) * d;
        const double r = sk / xk;
        s3 += r - log(r) - 1.0;
        mn = min_nan(mn, xk);
    }
    double v[5] = {s0, s1, s2, s3, mn};
    block_reduce_store<FB, 5, true>(v, rec + (int64_t)blockIdx.x * 5);
    if (blockIdx.x == 0 && threadIdx.x == 0) *mxslot = mx;
}
// final stage: the block records in block order into doubles 3..7 of the pinned record, (i, w_i, x_i) in front of them,
// and vp <- V[:,i] with i as it stands in device memory (no host round trip between the probe and the direction)
__device__ __forceinline__ void fw_div_probe_final_body(const double* __restrict__ rec, int nb,
                                                        const ValIdx* __restrict__ mxslot,
                                                        const double* __restrict__ x, int64_t n,
                                                        const double* __restrict__ V, int64_t ldv, int64_t m,
                                                        double* __restrict__ vp, double* __restrict__ pin) {
    reduce_final_body<FB, 5, true>(rec, nb, pin + 3);
    const ValIdx mx = *mxslot;
    const int64_t i = mx.i;
    const bool ok = i >= 0 && i < n;
    if (threadIdx.x == 0) {
        reinterpret_cast<int64_t*>(pin)[0] = i;
        pin[1] = mx.v;
        pin[2] = ok ? x[i] : __builtin_nan("");
    }
    if (ok)
        for (int64_t r = threadIdx.x; r < m; r += FB) vp[r] = V[r * ldv + i];
}
// u = sum of the row-split partials, as fw_wupdate sums them, kept for the apply; sum u^2 over the tree
__device__ __forceinline__ void fw_div_usum_body(const double* __restrict__ upart, int nsplit, int64_t n,
                                                 double* __restrict__ u, double* __restrict__ u2part) {
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * FB;
    for (int64_t k = (int64_t)blockIdx.x * FB + threadIdx.x; k < n; k += stride) {
        double a = 0.0;
        for (int s = 0; s < nsplit; ++s) a += upart[(int64_t)s * n + k];
        u[k] = a;
        acc += a * a;
    }
    double v[1] = {acc};
    block_reduce_store<FB, 1, false>(v, u2part + blockIdx.x);
}
// x <- x + a*(s - x) with the vertex implicit: the bits of vec_axpby(1, s, -1, x) followed by vec_axpby(1, x, a, d)
// (1*s, -1*x and 1*x are exact: one subtraction, one product, one addition)
__device__ __forceinline__ void fw_div_xupdate_body(double* __restrict__ x, int64_t n, int64_t p, double a,
                                                    double fill, double value) {
    const int64_t stride = (int64_t)gridDim.x * FB;
    for (int64_t k = (int64_t)blockIdx.x * FB + threadIdx.x; k < n; k += stride) {
        const double xk = x[k];
        const double d = ((k == p) ? value : fill) - xk;
        const double q = a * d;
        x[k] = xk + q;
    }
}

// one instance: the handle's pointers as arguments
__global__ __launch_bounds__(FB) void fw_div_probe_partial_kernel(const ValIdx* __restrict__ part, int nblk,
                                                                 const double* __restrict__ w,
                                                                 const double* __restrict__ x, int64_t n, double fill,
                                                                 double value, double* __restrict__ rec,
                                                                 ValIdx* __restrict__ mxslot) {
    fw_div_probe_partial_body(part, nblk, w, x, n, fill, value, rec, mxslot);
}
__global__ __launch_bounds__(FB) void fw_div_probe_final_kernel(const double* __restrict__ rec, int nb,
                                                               const ValIdx* __restrict__ mxslot,
                                                               const double* __restrict__ x, int64_t n,
                                                               const double* __restrict__ V, int64_t ldv, int64_t m,
                                                               double* __restrict__ vp, double* __restrict__ pin) {
    fw_div_probe_final_body(rec, nb, mxslot, x, n, V, ldv, m, vp, pin);
}
__global__ __launch_bounds__(FB) void fw_div_usum_kernel(const double* __restrict__ upart, int nsplit, int64_t n,
                                                        double* __restrict__ u, double* __restrict__ u2part) {
    fw_div_usum_body(upart, nsplit, n, u, u2part);
}
__global__ __launch_bounds__(FB) void fw_div_xupdate_kernel(double* __restrict__ x, int64_t n, int64_t p, double a,
                                                           double fill, double value) {
    fw_div_xupdate_body(x, n, p, a, fill, value);
}

// ---- the Bregman-step kernels: several iterations per host round trip (accbpg_fw_div_run) ------------------------
// The "run" forms of the four bodies above on the single handle's grids (Hv, u, the rank-one update and the update of
// w are the run forms of accbpg_fw_run, which read the FwRun in front of the slot).  Thread 0 of the last stage of the
// probe -- after sum u^2, which the trial values need -- predicts the decisions of the iteration with the text of
// fw_div_decide.hpp on the book the slot keeps (ld advanced with the device's own log), writes the step for the update
// kernels and the record straight into the pinned host array.  The host replays and checks every record: see the header.
__device__ __forceinline__ int fw_div_run_halted(const FwRun* run) {
    const volatile int32_t* r = reinterpret_cast<const volatile int32_t*>(run);
    return r[0] | r[1];                                         // stop | pad
}
struct FwDivRunArgs {       // what does not change inside a call
    int mode;
    double gamma, ls_ratio, epsilon;
    int64_t n;
    int nsteps;
};
// the probe record of a slot (or of the pinned one: the same layout) as fw_div_decide.hpp reads it
struct FwDivRecView {
    int64_t i;
    double w_i, x_i, sum_w, sum_w2, slope, div, min_x, sum_u2;
};
__device__ __forceinline__ FwDivRecView fw_div_view(const double* rec) {
    FwDivRecView v;
    v.i = reinterpret_cast<const int64_t*>(rec)[0];
    v.w_i = rec[1]; v.x_i = rec[2]; v.sum_w = rec[3]; v.sum_w2 = rec[4]; v.slope = rec[5]; v.div = rec[6];
    v.min_x = rec[7]; v.sum_u2 = rec[8];
    return v;
}
__device__ __forceinline__ void fw_div_record(accbpg_fw_div_step* __restrict__ out, const FwDivRecView& v,
                                              const FwdOut& o, double L, int status) {
    accbpg_fw_div_step st;
    st.probe.i = v.i; st.probe.w_i = v.w_i; st.probe.x_i = v.x_i; st.probe.sum_w = v.sum_w; st.probe.sum_w2 = v.sum_w2;
    st.probe.slope = v.slope; st.probe.div = v.div; st.probe.min_x = v.min_x; st.probe.sum_u2 = v.sum_u2;
    st.L = L; st.a = o.a; st.hcoef = o.hcoef; st.hdiv = o.hdiv; st.ld1 = o.ld1; st.q1 = o.q1; st.f1 = o.f1;
    st.trials = o.trials; st.status = status; st.reason = o.reason; st.reserved = 0;
    *out = st;
}
__device__ __forceinline__ FwdBook fw_div_book(const FwDivRunSlot* sl, int64_t m, double fill, double value) {
    FwdBook b;
    b.ld = sl->ld; b.q = sl->q; b.m = (double)m; b.radius = value; b.fill = fill; b.F_prev = sl->F_prev;
    return b;
}
__device__ __forceinline__ void fw_div_set_stop(FwRun* run, int32_t v) {
    *reinterpret_cast<volatile int32_t*>(&run->stop) = v;
}
// the classical step of iteration k from the probe record `v`: into the slot for the update kernels, or a hand-back
// into `out` (the record of iteration k; null when the call has no such record)
__device__ __forceinline__ void fw_div_next_classical(FwDivRunSlot* sl, FwdBook* b, const FwDivRecView& v, int64_t n,
                                                      int64_t k, FwdOut* o, accbpg_fw_div_step* out) {
    fw_descent_step(v, (long long)n, b, (long long)k, o);
    if (o->status == FWD_HANDED_BACK) {
        fw_div_set_stop(&sl->run, 2);
        if (out) fw_div_record(out, v, *o, 0.0, FWD_HANDED_BACK);
        return;
    }
    sl->run.p = v.i; sl->run.xscale = o->a; sl->run.xadd = 0.0; sl->run.hcoef = o->hcoef; sl->run.hdiv = o->hdiv;
    sl->ld = b->ld; sl->q = b->q;
}
// one thread: the slot at the start of a call; in the classical mode the step of iteration k0 from the pending probe
__global__ void fw_div_run_init_kernel(FwDivRunSlot* sl, FwDivRunArgs ra, int64_t m, double fill, double value,
                                       double L, double ld, double q, double F_prev, int64_t k0,
                                       const double* __restrict__ pin, accbpg_fw_div_step* __restrict__ out0) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    sl->run.stop = 0; sl->run.pad = 0; sl->run.p = -1;
    sl->run.xscale = 0.0; sl->run.xadd = 0.0; sl->run.hcoef = 0.0; sl->run.hdiv = 1.0;
    sl->ld = ld; sl->q = q; sl->F_prev = F_prev; sl->L = L;
    if (ra.mode == FWD_CLASSICAL) {
        for (int c = 0; c < 9; ++c) sl->rec[c] = pin[c];
        FwdBook b = fw_div_book(sl, m, fill, value);
        FwdOut o;
        fw_div_next_classical(sl, &b, fw_div_view(sl->rec), ra.n, k0, &o, out0);
    }
}
__global__ __launch_bounds__(FB) void fw_div_probe_partial_run_kernel(const FwRun* run, const ValIdx* __restrict__ part,
                                                                     int nblk, const double* __restrict__ w,
                                                                     const double* __restrict__ x, int64_t n,
                                                                     double fill, double value, double* __restrict__ rec,
                                                                     ValIdx* __restrict__ mxslot) {
    if (fw_div_run_halted(run)) return;
    fw_div_probe_partial_body(part, nblk, w, x, n, fill, value, rec, mxslot);
}
// (one workgroup: every thread reads the two words before thread 0 turns "stop after this apply" into stop)
__global__ __launch_bounds__(FB) void fw_div_probe_final_run_kernel(FwRun* run, const double* __restrict__ rec, int nb,
                                                                   const ValIdx* __restrict__ mxslot,
                                                                   const double* __restrict__ x, int64_t n,
                                                                   const double* __restrict__ V, int64_t ldv, int64_t m,
                                                                   double* __restrict__ vp, double* __restrict__ scratch) {
    const int halted = fw_div_run_halted(run);
    __syncthreads();
    if (halted) {
        if (threadIdx.x == 0 && run->stop == 0) fw_div_set_stop(run, 1);
        return;
    }
    fw_div_probe_final_body(rec, nb, mxslot, x, n, V, ldv, m, vp, scratch);
}
__global__ __launch_bounds__(FB) void fw_div_usum_run_kernel(const FwRun* __restrict__ run,
                                                            const double* __restrict__ upart, int nsplit, int64_t n,
                                                            double* __restrict__ u, double* __restrict__ u2part) {
    if (run->stop) return;
    fw_div_usum_body(upart, nsplit, n, u, u2part);
}
// one thread, behind sum u^2: the decisions of iteration k from the slot's probe record, the step for the update kernels
// and record j of the row `steps`
__device__ __forceinline__ void fw_div_run_decide(FwDivRunSlot* sl, const FwDivRunArgs& ra, int64_t m, double fill,
                                                  double value, int64_t k, int j,
                                                  accbpg_fw_div_step* __restrict__ steps) {
    const FwDivRecView v = fw_div_view(sl->rec);                // (doubles 0..7 by the stage before, 8 by this thread)
    FwdBook b = fw_div_book(sl, m, fill, value);
    FwdOut o;
    if (ra.mode != FWD_CLASSICAL) {
        double L = sl->L;
        fw_div_decide(v, (long long)ra.n, &b, &L, ra.mode, ra.gamma, ra.ls_ratio, ra.epsilon, (long long)k, &o);
        if (o.status == FWD_HANDED_BACK) {
            fw_div_set_stop(&sl->run, 2);
        } else {
            sl->run.p = v.i; sl->run.xscale = o.a; sl->run.xadd = 0.0; sl->run.hcoef = o.hcoef; sl->run.hdiv = o.hdiv;
            sl->ld = b.ld; sl->q = b.q; sl->F_prev = b.F_prev; sl->L = L;
            if (o.status == FWD_STOPPED) *reinterpret_cast<volatile int32_t*>(&sl->run.pad) = 1;
        }
        fw_div_record(steps + j, v, o, o.L, o.status);
        return;
    }
    // classical: this is the probe behind step k, whose scalars the slot still holds
    o.trials = 0; o.reason = FWD_HB_NONE;
    o.a = sl->run.xscale; o.hcoef = sl->run.hcoef; o.hdiv = sl->run.hdiv; o.ld1 = sl->ld; o.q1 = sl->q;
    const bool stop = fw_descent_probed(v, &b, ra.epsilon, &o.f1);
    sl->F_prev = b.F_prev;
    fw_div_record(steps + j, v, o, 0.0, stop ? FWD_STOPPED : FWD_APPLIED);
    if (stop) {
        fw_div_set_stop(&sl->run, 1);
        return;
    }
    FwdOut o2;
    fw_div_next_classical(sl, &b, v, ra.n, k + 1, &o2, (j + 1 < ra.nsteps) ? steps + j + 1 : nullptr);
}
__global__ __launch_bounds__(FB) void fw_div_u2final_run_kernel(FwDivRunSlot* sl, const double* __restrict__ u2part,
                                                               int nb, FwDivRunArgs ra, int64_t m, double fill,
                                                               double value, int64_t k, int j,
                                                               accbpg_fw_div_step* __restrict__ steps) {
    if (fw_run_stop(&sl->run)) return;
    reduce_final_body<FB, 1, false>(u2part, nb, sl->rec + 8);
    if (threadIdx.x != 0) return;
    fw_div_run_decide(sl, ra, m, fill, value, k, j, steps);
}
__global__ __launch_bounds__(FB) void fw_div_xupdate_run_kernel(const FwRun* __restrict__ run, double* __restrict__ x,
                                                               int64_t n, double fill, double value) {
    const FwRun r = *run;
    if (r.stop) return;
    fw_div_xupdate_body(x, n, r.p, r.xscale, fill, value);
}

// ---- the Bregman-step kernels: several iterations per host round trip for the active instances of a batch -------
// (accbpg_dopt_batch_fw_div_run)  The "batch-run" forms of the same bodies: the instance is the grid dimension of the
// lock-step forms, its pointers come from the batch's FwInst and FwDivInst tables, its step and its predictor's book from
// its own FwDivRunSlot.  A workgroup returns before it touches anything when ITS instance has stopped, is marked "stop
// after this apply" or was handed back (one load per workgroup, the same for all its threads) while the workgroups of the
// other instances go on.  blockIdx.x / gridDim.x, the FW_DIV_CAP block cap, the row split and the fixed summation tree
// are the single handle's; Hv, the pass over V and the rank-one update are the batch-run kernels of accbpg_dopt_batch_
// fw_run on this family's slots.  Thread 0 of an instance's last probe stage calls fw_div_run_decide with that instance's
// own k0, gamma, ls_ratio and epsilon and writes record j of that instance's row of the pinned array.
__global__ void fw_div_brun_init_kernel(FwDivRunSlot* runs, const FwDivInst* __restrict__ dtab, FwDivInitArgs ia,
                                        int mode, int64_t m, int64_t n, double fill, double value,
                                        accbpg_fw_div_step* __restrict__ steps) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;        // one thread per active instance
    if (a >= ia.n) return;
    const int i = ia.idx[a];
    FwDivRunSlot* sl = runs + i;
    sl->run.stop = 0; sl->run.pad = 0; sl->run.p = -1;
    sl->run.xscale = 0.0; sl->run.xadd = 0.0; sl->run.hcoef = 0.0; sl->run.hdiv = 1.0;
    sl->ld = ia.ld[a]; sl->q = ia.q[a]; sl->F_prev = ia.F_prev[a]; sl->L = ia.L[a]; sl->k0 = ia.k0[a];
    if (mode == FWD_CLASSICAL) {                                // the step of iteration k0 from the pending probe
        const double* pin = dtab[i].pin;
        for (int c = 0; c < 9; ++c) sl->rec[c] = pin[c];
        FwdBook b = fw_div_book(sl, m, fill, value);
        FwdOut o;
        fw_div_next_classical(sl, &b, fw_div_view(sl->rec), n, ia.k0[a], &o, steps + (size_t)i * ACCBPG_FW_RUN_MAX);
    }
}
__global__ __launch_bounds__(FB) void fw_div_probe_partial_brun_kernel(const FwInst* __restrict__ tab,
                                                                      const FwDivInst* __restrict__ dtab,
                                                                      const FwDivRunSlot* runs, FwProbeArgs pa,
                                                                      int64_t m, int64_t n, double fill, double value) {
    const int a = blockIdx.y, i = pa.idx[a];
    if (fw_div_run_halted(&runs[i].run)) return;
    const FwInst t = tab[i];
    double* ws = dtab[i].ws;
    fw_div_probe_partial_body(fw_part_of(t, m), pa.nblk[a], t.w, t.x, n, fill, value, fw_div_rec_of(ws, n),
                              fw_div_mxslot_of(ws, n));
}
// (one workgroup per instance: every thread reads the two words before thread 0 turns "stop after this apply" into stop)
__global__ __launch_bounds__(FB) void fw_div_probe_final_brun_kernel(const FwInst* __restrict__ tab,
                                                                    const FwDivInst* __restrict__ dtab,
                                                                    FwDivRunSlot* runs, BatchAct act, int nb,
                                                                    int64_t ldv, int64_t m, int64_t n) {
    const int i = act.idx[blockIdx.y];
    FwDivRunSlot* sl = runs + i;
    const int halted = fw_div_run_halted(&sl->run);
    __syncthreads();
    if (halted) {
        if (threadIdx.x == 0 && sl->run.stop == 0) fw_div_set_stop(&sl->run, 1);
        return;
    }
    const FwInst t = tab[i];
    double* ws = dtab[i].ws;
    fw_div_probe_final_body(fw_div_rec_of(ws, n), nb, fw_div_mxslot_of(ws, n), t.x, n, t.V, ldv, m, fw_vp_of(t, m),
                            sl->rec);
}
__global__ __launch_bounds__(FB) void fw_div_usum_brun_kernel(const FwInst* __restrict__ tab,
                                                             const FwDivInst* __restrict__ dtab,
                                                             const FwDivRunSlot* __restrict__ runs, BatchAct act,
                                                             int nsplit, int64_t n) {
    const int i = act.idx[blockIdx.y];
    if (runs[i].run.stop) return;
    double* ws = dtab[i].ws;
    fw_div_usum_body(tab[i].vws, nsplit, n, ws, fw_div_u2part_of(ws, n));
}
__global__ __launch_bounds__(FB) void fw_div_u2final_brun_kernel(const FwDivInst* __restrict__ dtab, FwDivRunSlot* runs,
                                                                FwDivDecideArgs da, int mode, int nsteps, int nb,
                                                                int64_t m, int64_t n, double fill, double value, int j,
                                                                accbpg_fw_div_step* __restrict__ steps) {
    const int a = blockIdx.y, i = da.idx[a];
    FwDivRunSlot* sl = runs + i;
    if (fw_run_stop(&sl->run)) return;
    reduce_final_body<FB, 1, false>(fw_div_u2part_of(dtab[i].ws, n), nb, sl->rec + 8);
    if (threadIdx.x != 0) return;
    const FwDivRunArgs ra{mode, da.gamma[a], da.ls_ratio[a], da.epsilon[a], n, nsteps};
    fw_div_run_decide(sl, ra, m, fill, value, sl->k0 + j, j, steps + (size_t)i * ACCBPG_FW_RUN_MAX);
}
__global__ __launch_bounds__(FB) void fw_div_xupdate_brun_kernel(const FwInst* __restrict__ tab,
                                                                const FwDivRunSlot* __restrict__ runs, BatchAct act,
                                                                int64_t n, double fill, double value) {
    const int i = act.idx[blockIdx.y];
    const FwRun r = runs[i].run;
    if (r.stop) return;
    fw_div_xupdate_body(tab[i].x, n, r.p, r.xscale, fill, value);
}
// w <- (w + hcoef u^2) / hdiv from the kept u (one "split") with stage 1 of the next probe, as accbpg_fw_div_apply
__global__ __launch_bounds__(FB) void fw_div_wupdate_probe_brun_kernel(const FwInst* __restrict__ tab,
                                                                      const FwDivInst* __restrict__ dtab,
                                                                      const FwDivRunSlot* __restrict__ runs,
                                                                      BatchAct act, int64_t m, int64_t n) {
    const int i = act.idx[blockIdx.y];
    const FwRun r = runs[i].run;
    if (r.stop) return;
    const FwInst t = tab[i];
    fw_wupdate_probe_body(t.w, n, dtab[i].ws, 1, r.hcoef, r.hdiv, t.x, 0, fw_part_of(t, m));
}
// what a launch of the family carries by value at most, inside the 4 KiB of kernel arguments at K = ACCBPG_BATCH_MAX
static_assert(sizeof(FwDivInitArgs) + 128 <= 4096 && sizeof(FwDivDecideArgs) + 128 <= 4096 &&
              sizeof(FwProbeArgs) + 128 <= 4096, "batched div-run kernel arguments");

// The active instances of a batch in lock-step (accbpg_dopt_batch_fw_div_probe / _fw_div_apply), by the convention of
// the step kernels above: blockIdx.y is the position among the active instances, blockIdx.x and gridDim.x are the single
// launch's, so the fixed tree adds every instance's entries in the single handle's order.  The state comes from the
// batch's FwInst table, the Bregman-step workspace and the pinned record from its FwDivInst table.  Hv = H V[:,i] and
// the pass over V between the probe and the sum of u are fw_gemv_h_batch / fw_vgemv_partial_batch as they stand.
__global__ __launch_bounds__(FB) void fw_div_probe_partial_batch_kernel(const FwInst* __restrict__ tab,
                                                                       const FwDivInst* __restrict__ dtab,
                                                                       FwProbeArgs pa, int64_t m, int64_t n, double fill,
                                                                       double value) {
    const int i = pa.idx[blockIdx.y];
    const FwInst t = tab[i];
    double* ws = dtab[i].ws;
    fw_div_probe_partial_body(fw_part_of(t, m), pa.nblk[blockIdx.y], t.w, t.x, n, fill, value, fw_div_rec_of(ws, n),
                              fw_div_mxslot_of(ws, n));
}
__global__ __launch_bounds__(FB) void fw_div_probe_final_batch_kernel(const FwInst* __restrict__ tab,
                                                                     const FwDivInst* __restrict__ dtab, BatchAct act,
                                                                     int nb, int64_t ldv, int64_t m, int64_t n) {
    const int i = act.idx[blockIdx.y];
    const FwInst t = tab[i];
    const FwDivInst d = dtab[i];
    fw_div_probe_final_body(fw_div_rec_of(d.ws, n), nb, fw_div_mxslot_of(d.ws, n), t.x, n, t.V, ldv, m, fw_vp_of(t, m),
                            d.pin);
}
__global__ __launch_bounds__(FB) void fw_div_usum_batch_kernel(const FwInst* __restrict__ tab,
                                                              const FwDivInst* __restrict__ dtab, BatchAct act,
                                                              int nsplit, int64_t n) {
    const int i = act.idx[blockIdx.y];
    double* ws = dtab[i].ws;
    fw_div_usum_body(tab[i].vws, nsplit, n, ws, fw_div_u2part_of(ws, n));
}
__global__ __launch_bounds__(FB) void fw_div_u2final_batch_kernel(const FwDivInst* __restrict__ dtab, BatchAct act,
                                                                 int nb, int64_t n) {
    const FwDivInst d = dtab[act.idx[blockIdx.y]];
    reduce_final_body<FB, 1, false>(fw_div_u2part_of(d.ws, n), nb, d.pin + 8);
}
__global__ __launch_bounds__(FB) void fw_div_xupdate_batch_kernel(const FwInst* __restrict__ tab, FwUpdArgs ua,
                                                                 int64_t n, double fill, double value) {
    const int a = blockIdx.y;
    fw_div_xupdate_body(tab[ua.idx[a]].x, n, ua.p[a], ua.xscale[a], fill, value);
}
// w <- (w + hcoef u^2) / hdiv from the kept u (one "split") with stage 1 of the next probe, as accbpg_fw_div_apply
__global__ __launch_bounds__(FB) void fw_div_wupdate_probe_batch_kernel(const FwInst* __restrict__ tab,
                                                                       const FwDivInst* __restrict__ dtab, FwUpdArgs ua,
                                                                       int64_t m, int64_t n) {
    const int a = blockIdx.y;
    const int i = ua.idx[a];
    const FwInst t = tab[i];
    fw_wupdate_probe_body(t.w, n, dtab[i].ws, 1, ua.hcoef[a], ua.hdiv[a], t.x, 0, fw_part_of(t, m));
}
// what a batched launch of the family carries by value at most, inside the 4 KiB of kernel arguments at K = ACCBPG_BATCH_MAX
static_assert(sizeof(FwUpdArgs) + 64 <= 4096 && sizeof(FwProbeArgs) + 64 <= 4096, "batched div-step kernel arguments");

__global__ __launch_bounds__(FB) void column_kernel(const double* __restrict__ V, int64_t ldv, int64_t m, int64_t j,
                                                   double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * FB;
    for (int64_t r = (int64_t)blockIdx.x * FB + threadIdx.x; r < m; r += stride) out[r] = V[r * ldv + j];
}

// out = in^T for an m x m matrix (used once per fw_init to form H = W^T W on the MFMA engine)
__global__ __launch_bounds__(FB) void transpose_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                      int64_t m) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int64_t c0 = (int64_t)blockIdx.x * 32, r0 = (int64_t)blockIdx.y * 32;
    for (int j = ty; j < 32; j += 8)
        tile[j][tx] = (r0 + j < m && c0 + tx < m) ? in[(r0 + j) * m + c0 + tx] : 0.0;
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < m && r0 + tx < m) out[(c0 + j) * m + r0 + tx] = tile[tx][j];
}

// symmetrise: copy the lower triangle of H onto the upper one
__global__ __launch_bounds__(FB) void mirror_lower_kernel(double* __restrict__ H, int64_t m) {
    const int64_t total = m * m;
    const int64_t stride = (int64_t)gridDim.x * FB;
    for (int64_t e = (int64_t)blockIdx.x * FB + threadIdx.x; e < total; e += stride) {
        const int64_t r = e / m, c = e - r * m;
        if (c > r) H[e] = H[c * m + r];
    }
}

}  // namespace accbpg

using namespace accbpg;

static int fw_alloc(accbpg_dopt* h) {
    if (h->fw_x) return ACCBPG_OK;
    ACC_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->fw_hpin_dev), h->hpin, 0));   // the pinned record, as the device addresses it
    ACC_HIP(acc_malloc(&h->fw_x, sizeof(double) * h->n, "fw_x"));
    ACC_HIP(acc_malloc(&h->fw_w, sizeof(double) * h->n, "fw_w"));
    ACC_HIP(acc_malloc(&h->fw_H, sizeof(double) * h->m * h->m, "fw_H"));
    ACC_HIP(acc_malloc(&h->fw_hv, sizeof(double) * fw_scratch_doubles(h->m), "fw_hv"));
    h->fw = FwInst{h->fw_x, h->fw_w, h->fw_H, h->fw_hv, h->V, h->vws, h->dscal + 10, h->fw_hpin_dev, h->vec_ok ? 1 : 0};
    return ACCBPG_OK;
}

namespace accbpg { int vt_nsplit(int64_t m, int64_t n, int num_cu); }
static int fw_nsplit(const accbpg_dopt* h) { return vt_nsplit(h->m, h->n, h->num_cu); }

// Every grid of a step at one shape on one device, without the instance dimension.  All four families of entry points
// launch on these, so an instance of a batch gets the single handle's partition and summation order.
struct FwGrids {
    unsigned nblk;          // stage 1 of a probe that finds no records waiting
    bool away2;             // the away search runs in two stages
    unsigned nb2;           // ... on this many slices
    unsigned gb, hb, rb;    // fw_xupdate_gather, fw_gemv_h, fw_rank1
    int ns;                 // row splits of the pass over V
    unsigned vgx;           // ... and its column blocks
    unsigned wb;            // fw_wupdate_probe: the stage-1 records the next probe finds
};
static FwGrids fw_grids(int64_t m, int64_t n, int num_cu) {
    const auto capped = [](int64_t v, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min(v, cap)); };
    FwGrids g;
    g.nblk = capped((n + (int64_t)FB * 8 - 1) / ((int64_t)FB * 8), FW_PART_MAX);    // eight elements per thread
    g.away2 = n >= 4096;    // (one workgroup scanning 2n doubles took 40 us of a 170 us step at n = 32768)
    g.nb2 = std::min(g.nblk, (unsigned)AWAY_NB);
    g.gb = capped((std::max(n, m) + FB - 1) / FB, 1024);
    g.hb = (unsigned)(((m + 1) / 2 + FB / 64 - 1) / (FB / 64));                     // one wave per pair of rows
    g.rb = capped(m, 4096);                                                         // a row per workgroup pass
    g.ns = vt_nsplit(m, n, num_cu);
    g.vgx = (unsigned)((n + VG_COLS - 1) / VG_COLS);
    g.wb = capped((n + FB - 1) / FB, FW_PART_MAX);                                  // one record pair per workgroup
    return g;
}
// the stage-1 records the last update of w left for a probe with this support threshold (0: none, run stage 1)
static int fw_part_waiting(const accbpg_dopt* h, int away) {
    return (h->fw_part_nblk > 0 && h->fw_part_away == (away != 0)) ? h->fw_part_nblk : 0;
}

// the pinned probe record of a handle, as accbpg_fw_probe
static void fw_read_probe(const accbpg_dopt* h, double logdet, accbpg_fw_probe* out) {
    const int64_t* ih = fw_rec_i(h->hpin);
    out->i = ih[0];
    out->j = ih[1];
    out->w_i = fw_rec_d(h->hpin)[0];
    out->w_j = fw_rec_d(h->hpin)[1];
    out->x_j = fw_rec_d(h->hpin)[2];
    out->logdet_H = logdet;
    out->q_prev = fw_rec_d(h->hpin)[6];
}

// a row of pinned step records before a run: "not reached"
static void fw_steps_reset(accbpg_fw_step* row, int nsteps) {
    for (int k = 0; k < nsteps; ++k) {
        row[k] = accbpg_fw_step{};
        row[k].p = -1;
        row[k].kind = -1;
        row[k].status = 3;
    }
}
// ... and after it: copy the row out, count the iterations that ran, leave on the handle what a later probe finds -- the
// stage-1 records of the last update if the run ended on one (as accbpg_fw_update leaves them); after a stop none, as
// after accbpg_fw_probe_step (x and w are as that probe read them).  Returns the record whose pivot lay outside [0, n).
static const accbpg_fw_step* fw_steps_harvest(accbpg_dopt* h, const accbpg_fw_step* row, int nsteps, unsigned wb,
                                              accbpg_fw_step* out, int* nrun_host) {
    const accbpg_fw_step* bad = nullptr;
    int nrun = 0;
    for (int k = 0; k < nsteps; ++k) {
        out[k] = row[k];
        if (row[k].status != 3) ++nrun;
        if (row[k].status == 2 && !bad) bad = row + k;
    }
    *nrun_host = nrun;
    h->fw_part_nblk = (nrun == nsteps && out[nsteps - 1].status == 0) ? (int)wb : 0;
    return bad;
}

static int read_scalars(accbpg_dopt* h, int nd, int ni) {
    (void)nd; (void)ni;
    ACC_HIP(hipMemcpyAsync(h->hpin, h->dscal, sizeof(double) * STATUS_DOUBLES, hipMemcpyDeviceToHost, h->stream));   // scalars + flags
    ACC_HIP(hipStreamSynchronize(h->stream));
    return ACCBPG_OK;
}

static int fw_ring_drain(accbpg_dopt* h);

extern "C" int accbpg_fw_init(accbpg_dopt* h, const double* x0_dev, double* logdet_gram_host) {
    if (!h || !x0_dev) return ACCBPG_ERR_ARG;
    ACC_TRY(fw_ring_drain(h));                                 // factorisations left in flight by an earlier run
    ACC_TRY(fw_alloc(h));
    const int64_t m = h->m;
    ACC_TRY(device_copy(h->fw_x, x0_dev, (size_t)h->n, h->stream));
    double* gram = chol_tiles_usable(h) ? h->Gbuf : h->Lbuf;
    ACC_TRY(launch_gram(h, h->fw_x, gram));                    // D_opt_alg.py:40
    ACC_TRY(launch_cholesky(h, h->Lbuf, nullptr, nullptr, gram));   // det / inv via the Cholesky factor (:41-42)
    ACC_TRY(read_scalars(h, 1, 4));
    const int* fl = reinterpret_cast<const int*>(h->hpin + 16);
    if (fl[FLAG_ABORT] && !h->chol_tiles_off) {                // one-launch factorisation abandoned: launch per block column
        h->chol_tiles_off = true;
        return accbpg_fw_init(h, x0_dev, logdet_gram_host);
    }
    if (fl[FLAG_NOT_PD]) {
        set_last_error("accbpg_fw_init: V diag(x0) V^T is singular or not positive definite");
        return ACCBPG_ERR_NOT_PD;
    }
    if (logdet_gram_host) *logdet_gram_host = h->hpin[0];
    ACC_TRY(launch_trtri(h));                                  // W = L^-1
    ACC_TRY(launch_colnorm(h, h->Wbuf, h->fw_w, 1.0));         // w_i = |W v_i|^2 = v_i^T H v_i (:45)
    // H = W^T W: transpose W into Tbuf (rows of W^T are k-contiguous), then one product
    dim3 tg((unsigned)((m + 31) / 32), (unsigned)((m + 31) / 32));
    transpose_kernel<<<tg, FB, 0, h->stream>>>(h->Wbuf, h->Tbuf, m);
    GemmOp op{};
    op.A = h->Tbuf; op.lda = m; op.B = h->Wbuf; op.ldb = m; op.C = h->fw_H; op.ldc = m;
    op.M = (int)m; op.N = (int)m; op.K = (int)m; op.lower_only = 1; op.alpha = 1.0; op.beta = 0.0;
    ACC_HIP(hipMemcpyAsync(h->chol_op, &op, sizeof(GemmOp), hipMemcpyHostToDevice, h->stream));
    ACC_TRY(launch_gemm_ops(h->chol_op, 1, (int)m, (int)m, true, h->stream));
    mirror_lower_kernel<<<1024, FB, 0, h->stream>>>(h->fw_H, m);
    ACC_HIP(hipMemsetAsync(h->dscal + 10, 0, sizeof(double), h->stream));   // q of "the previous update": none yet
    ACC_HIP(hipGetLastError());
    ACC_HIP(hipStreamSynchronize(h->stream));
    h->fw_ready = true;
    h->fw_part_nblk = 0;
    h->fw_div_i = -1;                                          // (Hv and u of an earlier accbpg_fw_div_probe_step are stale)
    return ACCBPG_OK;
}

// ---- log det(H) beside the steps (refresh_logdet = 2) ----------------------------------------------------------
// F[k] = log det(H_k) of the away-step variant (D_opt_alg.py:136) is a LOGGED value: no decision of the iteration
// reads it.  So its O(m^3) factorisation need not sit between two HBM-bound steps: H_k is copied into a slot of a ring
// (one copy kernel on the main stream, in order with the updates) and factored on that slot's own stream by that
// slot's own auxiliary handle -- own buffers, own hand-off flags, own scalars -- while the main stream probes, decides
// and applies the updates that follow; the value is collected when the slot comes round again, `depth` such calls
// later (or by accbpg_fw_logdet_flush).  Same kernels on the same matrix as the synchronous form (refresh_logdet =
// 1): the numbers are those.  Nothing of the slots is shared with the main handle, so an evaluation on the main
// handle while factorisations are in flight is safe.
static int fw_ring_setup(accbpg_dopt* h) {
    while ((int)h->fw_ring.size() < h->fw_ring_depth) {
        accbpg_dopt::FwSlot sl;
        ACC_HIP(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
        ACC_HIP(hipEventCreateWithFlags(&sl.ev_snap, hipEventDisableTiming));
        const int rc = accbpg_dopt_create(h->V, h->m, h->n, h->ldv, sl.stream, &sl.aux, 1);
        if (rc != ACCBPG_OK) {
            hipStreamDestroy(sl.stream);
            hipEventDestroy(sl.ev_snap);
            return rc;
        }
        h->fw_ring.push_back(sl);
    }
    for (auto& sl : h->fw_ring) {                              // (development switches of the main handle apply to its slots)
        sl.aux->chol_stall_test = h->chol_stall_test;
        sl.aux->chol_spin_limit = h->chol_spin_limit;
    }
    return ACCBPG_OK;
}

static int fw_slot_factor(accbpg_dopt::FwSlot& sl, const double* snap) {
    accbpg_dopt* a = sl.aux;
    ACC_TRY(launch_cholesky(a, a->Lbuf, nullptr, nullptr, snap));
    ACC_HIP(hipMemcpyAsync(a->hpin, a->dscal, sizeof(double) * STATUS_DOUBLES, hipMemcpyDeviceToHost, a->stream));
    ACC_HIP(hipEventRecord(a->ev_done, a->stream));
    return ACCBPG_OK;
}

// wait for the slot's factorisation and return its log det (NaN if the matrix was not positive definite)
static int fw_slot_collect(accbpg_dopt::FwSlot& sl, double* logdet) {
    *logdet = __builtin_nan("");
    if (!sl.pending) return ACCBPG_OK;
    accbpg_dopt* a = sl.aux;
    ACC_HIP(hipEventSynchronize(a->ev_done));
    const int* fl = reinterpret_cast<const int*>(a->hpin + 16);
    if (fl[FLAG_ABORT] && !a->chol_tiles_off) {
        // the one-launch factorisation gave up a wait: the snapshot (in Gbuf) is intact, factor it with a launch per
        // block column, and keep this slot on those
        a->chol_tiles_off = true;
        note_tiles_fallback("accbpg_fw_probe_step (side factorisation)");
        ACC_TRY(fw_slot_factor(sl, a->Gbuf));
        ACC_HIP(hipEventSynchronize(a->ev_done));
    }
    sl.pending = false;
    if (!fl[FLAG_NOT_PD]) *logdet = a->hpin[0];
    return ACCBPG_OK;
}

static int fw_ring_drain(accbpg_dopt* h) {
    for (auto& sl : h->fw_ring) {
        double unused;
        ACC_TRY(fw_slot_collect(sl, &unused));
    }
    h->fw_ring_collected = h->fw_ring_issued;
    return ACCBPG_OK;
}

extern "C" int accbpg_fw_logdet_ring(accbpg_dopt* h, int depth, int small_launches) {
    if (!h || depth < 1 || depth > 16 || small_launches < 0 || small_launches > 2) return ACCBPG_ERR_ARG;
    ACC_TRY(fw_ring_drain(h));
    h->fw_ring_depth = depth;
    h->fw_ring_small = small_launches;
    for (auto& sl : h->fw_ring) sl.aux->chol_tiles_off = false;   // (a slot that had to give up the one launch finds out again)
    h->fw_ring_issued = h->fw_ring_collected = 0;              // slot = issue count modulo depth
    return ACCBPG_OK;
}

extern "C" int accbpg_fw_logdet_pending(accbpg_dopt* h) {
    return h ? (int)(h->fw_ring_issued - h->fw_ring_collected) : 0;
}

// the oldest factorisation in flight (NaN when there is none)
extern "C" int accbpg_fw_logdet_flush(accbpg_dopt* h, double* logdet_host) {
    if (!h || !logdet_host) return ACCBPG_ERR_ARG;
    *logdet_host = __builtin_nan("");
    if (h->fw_ring_collected >= h->fw_ring_issued) return ACCBPG_OK;
    accbpg_dopt::FwSlot& sl = h->fw_ring[(size_t)(h->fw_ring_collected % h->fw_ring_depth)];
    ACC_TRY(fw_slot_collect(sl, logdet_host));
    ++h->fw_ring_collected;
    return ACCBPG_OK;
}

// The refresh_logdet == 2 step on its own: snapshot H_k into the ring slot that comes round and start its side
// factorisation; *collected_host is the value that slot held (the call made `depth` such calls ago), NaN if none.
extern "C" int accbpg_fw_logdet_snapshot(accbpg_dopt* h, double* collected_host) {
    if (!h || !collected_host || !h->fw_ready) return ACCBPG_ERR_ARG;
    double logdet = __builtin_nan("");
    *collected_host = logdet;
    ACC_TRY(fw_ring_setup(h));
    // the slot that comes round: collect what it holds -- the value of the call made `depth` such calls ago
    if (h->fw_ring_issued - h->fw_ring_collected >= h->fw_ring_depth) ACC_TRY(accbpg_fw_logdet_flush(h, &logdet));
    accbpg_dopt::FwSlot& sl = h->fw_ring[(size_t)(h->fw_ring_issued % h->fw_ring_depth)];
    accbpg_dopt* a = sl.aux;
    const int64_t T = (h->m + NB - 1) / NB;
    if (!a->chol_tiles_off)
        a->chol_tiles_off = h->fw_ring_small == 1 || (h->fw_ring_small == 2 && T * (T + 1) / 2 >= h->num_cu);
    double* snap = chol_tiles_usable(a) ? a->Gbuf : a->Lbuf;
    ACC_TRY(device_copy(snap, h->fw_H, (size_t)h->m * h->m, h->stream));   // H_k, in order with the updates
    ACC_HIP(hipEventRecord(sl.ev_snap, h->stream));
    ACC_HIP(hipStreamWaitEvent(sl.stream, sl.ev_snap, 0));
    ACC_TRY(fw_slot_factor(sl, snap));
    sl.pending = true;
    ++h->fw_ring_issued;
    *collected_host = logdet;
    return ACCBPG_OK;
}

extern "C" int accbpg_fw_probe_step(accbpg_dopt* h, int away, int refresh_logdet, accbpg_fw_probe* out) {
    if (!h || !out || !h->fw_ready) return ACCBPG_ERR_ARG;
    double logdet = __builtin_nan("");
    if (refresh_logdet == 2) {
        ACC_TRY(accbpg_fw_logdet_snapshot(h, &logdet));
    } else if (refresh_logdet) {
        // F[k] = log det(H) from a fresh factorisation of the maintained inverse (D_opt_alg.py:136)
        // (the factor goes to Lbuf; H itself is read in place by the one-launch kernel, copied otherwise)
        ACC_TRY(launch_cholesky(h, h->Lbuf, nullptr, nullptr, h->fw_H));
        ACC_TRY(read_scalars(h, 1, 4));
        const int* fl = reinterpret_cast<const int*>(h->hpin + 16);
        if (fl[FLAG_ABORT] && !h->chol_tiles_off) {
            h->chol_tiles_off = true;
            ACC_TRY(launch_cholesky(h, h->Lbuf, nullptr, nullptr, h->fw_H));
            ACC_TRY(read_scalars(h, 1, 4));
        }
        logdet = h->hpin[0];
        if (fl[FLAG_NOT_PD]) logdet = __builtin_nan("");
    }
    const FwGrids g = fw_grids(h->m, h->n, h->num_cu);
    const FwInst& t = h->fw;
    const int64_t n = h->n;
    ValIdx* part = fw_part_of(t, h->m);
    int nblk = fw_part_waiting(h, away);
    if (!nblk) {                                                // (else stage 1 came with the last update of w)
        nblk = (int)g.nblk;
        fw_probe_partial_kernel<<<g.nblk, FB, 0, h->stream>>>(t.w, t.x, n, away, part);
    }
    h->fw_part_nblk = 0;
    h->fw_part_away = (away != 0);
    double* dout = fw_rec_d(t.rec);
    int64_t* iout = fw_rec_i(t.rec);
    if (away && g.away2) {
        ValIdx *part2 = fw_part2_of(t, h->m), *mxslot = fw_mxslot_of(t, h->m);
        fw_probe_away_partial_kernel<<<g.nb2, FB, 0, h->stream>>>(part, nblk, t.w, t.x, n, part2, mxslot);
        fw_probe_away_final_kernel<<<1, FB, 0, h->stream>>>(part2, (int)g.nb2, mxslot, t.w, t.x, n, dout, iout, t.q);
    } else {
        fw_probe_final_kernel<<<1, FB, 0, h->stream>>>(part, nblk, t.w, t.x, n, away, dout, iout, t.q);
    }
    ACC_HIP(hipGetLastError());
    // (the final stage wrote its record straight into the pinned host buffer: the copy operation that used to follow it
    //  was 4 us of every 0.12 ms step)
    ACC_HIP(hipStreamSynchronize(h->stream));
    fw_read_probe(h, logdet, out);
    return ACCBPG_OK;
}

extern "C" int accbpg_fw_update(accbpg_dopt* h, int64_t p, double xscale, double xadd, double hcoef, double hdiv) {
    if (!h || !h->fw_ready || p < 0 || p >= h->n) {
        set_last_error("accbpg_fw_update: no Frank-Wolfe state (call accbpg_fw_init) or pivot index %lld outside [0, n)",
                       (long long)p);
        return ACCBPG_ERR_ARG;
    }
    const FwGrids g = fw_grids(h->m, h->n, h->num_cu);
    const FwInst& t = h->fw;
    const int64_t m = h->m, n = h->n;
    double* vp = fw_vp_of(t, m);
    fw_xupdate_gather_kernel<<<g.gb, FB, 0, h->stream>>>(t.x, n, p, xscale, xadd, t.V, h->ldv, m, vp);
    fw_gemv_h_kernel<<<g.hb, FB, 0, h->stream>>>(t.H, m, vp, t.hv);
    fw_rank1_kernel<<<g.rb, FB, 0, h->stream>>>(t.H, m, t.hv, hcoef, hdiv, vp, t.q);
    prof_begin(h, PROF_FWV);
    fw_vgemv_partial_kernel<<<dim3(g.vgx, (unsigned)g.ns), FB, 0, h->stream>>>(t.V, h->ldv, m, n, t.hv, g.ns, t.vws, h->vec_ok);
    prof_end(h, PROF_FWV);
    // w update fused with stage 1 of the next probe (same support threshold as the last probe call)
    fw_wupdate_probe_kernel<<<g.wb, FB, 0, h->stream>>>(t.w, n, t.vws, g.ns, hcoef, hdiv, t.x, h->fw_part_away ? 1 : 0,
                                                     fw_part_of(t, m));
    h->fw_part_nblk = (int)g.wb;
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

// ---- several iterations per synchronisation (accbpg_fw_run) -----------------------------------------------------
static int fw_run_alloc(accbpg_dopt* h) {
    if (!h->fw_steps_pin) {
        ACC_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->fw_steps_pin), sizeof(accbpg_fw_step) * ACCBPG_FW_RUN_MAX,
                              hipHostMallocDefault));
        ACC_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->fw_steps_dev), h->fw_steps_pin, 0));
    }
    if (!h->fw_run) ACC_HIP(acc_malloc(reinterpret_cast<void**>(&h->fw_run), sizeof(FwRunSlot), "fw_run"));
    return ACCBPG_OK;
}

extern "C" int accbpg_fw_run(accbpg_dopt* h, int away, double eps, int nsteps, accbpg_fw_step* steps_host,
                             int* nrun_host) {
    if (!h || !h->fw_ready || !steps_host || !nrun_host || nsteps < 1 || nsteps > ACCBPG_FW_RUN_MAX) return ACCBPG_ERR_ARG;
    ACC_TRY(fw_run_alloc(h));
    hipStream_t s = h->stream;
    fw_steps_reset(h->fw_steps_pin, nsteps);                    // (nothing of an earlier call is in flight: it synchronised)
    ACC_HIP(hipMemsetAsync(&h->fw_run->run, 0, sizeof(FwRun), s));
    const FwGrids g = fw_grids(h->m, h->n, h->num_cu);
    const FwInst& t = h->fw;
    const int64_t m = h->m, n = h->n;
    FwRun* run = &h->fw_run->run;
    double* rec = h->fw_run->rec;
    ValIdx *part = fw_part_of(t, m), *part2 = fw_part2_of(t, m), *mxslot = fw_mxslot_of(t, m);
    double* vp = fw_vp_of(t, m);
    int nblk = fw_part_waiting(h, away);
    if (!nblk) {                                                // (else stage 1 came with the last update of w)
        nblk = (int)g.nblk;
        fw_probe_partial_kernel<<<g.nblk, FB, 0, s>>>(t.w, t.x, n, away, part);
    }
    h->fw_part_nblk = 0;                                        // (no claim of reuse survives an error return below)
    h->fw_part_away = (away != 0);
    for (int k = 0; k < nsteps; ++k) {
        accbpg_fw_step* out = h->fw_steps_dev + k;
        if (away && g.away2) {
            fw_probe_away_partial_run_kernel<<<g.nb2, FB, 0, s>>>(run, part, nblk, t.w, t.x, n, part2, mxslot);
            fw_probe_away_final_run_kernel<<<1, FB, 0, s>>>(run, part2, (int)g.nb2, mxslot, t.w, t.x, m, n, eps, rec, t.q, out);
        } else {
            fw_probe_final_run_kernel<<<1, FB, 0, s>>>(run, part, nblk, t.w, t.x, m, n, away, eps, rec, t.q, out);
        }
        fw_xupdate_gather_run_kernel<<<g.gb, FB, 0, s>>>(run, t.x, n, t.V, h->ldv, m, vp);
        fw_gemv_h_run_kernel<<<g.hb, FB, 0, s>>>(run, t.H, m, vp, t.hv);
        fw_rank1_run_kernel<<<g.rb, FB, 0, s>>>(run, t.H, m, t.hv, vp, t.q);
        fw_vgemv_partial_run_kernel<<<dim3(g.vgx, (unsigned)g.ns), FB, 0, s>>>(run, t.V, h->ldv, m, n, t.hv, g.ns, t.vws, h->vec_ok);
        fw_wupdate_probe_run_kernel<<<g.wb, FB, 0, s>>>(run, t.w, n, t.vws, g.ns, t.x, away ? 1 : 0, part);
        nblk = (int)g.wb;                                       // the next probe's stage 1 came with this update
    }
    ACC_HIP(hipGetLastError());
    ACC_HIP(hipStreamSynchronize(s));
    if (const accbpg_fw_step* bad = fw_steps_harvest(h, h->fw_steps_pin, nsteps, g.wb, steps_host, nrun_host)) {
        set_last_error("accbpg_fw_update: no Frank-Wolfe state (call accbpg_fw_init) or pivot index %lld outside [0, n)",
                       (long long)bad->p);
        return ACCBPG_ERR_ARG;
    }
    return ACCBPG_OK;
}

extern "C" int accbpg_fw_get_state(accbpg_dopt* h, double* x_dev, double* w_dev, double* H_dev) {
    if (!h || !h->fw_ready) return ACCBPG_ERR_ARG;
    if (x_dev) ACC_TRY(device_copy(x_dev, h->fw_x, (size_t)h->n, h->stream));
    if (w_dev) ACC_TRY(device_copy(w_dev, h->fw_w, (size_t)h->n, h->stream));
    if (H_dev)
        ACC_TRY(device_copy(H_dev, h->fw_H, (size_t)h->m * h->m, h->stream));
    ACC_HIP(hipStreamSynchronize(h->stream));
    return ACCBPG_OK;
}

// ---- Bregman-step Frank-Wolfe on the maintained state (accbpg_fw_div_probe_step / accbpg_fw_div_apply) -----------
// Workspace behind the handle (allocated by the first probe, freed with it): u (n doubles), FW_DIV_CAP block records
// of five doubles, FW_DIV_CAP partial sums of u^2, (w_i, i) -- the accessors next to FwDivInst (internal.h); and a
// pinned record of 16 doubles: i, w_i, x_i, the five reductions, sum u^2.
static int fw_div_alloc(accbpg_dopt* h) {
    if (h->fw_div_ws) return ACCBPG_OK;
    if (!h->fw_div_pin) {
        ACC_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->fw_div_pin), sizeof(double) * 16, hipHostMallocDefault));
        ACC_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->fw_div_pin_dev), h->fw_div_pin, 0));
    }
    ACC_HIP(acc_malloc(&h->fw_div_ws, sizeof(double) * fw_div_ws_doubles(h->n), "fw_div_ws"));
    return ACCBPG_OK;
}

// the pinned record of a handle, as accbpg_fw_div_probe
static void fw_div_read_probe(const accbpg_dopt* h, accbpg_fw_div_probe* out) {
    const double* pin = h->fw_div_pin;
    out->i = reinterpret_cast<const int64_t*>(pin)[0];
    out->w_i = pin[1];
    out->x_i = pin[2];
    out->sum_w = pin[3];
    out->sum_w2 = pin[4];
    out->slope = pin[5];
    out->div = pin[6];
    out->min_x = pin[7];
    out->sum_u2 = pin[8];
}

extern "C" int accbpg_fw_div_probe_step(accbpg_dopt* h, double fill, double value, accbpg_fw_div_probe* out) {
    if (!h || !out || !h->fw_ready) return ACCBPG_ERR_ARG;
    ACC_TRY(fw_div_alloc(h));
    h->fw_div_i = -1;
    const FwGrids g = fw_grids(h->m, h->n, h->num_cu);
    const FwInst& t = h->fw;
    const int64_t m = h->m, n = h->n;
    hipStream_t s = h->stream;
    ValIdx* part = fw_part_of(t, m);
    int nblk = fw_part_waiting(h, 0);
    if (!nblk) {                                                // (else stage 1 came with the last update of w)
        nblk = (int)g.nblk;
        fw_probe_partial_kernel<<<g.nblk, FB, 0, s>>>(t.w, t.x, n, 0, part);
    }
    h->fw_part_nblk = 0;
    h->fw_part_away = false;
    const int nb = red_blocks(n, FW_DIV_CAP);
    double *rec = fw_div_rec_of(h->fw_div_ws, n), *u2part = fw_div_u2part_of(h->fw_div_ws, n), *vp = fw_vp_of(t, m);
    ValIdx* mxslot = fw_div_mxslot_of(h->fw_div_ws, n);
    fw_div_probe_partial_kernel<<<nb, FB, 0, s>>>(part, nblk, t.w, t.x, n, fill, value, rec, mxslot);
    fw_div_probe_final_kernel<<<1, FB, 0, s>>>(rec, nb, mxslot, t.x, n, t.V, h->ldv, m, vp, h->fw_div_pin_dev);
    // the direction of the step: Hv = H V[:,i], u = V^T Hv (the kernels of accbpg_fw_update on their grids), sum u^2
    fw_gemv_h_kernel<<<g.hb, FB, 0, s>>>(t.H, m, vp, t.hv);
    prof_begin(h, PROF_FWV);
    fw_vgemv_partial_kernel<<<dim3(g.vgx, (unsigned)g.ns), FB, 0, s>>>(t.V, h->ldv, m, n, t.hv, g.ns, t.vws, h->vec_ok);
    prof_end(h, PROF_FWV);
    fw_div_usum_kernel<<<nb, FB, 0, s>>>(t.vws, g.ns, n, h->fw_div_ws, u2part);
    reduce_final_kernel<FB, 1, false><<<1, FB, 0, s>>>(u2part, nb, h->fw_div_pin_dev + 8);
    ACC_HIP(hipGetLastError());
    ACC_HIP(hipStreamSynchronize(s));
    fw_div_read_probe(h, out);
    if (out->i < 0 || out->i >= n) {
        set_last_error("accbpg_fw_div_probe_step: pivot index %lld outside [0, n)", (long long)out->i);
        return ACCBPG_ERR_ARG;
    }
    h->fw_div_i = out->i;
    return ACCBPG_OK;
}

extern "C" int accbpg_fw_div_apply(accbpg_dopt* h, int64_t p, double a, double fill, double value, double hcoef,
                                   double hdiv) {
    // Hv, vp and u are those of the last accbpg_fw_div_probe_step; any call that moved the state since then has either
    // cleared fw_div_i (accbpg_fw_init) or left stage-1 records behind (an update of w)
    if (!h || !h->fw_ready || p < 0 || p >= h->n || h->fw_div_i != p || h->fw_part_nblk != 0) {
        set_last_error("accbpg_fw_div_apply: pivot %lld is not the index of the last accbpg_fw_div_probe_step on this state",
                       (long long)p);
        return ACCBPG_ERR_ARG;
    }
    const FwGrids g = fw_grids(h->m, h->n, h->num_cu);
    const FwInst& t = h->fw;
    const int64_t m = h->m, n = h->n;
    hipStream_t s = h->stream;
    h->fw_div_i = -1;
    fw_div_xupdate_kernel<<<g.gb, FB, 0, s>>>(t.x, n, p, a, fill, value);
    fw_rank1_kernel<<<g.rb, FB, 0, s>>>(t.H, m, t.hv, hcoef, hdiv, fw_vp_of(t, m), t.q);
    // u is summed already: one "split"; fused with stage 1 of the next probe as in accbpg_fw_update
    fw_wupdate_probe_kernel<<<g.wb, FB, 0, s>>>(t.w, n, h->fw_div_ws, 1, hcoef, hdiv, t.x, 0, fw_part_of(t, m));
    h->fw_part_nblk = (int)g.wb;
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

// ---- several Bregman-step iterations per synchronisation (accbpg_fw_div_run) ------------------------------------
static int fw_div_run_alloc(accbpg_dopt* h) {
    if (!h->fw_div_steps_pin) {
        ACC_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->fw_div_steps_pin),
                              sizeof(accbpg_fw_div_step) * ACCBPG_FW_RUN_MAX, hipHostMallocDefault));
        ACC_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->fw_div_steps_dev), h->fw_div_steps_pin, 0));
    }
    if (!h->fw_div_run)
        ACC_HIP(acc_malloc(reinterpret_cast<void**>(&h->fw_div_run), sizeof(FwDivRunSlot), "fw_div_run"));
    return ACCBPG_OK;
}
static const accbpg_fw_div_step* fw_div_steps_harvest(accbpg_dopt* h, const accbpg_fw_div_step* pinned, int nsteps,
                                                      bool classical, int64_t pending, unsigned wb,
                                                      accbpg_fw_div_step* steps_host, int* nrun_host);

extern "C" int accbpg_fw_div_run(accbpg_dopt* h, double fill, double value, const accbpg_fw_div_params* prm, int nsteps,
                                 accbpg_fw_div_step* steps_host, int* nrun_host) {
    if (!h || !h->fw_ready || !prm || !steps_host || !nrun_host || nsteps < 1 || nsteps > ACCBPG_FW_RUN_MAX ||
        prm->mode < FWD_LINESEARCH || prm->mode > FWD_CLASSICAL)
        return ACCBPG_ERR_ARG;
    const bool classical = prm->mode == FWD_CLASSICAL;
    if (classical && (h->fw_div_i < 0 || h->fw_part_nblk != 0 || prm->k0 < 1)) {
        set_last_error("accbpg_fw_div_run: the classical step needs the probe of accbpg_fw_div_probe_step pending on this "
                       "state, and k0 >= 1");
        return ACCBPG_ERR_ARG;
    }
    ACC_TRY(fw_div_alloc(h));
    ACC_TRY(fw_div_run_alloc(h));
    const FwGrids g = fw_grids(h->m, h->n, h->num_cu);
    const FwInst& t = h->fw;
    const int64_t m = h->m, n = h->n;
    hipStream_t s = h->stream;
    accbpg_fw_div_step* pinned = h->fw_div_steps_pin;           // (nothing of an earlier call is in flight: it synchronised)
    for (int k = 0; k < nsteps; ++k) {
        pinned[k] = accbpg_fw_div_step{};
        pinned[k].probe.i = -1;
        pinned[k].status = FWD_NOT_RUN;
    }
    FwDivRunSlot* sl = h->fw_div_run;
    FwRun* run = &sl->run;
    accbpg_fw_div_step* steps = h->fw_div_steps_dev;
    const FwDivRunArgs ra{prm->mode, prm->gamma, prm->ls_ratio, prm->epsilon, n, nsteps};
    ValIdx* part = fw_part_of(t, m);
    double* vp = fw_vp_of(t, m);
    const int nb = red_blocks(n, FW_DIV_CAP);
    double *rec = fw_div_rec_of(h->fw_div_ws, n), *u2part = fw_div_u2part_of(h->fw_div_ws, n), *u = h->fw_div_ws;
    ValIdx* mxslot = fw_div_mxslot_of(h->fw_div_ws, n);
    const int64_t pending = h->fw_div_i;
    int nblk = 0;
    if (!classical) {
        nblk = fw_part_waiting(h, 0);
        if (!nblk) {                                            // (else stage 1 came with the last update of w)
            nblk = (int)g.nblk;
            fw_probe_partial_kernel<<<g.nblk, FB, 0, s>>>(t.w, t.x, n, 0, part);
        }
    }
    h->fw_part_nblk = 0;                                        // (no claim survives an error return below)
    h->fw_part_away = false;
    h->fw_div_i = -1;
    fw_div_run_init_kernel<<<1, 1, 0, s>>>(sl, ra, m, fill, value, prm->L, prm->ld, prm->q, prm->F_prev, prm->k0,
                                           h->fw_div_pin_dev, steps);
    for (int j = 0; j < nsteps; ++j) {
        if (classical) {                                        // apply step k, then the probe behind it
            fw_div_xupdate_run_kernel<<<g.gb, FB, 0, s>>>(run, t.x, n, fill, value);
            fw_rank1_run_kernel<<<g.rb, FB, 0, s>>>(run, t.H, m, t.hv, vp, t.q);
            fw_wupdate_probe_run_kernel<<<g.wb, FB, 0, s>>>(run, t.w, n, u, 1, t.x, 0, part);
            nblk = (int)g.wb;
        }
        fw_div_probe_partial_run_kernel<<<nb, FB, 0, s>>>(run, part, nblk, t.w, t.x, n, fill, value, rec, mxslot);
        fw_div_probe_final_run_kernel<<<1, FB, 0, s>>>(run, rec, nb, mxslot, t.x, n, t.V, h->ldv, m, vp, sl->rec);
        fw_gemv_h_run_kernel<<<g.hb, FB, 0, s>>>(run, t.H, m, vp, t.hv);
        fw_vgemv_partial_run_kernel<<<dim3(g.vgx, (unsigned)g.ns), FB, 0, s>>>(run, t.V, h->ldv, m, n, t.hv, g.ns, t.vws, h->vec_ok);
        fw_div_usum_run_kernel<<<nb, FB, 0, s>>>(run, t.vws, g.ns, n, u, u2part);
        fw_div_u2final_run_kernel<<<1, FB, 0, s>>>(sl, u2part, nb, ra, m, fill, value, prm->k0 + j, j, steps);
        if (!classical) {                                       // the step the record describes
            fw_div_xupdate_run_kernel<<<g.gb, FB, 0, s>>>(run, t.x, n, fill, value);
            fw_rank1_run_kernel<<<g.rb, FB, 0, s>>>(run, t.H, m, t.hv, vp, t.q);
            fw_wupdate_probe_run_kernel<<<g.wb, FB, 0, s>>>(run, t.w, n, u, 1, t.x, 0, part);
            nblk = (int)g.wb;
        }
    }
    ACC_HIP(hipGetLastError());
    ACC_HIP(hipStreamSynchronize(s));
    const accbpg_fw_div_step* bad = fw_div_steps_harvest(h, pinned, nsteps, classical, pending, g.wb, steps_host, nrun_host);
    if (bad) {
        set_last_error("accbpg_fw_div_probe_step: pivot index %lld outside [0, n)", (long long)bad->probe.i);
        return ACCBPG_ERR_ARG;
    }
    return ACCBPG_OK;
}

// a row of pinned records before a run: "not reached"
static void fw_div_steps_reset(accbpg_fw_div_step* row, int nsteps) {
    for (int k = 0; k < nsteps; ++k) {
        row[k] = accbpg_fw_div_step{};
        row[k].probe.i = -1;
        row[k].status = FWD_NOT_RUN;
    }
}
// ... and after it: copy the row out, count the records that ran and leave on the handle what the step-by-step entries
// would have left where the call ended (`pending`: the handle's fw_div_i when the call started).  Returns the first
// record whose pivot lay outside [0, n).
static const accbpg_fw_div_step* fw_div_steps_harvest(accbpg_dopt* h, const accbpg_fw_div_step* pinned, int nsteps,
                                                      bool classical, int64_t pending, unsigned wb,
                                                      accbpg_fw_div_step* steps_host, int* nrun_host) {
    const int64_t n = h->n;
    int nrun = 0, last = -1;                                    // last: the last record behind which the state moved
    const accbpg_fw_div_step* bad = nullptr;
    for (int k = 0; k < nsteps; ++k) {
        steps_host[k] = pinned[k];
        if (pinned[k].status == FWD_NOT_RUN) continue;
        ++nrun;
        const bool in_range = pinned[k].probe.i >= 0 && pinned[k].probe.i < n;
        if (!in_range && !bad) bad = pinned + k;
        if (pinned[k].status != FWD_HANDED_BACK || !classical) last = k;
    }
    *nrun_host = nrun;
    if (last < 0) {                                             // (classical: the first step was handed back)
        h->fw_div_i = pending;
    } else {
        const accbpg_fw_div_step& r = pinned[last];
        const bool ends_on_probe = classical || r.status == FWD_HANDED_BACK;
        if (ends_on_probe) {
            const bool in_range = r.probe.i >= 0 && r.probe.i < n;
            h->fw_div_i = in_range ? r.probe.i : -1;
            double* pin = h->fw_div_pin;                        // the pending probe's record, as _probe_step leaves it
            reinterpret_cast<int64_t*>(pin)[0] = r.probe.i;
            pin[1] = r.probe.w_i; pin[2] = r.probe.x_i; pin[3] = r.probe.sum_w; pin[4] = r.probe.sum_w2;
            pin[5] = r.probe.slope; pin[6] = r.probe.div; pin[7] = r.probe.min_x; pin[8] = r.probe.sum_u2;
        } else {
            h->fw_part_nblk = (int)wb;                          // the stage-1 records of the last update of w
        }
    }
    return bad;
}

extern "C" int accbpg_fw_set_state(accbpg_dopt* h, const double* x_dev, const double* w_dev, const double* H_dev) {
    if (!h || !h->fw_ready || !x_dev || !w_dev || !H_dev) {
        set_last_error("accbpg_fw_set_state: no Frank-Wolfe state (call accbpg_fw_init) or a null argument");
        return ACCBPG_ERR_ARG;
    }
    h->fw_part_nblk = 0;
    h->fw_div_i = -1;
    ACC_TRY(device_copy(h->fw_x, x_dev, (size_t)h->n, h->stream));
    ACC_TRY(device_copy(h->fw_w, w_dev, (size_t)h->n, h->stream));
    ACC_TRY(device_copy(h->fw_H, H_dev, (size_t)h->m * h->m, h->stream));
    return ACCBPG_OK;
}

// ---- lock-step batches (accbpg_dopt_batch_fw_*) -----------------------------------------------------------------
// The Frank-Wolfe state stays in the instance handles; a batched call is ONE launch per step kernel over the active
// instances and -- for the probe -- one synchronisation.  What it leaves in an instance (x, w, H, the stage-1 records
// and their bookkeeping) is what the single-handle entries leave, so the two may be mixed.
static int fw_batch_table(accbpg_dopt_batch* b) {
    if (b->fw_table) return ACCBPG_OK;
    std::vector<FwInst> tab((size_t)b->K);
    for (int i = 0; i < b->K; ++i) {
        accbpg_dopt* h = b->inst[i];
        ACC_TRY(fw_alloc(h));
        tab[i] = h->fw;
    }
    ACC_HIP(acc_malloc(&b->fw_table, sizeof(FwInst) * (size_t)b->K, "fw_table"));
    ACC_HIP(hipMemcpy(b->fw_table, tab.data(), sizeof(FwInst) * (size_t)b->K, hipMemcpyHostToDevice));
    return ACCBPG_OK;
}

extern "C" int accbpg_dopt_batch_fw_init(accbpg_dopt_batch* b, const double* x0_dev, int64_t ldx, const int* active_host,
                                         double* logdet_gram_host, int* status_host) {
    if (!b || !x0_dev || !status_host || ldx < b->inst[0]->n) return ACCBPG_ERR_ARG;
    ACC_TRY(fw_batch_table(b));
    for (int i = 0; i < b->K; ++i) {
        if (active_host && !active_host[i]) continue;
        accbpg_dopt* h = b->inst[i];
        h->stream = b->stream;
        double ld = __builtin_nan("");
        const int rc = accbpg_fw_init(h, x0_dev + (size_t)i * ldx, &ld);
        if (rc == ACCBPG_ERR_HIP || rc == ACCBPG_ERR_ARG) return rc;
        if (rc != ACCBPG_OK) h->fw_ready = false;               // (x was overwritten: no state to step from)
        status_host[i] = rc;
        if (logdet_gram_host) logdet_gram_host[i] = ld;
    }
    return ACCBPG_OK;
}

extern "C" int accbpg_dopt_batch_fw_probe(accbpg_dopt_batch* b, int away, const int* active_host,
                                          accbpg_fw_probe* probes_host) {
    if (!b || !probes_host) return ACCBPG_ERR_ARG;
    const accbpg_dopt* h0 = b->inst[0];                         // one shape, one device: every instance's own partition
    const FwGrids g = fw_grids(h0->m, h0->n, h0->num_cu);
    const int64_t m = h0->m, n = h0->n;
    FwProbeArgs pa;
    BatchAct fresh;                                             // instances without stage-1 records for this threshold
    for (int i = 0; i < b->K; ++i) {
        if (active_host && !active_host[i]) continue;
        accbpg_dopt* h = b->inst[i];
        if (!h->fw_ready || !b->fw_table) {
            set_last_error("accbpg_dopt_batch_fw_probe: instance %d has no Frank-Wolfe state (accbpg_dopt_batch_fw_init)", i);
            return ACCBPG_ERR_ARG;
        }
        pa.idx[pa.n] = i;
        pa.nblk[pa.n] = fw_part_waiting(h, away);               // stage 1 came with the last update of w
        if (!pa.nblk[pa.n]) {
            pa.nblk[pa.n] = (int)g.nblk;
            fresh.idx[fresh.n++] = i;
        }
        ++pa.n;
    }
    if (pa.n == 0) return ACCBPG_OK;
    hipStream_t s = b->stream;
    const unsigned na = (unsigned)pa.n;
    if (fresh.n > 0)
        fw_probe_partial_batch_kernel<<<dim3(g.nblk, (unsigned)fresh.n), FB, 0, s>>>(b->fw_table, fresh, m, n, away);
    if (away && g.away2) {
        fw_probe_away_partial_batch_kernel<<<dim3(g.nb2, na), FB, 0, s>>>(b->fw_table, pa, m, n);
        fw_probe_away_final_batch_kernel<<<dim3(1, na), FB, 0, s>>>(b->fw_table, pa, (int)g.nb2, m, n);
    } else {
        fw_probe_final_batch_kernel<<<dim3(1, na), FB, 0, s>>>(b->fw_table, pa, m, n, away);
    }
    ACC_HIP(hipGetLastError());
    ACC_HIP(hipStreamSynchronize(s));                           // every record is in its instance's pinned buffer
    for (int a = 0; a < pa.n; ++a) {
        accbpg_dopt* h = b->inst[pa.idx[a]];
        h->fw_part_nblk = 0;
        h->fw_part_away = (away != 0);
        fw_read_probe(h, __builtin_nan(""), probes_host + pa.idx[a]);
    }
    return ACCBPG_OK;
}

extern "C" int accbpg_dopt_batch_fw_update(accbpg_dopt_batch* b, const int* active_host, const int64_t* p_host,
                                           const double* xscale_host, const double* xadd_host,
                                           const double* hcoef_host, const double* hdiv_host) {
    if (!b || !p_host || !xscale_host || !xadd_host || !hcoef_host || !hdiv_host) return ACCBPG_ERR_ARG;
    accbpg_dopt* h0 = b->inst[0];                               // one shape, one device: every instance's own partition
    const int64_t m = h0->m, n = h0->n, ldv = h0->ldv;
    FwUpdArgs ua;
    BatchAct act;
    for (int i = 0; i < b->K; ++i) {
        if (active_host && !active_host[i]) continue;
        accbpg_dopt* h = b->inst[i];
        if (!h->fw_ready || !b->fw_table || p_host[i] < 0 || p_host[i] >= n) {
            set_last_error("accbpg_dopt_batch_fw_update: instance %d: no Frank-Wolfe state (accbpg_dopt_batch_fw_init) or "
                           "pivot index %lld outside [0, n)", i, (long long)p_host[i]);
            return ACCBPG_ERR_ARG;                              // (nothing has been launched)
        }
        const int a = ua.n++;
        ua.idx[a] = i;
        if (h->fw_part_away) ua.awaymask |= 1ull << a;          // same support threshold as the instance's last probe
        ua.p[a] = p_host[i];
        ua.xscale[a] = xscale_host[i];
        ua.xadd[a] = xadd_host[i];
        ua.hcoef[a] = hcoef_host[i];
        ua.hdiv[a] = hdiv_host[i];
        act.idx[act.n++] = i;
    }
    if (ua.n == 0) return ACCBPG_OK;
    const FwGrids g = fw_grids(h0->m, h0->n, h0->num_cu);
    const unsigned na = (unsigned)ua.n;
    hipStream_t s = b->stream;
    fw_xupdate_gather_batch_kernel<<<dim3(g.gb, na), FB, 0, s>>>(b->fw_table, ua, m, n, ldv);
    fw_gemv_h_batch_kernel<<<dim3(g.hb, na), FB, 0, s>>>(b->fw_table, act, m);
    fw_rank1_batch_kernel<<<dim3(g.rb, na), FB, 0, s>>>(b->fw_table, ua, m);
    prof_begin(h0, PROF_FWV);
    fw_vgemv_partial_batch_kernel<<<dim3(g.vgx, (unsigned)g.ns, na), FB, 0, s>>>(b->fw_table, act, ldv, m, n, g.ns);
    prof_end(h0, PROF_FWV);
    fw_wupdate_probe_batch_kernel<<<dim3(g.wb, na), FB, 0, s>>>(b->fw_table, ua, m, n, g.ns);
    for (int a = 0; a < ua.n; ++a) b->inst[ua.idx[a]]->fw_part_nblk = (int)g.wb;
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

// ---- the Bregman-step probe and apply for the active instances (accbpg_dopt_batch_fw_div_probe / _fw_div_apply) ---
static int fw_div_batch_table(accbpg_dopt_batch* b) {
    if (b->fw_div_table) return ACCBPG_OK;
    std::vector<FwDivInst> tab((size_t)b->K);
    for (int i = 0; i < b->K; ++i) {
        accbpg_dopt* h = b->inst[i];
        ACC_TRY(fw_div_alloc(h));
        tab[i] = FwDivInst{h->fw_div_ws, h->fw_div_pin_dev};
    }
    ACC_HIP(acc_malloc(&b->fw_div_table, sizeof(FwDivInst) * (size_t)b->K, "fw_div_table"));
    ACC_HIP(hipMemcpy(b->fw_div_table, tab.data(), sizeof(FwDivInst) * (size_t)b->K, hipMemcpyHostToDevice));
    return ACCBPG_OK;
}

extern "C" int accbpg_dopt_batch_fw_div_probe(accbpg_dopt_batch* b, double fill, double value, const int* active_host,
                                              accbpg_fw_div_probe* out_host) {
    if (!b || !out_host) return ACCBPG_ERR_ARG;
    accbpg_dopt* h0 = b->inst[0];                               // one shape, one device: every instance's own partition
    const FwGrids g = fw_grids(h0->m, h0->n, h0->num_cu);
    const int64_t m = h0->m, n = h0->n, ldv = h0->ldv;
    FwProbeArgs pa;
    BatchAct act, fresh;                                        // fresh: instances without stage-1 records waiting
    for (int i = 0; i < b->K; ++i) {
        if (active_host && !active_host[i]) continue;
        const accbpg_dopt* h = b->inst[i];
        if (!h->fw_ready || !b->fw_table) {
            set_last_error("accbpg_dopt_batch_fw_div_probe: instance %d has no Frank-Wolfe state (accbpg_dopt_batch_fw_init)", i);
            return ACCBPG_ERR_ARG;                              // (nothing has been launched)
        }
        const int a = pa.n++;
        pa.idx[a] = i;
        act.idx[act.n++] = i;
        pa.nblk[a] = fw_part_waiting(h, 0);                     // stage 1 came with the last update of w
        if (!pa.nblk[a]) {
            pa.nblk[a] = (int)g.nblk;
            fresh.idx[fresh.n++] = i;
        }
    }
    if (pa.n == 0) return ACCBPG_OK;
    ACC_TRY(fw_div_batch_table(b));
    for (int a = 0; a < pa.n; ++a) {
        accbpg_dopt* h = b->inst[pa.idx[a]];
        h->fw_div_i = -1;
        h->fw_part_nblk = 0;
        h->fw_part_away = false;
    }
    hipStream_t s = b->stream;
    const unsigned na = (unsigned)pa.n;
    const int nb = red_blocks(n, FW_DIV_CAP);
    if (fresh.n > 0)
        fw_probe_partial_batch_kernel<<<dim3(g.nblk, (unsigned)fresh.n), FB, 0, s>>>(b->fw_table, fresh, m, n, 0);
    fw_div_probe_partial_batch_kernel<<<dim3((unsigned)nb, na), FB, 0, s>>>(b->fw_table, b->fw_div_table, pa, m, n, fill,
                                                                           value);
    fw_div_probe_final_batch_kernel<<<dim3(1, na), FB, 0, s>>>(b->fw_table, b->fw_div_table, act, nb, ldv, m, n);
    // the direction of every instance's step: Hv = H V[:,i], u = V^T Hv, sum u^2
    fw_gemv_h_batch_kernel<<<dim3(g.hb, na), FB, 0, s>>>(b->fw_table, act, m);
    prof_begin(h0, PROF_FWV);
    fw_vgemv_partial_batch_kernel<<<dim3(g.vgx, (unsigned)g.ns, na), FB, 0, s>>>(b->fw_table, act, ldv, m, n, g.ns);
    prof_end(h0, PROF_FWV);
    fw_div_usum_batch_kernel<<<dim3((unsigned)nb, na), FB, 0, s>>>(b->fw_table, b->fw_div_table, act, g.ns, n);
    fw_div_u2final_batch_kernel<<<dim3(1, na), FB, 0, s>>>(b->fw_div_table, act, nb, n);
    ACC_HIP(hipGetLastError());
    ACC_HIP(hipStreamSynchronize(s));                           // every record is in its instance's pinned buffer
    int bad_inst = -1;
    for (int a = 0; a < pa.n; ++a) {
        const int i = pa.idx[a];
        accbpg_dopt* h = b->inst[i];
        fw_div_read_probe(h, out_host + i);
        if (out_host[i].i < 0 || out_host[i].i >= n) {
            if (bad_inst < 0) bad_inst = i;
            continue;
        }
        h->fw_div_i = out_host[i].i;
    }
    if (bad_inst >= 0) {
        set_last_error("accbpg_dopt_batch_fw_div_probe: instance %d: pivot index %lld outside [0, n)", bad_inst,
                       (long long)out_host[bad_inst].i);
        return ACCBPG_ERR_ARG;
    }
    return ACCBPG_OK;
}

extern "C" int accbpg_dopt_batch_fw_div_apply(accbpg_dopt_batch* b, const int* active_host, const int64_t* p_host,
                                              const double* a_host, double fill, double value, const double* hcoef_host,
                                              const double* hdiv_host) {
    if (!b || !p_host || !a_host || !hcoef_host || !hdiv_host) return ACCBPG_ERR_ARG;
    const accbpg_dopt* h0 = b->inst[0];                         // one shape, one device: every instance's own partition
    const int64_t m = h0->m, n = h0->n;
    FwUpdArgs ua;
    for (int i = 0; i < b->K; ++i) {
        if (active_host && !active_host[i]) continue;
        const accbpg_dopt* h = b->inst[i];
        // the test of accbpg_fw_div_apply, per instance: Hv, vp and u are those of its last div probe
        if (!h->fw_ready || !b->fw_table || p_host[i] < 0 || p_host[i] >= n || h->fw_div_i != p_host[i] ||
            h->fw_part_nblk != 0) {
            set_last_error("accbpg_dopt_batch_fw_div_apply: instance %d: pivot %lld is not the index of the last div probe "
                           "on this state", i, (long long)p_host[i]);
            return ACCBPG_ERR_ARG;                              // (nothing has been launched)
        }
        const int a = ua.n++;
        ua.idx[a] = i;
        ua.p[a] = p_host[i];
        ua.xscale[a] = a_host[i];                               // the step length
        ua.hcoef[a] = hcoef_host[i];
        ua.hdiv[a] = hdiv_host[i];
    }
    if (ua.n == 0) return ACCBPG_OK;
    ACC_TRY(fw_div_batch_table(b));                             // (the probes may all have been single-handle ones)
    const FwGrids g = fw_grids(h0->m, h0->n, h0->num_cu);
    const unsigned na = (unsigned)ua.n;
    hipStream_t s = b->stream;
    fw_div_xupdate_batch_kernel<<<dim3(g.gb, na), FB, 0, s>>>(b->fw_table, ua, n, fill, value);
    fw_rank1_batch_kernel<<<dim3(g.rb, na), FB, 0, s>>>(b->fw_table, ua, m);
    fw_div_wupdate_probe_batch_kernel<<<dim3(g.wb, na), FB, 0, s>>>(b->fw_table, b->fw_div_table, ua, m, n);
    for (int a = 0; a < ua.n; ++a) {
        accbpg_dopt* h = b->inst[ua.idx[a]];
        h->fw_div_i = -1;
        h->fw_part_nblk = (int)g.wb;
    }
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

// ---- several iterations per synchronisation for the active instances (accbpg_dopt_batch_fw_run) ------------------
static int fw_batch_run_alloc(accbpg_dopt_batch* b) {
    if (!b->fw_bsteps_pin) {
        ACC_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->fw_bsteps_pin),
                              sizeof(accbpg_fw_step) * ACCBPG_FW_RUN_MAX * (size_t)b->K, hipHostMallocDefault));
        ACC_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&b->fw_bsteps_dev), b->fw_bsteps_pin, 0));
    }
    if (!b->fw_runs) ACC_HIP(acc_malloc(reinterpret_cast<void**>(&b->fw_runs), sizeof(FwRunSlot) * (size_t)b->K, "fw_runs"));
    return ACCBPG_OK;
}

extern "C" int accbpg_dopt_batch_fw_run(accbpg_dopt_batch* b, int away, const double* eps_host, int nsteps,
                                        const int* active_host, accbpg_fw_step* steps_host, int* nrun_host) {
    if (!b || !eps_host || !steps_host || !nrun_host || nsteps < 1 || nsteps > ACCBPG_FW_RUN_MAX) return ACCBPG_ERR_ARG;
    const accbpg_dopt* h0 = b->inst[0];                         // one shape, one device: every instance's own partition
    const FwGrids g = fw_grids(h0->m, h0->n, h0->num_cu);
    const int64_t m = h0->m, n = h0->n, ldv = h0->ldv;
    FwProbeArgs pa;                                             // the active set, and each instance's nblk at iteration 0
    BatchAct act, fresh;
    ::BatchVals eps;
    for (int i = 0; i < b->K; ++i) {
        if (active_host && !active_host[i]) continue;
        accbpg_dopt* h = b->inst[i];
        if (!h->fw_ready || !b->fw_table) {
            set_last_error("accbpg_dopt_batch_fw_run: instance %d has no Frank-Wolfe state (accbpg_dopt_batch_fw_init)", i);
            return ACCBPG_ERR_ARG;                              // (nothing has been launched)
        }
        const int a = pa.n++;
        pa.idx[a] = i;
        act.idx[act.n++] = i;
        eps.v[a] = eps_host[i];
        pa.nblk[a] = fw_part_waiting(h, away);                  // stage 1 came with the last update of w
        if (!pa.nblk[a]) {
            pa.nblk[a] = (int)g.nblk;
            fresh.idx[fresh.n++] = i;
        }
    }
    if (pa.n == 0) return ACCBPG_OK;
    ACC_TRY(fw_batch_run_alloc(b));
    const unsigned na = (unsigned)pa.n;
    hipStream_t s = b->stream;
    for (int a = 0; a < pa.n; ++a) {                            // (nothing of an earlier call is in flight: it synchronised)
        fw_steps_reset(b->fw_bsteps_pin + (size_t)pa.idx[a] * ACCBPG_FW_RUN_MAX, nsteps);
        b->inst[pa.idx[a]]->fw_part_nblk = 0;                   // (no claim of reuse survives an error return below)
        b->inst[pa.idx[a]]->fw_part_away = (away != 0);
    }
    ACC_HIP(hipMemsetAsync(b->fw_runs, 0, sizeof(FwRunSlot) * (size_t)b->K, s));
    if (fresh.n > 0)
        fw_probe_partial_batch_kernel<<<dim3(g.nblk, (unsigned)fresh.n), FB, 0, s>>>(b->fw_table, fresh, m, n, away);
    for (int k = 0; k < nsteps; ++k) {
        if (away && g.away2) {
            fw_probe_away_partial_brun_kernel<<<dim3(g.nb2, na), FB, 0, s>>>(b->fw_table, b->fw_runs, pa, m, n);
            fw_probe_away_final_brun_kernel<<<dim3(1, na), FB, 0, s>>>(b->fw_table, b->fw_runs, act, eps, (int)g.nb2, m, n,
                                                                       b->fw_bsteps_dev, k);
        } else {
            fw_probe_final_brun_kernel<<<dim3(1, na), FB, 0, s>>>(b->fw_table, b->fw_runs, pa, eps, m, n, away,
                                                                  b->fw_bsteps_dev, k);
        }
        fw_xupdate_gather_brun_kernel<<<dim3(g.gb, na), FB, 0, s>>>(b->fw_table, b->fw_runs, act, m, n, ldv);
        fw_gemv_h_brun_kernel<<<dim3(g.hb, na), FB, 0, s>>>(b->fw_table, b->fw_runs, act, m);
        fw_rank1_brun_kernel<<<dim3(g.rb, na), FB, 0, s>>>(b->fw_table, b->fw_runs, act, m);
        fw_vgemv_partial_brun_kernel<<<dim3(g.vgx, (unsigned)g.ns, na), FB, 0, s>>>(b->fw_table, b->fw_runs, act, ldv, m, n, g.ns);
        fw_wupdate_probe_brun_kernel<<<dim3(g.wb, na), FB, 0, s>>>(b->fw_table, b->fw_runs, act, m, n, g.ns, away ? 1 : 0);
        if (k == 0)
            for (int a = 0; a < pa.n; ++a) pa.nblk[a] = (int)g.wb;   // the next probe's stage 1 came with this update
    }
    const hipError_t launched = hipGetLastError();
    ACC_HIP(hipStreamSynchronize(s));                           // (also behind a launch error: nothing stays in flight)
    ACC_HIP(launched);
    int bad_inst = -1;
    long long bad_p = 0;
    for (int a = 0; a < act.n; ++a) {
        const int i = act.idx[a];
        const accbpg_fw_step* bad = fw_steps_harvest(b->inst[i], b->fw_bsteps_pin + (size_t)i * ACCBPG_FW_RUN_MAX, nsteps,
                                                     g.wb, steps_host + (size_t)i * nsteps, nrun_host + i);
        if (bad && bad_inst < 0) {
            bad_inst = i;
            bad_p = (long long)bad->p;
        }
    }
    if (bad_inst >= 0) {
        set_last_error("accbpg_dopt_batch_fw_run: instance %d: pivot index %lld outside [0, n)", bad_inst, bad_p);
        return ACCBPG_ERR_ARG;
    }
    return ACCBPG_OK;
}

// ---- several Bregman-step iterations per synchronisation for the active instances (accbpg_dopt_batch_fw_div_run) --
static int fw_div_batch_run_alloc(accbpg_dopt_batch* b) {
    if (!b->fw_div_bsteps_pin) {
        ACC_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->fw_div_bsteps_pin),
                              sizeof(accbpg_fw_div_step) * ACCBPG_FW_RUN_MAX * (size_t)b->K, hipHostMallocDefault));
        ACC_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&b->fw_div_bsteps_dev), b->fw_div_bsteps_pin, 0));
    }
    if (!b->fw_div_runs)
        ACC_HIP(acc_malloc(reinterpret_cast<void**>(&b->fw_div_runs), sizeof(FwDivRunSlot) * (size_t)b->K, "fw_div_runs"));
    return ACCBPG_OK;
}

extern "C" int accbpg_dopt_batch_fw_div_run(accbpg_dopt_batch* b, double fill, double value,
                                            const accbpg_fw_div_params* prm_host, int nsteps, const int* active_host,
                                            accbpg_fw_div_step* steps_host, int* nrun_host) {
    if (!b || !prm_host || !steps_host || !nrun_host || nsteps < 1 || nsteps > ACCBPG_FW_RUN_MAX) return ACCBPG_ERR_ARG;
    accbpg_dopt* h0 = b->inst[0];                               // one shape, one device: every instance's own partition
    const FwGrids g = fw_grids(h0->m, h0->n, h0->num_cu);
    const int64_t m = h0->m, n = h0->n, ldv = h0->ldv;
    FwProbeArgs pa;                                             // the active set, and each instance's nblk at iteration 0
    BatchAct act, fresh;
    FwDivInitArgs ia;
    FwDivDecideArgs da;
    int mode = -1;
    for (int i = 0; i < b->K; ++i) {                            // (every refusal below: nothing has been launched)
        if (active_host && !active_host[i]) continue;
        const accbpg_dopt* h = b->inst[i];
        const accbpg_fw_div_params& p = prm_host[i];
        if (!h->fw_ready || !b->fw_table) {
            set_last_error("accbpg_dopt_batch_fw_div_run: instance %d has no Frank-Wolfe state (accbpg_dopt_batch_fw_init)", i);
            return ACCBPG_ERR_ARG;
        }
        if (p.mode < FWD_LINESEARCH || p.mode > FWD_CLASSICAL || (mode >= 0 && p.mode != mode)) {
            set_last_error("accbpg_dopt_batch_fw_div_run: instance %d: mode %d (one mode of 0, 1, 2 for all active instances)",
                           i, (int)p.mode);
            return ACCBPG_ERR_ARG;
        }
        mode = p.mode;
        if (mode == FWD_CLASSICAL && (h->fw_div_i < 0 || h->fw_part_nblk != 0 || p.k0 < 1)) {
            set_last_error("accbpg_dopt_batch_fw_div_run: instance %d: the classical step needs a div probe pending on this "
                           "state, and k0 >= 1", i);
            return ACCBPG_ERR_ARG;
        }
        const int a = pa.n++;
        pa.idx[a] = act.idx[a] = ia.idx[a] = da.idx[a] = i;
        ia.k0[a] = p.k0; ia.L[a] = p.L; ia.ld[a] = p.ld; ia.q[a] = p.q; ia.F_prev[a] = p.F_prev;
        da.gamma[a] = p.gamma; da.ls_ratio[a] = p.ls_ratio; da.epsilon[a] = p.epsilon;
    }
    if (pa.n == 0) return ACCBPG_OK;
    act.n = ia.n = da.n = pa.n;
    const bool classical = mode == FWD_CLASSICAL;
    ACC_TRY(fw_div_batch_table(b));
    ACC_TRY(fw_div_batch_run_alloc(b));
    int64_t pending[BATCH_MAX];
    for (int a = 0; a < pa.n; ++a) {                            // (nothing of an earlier call is in flight: it synchronised)
        accbpg_dopt* h = b->inst[pa.idx[a]];
        fw_div_steps_reset(b->fw_div_bsteps_pin + (size_t)pa.idx[a] * ACCBPG_FW_RUN_MAX, nsteps);
        pending[a] = h->fw_div_i;
        pa.nblk[a] = (int)g.wb;
        if (!classical) {
            pa.nblk[a] = fw_part_waiting(h, 0);                 // stage 1 came with the last update of w
            if (!pa.nblk[a]) {
                pa.nblk[a] = (int)g.nblk;
                fresh.idx[fresh.n++] = pa.idx[a];
            }
        }
        h->fw_part_nblk = 0;                                    // (no claim survives an error return below)
        h->fw_part_away = false;
        h->fw_div_i = -1;
    }
    const unsigned na = (unsigned)pa.n;
    const unsigned nb = (unsigned)red_blocks(n, FW_DIV_CAP);
    hipStream_t s = b->stream;
    const FwInst* tab = b->fw_table;
    const FwDivInst* dtab = b->fw_div_table;
    FwDivRunSlot* runs = b->fw_div_runs;
    accbpg_fw_div_step* steps = b->fw_div_bsteps_dev;
    if (fresh.n > 0) fw_probe_partial_batch_kernel<<<dim3(g.nblk, (unsigned)fresh.n), FB, 0, s>>>(tab, fresh, m, n, 0);
    fw_div_brun_init_kernel<<<1, BATCH_MAX, 0, s>>>(runs, dtab, ia, mode, m, n, fill, value, steps);
    for (int j = 0; j < nsteps; ++j) {
        if (classical) {                                        // apply step k, then the probe behind it
            fw_div_xupdate_brun_kernel<<<dim3(g.gb, na), FB, 0, s>>>(tab, runs, act, n, fill, value);
            fw_rank1_brun_kernel<<<dim3(g.rb, na), FB, 0, s>>>(tab, runs, act, m);
            fw_div_wupdate_probe_brun_kernel<<<dim3(g.wb, na), FB, 0, s>>>(tab, dtab, runs, act, m, n);
        }
        fw_div_probe_partial_brun_kernel<<<dim3(nb, na), FB, 0, s>>>(tab, dtab, runs, pa, m, n, fill, value);
        fw_div_probe_final_brun_kernel<<<dim3(1, na), FB, 0, s>>>(tab, dtab, runs, act, (int)nb, ldv, m, n);
        fw_gemv_h_brun_kernel<<<dim3(g.hb, na), FB, 0, s>>>(tab, runs, act, m);
        fw_vgemv_partial_brun_kernel<<<dim3(g.vgx, (unsigned)g.ns, na), FB, 0, s>>>(tab, runs, act, ldv, m, n, g.ns);
        fw_div_usum_brun_kernel<<<dim3(nb, na), FB, 0, s>>>(tab, dtab, runs, act, g.ns, n);
        fw_div_u2final_brun_kernel<<<dim3(1, na), FB, 0, s>>>(dtab, runs, da, mode, nsteps, (int)nb, m, n, fill, value, j,
                                                              steps);
        if (!classical) {                                       // the step the record describes
            fw_div_xupdate_brun_kernel<<<dim3(g.gb, na), FB, 0, s>>>(tab, runs, act, n, fill, value);
            fw_rank1_brun_kernel<<<dim3(g.rb, na), FB, 0, s>>>(tab, runs, act, m);
            fw_div_wupdate_probe_brun_kernel<<<dim3(g.wb, na), FB, 0, s>>>(tab, dtab, runs, act, m, n);
            if (j == 0)
                for (int a = 0; a < pa.n; ++a) pa.nblk[a] = (int)g.wb;   // the next probe's stage 1 came with this update
        }
    }
    const hipError_t launched = hipGetLastError();
    ACC_HIP(hipStreamSynchronize(s));                           // (also behind a launch error: nothing stays in flight)
    ACC_HIP(launched);
    int bad_inst = -1;
    long long bad_p = 0;
    for (int a = 0; a < pa.n; ++a) {
        const int i = pa.idx[a];
        const size_t row = (size_t)i * ACCBPG_FW_RUN_MAX;
        const accbpg_fw_div_step* bad = fw_div_steps_harvest(b->inst[i], b->fw_div_bsteps_pin + row, nsteps, classical,
                                                             pending[a], g.wb, steps_host + row, nrun_host + i);
        if (bad && bad_inst < 0) {
            bad_inst = i;
            bad_p = (long long)bad->probe.i;
        }
    }
    if (bad_inst >= 0) {
        set_last_error("accbpg_dopt_batch_fw_div_run: instance %d: pivot index %lld outside [0, n)", bad_inst, bad_p);
        return ACCBPG_ERR_ARG;
    }
    return ACCBPG_OK;
}

// the host's replay of one instance's records (fw_div_replay.hpp): no stream, no device call
extern "C" int accbpg_fw_div_replay(const accbpg_fw_div_params* prm, int64_t n, int64_t m, double fill, double value,
                                    const accbpg_fw_div_step* steps, int nrun, double* F_out, double* L_or_alpha_out,
                                    accbpg_fw_div_params* book_out, int* agreed_out, int* verdict_out) {
    return fw_div_replay(prm, n, m, fill, value, steps, nrun, F_out, L_or_alpha_out, book_out, agreed_out, verdict_out);
}

namespace accbpg {
int vt_nsplit(int64_t m, int64_t n, int num_cu) {
    const int64_t colblocks = (n + VG_COLS - 1) / VG_COLS;
    // About 0.8 workgroups per CU in total, NOT several per CU: measured on MI355X, the pass streams fastest
    // when every CU follows one row range (config 3, 64 column blocks: 3 splits = 192 workgroups 124 us per
    // FW step, 4 splits 130, 16 splits 143; Poisson (8192,65536), 128 column blocks: 2 splits 0.835 of the
    // HBM peak, 8 splits 0.815, 1 split 0.76) -- fewer concurrent DRAM streams, and fewer partials to sum.
    int64_t s = (4 * (int64_t)num_cu / 5 + colblocks / 2) / colblocks;
    if (s > VG_MAXSPLIT) s = VG_MAXSPLIT;
    if (s > m / 8) s = m / 8;
    if (s < 1) s = 1;
    return (int)s;
}

// u = V^T q for a row-major m x n matrix: split-row partial sums into upart (nsplit*n doubles), then their sum
int launch_vt_times(const double* V, int64_t ldv, int64_t m, int64_t n, const double* q, double* upart, int nsplit,
                    double* u, bool vec_ok, hipStream_t s) {
    dim3 vg((unsigned)((n + VG_COLS - 1) / VG_COLS), (unsigned)nsplit);
    fw_vgemv_partial_kernel<<<vg, FB, 0, s>>>(V, ldv, m, n, q, nsplit, upart, vec_ok);
    int64_t wb = (n + FB - 1) / FB;
    if (wb > 2048) wb = 2048;
    fw_usum_kernel<<<(int)wb, FB, 0, s>>>(upart, nsplit, n, u);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}

// the two launches above with an instance dimension on their grids; every instance keeps the single launch's partition
int launch_vt_times_batch(const KyInst* tab, int K, int64_t ldv, int64_t m, int64_t n, bool first, int nsplit,
                          hipStream_t s) {
    dim3 vg((unsigned)((n + VG_COLS - 1) / VG_COLS), (unsigned)nsplit, (unsigned)K);
    vt_partial_batch_kernel<<<vg, FB, 0, s>>>(tab, ldv, m, n, first ? 1 : 0, nsplit);
    int64_t wb = (n + FB - 1) / FB;
    if (wb > 2048) wb = 2048;
    vt_usum_batch_kernel<<<dim3((unsigned)wb, (unsigned)K), FB, 0, s>>>(tab, nsplit, n);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}
}  // namespace accbpg

/* u = V^T q  (np.dot(q, V), applications.py:79): one pass over V on the split-row kernel */
extern "C" int accbpg_dopt_vt_times(accbpg_dopt* h, const double* q_dev, double* u_dev) {
    if (!h || !q_dev || !u_dev) return ACCBPG_ERR_ARG;
    return launch_vt_times(h->V, h->ldv, h->m, h->n, q_dev, h->vws, fw_nsplit(h), u_dev, h->vec_ok, h->stream);
}

extern "C" int accbpg_dopt_get_column(accbpg_dopt* h, int64_t j, double* out_dev) {
    if (!h || !out_dev || j < 0 || j >= h->n) return ACCBPG_ERR_ARG;
    int64_t gb = (h->m + FB - 1) / FB;
    if (gb > 1024) gb = 1024;
    column_kernel<<<(int)gb, FB, 0, h->stream>>>(h->V, h->ldv, h->m, j, out_dev);
    ACC_HIP(hipGetLastError());
    return ACCBPG_OK;
}
