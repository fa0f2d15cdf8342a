// The scalar decisions of one iteration of the Bregman-step Frank-Wolfe solvers (D_opt_FW_div_step /
// D_opt_FW_descent_step of the Python package), free of HIP: plain C++ over <cmath>, compiled by the host compiler in
// tests/test_fw_div_decide_cpu.py and inside fw_kernels.hip (built with -ffp-contract=off), where thread 0 of the last
// stage of a probe calls it (accbpg_fw_div_run).  The text follows D_opt_alg.py's _DivStepRun.decide, _DivBook.value /
// .scalars, algorithms_fw.py's _step_length and _DescentRun.step / .probed operation for operation: every + - * / in
// the order Python evaluates it, log where it says math.log, pow where it says **, min as Python's min, and comparisons
// through which a NaN falls as it does there.
//
// The device PREDICTS with this text and the host CHECKS: log and pow of the device need not round as the host's libm
// does, so the caller replays every record through the Python copy and owns the result.  Wherever the Python text would
// raise, leave the rank-one path or loop without a bound, the functions here hand the iteration back instead of
// deciding it (FWD_HB_*).
#ifndef ACCBPG_FW_DIV_DECIDE_HPP
#define ACCBPG_FW_DIV_DECIDE_HPP
#include <cmath>

#ifndef ACCBPG_FW_DIV_TRIALS_MAX
#define ACCBPG_FW_DIV_TRIALS_MAX 64     // line-search trials of one iteration; ample at ls_ratio >= 1.2
#endif
#if defined(__HIPCC__) || defined(__HIP__)
#define ACCBPG_FWD_FN __host__ __device__ inline
#else
#define ACCBPG_FWD_FN inline
#endif

namespace accbpg {

enum FwdMode { FWD_LINESEARCH = 0, FWD_FIXED_L = 1, FWD_CLASSICAL = 2 };
enum FwdStatus { FWD_APPLIED = 0, FWD_STOPPED = 1, FWD_HANDED_BACK = 2, FWD_NOT_RUN = 3 };
enum FwdReason {
    FWD_HB_NONE = 0,
    FWD_HB_BUDGET = 1,      // ACCBPG_FW_DIV_TRIALS_MAX trials without an accepted one
    FWD_HB_L_INF = 2,       // "L is infinite"
    FWD_HB_SLOPE = 3,       // "grad_d_prod must be non-positive"
    FWD_HB_MIN_X = 4,       // "Entries of x or y not positive."
    FWD_HB_PIVOT = 5,       // pivot outside [0, n)
    FWD_HB_CAP = 6,         // a is not < 1: the capped step (a full evaluation and a re-initialisation), or a NaN
    FWD_HB_ARITH = 7        // Python's arithmetic raises here (division by zero, overflow of **, log of a non-positive)
};

constexpr double FWD_SLOPE_FLOOR = 1e-6;    // _SLOPE_FLOOR (algorithms_fw.py)

struct FwdBook {            // _DivBook plus F[k-1] of the stop test
    double ld, q, m, radius, fill, F_prev;
};
struct FwdOut {
    double L;               // accepted (div step); untouched by the classical step
    int trials;
    double a, hcoef, hdiv, ld1, q1, f1;
    double fx;              // F[k]
    int status, reason;
};

// x ** y on two Python floats; false where Python raises (or leaves the reals)
ACCBPG_FWD_FN bool fwd_pow(double x, double y, double* r) {
    if (y == 0.0) { *r = 1.0; return true; }
    if (y == 1.0) { *r = x; return true; }      // what a correctly rounded pow returns; the device's pow is not one, and
                                                // at gamma == 2 the step length must not depend on it
    if (x == 0.0 && y < 0.0) return false;                               // ZeroDivisionError
    const bool fin = !__builtin_isinf(x) && !__builtin_isinf(y) && x == x && y == y;
    if (fin && x < 0.0 && floor(y) != y) return false;                   // a complex result
    const double v = pow(x, y);
    if (fin && __builtin_isinf(v)) return false;                         // OverflowError
    *r = v;
    return true;
}

// _step_length: min((-slope / (2 * L * dist)) ** (1 / (gamma - 1)), 1.0)
ACCBPG_FWD_FN bool fwd_step_length(double slope, double L, double dist, double gamma, double* a) {
    const double den = 2.0 * L * dist;
    const double g1 = gamma - 1.0;
    if (den == 0.0 || g1 == 0.0) return false;
    double r;
    if (!fwd_pow(-slope / den, 1.0 / g1, &r)) return false;
    *a = (1.0 < r) ? 1.0 : r;                                            // Python's min(r, 1.0)
    return true;
}

// _DivBook.value
template <class Probe>
ACCBPG_FWD_FN double fwd_value(const FwdBook& b, const Probe& rec) {
    return -b.ld - b.q * rec.sum_w;
}

// _DivBook.scalars (a < 1): hcoef, hdiv, ld1, q1, f1 into out
template <class Probe>
ACCBPG_FWD_FN bool fwd_scalars(const FwdBook& b, double a, const Probe& rec, FwdOut* out) {
    const double tau = a * (b.radius - b.fill) / (1.0 - a);
    const double den = 1.0 + tau * rec.w_i;
    if (den == 0.0) return false;
    const double hcoef = -tau / den;
    const double hdiv = 1.0 - a;
    if (hdiv <= 0.0 || den < 0.0) return false;                          // math.log: domain error
    const double ld1 = b.ld + b.m * log(hdiv) + log(den);
    const double q1 = b.q + a * (b.fill - b.q);
    const double sw1 = (rec.sum_w + hcoef * rec.sum_u2) / hdiv;
    out->hcoef = hcoef; out->hdiv = hdiv; out->ld1 = ld1; out->q1 = q1;
    out->f1 = -ld1 - q1 * sw1;
    return true;
}

ACCBPG_FWD_FN void fwd_hand_back(FwdOut* out, int reason) {
    out->status = FWD_HANDED_BACK;
    out->reason = reason;
}

// _DivStepRun.decide for iteration k: mode FWD_LINESEARCH or FWD_FIXED_L.  On FWD_APPLIED / FWD_STOPPED (the step is
// applied, then the solver stops) the book and *L are advanced; on FWD_HANDED_BACK nothing is.
template <class Probe>
ACCBPG_FWD_FN void fw_div_decide(const Probe& rec, long long n, FwdBook* book, double* Lio, int mode, double gamma,
                                 double ls_ratio, double epsilon, long long k, FwdOut* out) {
    const bool linesearch = (mode == FWD_LINESEARCH);
    out->L = *Lio; out->trials = 0; out->a = 0.0; out->hcoef = 0.0; out->hdiv = 0.0;
    out->ld1 = book->ld; out->q1 = book->q; out->f1 = 0.0; out->status = FWD_APPLIED; out->reason = FWD_HB_NONE;
    const double fx = fwd_value(*book, rec);
    out->fx = fx;
    if (!(rec.i >= 0 && rec.i < n)) return fwd_hand_back(out, FWD_HB_PIVOT);

    const double div = (rec.div != 0.0) ? rec.div : FWD_SLOPE_FLOOR;
    double slope = rec.slope;
    if (0.0 < slope && slope <= FWD_SLOPE_FLOOR) slope = 0.0;
    if (slope > 0.0) return fwd_hand_back(out, FWD_HB_SLOPE);
    if (!(rec.min_x > 0.0)) return fwd_hand_back(out, FWD_HB_MIN_X);

    double L = *Lio;
    if (linesearch) {
        if (ls_ratio == 0.0) return fwd_hand_back(out, FWD_HB_ARITH);
        L = L / ls_ratio;
    }
    bool accepted = false;
    int t = 0;
    for (; t < ACCBPG_FW_DIV_TRIALS_MAX; ++t) {
        double a;
        if (!fwd_step_length(slope, L, div, gamma, &a)) return fwd_hand_back(out, FWD_HB_ARITH);
        if (!(a < 1.0)) return fwd_hand_back(out, FWD_HB_CAP);
        out->trials = t + 1;                                             // trials that reached _DivBook.scalars
        if (!fwd_scalars(*book, a, rec, out)) return fwd_hand_back(out, FWD_HB_ARITH);
        out->a = a;
        if (!linesearch) { accepted = true; break; }
        if (__builtin_isinf(L)) return fwd_hand_back(out, FWD_HB_L_INF);
        double ag;
        if (!fwd_pow(a, gamma, &ag)) return fwd_hand_back(out, FWD_HB_ARITH);
        if (out->f1 <= fx + a * slope + ag * L * div) { accepted = true; break; }
        L = L * ls_ratio;
    }
    if (!accepted) return fwd_hand_back(out, FWD_HB_BUDGET);

    out->L = L;
    *Lio = L;
    const double d = fx - book->F_prev;
    const bool stop = k > 0 && fabs(d) < epsilon;
    book->ld = out->ld1; book->q = out->q1; book->F_prev = fx;
    out->status = stop ? FWD_STOPPED : FWD_APPLIED;
}

// _DescentRun.step: the step of iteration k >= 1 from the record of the probe before it; the book is advanced
template <class Probe>
ACCBPG_FWD_FN void fw_descent_step(const Probe& rec, long long n, FwdBook* book, long long k, FwdOut* out) {
    out->trials = 0; out->status = FWD_APPLIED; out->reason = FWD_HB_NONE;
    out->a = 0.0; out->hcoef = 0.0; out->hdiv = 0.0; out->ld1 = book->ld; out->q1 = book->q; out->f1 = 0.0;
    if (!(rec.i >= 0 && rec.i < n)) return fwd_hand_back(out, FWD_HB_PIVOT);
    const double a = 2.0 / (double)(k + 2);
    if (!fwd_scalars(*book, a, rec, out)) return fwd_hand_back(out, FWD_HB_ARITH);
    out->a = a;
    book->ld = out->ld1; book->q = out->q1;
}

// _DescentRun.probed: F[k] from the record of the probe behind step k, and the stop test
template <class Probe>
ACCBPG_FWD_FN bool fw_descent_probed(const Probe& rec, FwdBook* book, double epsilon, double* Fk) {
    const double f = fwd_value(*book, rec);
    const double d = f - book->F_prev;
    const bool stop = fabs(d) < epsilon || sqrt(rec.sum_w2) < epsilon;
    book->F_prev = f;
    *Fk = f;
    return stop;
}

}  // namespace accbpg
#endif
