// The host's replay of the records of accbpg_fw_div_run / accbpg_dopt_batch_fw_div_run, free of HIP: plain C++ over
// fw_div_decide.hpp, compiled by the host compiler in tests/test_fw_div_replay_cpu.py and into the library behind
// accbpg_fw_div_replay (no stream, no device call).  It is the loop of D_opt_alg.py's _div_device_steps /
// _descent_device_steps over the records that AGREE: per record, copy the book, take the host's decision on the
// record's probe with the host's libm, compare it with the device's bit for bit (NaN equal to NaN), commit the book only
// if they agree.  It stops at the first record that is not an agreed step and decides nothing about that record: the
// caller takes the returned book and runs that one record through the Python text, which keeps the one copy of the
// roll-back, the hand-back and every exception.
#ifndef ACCBPG_FW_DIV_REPLAY_HPP
#define ACCBPG_FW_DIV_REPLAY_HPP
#include <cmath>
#include <cstdint>
#include "../../include/accbpg_hip.h"
#include "fw_div_decide.hpp"

namespace accbpg {

enum FwdVerdict {
    FWD_RP_END = 0,         // every record agreed
    FWD_RP_STOP = 1,        // an agreed stop; that record is counted
    FWD_RP_DEVICE_HB = 2,   // the device handed the iteration back
    FWD_RP_HOST_HB = 3,     // the host's decision is itself a hand-back (the cap, an arithmetic error)
    FWD_RP_DISAGREE = 4,
    FWD_RP_PIVOT = 5        // pivot outside [0, n)
};

inline bool fwd_same_bits(double a, double b) {
    if (a != a && b != b) return true;
    uint64_t x, y;
    __builtin_memcpy(&x, &a, sizeof x);
    __builtin_memcpy(&y, &b, sizeof y);
    return x == y;
}

// Modes 0 and 1: steps[0 .. nrun) are the records of the call.  Mode 2: steps[0].probe is the probe that was pending
// when the call started (nothing else of steps[0] is read) and steps[1 .. nrun] are the records of the call -- the step
// of record j is decided from the probe of the record before it.
inline int fw_div_replay(const accbpg_fw_div_params* prm, int64_t n, int64_t m, double fill, double value,
                         const accbpg_fw_div_step* steps, int nrun, double* F_out, double* L_or_alpha_out,
                         accbpg_fw_div_params* book_out, int* agreed_out, int* verdict_out) {
    if (!prm || !book_out || !agreed_out || !verdict_out || nrun < 0 || nrun > ACCBPG_FW_RUN_MAX ||
        (nrun > 0 && (!steps || !F_out || !L_or_alpha_out)) || prm->mode < FWD_LINESEARCH || prm->mode > FWD_CLASSICAL)
        return ACCBPG_ERR_ARG;
    const bool classical = prm->mode == FWD_CLASSICAL;
    FwdBook book{prm->ld, prm->q, (double)m, value, fill, prm->F_prev};
    double L = prm->L;
    int j = 0, verdict = FWD_RP_END;
    for (; j < nrun; ++j) {
        const accbpg_fw_div_step& r = steps[classical ? j + 1 : j];
        const long long k = (long long)prm->k0 + j;
        const bool in_range = r.probe.i >= 0 && r.probe.i < n;
        FwdBook b = book;
        FwdOut o;
        if (r.status == FWD_HANDED_BACK) {
            verdict = (!classical && (r.reason == FWD_HB_PIVOT || !in_range)) ? FWD_RP_PIVOT : FWD_RP_DEVICE_HB;
            break;
        }
        if (r.status != FWD_APPLIED && r.status != FWD_STOPPED) { verdict = FWD_RP_DISAGREE; break; }
        if (!classical) {
            if (!in_range) { verdict = FWD_RP_PIVOT; break; }
            double Lj = L;
            fw_div_decide(r.probe, (long long)n, &b, &Lj, prm->mode, prm->gamma, prm->ls_ratio, prm->epsilon, k, &o);
            if (o.status == FWD_HANDED_BACK) { verdict = FWD_RP_HOST_HB; break; }
            if (!(fwd_same_bits(o.a, r.a) && fwd_same_bits(o.hcoef, r.hcoef) && fwd_same_bits(o.hdiv, r.hdiv) &&
                  fwd_same_bits(o.L, r.L) && o.status == r.status)) {
                verdict = FWD_RP_DISAGREE;
                break;
            }
            book = b;
            L = Lj;
            F_out[j] = o.fx;
            L_or_alpha_out[j] = o.L;
            if (o.status == FWD_STOPPED) { verdict = FWD_RP_STOP; ++j; break; }
            continue;
        }
        fw_descent_step(steps[j].probe, (long long)n, &b, k, &o);
        if (o.status == FWD_HANDED_BACK) { verdict = FWD_RP_HOST_HB; break; }
        if (!(fwd_same_bits(o.a, r.a) && fwd_same_bits(o.hcoef, r.hcoef) && fwd_same_bits(o.hdiv, r.hdiv))) {
            verdict = FWD_RP_DISAGREE;                           // (the record's probe saw another state)
            break;
        }
        if (!in_range) { verdict = FWD_RP_PIVOT; break; }
        double Fk;
        const bool stop = fw_descent_probed(r.probe, &b, prm->epsilon, &Fk);
        // (math.sqrt of a negative sum raises where the first half of the stop test does not hold)
        if (!(fabs(Fk - book.F_prev) < prm->epsilon) && r.probe.sum_w2 < 0.0) { verdict = FWD_RP_HOST_HB; break; }
        if (stop != (r.status == FWD_STOPPED)) { verdict = FWD_RP_DISAGREE; break; }
        book = b;
        F_out[j] = Fk;
        L_or_alpha_out[j] = o.a;
        if (stop) { verdict = FWD_RP_STOP; ++j; break; }
    }
    *book_out = *prm;
    book_out->k0 = prm->k0 + j;
    book_out->L = L;
    book_out->ld = book.ld;
    book_out->q = book.q;
    book_out->F_prev = book.F_prev;
    *agreed_out = j;
    *verdict_out = verdict;
    return ACCBPG_OK;
}

}  // namespace accbpg
#endif
