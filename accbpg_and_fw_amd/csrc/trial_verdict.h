// The status block of accbpg_dopt_burg_trial and the verdict the host reads off it after the trial's one wait.
// Plain C++ with no HIP dependency: the library includes it, and it compiles alone with a host compiler.
#pragma once
#include <stdint.h>

namespace accbpg {

// Layout in doubles.  Every stage of a trial writes its status words into its own slice of one device block, which one
// copy brings to pinned host memory.  An evaluation's slice is laid out as the handle's own status words are: 16
// scalars (scalar 0 = log det), then 8 int flags.
constexpr int TRIAL_EVAL_DOUBLES = 20;
constexpr int TRIAL_GRAD = 0;       // the gradient evaluation at y
constexpr int TRIAL_VALUE = 20;     // the value evaluation at x
constexpr int TRIAL_LS = 40;        // 4 doubles: <g, x-y>, D(x,y), D(z,z_prev), minimum over the divergences' entries
constexpr int TRIAL_PROX = 44;      // 8 ints: flags 0..3, {bisection, Newton} steps 4..5, the multi-workgroup give-up word 6
constexpr int TRIAL_CMP = 48;       // 1 int: the stamp of the F[k] compare when x_prev differs from the record
constexpr int TRIAL_DOUBLES = 49;

// indices into an evaluation's / the prox's int flags (the same as the library's FLAG_* constants)
constexpr int TRIAL_FLAG_NOT_PD = 0;
constexpr int TRIAL_FLAG_NEG_X = 1;
constexpr int TRIAL_FLAG_NONPOS = 2;
constexpr int TRIAL_FLAG_ABORT = 4;
constexpr int TRIAL_PROX_INFO = 4;
constexpr int TRIAL_PROX_GAVE_UP = 6;

// what the host knew when it enqueued the trial
struct TrialAsked {
    int cmp_stamp;      // stamp of the enqueued F[k] compare; 0: none was enqueued
    int prox_multi;     // the prox ran in its multi-workgroup form (only then is the give-up word written)
};

struct TrialVerdict {
    int replay;         // anything but a clean trial: the caller runs the same trial through the stepwise calls
    int fk_answered;    // (clean trials only) x_prev equals the value record bit for bit: F[k] is the record's value
    int chol_gave_up;   // a one-launch factorisation abandoned a wait: launch per block column from now on
    int prox_gave_up;   // the multi-workgroup prox abandoned a wait: one workgroup from now on
};

inline const int* trial_flags(const double* blk, int eval) {
    return reinterpret_cast<const int*>(blk + eval + 16);
}

inline TrialVerdict trial_verdict(const double* blk, TrialAsked asked) {
    TrialVerdict v = {0, 0, 0, 0};
    const int* fg = trial_flags(blk, TRIAL_GRAD);
    const int* fv = trial_flags(blk, TRIAL_VALUE);
    const int* px = reinterpret_cast<const int*>(blk + TRIAL_PROX);
    const int* cmp = reinterpret_cast<const int*>(blk + TRIAL_CMP);
    v.chol_gave_up = (fg[TRIAL_FLAG_ABORT] != 0) || (fv[TRIAL_FLAG_ABORT] != 0);
    v.prox_gave_up = asked.prox_multi && px[TRIAL_PROX_GAVE_UP] != 0;
    bool bad = v.chol_gave_up || v.prox_gave_up;
    bad = bad || fg[TRIAL_FLAG_NEG_X] || fg[TRIAL_FLAG_NOT_PD] || fv[TRIAL_FLAG_NEG_X] || fv[TRIAL_FLAG_NOT_PD];
    bad = bad || px[TRIAL_FLAG_NONPOS];                 // y.min() > 0, functions.py:270
    bad = bad || !(blk[TRIAL_LS + 3] > 0.0);            // functions.py:252 (a NaN replays too)
    v.replay = bad ? 1 : 0;
    v.fk_answered = (!bad && asked.cmp_stamp != 0 && cmp[0] != asked.cmp_stamp) ? 1 : 0;
    return v;
}

}  // namespace accbpg
