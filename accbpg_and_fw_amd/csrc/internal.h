// Internal declarations shared by the translation units of libaccbpg_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/accbpg_hip.h"
#include "dopt_plan.hpp"

namespace accbpg {

void set_last_error(const char* fmt, ...);
void note_tiles_fallback(const char* where);

// Every device allocation of the library goes through this pair (guard_alloc.hip): hipMalloc / hipFree, unless
// accbpg_debug_guard_bands is on, when the allocation gets a sentinel band on either side.  label names the buffer in
// the report of accbpg_debug_guard_check.  Pinned host memory does not come from here.
hipError_t acc_malloc(void** p, size_t bytes, const char* label);
hipError_t acc_free(void* p);
template <class T>
inline hipError_t acc_malloc(T** p, size_t bytes, const char* label) {
    return acc_malloc(reinterpret_cast<void**>(p), bytes, label);
}

#define ACC_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess) {                                                              \
            ::accbpg::set_last_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call,            \
                                     hipGetErrorString(e__));                                 \
            return ACCBPG_ERR_HIP;                                                            \
        }                                                                                     \
    } while (0)

#define ACC_TRY(call)                       \
    do {                                    \
        int rc__ = (call);                  \
        if (rc__ != ACCBPG_OK) return rc__; \
    } while (0)

// A kernel's limit of dynamic LDS is raised at the launch site, the first time the kernel is launched on a device (the
// attribute belongs to that device's function object): on this runtime a launch that asks for more dynamic LDS than the
// kernel's limit reports NO error -- not from the launch, not from hipGetLastError, not from a synchronize -- and leaves
// garbage (measured; a Gram variant that had been left out of a list of attribute calls went unnoticed until its results
// were compared).  Every launch that passes dynamic LDS goes through ACC_LAUNCH_LDS.
inline int ensure_lds(int device, const void* kernel, int bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, int> limit;
    std::lock_guard<std::mutex> guard(mu);
    const std::pair<int, const void*> key(device, kernel);
    auto it = limit.find(key);
    if (it != limit.end() && it->second >= bytes) return ACCBPG_OK;
    ACC_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    limit[key] = bytes;
    return ACCBPG_OK;
}
// (a kernel name with template commas goes in parentheses)
#define ACC_LAUNCH_LDS(device, kernel, grid, block, lds, stream, ...)                        \
    do {                                                                                     \
        auto k__ = kernel;                                                                   \
        ACC_TRY(::accbpg::ensure_lds((device), reinterpret_cast<const void*>(k__), (int)(lds))); \
        k__<<<(grid), (block), (lds), (stream)>>>(__VA_ARGS__);                              \
    } while (0)

// A batch of same-shaped instances evaluated by ONE launch per kernel family (blockIdx.y = position among the
// active instances): the per-instance pointers live in a device table, the active set travels as a kernel argument.
constexpr int BATCH_MAX = ACCBPG_BATCH_MAX;
struct BatchAct {
    int n = 0;
    int idx[BATCH_MAX] = {};
};
struct BatchInst {
    const double* V;        // design matrix of the instance
    double* slabs;          // stream-K slabs
    double* gram;           // Gram matrix target of func_grad
    double* Lbuf;
    double* Wbuf;
    double* Tbuf;
    double* dscal;          // scalars + status flags of the instance (slice of one array for the whole batch)
    int* dflag;
    int* chol_ready;
};

// Frank-Wolfe state of one instance as the step kernels (fw_kernels.hip) address it: the handle keeps its own
// (accbpg_dopt::fw, filled where the buffers are made), a batch keeps a device table of its instances
struct FwInst {
    double* x;              // fw_x
    double* w;              // fw_w
    double* H;              // fw_H
    double* hv;             // fw_hv: Hv, vp and the probe scratch behind them
    const double* V;
    double* vws;            // row-split partials of u = Hv^T V
    double* q;              // dscal + 10: q of the last update
    double* rec;            // the instance's pinned host record, as the device addresses it
    int64_t vec_ok;         // V rows are 16-byte aligned
};
// What lies behind FwInst::hv: Hv (m doubles), vp (m), 2 * FW_PART_MAX stage-1 probe records (the maximum and the masked
// minimum of each block), then, for the two-stage away search, AWAY_NB stage-2 records and (w_i, i).  Every kernel and
// the allocation go through these.
struct ValIdx {
    double v;
    int64_t i;
};
constexpr int FW_PART_MAX = 512;    // at most this many workgroups write stage-1 records
constexpr int AWAY_NB = 128;        // at most this many slices of the away variant's second stage
constexpr int FW_DIV_CAP = 512;     // block cap of the fixed-tree reductions of accbpg_fw_div_probe_step
__host__ __device__ inline double* fw_vp_of(const FwInst& t, int64_t m) { return t.hv + m; }
__host__ __device__ inline ValIdx* fw_part_of(const FwInst& t, int64_t m) { return reinterpret_cast<ValIdx*>(t.hv + 2 * m); }
__host__ __device__ inline ValIdx* fw_part2_of(const FwInst& t, int64_t m) { return fw_part_of(t, m) + 2 * FW_PART_MAX; }
__host__ __device__ inline ValIdx* fw_mxslot_of(const FwInst& t, int64_t m) { return fw_part2_of(t, m) + AWAY_NB; }
constexpr size_t fw_scratch_doubles(int64_t m) { return (size_t)(2 * m + 2 * (2 * FW_PART_MAX) + 16 + 2 * AWAY_NB + 4); }
// A probe record (the pinned host record, or the scratch one of a device-decided run) holds w_i, w_j, x_j in doubles
// 4..6, q of the last update in double 10, and i, j as two 64-bit integers at double 8: dout / iout of the final stage
__host__ __device__ inline double* fw_rec_d(double* rec) { return rec + 4; }
__host__ __device__ inline int64_t* fw_rec_i(double* rec) { return reinterpret_cast<int64_t*>(rec + 8); }

// The Bregman-step workspace of one instance (accbpg_fw_div_probe_step / accbpg_fw_div_apply) as the kernels address it;
// the handle keeps its own two pointers (fw_div_ws, fw_div_pin_dev), a batch keeps a device table beside fw_table.
// Behind ws: u (n doubles), FW_DIV_CAP block records of five doubles, FW_DIV_CAP partial sums of u^2, (w_i, i).
struct FwDivInst {
    double* ws;             // fw_div_ws
    double* pin;            // the instance's pinned record of 16 doubles, as the device addresses it
};
__host__ __device__ inline double* fw_div_rec_of(double* ws, int64_t n) { return ws + n; }
__host__ __device__ inline double* fw_div_u2part_of(double* ws, int64_t n) { return fw_div_rec_of(ws, n) + 5 * FW_DIV_CAP; }
__host__ __device__ inline ValIdx* fw_div_mxslot_of(double* ws, int64_t n) {
    return reinterpret_cast<ValIdx*>(fw_div_u2part_of(ws, n) + FW_DIV_CAP);
}
constexpr size_t fw_div_ws_doubles(int64_t n) { return (size_t)n + 6 * FW_DIV_CAP + 2; }

struct FwProbeArgs {        // active instances of a probe and the stage-1 records each has waiting
    int n = 0;
    int idx[BATCH_MAX] = {};
    int nblk[BATCH_MAX] = {};
};
struct FwUpdArgs {          // active instances of an update and their scalars, by position in idx
                            // (accbpg_dopt_batch_fw_div_apply: xscale carries the step length a, xadd is unused)
    int n = 0;
    int idx[BATCH_MAX] = {};
    unsigned long long awaymask = 0;    // bit a: support threshold of the fused stage 1 (1e-8 instead of 0)
    int64_t p[BATCH_MAX] = {};
    double xscale[BATCH_MAX] = {}, xadd[BATCH_MAX] = {}, hcoef[BATCH_MAX] = {}, hdiv[BATCH_MAX] = {};
};

// One instance of a batched Kumar-Yildirim start (accbpg_dopt_batch_kyinit) as its lock-step kernels address it: the
// instance's matrix and vt_times workspace, its m directions, and its slices of the call's scratch.  The table lives
// for one call.
struct MinMaxRec;
struct KyInst {
    const double* V;
    double* vws;            // row-split partials of the pass over V (the handle's)
    int64_t vec_ok;         // V rows are 16-byte aligned
    const double* B;        // m*m: row r = the direction of step r
    double* Q;              // m*m: column j at Q + j*m
    double* w;              // n: q^T V of the step
    double* q;              // m: deflated direction
    double* v;              // m: V[:,kmin] - V[:,kmax]
    double* c;              // m: Gram-Schmidt coefficients
    MinMaxRec* part;        // 128 stage-1 records of the arg-extremum
    int64_t* picked;        // 2m
};

// One handle's step as its "run" kernels read it (accbpg_fw_run): written by thread 0 of the probe's final stage, read
// by the update kernels of that step; once stop != 0 every later kernel of the call returns at once
struct FwRun {
    int32_t stop;           // 0 running; 1 the stop test held; 2 pivot outside [0, n)
    int32_t pad;
    int64_t p;
    double xscale, xadd, hcoef, hdiv;
};

// The same for one instance of a batch (accbpg_dopt_batch_fw_run): the batch owns K of these, entry i = instance i.  rec
// is the scratch probe record of the final stage, laid out as the pinned one.  A single handle's accbpg_fw_run owns one.
struct FwRunSlot {
    FwRun run;
    double rec[16];
};

// One handle's Bregman-step run (accbpg_fw_div_run).  run is what the reused "run" kernels read: p, hcoef, hdiv as there,
// xscale carries the step length a; run.stop != 0: every later kernel of the call returns at once; run.pad != 0: the stop
// test held with an applied step -- the kernels of that apply still run, the final stage of the next probe turns it into
// stop.  book and L are the predictor's (fw_div_decide.hpp), rec the scratch probe record laid out as the pinned one.
// A batch (accbpg_dopt_batch_fw_div_run) owns K of these, entry i = instance i; k0 is that instance's iteration number
// at the start of the call (the instances of a batch drift apart), unused on a single handle.
struct FwDivRunSlot {
    FwRun run;
    double ld, q, F_prev, L;
    double rec[16];
    int64_t k0;
};
// What a batched Bregman-step run carries by value: the slot of every active instance at the start of the call (the
// one-thread-per-instance init kernel), and what its decisions read in every iteration (the last stage of the probe)
struct FwDivInitArgs {
    int n = 0;
    int idx[BATCH_MAX] = {};
    int64_t k0[BATCH_MAX] = {};
    double L[BATCH_MAX] = {}, ld[BATCH_MAX] = {}, q[BATCH_MAX] = {}, F_prev[BATCH_MAX] = {};
};
struct FwDivDecideArgs {
    int n = 0;
    int idx[BATCH_MAX] = {};
    double gamma[BATCH_MAX] = {}, ls_ratio[BATCH_MAX] = {}, epsilon[BATCH_MAX] = {};
};

struct CholInst {                                  // one factorisation (one entry per instance of a batched launch)
    const double* src;      // matrix to factor (lower triangle significant), leading dimension ld
    double* L;              // off-diagonal tiles of the factor (may be src: in place)
    double* Ldiag;          // diagonal tiles of the factor
    double* Winv;           // inverses of the diagonal tiles (or null)
    double* logdet;         // scalar result
    int* flags;             // status flags (FLAG_NOT_PD, FLAG_ABORT)
    int* ready;             // hand-off flags, zero at launch: T*T tile flags, 4 per block column (the 16-column pieces of
                            // its factor), 1 per block row (its diagonal tile with the left updates applied)
    double* aux;            // T * CT_AUX doubles
    double* hand;           // T * 64*64 doubles: diagonal tiles on their way from their accumulators to the chain
    long long* trace;       // development aid: CT_NSTAMP wall-clock stamps per block column from the chain workgroups (or null)
};

constexpr int FLAG_NOT_PD = 0;  // index into the device flag array
constexpr int FLAG_NEG_X = 1;
constexpr int FLAG_NONPOS = 2;
constexpr int FLAG_BAD_G = 3;
constexpr int FLAG_ABORT = 4;   // the one-launch Cholesky gave up a wait (co-residency not reached in time)
constexpr int STATUS_DOUBLES = 20;   // 16 scalars + 8 status flags, copied to the host in one piece
constexpr int ACCBPG_RETRY = 100;    // internal: redo the evaluation with the launch-per-column Cholesky

enum ProfKind { PROF_GRAM = 0, PROF_CHOL = 1, PROF_TRTRI = 2, PROF_GRAD = 3, PROF_GRAMFIX = 4, PROF_FWV = 5, PROF_COUNT = 6 };

struct ProfSlot {
    std::vector<hipEvent_t> ev;   // pairs (start, stop)
    size_t used = 0;
    double total_ms = 0.0;
    int64_t launches = 0;
};

}  // namespace accbpg

struct accbpg_dopt {
    const double* V = nullptr;
    int64_t m = 0, n = 0, ldv = 0;
    hipStream_t stream = nullptr;
    int device = 0;
    int num_cu = 256;
    bool big = false;           // use the 256x128 tile for Gram / gradient products
    // set before the plans are built when the handle is one instance of a batch (accbpg_dopt_batch_create)
    bool force_big = false;     // 256x128 tiles also below m = 768 (interior shapes only)
    int gram_grid_cap = 0;      // stream-K workgroups of this instance's Gram launch (0: the whole chip)
    double* dscal_ext = nullptr;   // scalars + flags live in this slice of the batch's array instead of an own allocation
    bool vec_ok = false;        // V rows are 16-byte aligned

    double* Lbuf = nullptr;     // m*m : Gram matrix, then its Cholesky factor (lower)
    double* Wbuf = nullptr;     // m*m : inverse of the factor (lower, upper stays zero)
    double* Tbuf = nullptr;     // m*m : scratch of the inverse merges / FW refactorisation
    double* slabs = nullptr;    // stream-K partial accumulators
    accbpg::TileRC* tiles = nullptr;
    int64_t* wg_ranges = nullptr;     // [gram_grid][GRAM_RMAX][2] unit ranges of the Gram stream-K walk
    int32_t* gram_cstart = nullptr;   // per (entry, half): first index into gram_contrib
    int32_t* gram_contrib = nullptr;  // (workgroup, slab slot) pairs in k order
    int ntiles = 0, gram_grid = 0, gram_per = 0, gram_nslot = 2;
    int64_t kiters = 0;
    int gram_chunks = 1;        // column blocks of V the Gram matrix is formed over (one launch each; rows >= 65536 long)
    int64_t gram_nc = 0;        // columns per block
    double* Vblk = nullptr;     // owned copy of V stored block by block (rows >= 1 MiB apart only), read by the Gram launches
    double* dscal = nullptr;    // device scalars
    int* dflag = nullptr;       // device status flags
    double* hpin = nullptr;     // pinned host mirror (scalars then flags)
    double* vws = nullptr;      // vector-kernel workspace
    double* xbuf = nullptr;     // 16-byte aligned copy of an unaligned x (lazy)

    accbpg::GemmOp* ops = nullptr;            // device op table of the inverse merges
    std::vector<accbpg::GemmOp> ops_host;
    std::vector<accbpg::RedOp> red_host;
    using MergeStage = accbpg::MergeStage;    // launch list of the inverse merges (dopt_plan.hpp)
    std::vector<MergeStage> merge_stages;
    accbpg::RedOp* red = nullptr;
    double* Pbuf = nullptr;     // m*m: split-K partial products of the top merge levels
    accbpg::GemmOp* chol_op = nullptr;        // device slot for the trailing-update op

    // Frank-Wolfe state
    double *fw_x = nullptr, *fw_w = nullptr, *fw_H = nullptr, *fw_hv = nullptr;
    double* fw_hpin_dev = nullptr;  // device address of the pinned host record hpin (the probe's final stage writes there)
    accbpg::FwInst fw{};            // the above as the step kernels address them (filled by the allocation)
    bool fw_ready = false;
    // log det(H) of the away-step variant (D_opt_alg.py:136) factored beside the steps: a ring of snapshot slots, each an
    // auxiliary handle (own buffers, own stream) that factors a copy of H_k while the main stream goes on
    struct FwSlot {
        accbpg_dopt* aux = nullptr;     // owns snapshot / factor buffers, scalars, pinned mirror, ev_done
        hipStream_t stream = nullptr;   // created here
        hipEvent_t ev_snap = nullptr;   // recorded on the main stream behind the snapshot copy
        bool pending = false;
    };
    std::vector<FwSlot> fw_ring;
    int fw_ring_depth = 1;          // slots in use (factorisations in flight)
    int fw_ring_small = 2;          // how the slots factor: 0 one launch, 1 a launch per block column, 2 by size (as
                                    // accbpg_dopt_factor_in_small_launches)
    long long fw_ring_issued = 0, fw_ring_collected = 0;
    int fw_part_nblk = 0;       // probe stage-1 records left behind by the last w update (0: none)
    bool fw_part_away = false;  // support threshold they were computed for
    // accbpg_fw_run: the step's scalars and a scratch probe record on the device, the records of a call in pinned host
    // memory (allocated by the first call, freed with the handle)
    accbpg::FwRunSlot* fw_run = nullptr;
    accbpg_fw_step* fw_steps_pin = nullptr;     // ACCBPG_FW_RUN_MAX records
    accbpg_fw_step* fw_steps_dev = nullptr;     // ... as the device addresses them
    // accbpg_fw_div_probe_step / accbpg_fw_div_apply: u of the probed direction and the reduction records on the device,
    // the probe record in pinned host memory (allocated by the first probe, freed with the handle)
    double* fw_div_ws = nullptr;
    double* fw_div_pin = nullptr;
    double* fw_div_pin_dev = nullptr;           // ... as the device addresses it
    int64_t fw_div_i = -1;                      // index of the last probe while its Hv and u are current, else -1
    // accbpg_fw_div_run: the predictor's slot on the device, the records of a call in pinned host memory (allocated by
    // the first call, freed with the handle)
    accbpg::FwDivRunSlot* fw_div_run = nullptr;
    accbpg_fw_div_step* fw_div_steps_pin = nullptr;     // ACCBPG_FW_RUN_MAX records
    accbpg_fw_div_step* fw_div_steps_dev = nullptr;     // ... as the device addresses them

    bool use_glds = true;       // direct-to-LDS staging for interior big tiles (debug switch)
    int kern_variant = 0;       // schedule of the direct-to-LDS Gram / gradient kernels (development switch)
    int gram_rolled = 0;        // kern_variant 0 runs the Gram k-loop rolled over a runtime stage index (development switch)
    bool diag_inv_ready = false;  // the last factorisation wrote the inverses of the diagonal blocks into Wbuf
    bool has_duals = false;     // the Gram tile list holds dual diagonal tiles (direct-to-LDS kernel only)
    int chol_nk = 8;            // block columns per outer panel of the two-level scheme
    int chol_two_level_T = 64;  // block columns from which the Cholesky runs its two-level scheme (m > 4032)
    int chol_dbg = 0;           // timing ablation bits for chol_step_kernel (0 in production)
    // one-launch Cholesky (tile owners, T <= 32 block columns)
    bool chol_tiles_ok = false;     // the grid fits the chip (checked against the occupancy query at creation)
    bool chol_tiles_off = false;    // switched off (debug bit, or after a wait timed out)
    int chol_stall_test = 0;        // debug: make the launch time out
    long long chol_spin_limit = 20000000;   // 0.2 s of the 100 MHz wall clock
    int chol_tiles_grid = 0;
    int chol_slots = 0;             // workgroups of the one-launch kernel the chip holds at once (occupancy query x CUs, at most 2 per CU)
    void* chol_jobs = nullptr;      // CholJob[chol_tiles_grid]
    int* chol_ready = nullptr;      // T*T hand-off flags
    double* chol_aux = nullptr;     // T * CT_AUX doubles
    double* chol_hand = nullptr;    // T * 64*64 doubles: diagonal tiles handed from their accumulators to the chain
    long long* chol_trace = nullptr;   // development aid: stage stamps of the chain workgroups (null in production)
    double* Gbuf = nullptr;         // m*m: Gram matrix of func_grad when the one-launch Cholesky is in use (kept intact for a redo)
    const double* last_x = nullptr; // arguments of the evaluation in flight (for a redo)
    double* last_g = nullptr;
    int last_flag = 0;
    hipEvent_t ev_done = nullptr;   // recorded behind the result copy of every begin/end evaluation
    // record of the last value-only (flag 0) begin/end evaluation that completed without error; a later flag-0 begin
    // at the same device address whose 64-bit content equals the copy is answered with val_f (accbpg_dopt_value_reuse)
    bool val_reuse = true;          // look up and keep the record
    bool val_valid = false;         // the record is complete (host side; cleared while a flag-0 evaluation is in flight)
    bool val_pending = false;       // a flag-0 evaluation is in flight whose _end completes the record
    bool val_hit = false;           // the evaluation in flight was answered: _end returns val_answer
    const double* val_x = nullptr;  // the caller's device address of x
    double* val_copy = nullptr;     // n doubles: x as it was evaluated; behind them the compare kernel's result word
                                    // (allocated by the first flag-0 evaluation or lookup)
    double val_f = 0.0;             // f of the record
    double val_answer = 0.0;        // f of the answered evaluation in flight (from this record or the peer's)
    int val_gen = 0;                // stamp the next compare launch writes when it finds a difference
    int64_t val_compares = 0, val_answered = 0;
    // accbpg_dopt_burg_trial: the status words of a trial's stages, one slice each (trial_verdict.h), and their pinned
    // mirror (allocated by the first trial, freed with the handle)
    double* trial_stat = nullptr;
    double* trial_pin = nullptr;
    accbpg_dopt* val_peer = nullptr;            // lookups consult this handle's record after the own (read-only)
    std::vector<accbpg_dopt*> val_linked;       // the handles whose val_peer is this one (unlinked by destroy)
    bool prof_on = false;
    accbpg::ProfSlot prof[accbpg::PROF_COUNT];
};

// A batch of same-shaped D-optimal instances evaluated together (accbpg_dopt_batch_*)
struct accbpg_dopt_batch {
    int K = 0;
    std::vector<accbpg_dopt*> inst;
    hipStream_t stream = nullptr;
    int device = 0;
    bool fast = false;                      // one launch per kernel family over the active instances
    int chunk = 0;                          // ... at most this many instances per launch (their one-launch
                                            // factorisations must fit the chip together)
    accbpg::BatchInst* table = nullptr;     // device, K entries
    accbpg::CholInst* chol_table[2] = {nullptr, nullptr};   // device, K entries each: without / with diagonal-block inverses
    accbpg::GemmOp* ops_all = nullptr;      // device: the merge op tables of all instances, instance after instance
    accbpg::RedOp* red_all = nullptr;
    int ops_per_inst = 0, red_per_inst = 0;
    double* dscal_all = nullptr;            // device, K * 24 doubles (scalars + flags of every instance)
    double* hpin = nullptr;                 // pinned mirror
    // scratch of the batched length-n kernels (vec_kernels.hip), allocated on first use
    int* vflags = nullptr;                  // K * 8 ints: status flags + {bisection, newton} of the prox
    double* vout = nullptr;                 // K * 4 doubles: reduction results
    double* vpart = nullptr;                // K * 4 * 1024 doubles: reduction partials
    double* vws = nullptr;                  // workspace of the single-instance prox (long vectors, one instance at a time)
    double* vquot = nullptr;                // gavg / csum of one instance (avg_prox on long vectors), n doubles
    double* vpin = nullptr;                 // pinned mirror (K * 8 doubles)
    accbpg::FwInst* fw_table = nullptr;     // device, K entries: Frank-Wolfe state of every instance (built by the first accbpg_dopt_batch_fw_init)
    accbpg::FwDivInst* fw_div_table = nullptr;  // device, K entries: their Bregman-step workspaces (built by the first accbpg_dopt_batch_fw_div_*)
    // accbpg_dopt_batch_fw_run (allocated by the first call): every instance's step scalars + scratch record on the
    // device, and the records of a call in pinned host memory, row i (ACCBPG_FW_RUN_MAX records) = instance i
    accbpg::FwRunSlot* fw_runs = nullptr;
    accbpg_fw_step* fw_bsteps_pin = nullptr;
    accbpg_fw_step* fw_bsteps_dev = nullptr;    // ... as the device addresses them
    // accbpg_dopt_batch_fw_div_run (allocated by the first call): every instance's predictor slot on the device, and the
    // records of a call in pinned host memory, row i (ACCBPG_FW_RUN_MAX records) = instance i
    accbpg::FwDivRunSlot* fw_div_runs = nullptr;
    accbpg_fw_div_step* fw_div_bsteps_pin = nullptr;
    accbpg_fw_div_step* fw_div_bsteps_dev = nullptr;    // ... as the device addresses them
    // the evaluation in flight between _begin and _end
    accbpg::BatchAct pend_act;
    const double* pend_x = nullptr;
    double* pend_g = nullptr;
    int64_t pend_ldx = 0, pend_ldg = 0;
    int pend_flag = 0;
    bool pend_fused = false;
};
struct BatchVals { double v[accbpg::BATCH_MAX]; };          // one scalar per instance, as a kernel argument

namespace accbpg {

// batched launches over the active instances (dopt_kernels.hip)
int launch_gram_batch(accbpg_dopt_batch* b, const BatchAct& act, const double* xbase, int64_t ldx);
int launch_cholesky_batch(accbpg_dopt_batch* b, const BatchAct& act, bool with_inverse, const double* xbase, int64_t ldx);
int launch_trtri_batch(accbpg_dopt_batch* b, const BatchAct& act);
int launch_colnorm_batch(accbpg_dopt_batch* b, const BatchAct& act, double* gbase, int64_t ldg, double sign);

// dopt_kernels.hip
int dopt_init(accbpg_dopt* h);
int launch_gram(accbpg_dopt* h, const double* x, double* gram);
int launch_cholesky(accbpg_dopt* h, double* A /* m*m, factor goes here */, double* Winv = nullptr /* diagonal-block inverses */,
                    const double* xcheck = nullptr /* x >= 0 check folded into the reset launch */,
                    const double* src = nullptr /* matrix to factor when it is not A itself */,
                    double* xkeep = nullptr /* n doubles: receives a copy of xcheck in the same pass */,
                    double* status = nullptr /* 16 scalars + 8 int flags of this factorisation when not the handle's own */);
bool chol_tiles_usable(const accbpg_dopt* h);
int launch_trtri(accbpg_dopt* h);
int launch_colnorm(accbpg_dopt* h, const double* W, double* out, double sign);
int launch_gemm_ops(const GemmOp* ops_dev, int nops, int maxM, int maxN, bool b_kmajor, hipStream_t s);
int launch_test_gemm(const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                     int64_t M, int64_t N, int64_t K, int b_kmajor, double alpha, double beta, int config,
                     hipStream_t s);
int build_plans(accbpg_dopt* h);
void set_plan_flags(int flags);
int set_gemm_loop(int variant);
int debug_gram_variant(accbpg_dopt* h, const double* x, int var, int iters, double* ms_out);
int debug_grad_variant(accbpg_dopt* h, double* out, int var, int iters, double* ms_out);
int mfma_peak(int iters, double* tflops, hipStream_t s);
int pipe_probe(int iters, int mode, double* ms_out, hipStream_t s);

// vec_kernels.hip
int64_t vec_ws_doubles(int64_t n);
// per-(thread, device) scratch of the handle-free entry points: pinned host (32 doubles), device flags (8 ints),
// device result scalars (16 doubles)
int vec_scratch(double** pin, int** flags, double** out);
// the length-n stages of accbpg_dopt_burg_trial: the launches of accbpg_burg_simplex_div_prox (in the form its dispatch
// picks for n; flags8 = 8 device ints: flags, {bisection, newton}, and at gave_up_idx the multi-workgroup form's give-up
// word) and of accbpg_ls_terms (out4 = 4 device doubles), enqueued on s with no wait
int trial_prox_enqueue(const double* y_dev, const double* g_dev, double L, double eps, int64_t n, double* x_out_dev,
                       double* ws_dev, int* flags8, int gave_up_idx, hipStream_t s, bool* multi);
void trial_prox_gave_up();
int trial_ls_terms_enqueue(const double* g_dev, const double* x_dev, const double* y_dev, const double* z_dev,
                           const double* z1_dev, int64_t n, double* ws_dev, double* out4_dev, hipStream_t s);

// fw_kernels.hip
int vt_nsplit(int64_t m, int64_t n, int num_cu);
int launch_vt_times(const double* V, int64_t ldv, int64_t m, int64_t n, const double* q, double* upart, int nsplit,
                    double* u, bool vec_ok, hipStream_t s);
// the same for the K instances of a table in lock-step: w_i = V_i^T q_i (first: V_i^T B_i[0], the direction of step 0)
int launch_vt_times_batch(const KyInst* tab, int K, int64_t ldv, int64_t m, int64_t n, bool first, int nsplit,
                          hipStream_t s);
constexpr int VT_MAXSPLIT = 64;

// device-to-device copy as a kernel on the stream (no copy-engine hand-off between producer and consumer kernels)
int device_copy(double* dst, const double* src, size_t ndoubles, hipStream_t s);

// prof helpers
void prof_begin(accbpg_dopt* h, ProfKind k);
void prof_end(accbpg_dopt* h, ProfKind k);

}  // namespace accbpg
