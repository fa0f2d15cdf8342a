/*
 * accbpg_hip.h -- C-ABI of libaccbpg_hip.so: the MI355X (gfx950) implementation of the
 * per-iteration hot path of the accbpg package for D-optimal experiment design.
 *
 * The reference (DredderGun/accbpg_and_fw) is pure Python/NumPy and has no FFI of its own.
 * The seam this library sits behind is the duck-typed f/h object protocol its solver loops
 * call; each entry point below names the reference method whose
 * arithmetic it replaces.  All citations are relative to the reference tree.
 *
 * Conventions
 *   - every pointer named *_dev is a raw device pointer (e.g. torch.Tensor.data_ptr()),
 *     fp64, contiguous unless a leading dimension is given;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     0 / NULL means the default stream;
 *   - *_host outputs are plain host pointers; a call that has host outputs synchronises the
 *     stream before it returns, so the values are valid on return;
 *   - no entry point allocates memory the caller must free, none throws across the ABI;
 *   - return value: ACCBPG_OK, or an ACCBPG_ERR_* code that the Python shim maps to the
 *     exception type the reference raises in the same situation.
 *   - one handle per host thread; handles are bound to the device current at creation.
 */
#ifndef ACCBPG_HIP_H
#define ACCBPG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACCBPG_OK            0
#define ACCBPG_ERR_ASSERT    1   /* precondition violated -> AssertionError (functions.py:44-45,251-252,269-270,340) */
#define ACCBPG_ERR_NOT_PD    2   /* Gram matrix not positive definite -> ValueError (functions.py:48-50) */
#define ACCBPG_ERR_HIP       3   /* HIP runtime failure -> RuntimeError; see accbpg_last_error() */
#define ACCBPG_ERR_ARG       4   /* malformed call (null pointer, bad size) -> ValueError */

typedef struct accbpg_dopt accbpg_dopt;   /* opaque D-optimal objective handle */

int         accbpg_abi_version(void);
const char* accbpg_last_error(void);

/* ---- D-optimal objective: replaces DOptimalObj (accbpg/functions.py:27-59) ------------ */

/* Borrow V (m x n, row-major, leading dimension ldv >= n; the reference's `self.H`,
 * functions.py:32).  V must outlive the handle and must not change while it lives (for rows a megabyte or more
 * apart the handle keeps a copy of V stored in column blocks, which its Gram launches read).  The handle owns all workspace
 * (Gram matrix, Cholesky factor, inverse factor, stream-K slabs, pinned scalars).
 * is_shard != 0: V is a column block of a larger instance (design-point sharding), so the
 * reference's m < n precondition (functions.py:35) applies to the whole instance, not to it. */
int accbpg_dopt_create(const double* V_dev, int64_t m, int64_t n, int64_t ldv,
                       void* stream, accbpg_dopt** out, int is_shard);
int accbpg_dopt_destroy(accbpg_dopt* h);
int accbpg_dopt_set_stream(accbpg_dopt* h, void* stream);

/* func_grad(x, flag) of functions.py:43-59.  flag 0: value only (f_host), 1: gradient only
 * (g_dev), 2: both.  f = -log det(V diag(x) V^T), g_i = -v_i^T (V diag(x) V^T)^-1 v_i.
 * Returns ACCBPG_ERR_ASSERT if min(x) < 0 (functions.py:45), ACCBPG_ERR_NOT_PD if the
 * Cholesky factorisation meets a non-positive pivot (the reference tests slogdet sign <= 0,
 * functions.py:48-50). */
int accbpg_dopt_func_grad(accbpg_dopt* h, const double* x_dev, int flag,
                          double* f_host, double* g_dev);

/* func_grad split into enqueue / wait.  `begin` queues the whole evaluation on the handle's stream
 * and returns; `end` waits for it and reports f and the status.  Two handles on the same V with
 * different streams let INDEPENDENT evaluations overlap -- e.g. F[k] = f(x) and func_grad(y) of the
 * accelerated methods (accbpg/algorithms.py:135 and :148, :347 and :371; y does not depend on f(x)). */
int accbpg_dopt_func_grad_begin(accbpg_dopt* h, const double* x_dev, int flag, double* g_dev);
int accbpg_dopt_func_grad_end(accbpg_dopt* h, double* f_host);

/* *ms_host <- milliseconds from the completion (results on the host) of `first`'s last begin/end evaluation to
 * that of `second`'s; negative when `second` completed earlier.  Both evaluations must have been waited for.
 * Lets the solver stamp T[k] (the reference stamps it right after F[k] = f(x), accbpg/algorithms.py:135-137,
 * 347-349) at the moment f(x) was known although it ran beside the gradient evaluation. */
int accbpg_dopt_eval_gap_ms(accbpg_dopt* first, accbpg_dopt* second, double* ms_host);

/* Repeated value evaluations.  ABPG_gain evaluates f at the accepted line-search point twice (accbpg/algorithms.py:387,
 * then F[k+1] = f(x) at :347) with nothing in between; the kernels are deterministic, so the second result is the first,
 * bit for bit.  Every handle therefore keeps a record of its last VALUE-ONLY evaluation (flag 0 through
 * accbpg_dopt_func_grad_begin/_end or accbpg_dopt_func_grad) that returned ACCBPG_OK: the device address of x, a device
 * copy of x, and f.  A later flag-0 `begin` is ANSWERED with the recorded f -- no Gram product, no factorisation -- when
 *   - x_dev is the recorded device address (checked on the host: a different address costs nothing),
 *   - the n doubles there equal the copy as 64-bit patterns (one small launch, one 4-byte readback, one
 *     synchronisation of the handle's stream; -0.0 differs from +0.0, a NaN pattern equals itself),
 *   - the record is that of the same handle or of its peer (accbpg_dopt_value_peer), and
 *   - V is unchanged, as accbpg_dopt_create already requires.
 * `end` of an answered evaluation returns the value without waiting for the stream; accbpg_dopt_eval_gap_ms sees it as
 * completed when `begin` returned.  Gradient evaluations (flag 1, 2), the staged entry points (accbpg_dopt_gram,
 * _factor, _eval_gram), the sharded objective and batches neither write nor consult records.  A record is dropped by any
 * error return of begin/end, while a flag-0 evaluation of its handle is in flight, and by accbpg_dopt_value_reuse,
 * accbpg_dopt_factor_in_small_launches and the accbpg_debug_*_variant switches of a handle; the redo of an abandoned one-launch
 * factorisation always evaluates.
 *   accbpg_dopt_value_reuse(h, on): on = 0 switches lookups and the record off for h, anything else on (the default).
 *   accbpg_dopt_value_reuse_stats: compare launches made and evaluations answered on h since its creation.
 *   accbpg_dopt_value_recorded(h, x_dev): 1 when h or its peer holds a valid record at the device address x_dev (the
 *     host-side part of the lookup: no launch, no wait), else 0.  A caller that can ask for the compare inside a larger
 *     enqueue (accbpg_dopt_burg_trial) learns from it whether that is worth asking.
 *   accbpg_dopt_value_peer(h, peer): lookups on h consult peer's record after h's own (read-only: a handle writes its
 *     own record only; peer's counts while none of ITS flag-0 evaluations is in flight).  Both handles must be over
 *     the same V.  peer = NULL unlinks; destroying either handle unlinks too.  For the two handles of one objective
 *     whose value evaluations alternate between two streams. */
int accbpg_dopt_value_reuse(accbpg_dopt* h, int on);
int accbpg_dopt_value_reuse_stats(accbpg_dopt* h, int64_t* compares_host, int64_t* answered_host);
int accbpg_dopt_value_recorded(accbpg_dopt* h, const double* x_dev);
int accbpg_dopt_value_peer(accbpg_dopt* h, accbpg_dopt* peer);

/* The same computation in three stages, for design-point sharding across GPUs
 * (SURVEY.md 8(e).2): each rank forms its local Gram contribution, the caller all-reduces
 * gram_dev (m*m doubles, lower triangle significant) over RCCL, every rank factors it and
 * evaluates the gradient slice of its own columns.
 *   gram  : gram_dev <- lower(V diag(x) V^T) of this handle's columns      (functions.py:46)
 *   factor: in-place Cholesky of gram_dev into the handle; f_host <- -logdet (functions.py:48-51)
 *   grad  : g_dev[i] <- -|| L^-1 v_i ||^2 for this handle's columns          (functions.py:57-58) */
int accbpg_dopt_gram(accbpg_dopt* h, const double* x_dev, double* gram_dev);
int accbpg_dopt_factor(accbpg_dopt* h, const double* gram_dev, double* f_host);
int accbpg_dopt_grad(accbpg_dopt* h, double* g_dev);

/* Message forms for the sharded evaluation (SURVEY.md 8(e).2, section 5 "packed triangle"): only the lower
 * triangle of the local Gram matrix is significant, so the all-reduce carries m(m+1)/2 doubles,
 * packed[r(r+1)/2 + c] = G[r*m + c] for c <= r; accbpg_vec_count_bad leaves the number of entries of x that
 * violate the reference's `x.min() >= 0` (accbpg/functions.py:45; NaN counts) in count_dev[0] as a double, so
 * that it can travel as one more element of the same message and every rank sees every rank's violations. */
int accbpg_tri_pack(const double* G_dev, int64_t m, double* packed_dev, void* stream);
int accbpg_tri_unpack(const double* packed_dev, int64_t m, double* G_dev, void* stream);
int accbpg_vec_count_bad(const double* x_dev, int64_t n, double* count_dev, void* stream);

/* The sharded evaluation as one call, with the collectives inside the library (SURVEY.md 8(b) "dopt_shard_*",
 * 8(e).2): RCCL (librccl.so.1) is opened at run time.  `local` is a handle over this rank's columns V[:, lo:hi],
 * lo and hi from accbpg_dopt_shard_bounds (contiguous slices whose lengths differ by at most one).  Either `comm`
 * is an RCCL communicator of the caller's (an ncclComm_t; used, not owned), or it is null and the communicator
 * is made from the ACCBPG_SHARD_ID_BYTES-byte token that accbpg_shard_unique_id gave rank 0 and rank 0 handed round.
 * accbpg_dopt_shard_func_grad evaluates f(x) = -log det(V diag(x) V^T) (accbpg/functions.py:40-60) at the whole
 * length-n device vector x, which every rank holds: one all-reduce of the packed Gram triangle (+ the x >= 0
 * violation count) and, for flags 1 and 2, one all-gather of the gradient slices; g_dev receives the whole
 * gradient on every rank.  Return codes as accbpg_dopt_func_grad, the same on every rank -- EXCEPT ACCBPG_ERR_HIP: a HIP
 * or RCCL failure on one rank returns on that rank before the collective the other ranks are entering, and they stay in
 * it (RCCL has no timeout of its own); a caller that survives ACCBPG_ERR_HIP must tear the job down.  At world > 1 these
 * entry points have not run on hardware yet (one GPU per box in the builds so far): the message layout and the assembly
 * of unequal slices are covered with two gloo ranks on the CPU and with one rank on a GPU. */
#define ACCBPG_SHARD_ID_BYTES 128
typedef struct accbpg_dopt_shard accbpg_dopt_shard;
int accbpg_dopt_shard_bounds(int64_t n, int world, int rank, int64_t* lo, int64_t* hi);
int accbpg_shard_unique_id(void* id_out);
int accbpg_dopt_shard_create(accbpg_dopt* local, int64_t n, int world, int rank, const void* unique_id,
                             void* comm, accbpg_dopt_shard** out);
int accbpg_dopt_shard_func_grad(accbpg_dopt_shard* s, const double* x_dev, int flag, double* f_host, double* g_dev);
int accbpg_dopt_shard_destroy(accbpg_dopt_shard* s);
/* test hook: gather the gradient through the padded staging buffer (the path of unequal slices), `extra` spare
 * entries per rank */
int accbpg_debug_shard_pad(accbpg_dopt_shard* s, int64_t extra);

/* Linearity of the Gram matrix in x (an extension with no reference counterpart; opt-in from the
 * Python side): out <- a*G1 + b*G2 is the Gram matrix at a*x1 + b*x2 when G1, G2 are those at x1, x2;
 * accbpg_dopt_eval_gram finishes func_grad from a Gram matrix (Cholesky, log det, gradient). */
int accbpg_dopt_gram_lincomb(accbpg_dopt* h, double a, const double* G1_dev, double b,
                             const double* G2_dev, double* out_dev);
int accbpg_dopt_eval_gram(accbpg_dopt* h, const double* gram_dev, int flag, double* f_host, double* g_dev);

/* ---- Batches of same-shaped instances on one GPU (BASELINE config 4; SURVEY.md 8(b) "*_batched", 8(e).1) ----------
 * K independent D-optimal problems of one shape advance in lock-step: every entry point below covers the ACTIVE
 * instances (active_host[i] != 0; NULL = all) with ONE launch per kernel family and ONE readback, and reports a status
 * per instance.  Vectors are K x n arrays, row i = instance i, leading dimension ld.  The arithmetic of an instance is
 * that of accbpg_dopt_func_grad / accbpg_burg_simplex_div_prox / accbpg_ls_terms / accbpg_vec_axpby on the handle
 * accbpg_dopt_batch_instance(b, i) -- bit for bit -- so a batch and a loop over its instances give identical results.
 * The per-instance decisions (stopping, line search) stay with the caller, who re-issues the instances that need
 * another pass.  Shapes outside the fused path (m not a multiple of 256, n not a multiple of 128, unaligned rows) are
 * evaluated instance by instance behind the same interface.  A batch holds at most ACCBPG_BATCH_MAX instances;
 * accbpg_dopt_batch_create returns ACCBPG_ERR_ARG for more (split them over several batches). */
#define ACCBPG_BATCH_MAX 64
typedef struct accbpg_dopt_batch accbpg_dopt_batch;

/* V_dev_host: HOST array of K device pointers (m x n row-major matrices, leading dimension ldv, borrowed). */
int accbpg_dopt_batch_create(const double* const* V_dev_host, int K, int64_t m, int64_t n, int64_t ldv, void* stream,
                             accbpg_dopt_batch** out);
int accbpg_dopt_batch_destroy(accbpg_dopt_batch* b);
int accbpg_dopt_batch_set_stream(accbpg_dopt_batch* b, void* stream);
int accbpg_dopt_batch_size(accbpg_dopt_batch* b);
int accbpg_dopt_batch_is_fused(accbpg_dopt_batch* b);          /* 1: one launch per kernel family covers the batch */
int accbpg_dopt_batch_chunk(accbpg_dopt_batch* b);             /* instances one launch covers: all of them, unless their
                                                                  one-launch factorisations do not fit the chip together */
accbpg_dopt* accbpg_dopt_batch_instance(accbpg_dopt_batch* b, int i);   /* owned by the batch */

/* DOptimalObj.func_grad (accbpg/functions.py:43-59) for the active instances.  f_host[i], status_host[i]
 * (ACCBPG_OK / ACCBPG_ERR_ASSERT: min(x_i) < 0 / ACCBPG_ERR_NOT_PD) are written for those only. */
int accbpg_dopt_batch_func_grad(accbpg_dopt_batch* b, const double* x_dev, int64_t ldx, const int* active_host, int flag,
                                double* f_host, double* g_dev, int64_t ldg, int* status_host);
/* The same split into enqueue / wait (as accbpg_dopt_func_grad_begin / _end): two batches over the same matrices on
 * two streams let the value evaluations F[k] = f(x_i) run beside the gradient evaluations at y_i. */
int accbpg_dopt_batch_func_grad_begin(accbpg_dopt_batch* b, const double* x_dev, int64_t ldx, const int* active_host,
                                      int flag, double* g_dev, int64_t ldg);
int accbpg_dopt_batch_func_grad_end(accbpg_dopt_batch* b, double* f_host, int* status_host);

/* BurgEntropySimplex.div_prox_map(y_i, g_i, L_host[i]) (accbpg/functions.py:264-271, 336-356; y_dev NULL: prox_map).
 * info_host (optional): {bisection steps, Newton steps} per instance. */
int accbpg_dopt_batch_burg_simplex_div_prox(accbpg_dopt_batch* b, const double* y_dev, const double* g_dev, int64_t ld,
                                            const double* L_host, double eps, double* x_out_dev, const int* active_host,
                                            int* status_host, int* info_host);

/* The dual-averaging step of ABDA (accbpg/algorithms.py:483-485) for the active instances, one launch:
 *   gavg_out_i = gavg_i + wgt_host[i] * g_i,   z_out_i = BurgEntropySimplex.prox_map(gavg_out_i / csum_host[i], Lc_host[i])
 * with one rounding per operation -- bit for bit accbpg_vec_axpby(1.0, gavg_i, wgt, g_i), accbpg_vec_div_scalar and
 * accbpg_burg_simplex_div_prox(NULL, ...) in a row (which is what runs, instance by instance, for n > 32768).  Lc_host[i]
 * is L / csum as the caller computed it.  gavg_out_dev must not be gavg_dev (ACCBPG_ERR_ARG).  status_host[i]:
 * ACCBPG_ERR_ASSERT when Lc_host[i] is not positive, and nothing is written for that instance.  info_host (optional):
 * {bisection steps, Newton steps} per instance. */
int accbpg_dopt_batch_burg_simplex_avg_prox(accbpg_dopt_batch* b, const double* gavg_dev, const double* g_dev, int64_t ld,
                                            const double* wgt_host, const double* csum_host, const double* Lc_host,
                                            double eps, double* gavg_out_dev, double* z_out_dev, const int* active_host,
                                            int* status_host, int* info_host);

/* out_host[3i..3i+2] = { <g_i, x_i - y_i>, D_h(x_i, y_i), D_h(z_i, z1_i) } (accbpg/algorithms.py:153-154, 377-378, 387). */
int accbpg_dopt_batch_ls_terms(accbpg_dopt_batch* b, const double* g_dev, const double* x_dev, const double* y_dev,
                               const double* z_dev, const double* z1_dev, int64_t ld, const int* active_host,
                               double* out_host, int* status_host);

/* out_i = a_host[i] * x_i + b_host[i] * z_i (accbpg/algorithms.py:147,150). */
int accbpg_dopt_batch_axpby(accbpg_dopt_batch* b, const double* a_host, const double* x_dev, const double* b_host,
                            const double* z_dev, int64_t ld, const int* active_host, double* out_dev);

/* ---- Burg entropy on the simplex: replaces BurgEntropy / BurgEntropySimplex ------------
 * (accbpg/functions.py:238-271, 326-356).  `ws_dev` is caller-provided scratch of at least
 * accbpg_vec_workspace_doubles(n) doubles. */
int64_t accbpg_vec_workspace_doubles(int64_t n);

/* x_out <- argmin_{x in simplex} <g,x> + L*D_h(x,y)  = prox_map(g + L/y, L)
 * (functions.py:264-271 then 336-356): same start c = -min(gg)+1, same bisection, same
 * Newton recurrence, stall test and |phi| <= eps stopping rule; result not renormalised.
 * y_dev == NULL selects plain prox_map(g, L) (functions.py:336).  info_host (optional,
 * 2 ints) receives {bisection steps, Newton steps}.  ACCBPG_ERR_ASSERT if L <= 0 or
 * min(y) <= 0. */
int accbpg_burg_simplex_div_prox(const double* y_dev, const double* g_dev, double L, double eps,
                                 int64_t n, double* x_out_dev, double* ws_dev,
                                 int* info_host, void* stream);

/* out_host[0] <- D_h(x,y) = sum_i (x_i/y_i - log(x_i/y_i) - 1)   (functions.py:250-253).
 * ACCBPG_ERR_ASSERT if min(x) <= 0 or min(y) <= 0. */
int accbpg_burg_divergence(const double* x_dev, const double* y_dev, int64_t n,
                           double* out_host, double* ws_dev, void* stream);

/* Line-search terms in one readback: out_host = { <g, x - y>, D_h(x,y), D_h(z,z1) }
 * (algorithms.py:53, 153-154, 377-378, 387).  Any of (g), (z,z1) may be NULL to skip. */
int accbpg_ls_terms(const double* g_dev, const double* x_dev, const double* y_dev,
                    const double* z_dev, const double* z1_dev, int64_t n,
                    double* out_host, double* ws_dev, void* stream);

/* out <- a*x + b*z elementwise, rounded as NumPy rounds (1-theta)*x + theta*z
 * (algorithms.py:147,150,369,374): two products, one sum, no fused multiply-add. */
int accbpg_vec_axpby(double a, const double* x_dev, double b, const double* z_dev, int64_t n,
                     double* out_dev, void* stream);

/* One line-search trial of ABPG_gain with BurgEntropySimplex (accbpg/algorithms.py:369-387) enqueued whole on the
 * handle's stream and waited for ONCE.  None of the intermediate results decides what is launched next -- the launches
 * depend on theta and L, which the host knows before the trial, and on device vectors -- so the call enqueues, in this
 * order and with no host wait in between,
 *   a. if want_fk: the bit-for-bit compare of x_prev against the value record of h or its peer (the lookup of
 *      accbpg_dopt_func_grad_begin that answers F[k] = f(x_prev), :347) -- only when its host-side part already holds
 *      (record valid, same device address); otherwise F[k] is "not answered" at no cost,
 *   b. y = (1-theta) x_prev + theta z_prev                                    (accbpg_vec_axpby, :369)
 *   c. f(y), g = grad f(y)                                                    (accbpg_dopt_func_grad flag 2, :371)
 *   d. z = div_prox_map(z_prev, g, L)                                         (accbpg_burg_simplex_div_prox, :373)
 *   e. x = (1-theta) x_prev + theta z                                         (accbpg_vec_axpby, :374)
 *   f. <g, x-y>, D(x,y), D(z,z_prev)                                          (accbpg_ls_terms, :377-378, :387)
 *   g. f(x)                                                                   (accbpg_dopt_func_grad flag 0, :387)
 *   h. one copy of the stages' status words to pinned memory, one synchronisation of the stream.
 * The launches are those of the entry points named, in the forms they pick for this m and n: every output is theirs
 * bit for bit.  L is the prox constant theta^(gamma-1) * G * L of :373, eps the prox tolerance.  y_dev, g_dev, z_dev,
 * x_dev are n doubles each, distinct from each other and from the inputs; ws_dev as for the vector entry points.  No
 * accbpg_dopt_func_grad_begin may be waiting for its _end on h.
 * Returns ACCBPG_OK for a clean trial: out_host is filled, the value record of h is f(x) at x_dev (as after
 * accbpg_dopt_func_grad_end), and an enqueued compare counts in accbpg_dopt_value_reuse_stats (as answered when
 * out_host->fk_answered; then out_host->fk is F[k]).  Returns ACCBPG_TRIAL_REPLAY for anything else that is not a HIP
 * failure -- L <= 0, an entry of y or x negative, a Gram matrix not positive definite, a non-positive entry of z_prev
 * or of a divergence's arguments, a one-launch factorisation or a multi-workgroup prox that abandoned a wait (the
 * handle / the process then stays with the fallback form, as the stepwise entry points decide it): nothing is
 * committed, out_host and the four vectors are unspecified, h keeps no value record and its counters do not move.  The
 * caller then runs the same trial through the stepwise entry points, which raise what there is to raise.  Because the
 * record is gone (the value evaluation's reset launch has overwritten its copy of x), an F[k] that rode in a replayed
 * trial is evaluated in full by the stepwise lookup: the same bits, one answered evaluation fewer than the stepwise
 * calls alone would have counted.  Nothing is read back before the wait, so the stages behind a flagged one still run,
 * on whatever that stage left (a NaN ends the prox's scalar loops at once, each of them is bounded by 4096 steps, and
 * the multi-workgroup wait by its budget): a replayed trial always ends, but may cost more than the stepwise calls,
 * which stop at the first error.
 * Where h's own record and its peer's sit at the same address, only h's is compared (accbpg_dopt_func_grad_begin goes on
 * to the peer's when the contents differ): F[k] is then "not answered" and evaluated.  The event behind
 * accbpg_dopt_eval_gap_ms is recorded behind the status copy, as by accbpg_dopt_func_grad_begin. */
#define ACCBPG_TRIAL_REPLAY 5
typedef struct accbpg_trial_out {
    double fy;              /* f(y) */
    double lin, dxy, dzz;   /* <g, x-y>, D(x,y), D(z,z_prev) */
    double fx;              /* f(x) */
    double fk;              /* F[k] = f(x_prev) when fk_answered */
    int32_t prox_info[2];   /* {bisection steps, Newton steps} */
    int32_t fk_answered;
    int32_t reserved;
} accbpg_trial_out;
int accbpg_dopt_burg_trial(accbpg_dopt* h, const double* x_prev_dev, const double* z_prev_dev, double theta, double L,
                           double eps, int want_fk, double* y_dev, double* g_dev, double* z_dev, double* x_dev,
                           double* ws_dev, accbpg_trial_out* out_host);

/* out_host[0] <- <g, x - y>   (algorithms.py:53,168,387,406) */
int accbpg_vec_dot_diff(const double* g_dev, const double* x_dev, const double* y_dev, int64_t n,
                        double* out_host, double* ws_dev, void* stream);

/* out_host = { min(x), sum(x) } -- precondition checks and diagnostics. */
int accbpg_vec_min_sum(const double* x_dev, int64_t n, double* out_host, double* ws_dev, void* stream);

/* ---- callers either side of the path ------------------------------------- */

/* out <- x / d, NumPy true division (gavg/csum of ABDA, accbpg/algorithms.py:485) */
int accbpg_vec_div_scalar(const double* x_dev, double d, int64_t n, double* out_dev, void* stream);

/* out[i] <- fill, out[idx] <- value: the simplex vertex returned by lmo_simplex
 * (accbpg/functions_lmo.py:152-157: 1e-15 everywhere, radius at the first argmin of g). */
int accbpg_vec_vertex(int64_t idx, double value, double fill, int64_t n, double* out_dev, void* stream);

/* idx_host = {first argmin, first argmax} of x, val_host (optional) = {min, max}
 * (np.argmin / np.argmax, accbpg/applications.py:80-81; np.where(g == g.min())[0][0],
 * functions_lmo.py:155-156). */
int accbpg_vec_argminmax(const double* x_dev, int64_t n, int64_t* idx_host, double* val_host,
                         double* ws_dev, void* stream);

/* u <- V^T q (length n) for a length-m q: np.dot(q, V) of D_opt_KYinit (accbpg/applications.py:79). */
int accbpg_dopt_vt_times(accbpg_dopt* h, const double* q_dev, double* u_dev);

/* out <- V[:, j] (length m): the column reads of D_opt_KYinit (accbpg/applications.py:84). */
int accbpg_dopt_get_column(accbpg_dopt* h, int64_t j, double* out_dev);

/* Kumar-Yildirim start (accbpg/applications.py:59-95): all m steps on h's stream, one synchronisation at the end.
 * B_dev: m*m doubles, row i = the random direction b of step i (drawn by the caller, applications.py:74).
 * picked_host: 2m indices, [2i] = kmax, [2i+1] = kmin of step i (:80-83).
 * Q_dev: optional m*m doubles, column j contiguous at Q_dev + j*m, receives the orthonormal directions (:89);
 *        NULL = the call allocates and frees its own.
 * Per step: the Gram-Schmidt coefficients from the un-deflated vector (:77, :87), each dot summed in one fixed order;
 * the deflation in coefficient order (:78, :88); q^T V as accbpg_dopt_vt_times computes it (:79); first-index argmax /
 * argmin as accbpg_vec_argminmax (:80-81), clamped to [0, n); v = V[:,kmin] - V[:,kmax] (:84); Q[:,i] = q / ||q|| (:89).
 * Leaves the handle's solver state as it was (it uses the workspace of accbpg_dopt_vt_times only). */
int accbpg_dopt_kyinit(accbpg_dopt* h, const double* B_dev, int64_t* picked_host, double* Q_dev);

/* ---- Frank-Wolfe / Wolfe-Atwood state: replaces the bodies of D_opt_FW and --------------
 * D_opt_FW_away (accbpg/D_opt_alg.py:9-88, 91-185).  State (x, inverse H = (V X V^T)^-1,
 * w_i = v_i^T H v_i) lives in the handle. */

typedef struct accbpg_fw_probe {
    int64_t i;         /* argmax_i w_i                         (D_opt_alg.py:59,145)            */
    int64_t j;         /* away index                           (D_opt_alg.py:60-61 / 146-147)   */
    double  w_i;       /* w[i]                                                                */
    double  w_j;       /* w[j] (FW: min of w over x > 0)                                       */
    double  x_j;       /* x[j]                                                                */
    double  logdet_H;  /* log det of the maintained inverse H  (D_opt_alg.py:136)              */
    double  q_prev;    /* v_p^T H v_p of the LAST accbpg_fw_update's pivot column p in the inverse as it stood before
                          that update (0 before the first): det(H+) = det(H) (1 + hcoef q) / hdiv^m             */
} accbpg_fw_probe;

/* x <- x0; H <- (V diag(x0) V^T)^-1; w <- diag(V^T H V)   (D_opt_alg.py:39-45 / 123-129).
 * logdet_gram_host <- log det(V diag(x0) V^T). */
int accbpg_fw_init(accbpg_dopt* h, const double* x0_dev, double* logdet_gram_host);

/* Reduction pass over w, x: fills *probe_host.  away = 0: j = argmin of w over {x > 0}
 * (D_opt_alg.py:60-61); away = 1: j = argmin of (w - w_i) * [x > 1e-8], first index on ties
 * (D_opt_alg.py:146-147).  refresh_logdet != 0 also refactors H for logdet_H (D_opt_alg.py:136). */
int accbpg_fw_probe_step(accbpg_dopt* h, int away, int refresh_logdet, accbpg_fw_probe* probe_host);

/* refresh_logdet = 2 is the pipelined form of 1: log det(H) is a logged value that no decision of the iteration reads
 * (D_opt_alg.py:136 -> F[k] only), so a copy of the current H is factored on a side stream (by an auxiliary handle with
 * buffers of its own) while the caller goes on to probe, decide and update.  `depth` such factorisations may be in
 * flight (accbpg_fw_logdet_ring; default 1): probe_host->logdet_H holds the value that belongs to the call made this way
 * `depth` calls earlier (NaN while there is none), accbpg_fw_logdet_flush collects the oldest one still in flight (NaN
 * when none is), accbpg_fw_logdet_pending counts them.  Same kernels on the same matrices as form 1.
 * small_launches: how the side factorisations run, as accbpg_dopt_factor_in_small_launches (0 one launch, 1 a launch
 * per block column, 2 by size).  A caller that refreshes only every R-th call and advances log det(H) in between by
 * the matrix determinant lemma uses q_prev (D_opt_FW_away(..., logdet_refresh=R) of the Python package). */
int accbpg_fw_logdet_ring(accbpg_dopt* h, int depth, int small_launches);
int accbpg_fw_logdet_pending(accbpg_dopt* h);
int accbpg_fw_logdet_flush(accbpg_dopt* h, double* logdet_host);

/* One rank-one update with pivot column p (i for a Frank-Wolfe step, j for an away step):
 *   x <- x*xscale; x[p] += xadd; Hv = H V[:,p];
 *   H <- (H + hcoef * Hv Hv^T) * hscale_inv ...  written exactly as
 *   H <- (H + hcoef*outer(Hv,Hv)) / hdiv and w <- (w + hcoef*(Hv^T V)^2) / hdiv
 * with the scalars computed by the caller as the reference writes them
 * (D_opt_alg.py:75-82, 163-170, 172-179; hcoef carries its sign). */
int accbpg_fw_update(accbpg_dopt* h, int64_t p, double xscale, double xadd, double hcoef, double hdiv);

/* Copy state out (device to device): x (n), w (n), H (m*m, row-major).  NULL skips. */
int accbpg_fw_get_state(accbpg_dopt* h, double* x_dev, double* w_dev, double* H_dev);

/* Frank-Wolfe with a Bregman step (FW_alg_div_step / FW_alg_descent_step, accbpg/algorithms_fw.py:6-75, :210-247) on
 * the maintained state, for the D-optimal objective, the Burg kernel and the simplex LMO (functions_lmo.py:137-160).
 * The gradient is -w; the vertex is s_j = fill, s_i = value at i = first argmax of w; x+ = x + a (s - x) changes the
 * Gram matrix by the factor (1 - a) and a rank-one term in v_i (plus a dense term of relative size <= fill * n that
 * the caller accounts for to first order with sum_w).
 *   _probe_step: one pass over w and x fills the record, then the direction of the step is computed with i read from
 *       device memory: Hv = H V[:,i], u = V^T Hv (the kernels of accbpg_fw_update) and sum u^2.  Hv and u stay in the
 *       handle for _apply; they do not depend on the step length, so a line search needs no launch per trial.  ONE
 *       synchronisation.  The argmax follows np.argmin of -w (first index on ties, a NaN is picked).  The sums and the
 *       minimum run over the fixed tree of the length-n reductions (256 threads, four entries per thread, at most 512
 *       blocks, blocks in block order): repeated calls are bit-identical.
 *   _apply: x_j <- x_j + a (s_j - x_j), bit for bit accbpg_vec_axpby(1, s, -1, x) followed by
 *       accbpg_vec_axpby(1, x, a, d); H <- (H + hcoef Hv Hv^T) / hdiv; w <- (w + hcoef u^2) / hdiv, the update kernels
 *       of accbpg_fw_update on their grids.  p must be the i of the last _probe_step and the state must not have moved
 *       since (ACCBPG_ERR_ARG otherwise, nothing is launched).  Does not synchronise.
 * Both mix freely with accbpg_fw_init / accbpg_fw_get_state / accbpg_fw_probe_step / accbpg_fw_update. */
typedef struct accbpg_fw_div_probe {
    int64_t i;                 /* first-index argmax of w (= first argmin of the gradient -w), NaN as np.argmin */
    double  w_i, x_i;
    double  sum_w, sum_w2;     /* sum w_j, sum w_j^2 */
    double  slope;             /* sum_j (-w_j) * (s_j - x_j), s_j = fill except s_i = value; each op rounded once */
    double  div;               /* sum_j (s_j/x_j - log(s_j/x_j) - 1) */
    double  min_x;             /* NaN-keeping minimum of x */
    double  sum_u2;            /* sum_j u_j^2, u = V^T (H V[:,i]) */
} accbpg_fw_div_probe;
int accbpg_fw_div_probe_step(accbpg_dopt* h, double fill, double value, accbpg_fw_div_probe* out_host);
int accbpg_fw_div_apply(accbpg_dopt* h, int64_t p, double a, double fill, double value, double hcoef, double hdiv);

/* The refresh_logdet = 2 part of accbpg_fw_probe_step as a call of its own: copies the current H into the ring slot
 * that comes round and starts its side factorisation; *collected_host <- the value that slot held (the snapshot taken
 * `depth` such calls earlier), NaN while there is none.  accbpg_fw_probe_step(h, away, 2, ...) is this call followed by
 * the probe. */
int accbpg_fw_logdet_snapshot(accbpg_dopt* h, double* collected_host);

/* Several iterations per host round trip: the scalar decisions of an iteration (D_opt_alg.py:63-82 for away = 0,
 * :150-179 for away = 1) are taken ON THE DEVICE, by thread 0 of the probe's final stage, in plain float64 + - * / and
 * comparisons written operation for operation as the reference writes them (no fused multiply-add, NaN falls through
 * the comparisons as it does there):
 *   eps_pos = w_i / m - 1, eps_neg = 1 - w_j / m; stop when eps_pos <= eps && eps_neg <= eps           (:72, :159)
 *   away = 0, or eps_pos >= eps_neg: t = (w_i / m - 1) / (w_i - 1), update (i, 1 - t, t, -coef, 1 - t) with
 *       coef = t / (1 + t * (w_i - 1)) for away = 0 (:75-82), coef = t / (1 - t + t * w_i) for away = 1 (:162-170)
 *   otherwise: t = min((1 - w_j / m) / (w_j - 1), x_j / (1 - x_j)), coef = t / (1 + t - t * w_j), update
 *       (j, 1 + t, -t, coef, 1 + t)                                                                    (:171-179)
 * One call enqueues nsteps iterations (1 <= nsteps <= 1024), each the kernels of accbpg_fw_probe_step(h, away, 0, ...)
 * followed by those of accbpg_fw_update with the scalars read from device memory -- the same bodies on the same grids,
 * so x, w and H are bit for bit those of the step-by-step calls -- synchronises ONCE and copies the records out.  After
 * a stop (status 1 or 2) the remaining kernels of the call return at once: x, w, H and q_prev stay as the stop found
 * them and the later records read status 3.  *nrun_host <- the number of records with status != 3.  A pivot outside
 * [0, n) (status 2) applies no update and makes the call return ACCBPG_ERR_ARG with accbpg_fw_update's message; the
 * records are filled in all the same.  May be mixed freely with accbpg_fw_probe_step / accbpg_fw_update. */
#define ACCBPG_FW_RUN_MAX 1024   /* most iterations of one accbpg_fw_run call */
typedef struct accbpg_fw_step {
    int64_t i, j;  double w_i, w_j, x_j, q_prev;       /* the probe record, as accbpg_fw_probe */
    int64_t p;     double xscale, xadd, hcoef, hdiv;   /* the update the device applied        */
    int32_t kind;   /* 0 Frank-Wolfe step, 1 away step, -1 none */
    int32_t status; /* 0 update applied; 1 stop test held; 2 pivot outside [0,n); 3 not run (after a stop) */
} accbpg_fw_step;
int accbpg_fw_run(accbpg_dopt* h, int away, double eps, int nsteps, accbpg_fw_step* steps_host, int* nrun_host);

/* Several iterations of the Bregman-step solvers per host round trip.  The device PREDICTS the decisions of an
 * iteration -- thread 0 of the last stage of the probe, after sum u^2, with the text of csrc/fw_div_decide.hpp: the
 * slope band, div == 0 -> 1e-6, L / ls_ratio and the trial loop a -> (hcoef, hdiv, ld1, q1, f1) ->
 * f1 <= fx + a*slope + a^gamma * L * div, L * ls_ratio, the stop tests -- and the caller CHECKS: the device's log and
 * pow need not round as the host's do, so the caller replays every record with its own arithmetic and, where a decision
 * differs, restores an earlier state (accbpg_fw_set_state) and redoes the steps with accbpg_fw_div_probe_step /
 * accbpg_fw_div_apply.  prm carries the caller's exact ld, q and F[k0 - 1] at the start of the call; inside the call
 * the device advances its own.
 *   mode 0 (line search) and 1 (fixed L), FW_alg_div_step: iteration k = the kernels of accbpg_fw_div_probe_step,
 *       the decision, the kernels of accbpg_fw_div_apply.  status 0: step applied; 1: step applied and the stop test
 *       k > 0 && |F[k] - F[k-1]| < epsilon held (the solver applies, then stops); 2: handed back, NOTHING applied --
 *       `reason` says why (1 the trial budget ACCBPG_FW_DIV_TRIALS_MAX ran out, 2 L became infinite, 3 slope > 0,
 *       4 min_x is not > 0, 5 pivot outside [0, n), 6 a is not < 1: the capped step or a NaN, 7 the host's arithmetic
 *       raises there); 3: not run.
 *   mode 2 (classical step a = 2 / (k + 2)), FW_alg_descent_step: needs the probe of accbpg_fw_div_probe_step (or of an
 *       earlier call in this mode) pending, as accbpg_fw_div_apply does (ACCBPG_ERR_ARG otherwise); iteration k >= 1 =
 *       apply step k, probe, stop test |F[k] - F[k-1]| < epsilon || sqrt(sum_w2) < epsilon.  The record holds that
 *       probe, the step that led to it, f1 = F[k].  status 0: applied and probed; 1: the same and the stop test held (the
 *       state stays as the probe found it, its direction pending); 2: the step could not be decided, nothing applied.
 * One C loop of plain launches -- the bodies, grids, block caps and summation orders of the step-by-step entries, so
 * the probe fields, x, w and H are bit for bit theirs -- ONE synchronisation, and the records copied out once.  After
 * a stop or a hand-back every later kernel of the call returns before it touches x, w, H, u, the stage-1 records or the
 * pending pivot; later records read status 3.  *nrun_host <- the number of records with status != 3.  A record whose
 * pivot lies outside [0, n) makes the call return ACCBPG_ERR_ARG with accbpg_fw_div_probe_step's message, the records
 * filled in all the same.  1 <= nsteps <= ACCBPG_FW_RUN_MAX.  Mixes freely with accbpg_fw_div_probe_step /
 * accbpg_fw_div_apply / accbpg_fw_init. */
#define ACCBPG_FW_DIV_TRIALS_MAX 64
typedef struct accbpg_fw_div_params {
    int32_t mode;              /* 0 line search, 1 fixed L, 2 classical step */
    int32_t reserved;
    int64_t k0;                /* iteration number of the first step of the call */
    double  L, gamma, ls_ratio, epsilon;
    double  ld, q, F_prev;     /* the caller's book at the start of the call, F[k0 - 1] */
} accbpg_fw_div_params;
typedef struct accbpg_fw_div_step {
    accbpg_fw_div_probe probe;
    double  L;                 /* accepted (modes 0, 1) */
    double  a, hcoef, hdiv;    /* the step */
    double  ld1, q1, f1;       /* the device's own book behind the step; f1: trial value (modes 0, 1), F[k] (mode 2) */
    int32_t trials, status, reason, reserved;
} accbpg_fw_div_step;
int accbpg_fw_div_run(accbpg_dopt* h, double fill, double value, const accbpg_fw_div_params* prm, int nsteps,
                      accbpg_fw_div_step* steps_host, int* nrun_host);

/* The inverse of accbpg_fw_get_state: x (n), w (n), H (m*m, row-major) from device buffers of the caller, device to
 * device on the handle's stream (no synchronisation).  Leaves the stage-1 records and the pending pivot of
 * accbpg_fw_div_probe_step cleared, as accbpg_fw_init leaves them: accbpg_fw_div_apply without a new probe is
 * ACCBPG_ERR_ARG.  A null argument, or a handle without Frank-Wolfe state, is ACCBPG_ERR_ARG. */
int accbpg_fw_set_state(accbpg_dopt* h, const double* x_dev, const double* w_dev, const double* H_dev);

/* Lock-step Frank-Wolfe steps for the instances of a batch (accbpg_dopt_batch_create): ONE launch per step kernel
 * covers the active instances (active_host[i] != 0; NULL = all) and ONE synchronisation returns all probe records.
 * The state lives in the instance handles: after a batched step, x, w and H of instance i are bit for bit those of
 * accbpg_fw_update on accbpg_dopt_batch_instance(b, i), accbpg_fw_get_state on that handle returns them, and
 * single-handle and batched calls may be mixed.  Works for every shape a batch can hold.  All host arrays have K
 * entries, entry i = instance i; entries of inactive instances are neither read nor written.
 *   _fw_init:   accbpg_fw_init per active instance with x0 = row i of x0_dev (leading dimension ldx).  status_host[i]
 *               <- ACCBPG_OK or ACCBPG_ERR_NOT_PD (that instance has no state then; the others are initialised);
 *               logdet_gram_host (may be NULL) as accbpg_fw_init.
 *   _fw_probe:  the records of accbpg_fw_probe_step(h_i, away, 0, ...): logdet_H is NaN (log det(H) beside the steps:
 *               accbpg_fw_logdet_snapshot on the instance handles).
 *   _fw_update: accbpg_fw_update(h_i, p_host[i], xscale_host[i], xadd_host[i], hcoef_host[i], hdiv_host[i]).  A pivot
 *               outside [0, n) on an active instance returns ACCBPG_ERR_ARG before anything is launched. */
int accbpg_dopt_batch_fw_init(accbpg_dopt_batch* b, const double* x0_dev, int64_t ldx, const int* active_host,
                              double* logdet_gram_host, int* status_host);
int accbpg_dopt_batch_fw_probe(accbpg_dopt_batch* b, int away, const int* active_host, accbpg_fw_probe* probes_host);
int accbpg_dopt_batch_fw_update(accbpg_dopt_batch* b, const int* active_host, const int64_t* p_host,
                                const double* xscale_host, const double* xadd_host, const double* hcoef_host,
                                const double* hdiv_host);

/* accbpg_fw_div_probe_step / accbpg_fw_div_apply for the active instances of a batch in lock-step, by the contract of
 * accbpg_dopt_batch_fw_probe / _fw_update: ONE launch per step kernel covers the active instances (active_host[i] != 0;
 * NULL = all), all host arrays have K entries, entry i = instance i, and entries of inactive instances are neither
 * read nor written.  fill and value are shared by the instances.  Grids, row split and the fixed summation tree of
 * every instance are the single handle's, so the records and x, w, H of instance i are bit for bit those of the two
 * single-handle calls on accbpg_dopt_batch_instance(b, i).
 *   _fw_div_probe: the records of accbpg_fw_div_probe_step(h_i, fill, value, ...) behind ONE synchronisation.  An
 *       instance without stage-1 records waiting gets a fresh stage 1 in a launch over those instances alone.  Each
 *       instance's Hv and u stay in its own handle, and its bookkeeping is what the single-handle probe leaves.  An
 *       active instance without Frank-Wolfe state returns ACCBPG_ERR_ARG before anything is launched.  A pivot outside
 *       [0, n) on some instance returns ACCBPG_ERR_ARG with the first such instance named in the message; all records
 *       are filled in all the same and that instance accepts no _apply.
 *   _fw_div_apply: accbpg_fw_div_apply(h_i, p_host[i], a_host[i], fill, value, hcoef_host[i], hdiv_host[i]).  If on any
 *       active instance p_host[i] is not the index of that instance's last div probe, or its state has moved since,
 *       the call returns ACCBPG_ERR_ARG (the instance is named) before anything is launched: no instance moves.  Does
 *       not synchronise; leaves the stage-1 records of the next probe on every updated instance.
 * The instances' workspaces are their handles' own, so batched and single-handle div calls may be mixed on one state
 * (a batched probe followed by accbpg_fw_div_apply on the instance handle, or the converse), and both mix freely with
 * accbpg_fw_* on the handles and accbpg_dopt_batch_fw_init / _fw_probe / _fw_update / _fw_run: any of those that moves
 * the state between a div probe and its apply makes the apply refuse.  The table of workspace addresses is built by
 * the first of the two calls and freed by accbpg_dopt_batch_destroy. */
int accbpg_dopt_batch_fw_div_probe(accbpg_dopt_batch* b, double fill, double value, const int* active_host,
                                   accbpg_fw_div_probe* out_host);
int accbpg_dopt_batch_fw_div_apply(accbpg_dopt_batch* b, const int* active_host, const int64_t* p_host,
                                   const double* a_host, double fill, double value, const double* hcoef_host,
                                   const double* hdiv_host);

/* accbpg_fw_run for the active instances of a batch in lock-step: ONE launch per step kernel covers the active
 * instances (active_host[i] != 0; NULL = all; the set is fixed for the call), the decisions of every iteration are
 * taken on the device per instance, as accbpg_fw_run takes them and with eps_host[i], and ONE synchronisation returns
 * all records.  eps_host and nrun_host have K entries, steps_host K * nsteps: row i (nsteps records) belongs to
 * instance i; entries of inactive instances are neither read nor written.  1 <= nsteps <= ACCBPG_FW_RUN_MAX.
 * An instance that stops in mid-call (status 1 or 2) idles through the rest of the call while the others go on: its
 * x, w, H, stage-1 records and q_prev stay as the stop found them and its later records read status 3, as after
 * accbpg_fw_run.  Grids, row split and summation order of every instance are the single handle's, so x, w, H and the
 * records of instance i are bit for bit those of accbpg_fw_run(accbpg_dopt_batch_instance(b, i), away, eps_host[i],
 * nsteps, ...), and what the call leaves on the handle is what that call leaves: it may be mixed freely with
 * accbpg_fw_run, accbpg_fw_probe_step / accbpg_fw_update on the instance handles and accbpg_dopt_batch_fw_probe /
 * _fw_update.  An active instance without Frank-Wolfe state returns ACCBPG_ERR_ARG before anything is launched.  A
 * pivot outside [0, n) (status 2) on any instance makes the call return ACCBPG_ERR_ARG with the (first such) instance
 * named in the message; all records are filled in all the same.  Scratch is allocated by the first call and freed by
 * accbpg_dopt_batch_destroy. */
int accbpg_dopt_batch_fw_run(accbpg_dopt_batch* b, int away, const double* eps_host, int nsteps, const int* active_host,
                             accbpg_fw_step* steps_host, int* nrun_host);

/* accbpg_fw_div_run for the active instances of a batch in lock-step: ONE launch per step kernel covers the active
 * instances (active_host[i] != 0; NULL = all; the set is fixed for the call), every instance's decisions are predicted
 * on the device from its own slot, and ONE synchronisation returns all records.  One C loop of plain launches on the
 * batch's stream.  prm_host and nrun_host have K entries, steps_host K * ACCBPG_FW_RUN_MAX: row i (the first nsteps of
 * its ACCBPG_FW_RUN_MAX records) belongs to instance i; entries and rows of inactive instances are neither read nor
 * written.  prm_host[i] carries instance i's own k0, L, gamma, ls_ratio, epsilon, ld, q and F_prev (instances drift
 * apart after a roll-back or a hand-back; the decisions read k only in k > 0 and in 2 / (k + 2)); fill and value are
 * shared.  mode must be the same on every active instance, and in mode 2 every active instance needs its div probe
 * pending and k0 >= 1, as accbpg_fw_div_run does; so must every active instance have Frank-Wolfe state, and
 * 1 <= nsteps <= ACCBPG_FW_RUN_MAX: ACCBPG_ERR_ARG otherwise, before anything is launched -- no instance moves.
 * An instance that stops or is handed back in mid-call idles through the rest of the call while the others go on: its
 * workgroups return before they touch x, w, H, u, the stage-1 records or the pending pivot, and its later records read
 * status 3.  Grids, the 512-block cap, the row split and the fixed summation tree of every instance are the single
 * handle's, so x, w, H and the records of instance i are bit for bit those of accbpg_fw_div_run(
 * accbpg_dopt_batch_instance(b, i), fill, value, prm_host + i, nsteps, ...), and what the call leaves on the handle
 * (stage-1 records, pending pivot, pinned probe record) is what that call leaves: it mixes freely with
 * accbpg_fw_div_run, accbpg_fw_div_probe_step / accbpg_fw_div_apply on the instance handles and the other
 * accbpg_dopt_batch_fw_* calls.  A record whose pivot lies outside [0, n) on any instance makes the call return
 * ACCBPG_ERR_ARG with the (first such) instance named in the message; all records are filled in all the same and the
 * other instances' records are valid.  Scratch is allocated by the first call and freed by accbpg_dopt_batch_destroy. */
int accbpg_dopt_batch_fw_div_run(accbpg_dopt_batch* b, double fill, double value, const accbpg_fw_div_params* prm_host,
                                 int nsteps, const int* active_host, accbpg_fw_div_step* steps_host, int* nrun_host);

/* The host's replay of one instance's records of accbpg_fw_div_run / accbpg_dopt_batch_fw_div_run
 * (csrc/fw_div_replay.hpp): a pure host function -- no stream, no device call, callable with no GPU present.  From the
 * caller's book (prm: mode, k0, L, gamma, ls_ratio, epsilon, ld, q, F_prev; n, m, fill, value) it walks the records with
 * the host's libm: per record it copies the book, takes the host's decision on the record's probe, compares it with the
 * record bit for bit (NaN equal to NaN) -- modes 0 and 1: (a, hcoef, hdiv, L, status); mode 2: (a, hcoef, hdiv), then
 * the stop test -- and commits the book only if they agree.  It stops at the first record that is not an agreed step:
 *   *verdict_out: 0 end of records; 1 agreed stop (that record is counted in *agreed_out); 2 the device handed the
 *   iteration back; 3 the host's decision is itself a hand-back (the cap, an arithmetic error); 4 disagreement;
 *   5 pivot outside [0, n).
 * It decides nothing about that record: *book_out is the book BEFORE record *agreed_out (k0 advanced by *agreed_out),
 * for the caller to decide it.  F_out[j] <- F[k0 + j] and L_or_alpha_out[j] <- the accepted L (modes 0, 1) or the step
 * length (mode 2) of the agreed records.
 * steps: modes 0 and 1, the nrun records of the call.  Mode 2: nrun + 1 entries -- steps[0].probe is the probe that was
 * pending when the call started (nothing else of steps[0] is read: the step of a record is decided from the probe of the
 * record before it), steps[1 .. nrun] are the records.  0 <= nrun <= ACCBPG_FW_RUN_MAX. */
int accbpg_fw_div_replay(const accbpg_fw_div_params* prm, int64_t n, int64_t m, double fill, double value,
                         const accbpg_fw_div_step* steps, int nrun, double* F_out, double* L_or_alpha_out,
                         accbpg_fw_div_params* book_out, int* agreed_out, int* verdict_out);

/* accbpg_dopt_kyinit for all K instances of a batch in lock-step on the batch's stream: every launch of a step covers
 * the K instances (8 launches per step, 4 at step 0, whatever K is), all m steps are enqueued, one copy returns the
 * indices and the host waits once.
 * B_dev: K*m*m doubles, instance i's directions at B_dev + i*m*m, row r = the direction of step r.
 * picked_host: K*2m indices, instance i at picked_host + 2m*i, [2s] = kmax, [2s+1] = kmin of step s.
 * Q_dev: optional K*m*m doubles, instance i's block at Q_dev + i*m*m, row j of the block = Q[:, j]; NULL = the call's own.
 * Grids, row split and summation order of every instance are the single handle's: picked and Q of instance i are bit for
 * bit those of accbpg_dopt_kyinit(accbpg_dopt_batch_instance(b, i), B_dev + i*m*m, ...).
 * The call owns its scratch, one device allocation freed before it returns: per instance
 * [m*m for Q unless Q_dev is given] + n + 3m doubles + 128 arg-extremum records (32 bytes each) + 2m indices, and one
 * table entry (88 bytes).  Of the instances' handles it writes the workspace of accbpg_dopt_vt_times only: Gram /
 * Cholesky state, Frank-Wolfe state and value records stay as they were.  Works with or without the fused Gram path
 * (accbpg_dopt_batch_is_fused).  NULL b, B_dev or picked_host: ACCBPG_ERR_ARG. */
int accbpg_dopt_batch_kyinit(accbpg_dopt_batch* b, const double* B_dev, int64_t* picked_host, double* Q_dev);

/* ---- Poisson linear inverse problem with Burg L1 / L2 kernels -------- */

typedef struct accbpg_poisson accbpg_poisson;

/* f(x) = D_KL(b, Ax): replaces PoissonRegression.__init__ (accbpg/functions.py:89-94).  A is a row-major
 * m x n device matrix with leading dimension lda, b a length-m device vector; both stay owned by the caller
 * and must outlive the handle. */
int accbpg_poisson_create(const double* A_dev, int64_t m, int64_t n, int64_t lda, const double* b_dev,
                          void* stream, accbpg_poisson** out);
int accbpg_poisson_destroy(accbpg_poisson* h);
int accbpg_poisson_set_stream(accbpg_poisson* h, void* stream);

/* PoissonRegression.func_grad (accbpg/functions.py:102-120): flag 0 -> *f_host = sum(b*log(b/Ax) + Ax - b);
 * flag 1 -> g_dev = A^T (1 - b/Ax); flag 2 -> both.  Synchronises the stream when a value is returned. */
int accbpg_poisson_func_grad(accbpg_poisson* h, const double* x_dev, int flag, double* f_host, double* g_dev);

/* out_dev <- Ax of the last func_grad (length m). */
int accbpg_poisson_get_ax(accbpg_poisson* h, double* out_dev);

/* ---- KL-divergence nonnegative regression with Shannon-entropy kernels ----------------------------------- */

typedef struct accbpg_kldiv accbpg_kldiv;

/* f(x) = D_KL(Ax, b): replaces KLdivRegression.__init__ (accbpg/functions.py:123-134).  Same layout and
 * ownership rules as accbpg_poisson_create: A row-major m x n with leading dimension lda >= n (any base
 * alignment), b length m; both owned by the caller. */
int accbpg_kldiv_create(const double* A_dev, int64_t m, int64_t n, int64_t lda, const double* b_dev,
                        void* stream, accbpg_kldiv** out);
int accbpg_kldiv_destroy(accbpg_kldiv* h);
int accbpg_kldiv_set_stream(accbpg_kldiv* h, void* stream);

/* KLdivRegression.func_grad (accbpg/functions.py:141-158): flag 0 -> *f_host = sum(Ax*log(Ax/b) - Ax + b);
 * flag 1 -> g_dev = A^T log(Ax/b); flag 2 -> both.  Synchronises the stream when a value is returned. */
int accbpg_kldiv_func_grad(accbpg_kldiv* h, const double* x_dev, int flag, double* f_host, double* g_dev);

/* out_dev <- Ax of the last func_grad (length m). */
int accbpg_kldiv_get_ax(accbpg_kldiv* h, double* out_dev);

/* ---- Soft-margin SVM with the hinge loss (accbpg/functions.py:161-194) ------------------------------------ */

typedef struct accbpg_svm accbpg_svm;

/* f(x) = mean_i max(0, 1 - y_i (A x)_i) + (lamda/2) <x,x>: replaces SVM_fun.__init__ (accbpg/functions.py:162-165).
 * Same layout and ownership rules as accbpg_poisson_create: A row-major m x n with leading dimension lda >= n (any
 * base alignment), y length m as doubles (the labels, +-1 or anything else); both owned by the caller.  lamda is an
 * argument of every evaluation.  A failed allocation leaves nothing of the handle behind. */
int accbpg_svm_create(const double* A_dev, int64_t m, int64_t n, int64_t lda, const double* y_dev, void* stream,
                      accbpg_svm** out);
int accbpg_svm_destroy(accbpg_svm* h);
int accbpg_svm_set_stream(accbpg_svm* h, void* stream);

/* SVM_fun.func_grad (accbpg/functions.py:183-194).  flag 0 -> f_host[0..1] = { sum_i max(0, 1 - y_i (Ax)_i), <x,x> },
 * one pass over A and no gradient work; the caller forms F = f_host[0]/m + lamda/2*f_host[1], the reference's
 * operation order, and <x,x> has the bits of accbpg_vec_dot(x, x).  flag 1 -> g_dev = lamda*x - A^T r / m with
 * r_i = (y_i (Ax)_i < 1) ? y_i : 0, nothing waits for the device; flag 2 -> both.  flag 3 -> g_dev = A^T r / m alone
 * (subgradient_loss, :179-181), no wait.  A NaN margin keeps its NaN in the sum and counts as "not < 1" in r; every
 * row enters A^T r, so 0*NaN propagates as in NumPy.  g_dev must not be x_dev.  Synchronises the stream when a value
 * is returned. */
int accbpg_svm_func_grad(accbpg_svm* h, const double* x_dev, double lamda, int flag, double* f_host, double* g_dev);

/* out_dev <- A x of the last evaluation (length m), the margins before the labels. */
int accbpg_svm_get_ax(accbpg_svm* h, double* out_dev);

/* ---- Logistic regression (accbpg/ex_LR_L2L1Linf.py:19-54, accbpg/functions.py:1068-1104) with L2L1Linf ----- */

typedef struct accbpg_logistic accbpg_logistic;

/* f(x) = (1/m) sum_i log(1 + exp(-y_i (A x)_i)).  Same layout and ownership rules as accbpg_svm_create: A row-major
 * m x n with leading dimension lda >= n (any base alignment), y length m as doubles (+-1 or anything else); both owned
 * by the caller.  A failed allocation leaves nothing of the handle behind. */
int accbpg_logistic_create(const double* A_dev, int64_t m, int64_t n, int64_t lda, const double* y_dev, void* stream,
                           accbpg_logistic** out);
int accbpg_logistic_destroy(accbpg_logistic* h);
int accbpg_logistic_set_stream(accbpg_logistic* h, void* stream);

/* flag 0 -> f_host[0] = sum_i t_i, t_i = max(-s_i, 0) + log1p(exp(-|s_i|)) with s_i = y_i (Ax)_i, summed on the fixed
 * tree; one pass over A, the caller forms f = f_host[0]/m.  flag 1 -> g_dev = A^T r / m with r_i = -(y_i q_i),
 * q_i = sigma(-s_i) = (s_i >= 0) ? e/(1+e) : 1/(1+e), e = exp(-|s_i|); nothing waits for the device.  flag 2 -> both.
 * A NaN s_i gives NaN t_i and r_i; s_i = +inf gives t_i = 0, q_i = 0; s_i = -inf gives t_i = +inf, q_i = 1.  Every row
 * enters A^T r, so 0*NaN propagates.  g_dev must not be x_dev.  Synchronises the stream when a value is returned. */
int accbpg_logistic_func_grad(accbpg_logistic* h, const double* x_dev, int flag, double* f_host, double* g_dev);

/* out_dev <- a length-m vector of the last evaluation: which 0 -> A x, 1 -> t, 2 -> r. */
int accbpg_logistic_get(accbpg_logistic* h, int which, double* out_dev);

/* Margins along a segment x + a d.  After a func_grad at x the handle holds z = A x with its t and r.
 * line_begin: w <- A d in one pass over A (the A x kernel of func_grad with a plain store).
 * line_value: f_host[0] <- sum_i t(fma(a, w_i, z_i)) on the fixed tree, O(m); z, t and r stay as they are.
 * line_accept: z_i <- fma(a, w_i, z_i) with its t_i and r_i, O(m); w is spent, the next line begins anew.
 * func_grad_carried: flag as in func_grad, from the handle's current z, t and r: the sum of t, and A^T r / m.
 * A func_grad rebases the margins to its x and spends w.  ACCBPG_ERR_ARG on a handle whose margins (or whose w, for
 * line_value and line_accept) are not current. */
int accbpg_logistic_line_begin(accbpg_logistic* h, const double* d_dev);
int accbpg_logistic_line_value(accbpg_logistic* h, double a, double* f_host);
int accbpg_logistic_line_accept(accbpg_logistic* h, double a);
int accbpg_logistic_func_grad_carried(accbpg_logistic* h, int flag, double* f_host, double* g_dev);

/* The Frank-Wolfe direction at x for the gradient g (length n, an n x r iterate flat): s_out_dev <- lmo(g),
 * d_out_dev <- s - x, out5_host <- {sum g^2, <g, d>, sum d^2, ||s - c|| (l2 ball away from its centre, else 0),
 * 1.0 when the l2 ball returned its centre}, idx_host[0] <- the first argmin of g (the simplex vertex), with one
 * synchronisation.  lmo_kind 0: the l2 ball, s = c - (radius*g)/||g||, the centre itself when ||g|| < 1e-10, decided
 * on the device; 1: the l-infinity ball, s = c - radius*sign(g); 2: the simplex, s = 1e-15 with s[argmin] = radius.
 * The centre as in accbpg_lmo_l2_ball (ignored by the simplex).  Entry by entry s and d have the bits of
 * accbpg_lmo_* / accbpg_vec_vertex followed by accbpg_vec_axpby(1, s, -1, x), and the three sums those of
 * accbpg_vec_dot on them.  Returns ACCBPG_ERR_ASSERT when | ||s - c|| - radius | > 1e-10 on the l2 ball.  The outputs
 * must not alias each other or the inputs.  ws_dev: accbpg_vec_workspace_doubles(n) doubles. */
int accbpg_fw_direction(const double* g_dev, const double* x_dev, int lmo_kind, int center_kind,
                        const double* center_dev, double center_val, double radius, int64_t n, double* s_out_dev,
                        double* d_out_dev, double* out5_host, int64_t* idx_host, double* ws_dev, void* stream);

/* L2L1Linf.prox_map (y_dev NULL) and div_prox_map (accbpg/functions.py:817-835) in one elementwise launch and the
 * reference's operation order: w = g - L*y, v = -((1/L)*w), thr = lamda/L; |v| <= thr -> +0.0, v > thr -> v - thr,
 * v < -thr -> v + thr; clipped to [-B, B], a NaN kept.  L <= 0 returns ACCBPG_ERR_ASSERT. */
int accbpg_l2l1linf_prox(const double* y_dev, const double* g_dev, double L, double lamda, double B, int64_t n,
                         double* out_dev, void* stream);

/* *out_host = sum_i |x_i| on the fixed tree with the block count of accbpg_vec_dot (L2L1Linf.extra_Psi, :801).
 * ws_dev: accbpg_vec_workspace_doubles(n) doubles. */
int accbpg_l1_norm(const double* x_dev, int64_t n, double* out_host, double* ws_dev, void* stream);

/* One streaming pass, one readback: out_host[0..2] <- { <g, x-y>, (1/2)||x-y||^2, (1/2)||z-z1||^2 }, each a tree sum
 * of its elementwise terms (g NULL: 0; z and z1 NULL together: 0).  ws_dev: accbpg_vec_workspace_doubles(n) doubles. */
int accbpg_sq_ls_terms(const double* g_dev, const double* x_dev, const double* y_dev, const double* z_dev,
                       const double* z1_dev, int64_t n, double* out_host, double* ws_dev, void* stream);

/* Shannon-entropy prox maps.  kind 0: ShannonEntropy, y_dev == NULL -> exp(-g/L - 1) (accbpg/functions.py:423-429),
 * y_dev != NULL -> y*exp(-g/L) (:431-438, asserts y >= 0); kind 1: ShannonEntropyL1, the same with lamda + g
 * (:456-466); kind 2: ShannonEntropySimplex, the kind-0 result divided by its sum (:475-490, the div form asserts
 * y > 0; ws_dev: accbpg_vec_workspace_doubles(n) doubles).  A failed assertion or L <= 0 returns ACCBPG_ERR_ASSERT. */
int accbpg_shannon_div_prox(int kind, const double* y_dev, const double* g_dev, double L, double lamda, int64_t n,
                            double* x_out_dev, double* ws_dev, void* stream);

/* out_host[0..2] <- { <g, x - y>, D(x, y), D(z, z1) } with D(x,y) = sum(x*log((x+delta)/(y+delta))) + (sum(y) -
 * sum(x)) (ShannonEntropy.divergence, accbpg/functions.py:415-421), each of the three sums reduced on its own fixed
 * tree.  g_dev NULL skips the first term (0), z_dev = z1_dev = NULL the last.  Negative entries of x, y, z, z1
 * return ACCBPG_ERR_ASSERT (:418).  One readback; ws_dev: accbpg_vec_workspace_doubles(n) doubles. */
int accbpg_shannon_ls_terms(const double* g_dev, const double* x_dev, const double* y_dev, const double* z_dev,
                            const double* z1_dev, int64_t n, double delta, double* out_host, double* ws_dev,
                            void* stream);
/* *out_host <- D(x, y) alone (accbpg_shannon_ls_terms without g, z, z1). */
int accbpg_shannon_divergence(const double* x_dev, const double* y_dev, int64_t n, double delta, double* out_host,
                              double* ws_dev, void* stream);

/* ---- Symmetric NMF: f(X) = 0.5*||M - X X^T||_F^2 with quartic kernels and ball LMOs --------------------- */

typedef struct accbpg_symnmf accbpg_symnmf;

/* Replaces FrobeniusSymLoss.__init__ (accbpg/functions.py:913-920).  M_dev: n x n symmetric, row-major, leading
 * dimension ldm >= n (any base alignment), owned by the caller and borrowed for the handle's lifetime; r: columns of
 * the iterates X (n x r, row-major, contiguous); m_norm: ||M||_F as the caller computed it (the value's t1 term). */
int accbpg_symnmf_create(const double* M_dev, int64_t n, int64_t ldm, int64_t r, double m_norm, void* stream,
                         accbpg_symnmf** out);
int accbpg_symnmf_destroy(accbpg_symnmf* h);
int accbpg_symnmf_set_stream(accbpg_symnmf* h, void* stream);

/* FrobeniusSymLoss.func_grad without noise (accbpg/functions.py:958-976): flag 0 -> *f_host = 0.5*(m_norm^2 +
 * ||X^T X||_F^2) - <X, M X>; flag 1 -> g_dev (n x r) = 2*X(X^T X) - 2*M X; flag 2 -> both.  One fp64 MFMA pass over
 * M per call.  Synchronises the stream when a value is returned. */
int accbpg_symnmf_func_grad(accbpg_symnmf* h, const double* X_dev, int flag, double* f_host, double* g_dev);

/* Launch plan of the handle: out4 <- {k pieces of the M X product, rows per piece, wide tile (r > 64), row chunks of
 * X^T X}. */
int accbpg_symnmf_plan(accbpg_symnmf* h, int64_t* out4);

/* First stage of SumOf2nd4thPowers(PositiveOrthant).div_prox_map (accbpg/functions.py:546-577): out_dev <- z*y -
 * invL*g, clipped to [0, upper_bound] when clip == 1 (pass +inf for no upper bound); *ssq_host <- ||out||^2.  The
 * caller solves the cubic and divides (accbpg_vec_div_scalar).  ws_dev: accbpg_vec_workspace_doubles(n) doubles. */
int accbpg_quartic_prox_stage(const double* y_dev, const double* g_dev, double z, double invL, int clip,
                              double upper_bound, int64_t n, double* out_dev, double* ssq_host, double* ws_dev,
                              void* stream);

/* One streaming pass, one readback: out7_host <- { <g,x-y>, ||x||^2, ||y||^2, <y,x-y>, ||z||^2, ||z1||^2,
 * <z1,z-z1> } (g NULL: 0; z and z1 NULL together: zeros).  SumOf2nd4thPowers.divergence (:518-521) is
 * h(x) - (h(y) + (sigma + alpha*||y||^2) <y, x-y>). */
int accbpg_quartic_ls_terms(const double* g_dev, const double* x_dev, const double* y_dev, const double* z_dev,
                            const double* z1_dev, int64_t n, double* out7_host, double* ws_dev, void* stream);

/* lmo_l2_ball (accbpg/functions_lmo.py:16-51) for ||g|| = gnorm >= 1e-10: out_dev <- c - (radius*g)/gnorm with c =
 * center_val (center_kind 0) or center_dev (center_kind 1, same length as g); *dist_host <- ||out - c||.  Returns
 * ACCBPG_ERR_ASSERT when | ||out - c|| - radius | > 1e-10.  ws_dev: accbpg_vec_workspace_doubles(n) doubles. */
int accbpg_lmo_l2_ball(const double* g_dev, int center_kind, const double* center_dev, double center_val,
                       double radius, double gnorm, int64_t n, double* out_dev, double* dist_host, double* ws_dev,
                       void* stream);

/* lmo_linf_ball (accbpg/functions_lmo.py:106-134): out_dev <- c - radius*sign(g), sign(0) = 0; c as above. */
int accbpg_lmo_linf_ball(const double* g_dev, int center_kind, const double* center_dev, double center_val,
                         double radius, int64_t n, double* out_dev, void* stream);

/* Closed-form Burg-entropy prox maps on x > 0.  kind 0: BurgEntropy.prox_map L/g (accbpg/functions.py:255-262);
 * kind 1: BurgEntropyL1.prox_map L/(lamda+g) (:290-298); kind 2: BurgEntropyL2.prox_map (:316-323).  With
 * y_dev != NULL the argument is g - L*(-1/y) first, i.e. BurgEntropy.div_prox_map (:264-271).
 * ACCBPG_ERR_ASSERT where the reference asserts: L <= 0, y.min() <= 0, g.min() <= 0 (kind 0),
 * g.min() <= -lamda (kind 1). */
int accbpg_burg_reg_div_prox(int kind, const double* y_dev, const double* g_dev, double L, double lamda,
                             int64_t n, double* x_out_dev, void* stream);

/* *out_host = <x, y>  (np.dot(x, x) of BurgEntropyL2.extra_Psi, accbpg/functions.py:314). */
int accbpg_vec_dot(const double* x_dev, const double* y_dev, int64_t n, double* out_host, double* ws_dev,
                   void* stream);

/* ---- inexact-oracle accelerated methods (AIBM, AdaptFGM, UniversalGM; accbpg/algorithms.py:593-777) ---- */

/* One pass, one read-back: w_dev <- (a*u + b*v)/c with NumPy's rounding (two products, one sum, one division; no fused
 * multiply-add), out2_host <- { <g, w - x>, D_h(w, x) } with h the Burg entropy (kind 0, accbpg/functions.py:253) or
 * (1/2)||.||^2 (kind 1, :749-751).  c = 1 is AIBM's alpha/B*z + (1-alpha/B)*y (algorithms.py:628, :632); c = A is
 * (alpha*u + A_k*x_k)/A of AdaptFGM and UniversalGM (:686-689, :744-748).  g_dev NULL: the inner product is 0.
 * x_dev NULL: only w is written, nothing is read back (out2_host and ws_dev may be NULL).  ACCBPG_ERR_ASSERT (kind 0)
 * when an entry of w or x is not positive.  w_dev must not alias an input.  Sums use a fixed tree.
 * ws_dev: accbpg_vec_workspace_doubles(n) doubles. */
int accbpg_combine_ls_terms(int kind, double a, const double* u_dev, double b, const double* v_dev, double c,
                            const double* g_dev, const double* x_dev, int64_t n, double* w_dev, double* out2_host,
                            double* ws_dev, void* stream);

/* BurgEntropySimplex.prox_map of an accumulated gradient in one call: xi_out_dev <- xi + alpha*g (one product, one
 * sum: AIBM's xi_grad += alpha*grad_x, algorithms.py:630) and x_out_dev <- prox_map(xi_out, L) (:631) with the
 * algorithm of accbpg_burg_simplex_div_prox unchanged -- for a given xi_out the result is that entry's, bit for bit.
 * Up to n = 32768 the sum is formed as the prox kernel loads its argument; longer vectors take a pass of their own
 * in front of the multi-workgroup prox.  xi_out_dev must not alias an input.  info_host (optional) receives
 * {bisection steps, Newton steps}; without it the call does not wait for the device. */
int accbpg_burg_simplex_prox_acc(const double* xi_dev, double alpha, const double* g_dev, double L, double eps,
                                 int64_t n, double* xi_out_dev, double* x_out_dev, double* ws_dev, int* info_host,
                                 void* stream);

/* lmo_l2_ball_positive_orthant (accbpg/functions_lmo.py:54-102): out_dev <- max(c + radius*d, epsilon) with
 * d = -g/||g_neg|| where g < 0 and 0 elsewhere, ||g_neg|| the norm over the negative entries (fixed-tree sum);
 * c = center_dev, or zeros when it is NULL.  With no negative entry out_dev <- max(c, epsilon) and nothing is asserted
 * (:83-84).  info3_host <- { number of negative entries, ||out - c||, min(out) }.  ACCBPG_ERR_ASSERT where the
 * reference asserts: min(out) < epsilon (:97), ||out - c|| > radius + 1e-8 (:98).  One read-back; g stays on the
 * device.  ws_dev: accbpg_vec_workspace_doubles(n) doubles. */
int accbpg_lmo_l2_ball_pos(const double* g_dev, const double* center_dev, double radius, double epsilon, int64_t n,
                           double* out_dev, double* info3_host, double* ws_dev, void* stream);

/* ---- diagnostics ---------------------------------------------------------------------- */

/* Kernel time accounting for the roofline line of bench.py: accumulates HIP-event durations
 * of the named kernel family on the handle's stream between reset and read.
 * which: 0 = Gram stream-K kernel (weighted SYRK), 1 = Cholesky (all its launches), 2 = triangular
 * inverse (all its launches), 3 = gradient kernel (triangular product + column norms), 4 = Gram
 * fix-up kernel, 5 = the pass over V of a Frank-Wolfe update (u = Hv^T V).  enable != 0 turns event recording on.
 * For a batch (accbpg_dopt_batch_*) the batched launches are accounted on the handle accbpg_dopt_batch_instance(b, 0). */
int accbpg_dopt_profile_enable(accbpg_dopt* h, int enable);
int accbpg_dopt_profile_read(accbpg_dopt* h, int which, double* total_ms_host, int64_t* launches_host);
int accbpg_dopt_profile_reset(accbpg_dopt* h);

/* fp64 MFMA peak microbenchmark: runs `iters` dependent-free v_mfma_f64_16x16x4_f64 per wave on
 * every CU and reports achieved TFLOP/s (used to confirm the roofline constant on the box). */
int accbpg_mfma_f64_peak(int iters, double* tflops_host, void* stream);

/* Development probe: milliseconds for `iters` loop trips of 8 fp64 MFMAs (mode bit 0) and / or 128 fp64 vector FMAs
 * (mode bit 1) per wave, one wave per SIMD on every CU -- do the matrix and the vector pipe run at the same time? */
int accbpg_debug_pipe_probe(int iters, int mode, double* ms_host, void* stream);

/* Unit-test hook: C (MxN) <- alpha * A (MxK, row-major) * op(B) + beta*C on the MFMA engine.
 * b_kmajor != 0: B is K x N row-major; else B is N x K row-major (A * B^T). */
int accbpg_test_gemm(const double* A_dev, int64_t lda, const double* B_dev, int64_t ldb,
                     double* C_dev, int64_t ldc, int64_t M, int64_t N, int64_t K,
                     int b_kmajor, double alpha, double beta, int config, void* stream);

/* Timing ablations of the Gram kernel (development aid; variant 0 is the product kernel, the
 * others drop global loads / LDS staging / the barrier / fragment reads and produce wrong data
 * into scratch).  Average milliseconds per launch over `iters` launches.  Codes 10..29: the direct-to-LDS kernel's
 * schedules and their ablations (tools/ablate_gram.py names them); 28 = the production schedule with its k-loop rolled
 * over a runtime stage index, 30 = with the stage a compile-time constant (production), 34..36 / 31..33 = "loads only",
 * "reads only", "MFMA only" of 28 / 30. */
int accbpg_debug_gram_variant(accbpg_dopt* h, const double* x_dev, int variant, int iters, double* ms_host);
/* The same for the direct-to-LDS gradient kernel, on the inverse factor the handle holds from its last gradient
 * evaluation: variant 0 = the product kernel, 3 = its schedule before the k loop was split into phases, 10..13 = that
 * schedule with rectangular k-steps only / diagonal k-steps only / MFMAs only / no drain and restart between row
 * blocks (wrong data); 4 = the product kernel with every k-step on the block schedule (reads and loads issued as
 * blocks, as before they were dealt out between the MFMAs), 5 = dealt out in the placement the product kernel does not
 * use, 6 = only the rectangular k-steps dealt out (4, 5, 6: same bits as 0); 20..23 / 30..33 = variant 4 / variant 0
 * with MFMAs only / MFMAs and loads / MFMAs and fragment reads / everything but the counted wait and the barrier
 * (wrong data).  g_dev (n doubles) receives what the launches write. */
int accbpg_debug_grad_variant(accbpg_dopt* h, double* g_dev, int variant, int iters, double* ms_host);
/* For a handle whose evaluations run BESIDE another stream's MFMA-bound launches (the value evaluation the solvers
 * start next to a gradient evaluation, accbpg/algorithms.py:135 beside :148): factor with one launch per 64-wide
 * block column -- a few workgroups at a time -- instead of the one-launch kernel, whose waiting workgroups would
 * hold the compute units the other stream needs.  Same arithmetic in the same order: bit-identical results.
 * on: 0 = one launch (default), 1 = small launches, 2 = small launches where the one launch would put at least a
 * workgroup on every compute unit (m > 1408 on 256 CUs), one launch below that. */
int accbpg_dopt_factor_in_small_launches(accbpg_dopt* h, int on);

/* Development switch for handles created AFTER the call: bit 0 = plain stream-K ranges of the Gram kernel also where the
 * tile list is longer than the grid (m >= 4096), instead of whole tiles per workgroup (A/B measurements). */
int accbpg_debug_plan_flags(int flags);

/* Debug switch, process wide: guard bands around the library's own device buffers.  While `bytes` > 0 (a multiple of
 * 4096, so that the buffers keep their alignment and no kernel changes its form), every device buffer the library
 * allocates gets `bytes` of the bit pattern 0x7FF8A5A5A5A5A5A5 in front of it and at least as many behind it (up to the
 * end of the buffer's last 4096-byte page); the fill is synchronous.  0 turns the switch off (the default: the
 * allocations are plain hipMalloc / hipFree); buffers made while it was on keep their bands until they are freed.
 * ACCBPG_ERR_ARG for any other value. */
int accbpg_debug_guard_bands(int64_t bytes);
/* Synchronises the current device and compares the bands of every live banded buffer with the pattern.
 * out3 = {live banded buffers, damaged bands, damaged bytes}.  When a band is damaged, accbpg_last_error names the first
 * one (in address order): the buffer's label, the side, and the offset of the first damaged byte -- negative from the
 * buffer's first byte for the front band, non-negative from the first byte past the buffer for the back band.  Returns
 * ACCBPG_OK whether or not it found damage. */
int accbpg_debug_guard_check(int64_t* out3);

/* Development switch, process wide, read at every launch: the k-loop of the products on the 64x64 tile (the merges of
 * the triangular inverse, their batched form, the trailing updates of the m > 2048 Cholesky, accbpg_test_gemm config 0).
 * 0 = production (the global loads of three k-steps in flight), 1 = the loop with one k-step of look-ahead that
 * production had before, 2..4 = that many k-steps in flight (A/B measurements).  Bit-identical results from all. */
int accbpg_debug_gemm_loop(int variant);

/* Development switch, process wide, read at every accbpg_burg_simplex_div_prox call.
 * variant: 0 = by size (production), 1 = burg_prox_kernel<0> (one workgroup, gg re-read from the workspace),
 * 2 = burg_prox_multi_kernel<8>, 3 = burg_prox_multi_kernel<32>.  A forced multi form whose workgroup count would
 * exceed 128 returns ACCBPG_ERR_ARG from the prox call, nothing launched.  Forcing 2 or 3 ignores the "multi off" latch
 * for that call but still sets it on a timeout. */
int accbpg_debug_prox_variant(int variant);
/* out3_host <- { variant the LAST prox call of this host thread launched (1, 2, 3 as above; 10, 11, 12 =
 * burg_prox_kernel<2>, <8>, <32>; a call that fell back after a timeout reports the kernel that produced the result),
 * workgroups of that launch, the "multi off" latch (0/1) }. */
int accbpg_debug_prox_state(int* out3_host);

/* Timing ablation bits for the Cholesky step kernel (development aid; 0 = product behaviour):
 * 1 skip the diagonal-block factorisation, 2 skip the panel solve, 4 skip the MFMA products; 8, 16, 32 switch
 * off the row solves / MFMA updates / 16x16 factor inside the 64x64 factorisation.  256 / 512 select the
 * register-staged / direct-to-LDS Gram and gradient kernels; bits 30..31 select the schedule of the direct-to-LDS
 * kernels (0 product, 1 / 2 development variants; bit-identical results); 1024 runs schedule 0 of the Gram kernel with
 * its k-loop rolled over a runtime stage index, as before the stage became a compile-time constant (the loop of timing
 * code 28 of accbpg_debug_gram_variant; without the bit, schedule 0 is the loop of code 30; bit-identical results).
 * 2048 sets the scheme of the factorisation
 * (results agree to rounding): bits 12..23 = number of 64-wide block columns from which the two-level scheme
 * runs (default 64), bits 24..29 = block columns per outer panel (default 8; 0 leaves it). */
int accbpg_debug_chol_variant(accbpg_dopt* h, int bits);
/* Development aid for the one-launch Cholesky (m <= 2048): factor gram_dev once while the workgroups on its critical
 * chain stamp the 100 MHz wall clock at their stage boundaries.  stamps_host: 32 x ceil(m/64) int64 (per block column:
 * workgroup start, left updates in, first piece of the previous factor here, last piece here, panel solve done,
 * diagonal tile staged, factored, published; then per 16-column piece of the streamed panel solve: asked for,
 * in LDS, solved, folded).  with_inverse != 0 also forms the inverses of the diagonal blocks (as a gradient evaluation). */
int accbpg_debug_chol_trace(accbpg_dopt* h, const double* gram_dev, int with_inverse, int64_t* stamps_host);

#ifdef __cplusplus
}
#endif
#endif /* ACCBPG_HIP_H */
