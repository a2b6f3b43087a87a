/* zfista_hip.h - C ABI of libzfista_hip.so, the MI355X (gfx950) engine behind
 * zfista_amd.minimize_proximal_gradient().
 *
 * The reference (zalgo3/zfista) has no FFI: the path it replaces is the Python
 * keyword API zfista/proximal_gradient.py:311-331.  This header is therefore the
 * interface the drop-in's own Python host binds through ctypes (INTEGRATION.md
 * shows the binding a zfista maintainer would add).  Every entry point names the
 * reference lines whose arithmetic it carries.
 *
 * Conventions: plain C, no exceptions across the boundary; every function
 * returns ZF_OK (0) or a negative ZF_ERR_* and leaves a message retrievable with
 * zf_last_error() (thread-local); sizes are int64_t, reals are double (the
 * reference is float64 throughout: zfista/problems.py:22); "dev" pointers are
 * device (HBM) addresses owned by the caller unless stated; `stream` is a
 * hipStream_t passed as void* (NULL = the default stream).  One solver object
 * per host thread/process and GPU; stream-ordered; thread-compatible, not
 * thread-safe.
 *
 * Caller-owned output memory is SIZED (ABI 4): every entry point that writes a struct or a
 * library-defined amount of data into caller memory takes the capacity of that buffer and
 * returns ZF_ERR_ARG - writing nothing - when it is too small (a host compiled against an
 * older, smaller zf_control is refused instead of overrun).  Arrays whose length is an
 * argument of the same call (n, m) are the caller's to size.
 */
#ifndef ZFISTA_HIP_H
#define ZFISTA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZF_ABI_VERSION 7

/* ---- status codes ------------------------------------------------------ */
#define ZF_OK 0
#define ZF_ERR_HIP (-1)      /* a HIP runtime call failed (message has details) */
#define ZF_ERR_ARG (-2)      /* invalid argument */
#define ZF_ERR_STATE (-3)    /* call sequence violated */
#define ZF_ERR_NODEVICE (-4) /* no usable GPU */

/* ---- zf_control.status: where the device-resident loop stands ---------- */
#define ZF_RUNNING 0
#define ZF_CONVERGED 1          /* err < tol            proximal_gradient.py:525-529 */
#define ZF_MAXITER 2            /* loop exhausted       proximal_gradient.py:539-543 */
#define ZF_BACKTRACK_FAILED 3   /* RuntimeError         proximal_gradient.py:306-307 */

/* ---- problem kinds (single objective, recognised descriptors) ---------- */
#define ZF_PROBLEM_DIAG_QUAD_L1 1     /* f = 1/2 sum d_i (x_i-c_i)^2, g = lam |x|_1 (+box) */
#define ZF_PROBLEM_LEAST_SQUARES_L1 2 /* f = scale |Ax-b|^2,          g = lam |x|_1 (+box) */
#define ZF_PROBLEM_BLUR_HAAR_L1 3     /* (ABI 5) f = scale |B W^-1 x - b|^2 with B an op_k x op_k correlation with symmetric
                                         boundary and W one orthonormal Haar level: the operator-form LASSO of the
                                         reference's examples/cameraman.ipynb:219-272; g = lam |x|_1 (+box)        */
#define ZF_PROBLEM_SPARSE_LS_L1 4     /* f = scale |Ax-b|^2 with A a CSR matrix behind a zf_spmat handle
                                         (zf_solver_create_sparse);     g = lam |x|_1 (+box)                       */
#define ZF_PROBLEM_LOGISTIC_L1 5      /* f = scale sum_i softplus(-b_i (Ax)_i), b_i in {-1, +1} (the labels; the caller checks
                                         them), A dense row-major as for kind 2; g = lam |x|_1 (+box); world = 1        */
#define ZF_PROBLEM_SPARSE_LOGISTIC_L1 6 /* the same f with A a CSR matrix behind a zf_spmat handle (zf_solver_create_sparse) */

#define ZF_PACK_LEN 8    /* doubles in one per-trial scalar pack */
#define ZF_MAX_SUB_ITERS 16 /* packs per pass: a rank's pack buffer holds sub_iters x ZF_PACK_LEN doubles */
#define ZF_DEFAULT_SUB_ITERS 16
#define ZF_MAX_LAG (2 * ZF_MAX_SUB_ITERS - 2) /* accepted iterations a solve may run ahead of its stored iterates */
#define ZF_PEND_FLUSH (-1) /* zf_control.pend_status: materialise the lagging iterates, then keep running */
#define ZF_TRACE_COLS 8  /* doubles per accepted iteration in the trace ring */
#define ZF_RING 1024     /* capacity (iterations) of the trace and momentum rings */

/* Device-resident control block of the line-search / termination logic
 * (proximal_gradient.py:279-307,510,525-538).  Lives in HBM; the decide kernel
 * is its only writer while a chunk of trials is in flight; zf_solver_poll()
 * copies it to the host.  Field order is ABI: the Python host mirrors it as a
 * numpy structured dtype and checks zf_sizeof_control(). */
typedef struct zf_control {
    double lr;            /* current learning rate; only ever shrinks (:305)          */
    double F_old;         /* F(x_k) = f + g at the latest accepted iterate (:279)    */
    double f_x, g_x;      /* its two parts                                            */
    double err;           /* max|x_k - y_k| of the latest accepted iteration (:510)  */
    double fun;           /* model value of the latest accepted trial (:149-155)     */
    double tol;           /* outer tolerance (:525)                                   */
    double tol_internal;  /* slack of the sufficient-decrease test (:303, tol=...)   */
    double decay_rate;    /* (:305); == 1 accepts unconditionally (:298)             */
    double f_y;           /* f(y_k) of the current line search                        */
    int64_t nit;          /* accepted outer iterations so far                         */
    int64_t max_iter;
    int64_t trial;        /* trials spent in the current line search                  */
    int64_t max_backtrack;
    int64_t total_trials; /* over the whole run                                       */
    int32_t status;       /* ZF_RUNNING ...                                           */
    int32_t cur;          /* which x buffer holds x_k                                 */
    int32_t nesterov;
    int32_t deprecated;   /* deprecated acceptance test (:300-302)                    */
    int32_t need_grad;    /* least squares: gradient at y_k must be (re)computed      */
    int32_t world;        /* ranks whose packs are summed by the decide step          */
    int32_t accept_mode;  /* (ABI 6) ZF_ACCEPT_*: how the sufficient-decrease test (:303) is evaluated */
    int32_t reserved0;
    double beta_next;     /* momentum factor of the next trial (:533), resolved from the
                             momentum ring by the decide step so that a trial kernel needs
                             ONE dependent scalar load (this block) before its first
                             vector load                                               */
    int32_t ring_size;    /* x buffers: 3 (one iteration per pass), 4 (chains), 6 (run-ahead) */
    int32_t sub_iters;    /* S: trials one pass chains in registers (temporal blocking) */
    int32_t prev;         /* which x buffer holds x_{k-1}                             */
    /* Deferred materialisation (temporal blocking, csrc/zf_decide.h).  A pass stores only the last two
     * iterates of its chain.  When a chain of fresh trials breaks after `a` acceptances (a rejection
     * or a termination in the middle), those a iterations ARE accepted - counters, F_old, trace rows
     * move on - but their iterates exist in no buffer: `lag` counts them, lag_lr[] keeps the step
     * size each was accepted with, and the buffers `cur` / `prev` hold x_{nit-lag}, x_{nit-lag-1}.
     * The next pass recomputes the lagging iterates element-wise in registers (no reductions: their
     * decisions are known) and chains its fresh trials behind them.  pend_status != 0: the next
     * pass only materialises (no fresh trials); afterwards status = pend_status (a final status
     * reached while iterates were lagging) or, for ZF_PEND_FLUSH, the solve simply continues. */
    int32_t lag;
    int32_t pend_status;
    int32_t pass_seq;     /* number of the step whose pass was decided inside its trial launch (0: none yet) */
    double lag_lr[ZF_MAX_LAG];
} zf_control;

/* zf_options.accept_mode / zf_control.accept_mode (ABI 6).  The reference accepts a trial when
 *     F(x+) - F(x_k) <= fun + tol_internal,  fun = <grad f(y), x+ - y> + g(x+) + |x+ - y|^2 / 2 / lr + (f(y) - F(x_k))   (:149-155, :303)
 * - two differences of O(|F|) numbers.  In exact arithmetic F(x_k) and g(x+) cancel and the test reads
 *     [f(x+) - f(y)] - <grad f(y), x+ - y> - |x+ - y|^2 / 2 / lr <= tol_internal.
 * ZF_ACCEPT_REFERENCE evaluates the reference's expression as it stands (default: same decisions as the reference, and
 * below double-precision resolution once |x+ - y|^2 << ulp(F): at n = 1e8 trials are rejected by rounding noise from
 * iteration ~90 on).  ZF_ACCEPT_RESOLVED (opt-in; separable problems) evaluates the second form with f(x+) - f(y)
 * accumulated element by element (pack slot 7), so the test resolves ~1e-16 of the step, not of F; f(x+) is then reported
 * as f(y) + [f(x+) - f(y)].  Iterates of accepted trials are the same arithmetic either way.  One difference by design:
 * with F(x_k) = inf (x_k outside the box) the reference's expression accepts every trial (-inf <= -inf); the resolved form
 * still tests the smooth part.
 * ZF_ACCEPT_REMAINDER (opt-in; ZF_PROBLEM_LEAST_SQUARES_L1 and ZF_PROBLEM_SPARSE_LS_L1) moves the dot product to the left as
 * well: the Taylor remainder R = f(x+) - f(y) - <grad f(y), x+ - y> of a loss of the margins s = A x can be formed without
 * cancelling anything - for least squares it is exactly scale |A (x+ - y)|^2 = scale sum_i (s+_i - s_y,i)^2 with
 * s_y = s_k + beta (s_k - s_{k-1}), both margin vectors being in HBM already - and the test reads
 *     R - |x+ - y|^2 / 2 / lr <= tol_internal          (:301, deprecated: R <= g(x+) + |x+ - y|^2 / 2 / lr + tol_internal),
 * every term non-negative and of the size of the step (pack slot 7 carries R).  f(x+) is computed and reported exactly as
 * under ZF_ACCEPT_REFERENCE: where both modes decide alike, iterates and traces are bit-identical.  With F(x_k) = inf this
 * mode, too, still tests the smooth part. */
#define ZF_ACCEPT_REFERENCE 0
#define ZF_ACCEPT_RESOLVED 1
#define ZF_ACCEPT_REMAINDER 2

typedef struct zf_problem_desc {
    int32_t kind;      /* ZF_PROBLEM_*                                                */
    int32_t world;     /* ranks sharing the decision vector (1 = unsharded)           */
    int32_t rank;
    int32_t row_sharded; /* LEAST_SQUARES_L1, world > 1: 0 = the COLUMNS of A and x are split over the
                            ranks (b replicated; the m-vector A_p x_p is exchanged once per trial);
                            1 = the ROWS of A and b are split, x is replicated on every rank and the
                            n-vector A_p^T r_p is exchanged ("all-reduce of A^T r")          */
    int64_t n;         /* length of x held by this rank (its shard; the whole x if row_sharded) */
    int64_t m_rows;    /* least squares: rows of A held by this rank (0 otherwise)   */
    const double* d;   /* dev, n   - DIAG_QUAD_L1                                     */
    const double* c;   /* dev, n   - DIAG_QUAD_L1                                     */
    const double* A;   /* dev, m_rows x n row-major - LEAST_SQUARES_L1                */
    const double* b;   /* dev, m_rows                                                 */
    double scale;      /* LEAST_SQUARES_L1: f = scale |Ax-b|^2                        */
    double lam;        /* l1 weight                                                   */
    double box_lo;     /* -inf / +inf when there is no box                            */
    double box_hi;
    /* (ABI 5) ZF_PROBLEM_BLUR_HAAR_L1: x = the Haar coefficients [cA, cH, cV, cD] (each op_h/2 x op_w/2, row-major) of an
     * op_h x op_w image (both even; n = m_rows = op_h * op_w), b = the observed image (dev), op_taps = the correlation
     * kernel, op_k x op_k row-major (dev; op_k odd, <= 15).  Zero for the other kinds. */
    int64_t op_h, op_w;
    const double* op_taps;
    int32_t op_k;
    int32_t op_reserved;
} zf_problem_desc;

typedef struct zf_options {  /* keyword arguments of proximal_gradient.py:317-330 */
    double lr;
    double tol;
    double tol_internal;
    double decay_rate;
    int64_t max_iter;
    int64_t max_backtrack_iter;
    int32_t nesterov;
    int32_t deprecated;
    int32_t sub_iters;   /* S: trials one pass over the data chains in registers, for separable
                            problems (temporal blocking): 0 = library default (ZF_SUB_ITERS in the
                            environment, else ZF_DEFAULT_SUB_ITERS), 1 / 2 / 4 / 8 / 16 explicit.  Results do not depend on it;
                            lam >= 0, lr > 0, decay_rate > 0 are required by the fused kernels.     */
    int32_t accept_mode; /* (ABI 6; was reserved = 0) ZF_ACCEPT_REFERENCE, ZF_ACCEPT_RESOLVED (ZF_PROBLEM_DIAG_QUAD_L1 only) or
                            ZF_ACCEPT_REMAINDER (ZF_PROBLEM_LEAST_SQUARES_L1, ZF_PROBLEM_SPARSE_LS_L1 only) */
} zf_options;

typedef struct zf_solver zf_solver; /* opaque; owns x ring, partials, control, rings */

/* ---- library, device, memory ------------------------------------------- */
int zf_abi_version(void);
const char* zf_last_error(void);
int64_t zf_sizeof_control(void);
int zf_device_count(int* count);
int zf_set_device(int device);
int zf_malloc(void** dev_ptr, int64_t bytes);
int zf_free(void* dev_ptr);
int zf_memcpy_h2d(void* dst_dev, const void* src_host, int64_t bytes, void* stream);
int zf_memcpy_d2h(void* dst_host, const void* src_dev, int64_t bytes, void* stream);
int zf_memcpy_d2d(void* dst_dev, const void* src_dev, int64_t bytes, void* stream);
int zf_stream_synchronize(void* stream);
/* release the library's staging workspaces (one per host thread and device, used by zf_host_* / zf_dev_*);
 * call when none of those is in flight - a later call allocates again */
int zf_shutdown(void);

/* ---- RCCL communicator (x sharded over the GPUs of one node) -----
 * One rank per GPU/process.  Rank 0 calls zf_comm_unique_id and ships the 128 bytes to the other ranks
 * over any host channel; then every rank calls zf_comm_create (collective) with its GPU current.
 * librccl is loaded with dlopen on first use - single-GPU users never need it. */
typedef struct zf_comm zf_comm;
int zf_comm_unique_id(void* id128);
int zf_comm_create(zf_comm** out, int32_t rank, int32_t world, const void* id128);
int zf_comm_destroy(zf_comm* c);
/* in-process stand-in (tests on one GPU, where RCCL cannot place two ranks): `world` communicators for
 * `world` host threads with a stream each; all-gathers go through a shared staging buffer, a host
 * barrier and stream events.  cap_doubles bounds the per-rank count of an all-gather. */
int zf_comm_create_local_group(zf_comm** out_world, int32_t world, int64_t cap_doubles);
int zf_comm_info(zf_comm* c, int32_t* rank, int32_t* world);
/* What the communicator says about itself (ABI 5): nccl_* come from RCCL's own queries of the ncclComm_t
 * (ncclCommCount / ncclCommUserRank / ncclCommCuDevice; -1 for the in-process stand-in), not from what the caller
 * passed to zf_comm_create; `library` is the file the RCCL symbols were resolved from.  out_bytes = capacity of *out
 * (a short buffer is refused before anything is written). */
typedef struct zf_comm_desc {
    int32_t rank, world;      /* as given at creation */
    int32_t kind;             /* 0: RCCL communicator, 1: in-process thread-rank group */
    int32_t nccl_count;       /* ranks RCCL reports for this communicator */
    int32_t nccl_user_rank;
    int32_t nccl_device;
    int32_t rccl_version;     /* ncclGetVersion (0: not available) */
    int32_t reserved;
    int64_t all_gathers;      /* zf_comm_all_gather calls issued on this communicator so far */
    char library[256];
} zf_comm_desc;
int zf_comm_describe(zf_comm* c, zf_comm_desc* out, int64_t out_bytes);
/* recv (world x count doubles, rank-major) <- send (count doubles) of every rank; stream-ordered */
int zf_comm_all_gather(zf_comm* c, const double* send_dev, double* recv_dev, int64_t count, void* stream);

/* f(x) and (grad_out_host != NULL) jac_f(x) of ZF_PROBLEM_BLUR_HAAR_L1 for a host vector x (n = h * w doubles): the
 * problem's callbacks outside the device-resident loop (ABI 5) */
int zf_op_eval(const double* taps_dev, int32_t k, const double* b_dev, int64_t h, int64_t w, double scale,
               const double* x_host, double* f_out, double* grad_out_host);

/* ---- the decision step on the host (no GPU needed) ----------------------
 * Same inline function the decide kernel runs (csrc/zf_decide.h); exported so
 * the control logic of proximal_gradient.py:279-307,510,525-543 can be tested
 * on a machine without a GPU.  `packs` holds `world` packs of ZF_PACK_LEN
 * doubles; `trace` is a ZF_RING x ZF_TRACE_COLS ring. */
int zf_decide_host(zf_control* ctl, int64_t ctl_bytes /* == zf_sizeof_control() */, const double* packs,
                   double* trace);

/* ---- device-resident single-objective solver -----------------------------
 * Replaces the body of the outer loop, proximal_gradient.py:474-538, for the
 * recognised problem kinds.  One "step" = one pass over the data = a chain of up to sub_iters
 * line-search trials, each assuming the one before was accepted (least squares: one trial):
 *   trial kernel  : y = x_k + beta (x_k - x_{k-1})            (:534)
 *                   x+ = prox_{lr g}(y - lr grad f(y))         (:148)
 *                   per-block partials of f(y), <grad f,x+-y>, |x+-y|^2,
 *                   g(x+), f(x+), max|x+-y|                    (:140,:150-152,:295,:510)
 *   finalize      : fixed-order reduction of the partials -> one pack per trial
 *   decide        : per trial, in order: model value, acceptance, lr decay, termination,
 *                   trace row (:149-155,:298-305,:525); a chain that holds is committed
 *                   (buffer hand-over); one that breaks after >= 1 accepted trials leaves those
 *                   iterations accepted but not stored (zf_control.lag; csrc/zf_decide.h) and
 *                   the next pass recomputes them in registers ahead of its fresh trials
 */
int zf_solver_create(zf_solver** out, const zf_problem_desc* desc, const zf_options* opt,
                     void* stream);
int zf_solver_destroy(zf_solver* s);
/* copy x0 (dev, n) into the ring and evaluate f(x0), g(x0) -> local init pack (:463-466) */
int zf_solver_enqueue_init(zf_solver* s, const double* x0_dev);
/* consume the (gathered) init packs: F_old = sum over ranks; world == 1 may skip the gather */
int zf_solver_enqueue_init_commit(zf_solver* s);
/* momentum factors beta_j for accepted-iteration indices first..first+count-1 (:531-533) */
int zf_solver_set_beta(zf_solver* s, int64_t first, const double* beta_host, int64_t count);
/* world == 1: enqueue `steps` complete steps (trial+finalize+decide), no host sync; a step accepts
 * between 0 and sub_iters iterations, so poll before the device can be ZF_RING iterations ahead.
 * CONTRACT: a step runs the pass the host EXPECTS from the control block of its last zf_solver_poll (advanced on
 * the assumption that every trial since was accepted).  When the device takes another turn - a trial rejected, a
 * termination inside a chain - the steps already enqueued behind it may be no-ops (no kernel finds its shape, the
 * control block stays as it is) until the next zf_solver_poll: N steps advance the solve by AT MOST N passes, and
 * only the first step after a poll is guaranteed to run.  Behind a chunk that saw rejections the library launches a
 * fallback kernel with every step, so such chunks lose no passes.  ZF_SPECULATE=0 launches every shape always. */
int zf_solver_enqueue_steps(zf_solver* s, int64_t steps);
/* after initialisation: fix the launch geometry (interleaved tiles per workgroup) of the trial
 * kernel.  It is a function of n only - never of a timing measurement, the chain length or the
 * device - because it decides the rounding of the reduced sums: the same problem takes the same
 * decisions in every process.  ZF_TILES_PER_WG=<n> overrides it (experiments). */
int zf_solver_autotune(zf_solver* s, int32_t* chosen_tiles);
/* make the next step materialise iterates that lag behind the accepted count (zf_control.lag),
 * so that buffers cur / prev hold x_k, x_{k-1} afterwards; stream-ordered, no-op without lag */
int zf_solver_flush(zf_solver* s);
/* world > 1 with a communicator attached: the solver issues the exchanges of a sharded step itself
 * (packed all-gather of the scalar packs; for column-sharded least squares also of A_p x_p) on its
 * stream - zf_solver_enqueue_steps then works for world > 1 and a pass needs no host code.
 * zf_solver_enqueue_init_all = init + exchanges + commit in one call (world == 1 too).
 * Call it BEFORE zf_solver_enqueue_init / _init_all / zf_solver_restore: a one-rank solver may grow its iterate ring for
 * passes ahead here; once an initialisation is enqueued, a call that would grow it is refused with ZF_ERR_STATE (nothing
 * attached). */
int zf_solver_set_comm(zf_solver* s, zf_comm* comm);
int zf_solver_enqueue_init_all(zf_solver* s, const double* x0_dev);
/* world > 1 without one: the two halves of a step; the caller gathers pack_local -> pack_all between them */
int zf_solver_enqueue_trial(zf_solver* s);
int zf_solver_enqueue_decide(zf_solver* s);
/* device addresses of this rank's packs (sub_iters x ZF_PACK_LEN doubles) and of the gathered
 * packs (world x sub_iters x ZF_PACK_LEN doubles, rank-major); zf_solver_sub_iters() tells S */
int zf_solver_sub_iters(zf_solver* s, int32_t* sub_iters);
/* streaming return_all (proximal_gradient.py:521-524): from now on every trial also stores its
 * iterate x_{k+1} into slot (k + 1) % cap_slots of the caller-owned ring `hist_dev` (slots `stride`
 * doubles apart, stride >= n and a multiple of 64) - 8 more bytes per element and iteration, no host
 * transfer, chains stay 8 long.  Slot 0 (x0) is the caller's.  Chain lengths 1 and 8. */
int zf_solver_set_history(zf_solver* s, double* hist_dev, int64_t cap_slots, int64_t stride);
/* change max_iter of a live solve (stream-ordered); a solve stopped by ZF_MAXITER resumes when
 * the new bound is above nit - how a caller continues `res.nit < max_iter` runs (:539) */
int zf_solver_set_max_iter(zf_solver* s, int64_t max_iter);
int zf_solver_pack_ptrs(zf_solver* s, double** pack_local_dev, double** pack_all_dev);
/* make the solver write / read caller-owned pack buffers instead (e.g. torch
 * tensors the collective runs on); sizes as above; must outlive the solver */
int zf_solver_set_pack_buffers(zf_solver* s, double* pack_local_dev, double* pack_all_dev);
/* sharded least squares.  Column blocks (x split): the m-vector A_p x_p of every rank
 * is exchanged once per trial.  Row blocks (desc.row_sharded, x replicated): the n-vector
 * 2 scale A_p^T r_p is exchanged instead (s_part / s_all then hold n and world x n doubles) and the
 * init needs no exchange of its own.  Between
 * zf_solver_enqueue_trial() and zf_solver_enqueue_trial_finish() (and between
 * zf_solver_enqueue_init() and zf_solver_enqueue_init_finish()) the caller gathers
 * s_part (m doubles) of all ranks into s_all (world x m, rank-major); the finish call
 * adds the parts in rank order.  Both finish calls are no-ops for other problems. */
int zf_solver_svec_ptrs(zf_solver* s, double** s_part_dev, double** s_all_dev);
int zf_solver_set_svec_buffers(zf_solver* s, double* s_part_dev, double* s_all_dev);
int zf_solver_enqueue_trial_finish(zf_solver* s);
int zf_solver_enqueue_init_finish(zf_solver* s);
/* synchronise the stream, copy out the control block and (trace_host != NULL) the trace ring.
 * ctl_bytes / trace_bytes: capacity of the two host buffers; ZF_ERR_ARG, nothing written, unless
 * ctl_bytes >= zf_sizeof_control() and trace_bytes >= ZF_RING * ZF_TRACE_COLS * 8 */
int zf_solver_poll(zf_solver* s, zf_control* ctl_host, int64_t ctl_bytes, double* trace_host, int64_t trace_bytes);
/* device address / host copy of the latest accepted iterate x_k (local shard) */
int zf_solver_x_dev(zf_solver* s, const double** x_dev);
int zf_solver_get_x(zf_solver* s, double* x_host, int64_t count /* capacity in doubles, >= n */);
/* checkpoint / resume: zf_solver_poll + zf_solver_get_x + zf_solver_get_x_prev are the state of a
 * solve (x_k, x_{k-1}, control block); zf_solver_restore puts it into a freshly created solver
 * instead of zf_solver_enqueue_init(+_commit), after which the host re-uploads the momentum
 * factors from accepted count `nit` on.  The resumed solve continues bit for bit, provided it is advanced the way the saved
 * one was: by zf_solver_enqueue_steps (with or without a communicator, attached before the restore), or by the host-driven
 * sequence zf_solver_enqueue_trial / _trial_finish / _decide on caller-owned pack buffers (zf_solver_set_pack_buffers before
 * the restore: that is how the solver tells the two apart - on a shape of the fused small-matrix path they sum A x in
 * different orders, and the restore rebuilds A x_k, A x_{k-1} in the order of the sequence it expects). */
int zf_solver_get_x_prev(zf_solver* s, double* x_host, int64_t count /* >= n */);
int zf_solver_restore(zf_solver* s, const double* xk_dev, const double* xprev_dev, const zf_control* saved,
                      int64_t saved_bytes /* == zf_sizeof_control(): a block of another layout is refused */);
/* average duration (ms) of the trial kernel over the launches since the last
 * call, measured with HIP events on the solver's stream; resets the window.
 * What the event pair brackets depends on the kind: the fused trial kernel (the prox step) for ZF_PROBLEM_DIAG_QUAD_L1,
 * ZF_PROBLEM_LEAST_SQUARES_L1 and ZF_PROBLEM_BLUR_HAAR_L1 - the sweeps over A are NOT in it - but the WHOLE trial
 * (residual at y, both sweeps, prox step, f(x+), finalize) for ZF_PROBLEM_SPARSE_LS_L1.  The logistic kinds follow their
 * siblings: ZF_PROBLEM_LOGISTIC_L1 as kind 2, ZF_PROBLEM_SPARSE_LOGISTIC_L1 as kind 4.  The same holds for
 * zf_solver_pass_stats(_ex) and zf_solver_pass_records. */
int zf_solver_trial_kernel_ms(zf_solver* s, double* avg_ms, int64_t* launches);
/* since creation: out[0] = trial steps issued, out[1] = trial kernels launched for them; with count >= 4 also
 * out[2] = out[3] = 0 (ABI 5: the counts of a multi-pass kernel that round 5 withdrew).  A chained pass has
 * one of several shapes (full chain, short, general, a mid chain of 9 .. 15 trials) and needs one kernel; the host
 * launches the one it expects once a poll has shown it the control block - unsharded, and sharded through the
 * library's communicator; behind a chunk that saw rejections the general body rides along as the complement of the
 * expected kernel (on small grids: alone); with nothing known, the three kernels that between them run every shape.
 * With count >= 6 also out[4] = run-ahead passes launched, out[5] = those of them launched while their predecessor
 * was still in flight: on grids the device holds at once consecutive full chains go alternately to the solver's stream and a
 * second one of its own, pass p + 1 running while pass p is finalised (zf_runahead_kernel; ZF_RUNAHEAD=0: off; six iterate
 * buffers instead of four).  zf_solver_enqueue_steps returns with the solver's stream made to wait for the second.
 * (ABI 6) With count >= 8, as of the last zf_solver_poll: out[6] = waits of run-ahead passes that GAVE UP (a workgroup's
 * for its predecessor workgroup, a deciding wave's for the decision before it: ZF_RUNAHEAD_SPIN_LIMIT polls, ~15 ms -
 * the device did not hold two passes of this solver at once, i.e. it is shared), out[7] = run-ahead passes that turned
 * out VOID (a prediction failed, or a wait gave up).  After the first wait that gave up the solver launches no further
 * run-ahead passes (count >= 11: out[10] = 1) and runs one launch per pass - same results, no 15 ms stalls.
 * With count >= 10: out[8] = passes launched AHEAD at kernel granularity, out[9] = those of them void: sharded solves through
 * the library's communicator (and, ZF_AHEAD_UNSHARDED=1, unsharded grids the run-ahead kernel does not take) run the trial
 * kernels of consecutive exactly predicted full / mid chains back to back on the solver's stream, each on the head the host
 * expects, while finalisation, all-gather and decide of the pass before run on the second stream (ZF_AHEAD=0: off).
 * With count >= 12, as of the last zf_solver_poll: out[11] = second passes of a run (of either scheme) whose first pass
 * started behind a pass that broke unseen and left on a head that did not come true; they run no body (the buffers they
 * would write hold the real x_k, x_{k-1} then). */
int zf_solver_launch_counts(zf_solver* s, int64_t* out, int64_t count /* >= 2 */);
/* least squares: the kernels the passes of zf_solver_enqueue_steps run, fixed at zf_solver_create.  out[0] = the column
 * sweep A^T r: 0 not least squares, 1 the small-matrix step kernel (zf_ls_small_step_kernel), 2 the MFMA sweep
 * (zf_gemvT_partial_mfma_kernel), 3 the VALU sweep with 16-byte loads (zf_gemvT_partial_kernel<2>), 4 with scalar loads
 * (<1>); out[1] = the row sweep A x+: 1 zf_ls_small_rows_kernel, 2 zf_gemv_rows_kernel<2>, 3 <1>; out[2] = row slices
 * of the general column sweep, out[3] = rows per slice (the last slice may be shorter).
 * (A host-driven trial - zf_solver_enqueue_trial - always takes the general path.)
 * The operator problem (ZF_PROBLEM_BLUR_HAAR_L1) reports its plan in the same four slots: out[0] = tile height (8 or 32
 * rows), out[1] = 1 the separable (rank-1) correlation / 0 the general one, out[2] = 1 workgroups walk their tiles /
 * 0 one workgroup per tile, out[3] = 1 the prox step runs in the adjoint kernel's epilogue / 0 a launch of its own.
 * Sparse least squares (ZF_PROBLEM_SPARSE_LS_L1): out[0] = 5, out[1] = lanes per row of the sweep over A, out[2] = lanes
 * per row of the sweep over A^T, out[3] = split rows of A plus split rows of A^T.  (Beyond 32768 rows this kind forms
 * r = A y - b, f(y) and f(x+) with up to 1024 workgroups and adds their chunk sums in chunk order; up to there with the one
 * workgroup of the dense kind: the order of those two sums is a function of m alone, and changes at that size.)
 * The logistic kinds report the plan of their storage form in the same slots: ZF_PROBLEM_LOGISTIC_L1 out[0] = 2, 3 or 4 and
 * out[1] = 2 or 3 as ZF_PROBLEM_LEAST_SQUARES_L1 (never 1: the small-matrix kernels hold the squared loss), out[2], out[3]
 * the slices; ZF_PROBLEM_SPARSE_LOGISTIC_L1 out[0] = 5 and the lanes / split rows as ZF_PROBLEM_SPARSE_LS_L1.  (Both form
 * rho(y), f(y) and f(x+) with one workgroup up to 32768 rows and with up to 1024 beyond, chunk sums added in chunk order.)
 * A dense matrix stored in fp32 (zf_solver_set_matrix_f32, either dense kind): out[0] = 6, 7 or 8 - the column sweep
 * zf_gemvT_partial_f32_kernel<4> (16-byte loads of four floats, n % 4 == 0), <2> (8-byte loads, n % 4 == 2), <1> (odd n) -
 * out[1] = 4, 5 or 6 - the row sweep zf_gemv_rows_f32_kernel<4>, <2>, <1> - out[2], out[3] the slices of the fp32 rule.
 * K responses (zf_solver_set_responses, either dense kind): out[0] = 9 or 10 - the column sweep zf_mr_cols_partial_kernel<K, 2>
 * (16-byte loads, even n) or <K, 1> (odd n; n the matrix's own column count) - out[1] = 7 or 8 - the row sweep
 * zf_mr_rows_kernel<K, 2>, <K, 1> - out[2], out[3] the slices of that rule on the matrix's own shape.
 * count >= 6 (dense kinds; what the first four slots hold does not depend on count): out[4] = K (1 without the setter), out[5] = the
 * rows a workgroup of the K-response row sweep owns (0 without the setter).  The sparse kinds keep 5, L(A), L(A^T), split rows in the
 * first four slots whatever K is (the handle's plan serves every K); count >= 6: out[4] = K (zf_solver_create_sparse_responses; 1
 * otherwise), out[5] = 0.
 * Other problems: zeros. */
int zf_solver_ls_plan(zf_solver* s, int64_t* out, int64_t count /* >= 4 */);
/* the same window split by the shape of the pass, which the kernel logs itself: out[0], out[1] = mean
 * ms and count of full chains (sub_iters fresh trials, nothing replayed); out[2], out[3] = every other
 * pass (shorter chains, replays, materialise-only).  Resets the window. */
int zf_solver_pass_stats(zf_solver* s, double* out, int64_t count /* >= 4 */);
/* the same window plus out[4] = fresh trials and out[5] = replayed iterations the other passes carried */
int zf_solver_pass_stats_ex(zf_solver* s, double* out, int64_t count /* >= 6 */);
/* sharded solves, timing on (ABI 5): out[0] = mean ms, out[1] = count of the per-pass pack exchanges since the last
 * call, each timed on this rank's stream from "my packs are ready" to "the gathered packs are here" */
int zf_solver_exchange_stats(zf_solver* s, double* out, int64_t count /* >= 2 */);
/* timing on (ABI 5): one (shape, milliseconds) pair per launch that ran a pass since the last call, oldest first; shape =
 * fresh trials | lagging iterations << 5; launches whose pass turned out void (it ran ahead on a head that did not come true)
 * are left out; *count = pairs written (<= cap_pairs) */
int zf_solver_pass_records(zf_solver* s, double* out, int64_t cap_pairs, int64_t* count);
int zf_solver_set_timing(zf_solver* s, int32_t enabled);

/* ---- vector kernels for opaque (Python) callbacks ------------------------
 * The solver's own O(n) arithmetic when f/g/jac_f/prox are arbitrary host
 * callables: v = y - lr*jac (:148), {<jac,x-y>, |x-y|^2, max|x-y|} (:150-152,
 * :510) and y = x + beta (x - x_old) (:534).  Host pointers in, host pointers
 * out; the library stages through its own device workspace. */
int zf_host_grad_step(double* v_host, const double* y_host, const double* jac_host, double lr,
                      int64_t n);
int zf_host_model_terms(const double* jac_host, const double* x_host, const double* y_host,
                        int64_t n, double out3[3]);
int zf_host_momentum(double* y_out_host, const double* x_host, const double* x_old_host,
                     double beta, int64_t n);
/* the same three expressions on device vectors (callbacks written against device tensors:
 * iterates stay in HBM; zf_dev_model_terms synchronises `stream` to return its three scalars).
 * Sharing: the zf_dev_* calls and zf_eval_diag_l1 of ONE host thread share, per device, one buffer of block
 * partials and one 8-double result block (the staging workspace of the zf_host_* calls, which zf_shutdown
 * releases).  A call only enqueues work on `stream`, so two calls of one thread on DIFFERENT streams would
 * overwrite each other's partials: the caller orders them against each other (an event, a synchronisation, or
 * simply one stream per thread).  Calls of different host threads never share: solve_on_streams gives each
 * stream a thread of its own. */
int zf_dev_grad_step(double* v_dev, const double* y_dev, const double* jac_dev, double lr, int64_t n, void* stream);
int zf_dev_model_terms(const double* jac_dev, const double* x_dev, const double* y_dev, int64_t n,
                       double out3_host[3], void* stream);
int zf_dev_model_terms_async(const double* jac_dev, const double* x_dev, const double* y_dev, int64_t n,
                             double* out3_dev, void* stream);   /* no synchronisation; scalars stay on the device */
int zf_dev_momentum(double* y_out_dev, const double* x_dev, const double* x_old_dev, double beta, int64_t n,
                    void* stream);
/* Multi-objective trial with callbacks on device tensors (m >= 2): the solver's own expressions of
 * _dual_minimized_fun_jac (:162-173) around the caller's prox_wsum_g and g.
 *   zf_dev_mo_combine:    v = y - lr (w @ J) (:164), ss_dev[0] = |w @ J|^2 (:171); J m x n row-major, w on the host
 *   zf_dev_mo_post_terms: out_dev[0..m) = J_i . (p - y) (:173), out_dev[m] = |p - v|^2 (:168)
 * stream-ordered, nothing synchronised (the caller fetches the scalars with its own in one transfer) */
int zf_dev_mo_combine(double* v_dev, const double* y_dev, const double* J_dev, const double* w_host, double lr,
                      int32_t m, int64_t n, double* ss_dev, void* stream);
int zf_dev_mo_post_terms(const double* J_dev, const double* y_dev, const double* p_dev, const double* v_dev,
                         int32_t m, int64_t n, double* out_dev /* m + 1 */, void* stream);

/* ---- operator evaluations at a host point ---------------------------------
 * The callback contract of proximal_gradient.py rows f / g / jac_f /
 * prox_wsum_g (:140-148) for the recognised operators, evaluated on the GPU at
 * a point given in host memory (problem data stays in HBM).  These back the
 * NumPy-callable methods of zfista_amd.problems.* . */
/* out = sign(x) max(|x| - tau, 0), then clip to [lo, hi]   (problems.py:128-137) */
int zf_host_prox_l1_box(double* out_host, const double* x_host, double tau, double lo, double hi,
                        int64_t n);
/* out = sum |x_i|   (the l1 value of g, tests/test_proximal_gradient.py:53) */
int zf_host_asum(const double* x_host, int64_t n, double* out);
/* out = d * (x - c) */
int zf_host_diag_grad(double* out_host, const double* x_host, const double* d_dev,
                      const double* c_dev, int64_t n);
/* The Taylor remainder of the squared loss as a ZF_ACCEPT_REMAINDER solver forms it, for caller-supplied margins (host
 * arrays of m doubles): R = scale sum_i (s+_i - s_y,i)^2, s_y = s_k + beta (s_k - s_{k-1}) (nesterov != 0) or s_k.
 * wide = 0: the one-workgroup kernel (dense problems; sparse ones up to 32768 rows); wide = 1: the chunked pair of kernels
 * (sparse problems beyond).  For element-wise tests of those kernels, outside any solve. */
int zf_ls_remainder_eval(const double* s_plus_host, const double* s_k_host, const double* s_km1_host, int64_t m, double beta,
                         int32_t nesterov, double scale, int32_t wide, double* r_out);

/* ---- sparse least squares (ZF_PROBLEM_SPARSE_LS_L1) -------------------------
 * A (m x n) comes as TWO canonical CSR matrices in HBM - A itself and A^T, each with sorted, duplicate-free column
 * indices: int64 row pointers (rows + 1), int32 column indices, float64 values; 24 B per stored element for the pair.
 * Both sweeps of a trial are row sums against a gathered vector (csrc/zf_kernels_spmv.h): s+ = A x+ on the first,
 * grad f(y) = 2 scale A^T r on the second - no atomics, every sum in an order fixed by the matrix and its plan.
 * The device arrays stay the caller's and must outlive the handle; m, n < 2^31; nnz = 0 is legal (indices / values
 * may then be NULL).
 * The plan of one matrix is built by the caller on the host from its row pointers (zfista_amd.sparse.plan_rows):
 * `lanes` lanes walk a row (a power of two, 4 .. 64, from the mean row length); rows LONGER than `threshold` elements
 * are cut into segments of `threshold` elements (the last one shorter) summed by a wave each, and added per row in
 * segment order.  split_row (nsplit, increasing), split_first (nsplit + 1: the first segment of each split row, ending
 * with nseg) and seg_start (nseg: the first element of each segment) are HOST arrays.  zf_spmat_create copies the row
 * pointers to the host once and checks the plan against them - split_row must list exactly the rows longer than
 * `threshold`, the segments of a row must start with the row, lie `threshold` apart and cover it - returns ZF_ERR_ARG for
 * a plan that does not fit, and keeps device copies.  plan_bytes = sizeof(zf_spmv_plan).
 * The handle is immutable once created: any number of solvers and zf_margins_* calls may use it at the same time, on any
 * streams (the segment sums of split rows belong to each solver / each call). */
typedef struct zf_spmv_plan {
    int32_t lanes;
    int32_t reserved;
    int64_t threshold;
    int64_t nsplit;
    int64_t nseg;
    const int64_t* split_row;
    const int64_t* split_first;
    const int64_t* seg_start;
} zf_spmv_plan;
typedef struct zf_spmat zf_spmat; /* opaque */
int zf_spmat_create(zf_spmat** out, int64_t m, int64_t n, int64_t nnz, const int64_t* indptr_dev, const int32_t* indices_dev,
                    const double* values_dev, const zf_spmv_plan* plan, const int64_t* t_indptr_dev, const int32_t* t_indices_dev,
                    const double* t_values_dev, const zf_spmv_plan* t_plan, int64_t plan_bytes);
int zf_spmat_destroy(zf_spmat* h);
/* zf_solver_create for ZF_PROBLEM_SPARSE_LS_L1 and ZF_PROBLEM_SPARSE_LOGISTIC_L1: desc->kind = 4 or 6, A = NULL, b (dev, m), m_rows = m and n as the handle's,
 * scale, lam and the box as for the dense kind, world = 1.  The handle must outlive the solver.  Everything else - init,
 * steps, poll, restore, history - is the solver's as for every kind. */
int zf_solver_create_sparse(zf_solver** out, const zf_problem_desc* desc, const zf_spmat* h, const zf_options* opt, void* stream);

/* ---- K responses on one CSR matrix, on the two sparse kinds 4, 6 (csrc/zf_kernels_spmm.h) -------------------------------------------
 * The problem of zf_solver_set_responses - X in R^{n x K}, B in R^{m x K}, the margins problem of A (x) I_K on vectors flattened in C
 * order, x[j K + k] = X[j][k] - with A behind a zf_spmat handle.  Row i K + k of A (x) I_K holds the elements of row i of A, in the same
 * order, at columns j K + k: the K values a stored element needs are K 8 contiguous bytes, so one index, one value and one gathered
 * line serve K responses.  The two sweeps sum response k exactly as the plain sweeps sum a vector (the same lanes per row, the same
 * element order per lane, two roundings per element, one shuffle tree, the handle's segments for long rows): every value a solve or
 * an evaluation produces is bit-equal to the plain sparse kind on the stored Kronecker matrix.  The handle is used as it is - no new
 * plan, no upload - and stays immutable; a solver's or an evaluation's own segment sums hold nseg K doubles.  No LDS, no atomics:
 * equal columns of the input give bit-equal columns of the output; a non-finite value in one column leaves the bits of the others.
 * Everything element-wise around the sweeps runs unchanged on m K and n K entries (beyond 32768 rows of m K the unweighted squared
 * loss forms its residuals with up to 1024 workgroups, as the sparse kind does by its row count).  Additive to ABI 6.
 * zf_solver_create_sparse_responses: zf_solver_create_sparse with desc->m_rows = K h->m, desc->n = K h->n, desc->b of m K values.
 * ZF_ERR_ARG: K outside 2 .. 16, dimensions that are not K times the handle's, a kind other than 4 / 6, world > 1,
 * ZF_ACCEPT_REMAINDER / ZF_ACCEPT_RESOLVED.  Such a solver has the option "responses" of the options table below (m K row weights,
 * n K penalty factors).  zf_solver_create_sparse keeps its dimension check and zf_solver_set_responses keeps refusing the sparse
 * kinds: K is set at creation or never.  A solver not created here launches and
 * allocates what it did.  Vectors of n K >= 2^31 entries are indexed in 64 bits (n < 2^31, n K is not). */
int zf_solver_create_sparse_responses(zf_solver** out, const zf_problem_desc* desc, const zf_spmat* h, int32_t K, const zf_options* opt,
                                      void* stream);
/* One sweep alone, for element-wise tests of those kernels, outside any solve: out_host = out_scale * A in_host (transpose == 0: in
 * n K, out m K doubles) or out_scale * A^T in_host (in m K, out n K), response-interleaved.  K = 1 runs the plain sweep
 * (zf_launch_spmv), K = 2 .. 16 the K-response one (zf_launch_spmm).  ZF_ERR_ARG: a NULL argument, K outside 1 .. 16. */
int zf_spmat_mr_apply(const zf_spmat* h, int32_t transpose, int32_t K, double out_scale, const double* in_host, double* out_host);

/* ---- duality gap at x_k of a live solver (csrc/zf_kernels_gap.h) ---------------------------------------------------------------
 * The values of zf_margins_gap (below: the certificate, loss by loss) at the current x_k of a live solver of kind 2, 4, 5 or 6, on
 * the solver's stream (synchronises it).
 * The margins A x_k are the solver's own (its margin ring: no sweep over A); one sweep over A^T forms g.  The workspace (one
 * m-vector, one n-vector, chunk results) is allocated by the first call: a solve that never asks launches and allocates
 * nothing more than before.  r, the gradient, the trial's scalars and the control block are not touched - the call may come
 * at any point between two zf_solver_enqueue_steps, also between a rejected trial and its retry, and the solve continues bit
 * for bit.  ZF_ERR_ARG: count < 8, another problem kind, world > 1, a finite box (the dual of the boxed problem is another
 * one).  ZF_ERR_STATE: not initialised. */
int zf_solver_duality_gap(zf_solver* s, double* out, int64_t count /* >= 8 */);

/* ---- the options of a margins solver: which of the eight zf_solver_set_* entries exist together -----------------------------------
 * The sections below say what each option computes.  All eight are called after zf_solver_create(_sparse, _sparse_responses) and
 * before zf_solver_enqueue_init / zf_solver_restore: ZF_ERR_STATE afterwards (zf_solver_set_matrix_f32: ZF_ERR_ARG).  Every other
 * refusal is ZF_ERR_ARG: a NULL solver or pointer, world > 1, a bad argument (its section), and what the three tables refuse.  A
 * refused call leaves the solver as it was, and zf_last_error names the entry and - for a pair - the option already present.  One
 * record and one rule table hold all of this (csrc/zf_solver_options.h); a resumed solve sets its options again before
 * zf_solver_restore (a snapshot carries none of them).  Every option but an explicit l2 = 0 takes a matrix small enough for the
 * two fused small-matrix launches to the general path, for good, and zf_solver_ls_plan says so.
 *
 * options by kinds (+: admitted; kinds 1 and 3 admit none)
 *                      2 least squares  4 sparse LS  5 logistic  6 sparse logistic
 *   l2                 +                +            +           +
 *   penalty_factors    +                +            +           +
 *   huber              +                +            .           .
 *   poisson            +                +            .           .
 *   multinomial        +                +            .           .
 *   row_weights        +                +            +           +
 *   matrix_f32         +                .            +           .
 *   responses          +                .            +           .            (sparse: K comes from zf_solver_create_sparse_responses)
 *
 * options by accept modes (x: refused; ZF_ACCEPT_RESOLVED exists for kind 1 only, which admits no option)
 *                      ZF_ACCEPT_REFERENCE  ZF_ACCEPT_REMAINDER
 *   l2                 +                    +
 *   penalty_factors    +                    +          (both touch g only)
 *   huber              +                    x          (scale |A (x+ - y)|^2 is the Taylor remainder of the squared loss alone)
 *   poisson            +                    x
 *   multinomial        +                    x
 *   row_weights        +                    x          (the residual kernels that form the remainder carry no weights)
 *   matrix_f32         +                    +
 *   responses          +                    x
 *
 * options by options (x: refused together, in either call order; +: compose, in any order; o: compose in ONE order; diagonal: a second call - 2 replaces the value, x is refused)
 *                      l2  penalty_factors  huber  poisson  multinomial  row_weights  matrix_f32  responses
 *   l2                 2   x                +      +        +            +            +           +
 *   penalty_factors    x   2                +      +        +            +            +           +
 *   huber              +   +                2      x        x            +            +           x
 *   poisson            +   +                x      2        x            +            +           x
 *   multinomial        +   +                x      x        x            +            x           o
 *   row_weights        +   +                +      +        +            2            +           +
 *   matrix_f32         +   +                +      +        x            +            2           x
 *   responses          +   +                x      x        o            +            x           x
 *
 * l2 x penalty_factors: the ridge term would need the factors too (not built); l2 = 0 is "not set" and is accepted beside them.
 * One loss per solver.  The K-response sweeps read an fp64 A and carry the square, the logistic and the multinomial loss.
 * The one ordering rule (o): zf_solver_set_multinomial needs the K >= 2 responses already there - a dense solver calls
 * zf_solver_set_responses BEFORE it, a sparse one comes from zf_solver_create_sparse_responses - so it is refused on a matrix
 * stored in fp32 and, like the responses, cannot be called twice. */

/* ---- elastic net: g(x) = lam |x|_1 + (l2 / 2) |x|^2 (+ box) for the margins kinds 2, 4, 5, 6 ------------------------------
 * Additive to ABI 6: no struct field, no version change.  prox_{w g}(v) = clip(soft_threshold(v, lam w) * shrink, lo, hi) with
 * shrink = 1 / (1 + l2 w) formed once per trial as a scalar; the element is multiplied by it (no division per element), the
 * iterate arithmetic stays uncontracted: x+ is that expression bit for bit.  The clip behind the shrink is the exact prox.
 * zf_solver_set_l2 (when, and with what: the options table above).  ZF_ERR_ARG of its own: l2 < 0 or not finite.  With l2 > 0 every
 * trial runs the elastic-net step kernel (zf_trial_enet_kernel: the general vector path), F(x0) includes the ridge term, and
 * zf_solver_duality_gap evaluates the ridge form of the certificate (zf_margins_gap).  l2 = 0 changes nothing: the launches,
 * allocations and bits of a solver that was never asked. */
int zf_solver_set_l2(zf_solver* s, double l2);
/* out = clip(soft_threshold(x, tau) * shrink, lo, hi) at a host vector: the elastic-net prox with tau = lam w and the caller's
 * scalar shrink = 1 / (1 + l2 w) */
int zf_host_prox_enet_box(double* out_host, const double* x_host, double tau, double shrink, double lo, double hi, int64_t n);
/* out = sum_i (lam |x_i| + (l2 / 2) x_i^2), each term two fused multiply-adds into the running sum (as the step kernel forms g(x+)) */
int zf_host_enet_g(const double* x_host, int64_t n, double lam, double l2, double* out);

/* ---- gap-safe screening and column restriction (csrc/zf_kernels_screen.h) ------------------------------------------------
 * phi_i' is L-Lipschitz (least squares L = 2 scale, logistic L = scale / 4), so the dual optimum lies within r = sqrt(2 L gap)
 * of the dual point of a gap evaluation, and column j is zero at every optimum when alpha |g_j| + r |a_j|_2 < lam.  In fp64
 * the radius is widened to r_eff = r + E, E |a_j| a bound of the rounding of the left side (derived in zf_kernels_screen.h).
 * All kernels: fp64, no atomics, every sum and every output order fixed by the matrix and the mask alone.
 * Column norms: norms_dev (n doubles) = |a_j|_2, stats_dev (2 doubles) = [sum_j |a_j|^2, max_j |a_j|]; sparse: row sums of squares
 * over the stored A^T with its plan; dense: row-major A (m_rows x n).  An empty column has norm 0 exactly. */
int zf_spmat_col_norms(const zf_spmat* h, double* norms_dev, double* stats_dev);
int zf_dense_col_norms(const double* A_dev, int64_t m_rows, int64_t n, double* norms_dev, double* stats_dev);
/* index_dev (n int32) = the exclusive scan of a caller's mask keep_dev (n bytes, non-zero = kept), *count_out = the kept count:
 * one workgroup up to 4096 elements, contiguous chunks combined in chunk order beyond. */
int zf_screen_scan(const uint8_t* keep_dev, int64_t n, int32_t* index_dev, int64_t* count_out);
/* The restriction of a matrix handle to its kept columns, in two calls around the caller's scans of the lengths.
 * zf_spmat_restrict_count: index_dev (n) = the scan of keep_dev, *count_out = k; len_dev (m int64) = the kept elements of every row
 * of A; t_len_dev[c] (c < k; room for n) = the length of the c-th kept row of A^T; seg_off_dev (int32, one per segment of A's plan;
 * may be NULL without split rows) = where the kept elements of a segment start inside their row.
 * zf_spmat_restrict_fill: with indptr_dev (m + 1) and t_indptr_dev (k + 1) the exclusive scans of those lengths, both ending at
 * nnz_new (checked), writes the canonical CSR of A[:, keep] - every row's kept elements in stored order, columns renumbered -
 * and of its transpose (the kept rows of A^T, whole).  keep, index and seg_off must be those of the count call. */
int zf_spmat_restrict_count(const zf_spmat* h, const uint8_t* keep_dev, int32_t* index_dev, int64_t* len_dev, int64_t* t_len_dev,
                            int32_t* seg_off_dev, int64_t* count_out);
int zf_spmat_restrict_fill(const zf_spmat* h, const uint8_t* keep_dev, const int32_t* index_dev, const int32_t* seg_off_dev, int64_t k,
                           int64_t nnz_new, const int64_t* indptr_dev, int32_t* indices_dev, double* values_dev,
                           const int64_t* t_indptr_dev, int32_t* t_indices_dev, double* t_values_dev);
/* out_dev (m_rows x k, row-major) = A[:, keep]; index_dev (n): scratch for the scan of keep_dev; k must be the kept count (>= 1). */
int zf_dense_restrict(const double* A_dev, int64_t m_rows, int64_t n, const uint8_t* keep_dev, int32_t* index_dev, int64_t k,
                      double* out_dev);

/* ---- Huber's loss on the least-squares kinds 2 and 4 (csrc/zf_kernels_loss.h) -------------------------------------------
 * f(x) = scale sum_i H(r_i), r = A x - b, H(r) = r^2 for |r| <= delta and delta (2 |r| - delta) beyond (scale = 1/2: the textbook
 * function); grad f = 2 scale A^T c, c = clip(r, -delta, delta).  Every kernel forms c = copysign(min(|r|, delta), r) - exact
 * given r - and H = c (2 r - c): two roundings, never negative, r r on an unclipped row.  The sum is a plain sum.  A NaN margin
 * gives a NaN f.  Additive to ABI 6: no problem kind, no struct field, no version change.
 * zf_solver_set_huber (when, and with what: the options table above).  ZF_ERR_ARG of its own: delta not finite or <= 0.  A trial
 * then runs the loss kernels where it ran the residual kernels - at y (c to the residual buffer, f(y)) and at x+ (f(x+)); the A^T
 * sweep (with the same 2 scale), the prox step, the decision, history and snapshots are the least-squares kinds' own.  A solver
 * that was never asked launches and allocates what it did. */
int zf_solver_set_huber(zf_solver* s, double delta);

/* ---- per-row sample weights on the four margins kinds 2, 4, 5, 6 (csrc/zf_kernels_loss.h) -----------------------------------
 * f(x) = scale sum_i w_i phi_i(z_i) - a weighted SUM, not a mean; the weights are used as given - and
 * grad f = gfac A^T (w o psi(z)), gfac = 2 scale (square, Huber) | scale (logistic), phi and psi per row as the unweighted
 * kernels form them, then one product for each output: rho_i = w_i psi_i, acc += w_i phi_i (two roundings per row).  The sum is a
 * plain sum times scale (the sqrt()^2 of the unweighted squared loss is not used).  A row with w_i == 0 is a row that is not
 * there: rho_i = +0 and its term +0 whatever b_i holds, NaN and Inf included.  No guarantee for non-finite entries of A.
 * w_dev: m_rows doubles in device memory, finite and >= 0 with at least one > 0 (the caller's check: the library does not read
 * them on the host).  Additive to ABI 6: no problem kind, no struct field, no version change. */
enum { ZF_LOSS_SQUARE = 0, ZF_LOSS_LOGISTIC = 1, ZF_LOSS_HUBER = 2 };
/* zf_solver_set_row_weights (when, and with what: the options table above).  The pointer is borrowed, as b is.  The three loss
 * sites of a trial, f of the initial point and zf_solver_duality_gap then take the weighted kernels; the two sweeps, the prox
 * step, the decision, history and snapshots stay as they are.  A solver that was never asked launches and allocates what it did. */
int zf_solver_set_row_weights(zf_solver* s, const double* w_dev);

/* ---- the Poisson loss with a log link on the least-squares kinds 2 and 4 (csrc/zf_kernels_loss.h) ------------------------
 * f(x) = scale sum_i w_i (exp(z_i) - b_i z_i), z = A x, with counts b_i >= 0, finite, not necessarily integers (a rate
 * count / exposure with the exposure as the row weight is the exposure model); the constant log b! is dropped.
 * grad f = scale A^T (w o psi), psi_i = exp(z_i) - b_i.  Every kernel forms ONE e = exp(z) per row, psi = e - b and
 * phi = e - b z (two roundings); the sum is a plain sum times scale.  A margin beyond the range of exp gives f = +inf, never NaN:
 * the acceptance test rejects such a trial and the line search backtracks.  A NaN margin gives a NaN f.  The library does not
 * read b on the host: b >= 0 is the caller's check.  Additive to ABI 6: no problem kind, no struct field, no version change.
 * zf_solver_set_poisson (when, and with what: the options table above).  A trial then runs the loss kernels where it ran the
 * residual kernels - at y (psi to the residual buffer, f(y)) and at x+ (f(x+)); the A^T sweep runs with `scale` for `2 scale`;
 * the prox step, the decision, history and snapshots are the least-squares kinds' own.  A solver that was never asked launches
 * and allocates what it did. */
enum { ZF_LOSS_POISSON = 3 };   /* the fourth ZF_LOSS_* code (struct zf_loss of csrc/zf_loss_dispatch.h) */
int zf_solver_set_poisson(zf_solver* s);

/* ---- per-column penalty factors on the four margins kinds 2, 4, 5, 6 --------------------------------------------------------
 * g(x) = lam sum_j p_j |x_j| (+ box), p_j >= 0: p_j = 0 leaves column j unpenalised (an intercept: a column of ones with p = 0).
 * Additive to ABI 6: no struct field, no version change.  p_dev: n doubles in device memory, 16-byte aligned, borrowed as b is
 * (it must outlive the solver); its values are the caller's responsibility (finite, >= 0; > 0 for the certificate).
 * prox_{w g}(v)_j = clip(soft_threshold(v_j, (lam w) p_j), lo, hi): t = lam w once per trial, tau_j = t * p_j per element, the
 * fourth running sum takes fma(p_j, |x+_j|, sum) and keeps its scale lam (zf_trial_pf_kernel; 8 n bytes more per trial).  p = 1
 * gives the iterates and packs of a solver that was never asked, bit for bit; p_j = 0 gives x+_j = v_j exactly.
 * zf_solver_set_penalty_factors (when, and with what: the options table above).  ZF_ERR_ARG of its own: a misaligned pointer.
 * Every trial then runs the general vector path. */
int zf_solver_set_penalty_factors(zf_solver* s, const double* p_dev);
/* out = clip(sign(x) * max(|x| - t * p, 0), lo, hi) at host vectors, NumPy's expression operation by operation */
int zf_host_prox_pf_box(double* out_host, const double* x_host, const double* p_host, double t, double lo, double hi, int64_t n);
/* out = lam * sum_i p_i |x_i|, each term one fused multiply-add into the running sum (as the step kernel forms it) */
int zf_host_pf_g(const double* x_host, const double* p_host, int64_t n, double lam, double* out);

/* ---- a dense matrix stored in fp32 on the two dense kinds 2, 5 -----------------------------------------------------------------
 * Both sweeps of a trial stream A and nothing else of size, so storing A in fp32 halves their bytes and the footprint of A.
 * Every other value stays double: x, r, the accumulators, the outputs; an element is widened in a register, exactly.  The solver
 * therefore solves, in fp64 arithmetic, exactly the fp64 problem on float64(A32) - with sums in another order than the fp64 sweeps
 * take (csrc/zf_kernels_gemv_f32.h).  Additive to ABI 6: no struct field, no version change.
 * zf_solver_set_matrix_f32: after zf_solver_create, before zf_solver_enqueue_init / zf_solver_restore.  A32_dev: m_rows x n floats,
 * row-major, device memory, 16-byte aligned, borrowed as desc->A is.  zf_solver_create still wants a non-NULL, 16-byte-aligned
 * desc->A (the same address will do); after this call nothing reads it.  From then on every sweep of the solver - the trial's two,
 * the initial evaluation, zf_solver_duality_gap - takes the fp32 kernels, the slices are those of the fp32 rule (panels of
 * 256 * V columns, V = 4 / 2 / 1 for n % 4 == 0 / n % 4 == 2 / odd n; at most 64 slices of at least 8 rows), a matrix small enough
 * for the two fused small-matrix launches takes the general path, ZF_GEMV_MFMA has no effect, and zf_solver_ls_plan says so.
 * When, and with what: the options table above.  ZF_ERR_ARG of its own: a misaligned pointer, and - where the other seven answer
 * ZF_ERR_STATE - a solver that is already initialised.  A solver that was never asked launches and allocates what it did. */
int zf_solver_set_matrix_f32(zf_solver* s, const float* A32_dev);

/* ---- K responses on one dense matrix, on the two dense kinds 2, 5 ---------------------------------------------------------------
 * X in R^{n x K}, B in R^{m x K}: f(X) = scale sum_k sum_i W_ik phi((A x_k)_i ; B_ik), g(X) = lam sum_jk P_jk |X_jk| (+ the ridge term,
 * + a box) is the margins problem of the matrix A (x) I_K on vectors flattened in C order: x[j K + k] = X[j][k], b[i K + k] = B[i][k].
 * Everything element-wise around the two sweeps runs unchanged on m K and n K entries; the sweeps (csrc/zf_kernels_mr.h) multiply A
 * into K columns and read A once, so K solves cost one solve's bytes.  Additive to ABI 6: no struct field, no version change.
 * zf_solver_set_responses: after zf_solver_create, before zf_solver_enqueue_init / zf_solver_restore.  The solver was created with
 * desc->m_rows = m K, desc->n = n K, desc->A the m x n matrix, desc->b the m K targets (labels +-1 for the logistic kind).  From then
 * on every sweep of the solver - the trial's two, the initial evaluation and zf_solver_restore, zf_solver_duality_gap - takes the
 * K-response kernels, the slices are those of the rule on m x n, the unweighted squared loss forms its residuals with up to 1024
 * workgroups beyond 32768 rows of m K (as the sparse kind does), a matrix small enough for the two fused small-matrix launches takes
 * the general path, ZF_GEMV_MFMA has no effect, and zf_solver_ls_plan says so.
 * When, and with what: the options table above (row weights are m K weights then, penalty factors n K factors).  ZF_ERR_ARG of
 * its own: K outside 2 .. 16, m_rows or n not a multiple of K.  A solver that was never asked launches and allocates what it did. */
int zf_solver_set_responses(zf_solver* s, int32_t K);

/* ---- the multinomial (softmax) loss on K responses, on the least-squares kinds 2 and 4 (csrc/zf_kernels_softmax.h) ---------------
 * Y in R^{m x K} with rows on the probability simplex (a one-hot row is a class label), X in R^{n x K}, flattened as above:
 *     f(X) = scale sum_i w_i [logsumexp(z_i) - <y_i, z_i>],  z_i = (A X)_i in R^K,   grad f = scale A^T (w o (softmax(Z) - Y)).
 * The one loss that couples the K margins of a row; penalty, prox step, decision, history, snapshots and both K-response sweeps are
 * the K-response solver's own.  One row, in every kernel: mx = max_k z_k, d_k = z_k - mx, e_k = exp(d_k), S = sum_k e_k (k order),
 * rS = 1 / S (one division), p_k = e_k rS, psi_k = p_k - y_k, phi = log S + sum_k y_k (-d_k) (every term >= 0; equal to
 * logsumexp - <y, z> because sum_k y_k = 1: the caller's check, the library does not read Y on the host).  Nothing overflows for a
 * finite margin; a NaN or +inf margin gives a NaN f, and so does a -inf margin on a class with y_k = 0 (0 * inf); a -inf margin on a
 * class with y_k > 0 gives f = +inf (phi = y_k * inf), which the acceptance test rejects.
 * Row weights stay one double per FLATTENED entry (m K of them, zf_solver_set_row_weights as before) so that neither the ABI nor
 * the snapshot format changes, but a row of this loss has ONE weight: the kernels read w[i K] alone - the caller repeats w_i K
 * times - and w_i == 0 is a row that is not there, whatever y_i holds.
 * zf_solver_set_multinomial (when, and with what: the options table above, and its ordering rule).  ZF_ERR_ARG of its own: b (the
 * rows of Y) not 16-byte aligned.  A solver that was never asked launches and allocates what it did.  Additive to ABI 7: one
 * enumerator, one entry, no struct change. */
enum { ZF_LOSS_MULTINOMIAL = 4 };   /* the fifth ZF_LOSS_* code */
int zf_solver_set_multinomial(zf_solver* s);

/* ---- the margins problems at a host point: f / grad, the certificate, the screen (ABI 7) --------------------------------------------
 * One descriptor names the storage of A, the loss and the options of the problem
 *     f(x) = scale sum_i w_i phi((A x)_i ; b_i),   g(x) = lam sum_j p_j |x_j| + (l2 / 2) |x|^2
 * and three entries evaluate it at a point given in host memory (problem data stays in HBM), on the rows kernels and the sweeps a
 * solver of that storage and loss runs.  These back f, jac_f, duality_gap and screen of zfista_amd.problems.*.  A new loss or a new
 * storage is a new value of a field: no entry is added.  (They replace the 32 per-loss entries of ABI 6: INTEGRATION.md lists them.)
 * Exactly one of A / A32 / spmat is set.  Dense: m_rows x n row-major in device memory, 16-byte aligned; a handle knows its own
 * sizes and m_rows, n are ignored.  K responses (1 .. 16; K > 1: ZF_LOSS_SQUARE / ZF_LOSS_LOGISTIC / ZF_LOSS_MULTINOMIAL on A or spmat
 * only; ZF_LOSS_MULTINOMIAL needs K >= 2, b holds the rows of Y and w one weight per row repeated K times): m_rows and n
 * stay the MATRIX's, b / w hold m_rows K, p / x_host / grad_out_host n K doubles, response-interleaved (x[j K + k] = X[j][k]); K = 1
 * is the plain problem.  w (row weights, finite and >= 0) and p (penalty factors, > 0) may each be NULL: the unweighted / unfactored
 * problem - other kernels, other bits than w = 1.  delta: Huber's, finite and > 0; ignored for the other losses. */
typedef struct zf_eval_desc {
    const double* A;          /* dev: dense fp64 matrix, or NULL                                       */
    const float* A32;         /* dev: dense matrix stored in fp32 (zf_solver_set_matrix_f32), or NULL  */
    const zf_spmat* spmat;    /* CSR handle (zf_spmat_create), or NULL                                 */
    int64_t m_rows, n;        /* dense: the matrix's sizes                                             */
    const double* b;          /* dev, m_rows K: targets / labels +-1 / counts                          */
    const double* w;          /* dev, m_rows K, or NULL                                                */
    const double* p;          /* dev, n K, or NULL (the certificate only)                              */
    double scale, lam, l2, delta;
    int32_t loss;             /* ZF_LOSS_SQUARE / _LOGISTIC / _HUBER / _POISSON / _MULTINOMIAL         */
    int32_t K;
} zf_eval_desc;
int64_t zf_sizeof_eval_desc(void);
/* ZF_ERR_ARG from all three, before anything touches a device or is written: d NULL or desc_bytes != zf_sizeof_eval_desc(); not exactly
 * one matrix; b, x_host or the output pointer NULL; dense m_rows or n < 1, a misaligned matrix; an unknown loss; a bad delta with
 * ZF_LOSS_HUBER; K outside 1 .. 16, K > 1 with another loss than square / logistic / multinomial or with A32; ZF_LOSS_MULTINOMIAL
 * with K = 1 or with A32.
 *
 * zf_margins_eval: *f_out = f(x) and (grad_out_host != NULL) grad f(x) = gfac A^T (w o psi(A x)), gfac = 2 scale (square, Huber) |
 * scale (logistic, Poisson).  Reads neither lam, l2 nor p.  The column sweep of a dense fp64 A is always the VALU one: jac_f has the
 * same bits whatever n % 32 is.  Per loss (z = A x):
 *   square    phi = (z - b)^2 (tests/test_proximal_gradient.py:49-57); unweighted: f from the residual kernels, sqrt(sum)^2
 *   logistic  phi = softplus(-b z), psi = -b sigma(-b z), b = +-1.  Finite for every finite margin: one exp(-|t|) per row feeds
 *             softplus(t) = max(t, 0) + log1p(e) and sigma(t) = t >= 0 ? 1 / (1 + e) : e / (1 + e)
 *   Huber     phi = H(r), psi = c = clip(r, -delta, delta), r = z - b (the section of zf_solver_set_huber)
 *   Poisson   phi = exp(z) - b z, psi = exp(z) - b (the section of zf_solver_set_poisson)
 *   multinomial  per row of K margins: phi = log S + sum_k y_k (mx - z_k), psi_k = e_k / S - y_k; gfac = scale (the section of
 *             zf_solver_set_multinomial)
 * weighted: rho_i = w_i psi_i, acc += w_i phi_i (the section of zf_solver_set_row_weights). */
int zf_margins_eval(const zf_eval_desc* d, int64_t desc_bytes, const double* x_host, double* f_out, double* grad_out_host /* or NULL */);

/* zf_margins_gap: the duality-gap certificate (csrc/zf_kernels_gap.h).
 * P(x) = sum_i phi_i((A x)_i) + lam |x|_1.  Dual point nu = alpha grad phi(A x), alpha = min(1, lam / |g|_inf) (1 when g = 0),
 * g = grad f(x) = A^T grad phi(A x): |A^T nu|_inf <= lam, D = -sum_i phi_i^*(nu_i) <= min P.  The reference has no such certificate;
 * its stopping test |x+ - y|_inf < tol measures the step.
 * out (count >= 8 doubles) = [P, D, gap, alpha, |g|_inf, f(x), lam |x|_1, rows gap].  `gap` is NOT P - D (a difference of two
 * numbers of the size of F) but the sum of the two Fenchel-Young gaps, every term >= 0:
 *   rows     per loss, below
 *   columns  sum_j (lam |x_j| + alpha g_j x_j), term by term
 * with 1 - alpha = max(0, (|g|_inf - lam) / |g|_inf).  Finite for every finite margin; alpha = 1 gives a rows gap of exactly 0;
 * a NaN or +-inf in x or g gives a NaN gap.  No atomics, every sum in an order fixed by m or n alone.  g by the column sweep a solver
 * of this shape runs (dense fp64, K = 1: MFMA when n % 32 == 0 and ZF_GEMV_MFMA is not 0).  zf_solver_duality_gap of a solver with
 * the same storage, loss and options writes the same values, bit for bit.
 * ZF_ERR_ARG also: count < 8; scale not > 0, lam < 0, l2 negative or not finite; p together with l2 > 0.
 *
 * Square.  rows = scale (1 - alpha)^2 |A x - b|^2.
 * Logistic.  rows = scale sum_i KL(alpha q_i || q_i), q_i = sigma(-b_i (A x)_i); the row terms depend on alpha: a second rows pass
 * follows the n-passes.
 * Huber.  phi_i^*(nu) = nu b_i + nu^2 / (4 scale) on |nu| <= 2 scale delta, and nu = alpha 2 scale c never leaves that interval.  One
 * rows pass stores c and returns sum H, sum c^2, sum b c and T = sum |c| (|r| - |c|) (every term >= 0, exactly 0 on an unclipped
 * row); none depends on alpha:
 *   P = scale sum H + lam |x|_1                    D = -scale (alpha^2 sum c^2 + 2 alpha sum b c)
 *   rows = scale (1 - alpha) ((1 - alpha) sum c^2 + 2 T)
 * delta >= max |r| gives the least-squares rows gap scale (1 - alpha)^2 |r|^2.
 * Poisson.  h(z) = e^z - b z has h^*(u) = v log v - v, v = u + b >= 0 (0 log 0 = 0); with nu = alpha grad phi(z),
 * v = alpha e^z + (1 - alpha) b >= 0 always.
 *   P = f + lam |x|_1                                D = -scale sum w (v log v - v)
 *   rows = scale sum w [e^z - v + v (log v - z)]     every term >= 0, exactly 0 at alpha = 1
 * The row terms depend on alpha: a second rows pass follows the n-passes, as for the logistic loss.
 * Multinomial.  The conjugate of logsumexp(z) - <y, z> at theta is sum_k v_k log v_k with v = theta + y on the simplex; theta = alpha psi
 * gives v = alpha p + (1 - alpha) y, a convex combination: feasible for every alpha in [0, 1].
 *   D = -scale sum_i w_i sum_k v_ik log v_ik (0 log 0 = 0)     rows = scale sum_i w_i KL(v_i || p_i), log p_k = d_k - log S
 * each row term clamped at 0, not formed at alpha = 1, finite for every finite margin; the composition is the logistic one.
 * Row weights (w).  Every row term times w_i ((w phi)^*(w u) = w phi^*(u); the dual point is nu = alpha grad phi(z) as before):
 * square sum w r^2, sum w b r; Huber sum w H, sum w c^2, sum w b c, sum w |c| (|r| - |c|); logistic sum w KL,
 * sum w [p log p + (1 - p) log(1 - p)].  The n-passes and the compositions are unchanged.
 * Ridge (l2 > 0).  The ridge term is n more rows phi(t) = (l2 / 2) t^2 at z = x.  gt = grad f(x) + l2 x = fma(l2, x, g),
 * alpha = min(1, lam / |gt|_inf) (1 when gt = 0), 1 - alpha and alpha log alpha as above;
 *   P = f + lam |x|_1 + (l2 / 2) sum x^2          D = D_loss(alpha) - (l2 / 2) alpha^2 sum x^2
 *   ridge = (l2 / 2) (1 - alpha)^2 sum x^2        columns = sum_j (lam |x_j| + alpha gt_j x_j), term by term, clamped at 0
 *   gap = rows + ridge + columns                  (rows: the loss part, as above)
 * out = the eight values above with |gt|_inf in [4]; count >= 10: [8] = (l2 / 2) sum x^2, [9] = the ridge part of the gap.
 * The |.|_inf pass forms gt on the fly from g and x (16 n bytes).  l2 = 0 runs the l1 evaluation (the same kernels, the same eight
 * values) and writes [8] = [9] = 0 into a buffer of ten.  zf_solver_duality_gap of a solver with l2 > 0 writes the same ten values
 * (count >= 10; the first eight otherwise); of any other solver the eight it wrote before, whatever count.
 * Penalty factors (p > 0, l2 = 0).  The dual constraint is |a_j^T theta| <= lam p_j.  With g'_j = g_j / p_j and x'_j = x_j p_j every
 * quantity is that of the unfactored evaluation of this loss at (g', x'): one n-pass writes g' and x' (an IEEE division and a
 * multiplication per element) between g = grad f(x) and the tails, which run unchanged.  out: the eight slots with
 * [4] = max_j |g_j| / p_j and [6] = lam sum p_j |x_j| = g(x).  A p_j = 0 divides by zero: the dual candidate cannot be made feasible
 * by scaling (it needs a_j^T theta = 0 exactly), and the callers above this level refuse.
 * K responses.  The evaluation of the m_rows K x n K problem: one alpha scales the dual candidate of all K responses, so it is
 * feasible for each of them and the gap is a sum of K non-negative gaps. */
int zf_margins_gap(const zf_eval_desc* d, int64_t desc_bytes, const double* x_host, double* out, int64_t count /* >= 8; 10 for all */);

/* zf_margins_screen: zf_margins_gap - the same kernels in the same order, out[0 .. 8) the same bits - followed by the gap-safe screen
 * of the call's g (the section "gap-safe screening" above): keep_dev (n bytes) = !(alpha |g_j| + r_eff |a_j| < lam), index_dev (n
 * int32) = the exclusive scan of keep (the new column number of a kept column), out[8 .. 12) = [r, E, r_eff, kept count].  A
 * non-finite gap, alpha or g_j keeps everything.  norms_dev / stats_dev as the norms calls left them; max_row / max_col: the stored
 * elements of the longest row / column of A, read for a handle only (dense: n and m_rows, taken from the sizes).
 * Huber's loss: the rule with L = 2 scale and the guard with c for r, |c|_2 = sqrt(sum c^2) - the clip is exact and 1-Lipschitz.  The
 * radius, mask, scan and restriction kernels are the same.
 * ZF_ERR_ARG also, each with a message of its own: count < 12; ZF_LOSS_POISSON (exp is not globally Lipschitz, so the gap-safe radius
 * does not apply); ZF_LOSS_MULTINOMIAL (screening needs per-response gaps); w, p, l2 > 0, A32 or K > 1 (the rule and its rounding guard are not built for them); dense n > 2^31 - 1; norms_dev,
 * stats_dev, keep_dev or index_dev NULL; a handle with max_row or max_col < 0. */
int zf_margins_screen(const zf_eval_desc* d, int64_t desc_bytes, const double* x_host, double* out, int64_t count /* >= 12 */,
                      const double* norms_dev, const double* stats_dev, int64_t max_row, int64_t max_col, uint8_t* keep_dev,
                      int32_t* index_dev);

/* ---- multi-objective trial (m >= 2), device side ---------------------------
 * The dual of the scalarised subproblem is minimised on the host by SciPy exactly
 * as the reference does (proximal_gradient.py:179-205); every O(n) expression runs
 * on the GPU with x_k, x_{k-1}, y, x+ and J (m x n) resident in HBM.  g / prox are
 * the shifted-l1 + box family of zfista/problems.py:101-138. */
#define ZF_MO_GENERIC 0 /* f, jac_f are host callbacks; J is uploaded per trial     */
#define ZF_MO_JOS1 1    /* zfista/problems.py:193-205  (m = 2)                      */
#define ZF_MO_FDS 2     /* zfista/problems.py:309-328  (m = 3)                      */
typedef struct zf_mo zf_mo;
int zf_mo_create(zf_mo** out, int32_t kind, int32_t m, int64_t n, const double* l1_ratios_host,
                 const double* l1_shifts_host, double box_lo, double box_hi, void* stream);
/* x sharded over ranks in contiguous blocks: this engine holds [offset, offset+n)
 * of n_global features.  `fn` is called synchronously inside every call that reduces (eval_F,
 * prepare, dual_eval, recover, post_terms) with this rank's raw totals and must replace them by
 * the combination over all ranks - sums added in rank order, entry max_index (>= 0) a maximum -
 * so that every rank continues with identical scalars; returns nonzero on failure. */
typedef int (*zf_mo_exchange_fn)(void* ctx, double* vals, int32_t count, int32_t max_index);
int zf_mo_set_shard(zf_mo* s, int64_t n_global, int64_t offset, zf_mo_exchange_fn fn, void* ctx);
/* the same sharding over a communicator of the library instead of a callback: the totals of every reduction are
 * all-gathered on the stream and added in rank order on the device, and zf_mo_solve_dual exchanges once per BATCH
 * of its search (<= m + 1 points: ~3 collectives per trial) instead of once per dual evaluation.  The persistent-kernel
 * search (zf_mo_solve_dual_device / zf_mo_trial_launch) stays single-rank; zf_mo_solve_dual_stream is the device-driven
 * search of a sharded x.  zf_mo_exchange_count: collectives so far. */
int zf_mo_set_comm(zf_mo* s, zf_comm* comm, int64_t n_global, int64_t offset);
int zf_mo_exchange_count(zf_mo* s, int64_t* count);
/* per-coordinate box bounds (host arrays of n) instead of the scalar pair given at creation */
int zf_mo_set_bounds(zf_mo* s, const double* lo_host, const double* hi_host);
int zf_mo_destroy(zf_mo* s);
int zf_mo_set_x0(zf_mo* s, const double* x0_host);              /* :463-465 */
/* point selector `which`: 0 = x_k, 1 = y, 2 = x+ (trial point), 3 = x_{k-1} */
int zf_mo_eval_F(zf_mo* s, int32_t which, double* f_out /* m or NULL */, double* g_out /* m */); /* :279,:295 */
int zf_mo_prepare(zf_mo* s, double* f_y_out /* m */);           /* J = jac_f(y), f(y)   :140,:142 */
/* the same, stream-ordered and without a host round trip (built-in problems, unsharded x): f(y) is
 * formed and kept on the device for zf_mo_solve_dual_device, which hands it back with its result;
 * zf_mo_get_f_y fetches it otherwise (synchronises) */
int zf_mo_prepare_async(zf_mo* s);
/* Fused outer iteration (JOS1 / FDS, unsharded x), on / off: zf_mo_commit and
 * zf_mo_prepare_async only record what is due and the next zf_mo_solve_dual_device forms y = x_k +
 * beta (x_k - x_{k-1}) (:534), f(y) (:140) and J = jac_f(y) (:142) inside its one kernel: one launch and one
 * read-back per trial.  Every other entry point first brings the buffers up to date, so results do not change. */
int zf_mo_set_fused(zf_mo* s, int32_t on);
/* Trials launched AHEAD of their predecessor's result (fused mode; the outer loop :474-538 without the host in its
 * critical path).  zf_mo_trial_launch enqueues one trial (after zf_mo_prepare_async) and returns a ticket;
 * zf_mo_trial_wait returns its result and the acceptance decision (:298-303) the kernel took on F(x+) formed on
 * the device.  A trial launched with gated = 1 - after zf_mo_commit + zf_mo_prepare_async, before the result of
 * the trial before it is known - runs only if that trial was accepted (else it exits at once having touched
 * nothing: *skipped_out = 1; call zf_mo_uncommit, then retry with a smaller step) and takes F(x_k) from that
 * trial's F(x+) on the device (F_old may then be NULL); gated = 2: it also starts its search from that trial's
 * weights (warm_start, :286-288), likewise taken on the device.  At most one trial may be in flight ahead of the
 * one waited for.  *ticket_out = -1: not a device trial (sharded x, m > 8, the grid not co-resident) - use the host loop. */
int zf_mo_trial_launch(zf_mo* s, double lr, const double* F_old /* m or NULL */, int32_t deprecated,
                       const double* w0 /* m or NULL */, double tol, int64_t max_iter, double accept_tol,
                       int32_t decay_is_one, int32_t gated, int32_t* ticket_out);
int zf_mo_trial_wait(zf_mo* s, int32_t ticket, double* w_out, double* fun_out, int64_t* nit_out, int32_t* ok_out,
                     int64_t* evals_out, double* err_out, double* f_x_out, double* g_x_out, double* f_y_out,
                     int32_t* accepted_out, int32_t* skipped_out);
int zf_mo_uncommit(zf_mo* s);   /* undo of zf_mo_commit (+ zf_mo_prepare_async) after a skipped gated trial */
/* The device trial keeps its whole grid spinning on grid-wide hand-overs, so every workgroup must be resident at
 * once.  What the device can hold of the kernel is checked at launch (hipOccupancyMaxActiveBlocksPerMultiprocessor;
 * if it cannot: *ticket_out = -1 / *ok_out = 0, nothing launched).  If other work occupies CUs at run time a wait
 * gives up after ZF_MO_SPIN_LIMIT polls (default 2^24, seconds): the reducer publishes no totals, every workgroup
 * leaves, *ok_out = -1.  Then: zf_mo_trial_wait the trial launched ahead (it was skipped), zf_mo_uncommit,
 * zf_mo_invalidate_prepare (y, f(y), J of that trial are due again) and continue with zf_mo_solve_dual +
 * zf_mo_recover. */
int zf_mo_invalidate_prepare(zf_mo* s, int32_t ticket /* of the trial that gave up; -1: the most recent launch */);
int zf_mo_debug_force_timeout(zf_mo* s, int32_t launches);   /* test hook: the next `launches` device trials give up */
int zf_mo_get_f_y(zf_mo* s, double* f_y_out /* m */);
int zf_mo_set_jac(zf_mo* s, const double* J_host);              /* generic kind         :142 */
/* out[0..m) = g_i(p), out[m] = |p-v|^2, out[m+1] = |w@J|^2, out[m+2..2m+2) = J_i.(p-y)   :162-173 */
int zf_mo_dual_eval(zf_mo* s, double lr, const double* w_host, double* out);
/* H_out (m x m): the generalised Hessian of the dual (:161-177) at w, d jac_i / d w_k on the quadratic piece w sits
 * in - from the derivative of prox_wsum_g through its composed soft-thresholds and the clip (problems.py:126-138);
 * what the device-side search builds its Newton model from instead of finite-difference probes.  m <= 5. */
int zf_mo_dual_hessian(zf_mo* s, double lr, const double* w_host, double* H_out);
/* the whole dual search of one trial inside the library (opt-in replacement of the two SciPy
 * calls :179-205): m = 2 bracketing root finder on the monotone derivative, m >= 3 projected
 * Newton on the simplex; every evaluation is one zf_mo_dual_eval.  *ok_out = 0: not attempted
 * (non-finite start), fall back to the reference's calls. */
int zf_mo_solve_dual(zf_mo* s, double lr, const double* f_y, const double* F_old, int32_t deprecated,
                     const double* w0, double tol, int64_t max_iter, double* w_out, double* fun_out,
                     int64_t* nit_out, int32_t* ok_out, int64_t* evals_out);
/* (ABI 6) the same search for an x SHARDED over a library communicator (zf_mo_set_comm) with the state machine in DEVICE
 * memory: a batch = evaluation kernel -> reduce -> ONE zf_comm_all_gather -> a one-wave kernel that adds the totals in rank
 * order, composes D(w), grad D(w) (:165-177) and advances the machine; batches are enqueued back to back and the host looks
 * once per six of them (zf_mo_solve_dual synchronises with the host once per batch).  What dual_solver="device" runs when x
 * is sharded.  Arguments and results as zf_mo_solve_dual; zf_mo_recover follows. */
int zf_mo_solve_dual_stream(zf_mo* s, double lr, const double* f_y, const double* F_old, int32_t deprecated,
                            const double* w0, double tol, int64_t max_iter, double* w_out, double* fun_out,
                            int64_t* nit_out, int32_t* ok_out, int64_t* evals_out);
/* the same search and the primal recovery (:206, :510) inside ONE persistent kernel: the dual
 * evaluations run on register-resident (J, y), their sums are combined by a last-arriver reduction,
 * the solver's state machine advances on the device; f(x+), g(x+) (:295) come out of the same pass
 * (f_x_out[0] = NaN when f is a host callback); one launch and one read-back per trial.
 * *ok_out = 0: not attempted (non-finite start, x sharded over ranks, m > 8, grid not co-resident) - fall back to
 * zf_mo_solve_dual / the reference's calls + zf_mo_recover.  *ok_out = -1: a grid-wide wait gave up (see
 * zf_mo_invalidate_prepare); same fall-back. */
int zf_mo_solve_dual_device(zf_mo* s, double lr, const double* f_y, const double* F_old, int32_t deprecated,
                            const double* w0, double tol, int64_t max_iter, double* w_out, double* fun_out,
                            int64_t* nit_out, int32_t* ok_out, int64_t* evals_out, double* err_out,
                            double* f_x_out /* m or NULL */, double* g_x_out /* m or NULL */,
                            double* f_y_out /* m or NULL: the f(y) used; f_y may be NULL after zf_mo_prepare_async */);
/* diagnostics of the last device solve: [0] batches (grid-wide hand-overs), [1] dual evaluations,
 * [2..5] shader-clock cycles of workgroup 0: whole kernel / evaluation loops / hand-overs / solver steps */
int zf_mo_solve_stats(zf_mo* s, int64_t* out, int64_t count /* >= 6 */);
int zf_mo_recover(zf_mo* s, double lr, const double* w_host, double* err_out);   /* :206, :510 */
int zf_mo_commit(zf_mo* s, double beta, int32_t nesterov);      /* :530-538 */
int zf_mo_get(zf_mo* s, int32_t which, double* host, int64_t count /* >= n */);
int zf_mo_put(zf_mo* s, int32_t which, const double* host);
int zf_mo_get_jac(zf_mo* s, double* J_host, int64_t count /* >= m * n */);
int zf_mo_prox_host(zf_mo* s, const double* weight_host, const double* x_host, double* out_host); /* problems.py:119-138 */
/* generic kind, after the user's prox callback produced p (host):
 * out[0..m) = J_i.(p - y), out[m] = |p - (y - lr w@J)|^2          proximal_gradient.py:168,173 */
int zf_mo_post_terms(zf_mo* s, double lr, const double* w_host, const double* p_host, double* out);

/* ---- device vector kernels (device pointers) ----------------------------- */
int zf_eval_diag_l1(const double* x_dev, const double* d_dev, const double* c_dev, double lam,
                    int64_t n, double out2_host[2], void* stream); /* f(x), g(x) */

#ifdef __cplusplus
}
#endif
#endif /* ZFISTA_HIP_H */
