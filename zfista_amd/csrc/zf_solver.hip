// zf_solver.hip - device-resident single-objective proximal-gradient solver
// and the C ABI of include/zfista_hip.h (gfx950 only).
//
// Replaces the outer loop body of zfista/proximal_gradient.py:474-538 for the
// recognised problem kinds.  The host enqueues "steps" (one line-search trial
// each) back to back on one HIP stream; acceptance, lr decay, termination and
// buffer rotation happen in a one-workgroup decide kernel, so there is no host
// round trip inside a chunk of steps.
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <tuple>
#include <vector>

#include "zf_common.h"
#include "zf_decide.h"
#include "zf_kernels_gemv.h"
#include "zf_kernels_ls_small.h"
#include "zf_kernels_gemv_f32.h"
#include "zf_kernels_mr.h"
#include "zf_kernels_op.h"
#include "zf_spmv.h"
#include "zf_matview.h"
#include "zf_screen.h"
#include "zf_kernels_loss.h"
#include "zf_kernels_gap.h"
#include "zf_kernels_softmax.h"
#include "zf_loss_dispatch.h"
#include "zf_kernels_step.h"
#include "zf_solver_options.h"
#include "zf_trial_launch.h"

thread_local char zf_errbuf[512] = "";

// for the entry points that allocate, launch and free in one call: run everything, keep the first HIP error in `rc`
#define ZF_KEEP_FIRST(expr)                                                       \
    do {                                                                          \
        hipError_t _e = (expr);                                                   \
        if (_e != hipSuccess && rc == ZF_OK)                                      \
            rc = zf_fail(ZF_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e));     \
    } while (0)

// ---------------------------------------------------------------------------
// finalize / decide kernels
// ---------------------------------------------------------------------------
// s_out = sum over ranks (rank order) of the gathered parts A_p x_p; slot as in zf_gemv_rows_kernel
__global__ __launch_bounds__(ZF_BLOCK) void zf_sum_parts_kernel(const zf_control* ctl, const double* __restrict__ s_all,
                                                                int world, int64_t m, zf_ring3 sr, int slot) {
    int idx = 0;
    if (slot >= 0) {
        if (ctl->status != ZF_RUNNING) return;
        idx = (ctl->cur + slot) % 3;
    }
    double* __restrict__ out = sr.p[idx];
    const int64_t stride = (int64_t)gridDim.x * ZF_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * ZF_BLOCK + threadIdx.x; i < m; i += stride) {
        double t = s_all[i];
        for (int r = 1; r < world; ++r) t += s_all[(int64_t)r * m + i];
        out[i] = t;
    }
}

// sharded x: packs = world x sub x ZF_PACK_LEN (rank-major).  The sub-iterations of a pass are
// examined in order; the first rejection / termination discards the speculative rest.
// stamped != 0 (separable problems): every rank's packs carry zf_pack_stamp of the control block their pass read.
// A step whose predicted shape kernel did not match (zf_predict_parts) produced none: the gathered packs are those of
// an earlier step, and this decide step must leave the control block alone - the host finds it unchanged at its next
// poll and launches every shape again.  All ranks hold the same control block and see the same gathered packs, so
// all of them skip together.
__global__ __launch_bounds__(64) void zf_decide_kernel(zf_control* ctl, const double* packs, double* trace,
                                                       const double* beta_ring, int sub, int stamped) {
    __shared__ zf_trial_eval s_pre[ZF_MAX_SUB_ITERS];
    if (blockIdx.x != 0) return;
    const int lane = threadIdx.x;
    if (stamped != 0) {
        const double want = zf_pack_stamp(ctl);
        const int world = ctl->world;
        for (int r = 0; r < world; ++r)
            if (packs[(int64_t)r * sub * ZF_PACK_LEN + 6] != want) return;
    }
    double pk[ZF_PACK_LEN] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (lane < sub) zf_reduce_packs(packs + lane * ZF_PACK_LEN, ctl->world, sub * ZF_PACK_LEN, pk);   // rank order
    zf_decide_pass_wave(ctl, packs, pk, trace, beta_ring, lane, 1, s_pre);
}

// The decide step of a SHARDED pass that ran ahead of its predecessor's decision (zf_decide_ahead, zf_kernels_step.h):
// as zf_decide_kernel, but the control block is first checked against the head the pass's trial kernel ran on - a
// pass on a head that did not come true is void - and the done / good word is published for the trial kernel two
// passes on.  All ranks hold the same block and the same gathered packs: all of them decide, or void, together.
__global__ __launch_bounds__(64) void zf_decide_ahead_kernel(zf_control* ctl, const double* packs, double* trace, const double* beta_ring,
                                                             int sub, zf_ahead_check H, unsigned long long* ra_word, unsigned* ra_stats,
                                                             int* pass_log, int pass_slot, int pass_tag) {
    __shared__ zf_trial_eval s_pre[ZF_MAX_SUB_ITERS];
    if (blockIdx.x != 0) return;
    const int lane = threadIdx.x;
    bool packs_ok = true;
    {
        const double want = zf_pack_stamp(ctl);
        const int world = ctl->world;
        for (int r = 0; r < world; ++r)
            if (packs[(int64_t)r * sub * ZF_PACK_LEN + 6] != want) packs_ok = false;
    }
    double pk[ZF_PACK_LEN] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (lane < sub) zf_reduce_packs(packs + lane * ZF_PACK_LEN, ctl->world, sub * ZF_PACK_LEN, pk);   // rank order
    zf_decide_ahead(ctl, packs, pk, trace, beta_ring, lane, 1, s_pre, H, packs_ok, ra_word, ra_stats, pass_log, pass_slot, pass_tag);
}

__global__ void zf_set_max_iter_kernel(zf_control* ctl, int64_t max_iter) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    ctl->max_iter = max_iter;
    if (ctl->status == ZF_MAXITER && ctl->nit < max_iter) ctl->status = ZF_RUNNING;
    if (ctl->pend_status == ZF_MAXITER && ctl->nit < max_iter) ctl->pend_status = 0;   // keep going instead
}

// ask the next pass to materialise lagging iterates (x_k, x_{k-1} into buffers) and nothing else
__global__ void zf_flush_kernel(zf_control* ctl) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (ctl->status == ZF_RUNNING && ctl->lag > 0 && ctl->pend_status == 0) ctl->pend_status = ZF_PEND_FLUSH;
}

// after the host refilled the momentum ring: re-resolve the factor of the pending trial
__global__ void zf_refresh_beta_kernel(zf_control* ctl, const double* beta_ring) {
    if (threadIdx.x == 0 && blockIdx.x == 0) zf_resolve_beta(ctl, beta_ring);
}

// initial F(x0): partials [f raw, |x|_1, violations] -> init pack [f, g, 0...]
// elastic net: g(x0) = sum (lam |x| + (l2 / 2) x^2) in the partials row of |x|_1 (zf_eval_kernel's layout: [0] unused - f comes
// from the margins - [1] g  [2] box violations), term by term as zf_elem_vec_enet forms g(x+); zf_init_finalize_kernel
// then takes it with lam = 1
template <bool BOX>
__global__ __launch_bounds__(ZF_BLOCK) void zf_eval_enet_kernel(const double* __restrict__ x, double lam, double hl2, double lo, double hi,
                                                                int64_t n, double* partials) {
    __shared__ double lds[ZF_WAVES * 3];
    double g = 0.0, viol = 0.0;
    const int64_t stride = (int64_t)gridDim.x * ZF_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * ZF_BLOCK + threadIdx.x; i < n; i += stride) {
        const double xv = x[i];
        g = __builtin_fma(lam, fabs(xv), g);
        g = __builtin_fma(hl2 * xv, xv, g);
        if (BOX) viol += (xv < lo || xv > hi) ? 1.0 : 0.0;
    }
    const double sums[3] = {0.0, g, viol};
    const double maxs[1] = {0.0};
    double out = 0.0;
    zf_block_reduce<3, 0, ZF_WAVES>(sums, maxs, lds, out);
    if (threadIdx.x < 3) partials[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = out;
}

// penalty factors: g(x0) / lam = sum p_j |x_j| in the same row, term by term as zf_elem_vec_pf forms it (p = 1: the sums of
// zf_eval_kernel, bit for bit); zf_init_finalize_kernel takes it with lam as before
template <bool BOX>
__global__ __launch_bounds__(ZF_BLOCK) void zf_eval_pf_kernel(const double* __restrict__ x, const double* __restrict__ p, double lo, double hi,
                                                              int64_t n, double* partials) {
    __shared__ double lds[ZF_WAVES * 3];
    double g = 0.0, viol = 0.0;
    const int64_t stride = (int64_t)gridDim.x * ZF_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * ZF_BLOCK + threadIdx.x; i < n; i += stride) {
        const double xv = x[i];
        g = __builtin_fma(p[i], fabs(xv), g);
        if (BOX) viol += (xv < lo || xv > hi) ? 1.0 : 0.0;
    }
    const double sums[3] = {0.0, g, viol};
    const double maxs[1] = {0.0};
    double out = 0.0;
    zf_block_reduce<3, 0, ZF_WAVES>(sums, maxs, lds, out);
    if (threadIdx.x < 3) partials[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = out;
}

struct zf_init_args {
    const double* partials;
    int nblocks;
    double f_scale, lam;
    const double* f_ext;
    double* pack;
    int contribute_g;   // row-sharded least squares: x is replicated, only rank 0 contributes g(x0)
};
__global__ __launch_bounds__(ZF_FIN_BLOCK) void zf_init_finalize_kernel(zf_init_args I) {
    __shared__ double lds[(ZF_FIN_BLOCK / 64) * 8];
    __shared__ double totals[8];
    zf_finalize_partials(I.partials, I.nblocks, 3, -1, lds, totals);
    if (threadIdx.x == 0) {
        const double f = I.f_ext ? *I.f_ext : I.f_scale * totals[0];
        double g = I.lam * totals[1];
        if (totals[2] > 0.0) g = INFINITY;   // zfista/problems.py:104-106
        I.pack[0] = f;
        I.pack[1] = I.contribute_g ? g : 0.0;
        for (int k = 2; k < ZF_PACK_LEN; ++k) I.pack[k] = 0.0;
        I.pack[2] = I.contribute_g ? totals[2] : 0.0;
    }
}
__global__ void zf_init_commit_kernel(zf_control* ctl, const double* packs, int f_replicated, int stride) {
    if (threadIdx.x || blockIdx.x) return;
    double f = packs[0], g = packs[1], viol = packs[2];
    for (int r = 1; r < ctl->world; ++r) {
        if (!f_replicated) f = f + packs[r * stride + 0];
        g = g + packs[r * stride + 1];
        viol = viol + packs[r * stride + 2];
    }
    if (viol > 0.0) g = INFINITY;
    ctl->f_x = f;
    ctl->g_x = g;
    ctl->F_old = f + g;   // proximal_gradient.py:279 at the first line search
}

// ---------------------------------------------------------------------------
// solver object
// ---------------------------------------------------------------------------
struct zf_comm;
extern "C" int zf_comm_all_gather(zf_comm* c, const double* send_dev, double* recv_dev, int64_t count, void* stream);
extern "C" int zf_comm_info(zf_comm* c, int32_t* rank, int32_t* world);

struct zf_solver {
    zf_problem_desc desc;
    zf_options opt;
    hipStream_t stream;
    int grid;                 // trial kernel grid
    bool box;
    int accept_mode = ZF_ACCEPT_REFERENCE;   // ZF_ACCEPT_*: what the control block, snapshots and the resume code carry
    bool res = false;         // ... == ZF_ACCEPT_RESOLVED: the kernels accumulate f(x+) - f(y) element by element (zf_elem_diag<..., RES>)
    bool rem = false;         // ... == ZF_ACCEPT_REMAINDER: the residual kernels at x+ also leave R = scale |A (x+ - y)|^2 in ls_scal[2]
    // device memory owned by the solver
    double* xbuf = nullptr;   // ring * n_pad
    double* xb[ZF_MAX_RING] = {};
    int sub = 1;              // FISTA iterations computed per pass (temporal blocking; separable f only)
    int ring = 3;             // iterate buffers (zf_decide.h: zf_free_bufs)
    double* partials = nullptr;   // init-time evaluation partials
    double* blk_part = nullptr;   // ZF_NPART x max_grid per-workgroup partials of the trial kernel
    double* slice_part = nullptr; // ZF_NPART x ZF_FIN_WGS
    unsigned* fin_cnt = nullptr;  // arrival counters: of the finalize workgroups / of the in-kernel finalisation (zf_pass_tail)
    double* grp_part = nullptr;   // ZF_NPART x S x ZF_FIN_GROUPS group rows of the in-kernel finalisation
    zf_env env;                   // the environment switches as zf_solver_create read them
    char* ctl_trace = nullptr;    // one allocation: the control block (ZF_CTL_SLOT bytes) and the trace ring behind it
    char* mail = nullptr;         // pinned host mirror of ctl_trace: what a poll copies into
    zf_control* ctl = nullptr;    // = ctl_trace
    double* trace = nullptr;      // = ctl_trace + ZF_CTL_SLOT: ZF_RING * ZF_TRACE_COLS
    double* beta_ring = nullptr;  // ZF_RING
    double* pack_local = nullptr; // ZF_PACK_LEN
    double* pack_all = nullptr;   // world * ZF_PACK_LEN
    // least squares
    double* grad = nullptr;       // n
    double* sbuf = nullptr;       // 3 * m_pad
    zf_ring3 sring = {{nullptr, nullptr, nullptr}};
    double* resid = nullptr;      // m_rows
    double* ls_scal = nullptr;    // [0] f(y) [1] f(x+) [2] the Taylor remainder R of the trial (ZF_ACCEPT_REMAINDER)
    double* s_part = nullptr;     // sharded: this rank's A_p x_p (m)
    double* s_all = nullptr;      // sharded: gathered parts (world x m, rank-major)
    bool own_svec = true;
    bool initialised = false;
    bool init_enqueued = false;   // zf_solver_enqueue_init(_all) ran: x0 is in the ring (zf_solver_set_comm may no longer reallocate it)
    bool own_packs = true;
    // the matrix kinds: the options of the eight zf_solver_set_* entries (zf_solver_options.h: the record, the rules, what follows
    // from them - zf_loss_of, zf_mat_of, zf_small_open below); small_shape, mfma_shape: what zf_solver_create found of the shape for
    // them (zf_options_base); sp: the caller's CSR handle (never written through), NULL for dense - and what the sweeps write between
    // their launches: the slab of ws.slices * n doubles, or this solver's segment sums of the split rows of A / of A^T
    zf_solver_options o;
    bool small_shape = false;
    bool mfma_shape = false;
    const zf_spmat* sp = nullptr;
    zf_sweep_ws ws = {nullptr, 1, 0, nullptr, nullptr};
    bool loss_part = false;       // the dense least-squares kind holds the 2 x ZF_SPMV_RESID_MAX_CHUNKS chunk sums of the loss kernels (zf_solver_set_option)
    double* gap_xp = nullptr;     // penalty factors: the certificate's scaled iterate p o x_k (n doubles, allocated by the first zf_solver_duality_gap)
    zf_op_plan op_plan = {};      // operator problem: which instantiation of the correlation kernels runs it (zf_op_make_plan)
    double* op_buf = nullptr;     // its taps as launched (zero-padded to K x K) and, behind them, the rank-1 factors u, v when the kernel is separable
    const double* op_taps = nullptr, *op_sep = nullptr;
    double* row_part = nullptr;   // ls_small: workgroup sums of the row kernel; sparse and logistic: chunk sums of the two residuals / losses
    unsigned* ls_cnt = nullptr;
    int64_t ntiles = 1;           // 16 KiB tiles of the trial kernel
    int tiles = 1;                // interleaved tiles per workgroup (zf_solver_autotune picks it)
    int max_grid = 1;
    // trial-kernel timing
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    double ms_total = 0.0;
    int64_t ms_count = 0;
    std::vector<std::pair<int, float>> records;   // (shape, ms) of every timed launch since the last zf_solver_pass_records
    // the per-pass exchange of a sharded solve (zf_gather_packs), bracketed the same way when timing is on
    std::vector<std::pair<hipEvent_t, hipEvent_t>> xev_pool;
    size_t xev_used = 0;
    double xms_total = 0.0;
    int64_t xms_count = 0;
    // the shape of every timed pass, written by the kernel itself (the host cannot know it at launch)
    int* pass_log = nullptr;              // ZF_PASS_LOG slots (device; inside ctl_trace, behind the trace ring)
    int64_t launches = 0;                 // timed launches so far (slot = launches % ZF_PASS_LOG)
    int64_t first_uncollected = 0;
    double ms_full = 0.0, ms_part = 0.0;  // S-trial chains without replay / everything else
    int64_t n_full = 0, n_part = 0;
    int64_t fresh_part = 0, lag_part = 0;   // fresh trials / replayed iterations carried by the other passes
    zf_comm* comm = nullptr;              // RCCL communicator (zf_solver_set_comm): the solver gathers itself
    // Which shape-specific kernel a pass needs is decided on the device; the host PREDICTS it from the control
    // block of its last poll (zf_predict_parts) and launches only that one.  A wrong prediction costs passes that
    // do nothing (no kernel finds its shape, the control block stays as it is), never a wrong result.
    int part_mask = 7;                    // ZF_K_* bits (ZF_K_ALL until a prediction says otherwise)
    int mid_len = 0;                      // ZF_K_MID: trials of the mid chain
    int fb_part = -1, fb_len = 0;         // ZF_K_FALLBACK: the general body runs what this kernel does not (-1: everything)
    int64_t steps_issued = 0, kernels_issued = 0;   // trial steps and the shape kernels launched for them (zf_solver_launch_counts)
    int pass_seq = 0;                     // step counter (zf_step_args.pass_seq)
    zf_control shadow;                    // the control block as the host expects it after the passes enqueued so far
    bool shadow_valid = false;            // false until the next poll (after init / restore / flush / set_max_iter ...)
    bool careful = false;                 // the last chunk saw rejections: launch every kernel a pass may need
    int64_t steps_since_poll = 0;         // trial steps issued since the shadow was read
    int64_t polled_rejections = 0;
    // Run-ahead passes (zf_runahead_kernel): consecutive full chains of a grid the device holds at once go alternately
    // to `stream` and `stream2`; stream k has its own rows / group rows / counters / packs (two passes are in flight)
    bool ra = false;                      // eligible (separable f, chains of 16, one rank, a one-round grid) and not switched off (ZF_RUNAHEAD=0)
    int ra_cap = -1;                      // co-resident workgroups of the run-ahead full chain (-1: not asked yet)
    int ra_cap_mid[ZF_MAX_SUB_ITERS] = {};   // ... of the run-ahead mid chain of that length (0: no such kernel; asked at the first use: -1)
    hipStream_t stream2 = nullptr;
    hipStream_t stream3 = nullptr;        // sharded run-ahead passes: all-gather + decide of the pass before, beside the two trial streams
    hipEvent_t ra_join3 = nullptr;        // stream3 -> stream at the end of such a run
    bool ra_c_pending = false;            // stream3 holds work `stream` has not been made to wait for
    bool chunk_last = false;              // the step being enqueued is the last of its zf_solver_enqueue_steps call
    bool ra_sharded = true;               // ZF_RUNAHEAD_SHARDED: one-round grids behind a library communicator take run-ahead passes (else passes ahead)
    int64_t ras_passes = 0;               // sharded run-ahead passes launched
    hipEvent_t ra_join = nullptr;         // stream2 -> stream at the end of a run of run-ahead passes
    hipEvent_t ra_fork = nullptr;         // stream -> stream2 in front of a run
    bool ra_b_pending = false;            // stream2 holds work `stream` has not been made to wait for
    bool ra_fork_due = false;             // ra_fork was recorded in front of the current run and stream2 has not waited for it yet
    int ra_last = 0, ra_last2 = 0;        // pass_seq of the last / last but one run-ahead pass of the current run (0: none)
    int ra_last_idx = 0;                  // stream of the last one
    zf_pass_head ra_last_head = {};       // its head (whose buffers the next pass must not write)
    unsigned long long* ra_word = nullptr;
    unsigned* ra_flags = nullptr;         // max_grid + 32 words
    double* blk_part2 = nullptr;
    double* grp_part2 = nullptr;
    unsigned* fin_cnt2 = nullptr;
    double* pack2 = nullptr;
    int64_t ra_passes = 0, ra_ahead = 0;  // run-ahead kernels launched / of them behind a pass still in flight (zf_solver_launch_counts)
    // What the device reports about passes that ran ahead: four counters in the slack of the control block's slot,
    // copied with every poll - [0] waits that gave up (a run-ahead workgroup's, or a deciding wave's), [1] void run-ahead
    // passes, [2] void passes AHEAD (below), [3] second passes of a run (either scheme) whose first pass left on a head
    // that did not come true (they run no body).  After the first wait that gave up the solver launches no further
    // run-ahead passes (ra_off): the device is being shared, and every such wait costs its whole limit.
    unsigned* ra_stats = nullptr;         // = ctl_trace + ZF_STATS_OFF
    int64_t ra_timeouts = 0, ra_voids = 0, ah_voids = 0, second_voids = 0;   // as of the last poll
    bool ra_off = false;
    // Passes AHEAD at kernel granularity (zf_trial_kernel<..., AHEAD>, zf_tail_kernel, zf_decide_ahead_kernel): sharded
    // solves through the library's communicator, and (ZF_AHEAD_UNSHARDED) unsharded grids of more than one round.  The
    // trial kernels of consecutive exactly predicted full / mid chains go back to back to `stream`, each on the head the
    // host expects; rows -> packs (-> all-gather) -> decide of pass p run on `stream2` behind an event, beside the
    // trial kernel of pass p + 1; the trial kernel of pass p + 2 is launched behind an event of decide p.
    bool ah = false;                      // eligible (separable f, chains of 16, nontemporal policy, six buffers) and not switched off (ZF_AHEAD=0)
    bool ah_unsharded = false;            // ... also without a communicator
    hipEvent_t ah_evT[4] = {}, ah_evD[4] = {};   // trial kernel done (stream) / decided (stream2), by pass number of the run % 4
    int ah_run = 0;                       // passes of the current run so far
    int ah_last_nf = 0;                   // fresh trials of the last one
    int run_mode = 0;                     // what the current run of passes in flight consists of: 0 none, 1 run-ahead passes (workgroup granularity), 2 passes ahead (kernel granularity) - a run is one or the other
    int64_t ah_passes = 0;                // passes launched ahead since creation
    // streaming return_all: caller-owned ring of iterates in HBM (zf_solver_set_history)
    double* hist = nullptr;
    int64_t hist_cap = 0, hist_stride = 0;
    // zf_solver_duality_gap: its workspace (one m-vector, one n-vector, chunk results, scalars), allocated by the first call -
    // a solve that never asks for the gap allocates and launches nothing for it
    zf_gap_ws gap = {nullptr, nullptr, nullptr, nullptr};
};
constexpr int ZF_PASS_LOG = 4096;
constexpr size_t ZF_CTL_SLOT = (sizeof(zf_control) + 255) / 256 * 256;   // bytes in front of the trace ring (zf_solver::ctl_trace)
constexpr size_t ZF_STATS_OFF = ZF_CTL_SLOT - 32;                         // the run-ahead counters (zf_solver::ra_stats): 8 words in the slot's slack
static_assert(sizeof(zf_control) <= ZF_STATS_OFF, "the run-ahead counters live behind the control block, inside its slot");
constexpr size_t ZF_TRACE_BYTES = sizeof(double) * ZF_RING * ZF_TRACE_COLS;
constexpr size_t ZF_MAIL_BYTES = ZF_CTL_SLOT + ZF_TRACE_BYTES + sizeof(int) * ZF_PASS_LOG;

static int zf_tiles_for(int64_t ntiles);
// passes ahead at kernel granularity for UNSHARDED grids of more than one round (ZF_AHEAD_UNSHARDED overrides)
constexpr bool ZF_AHEAD_UNSHARDED_DEFAULT = false;

// The one reader of the environment (zf_common.h); "ZF_X=0" switches a default off, any other value on.
zf_env zf_env_read() {
    zf_env v;
    const char* e;
    v.speculate = !((e = getenv("ZF_SPECULATE")) && atoi(e) == 0);
    v.pass_seq_start = (e = getenv("ZF_PASS_SEQ_START")) ? (int)std::min<long long>(std::max<long long>(atoll(e), 0), 0x7ffffff0LL) : 0;
    v.sub_iters = (e = getenv("ZF_SUB_ITERS")) ? atoi(e) : 0;
    v.runahead = !((e = getenv("ZF_RUNAHEAD")) && atoi(e) == 0);
    v.tiles_per_wg = (e = getenv("ZF_TILES_PER_WG")) ? std::max(1, atoi(e)) : 0;
    // ~15 ms, some tens of passes' worth; 0: every pass behind a pass in flight gives up at once (tests)
    v.runahead_spin = (e = getenv("ZF_RUNAHEAD_SPIN_LIMIT")) ? (unsigned)strtoul(e, nullptr, 10) : 1u << 13;
    v.runahead_sharded = (e = getenv("ZF_RUNAHEAD_SHARDED")) ? (atoi(e) != 0 ? 1 : 0) : -1;
    v.ahead = !((e = getenv("ZF_AHEAD")) && atoi(e) == 0);
    v.ahead_unsharded = (e = getenv("ZF_AHEAD_UNSHARDED")) ? atoi(e) != 0 : ZF_AHEAD_UNSHARDED_DEFAULT;
    v.gemv_mfma = !((e = getenv("ZF_GEMV_MFMA")) && atoi(e) == 0);
    v.ls_small = !((e = getenv("ZF_LS_SMALL")) && atoi(e) == 0);
    v.op_separable = !((e = getenv("ZF_OP_SEPARABLE")) && atoi(e) == 0);
    v.op_fuse_prox = !((e = getenv("ZF_OP_FUSE_PROX")) && atoi(e) == 0);
    v.op_persist = !((e = getenv("ZF_OP_PERSIST")) && atoi(e) == 0);
    v.mo_spin_limit = (e = getenv("ZF_MO_SPIN_LIMIT")) ? atoll(e) : 0;
    return v;
}

static int zf_solver_free_all(zf_solver* s) {
    if (s->stream2) (void)hipStreamDestroy(s->stream2);
    if (s->stream3) (void)hipStreamDestroy(s->stream3);
    if (s->ra_join3) (void)hipEventDestroy(s->ra_join3);
    for (int k = 0; k < 4; ++k) {
        if (s->ah_evT[k]) (void)hipEventDestroy(s->ah_evT[k]);
        if (s->ah_evD[k]) (void)hipEventDestroy(s->ah_evD[k]);
    }
    if (s->ra_join) (void)hipEventDestroy(s->ra_join);
    if (s->ra_fork) (void)hipEventDestroy(s->ra_fork);
    void* ptrs[] = {s->ws.part_A, s->ws.part_At, s->op_buf, s->row_part, s->ls_cnt, s->blk_part, s->slice_part, s->fin_cnt, s->grp_part, s->xbuf, s->partials, s->ctl_trace, s->beta_ring,
                    s->ra_word, s->ra_flags, s->blk_part2, s->grp_part2, s->fin_cnt2, s->pack2,
                    s->own_packs ? s->pack_local : nullptr, s->own_packs ? s->pack_all : nullptr,
                    s->grad, s->sbuf, s->resid, s->ws.slab, s->ls_scal, s->gap.rvec, s->gap.g, s->gap.part, s->gap.scal, s->gap_xp,
                    s->own_svec ? s->s_part : nullptr, s->own_svec ? s->s_all : nullptr};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (s->mail) (void)hipHostFree(s->mail);
    for (auto& e : s->ev_pool) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    for (auto& e : s->xev_pool) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    return ZF_OK;
}

// the trial kernels' variant of this solver (zf_trial_launch.h)
static zf_trial_sel zf_sel_of(const zf_solver* s) { return zf_trial_sel{s->opt.nesterov != 0, s->box, s->res}; }

static bool zf_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// least squares with an explicit matrix - dense, or CSR (zf_kernels_spmv.h) - or with the blur o inverse-Haar operator
// (zf_kernels_op.h): everything around the two applications of A / its adjoint is shared
static bool zf_is_ls(int kind) {
    return kind == ZF_PROBLEM_LEAST_SQUARES_L1 || kind == ZF_PROBLEM_BLUR_HAAR_L1 || kind == ZF_PROBLEM_SPARSE_LS_L1;
}
// the logistic loss of the margins A x (zf_kernels_loss.h) on the same two storage forms of A: the trial of the squared
// loss with the residual kernels swapped for the loss kernels and the sweeps called with scale for 2 scale
static bool zf_is_logistic(int kind) { return kind == ZF_PROBLEM_LOGISTIC_L1 || kind == ZF_PROBLEM_SPARSE_LOGISTIC_L1; }
static bool zf_is_dense_mat(int kind) { return kind == ZF_PROBLEM_LEAST_SQUARES_L1 || kind == ZF_PROBLEM_LOGISTIC_L1; }
static bool zf_is_sparse_mat(int kind) { return kind == ZF_PROBLEM_SPARSE_LS_L1 || kind == ZF_PROBLEM_SPARSE_LOGISTIC_L1; }
// f is a loss of A x: the margins of x_k, x_{k-1} are kept in a ring and A y follows by linearity
static bool zf_has_margins(int kind) { return zf_is_ls(kind) || zf_is_logistic(kind); }
// ---- what a solver's options record implies (zf_solver_options.h) ----
static_assert(ZF_OPT_MAX_K == ZF_MR_MAX_K && ZF_OPT_MAX_K == ZF_SPMM_MAX_K, "one bound of the response count");
static zf_options_base zf_base_of(const zf_solver* s) {
    const zf_problem_desc& d = s->desc;
    return zf_options_base{(int)d.kind, (int)d.world, s->accept_mode, s->init_enqueued || s->initialised, d.m_rows, d.n, d.b, s->small_shape, s->mfma_shape};
}
// the loss (zf_loss_dispatch.h)
static zf_loss zf_loss_of(const zf_solver* s) { return zf_loss{zf_options_loss(s->desc.kind, s->o), s->o.huber, s->o.roww, s->o.K}; }
// A as the two sweeps see it (zf_matview.h): desc.A, or the matrix stored in fp32 (nothing reads desc.A then), or the handle's
// (o: the solver's record, or the record a setter is about to store)
static zf_matview zf_mat_of(const zf_solver* s, const zf_solver_options& o) {
    const zf_options_view v = zf_options_view_of(zf_base_of(s), o);
    return zf_matview{v.f32 ? nullptr : s->desc.A, v.m, v.n, s->sp, s->sp != nullptr, o.A32, v.K, v.mfma};
}
static zf_matview zf_mat_of(const zf_solver* s) { return zf_mat_of(s, s->o); }
// cache-resident A: two fused launches per trial (zf_kernels_ls_small.h)
static bool zf_small_open(const zf_solver* s) { return zf_options_small_open(zf_base_of(s), s->o); }
// the factor of the g sum in the finalisation of a trial and of the initial point: the l1 kernels leave sum |x| (or sum p |x|) there
static double zf_g_scale(const zf_solver* s) { return zf_options_g_is_whole(s->o) ? 1.0 : s->desc.lam; }
static zf_op_args zf_op_of(const zf_problem_desc& d, const zf_control* ctl, const zf_op_plan& pl, const double* taps, const double* sep) {
    zf_op_args P;
    P.ctl = ctl;
    P.H = (int)d.op_h;
    P.W = (int)d.op_w;
    P.K = pl.K;
    P.taps = taps;
    P.sep = pl.sep ? sep : nullptr;
    P.tiles = pl.grid;
    return P;
}
static zf_op_args zf_op_of(const zf_solver* s, const zf_control* ctl) { return zf_op_of(s->desc, ctl, s->op_plan, s->op_taps, s->op_sep); }
static zf_op_fuse zf_op_no_fuse() {
    zf_op_fuse F;
    memset(&F, 0, sizeof(F));
    return F;
}
constexpr int64_t ZF_OP_FUSE_MAX_PIXELS = int64_t(5) << 20;   // operator problem: the prox step rides in the adjoint kernel up to this size
// The taps as the kernels take them: K x K with K the launched size (1 x 1 is zero-padded to 3 x 3), and - when the
// kernel has rank 1 and ZF_OP_SEPARABLE is not 0 - its factors u, v behind them; the plan as `env` shapes it.  *buf: one
// device allocation (caller frees); `st`: the stream the upload is ordered on.
static int zf_op_prepare(const zf_env& env, const double* taps_dev, int k, int64_t h, int64_t w, hipStream_t st, zf_op_plan* pl,
                         double** buf, const double** taps_out, const double** sep_out) {
    double host[ZF_OP_MAXK * ZF_OP_MAXK];
    ZF_HIP(hipMemcpyAsync(host, taps_dev, sizeof(double) * k * k, hipMemcpyDeviceToHost, st));
    ZF_HIP(hipStreamSynchronize(st));
    const int K = k < 3 ? 3 : k;
    double up[ZF_OP_MAXK * ZF_OP_MAXK + 2 * (ZF_OP_MAXK + 1)];
    memset(up, 0, sizeof(up));
    const int pad = (K - k) / 2;
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) up[(i + pad) * K + j + pad] = host[i * k + j];
    double* u = up + ZF_OP_MAXK * ZF_OP_MAXK;
    double* v = u + ZF_OP_MAXK + 1;
    const bool sep = env.op_separable && zf_op_factor_rank1(up, K, u, v);
    *pl = zf_op_make_plan(h, w, k, sep, env.op_persist);
    pl->fuse_prox = env.op_fuse_prox && h * w <= ZF_OP_FUSE_MAX_PIXELS;
    ZF_HIP(hipMalloc(buf, sizeof(up)));
    ZF_HIP(hipMemcpyAsync(*buf, up, sizeof(up), hipMemcpyHostToDevice, st));
    ZF_HIP(hipStreamSynchronize(st));   // `up` is a stack object
    *taps_out = *buf;
    *sep_out = *buf + ZF_OP_MAXK * ZF_OP_MAXK;
    return ZF_OK;
}

// s[(cur + slot) % 3] = A x[(cur + slot) % 3] inside the loop (ctl given), or sout.p[0] = A xr.p[0] outside it (ctl NULL): the
// operator's own kernel, or the row sweep of the solver's matrix view
static void zf_launch_apply_A(zf_solver* s, const zf_control* ctl, zf_ring3 xr, zf_ring3 sout, int slot) {
    if (s->desc.kind == ZF_PROBLEM_BLUR_HAAR_L1)   // (the operator is no matrix view)
        zf_launch_op_apply(s->op_plan, s->stream, zf_op_of(s, ctl), xr.p[0], xr.p[1], xr.p[2], sout.p[0], sout.p[1], sout.p[2], slot,
                           zf_op_no_fuse());
    else
        zf_launch_apply(zf_mat_of(s), s->stream, ctl, xr, sout, slot, s->ws);
}

// What two passes in flight need: the second stream (non-blocking, at the highest priority: what runs there - a waiting
// pass, or the small kernels that finalise and decide a pass beside the next pass's trial kernel - must not queue behind
// that kernel's workgroups), the events, the done / good word and the per-workgroup flags, a second set of rows / group
// rows / counters / packs.  Idempotent.
static hipError_t zf_second_stream(zf_solver* s) {
    if (s->stream2) return hipSuccess;
    hipError_t e;
#define ZF_E(expr)                  \
    do {                            \
        e = (expr);                 \
        if (e != hipSuccess) return e; \
    } while (0)
    int lo = 0, hi = 0;
    ZF_E(hipDeviceGetStreamPriorityRange(&lo, &hi));
    ZF_E(hipStreamCreateWithPriority(&s->stream2, hipStreamNonBlocking, hi));
    ZF_E(hipStreamCreateWithPriority(&s->stream3, hipStreamNonBlocking, hi));
    ZF_E(hipEventCreateWithFlags(&s->ra_join3, hipEventDisableTiming));
    ZF_E(hipEventCreateWithFlags(&s->ra_join, hipEventDisableTiming));
    ZF_E(hipEventCreateWithFlags(&s->ra_fork, hipEventDisableTiming));
    for (int k = 0; k < 4; ++k) {
        ZF_E(hipEventCreateWithFlags(&s->ah_evT[k], hipEventDisableTiming));
        ZF_E(hipEventCreateWithFlags(&s->ah_evD[k], hipEventDisableTiming));
    }
    ZF_E(hipMalloc(&s->ra_word, 128));
    ZF_E(hipMemsetAsync(s->ra_word, 0, 128, s->stream));
    ZF_E(hipMalloc(&s->ra_flags, sizeof(unsigned) * (s->max_grid + 32)));
    ZF_E(hipMemsetAsync(s->ra_flags, 0, sizeof(unsigned) * (s->max_grid + 32), s->stream));
    ZF_E(hipMalloc(&s->blk_part2, sizeof(double) * ZF_NPART * s->sub * s->max_grid));
    ZF_E(hipMalloc(&s->grp_part2, sizeof(double) * ZF_NPART * s->sub * ZF_FIN_GROUPS));
    ZF_E(hipMalloc(&s->fin_cnt2, sizeof(unsigned) * ZF_FIN_CNT_STRIDE * (ZF_FIN_GROUPS + 2)));
    ZF_E(hipMemsetAsync(s->fin_cnt2, 0, sizeof(unsigned) * ZF_FIN_CNT_STRIDE * (ZF_FIN_GROUPS + 2), s->stream));
    ZF_E(hipMalloc(&s->pack2, sizeof(double) * ZF_PACK_LEN * s->sub));
#undef ZF_E
    return hipSuccess;
}

// sp: the matrix handle of ZF_PROBLEM_SPARSE_LS_L1 (zf_solver_create_sparse), NULL for every other kind; K > 1: the responses of
// zf_solver_create_sparse_responses (desc holds the flattened lengths sp->m K and sp->n K)
static int zf_solver_create_impl(zf_solver** out, const zf_problem_desc* desc, const zf_options* opt, void* stream, const zf_spmat* sp,
                                 int K = 1) {
    ZF_REQUIRE(out && desc && opt, "zf_solver_create: null argument");
    ZF_REQUIRE(desc->n >= 1, "zf_solver_create: n must be >= 1");
    ZF_REQUIRE(desc->world >= 1 && desc->rank >= 0 && desc->rank < desc->world,
               "zf_solver_create: bad world/rank");
    ZF_REQUIRE(opt->max_iter >= 1, "zf_solver_create: max_iter must be >= 1");
    ZF_REQUIRE(opt->max_backtrack_iter >= 0, "zf_solver_create: max_backtrack_iter must be >= 0");
    // the fused kernels threshold with tau = lam * lr >= 0 (zf_soft_threshold_nn)
    ZF_REQUIRE(desc->lam >= 0.0 && opt->lr > 0.0 && opt->decay_rate > 0.0,
               "zf_solver_create: needs lam >= 0, lr > 0, decay_rate > 0 (use the callback path otherwise)");
    if (desc->kind == ZF_PROBLEM_DIAG_QUAD_L1) {
        ZF_REQUIRE(desc->d && desc->c, "zf_solver_create: d and c are required");
        ZF_REQUIRE(zf_aligned16(desc->d) && zf_aligned16(desc->c),
                   "zf_solver_create: d and c must be 16-byte aligned");
    } else if (zf_is_dense_mat(desc->kind)) {
        ZF_REQUIRE(desc->A && desc->b && desc->m_rows >= 1, "zf_solver_create: A, b, m_rows required");
        ZF_REQUIRE(zf_aligned16(desc->A), "zf_solver_create: A must be 16-byte aligned");
        ZF_REQUIRE(desc->kind == ZF_PROBLEM_LEAST_SQUARES_L1 || desc->world == 1, "zf_solver_create: logistic regression is not sharded");
    } else if (desc->kind == ZF_PROBLEM_BLUR_HAAR_L1) {
        ZF_REQUIRE(desc->b && desc->op_taps, "zf_solver_create: b (the observed image) and op_taps are required");
        ZF_REQUIRE(desc->op_h >= 2 && desc->op_w >= 2 && desc->op_h % 2 == 0 && desc->op_w % 2 == 0 &&
                       desc->op_h * desc->op_w == desc->n && desc->m_rows == desc->n,
                   "zf_solver_create: the image must be op_h x op_w (both even) with n = m_rows = op_h * op_w");
        ZF_REQUIRE(desc->op_k >= 1 && desc->op_k % 2 == 1 && desc->op_k <= ZF_OP_MAXK && desc->op_k / 2 < desc->op_h &&
                       desc->op_k / 2 < desc->op_w,
                   "zf_solver_create: op_k must be odd, at most 15 and smaller than twice the image");
        ZF_REQUIRE(desc->world == 1, "zf_solver_create: the operator problem is not sharded");
    } else if (zf_is_sparse_mat(desc->kind)) {
        ZF_REQUIRE(sp, "zf_solver_create: ZF_PROBLEM_SPARSE_LS_L1 and ZF_PROBLEM_SPARSE_LOGISTIC_L1 take their matrix through zf_solver_create_sparse");
        ZF_REQUIRE(desc->b && !desc->A, "zf_solver_create_sparse: b is required and A must be NULL (the matrix is the handle's)");
        if (K > 1)
            ZF_REQUIRE(desc->m_rows == sp->m * K && desc->n == sp->n * K,
                       "zf_solver_create_sparse_responses: m_rows and n must be K times the matrix handle's");
        else
            ZF_REQUIRE(desc->m_rows == sp->m && desc->n == sp->n, "zf_solver_create_sparse: m_rows and n differ from the matrix handle's");
        ZF_REQUIRE(desc->world == 1, "zf_solver_create_sparse: sparse problems are not sharded");
    } else {
        return zf_fail(ZF_ERR_ARG, "zf_solver_create: unknown problem kind");
    }
    zf_solver* s = new (std::nothrow) zf_solver();
    if (!s) return zf_fail(ZF_ERR_ARG, "zf_solver_create: out of host memory");
    s->desc = *desc;
    s->opt = *opt;
    s->env = zf_env_read();
    if (zf_is_sparse_mat(desc->kind)) {
        s->sp = sp;
        s->o.K = K;
    }
    s->mfma_shape = zf_is_dense_mat(desc->kind) && desc->n % 32 == 0 && s->env.gemv_mfma;
    s->pass_seq = s->env.pass_seq_start;
    s->stream = reinterpret_cast<hipStream_t>(stream);
    s->box = !(desc->box_lo == -INFINITY && desc->box_hi == INFINITY);
    if (opt->accept_mode != ZF_ACCEPT_REFERENCE) {
        const bool res_ok = opt->accept_mode == ZF_ACCEPT_RESOLVED && desc->kind == ZF_PROBLEM_DIAG_QUAD_L1;
        const bool rem_ok = opt->accept_mode == ZF_ACCEPT_REMAINDER &&
                            (desc->kind == ZF_PROBLEM_LEAST_SQUARES_L1 || desc->kind == ZF_PROBLEM_SPARSE_LS_L1);
        if (!res_ok && !rem_ok) {
            delete s;
            return zf_fail(ZF_ERR_ARG, "zf_solver_create: accept_mode must be ZF_ACCEPT_REFERENCE, ZF_ACCEPT_RESOLVED for "
                                       "ZF_PROBLEM_DIAG_QUAD_L1 (the element-wise difference f(x+) - f(y) exists for the separable problem only), or "
                                       "ZF_ACCEPT_REMAINDER for ZF_PROBLEM_LEAST_SQUARES_L1 and ZF_PROBLEM_SPARSE_LS_L1 (the Taylor remainder "
                                       "scale |A (x+ - y)|^2 is formed by the least-squares residual kernels only)%s");
        }
        s->accept_mode = opt->accept_mode;
        s->res = res_ok;
        s->rem = rem_ok;
    }
    const int64_t n = desc->n;
    const int64_t n_pad = (n + 63) & ~int64_t(63);   // keep every ring buffer 512-B aligned
    {   // one workgroup per tile of ZF_TILE_UNITS 16-byte units (zf_kernels_step.h)
        int64_t ntiles = (n / 2 + ZF_TILE_UNITS - 1) / ZF_TILE_UNITS;
        if (ntiles < 1) ntiles = 1;
        if (ntiles > 0x7fffffff) {
            delete s;
            return zf_fail(ZF_ERR_ARG, "zf_solver_create: n too large for one rank");
        }
        s->ntiles = ntiles;
        s->grid = (int)ntiles;            // tiles_per_wg = 1: the largest grid; buffers are sized for it
        s->max_grid = s->grid;
    }
#define ZF_TRY(expr)                                                                    \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            zf_solver_free_all(s);                                                      \
            delete s;                                                                   \
            return zf_fail(ZF_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e));         \
        }                                                                               \
    } while (0)
    if (desc->kind == ZF_PROBLEM_DIAG_QUAD_L1) {
        // every term of the recursion is elementwise for this f, so one pass may run `sub`
        // consecutive iterations in registers (zf_kernels_step.h); 0 = library default
        int sub = opt->sub_iters;
        if (sub <= 0) sub = s->env.sub_iters;
        if (sub <= 0) sub = ZF_DEFAULT_SUB_ITERS;
        if (sub > ZF_MAX_SUB) sub = ZF_MAX_SUB;
        s->sub = sub >= 16 ? 16 : sub >= 8 ? 8 : sub >= 4 ? 4 : sub >= 2 ? 2 : 1;
        // (the kernels of ZF_ACCEPT_RESOLVED exist for chains of 16 and single trials, nontemporal policy)
        if (s->res && s->sub != 16) s->sub = 1;
    }
    s->ring = s->sub > 1 ? 4 : 3;   // x_k, x_{k-1} + the one or two iterates a pass stores
    {   // passes that run ahead of their predecessor's decision (chains of 16 of the separable problem), two ways:
        // * run-ahead passes at WORKGROUP granularity (zf_runahead_kernel): one rank, a grid the device holds at once
        //   (the geometry is a function of n; what the device holds of the kernel is asked of the runtime): full chains of
        //   every variant, mid chains where the per-pass mid chains exist (no box);
        // * passes AHEAD at KERNEL granularity: every grid, boxes too; for sharded solves through the library's
        //   communicator (zf_solver_set_comm) and - ZF_AHEAD_UNSHARDED - unsharded grids the other scheme does not take.
        const int t = s->env.tiles_per_wg > 0 ? s->env.tiles_per_wg : zf_tiles_for(s->ntiles);
        const int64_t grid = (s->ntiles + t - 1) / t;
        const bool chains16 = desc->kind == ZF_PROBLEM_DIAG_QUAD_L1 && s->sub >= 16;
        // (world > 1, or one rank behind a communicator: the SHARDED run-ahead passes - same kernels, packs instead of a decision)
        s->ra = s->env.runahead && chains16;
        if (s->env.runahead_sharded >= 0) s->ra_sharded = s->env.runahead_sharded != 0;
        if (s->ra) {
            s->ra_cap = zf_runahead_capacity(zf_sel_of(s), s->sub);
            s->ra = grid <= s->ra_cap;
            for (int l = 0; l < ZF_MAX_SUB_ITERS; ++l) s->ra_cap_mid[l] = -1;
        }
        s->ah = s->env.ahead && chains16;
        s->ah_unsharded = s->ah && desc->world == 1 && s->env.ahead_unsharded;
    }
    if (s->ra || (s->ah && (desc->world > 1 || s->ah_unsharded))) {
        s->ring = 6;   // a pass never writes what its predecessor reads (zf_free_bufs)
        // (no second stream - a runtime without stream priorities, an allocation that failed: every pass then runs on the
        //  caller's stream, one launch at a time; nothing else depends on it)
        if (zf_second_stream(s) != hipSuccess) {
            (void)hipGetLastError();
            s->ra = false;
            s->ah = false;
        }
    }
    ZF_TRY(hipMalloc(&s->xbuf, sizeof(double) * s->ring * n_pad));
    for (int k = 0; k < s->ring; ++k) s->xb[k] = s->xbuf + k * n_pad;
    ZF_TRY(hipMalloc(&s->partials, sizeof(double) * ZF_NPART * ZF_MAX_GRID));
    {   // (the small least-squares step kernel has n / 32 workgroups: more than tiles)
        int64_t parts = std::max<int64_t>(s->max_grid, n / LS_SMALL_COLS + 1);
        // (operator problem: the fused prox step writes a row per workgroup of the adjoint kernel - one per image tile, and a
        //  narrow image has more tiles than n / 32: 1000 x 2 is 125 tiles of 64 x 8 on 2000 coefficients.  The tile count
        //  depends on the image and the kernel size only, not on the path zf_op_prepare picks below.)
        if (desc->kind == ZF_PROBLEM_BLUR_HAAR_L1)
            parts = std::max<int64_t>(parts, zf_op_make_plan(desc->op_h, desc->op_w, (int)desc->op_k, false, false).grid);
        ZF_TRY(hipMalloc(&s->blk_part, sizeof(double) * ZF_NPART * s->sub * parts));
    }
    ZF_TRY(hipMalloc(&s->slice_part, sizeof(double) * ZF_NPART * s->sub * ZF_FIN_WGS));
    ZF_TRY(hipMalloc(&s->fin_cnt, sizeof(unsigned) * ZF_FIN_CNT_STRIDE * (ZF_FIN_GROUPS + 2)));
    ZF_TRY(hipMemsetAsync(s->fin_cnt, 0, sizeof(unsigned) * ZF_FIN_CNT_STRIDE * (ZF_FIN_GROUPS + 2), s->stream));
    ZF_TRY(hipMalloc(&s->grp_part, sizeof(double) * ZF_NPART * s->sub * ZF_FIN_GROUPS));
    // the control block and the trace ring side by side, and a pinned host mirror of both: a poll is ONE DMA into
    // pinned memory (two copies into the caller's pageable arrays cost 34 us on an idle stream, this costs a third)
    //  - and, behind them, the log of pass shapes the kernels keep when timing is on)
    ZF_TRY(hipMalloc(&s->ctl_trace, ZF_MAIL_BYTES));
    s->ctl = reinterpret_cast<zf_control*>(s->ctl_trace);
    s->trace = reinterpret_cast<double*>(s->ctl_trace + ZF_CTL_SLOT);
    s->pass_log = reinterpret_cast<int*>(s->ctl_trace + ZF_CTL_SLOT + ZF_TRACE_BYTES);
    s->ra_stats = reinterpret_cast<unsigned*>(s->ctl_trace + ZF_STATS_OFF);
    ZF_TRY(hipMemsetAsync(s->ctl_trace, 0, ZF_CTL_SLOT, s->stream));
    ZF_TRY(hipMemsetAsync(s->pass_log, 0xff, sizeof(int) * ZF_PASS_LOG, s->stream));   // (no launch carries tag 0x7fff + negative sign)
    ZF_TRY(hipHostMalloc(&s->mail, ZF_MAIL_BYTES, hipHostMallocDefault));
    ZF_TRY(hipMalloc(&s->beta_ring, sizeof(double) * ZF_RING));
    ZF_TRY(hipMalloc(&s->pack_local, sizeof(double) * ZF_PACK_LEN * s->sub));
    ZF_TRY(hipMalloc(&s->pack_all, sizeof(double) * ZF_PACK_LEN * s->sub * desc->world));
    ZF_TRY(hipMemsetAsync(s->trace, 0, sizeof(double) * ZF_RING * ZF_TRACE_COLS, s->stream));
    ZF_TRY(hipMemsetAsync(s->beta_ring, 0, sizeof(double) * ZF_RING, s->stream));
    ZF_TRY(hipMemsetAsync(s->pack_all, 0, sizeof(double) * ZF_PACK_LEN * s->sub * desc->world, s->stream));
    if (zf_has_margins(desc->kind)) {   // the gradient, the ring of margins A x, psi(y) and the scalars of a trial
        const int64_t m_pad = (desc->m_rows + 63) & ~int64_t(63);   // (the operator: m_rows = n)
        ZF_TRY(hipMalloc(&s->grad, sizeof(double) * n_pad));
        ZF_TRY(hipMalloc(&s->sbuf, sizeof(double) * 3 * m_pad));
        for (int k = 0; k < 3; ++k) s->sring.p[k] = s->sbuf + k * m_pad;
        ZF_TRY(hipMalloc(&s->resid, sizeof(double) * m_pad));
        ZF_TRY(hipMalloc(&s->ls_scal, sizeof(double) * 8));
    }
    if (desc->kind == ZF_PROBLEM_BLUR_HAAR_L1) {
        if (zf_op_prepare(s->env, desc->op_taps, (int)desc->op_k, desc->op_h, desc->op_w, s->stream, &s->op_plan, &s->op_buf, &s->op_taps, &s->op_sep) != ZF_OK) {
            zf_solver_free_all(s);
            delete s;
            return ZF_ERR_HIP;   // (message set by zf_op_prepare)
        }
        ZF_TRY(hipMalloc(&s->row_part, sizeof(double) * 2 * s->op_plan.grid));   // shares of |r(y)|^2 and of |s+ - b|^2
        ZF_TRY(hipMemsetAsync(s->row_part, 0, sizeof(double) * 2 * s->op_plan.grid, s->stream));
        ZF_TRY(hipMalloc(&s->ls_cnt, 64));
        ZF_TRY(hipMemsetAsync(s->ls_cnt, 0, 64, s->stream));
    }
    if (zf_is_sparse_mat(desc->kind)) {   // the segment sums of split rows, where the dense kind has its slab
        // (per solver: solves that share a matrix handle may run at the same time on other streams)
        // (K responses: a segment holds K sums)
        if (sp->A.nseg > 0) ZF_TRY(hipMalloc(&s->ws.part_A, sizeof(double) * sp->A.nseg * K));
        if (sp->At.nseg > 0) ZF_TRY(hipMalloc(&s->ws.part_At, sizeof(double) * sp->At.nseg * K));
        // chunk sums of |r(y)|^2 and of |s+ - b|^2 (logistic: of the two losses); ZF_ACCEPT_REMAINDER: and of |s+ - s_y|^2
        ZF_TRY(hipMalloc(&s->row_part, sizeof(double) * 3 * ZF_SPMV_RESID_MAX_CHUNKS));
    }
    if (zf_is_dense_mat(desc->kind)) {
        const int64_t m = desc->m_rows;
        zf_view_slices(zf_mat_of(s), &s->ws.slices, &s->ws.rows_per_slice);
        ZF_TRY(hipMalloc(&s->ws.slab, sizeof(double) * s->ws.slices * n));
        if (desc->world > 1) {   // exchanged vector: A_p x_p (m) for column blocks, A_p^T r_p (n) for row blocks
            const int64_t len = desc->row_sharded ? n : m;
            ZF_TRY(hipMalloc(&s->s_part, sizeof(double) * ((len + 63) & ~int64_t(63))));
            ZF_TRY(hipMalloc(&s->s_all, sizeof(double) * len * desc->world));
        }
        // launch-bound sizes (BASELINE cfg1): two fused launches per trial; ZF_LS_SMALL=0 keeps the general path
        // (the squared loss is written into those two kernels: the logistic kind always takes the general path)
        // (an option set later leaves the path: zf_options_small_open)
        s->small_shape = desc->kind == ZF_PROBLEM_LEAST_SQUARES_L1 && desc->world == 1 && n % LS_SMALL_COLS == 0 && m <= LS_SMALL_MAX_M &&
                         m * n <= LS_SMALL_MAX_ELEMS && zf_aligned16(desc->A) && s->env.ls_small;
        if (s->small_shape) {
            // (twice the workgroups of the rows kernel: their sums of (s+ - b)^2 and - ZF_ACCEPT_REMAINDER - of (s+ - s_y)^2)
            ZF_TRY(hipMalloc(&s->row_part, sizeof(double) * 2 * ((m + ZF_WAVES - 1) / ZF_WAVES)));
            ZF_TRY(hipMalloc(&s->ls_cnt, 64));
            ZF_TRY(hipMemsetAsync(s->ls_cnt, 0, 64, s->stream));
        }
        if (desc->kind == ZF_PROBLEM_LOGISTIC_L1)   // chunk sums of the loss at y and at x+ (read beyond ZF_SPMV_WIDE_RESID_MIN_ROWS rows)
            ZF_TRY(hipMalloc(&s->row_part, sizeof(double) * 2 * ZF_SPMV_RESID_MAX_CHUNKS));
    }
#undef ZF_TRY
    *out = s;
    return ZF_OK;
}

extern "C" int zf_solver_create(zf_solver** out, const zf_problem_desc* desc, const zf_options* opt, void* stream) {
    return zf_solver_create_impl(out, desc, opt, stream, nullptr);
}

extern "C" int zf_solver_create_sparse(zf_solver** out, const zf_problem_desc* desc, const zf_spmat* h, const zf_options* opt, void* stream) {
    ZF_REQUIRE(out && desc && h && opt, "zf_solver_create_sparse: null argument");
    ZF_REQUIRE(zf_is_sparse_mat(desc->kind), "zf_solver_create_sparse: desc->kind must be ZF_PROBLEM_SPARSE_LS_L1 or ZF_PROBLEM_SPARSE_LOGISTIC_L1");
    return zf_solver_create_impl(out, desc, opt, stream, h);
}

// K responses on one CSR matrix (include/zfista_hip.h): the sparse solver of the flattened problem whose two sweeps take
// zf_launch_spmm on the handle as it is
extern "C" int zf_solver_create_sparse_responses(zf_solver** out, const zf_problem_desc* desc, const zf_spmat* h, int32_t K,
                                                 const zf_options* opt, void* stream) {
    ZF_REQUIRE(out && desc && h && opt, "zf_solver_create_sparse_responses: null argument");
    ZF_REQUIRE(zf_is_sparse_mat(desc->kind),
               "zf_solver_create_sparse_responses: desc->kind must be ZF_PROBLEM_SPARSE_LS_L1 or ZF_PROBLEM_SPARSE_LOGISTIC_L1");
    ZF_REQUIRE(K >= 2 && K <= ZF_SPMM_MAX_K, "zf_solver_create_sparse_responses: K must be 2 .. 16");
    ZF_REQUIRE(desc->world == 1, "zf_solver_create_sparse_responses: not for a sharded solve (world > 1)");
    ZF_REQUIRE(opt->accept_mode == ZF_ACCEPT_REFERENCE, "zf_solver_create_sparse_responses: not with ZF_ACCEPT_REMAINDER or ZF_ACCEPT_RESOLVED");
    return zf_solver_create_impl(out, desc, opt, stream, h, K);
}

extern "C" int zf_solver_destroy(zf_solver* s) {
    if (!s) return ZF_OK;
    (void)hipStreamSynchronize(s->stream);
    zf_solver_free_all(s);
    delete s;
    return ZF_OK;
}

// ---- launches ---------------------------------------------------------------
// Bits of zf_solver::part_mask: which shape-specific kernels a step launches (zf_trial_kernel, PART).  Each exits at
// once unless the pass has its shape (zf_pass_claims).
enum {
    ZF_K_FULL = 1,       // PART 0: the full chain
    ZF_K_SHORT = 2,      // PART 1: up to S / 2 fresh trials behind the lagging iterations, materialise-only passes
    ZF_K_GENERAL = 4,    // PART 2 (S = 16): the general body on the shapes of its own (more than S / 2 fresh trials)
    ZF_K_MID = 8,        // PART 3 (S = 16): the branch-free mid chain of s->mid_len trials
    ZF_K_FALLBACK = 16,  // PART 2 as the fallback: every shape the kernel named by s->fb_part / fb_len does NOT run (-1: every shape)
    ZF_K_ALL = ZF_K_FULL | ZF_K_SHORT | ZF_K_GENERAL,   // nothing is known: between them these three run every shape
};

static void zf_launch_trial_kernels(zf_solver* s, const zf_step_args& a, bool grad_inline) {
    const zf_trial_sel v = zf_sel_of(s);
    const int mask = s->part_mask;
    const int grid = s->grid;
    hipStream_t st = s->stream;
    if (!grad_inline) {   // least squares: one trial per pass
        if (s->o.l2 > 0.0) zf_launch_enet(v, s->hist != nullptr, grid, st, a, s->o.l2);
        else if (s->o.pf) {   // (the factors travel in the stream the vector path leaves unused)
            zf_step_args f = a;
            f.p1 = s->o.pf;
            zf_launch_pf(v, s->hist != nullptr, grid, st, f);
        } else if (s->hist) zf_launch_hist(v, false, 1, 0, grid, st, a);
        else zf_launch_vec(v, grid, st, a);
        return;
    }
    if (s->hist) {   // (zf_solver_set_history allowed only chain lengths 1 and 8)
        const int S = s->sub == 8 ? 8 : 1;
        if (mask & ZF_K_FULL) zf_launch_hist(v, true, S, 0, grid, st, a);
        if (S > 1 && (mask & ZF_K_SHORT)) zf_launch_hist(v, true, S, 1, grid, st, a);
        return;
    }
    if (s->sub >= 16) {
        if (mask & ZF_K_FULL) zf_launch_s16_full(v, grid, st, a);
        if (mask & ZF_K_SHORT) zf_launch_s16_short(v, grid, st, a);
        if (mask & ZF_K_MID) zf_launch_s16_mid(v, s->mid_len, grid, st, a);   // (zf_predict_parts checked that it exists)
        if (mask & ZF_K_GENERAL) zf_launch_s16_general(v, grid, st, a);
        if (mask & ZF_K_FALLBACK) {
            zf_step_args f = a;
            f.fb_on = 1;
            f.fb_part = s->fb_part;
            f.fb_len = s->fb_len;
            zf_launch_s16_general(v, grid, st, f);
        }
        return;
    }
    if (mask & ZF_K_FULL) zf_launch_chain(v, s->sub, 0, grid, st, a);
    if (s->sub > 1 && (mask & ZF_K_SHORT)) zf_launch_chain(v, s->sub, 1, grid, st, a);
}

// f(x+) of the trial from s+ = sring[(cur + 1) % 3] (one workgroup); ZF_ACCEPT_REMAINDER: the instantiation that also leaves
// the Taylor remainder R in ls_scal[2]
static void zf_launch_resid_x(zf_solver* s) {
    const zf_problem_desc& d = s->desc;
    if (s->rem)
        hipLaunchKernelGGL(zf_resid_x_rem_kernel, dim3(1), dim3(RESID_BLOCK), 0, s->stream, s->ctl, s->sring, 1, d.b, d.scale,
                           d.m_rows, s->ls_scal + 1, (int)s->opt.nesterov, 0.0, s->ls_scal + 2);
    else
        hipLaunchKernelGGL(zf_resid_x_kernel, dim3(1), dim3(RESID_BLOCK), 0, s->stream, s->ctl, s->sring, 1, d.b, d.scale,
                           d.m_rows, s->ls_scal + 1);
}

// second launch of a step: partials -> pack (+ decide when x is unsharded)
static void zf_launch_finalize(zf_solver* s, bool decide) {
    const zf_problem_desc& d = s->desc;
    zf_finalize_args F;
    F.blk_part = s->blk_part;
    F.nblocks = s->grid;
    F.sub_iters = s->sub;
    F.slice_part = s->slice_part;
    F.cnt = s->fin_cnt;
    for (int k = 0; k < ZF_NPART; ++k) F.scale[k] = 1.0;
    F.scale[3] = zf_g_scale(s);       // g = lam * sum|x| (elastic net: the fourth sum is g(x+) itself, zf_elem_vec_enet)
    F.f_y_ext = nullptr;
    F.f_x_ext = nullptr;
    F.r_ext = nullptr;
    F.contribute_f = 1;
    F.contribute_x = 1;
    if (d.kind == ZF_PROBLEM_DIAG_QUAD_L1) {
        F.scale[0] = 0.5;             // f = 0.5 * sum(d (x-c)^2)
        F.scale[4] = 0.5;
    } else {
        F.f_y_ext = s->ls_scal + 0;   // f(y), f(x+) come from the GEMV side and are replicated
        F.f_x_ext = s->ls_scal + 1;
        if (s->rem) F.r_ext = s->ls_scal + 2;   // (contributed as f(x+) is)
        // column blocks: f is replicated, the x sums are partial; row blocks: the other way round
        F.contribute_f = (d.world == 1 || d.rank == 0 || d.row_sharded) ? 1 : 0;
        F.contribute_x = (d.world == 1 || d.rank == 0 || !d.row_sharded) ? 1 : 0;
    }
    F.pack = s->pack_local;
    F.ctl = s->ctl;
    F.decide = decide ? 1 : 0;
    F.trace = s->trace;
    F.beta_ring = s->beta_ring;
    int wgs = (s->grid + ZF_FIN_THREADS - 1) / ZF_FIN_THREADS;   // no more workgroups than slices of work
    // up to 1024 rows of partials one workgroup (four rows per thread) does it alone: publishing slice sums,
    // the ticket and the last arriver's gather are three dependent round trips to memory (~7 us of a ~20 us kernel)
    if (s->grid <= 1024) wgs = 1;
    if (wgs > ZF_FIN_WGS) wgs = ZF_FIN_WGS;
    if (wgs < 1) wgs = 1;
    if (s->sub == 16) hipLaunchKernelGGL(zf_finalize_kernel<16>, dim3(wgs), dim3(ZF_FIN_THREADS), 0, s->stream, F);
    else if (s->sub == 8) hipLaunchKernelGGL(zf_finalize_kernel<8>, dim3(wgs), dim3(ZF_FIN_THREADS), 0, s->stream, F);
    else if (s->sub == 4) hipLaunchKernelGGL(zf_finalize_kernel<4>, dim3(wgs), dim3(ZF_FIN_THREADS), 0, s->stream, F);
    else if (s->sub == 2) hipLaunchKernelGGL(zf_finalize_kernel<2>, dim3(wgs), dim3(ZF_FIN_THREADS), 0, s->stream, F);
    else hipLaunchKernelGGL(zf_finalize_kernel<1>, dim3(wgs), dim3(ZF_FIN_THREADS), 0, s->stream, F);
}

// the arguments every trial launch shares; the in-kernel finalisation off (fin_mode 0)
static void zf_fill_step_args(const zf_solver* s, zf_step_args& a) {
    const zf_problem_desc& d = s->desc;
    memset(&a, 0, sizeof(a));
    a.ctl = s->ctl;
    a.beta_ring = s->beta_ring;
    for (int k = 0; k < ZF_MAX_RING; ++k) a.xb[k] = s->xb[k < s->ring ? k : 0];
    a.lam = d.lam;
    a.lo = d.box_lo;
    a.hi = d.box_hi;
    a.n = d.n;
    a.tiles_per_wg = s->tiles;
    a.blk_part = s->blk_part;
    a.pass_log = nullptr;
    a.pass_tag = 0;
    a.pass_slot = 0;
    a.hist = s->hist;
    a.hist_cap = s->hist_cap > 0 ? s->hist_cap : 1;
    a.hist_stride = s->hist_stride;
    a.fin_mode = 0;
    a.accept_mode = s->res ? ZF_ACCEPT_RESOLVED : ZF_ACCEPT_REFERENCE;
}

// Groups of the in-kernel finalisation: up to ZF_FIN_GROUPS workgroups reduce as ONE level (every workgroup its
// own "group"); beyond that ceil(grid / ZF_FIN_GROUPS) consecutive workgroups form a group.  A function of the
// grid only.
static void zf_fin_groups(int grid, int* gsz, int* ng) {
    if (grid <= ZF_FIN_GROUPS) {
        *gsz = 1;
        *ng = grid;
        return;
    }
    *gsz = (grid + ZF_FIN_GROUPS - 1) / ZF_FIN_GROUPS;
    *ng = (grid + *gsz - 1) / *gsz;
}

// grids of at most this many workgroups are latency-bound: a second (idle) launch per pass costs more than a slower body
constexpr int ZF_SMALL_GRID = 64;
// tiles per workgroup (a function of n: zf_tiles_for) between which a run of run-ahead passes may START with a mid chain
constexpr int ZF_RA_MID_START_MIN_TILES = 4;    // n >= ~4e6
constexpr int ZF_RA_MID_START_MAX_TILES = 12;   // n <= ~1.2e7

// move the shadow control block past a pass on the assumption that every fresh trial is accepted and nothing
// terminates but max_iter - true for whole chunks in the regime a line search settles in
static void zf_shadow_advance(zf_control& c) {
    const int ring = c.ring_size > 0 ? c.ring_size : 3;
    if (c.pend_status != 0) {
        if (c.lag > 0) zf_commit_chain(&c, c.cur, c.prev, ring, c.lag);
        c.lag = 0;
        if (c.pend_status > 0) c.status = c.pend_status;
        c.pend_status = 0;
        return;
    }
    const int nf = zf_fresh_len(&c);
    c.nit += nf;
    c.total_trials += nf;   // (every trial accepted: zf_pack_stamp of a pass ahead is computed from the shadow)
    if (c.lag + nf > 0) zf_commit_chain(&c, c.cur, c.prev, ring, c.lag + nf);   // (the buffers too: a run-ahead pass is told where to read)
    c.lag = 0;
    if (c.nit >= c.max_iter) c.status = ZF_MAXITER;
}

// The kernels of the next step (ZF_K_* bits; s->mid_len, s->fb_part, s->fb_len beside them), and the shadow control
// block moved past that pass.  The shape rule is the kernel's own (zf_pass_part, zf_fresh_len).
// * nothing known (no poll yet, a host-driven exchange, ZF_SPECULATE=0): the three kernels that between them run every shape;
// * the shadow is what the device holds, or what it holds if no chain broke since the poll: the ONE kernel of that shape;
// * the last chunk saw rejections ("careful"): the first step after the poll is still exact; behind it the optimistic
//   prediction plus the general body as its complement (whatever shape the pass has, exactly one of the two runs it)
//   - on small grids, where an idle launch costs more than the general body loses, the general body alone;
// * the shadow says the solve is over (and the device may not be: a chain broke): every shape again.
// A wrong prediction costs passes that do nothing (no kernel finds its shape, the control block stays as it is) until
// the next poll - never a wrong result.
static int zf_predict_parts(zf_solver* s) {
    // (x sharded: only with the library's communicator, whose decide step checks that every rank's packs are those
    //  of this step - all ranks predict from identical control blocks; a host-driven exchange launches everything)
    if (!s->env.speculate || s->sub <= 1 || !s->shadow_valid || (s->desc.world != 1 && !s->comm) ||
        s->desc.kind != ZF_PROBLEM_DIAG_QUAD_L1)
        return ZF_K_ALL;
    zf_control& c = s->shadow;
    const int S = s->sub;
    const bool s16 = S >= 16;
    if (c.status != ZF_RUNNING) {
        // The shadow has reached the end of the solve.  If the device has not - chains broke; in a solve that crosses
        // the resolution limit of the acceptance test MOST steps are issued in this state, the optimistic shadow being
        // done after max_iter / S of them - any shape may be due: the three kernels that between them run every shape,
        // each on the shapes it runs best (the general body alone took these solves from 5 880 to 4 900 it/s at n = 1e8:
        // it runs the replaying shapes at 1.65 ms against 1.28).  Grids of a few workgroups: the general body alone.
        if (!s16) return ZF_K_ALL;
        if (s->grid > ZF_SMALL_GRID) {   // PART 1 on its shapes, the general body on every other one: two launches, one of them runs
            s->fb_part = 1;
            s->fb_len = 0;
            return ZF_K_SHORT | ZF_K_FALLBACK;
        }
        s->fb_part = -1;
        return ZF_K_FALLBACK;
    }
    const int lag = c.lag;
    const int nf = zf_fresh_len(&c);
    int part = zf_pass_part(S, lag, nf);
    const zf_trial_sel v = zf_sel_of(s);
    if (part == 3 && !zf_have_s16_mid(v, nf)) part = 2;
    int mask = part == 3 ? ZF_K_MID : (1 << part);
    s->mid_len = nf;
    if (s->careful && s->steps_since_poll > 0) {
        // Chains have been breaking: behind the first step the shape is no longer known.  A pass behind a broken chain
        // replays and has at most S / 2 fresh trials, or only materialises (PART 1); a pass with nothing lagging far
        // from max_iter is a full chain (PART 0); near max_iter it may be any length (PART 2 as well).  The general
        // body could run all of them alone - one launch, never idle - but it runs the replaying shapes at 1.65 ms
        // where PART 1 needs 1.28 (n = 1e8, tools/r4_noise.sh): only grids of a few workgroups, where a launch costs
        // more than a body, take it.
        const int64_t left = c.max_iter - c.nit;
        if (!s16) {
            mask = ZF_K_ALL;
        } else if (s->grid <= ZF_SMALL_GRID) {
            s->fb_part = -1;
            mask = ZF_K_FALLBACK;
        } else {
            if (left >= 2 * (int64_t)S) {
                mask = ZF_K_FULL | ZF_K_SHORT;
            } else {   // near max_iter any length may be due: PART 1 on its shapes, the general body on all others
                s->fb_part = 1;
                s->fb_len = 0;
                mask = ZF_K_SHORT | ZF_K_FALLBACK;
            }
        }
    }
    zf_shadow_advance(c);
    return mask;
}

// `stream` waits for what stream2 holds; the next run-ahead pass starts a new run (it reads the real control block)
static int zf_ra_join(zf_solver* s) {
    if (s->ra_b_pending) {
        ZF_HIP(hipEventRecord(s->ra_join, s->stream2));
        ZF_HIP(hipStreamWaitEvent(s->stream, s->ra_join, 0));
        s->ra_b_pending = false;
    }
    if (s->ra_c_pending) {
        ZF_HIP(hipEventRecord(s->ra_join3, s->stream3));
        ZF_HIP(hipStreamWaitEvent(s->stream, s->ra_join3, 0));
        s->ra_c_pending = false;
    }
    s->ra_last = s->ra_last2 = 0;
    s->run_mode = 0;
    return ZF_OK;
}

// A full chain the shadow predicts exactly, as a run-ahead pass (zf_runahead_kernel): behind another one of the same
// run it goes to the other stream and starts while that one is still finalising.  `before`: the shadow control block
// in front of this pass.
static int zf_gather_packs(zf_solver* s, int64_t packs, hipStream_t st, const double* src = nullptr);

// SHARDED (s->comm; round 5): the same kernels, the same flags between workgroups of consecutive passes - but the pass ends
// with its packs (zf_pass_tail: decide == 0), and the all-gather + zf_decide_ahead_kernel of pass p run on a THIRD stream behind
// an event, beside the workgroups of pass p + 1:
//   stream  : T(0)            | [wait decided(0)] T(2) ...
//   stream2 :    T(1) (workgroup j behind workgroup j of T(0))  | [wait decided(1)] T(3) ...
//   stream3 : [wait T(0)] gather, decide(0) | [wait T(1)] gather, decide(1) | ...
// The decide step checks the block against the head the pass ran on (a pass on a head that did not come true is void) and
// publishes the done / good word the kernels read.  What a sharded one-round grid gets out of it is what the unsharded one
// gets: the finalisation, the exchange and the decision of a pass no longer lie between two passes.
static int zf_launch_runahead(zf_solver* s, zf_step_args a, const zf_control& before, int nf, hipEvent_t e0, hipEvent_t e1) {
    const zf_trial_sel v = zf_sel_of(s);
    const bool sharded = s->comm != nullptr;
    const int mode = sharded ? 3 : 1;
    zf_pass_head h;
    h.cur = before.cur;
    h.prev = before.prev;
    h.ring = before.ring_size;
    h.lr = before.lr;
    h.beta_next = 0.0;
    h.nit = before.nit;
    bool chain = s->run_mode == mode && s->ra_last != 0 && a.pass_seq > s->ra_last;
    if (chain) {   // what this pass writes, the pass in flight must not be reading (six buffers in ring order: it never is)
        int f0, f1;
        zf_free_bufs(h.cur, h.prev, h.ring, &f0, &f1);
        const zf_pass_head& q = s->ra_last_head;
        if (f0 == q.cur || f0 == q.prev || f1 == q.cur || f1 == q.prev || h.nit != q.nit + s->ah_last_nf) chain = false;
    }
    int idx = 0;
    if (!chain) {
        int rc = zf_ra_join(s);
        if (rc) return rc;
        // The second stream may go on once the solver's stream has reached this point - NOT earlier: were a per-pass
        // kernel still running in front of this pass, the pass behind it would fill the CUs with waiting workgroups
        // before this one is dispatched, and this one would trickle through the slots they leave (not measured: ruled
        // out by construction).  Recorded before the launch, so the two passes still start together.
        ZF_HIP(hipEventRecord(s->ra_fork, s->stream));
        s->ra_fork_due = true;   // (waited for when - if - a pass of this run goes to the second stream)
        s->ah_run = 0;
    } else {
        idx = 1 - s->ra_last_idx;
        if (idx == 1 && s->ra_fork_due) {
            ZF_HIP(hipStreamWaitEvent(s->stream2, s->ra_fork, 0));
            s->ra_fork_due = false;
        }
    }
    const int k = s->ah_run;   // (number of the pass within its run: the events of a sharded run go by k % 4)
    a.ra_word = s->ra_word;
    a.ra_flags = s->ra_flags;
    a.ra_stats = s->ra_stats;
    a.ra_wait = chain ? s->ra_last : 0;
    a.ra_need = chain ? s->ra_last2 : 0;
    a.ra_spin = s->env.runahead_spin;
    a.ra_head = h;
    if (idx == 1) {
        a.blk_part = s->blk_part2;
        a.grp_part = s->grp_part2;
        a.fin_cnt = s->fin_cnt2;
        a.pack = s->pack2;
    }
    hipStream_t st = idx == 1 ? s->stream2 : s->stream;
    if (sharded) {
        a.decide = 0;
        a.head_nf = nf;
        a.head_stamp = zf_pack_stamp(&before);
        // pass k writes what pass k - 2 (same stream) read, and reuses its rows and packs: that pass must have been DECIDED
        // (third stream) - and as expected, which the kernel checks (ra_need)
        if (k >= 2) ZF_HIP(hipStreamWaitEvent(st, s->ah_evD[(k - 2) & 3], 0));
    }
    if (e0) ZF_HIP(hipEventRecord(e0, st));
    if (!zf_launch_s16_runahead(v, nf, s->grid, st, a)) return zf_fail(ZF_ERR_STATE, "zf_launch_runahead: no run-ahead kernel of that length%s");
    if (e1) ZF_HIP(hipEventRecord(e1, st));
    if (sharded) {
        // exchange and decide step: on the third stream behind an event - but for the LAST pass of a chunk, which nothing
        // runs beside: on the pass's own stream (one hop between queues, ~20 us, less in front of the poll; the decide steps stay
        // in order through the event of the one before, long signalled by then)
        hipStream_t ds = s->stream3;
        if (s->chunk_last) {
            ds = st;
            if (k >= 1) ZF_HIP(hipStreamWaitEvent(ds, s->ah_evD[(k - 1) & 3], 0));
        } else if (e1) {
            ZF_HIP(hipStreamWaitEvent(ds, e1, 0));
        } else {
            ZF_HIP(hipEventRecord(s->ah_evT[k & 3], st));
            ZF_HIP(hipStreamWaitEvent(ds, s->ah_evT[k & 3], 0));
        }
        int rc = zf_gather_packs(s, s->sub, ds, a.pack);
        if (rc) return rc;
        zf_ahead_check H;
        H.head = h;
        H.nf = nf;
        H.seq = a.pass_seq;
        hipLaunchKernelGGL(zf_decide_ahead_kernel, dim3(1), dim3(64), 0, ds, s->ctl, s->pack_all, s->trace, s->beta_ring, s->sub, H,
                           s->ra_word, s->ra_stats, a.pass_log, a.pass_slot, a.pass_tag);
        ZF_HIP(hipEventRecord(s->ah_evD[k & 3], ds));
        if (ds == s->stream3) s->ra_c_pending = true;
        s->ras_passes += 1;
    }
    s->run_mode = mode;
    s->ah_run = k + 1;
    s->ah_last_nf = nf;
    s->ra_last2 = chain ? s->ra_last : 0;
    s->ra_last = a.pass_seq;
    s->ra_last_idx = idx;
    s->ra_last_head = h;
    if (idx == 1) s->ra_b_pending = true;
    s->ra_passes += 1;
    if (chain) s->ra_ahead += 1;
    return ZF_OK;
}


// A full or mid chain the shadow predicts exactly, as a pass AHEAD of its predecessor's decision at kernel granularity:
//   stream  : ... T(p) | T(p+1) | [wait decided(p)] T(p+2) ...        trial kernels back to back, each on the head the
//                                                                     host expects (zf_trial_kernel<..., AHEAD>)
//   stream2 : [wait T(p) done] rows -> packs (-> all-gather) -> decide(p) | ...   beside T(p+1)
// T(p+2) writes the buffers T(p) read; it is launched behind the event of decide(p) and leaves at once unless pass p went
// as expected (ra_need).  decide(p) checks the control block against the head T(p) ran on: a pass on a head that did not
// come true is VOID (zf_decide_ahead).  Nothing waits inside a kernel: every grid size, every sharing of the device.
// `before`: the shadow control block in front of this pass; nf: its fresh trials; part: 0 full chain, 3 mid chain.
static int zf_launch_ahead(zf_solver* s, zf_step_args a, const zf_control& before, int part, int nf, hipEvent_t e0, hipEvent_t e1) {
    const zf_trial_sel v = zf_sel_of(s);
    zf_pass_head h;
    h.cur = before.cur;
    h.prev = before.prev;
    h.ring = before.ring_size;
    h.lr = before.lr;
    h.beta_next = 0.0;
    h.nit = before.nit;
    bool chain = s->run_mode == 2 && s->ra_last != 0 && a.pass_seq > s->ra_last;
    if (chain) {   // what this pass writes, the pass before it must not be reading (six buffers in ring order: it never is)
        int f0, f1;
        zf_free_bufs(h.cur, h.prev, h.ring, &f0, &f1);
        const zf_pass_head& q = s->ra_last_head;
        if (f0 == q.cur || f0 == q.prev || f1 == q.cur || f1 == q.prev || h.nit != q.nit + s->ah_last_nf) chain = false;
    }
    if (!chain) {
        int rc = zf_ra_join(s);   // (the solver's stream now comes behind every decide step so far: the block is what this head was read from)
        if (rc) return rc;
        s->ah_run = 0;
    }
    const int k = s->ah_run;
    // the pass two before this one has been decided (its inputs are this pass's outputs): kernel-granularity dependency
    if (k >= 2) ZF_HIP(hipStreamWaitEvent(s->stream, s->ah_evD[(k - 2) & 3], 0));
    a.ra_word = s->ra_word;
    a.ra_stats = s->ra_stats;
    a.ra_need = chain ? s->ra_last2 : 0;
    a.ra_wait = chain ? s->ra_last : 0;   // (0: the first pass of a run - its kernel checks the block against the head)
    a.ra_head = h;
    a.head_nf = nf;
    a.head_stamp = zf_pack_stamp(&before);
    a.fin_mode = 2;
    a.fin_grid = s->grid;
    a.blk_part = (k & 1) ? s->blk_part2 : s->blk_part;   // rows of pass p are read on stream2 while T(p+1) writes its own
    if (e0) ZF_HIP(hipEventRecord(e0, s->stream));
    if (part == 0) zf_launch_s16_ahead_full(v, s->grid, s->stream, a);
    else if (!zf_launch_s16_ahead_mid(v, nf, s->grid, s->stream, a)) return zf_fail(ZF_ERR_STATE, "zf_launch_ahead: no mid chain of that length%s");
    // "trial kernel p is done": the timing mode's closing event when there is one (a wait captures what the event holds NOW) -
    // every event packet between two trial kernels costs the chain 3-6 us (profiles/r05_event_probe.txt)
    if (e1) {
        ZF_HIP(hipEventRecord(e1, s->stream));
        ZF_HIP(hipStreamWaitEvent(s->stream2, e1, 0));
    } else {
        ZF_HIP(hipEventRecord(s->ah_evT[k & 3], s->stream));
        ZF_HIP(hipStreamWaitEvent(s->stream2, s->ah_evT[k & 3], 0));
    }
    // rows -> packs; unsharded: the deciding wave of the same launch decides
    a.decide = s->comm ? 0 : 1;
    zf_launch_s16_tail(s->stream2, a);
    if (s->comm) {
        int rc = zf_gather_packs(s, s->sub, s->stream2);
        if (rc) return rc;
        zf_ahead_check H;
        H.head = h;
        H.nf = nf;
        H.seq = a.pass_seq;
        hipLaunchKernelGGL(zf_decide_ahead_kernel, dim3(1), dim3(64), 0, s->stream2, s->ctl, s->pack_all, s->trace, s->beta_ring, s->sub, H,
                           s->ra_word, s->ra_stats, a.pass_log, a.pass_slot, a.pass_tag);
    }
    ZF_HIP(hipEventRecord(s->ah_evD[k & 3], s->stream2));
    s->ra_b_pending = true;
    s->run_mode = 2;
    s->ra_last2 = chain ? s->ra_last : 0;
    s->ra_last = a.pass_seq;
    s->ra_last_head = h;
    s->ah_last_nf = nf;
    s->ah_run = k + 1;
    s->ah_passes += 1;
    return ZF_OK;
}

// ---- one trial, by problem kind (zf_launch_trial: the shared prologue and the dispatch) ----
// the separable problem: chains of trials in registers, passes that run ahead of their predecessor's decision
static int zf_trial_diag(zf_solver* s, zf_step_args& a, bool decide_in_launch, bool dry, bool* done_ahead, hipEvent_t e0, hipEvent_t e1) {
    const zf_problem_desc& d = s->desc;
    a.p0 = d.d;
    a.p1 = d.c;
    if (!dry) {
        // the pass finalises itself (zf_pass_tail): packs, and - unsharded - the decide pass, in the same launch
        a.fin_mode = 1;
        zf_fin_groups(s->grid, &a.fin_gsz, &a.fin_ng);
        a.grp_part = s->grp_part;
        a.fin_cnt = s->fin_cnt;
        a.fin_scale_f = 0.5;   // f = 0.5 * sum(d (x-c)^2)
        a.fin_scale_g = d.lam; // g = lam * sum|x|
        a.pack = s->pack_local;
        a.ctl_rw = s->ctl;
        a.decide = (d.world == 1 && decide_in_launch) ? 1 : 0;
        a.trace = s->trace;
        s->pass_seq = s->pass_seq >= 0x7ffffff0 ? 1 : s->pass_seq + 1;
        a.pass_seq = s->pass_seq;
    }
    zf_control before;
    // passes that run ahead of their predecessor's decision: at workgroup granularity (unsharded one-round grids), or
    // at kernel granularity (through the library's communicator; ZF_AHEAD_UNSHARDED: other unsharded grids)
    const bool two_streams = s->stream2 != nullptr && !dry && !s->hist && s->shadow_valid;
    // (behind a communicator only from zf_solver_enqueue_steps, which hands over done_ahead: a caller that drives trial /
    //  exchange / decide itself - zf_solver_enqueue_trial - gets one pass at a time, whatever is attached)
    const bool ra_can = two_streams && s->ra && !s->ra_off &&
                        (s->comm ? (!decide_in_launch && done_ahead != nullptr && s->ra_sharded && s->stream3 != nullptr) : decide_in_launch);
    // (unsharded: what the run-ahead kernel does not take - grids of several rounds, clipped problems, and on its own
    //  grids the mid chains of a shared tail)
    const bool ah_can = two_streams && s->ah && s->ring >= 6 &&
                        (s->comm ? (!decide_in_launch && done_ahead != nullptr) : (decide_in_launch && s->ah_unsharded && d.world == 1));
    const bool have_before = ra_can || ah_can;
    if (have_before) before = s->shadow;
    s->part_mask = (dry || !(decide_in_launch || s->comm)) ? ZF_K_ALL : zf_predict_parts(s);
    // the ONE kernel the shadow predicts (not a pair behind a chunk that saw rejections), nothing lagging
    const bool exact = have_before && before.status == ZF_RUNNING && before.lag == 0 && before.pend_status == 0 &&
                       before.ring_size == s->ring;
    const int nf_before = exact ? zf_fresh_len(&before) : 0;
    bool ra_ok = ra_can && exact && s->part_mask == ZF_K_FULL && nf_before == s->sub && s->grid <= s->ra_cap;
    // A mid chain (the passes of a tail shared by two passes, the tail itself): its own kernel, its own capacity.  Behind a
    // pass of the same run it always runs ahead (the alternative joins the two streams first).  A run that STARTS with
    // one - blocks of K = 20: 10 + 10 - pays only in the middle of the one-round sizes (profiles/r05_runahead_mid_k20_by_size.jsonl:
    // n = 4e6 .. 1e7 +2-3 %, with bench.py's events +4-7 %): below, two launches on one stream cost less than the fork and
    // join of two; above, the chain of <= 10 trials is HBM-bound and its per-pass kernel loads through registers, 4 % faster
    // than the DMA pipeline the coherent loads need.
    const bool mid_run = (s->run_mode == 1 || s->run_mode == 3) && s->ra_last != 0;
    if (ra_can && exact && !ra_ok && s->part_mask == ZF_K_MID && nf_before == s->mid_len && nf_before < ZF_MAX_SUB_ITERS &&
        (mid_run || (s->tiles >= ZF_RA_MID_START_MIN_TILES && s->tiles <= ZF_RA_MID_START_MAX_TILES))) {
        int& cap = s->ra_cap_mid[nf_before];
        if (cap < 0) cap = zf_runahead_capacity(zf_sel_of(s), nf_before);
        ra_ok = cap > 0 && s->grid <= cap;
    }
    const bool ah_ok = ah_can && !ra_ok && exact && ((s->part_mask == ZF_K_FULL && nf_before == s->sub) ||
                                                      (s->part_mask == ZF_K_MID && nf_before == s->mid_len));
    if (s->stream2 && a.pass_seq == 1 && !dry) {   // (the step counter started or wrapped: sequence numbers are compared)
        int rc = zf_ra_join(s);
        if (rc) return rc;
        ZF_HIP(hipMemsetAsync(s->ra_word, 0, 128, s->stream));
        ZF_HIP(hipMemsetAsync(s->ra_flags, 0, sizeof(unsigned) * (s->max_grid + 32), s->stream));
        // (the second stream must not find the flags of the numbers before the wrap: they satisfy every wait)
        ZF_HIP(hipEventRecord(s->ra_fork, s->stream));
        ZF_HIP(hipStreamWaitEvent(s->stream2, s->ra_fork, 0));
    }
    if (!dry) {
        s->steps_since_poll += 1;
        const int shapes = s->part_mask & (s->sub >= 16 ? 31 : s->sub > 1 ? 3 : 1);
        s->steps_issued += 1;
        s->kernels_issued += __builtin_popcount(shapes);
    }
    if (ra_ok) {
        int rc = zf_launch_runahead(s, a, before, nf_before, e0, e1);
        if (rc) return rc;
        if (s->comm && done_ahead) *done_ahead = true;   // (exchange and decide step are enqueued: third stream)
    } else if (ah_ok) {
        int rc = zf_launch_ahead(s, a, before, s->part_mask == ZF_K_FULL ? 0 : 3, nf_before, e0, e1);
        if (rc) return rc;
        if (done_ahead) *done_ahead = true;
    } else {
        if (s->stream2) {
            int rc = zf_ra_join(s);
            if (rc) return rc;
        }
        if (e0) ZF_HIP(hipEventRecord(e0, s->stream));
        zf_launch_trial_kernels(s, a, true);
        if (e1) ZF_HIP(hipEventRecord(e1, s->stream));
    }
    s->part_mask = ZF_K_ALL;
    ZF_HIP(hipGetLastError());
    return ZF_OK;
}

// cache-resident A: the whole trial in two launches (zf_kernels_ls_small.h)
static int zf_trial_ls_small(zf_solver* s, const zf_step_args& a, hipEvent_t e0, hipEvent_t e1) {
    const zf_problem_desc& d = s->desc;
    zf_ls_small_args P;
    P.ctl = s->ctl;
    P.beta_ring = s->beta_ring;
    for (int k = 0; k < 3; ++k) P.xb[k] = s->xb[k];
    P.sring = s->sring;
    P.A = d.A;
    P.b = d.b;
    P.m = d.m_rows;
    P.n = d.n;
    P.scale = d.scale;
    P.lam = d.lam;
    P.lo = d.box_lo;
    P.hi = d.box_hi;
    P.ls_scal = s->ls_scal;
    P.blk_part = s->blk_part;
    P.grid_step = (int)(d.n / LS_SMALL_COLS);
    P.row_part = s->row_part;
    P.row_part_r = s->row_part + (d.m_rows + ZF_WAVES - 1) / ZF_WAVES;
    P.cnt = s->ls_cnt;
    P.pack = s->pack_local;
    P.trace = s->trace;
    P.hist = s->hist;
    P.hist_cap = s->hist_cap > 0 ? s->hist_cap : 1;
    P.hist_stride = s->hist_stride;
    P.pass_log = a.pass_log;
    P.pass_slot = a.pass_slot;
    P.pass_tag = a.pass_tag;
    const bool nest = s->opt.nesterov != 0;
    dim3 gs(P.grid_step), gr((unsigned)((d.m_rows + ZF_WAVES - 1) / ZF_WAVES)), b(ZF_BLOCK);
    if (e0) ZF_HIP(hipEventRecord(e0, s->stream));
    if (nest && s->box) hipLaunchKernelGGL((zf_ls_small_step_kernel<true, true>), gs, b, 0, s->stream, P);
    else if (nest) hipLaunchKernelGGL((zf_ls_small_step_kernel<true, false>), gs, b, 0, s->stream, P);
    else if (s->box) hipLaunchKernelGGL((zf_ls_small_step_kernel<false, true>), gs, b, 0, s->stream, P);
    else hipLaunchKernelGGL((zf_ls_small_step_kernel<false, false>), gs, b, 0, s->stream, P);
    if (e1) ZF_HIP(hipEventRecord(e1, s->stream));
    if (s->rem) hipLaunchKernelGGL(zf_ls_small_rows_kernel<true>, gr, b, 0, s->stream, P);
    else hipLaunchKernelGGL(zf_ls_small_rows_kernel<false>, gr, b, 0, s->stream, P);
    ZF_HIP(hipGetLastError());
    return ZF_OK;
}

// the blur o inverse-Haar operator
static int zf_trial_op(zf_solver* s, zf_step_args& a, bool decide_in_launch, hipEvent_t e0, hipEvent_t e1) {
    const zf_problem_desc& d = s->desc;
    const int64_t m = d.m_rows;
    // TWO launches per trial (unsharded, deciding in the launch): the adjoint kernel - the residual at y formed in its
    // tile load, the PROX STEP in its epilogue (round 5; ZF_OP_FUSE_PROX=0 or a history ring: a launch of its own
    // in between) - and s+ = B W^-1 x+ whose last workgroup sums f(y), f(x+) and the prox step's partials and decides
    // (zf_op_fuse) - instead of resid_y / adjoint / prox / apply / resid_x / finalize
    zf_op_fuse F;
    memset(&F, 0, sizeof(F));
    F.on = 1;
    F.b = d.b;
    for (int k = 0; k < 3; ++k) F.sk[k] = s->sring.p[k];
    F.scale = d.scale;
    F.lam = d.lam;
    F.nesterov = s->opt.nesterov;
    F.part_y = s->row_part;
    F.part_x = s->row_part + s->op_plan.grid;
    F.cnt = s->ls_cnt;
    F.blk_part = s->blk_part;
    F.grid_step = s->grid;
    F.ls_scal = s->ls_scal;
    F.pack = s->pack_local;
    F.ctl_rw = s->ctl;
    F.trace = s->trace;
    F.beta_ring = s->beta_ring;
    // (images whose six arrays - x_k, x_{k-1}, x+, the two cached B W^-1 x, b - no longer fit the 256 MB of memory-side
    //  cache gain nothing: 3072^2 and 4096^2 -0.3 ... -0.7 %, the epilogue's 256-byte pieces of four coefficient
    //  quadrants go to HBM at 0.56 of peak where the separate step streams at 0.74; up to 2048^2: +6 ... +16 %,
    //  profiles/r05_operator_fuse_prox_ab.txt)
    const bool fuse_prox = s->op_plan.fuse_prox && decide_in_launch && !s->hist;
    if (fuse_prox) {
        F.prox = 1;
        F.box = s->box ? 1 : 0;
        F.lo = d.box_lo;
        F.hi = d.box_hi;
        for (int k = 0; k < 3; ++k) F.xb[k] = s->xb[k];
        F.step_part = s->blk_part;
        F.grid_step = s->op_plan.grid;
        F.pass_log = a.pass_log;
        F.pass_slot = a.pass_slot;
        F.pass_tag = a.pass_tag;
        if (e0) ZF_HIP(hipEventRecord(e0, s->stream));
        zf_launch_op_adjoint(s->op_plan, s->stream, zf_op_of(s, s->ctl), nullptr, s->grad, 2 * d.scale, F);
        if (e1) ZF_HIP(hipEventRecord(e1, s->stream));
    } else {
        zf_launch_op_adjoint(s->op_plan, s->stream, zf_op_of(s, s->ctl), nullptr, s->grad, 2 * d.scale, F);
        a.p0 = s->grad;
        a.p1 = nullptr;
        if (e0) ZF_HIP(hipEventRecord(e0, s->stream));
        zf_launch_trial_kernels(s, a, false);
        if (e1) ZF_HIP(hipEventRecord(e1, s->stream));
    }
    if (decide_in_launch) {
        zf_launch_op_apply(s->op_plan, s->stream, zf_op_of(s, s->ctl), s->xb[0], s->xb[1], s->xb[2], s->sring.p[0], s->sring.p[1],
                           s->sring.p[2], 1, F);
    } else {   // (a host-driven step sequence: s+, f(x+) and the finalize launch as for a matrix)
        zf_ring3 xr3 = {{s->xb[0], s->xb[1], s->xb[2]}};
        zf_launch_apply_A(s, s->ctl, xr3, s->sring, 1);
        hipLaunchKernelGGL(zf_resid_x_kernel, dim3(1), dim3(RESID_BLOCK), 0, s->stream, s->ctl, s->sring, 1, d.b,
                           d.scale, m, s->ls_scal + 1);
        zf_launch_finalize(s, false);
    }
    ZF_HIP(hipGetLastError());
    return ZF_OK;
}

// the matrix kinds, dense and CSR, on the two sweeps of zf_matview.h: loss at y, adjoint, prox step, A x+, loss at x+, finalize
static int zf_trial_matrix(zf_solver* s, zf_step_args& a, bool decide_in_launch, hipEvent_t e0, hipEvent_t e1) {
    const zf_problem_desc& d = s->desc;
    const int64_t m = d.m_rows;
    // (the sparse kind times the whole trial - the event pair brackets every launch of it; the dense kind the prox step alone)
    const bool time_whole = (s->sp != nullptr);
    // every loss but the unweighted squared one: psi(y), f(y) and f(x+) from its rows kernels, grad = gfac A^T psi by the same sweeps
    const zf_loss loss = zf_loss_of(s);
    const double gfac = zf_gfac(loss, d.scale);
    if (time_whole && e0) ZF_HIP(hipEventRecord(e0, s->stream));
    // (1) r = A y - b by linearity, f(y); grad = 2 scale A^T r   [only when y changed]
    // (sparse matrices have 1e5 .. 1e7 rows: beyond what one workgroup should walk, the residuals take many - zf_kernels_spmv.h)
    // (K responses: m is m K rows of the interleaved margins - the same threshold on the same count, so the order of f is a
    //  function of the row count alone)
    const bool wide_resid = (d.kind == ZF_PROBLEM_SPARSE_LS_L1 || (s->o.K > 1 && d.kind == ZF_PROBLEM_LEAST_SQUARES_L1)) &&
                            m > ZF_SPMV_WIDE_RESID_MIN_ROWS;
    if (!zf_launch_loss_y(s->stream, s->ctl, s->sring.p[0], s->sring.p[1], s->sring.p[2], d.b, loss, s->resid, d.scale, m,
                          (int)s->opt.nesterov, s->row_part, s->ls_scal + 0)) {
        if (wide_resid)
            zf_launch_spmv_resid_y(s->stream, s->ctl, s->sring.p[0], s->sring.p[1], s->sring.p[2], d.b, s->resid, d.scale, m,
                                   (int)s->opt.nesterov, s->row_part, s->ls_scal + 0);
        else
            hipLaunchKernelGGL(zf_resid_y_kernel, dim3(1), dim3(RESID_BLOCK), 0, s->stream, s->ctl, s->beta_ring, s->sring, d.b,
                               s->resid, d.scale, m, s->ls_scal + 0, (int)s->opt.nesterov);
    }
    // (row blocks: this rank's part 2 scale A_p^T r_p goes to s_part, its combine unguarded; the caller gathers the parts
    //  and zf_solver_enqueue_trial_finish() adds them and runs the rest of the trial)
    const bool rows = d.world > 1 && d.row_sharded;
    zf_launch_adjoint(zf_mat_of(s), s->stream, s->ctl, s->resid, rows ? s->s_part : s->grad, gfac, s->ws, !rows);
    if (rows) {
        // (the prox step of a row-sharded trial runs in zf_solver_enqueue_trial_finish, after the exchange: the
        //  event pair and the log slot taken by zf_launch_trial belong to a launch that does not happen here - give them
        //  back, or zf_collect_timing would read events that were never recorded)
        if (s->timing) {
            s->ev_used -= 1;
            if (a.pass_log) s->launches -= 1;
        }
        ZF_HIP(hipGetLastError());
        return ZF_OK;
    }
    // (2) fused prox step with the gradient vector in HBM
    a.p0 = s->grad;
    a.p1 = nullptr;
    if (!time_whole && e0) ZF_HIP(hipEventRecord(e0, s->stream));
    zf_launch_trial_kernels(s, a, false);
    if (!time_whole && e1) ZF_HIP(hipEventRecord(e1, s->stream));
    // (3) s+ = A x+ ; f(x+).  Sharded x (column blocks): this rank's A_p x_p+ goes to
    // s_part; the caller gathers the parts and zf_solver_enqueue_trial_finish() adds them.
    zf_ring3 xr = {{s->xb[0], s->xb[1], s->xb[2]}};
    zf_ring3 sout = s->sring;
    if (d.world > 1) sout = {{s->s_part, s->s_part, s->s_part}};   // (column blocks; row blocks returned above)
    zf_launch_apply(zf_mat_of(s), s->stream, s->ctl, xr, sout, 1, s->ws);
    if (d.world == 1) {
        if (!zf_launch_loss_x(s->stream, s->ctl, s->sring.p[0], s->sring.p[1], s->sring.p[2], 1, d.b, loss, d.scale, m,
                              s->row_part + ZF_SPMV_RESID_MAX_CHUNKS, s->ls_scal + 1)) {
            if (wide_resid && s->rem && (s->sp != nullptr))   // (ZF_ACCEPT_REMAINDER beyond the threshold: the sparse kind only)
                zf_launch_spmv_resid_x_rem(s->stream, s->ctl, s->sring.p[0], s->sring.p[1], s->sring.p[2], 1, d.b, d.scale, m,
                                           (int)s->opt.nesterov, 0.0, s->row_part + ZF_SPMV_RESID_MAX_CHUNKS,
                                           s->row_part + 2 * ZF_SPMV_RESID_MAX_CHUNKS, s->ls_scal + 1, s->ls_scal + 2);
            else if (wide_resid)   // (the sparse kind, or K responses, beyond the threshold)
                zf_launch_spmv_resid_x(s->stream, s->ctl, s->sring.p[0], s->sring.p[1], s->sring.p[2], 1, d.b, d.scale, m,
                                       s->row_part + ZF_SPMV_RESID_MAX_CHUNKS, s->ls_scal + 1);
            else
                zf_launch_resid_x(s);
        }
        zf_launch_finalize(s, decide_in_launch);
    }
    if (time_whole && e1) ZF_HIP(hipEventRecord(e1, s->stream));
    ZF_HIP(hipGetLastError());
    return ZF_OK;
}

// returns in *done_ahead (if given) whether the step was a pass ahead: tail, exchange and decide are then enqueued too
static int zf_launch_trial(zf_solver* s, bool decide_in_launch, bool dry = false, bool* done_ahead = nullptr) {
    const zf_problem_desc& d = s->desc;
    zf_step_args a;
    zf_fill_step_args(s, a);
    if (done_ahead) *done_ahead = false;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (s->timing && !dry) {
        a.pass_log = s->pass_log;
        a.pass_slot = (int)(s->launches % ZF_PASS_LOG);
        a.pass_tag = (int)(s->launches & 0x7fff) << 16;
        s->launches += 1;
    }
    if (s->timing) {
        if (s->ev_used == s->ev_pool.size()) {
            hipEvent_t x, y;
            ZF_HIP(hipEventCreate(&x));
            ZF_HIP(hipEventCreate(&y));
            s->ev_pool.emplace_back(x, y);
        }
        e0 = s->ev_pool[s->ev_used].first;
        e1 = s->ev_pool[s->ev_used].second;
        s->ev_used++;
    }
    if (d.kind == ZF_PROBLEM_DIAG_QUAD_L1) return zf_trial_diag(s, a, decide_in_launch, dry, done_ahead, e0, e1);
    if (zf_small_open(s) && !dry && decide_in_launch) return zf_trial_ls_small(s, a, e0, e1);
    if (d.kind == ZF_PROBLEM_BLUR_HAAR_L1) return zf_trial_op(s, a, decide_in_launch, e0, e1);
    return zf_trial_matrix(s, a, decide_in_launch, e0, e1);
}

// sharded least squares, second half of a trial: s+ = sum over ranks of A_p x_p+ (rank
// order), f(x+), local pack (f values contributed by rank 0 only: they are replicated)
extern "C" int zf_solver_enqueue_trial_finish(zf_solver* s) {
    ZF_REQUIRE(s && s->initialised, "zf_solver_enqueue_trial_finish: solver not initialised");
    const zf_problem_desc& d = s->desc;
    if (d.kind != ZF_PROBLEM_LEAST_SQUARES_L1 || d.world == 1) return ZF_OK;
    const int64_t m = d.m_rows;
    if (d.row_sharded) {
        // row blocks: grad = sum over ranks (rank order) of the gathered parts, then - on the full,
        // replicated x, identically on every rank - the prox step, this rank's rows of A x+ and its
        // part of f(x+); the pack carries the replicated x sums from rank 0 only
        const int64_t n = d.n;
        zf_ring3 g3 = {{s->grad, s->grad, s->grad}};
        hipLaunchKernelGGL(zf_sum_parts_kernel, dim3(zf_grid_for(n)), dim3(ZF_BLOCK), 0, s->stream, nullptr, s->s_all,
                           (int)d.world, n, g3, -1);
        zf_step_args a;
        zf_fill_step_args(s, a);
        a.p0 = s->grad;
        a.p1 = nullptr;
        zf_launch_trial_kernels(s, a, false);
        zf_ring3 xr = {{s->xb[0], s->xb[1], s->xb[2]}};
        zf_launch_apply(zf_mat_of(s), s->stream, s->ctl, xr, s->sring, 1, s->ws);
        zf_launch_resid_x(s);
        zf_launch_finalize(s, false);
        ZF_HIP(hipGetLastError());
        return ZF_OK;
    }
    hipLaunchKernelGGL(zf_sum_parts_kernel, dim3(zf_grid_for(m)), dim3(ZF_BLOCK), 0, s->stream, s->ctl, s->s_all,
                       (int)d.world, m, s->sring, 1);
    zf_launch_resid_x(s);
    zf_launch_finalize(s, false);
    ZF_HIP(hipGetLastError());
    return ZF_OK;
}

// least squares: with s0 = A x0 in sring[0], finish F(x0): A x_{-1} = A x0, f(x0), g(x0), init pack
static int zf_init_ls_tail(zf_solver* s) {
    const zf_problem_desc& d = s->desc;
    const int64_t n = d.n, m = d.m_rows;
    zf_ring3 s0 = {{s->sring.p[0], s->sring.p[0], s->sring.p[0]}};
    ZF_HIP(hipMemcpyAsync(s->sring.p[2], s->sring.p[0], sizeof(double) * m, hipMemcpyDeviceToDevice, s->stream));
    // (a loss with rows kernels of its own: in the order the loop sums f(x+))
    const bool own_rows = zf_launch_loss_x(s->stream, nullptr, s0.p[0], s0.p[0], s0.p[0], -1, d.b, zf_loss_of(s), d.scale, m, s->row_part,
                                           s->ls_scal + 1);
    if (!own_rows && m > (int64_t)1 << 18) {   // long residuals (the operator problem at image sizes beyond 512 x 512): two launches, many workgroups
        const int wgs = zf_grid_for(m / 8);
        hipLaunchKernelGGL(zf_resid_x_wide_kernel, dim3(wgs), dim3(ZF_BLOCK), 0, s->stream, s0.p[0], d.b, m, s->partials);
        hipLaunchKernelGGL(zf_resid_x_finish_kernel, dim3(1), dim3(RESID_BLOCK), 0, s->stream, s->partials, wgs, d.scale, s->ls_scal + 1);
    } else if (!own_rows) {
        hipLaunchKernelGGL(zf_resid_x_kernel, dim3(1), dim3(RESID_BLOCK), 0, s->stream, nullptr, s0, -1, d.b, d.scale,
                           m, s->ls_scal + 1);
    }
    const int g = zf_grid_for(n);
    if (s->o.l2 > 0.0) {   // (x0 != 0 on every warm start of a path)
        if (s->box)
            hipLaunchKernelGGL(zf_eval_enet_kernel<true>, dim3(g), dim3(ZF_BLOCK), 0, s->stream, s->xb[0], d.lam, 0.5 * s->o.l2, d.box_lo,
                               d.box_hi, n, s->partials);
        else
            hipLaunchKernelGGL(zf_eval_enet_kernel<false>, dim3(g), dim3(ZF_BLOCK), 0, s->stream, s->xb[0], d.lam, 0.5 * s->o.l2, d.box_lo,
                               d.box_hi, n, s->partials);
    } else if (s->o.pf) {
        if (s->box)
            hipLaunchKernelGGL(zf_eval_pf_kernel<true>, dim3(g), dim3(ZF_BLOCK), 0, s->stream, s->xb[0], s->o.pf, d.box_lo, d.box_hi, n, s->partials);
        else
            hipLaunchKernelGGL(zf_eval_pf_kernel<false>, dim3(g), dim3(ZF_BLOCK), 0, s->stream, s->xb[0], s->o.pf, d.box_lo, d.box_hi, n, s->partials);
    } else if (s->box)
        hipLaunchKernelGGL((zf_eval_kernel<false, true>), dim3(g), dim3(ZF_BLOCK), 0, s->stream, s->xb[0], nullptr,
                           nullptr, d.box_lo, d.box_hi, n, s->partials);
    else
        hipLaunchKernelGGL((zf_eval_kernel<false, false>), dim3(g), dim3(ZF_BLOCK), 0, s->stream, s->xb[0], nullptr,
                           nullptr, d.box_lo, d.box_hi, n, s->partials);
    zf_init_args I;
    I.partials = s->partials;
    I.nblocks = g;
    I.f_scale = 0.0;
    I.lam = zf_g_scale(s);
    I.f_ext = s->ls_scal + 1;
    I.pack = s->pack_local;
    I.contribute_g = (d.world == 1 || !d.row_sharded || d.rank == 0) ? 1 : 0;
    hipLaunchKernelGGL(zf_init_finalize_kernel, dim3(1), dim3(ZF_FIN_BLOCK), 0, s->stream, I);
    ZF_HIP(hipGetLastError());
    if (d.world == 1)
        ZF_HIP(hipMemcpyAsync(s->pack_all, s->pack_local, sizeof(double) * ZF_PACK_LEN, hipMemcpyDeviceToDevice,
                              s->stream));
    return ZF_OK;
}

extern "C" int zf_solver_svec_ptrs(zf_solver* s, double** s_part_dev, double** s_all_dev) {
    ZF_REQUIRE(s && s_part_dev && s_all_dev, "zf_solver_svec_ptrs: null argument");
    *s_part_dev = s->s_part;
    *s_all_dev = s->s_all;
    return ZF_OK;
}

extern "C" int zf_solver_set_svec_buffers(zf_solver* s, double* s_part_dev, double* s_all_dev) {
    ZF_REQUIRE(s && s_part_dev && s_all_dev, "zf_solver_set_svec_buffers: null argument");
    ZF_REQUIRE(!s->initialised, "zf_solver_set_svec_buffers: call before zf_solver_enqueue_init");
    ZF_REQUIRE(s->desc.kind == ZF_PROBLEM_LEAST_SQUARES_L1 && s->desc.world > 1,
               "zf_solver_set_svec_buffers: only for sharded least squares (m doubles per rank for column blocks, n for row blocks)");
    if (s->own_svec) {
        if (s->s_part) (void)hipFree(s->s_part);
        if (s->s_all) (void)hipFree(s->s_all);
    }
    s->own_svec = false;
    s->s_part = s_part_dev;
    s->s_all = s_all_dev;
    return ZF_OK;
}

extern "C" int zf_solver_enqueue_init(zf_solver* s, const double* x0_dev) {
    ZF_REQUIRE(s && x0_dev, "zf_solver_enqueue_init: null argument");
    s->init_enqueued = true;
    s->shadow_valid = false;   // (the control block changes behind the host's back: predict again after the next poll)
    const zf_problem_desc& d = s->desc;
    const int64_t n = d.n;
    // x_k = x_{k-1} = y = x0  (proximal_gradient.py:463-465)
    ZF_HIP(hipMemcpyAsync(s->xb[0], x0_dev, sizeof(double) * n, hipMemcpyDeviceToDevice, s->stream));
    ZF_HIP(hipMemcpyAsync(s->xb[s->ring - 1], x0_dev, sizeof(double) * n, hipMemcpyDeviceToDevice, s->stream));
    zf_control c;
    memset(&c, 0, sizeof(c));
    c.lr = s->opt.lr;
    c.tol = s->opt.tol;
    c.tol_internal = s->opt.tol_internal;
    c.decay_rate = s->opt.decay_rate;
    c.max_iter = s->opt.max_iter;
    c.max_backtrack = s->opt.max_backtrack_iter;
    c.status = (s->opt.max_backtrack_iter == 0) ? ZF_BACKTRACK_FAILED : ZF_RUNNING;  // :280,:306
    c.cur = 0;
    c.nesterov = s->opt.nesterov;
    c.deprecated = s->opt.deprecated;
    c.accept_mode = s->accept_mode;
    c.need_grad = 1;
    c.world = d.world;
    c.ring_size = s->ring;
    c.sub_iters = s->sub;
    c.prev = s->ring - 1;   // x_{-1} = x_0 (:463-465)
    c.lag = 0;
    c.pend_status = 0;
    ZF_HIP(hipMemcpyAsync(s->ctl, &c, sizeof(c), hipMemcpyHostToDevice, s->stream));
    ZF_HIP(hipStreamSynchronize(s->stream));   // `c` is a stack object
    zf_init_args I;
    I.partials = s->partials;
    I.lam = d.lam;
    I.pack = s->pack_local;
    I.f_ext = nullptr;
    I.contribute_g = 1;
    const int g = zf_grid_for(n);
    I.nblocks = g;
    if (d.kind == ZF_PROBLEM_DIAG_QUAD_L1) {
        I.f_scale = 0.5;
        if (s->box)
            hipLaunchKernelGGL((zf_eval_kernel<true, true>), dim3(g), dim3(ZF_BLOCK), 0, s->stream, s->xb[0],
                               d.d, d.c, d.box_lo, d.box_hi, n, s->partials);
        else
            hipLaunchKernelGGL((zf_eval_kernel<true, false>), dim3(g), dim3(ZF_BLOCK), 0, s->stream, s->xb[0],
                               d.d, d.c, d.box_lo, d.box_hi, n, s->partials);
    } else {
        // s0 = A x0 (sharded: this rank's A_p x0_p into s_part; zf_solver_enqueue_init_finish()
        // continues after the caller gathered the parts)
        zf_ring3 xr = {{s->xb[0], s->xb[0], s->xb[0]}};
        double* dst = (d.world > 1 && !d.row_sharded) ? s->s_part : s->sring.p[0];   // row blocks: A_p x0 is local
        zf_ring3 s0 = {{dst, dst, dst}};
        zf_launch_apply_A(s, nullptr, xr, s0, -1);
        ZF_HIP(hipGetLastError());
        if (d.world > 1 && !d.row_sharded) return ZF_OK;
        return zf_init_ls_tail(s);
    }
    hipLaunchKernelGGL(zf_init_finalize_kernel, dim3(1), dim3(ZF_FIN_BLOCK), 0, s->stream, I);
    ZF_HIP(hipGetLastError());
    if (d.world == 1)
        ZF_HIP(hipMemcpyAsync(s->pack_all, s->pack_local, sizeof(double) * ZF_PACK_LEN,
                              hipMemcpyDeviceToDevice, s->stream));
    return ZF_OK;
}

// Resume a solve from a saved state: the iterates in buffers `cur`, `prev`
// (device, n each; x_k, x_{k-1} once zf_solver_flush() has run) and the control block
// zf_solver_poll() returned when the state was taken.  Counters, lr, F(x_k), status continue from
// the saved values; buffer indices and the chain geometry are this solver's.  The momentum ring is NOT part of the state: the
// host re-uploads the factors from accepted count `nit` on (zf_solver_set_beta), which also
// resolves beta_next.  Least squares: A x_k and A x_{k-1} are recomputed by the same kernel that
// produced them (unsharded only), so that the resumed solve continues bit for bit.  On the general paths that is
// zf_launch_apply_A for every iterate.  On the fused small-matrix path (zf_small_open) the kernel depends on the iterate's
// accepted count: x_0 got its margins from zf_solver_enqueue_init (zf_gemv_rows_kernel), every later iterate is the x+ of
// an accepted trial of zf_ls_small_rows_kernel - another summation order, other last bits.  Index rule, from saved->nit:
//     A x_k      in the small-matrix order (zf_ls_small_apply_kernel) iff nit >= 1
//     A x_{k-1}  in the small-matrix order                            iff nit >= 2     (nit <= 1: x_{k-1} is x_0)
// zf_small_open alone only says that the shape is eligible: the fused kernels run when a pass decides in its launch
// (zf_solver_enqueue_steps without a communicator).  Behind a communicator (one rank too: zf_solver_set_comm comes before the
// restore) and in the host-driven sequence trial / gather / decide every margin vector comes from the general row sweep, and
// is rebuilt by it: zf_fused_small_runs.
// Whether the passes of this solver run the fused small-matrix kernels (zf_launch_trial: zf_small_open and the decision in the
// launch).  Not behind a communicator, whose steps decide in a launch of their own; not with caller-owned pack buffers
// (zf_solver_set_pack_buffers), the mark of the host-driven sequence zf_solver_enqueue_trial / _trial_finish / _decide.
static bool zf_fused_small_runs(const zf_solver* s) { return zf_small_open(s) && !s->comm && s->own_packs; }

extern "C" int zf_solver_restore(zf_solver* s, const double* xk_dev, const double* xprev_dev,
                                 const zf_control* saved, int64_t saved_bytes) {
    ZF_REQUIRE(s && xk_dev && xprev_dev && saved, "zf_solver_restore: null argument");
    // (nothing is read or written through `s` before the caller's sizes have been checked)
    ZF_REQUIRE(saved_bytes == (int64_t)sizeof(zf_control),
               "zf_solver_restore: saved_bytes differs from zf_sizeof_control() (a control block of another ABI version)");
    const zf_problem_desc& d = s->desc;
    ZF_REQUIRE(d.kind == ZF_PROBLEM_DIAG_QUAD_L1 || d.world == 1,
               "zf_solver_restore: sharded least squares is not supported");
    ZF_REQUIRE(saved->nit >= 0 && saved->lr > 0.0, "zf_solver_restore: implausible control block");
    const int64_t n = d.n;
    s->shadow_valid = false;   // (the control block changes behind the host's back: predict again after the next poll)
    ZF_HIP(hipMemcpyAsync(s->xb[0], xk_dev, sizeof(double) * n, hipMemcpyDeviceToDevice, s->stream));
    ZF_HIP(hipMemcpyAsync(s->xb[s->ring - 1], xprev_dev, sizeof(double) * n, hipMemcpyDeviceToDevice, s->stream));
    zf_control c = *saved;
    c.tol = s->opt.tol;
    c.tol_internal = s->opt.tol_internal;
    c.decay_rate = s->opt.decay_rate;
    c.max_iter = s->opt.max_iter;
    c.max_backtrack = s->opt.max_backtrack_iter;
    c.nesterov = s->opt.nesterov;
    c.deprecated = s->opt.deprecated;
    c.accept_mode = s->accept_mode;   // (this solver's: the test a resumed solve runs is the resuming caller's choice)
    c.cur = 0;
    c.prev = s->ring - 1;
    c.ring_size = s->ring;
    c.world = d.world;
    c.need_grad = 1;
    // lagging iterations (accepted, iterates not stored) travel with the state when the chain
    // geometry can replay them; zf_solver_flush() before the snapshot removes them
    ZF_REQUIRE(saved->lag >= 0 && saved->lag <= 2 * s->sub - 2,
               "zf_solver_restore: the saved state lags more iterations than this chain length can replay "
               "(zf_solver_flush before taking the snapshot)");
    c.sub_iters = s->sub;
    c.pass_seq = 0;   // (step numbers are this solver's own)
    if (c.status == ZF_MAXITER && c.nit < c.max_iter) c.status = ZF_RUNNING;   // a larger max_iter continues (:539)
    // (packs of passes from before the restore must not pass for packs of the restored state: zf_pack_stamp)
    if (s->pack_all)
        ZF_HIP(hipMemsetAsync(s->pack_all, 0, sizeof(double) * ZF_PACK_LEN * s->sub * d.world, s->stream));
    ZF_HIP(hipMemcpyAsync(s->ctl, &c, sizeof(c), hipMemcpyHostToDevice, s->stream));
    ZF_HIP(hipStreamSynchronize(s->stream));   // `c` is a stack object
    if (zf_has_margins(d.kind)) {
        const int at[2] = {0, 2};   // A x_k -> sring[cur], A x_{k-1} -> sring[(cur + 2) % 3]
        for (int k = 0; k < 2; ++k) {
            double* xsrc = s->xb[at[k]];
            double* dst = s->sring.p[at[k]];
            // (small-matrix path: x_k has accepted count nit, x_{k-1} has nit - 1; count 0 - and x_{-1} - is x0, from the row
            //  sweep of the initialisation; every other iterate is the x+ of an accepted trial of the rows kernel)
            if (zf_fused_small_runs(s) && saved->nit >= 1 + k) {
                const dim3 gr((unsigned)((d.m_rows + ZF_WAVES - 1) / ZF_WAVES));
                hipLaunchKernelGGL(zf_ls_small_apply_kernel, gr, dim3(ZF_BLOCK), 0, s->stream, d.A, xsrc, dst, d.m_rows, d.n);
                continue;
            }
            zf_ring3 xr = {{xsrc, xsrc, xsrc}};
            zf_ring3 so = {{dst, dst, dst}};
            zf_launch_apply_A(s, nullptr, xr, so, -1);
        }
        ZF_HIP(hipGetLastError());
    }
    s->initialised = true;
    return ZF_OK;
}

extern "C" int zf_solver_get_x_prev(zf_solver* s, double* x_host, int64_t count) {
    ZF_REQUIRE(s && x_host, "zf_solver_get_x_prev: null argument");
    ZF_REQUIRE(count >= s->desc.n, "zf_solver_get_x_prev: the host buffer holds fewer than n doubles");
    zf_control c;
    ZF_HIP(hipMemcpyAsync(&c, s->ctl, sizeof(c), hipMemcpyDeviceToHost, s->stream));
    ZF_HIP(hipStreamSynchronize(s->stream));
    ZF_HIP(hipMemcpyAsync(x_host, s->xb[c.prev], sizeof(double) * s->desc.n, hipMemcpyDeviceToHost, s->stream));
    ZF_HIP(hipStreamSynchronize(s->stream));
    return ZF_OK;
}

// sharded least squares, second half of the initialisation: s0 = sum of the gathered parts
extern "C" int zf_solver_enqueue_init_finish(zf_solver* s) {
    ZF_REQUIRE(s, "zf_solver_enqueue_init_finish: null solver");
    const zf_problem_desc& d = s->desc;
    if (d.kind != ZF_PROBLEM_LEAST_SQUARES_L1 || d.world == 1 || d.row_sharded) return ZF_OK;
    zf_ring3 s0 = {{s->sring.p[0], s->sring.p[0], s->sring.p[0]}};
    hipLaunchKernelGGL(zf_sum_parts_kernel, dim3(zf_grid_for(d.m_rows)), dim3(ZF_BLOCK), 0, s->stream, nullptr,
                       s->s_all, (int)d.world, d.m_rows, s0, -1);
    ZF_HIP(hipGetLastError());
    return zf_init_ls_tail(s);
}

extern "C" int zf_solver_enqueue_init_commit(zf_solver* s) {
    ZF_REQUIRE(s, "zf_solver_enqueue_init_commit: null solver");
    // column-sharded least squares: f(x0) is replicated (taken once); row blocks and P-diag: partial sums
    const int f_repl = (s->desc.kind == ZF_PROBLEM_LEAST_SQUARES_L1 && !s->desc.row_sharded) ? 1 : 0;
    hipLaunchKernelGGL(zf_init_commit_kernel, dim3(1), dim3(64), 0, s->stream, s->ctl, s->pack_all, f_repl,
                       s->sub * ZF_PACK_LEN);
    ZF_HIP(hipGetLastError());
    s->initialised = true;
    return ZF_OK;
}

extern "C" int zf_solver_set_beta(zf_solver* s, int64_t first, const double* beta_host, int64_t count) {
    ZF_REQUIRE(s && beta_host, "zf_solver_set_beta: null argument");
    ZF_REQUIRE(first >= 0 && count >= 0 && count <= ZF_RING, "zf_solver_set_beta: bad range");
    // ring index = accepted-iteration count % ZF_RING; at most two contiguous pieces
    int64_t done = 0;
    while (done < count) {
        const int64_t pos = (first + done) % ZF_RING;
        int64_t len = count - done;
        if (len > ZF_RING - pos) len = ZF_RING - pos;
        ZF_HIP(hipMemcpyAsync(s->beta_ring + pos, beta_host + done, sizeof(double) * len,
                              hipMemcpyHostToDevice, s->stream));
        done += len;
    }
    hipLaunchKernelGGL(zf_refresh_beta_kernel, dim3(1), dim3(64), 0, s->stream, s->ctl, s->beta_ring);
    ZF_HIP(hipGetLastError());
    ZF_HIP(hipStreamSynchronize(s->stream));   // beta_host may be reused by the caller
    return ZF_OK;
}

extern "C" int zf_solver_enqueue_trial(zf_solver* s) {
    ZF_REQUIRE(s && s->initialised, "zf_solver_enqueue_trial: solver not initialised");
    return zf_launch_trial(s, false);
}

extern "C" int zf_solver_enqueue_decide(zf_solver* s) {
    ZF_REQUIRE(s && s->initialised, "zf_solver_enqueue_decide: solver not initialised");
    // (separable problems finalise in the trial launch and stamp their packs: zf_pack_stamp)
    const int stamped = s->desc.kind == ZF_PROBLEM_DIAG_QUAD_L1 ? 1 : 0;
    hipLaunchKernelGGL(zf_decide_kernel, dim3(1), dim3(64), 0, s->stream, s->ctl, s->pack_all, s->trace,
                       s->beta_ring, s->sub, stamped);
    ZF_HIP(hipGetLastError());
    return ZF_OK;
}

// Streaming return_all (proximal_gradient.py:521-524 keeps every iterate): `hist_dev` is a caller-owned
// ring of `cap_slots` iterates, `stride` doubles apart (>= n, a multiple of 64: slots stay 512-B
// aligned).  From now on every trial stores its iterate x_{k+1} into slot (k + 1) % cap_slots as it
// computes it - the iterates inside a chain of 8 exist nowhere else - so recording costs 8 more bytes
// per element and iteration and no host transfer; x0 (slot 0) is the caller's.  The caller reads slots
// of accepted iterations after a poll and must not let the solve run cap_slots iterations ahead of
// what it still needs.  Chain lengths 1 and 8 only (2 and 4 fall back to 1 at creation).
extern "C" int zf_solver_set_history(zf_solver* s, double* hist_dev, int64_t cap_slots, int64_t stride) {
    ZF_REQUIRE(s && hist_dev && cap_slots >= 2, "zf_solver_set_history: bad argument");
    ZF_REQUIRE(stride >= s->desc.n && stride % 64 == 0 && zf_aligned16(hist_dev),
               "zf_solver_set_history: stride must be >= n and a multiple of 64 doubles, the ring 16-byte aligned");
    ZF_REQUIRE(s->sub == 1 || s->sub == 8, "zf_solver_set_history: chain length must be 1 or 8");
    ZF_REQUIRE(!s->res || s->sub == 1, "zf_solver_set_history: with ZF_ACCEPT_RESOLVED the recording kernels exist for single trials only (sub_iters 1)");
    ZF_REQUIRE(cap_slots > 2 * s->sub, "zf_solver_set_history: the ring must hold more than two chains");
    s->hist = hist_dev;
    s->hist_cap = cap_slots;
    s->hist_stride = stride;
    return ZF_OK;
}

// ---- the eight options of a margins solver (include/zfista_hip.h: the compatibility table; zf_solver_options.h: the rules) ----
// One option into the record: the rule table's verdict, then what the record with the option needs allocated - the dense
// least-squares kind's chunk sums of the loss kernels (2 x ZF_SPMV_RESID_MAX_CHUNKS, as the dense logistic kind holds them; the fused
// small-matrix path's are shorter), a slab for the slices of the column sweep over the new view (regrown only when the new rule
// takes more slices than the present one) - then the assignments.  A refusal or a failed allocation leaves the solver as it was.
static int zf_solver_set_option(zf_solver* s, int opt, const zf_option_arg& a) {
    char why[400];
    const zf_options_base B = zf_base_of(s);
    const int rc = zf_option_check(B, s->o, opt, a, why, sizeof(why));
    if (rc) return zf_fail(rc, "%s%s", why);
    zf_solver_options next = s->o;
    zf_option_store(&next, opt, a);
    double *part = nullptr, *slab = nullptr;
    if (zf_options_need_loss_part(B, next) && !s->loss_part) ZF_HIP(hipMalloc(&part, sizeof(double) * 2 * ZF_SPMV_RESID_MAX_CHUNKS));
    int slices = s->ws.slices;
    int64_t rows_per_slice = s->ws.rows_per_slice;
    if (zf_is_dense_mat(B.kind)) zf_view_slices(zf_mat_of(s, next), &slices, &rows_per_slice);
    const hipError_t e = slices > s->ws.slices ? hipMalloc(&slab, sizeof(double) * slices * B.n) : hipSuccess;
    if (e != hipSuccess) {
        if (part) (void)hipFree(part);
        return zf_fail(ZF_ERR_HIP, "%s: the slab of the column sweep: %s", ZF_OPTION_RULES[opt].entry, hipGetErrorString(e));
    }
    if (part) {
        if (s->row_part) (void)hipFree(s->row_part);
        s->row_part = part;
        s->loss_part = true;
    }
    if (slab) {
        if (s->ws.slab) (void)hipFree(s->ws.slab);
        s->ws.slab = slab;
    }
    s->ws.slices = slices;
    s->ws.rows_per_slice = rows_per_slice;
    s->o = next;
    s->small_shape = zf_options_small_open(B, next);   // (a solver that has left the path stays off it: l2 > 0 and then l2 = 0 runs the l1 kernels of the general path)
    return ZF_OK;
}

// (what each option is and computes: include/zfista_hip.h, section by section; all between create and init)
extern "C" int zf_solver_set_l2(zf_solver* s, double l2) {
    ZF_REQUIRE(s, "zf_solver_set_l2: null argument");
    return zf_solver_set_option(s, ZF_OPT_L2, zf_option_arg{l2, nullptr, 0});
}
extern "C" int zf_solver_set_penalty_factors(zf_solver* s, const double* p_dev) {
    ZF_REQUIRE(s, "zf_solver_set_penalty_factors: null argument");
    return zf_solver_set_option(s, ZF_OPT_PF, zf_option_arg{0.0, p_dev, 0});
}
extern "C" int zf_solver_set_huber(zf_solver* s, double delta) {
    ZF_REQUIRE(s, "zf_solver_set_huber: null argument");
    return zf_solver_set_option(s, ZF_OPT_HUBER, zf_option_arg{delta, nullptr, 0});
}
extern "C" int zf_solver_set_poisson(zf_solver* s) {
    ZF_REQUIRE(s, "zf_solver_set_poisson: null argument");
    return zf_solver_set_option(s, ZF_OPT_POISSON, zf_option_arg{0.0, nullptr, 0});
}
extern "C" int zf_solver_set_multinomial(zf_solver* s) {
    ZF_REQUIRE(s, "zf_solver_set_multinomial: null argument");
    return zf_solver_set_option(s, ZF_OPT_MULTINOMIAL, zf_option_arg{0.0, nullptr, 0});
}
extern "C" int zf_solver_set_row_weights(zf_solver* s, const double* w_dev) {
    ZF_REQUIRE(s, "zf_solver_set_row_weights: null argument");
    return zf_solver_set_option(s, ZF_OPT_ROWW, zf_option_arg{0.0, w_dev, 0});
}
extern "C" int zf_solver_set_matrix_f32(zf_solver* s, const float* A32_dev) {
    ZF_REQUIRE(s, "zf_solver_set_matrix_f32: null argument");
    return zf_solver_set_option(s, ZF_OPT_A32, zf_option_arg{0.0, A32_dev, 0});
}
extern "C" int zf_solver_set_responses(zf_solver* s, int32_t K) {
    ZF_REQUIRE(s, "zf_solver_set_responses: null argument");
    return zf_solver_set_option(s, ZF_OPT_K, zf_option_arg{0.0, nullptr, (int)K});
}

extern "C" int zf_solver_launch_counts(zf_solver* s, int64_t* out, int64_t count) {
    ZF_REQUIRE(s && out, "zf_solver_launch_counts: null argument");
    ZF_REQUIRE(count >= 2, "zf_solver_launch_counts: the output holds fewer than 2 values");
    out[0] = s->steps_issued;
    out[1] = s->kernels_issued;
    if (count >= 4) out[2] = out[3] = 0;   // (ABI 5: the withdrawn multi-pass kernel's counts)
    if (count >= 6) {   // run-ahead passes launched, and those of them launched behind a pass still in flight
        out[4] = s->ra_passes;
        out[5] = s->ra_ahead;
    }
    if (count >= 8) {   // (ABI 6) as of the last poll: waits of run-ahead passes that gave up; void run-ahead passes
        out[6] = s->ra_timeouts;
        out[7] = s->ra_voids;
    }
    if (count >= 10) {  // (ABI 6) passes launched ahead at kernel granularity; of them void, as of the last poll
        out[8] = s->ah_passes;
        out[9] = s->ah_voids;
    }
    if (count >= 11) out[10] = s->ra_off ? 1 : 0;   // run-ahead passes were switched off for this solver after a wait gave up
    if (count >= 12) out[11] = s->second_voids;      // second passes of a run whose first pass left on its head, as of the last poll
    return ZF_OK;
}

// which least-squares kernels zf_solver_create chose for the passes of zf_solver_enqueue_steps (include/zfista_hip.h)
extern "C" int zf_solver_ls_plan(zf_solver* s, int64_t* out, int64_t count) {
    ZF_REQUIRE(s && out, "zf_solver_ls_plan: null argument");
    ZF_REQUIRE(count >= 4, "zf_solver_ls_plan: the output holds fewer than 4 values");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (s->desc.kind == ZF_PROBLEM_BLUR_HAAR_L1) {   // the operator plan (zf_op_plan; fused: as zf_launch_trial decides it)
        const zf_op_plan& pl = s->op_plan;
        out[0] = pl.ty;
        out[1] = pl.sep ? 1 : 0;
        out[2] = pl.persist ? 1 : 0;
        out[3] = (pl.fuse_prox && !s->hist) ? 1 : 0;
        return ZF_OK;
    }
    if (zf_is_sparse_mat(s->desc.kind)) {
        out[0] = 5;
        out[1] = s->sp->A.lanes;
        out[2] = s->sp->At.lanes;
        out[3] = s->sp->A.nsplit + s->sp->At.nsplit;
        if (count >= 6) {   // responses (zf_solver_create_sparse_responses; 1 otherwise)
            out[4] = s->o.K;
            out[5] = 0;
        }
        return ZF_OK;
    }
    if (!zf_is_dense_mat(s->desc.kind)) return ZF_OK;
    const zf_matview V = zf_mat_of(s);
    const bool odd = V.n % 2 != 0;   // (K responses: the parity of the matrix's own column count)
    out[0] = zf_small_open(s) ? 1 : V.mfma ? 2 : odd ? 4 : 3;
    out[1] = zf_small_open(s) ? 1 : odd ? 3 : 2;
    if (V.A32) {   // zf_kernels_gemv_f32.h: 16-byte, 8-byte or scalar loads of floats
        const int w = zf_f32_width(V.n);
        out[0] = w == 4 ? 6 : w == 2 ? 7 : 8;
        out[1] = w == 4 ? 4 : w == 2 ? 5 : 6;
    }
    if (V.k > 1) {   // zf_kernels_mr.h: 16-byte or scalar loads of A, K right-hand sides
        out[0] = odd ? 10 : 9;
        out[1] = odd ? 8 : 7;
    }
    out[2] = s->ws.slices;
    out[3] = s->ws.rows_per_slice;
    if (count >= 6) {   // responses, and the rows a workgroup of the row sweep owns (0: the plain sweeps' own constant)
        out[4] = V.k;
        out[5] = V.k > 1 ? zf_mr_rows_per_wg(V.k) : 0;
    }
    return ZF_OK;
}

extern "C" int zf_solver_sub_iters(zf_solver* s, int32_t* sub_iters) {
    ZF_REQUIRE(s && sub_iters, "zf_solver_sub_iters: null argument");
    *sub_iters = s->sub;
    return ZF_OK;
}

extern "C" int zf_solver_set_max_iter(zf_solver* s, int64_t max_iter) {
    ZF_REQUIRE(s && s->initialised, "zf_solver_set_max_iter: solver not initialised");
    ZF_REQUIRE(max_iter >= 1, "zf_solver_set_max_iter: max_iter must be >= 1");
    if (s->shadow_valid) {   // (mirror of zf_set_max_iter_kernel on the host's expectation)
        zf_control& c = s->shadow;
        c.max_iter = max_iter;
        if (c.status == ZF_MAXITER && c.nit < max_iter) c.status = ZF_RUNNING;
        if (c.pend_status == ZF_MAXITER && c.nit < max_iter) c.pend_status = 0;
    }
    s->opt.max_iter = max_iter;
    hipLaunchKernelGGL(zf_set_max_iter_kernel, dim3(1), dim3(64), 0, s->stream, s->ctl, max_iter);
    ZF_HIP(hipGetLastError());
    return ZF_OK;
}

// world == 1: make the next step materialise lagging iterates (no-op when there are none), so
// that x_k, x_{k-1} are in buffers `cur`, `prev` at the next poll - snapshots, history taps
extern "C" int zf_solver_flush(zf_solver* s) {
    ZF_REQUIRE(s && s->initialised, "zf_solver_flush: solver not initialised");
    if (s->shadow_valid) {   // (mirror of zf_flush_kernel)
        zf_control& c = s->shadow;
        if (c.status == ZF_RUNNING && c.lag > 0 && c.pend_status == 0) c.pend_status = ZF_PEND_FLUSH;
    }
    hipLaunchKernelGGL(zf_flush_kernel, dim3(1), dim3(64), 0, s->stream, s->ctl);
    ZF_HIP(hipGetLastError());
    return ZF_OK;
}

// Attach an RCCL communicator (zf_comm_create; its rank / world must be the descriptor's): from now on
// zf_solver_enqueue_init_all and zf_solver_enqueue_steps issue the exchanges of a sharded step - the
// packed all-gather of the scalar packs (C1), and for column-sharded least squares the all-gather of
// A_p x_p (C2) - themselves, on the solver's stream.  The communicator must outlive the solver.
extern "C" int zf_solver_set_comm(zf_solver* s, zf_comm* comm) {
    ZF_REQUIRE(s && comm, "zf_solver_set_comm: null argument");
    int32_t rank = 0, world = 1;
    int rc = zf_comm_info(comm, &rank, &world);
    if (rc) return rc;
    ZF_REQUIRE(rank == s->desc.rank && world == s->desc.world, "zf_solver_set_comm: rank / world differ from the problem descriptor");
    // passes ahead of their predecessor's decision (zf_launch_ahead) need six iterate buffers: a one-rank solver created with
    // four grows its ring here - which would lose the x0 an enqueued initialisation has already copied into it (and leave the
    // device's control block with the old ring size).  Refused, nothing attached: the caller attaches first, then initialises.
    if (s->ah && s->ring < 6 && (s->init_enqueued || s->initialised))
        return zf_fail(ZF_ERR_STATE, "zf_solver_set_comm: call before zf_solver_enqueue_init / zf_solver_enqueue_init_all / "
                                     "zf_solver_restore (attaching a communicator grows the iterate ring, which holds x0 once the "
                                     "initialisation is enqueued)%s");
    s->comm = comm;
    {   // Thread ranks (the in-process group: several ranks of ONE device) do not hold two passes of every rank at once - sharded
        // run-ahead passes would wait for workgroups that have no slot (correct, counted, switched off at the first poll, but
        // 15 ms per wait): those groups keep to passes ahead, which never wait inside a kernel.  ZF_RUNAHEAD_SHARDED=1 insists.
        zf_comm_desc cd;
        if (world > 1 && s->env.runahead_sharded < 0 && zf_comm_describe(comm, &cd, (int64_t)sizeof(cd)) == ZF_OK && cd.kind == 1)
            s->ra_sharded = false;
    }
    // passes ahead of their predecessor's decision (zf_launch_ahead) need six iterate buffers and the second stream: a
    // one-rank solver was created without knowing that a communicator would follow (before the initialisation only)
    if (s->ah && !s->initialised && (s->ring < 6 || !s->stream2)) {
        ZF_HIP(hipStreamSynchronize(s->stream));
        if (s->ring < 6) {
            const int64_t n_pad = (s->desc.n + 63) & ~int64_t(63);
            double* nb = nullptr;
            if (hipMalloc(&nb, sizeof(double) * 6 * n_pad) == hipSuccess) {
                (void)hipFree(s->xbuf);
                s->xbuf = nb;
                s->ring = 6;
                for (int k = 0; k < s->ring; ++k) s->xb[k] = s->xbuf + k * n_pad;
            } else {
                (void)hipGetLastError();   // (no room for two more iterates: the solve runs one pass at a time)
            }
        }
        if (s->ring >= 6 && zf_second_stream(s) != hipSuccess) {
            (void)hipGetLastError();
            s->ah = false;   // (the sequence trial -> all-gather -> decide on the caller's stream, as without passes ahead)
        }
    }
    return ZF_OK;
}

static int zf_gather_packs(zf_solver* s, int64_t packs, hipStream_t st, const double* src) {
    if (!st) st = s->stream;
    if (!src) src = s->pack_local;
    if (!s->timing) return zf_comm_all_gather(s->comm, src, s->pack_all, packs * ZF_PACK_LEN, st);
    // timed: from "this rank's packs are ready" to "the gathered packs are here" on this rank's stream - the
    // collective itself plus the wait for the slowest rank (zf_solver_exchange_stats)
    if (s->xev_used == s->xev_pool.size()) {
        hipEvent_t x, y;
        ZF_HIP(hipEventCreate(&x));
        ZF_HIP(hipEventCreate(&y));
        s->xev_pool.emplace_back(x, y);
    }
    const auto& ev = s->xev_pool[s->xev_used++];
    ZF_HIP(hipEventRecord(ev.first, st));
    const int rc = zf_comm_all_gather(s->comm, src, s->pack_all, packs * ZF_PACK_LEN, st);
    ZF_HIP(hipEventRecord(ev.second, st));
    return rc;
}
static int zf_gather_svec(zf_solver* s, bool at_init = false) {
    if (s->desc.kind != ZF_PROBLEM_LEAST_SQUARES_L1 || s->desc.world == 1) return ZF_OK;
    if (s->desc.row_sharded) {   // the n-vector A_p^T r_p of a trial; the init has nothing to exchange
        if (at_init) return ZF_OK;
        return zf_comm_all_gather(s->comm, s->s_part, s->s_all, s->desc.n, s->stream);
    }
    return zf_comm_all_gather(s->comm, s->s_part, s->s_all, s->desc.m_rows, s->stream);
}

// the whole initialisation of a solver with a communicator: init, exchanges, commit (world == 1 too)
extern "C" int zf_solver_enqueue_init_all(zf_solver* s, const double* x0_dev) {
    ZF_REQUIRE(s && x0_dev, "zf_solver_enqueue_init_all: null argument");
    int rc = zf_solver_enqueue_init(s, x0_dev);
    if (rc) return rc;
    if (s->comm) {
        if ((rc = zf_gather_svec(s, true))) return rc;
        if ((rc = zf_solver_enqueue_init_finish(s))) return rc;
        // the init pack sits at the head of this rank's pack buffer; ranks are sub x ZF_PACK_LEN apart in
        // pack_all (zf_init_commit_kernel's stride), so the whole buffer is gathered
        if ((rc = zf_gather_packs(s, s->sub, nullptr))) return rc;
    } else {
        ZF_REQUIRE(s->desc.world == 1, "zf_solver_enqueue_init_all: world > 1 needs zf_solver_set_comm");
    }
    return zf_solver_enqueue_init_commit(s);
}

extern "C" int zf_solver_enqueue_steps(zf_solver* s, int64_t steps) {
    ZF_REQUIRE(s && s->initialised, "zf_solver_enqueue_steps: solver not initialised");
    ZF_REQUIRE(s->desc.world == 1 || s->comm, "zf_solver_enqueue_steps: world > 1 needs zf_solver_set_comm "
                                              "(or the caller's own trial / gather / decide sequence)");
    ZF_REQUIRE(steps >= 0 && steps <= ZF_RING, "zf_solver_enqueue_steps: steps must be in [0, ZF_RING]");
    for (int64_t k = 0; k < steps; ++k) {
        int rc;
        if (!s->comm) {
            if ((rc = zf_launch_trial(s, true))) return rc;
            continue;
        }
        // sharded step: trial -> (C2) -> finish -> C1 -> decide; every rank runs the same decide on the
        // same gathered packs, so nothing else is exchanged.  A pass AHEAD (zf_launch_ahead) has enqueued all of it
        // already: finalisation, exchange and decide on the second stream, beside the next pass's trial kernel.
        bool ahead = false;
        s->chunk_last = k + 1 == steps;
        rc = zf_launch_trial(s, false, false, &ahead);
        s->chunk_last = false;
        if (rc) return rc;
        if (ahead) continue;
        if ((rc = zf_gather_svec(s))) return rc;
        if ((rc = zf_solver_enqueue_trial_finish(s))) return rc;
        if ((rc = zf_gather_packs(s, s->sub, nullptr))) return rc;
        if ((rc = zf_solver_enqueue_decide(s))) return rc;
    }
    // everything enqueued on the solver's stream after this call (a poll's copy, a snapshot, another solver's work on
    // the caller's stream) comes behind the passes on the second stream as well
    if (s->stream2) return zf_ra_join(s);
    return ZF_OK;
}

static void zf_set_tiles(zf_solver* s, int tiles) {
    if (tiles < 1) tiles = 1;
    if (tiles > ZF_MAX_TILES_PER_WG) tiles = ZF_MAX_TILES_PER_WG;
    s->tiles = tiles;
    s->grid = (int)((s->ntiles + tiles - 1) / tiles);
}

// Launch geometry of the trial kernel: T interleaved tiles per workgroup.  T decides which
// elements a thread accumulates, hence the rounding of the six sums and, at a knife edge, an
// accept / reject decision - so it is a FUNCTION OF n ONLY (never of a timing measurement, the
// chain length or the device found at run time): the same problem takes the same decisions in every
// process, on every rank layout with equal shard sizes, for every S and after every restore.
// Up to 512 tiles: T = 1.  From there on the grid is a
// round or more deep and T follows the rounds: the chained kernels keep two workgroups per CU resident - 512
// on the 256 CUs of an MI355X - and a workgroup costs its T tiles plus ~0.3 of a tile for its start and
// epilogue (6 S wave reductions), so a pass takes  rounds(T) x (T + 0.3)  tile times with
// rounds = ceil(ceil(tiles / T) / 512); T is the smallest minimiser in 8 .. 24 (n = 1e8: 4 rounds of 24
// tiles instead of 12 of 8: 1.285 -> 1.26 ms per 16-chain pass; the sweep T = 2 .. 96 is in DESIGN.md 4.1;
// n = 1e7: ONE round of 489 workgroups of 10 tiles instead of 611 of 8 - a second round 19 % full: 0.149 ->
// 0.128 ms per 16-chain pass, round 3; round 2 had measured "no faster" through a 22 us finalize launch).
// (Round 1 picked T by timing; tools/tune_trial.hip keeps that experiment.)  ZF_TILES_PER_WG=<n>
// overrides it for experiments and changes the rounding of the sums with it.
static int zf_tiles_for(int64_t ntiles) {
    constexpr int64_t SLOTS = 512;
    if (ntiles <= SLOTS) return 1;
    // (round 4) between one round of single-tile workgroups and 4096 tiles the same cost rule over T = 1 .. 8: whole
    // rounds here too - n = 2e6 runs ONE round of 489 workgroups of 2 tiles instead of two rounds of single tiles - and
    // a grid the device holds at once, which is what lets passes run ahead of each other (zf_runahead_kernel)
    const int t_lo = ntiles < 4096 ? 1 : 8, t_hi = ntiles < 4096 ? 8 : ZF_MAX_TILES_PER_WG;
    int best_t = t_lo;
    double best_cost = 0.0;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int64_t wgs = (ntiles + t - 1) / t;
        const int64_t rounds = (wgs + SLOTS - 1) / SLOTS;
        const double cost = (double)rounds * ((double)t + 0.3);
        if (t == t_lo || cost < best_cost - 1e-9) {
            best_cost = cost;
            best_t = t;
        }
    }
    return best_t;
}

extern "C" int zf_solver_autotune(zf_solver* s, int32_t* chosen_tiles) {
    ZF_REQUIRE(s && s->initialised, "zf_solver_autotune: solver not initialised");
    if (s->env.tiles_per_wg > 0) zf_set_tiles(s, s->env.tiles_per_wg);
    else if (s->desc.kind == ZF_PROBLEM_DIAG_QUAD_L1) zf_set_tiles(s, zf_tiles_for(s->ntiles));
    else zf_set_tiles(s, 1);
    if (chosen_tiles) *chosen_tiles = s->tiles;
    return ZF_OK;
}

extern "C" int zf_solver_pack_ptrs(zf_solver* s, double** pack_local_dev, double** pack_all_dev) {
    ZF_REQUIRE(s && pack_local_dev && pack_all_dev, "zf_solver_pack_ptrs: null argument");
    *pack_local_dev = s->pack_local;
    *pack_all_dev = s->pack_all;
    return ZF_OK;
}

extern "C" int zf_solver_set_pack_buffers(zf_solver* s, double* pack_local_dev, double* pack_all_dev) {
    ZF_REQUIRE(s && pack_local_dev && pack_all_dev, "zf_solver_set_pack_buffers: null argument");
    ZF_REQUIRE(!s->initialised, "zf_solver_set_pack_buffers: call before zf_solver_enqueue_init");
    if (s->pack_local && s->own_packs) (void)hipFree(s->pack_local);
    if (s->pack_all && s->own_packs) (void)hipFree(s->pack_all);
    s->own_packs = false;
    s->pack_local = pack_local_dev;
    s->pack_all = pack_all_dev;
    return ZF_OK;
}

// log_in_mail: the caller (a poll) has just copied the log into the pinned mirror, with the control block and the trace
static int zf_collect_timing(zf_solver* s, bool log_in_mail = false) {
    if (!log_in_mail && s->ev_used > 0) {
        const size_t off = ZF_CTL_SLOT + ZF_TRACE_BYTES;
        ZF_HIP(hipMemcpyAsync(s->mail + off, s->ctl_trace + off, sizeof(int) * ZF_PASS_LOG, hipMemcpyDeviceToHost, s->stream));
        ZF_HIP(hipStreamSynchronize(s->stream));
    }
    const bool have_log = s->ev_used > 0 && s->ev_used <= (size_t)ZF_PASS_LOG &&
                          s->launches - s->first_uncollected == (int64_t)s->ev_used;
    const int* log = reinterpret_cast<const int*>(s->mail + ZF_CTL_SLOT + ZF_TRACE_BYTES);
    for (size_t k = 0; k < s->ev_used; ++k) {
        float ms = 0.f;
        ZF_HIP(hipEventElapsedTime(&ms, s->ev_pool[k].first, s->ev_pool[k].second));
        s->ms_total += ms;
        s->ms_count += 1;
        if (have_log) {
            const int64_t launch = s->first_uncollected + (int64_t)k;
            const int entry = log[launch % ZF_PASS_LOG];
            // the launch found the solve finished and exited: the slot still holds what an earlier launch wrote
            if (entry < 0 || (entry >> 16) != (int)(launch & 0x7fff)) continue;
            const int shape = entry & 0xffff;   // zf_log_shape: fresh trials | lagging iterations << 5 | passes << 10
            if (shape == 0) continue;           // a pass that ran ahead and turned out VOID: the launch ran, its pass does not count
            if (s->records.size() < 65536) s->records.emplace_back(shape, ms);
            const int nf = shape & 31, lag = (shape >> 5) & 31, cnt = (shape >> 10) & 63;
            if (lag == 0 && nf == s->sub) {
                // (a persistent launch ran cnt full-chain passes back to back: its duration counts for all of them)
                s->ms_full += ms;
                s->n_full += cnt > 0 ? cnt : 1;
            } else {
                s->ms_part += ms;
                s->n_part += 1;
                s->fresh_part += nf;
                s->lag_part += lag;
            }
        }
    }
    s->first_uncollected = s->launches;
    s->ev_used = 0;
    for (size_t k = 0; k < s->xev_used; ++k) {
        float ms = 0.f;
        ZF_HIP(hipEventElapsedTime(&ms, s->xev_pool[k].first, s->xev_pool[k].second));
        s->xms_total += ms;
        s->xms_count += 1;
    }
    s->xev_used = 0;
    return ZF_OK;
}

// Timing on: the launches that ran a pass since the last call, one (shape, milliseconds) pair each - shape = fresh trials |
// lagging iterations << 5 | passes of a persistent launch << 10 (zf_log_shape) - oldest first; *count receives how
// many pairs were written (at most cap_pairs; the rest is dropped).  For per-shape kernel statistics (tools/long_run.py).
extern "C" int zf_solver_pass_records(zf_solver* s, double* out, int64_t cap_pairs, int64_t* count) {
    ZF_REQUIRE(out && count && cap_pairs >= 0, "zf_solver_pass_records: bad argument");
    ZF_REQUIRE(s, "zf_solver_pass_records: null solver");
    ZF_HIP(hipStreamSynchronize(s->stream));
    int rc = zf_collect_timing(s);
    if (rc) return rc;
    int64_t k = 0;
    for (; k < (int64_t)s->records.size() && k < cap_pairs; ++k) {
        out[2 * k] = (double)s->records[k].first;
        out[2 * k + 1] = (double)s->records[k].second;
    }
    *count = k;
    s->records.clear();
    return ZF_OK;
}

// Sharded solves with timing on: out[0] = mean ms, out[1] = count of the per-pass pack exchanges since the last
// call - each measured on this rank's stream from "my packs are ready" to "the gathered packs are here" (the
// collective and the wait for the slowest rank).  Resets its window.
extern "C" int zf_solver_exchange_stats(zf_solver* s, double* out, int64_t count) {
    ZF_REQUIRE(out && count >= 2, "zf_solver_exchange_stats: needs a buffer of >= 2 doubles");
    ZF_REQUIRE(s, "zf_solver_exchange_stats: null solver");
    ZF_HIP(hipStreamSynchronize(s->stream));
    int rc = zf_collect_timing(s);
    if (rc) return rc;
    out[0] = s->xms_count ? s->xms_total / (double)s->xms_count : 0.0;
    out[1] = (double)s->xms_count;
    s->xms_total = 0.0;
    s->xms_count = 0;
    return ZF_OK;
}

extern "C" int zf_solver_poll(zf_solver* s, zf_control* ctl_host, int64_t ctl_bytes, double* trace_host,
                              int64_t trace_bytes) {
    ZF_REQUIRE(s && ctl_host, "zf_solver_poll: null argument");
    // (a host built against an older, smaller zf_control is refused - not overrun)
    ZF_REQUIRE(ctl_bytes >= (int64_t)sizeof(zf_control),
               "zf_solver_poll: ctl_bytes is smaller than zf_sizeof_control() (host built against another ABI version?)");
    ZF_REQUIRE(!trace_host || trace_bytes >= (int64_t)(sizeof(double) * ZF_RING * ZF_TRACE_COLS),
               "zf_solver_poll: trace_bytes is smaller than ZF_RING * ZF_TRACE_COLS doubles");
    const size_t trace_len = ZF_TRACE_BYTES;
    const bool with_log = s->ev_used > 0;   // (events were recorded: the kernels logged their pass shapes)
    const size_t want = with_log ? ZF_MAIL_BYTES : trace_host ? ZF_CTL_SLOT + trace_len : ZF_CTL_SLOT;
    ZF_HIP(hipMemcpyAsync(s->mail, s->ctl_trace, want, hipMemcpyDeviceToHost, s->stream));
    ZF_HIP(hipStreamSynchronize(s->stream));
    memcpy(ctl_host, s->mail, sizeof(zf_control));
    if (trace_host) memcpy(trace_host, s->mail + ZF_CTL_SLOT, trace_len);
    {   // what the host now knows about the device: the basis of the next chunk's predictions
        const int64_t rej = ctl_host->total_trials - ctl_host->nit;
        s->careful = s->shadow_valid ? (rej != s->polled_rejections) : (rej != 0);
        s->polled_rejections = rej;
        s->shadow = *ctl_host;
        s->shadow_valid = true;
        s->steps_since_poll = 0;
        // what the passes that ran ahead report (zf_solver::ra_stats).  A wait that gave up means the device does not hold
        // two passes of this solver at once - it is being shared - and every further one would cost its whole limit again:
        // no more run-ahead passes for this solver (passes ahead at kernel granularity never wait and go on)
        const unsigned* st = reinterpret_cast<const unsigned*>(s->mail + ZF_STATS_OFF);
        s->ra_timeouts = st[0];
        s->ra_voids = st[1];
        s->ah_voids = st[2];
        s->second_voids = st[3];
        if (s->ra_timeouts > 0) s->ra_off = true;
    }
    return zf_collect_timing(s, with_log);
}

extern "C" int zf_solver_x_dev(zf_solver* s, const double** x_dev) {
    ZF_REQUIRE(s && x_dev, "zf_solver_x_dev: null argument");
    zf_control c;
    ZF_HIP(hipMemcpyAsync(&c, s->ctl, sizeof(c), hipMemcpyDeviceToHost, s->stream));
    ZF_HIP(hipStreamSynchronize(s->stream));
    *x_dev = s->xb[c.cur];
    return ZF_OK;
}

extern "C" int zf_solver_get_x(zf_solver* s, double* x_host, int64_t count) {
    ZF_REQUIRE(s && x_host, "zf_solver_get_x: null argument");
    ZF_REQUIRE(count >= s->desc.n, "zf_solver_get_x: the host buffer holds fewer than n doubles");
    const double* xd = nullptr;
    int rc = zf_solver_x_dev(s, &xd);
    if (rc) return rc;
    ZF_HIP(hipMemcpyAsync(x_host, xd, sizeof(double) * s->desc.n, hipMemcpyDeviceToHost, s->stream));
    ZF_HIP(hipStreamSynchronize(s->stream));
    return ZF_OK;
}

extern "C" int zf_solver_set_timing(zf_solver* s, int32_t enabled) {
    ZF_REQUIRE(s, "zf_solver_set_timing: null solver");
    s->timing = enabled != 0;
    return ZF_OK;
}

// Trial-kernel durations since the last call, split by the shape of the pass (the kernel logs it):
// out[0], out[1] = mean ms and count of full chains (S fresh trials, nothing replayed);
// out[2], out[3] = mean ms and count of every other pass (shorter chains, replays, materialise-only).
// Launches that found the solve finished are not counted.  Resets the window; call it INSTEAD of
// zf_solver_trial_kernel_ms (which resets the same window).
extern "C" int zf_solver_pass_stats(zf_solver* s, double* out, int64_t count) {
    ZF_REQUIRE(s && out && count >= 4, "zf_solver_pass_stats: needs a buffer of >= 4 doubles");
    ZF_HIP(hipStreamSynchronize(s->stream));
    int rc = zf_collect_timing(s);
    if (rc) return rc;
    out[0] = s->n_full ? s->ms_full / (double)s->n_full : 0.0;
    out[1] = (double)s->n_full;
    out[2] = s->n_part ? s->ms_part / (double)s->n_part : 0.0;
    out[3] = (double)s->n_part;
    s->ms_full = s->ms_part = 0.0;
    s->n_full = s->n_part = 0;
    s->fresh_part = s->lag_part = 0;
    s->ms_total = 0.0;
    s->ms_count = 0;
    return ZF_OK;
}

// The same window with the work of the other passes: out[4] = fresh trials, out[5] = replayed iterations
// they carried in total (a pass of the shared tail before max_iter runs about left / 2 fresh trials, a pass
// after a broken chain replays the lagging iterations first).
extern "C" int zf_solver_pass_stats_ex(zf_solver* s, double* out, int64_t count) {
    ZF_REQUIRE(s && out && count >= 6, "zf_solver_pass_stats_ex: needs a buffer of >= 6 doubles");
    ZF_HIP(hipStreamSynchronize(s->stream));
    int rc = zf_collect_timing(s);
    if (rc) return rc;
    out[4] = (double)s->fresh_part;
    out[5] = (double)s->lag_part;
    return zf_solver_pass_stats(s, out, 4);
}

extern "C" int zf_solver_trial_kernel_ms(zf_solver* s, double* avg_ms, int64_t* launches) {
    ZF_REQUIRE(s && avg_ms && launches, "zf_solver_trial_kernel_ms: null argument");
    ZF_HIP(hipStreamSynchronize(s->stream));
    int rc = zf_collect_timing(s);
    if (rc) return rc;
    *launches = s->ms_count;
    *avg_ms = s->ms_count ? s->ms_total / (double)s->ms_count : 0.0;
    s->ms_total = 0.0;
    s->ms_count = 0;
    s->ms_full = s->ms_part = 0.0;
    s->n_full = s->n_part = 0;
    s->fresh_part = s->lag_part = 0;
    return ZF_OK;
}

// ---------------------------------------------------------------------------
// library / device / memory
// ---------------------------------------------------------------------------
extern "C" int zf_abi_version(void) { return ZF_ABI_VERSION; }
extern "C" const char* zf_last_error(void) { return zf_errbuf; }
extern "C" int64_t zf_sizeof_control(void) { return (int64_t)sizeof(zf_control); }
extern "C" int64_t zf_sizeof_eval_desc(void) { return (int64_t)sizeof(zf_eval_desc); }

extern "C" int zf_device_count(int* count) {
    ZF_REQUIRE(count, "zf_device_count: null argument");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return zf_fail(ZF_ERR_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return ZF_OK;
}
extern "C" int zf_set_device(int device) {
    ZF_HIP(hipSetDevice(device));
    return ZF_OK;
}
extern "C" int zf_malloc(void** dev_ptr, int64_t bytes) {
    ZF_REQUIRE(dev_ptr && bytes >= 0, "zf_malloc: bad argument");
    ZF_HIP(hipMalloc(dev_ptr, (size_t)(bytes > 0 ? bytes : 16)));
    return ZF_OK;
}
extern "C" int zf_free(void* dev_ptr) {
    if (dev_ptr) ZF_HIP(hipFree(dev_ptr));
    return ZF_OK;
}
extern "C" int zf_memcpy_h2d(void* dst, const void* src, int64_t bytes, void* stream) {
    ZF_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    ZF_HIP(hipStreamSynchronize((hipStream_t)stream));
    return ZF_OK;
}
extern "C" int zf_memcpy_d2h(void* dst, const void* src, int64_t bytes, void* stream) {
    ZF_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    ZF_HIP(hipStreamSynchronize((hipStream_t)stream));
    return ZF_OK;
}
extern "C" int zf_memcpy_d2d(void* dst, const void* src, int64_t bytes, void* stream) {
    ZF_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ZF_OK;
}
extern "C" int zf_stream_synchronize(void* stream) {
    ZF_HIP(hipStreamSynchronize((hipStream_t)stream));
    return ZF_OK;
}

extern "C" int zf_decide_host(zf_control* ctl, int64_t ctl_bytes, const double* packs, double* trace) {
    ZF_REQUIRE(ctl && packs && trace, "zf_decide_host: null argument");
    ZF_REQUIRE(ctl_bytes == (int64_t)sizeof(zf_control), "zf_decide_host: ctl_bytes differs from zf_sizeof_control()");
    zf_decide_pass(ctl, packs, trace);
    return ZF_OK;
}

// R = scale sum (s+ - s_y)^2 by the kernels of a ZF_ACCEPT_REMAINDER solver, for margins given in host memory (element-wise tests)
extern "C" int zf_ls_remainder_eval(const double* s_plus_host, const double* s_k_host, const double* s_km1_host, int64_t m, double beta,
                                    int32_t nesterov, double scale, int32_t wide, double* r_out) {
    ZF_REQUIRE(s_plus_host && s_k_host && s_km1_host && r_out && m >= 1, "zf_ls_remainder_eval: bad argument");
    ZF_REQUIRE(wide == 0 || wide == 1, "zf_ls_remainder_eval: wide must be 0 (one workgroup) or 1 (chunked)");
    double *sv = nullptr, *b = nullptr, *part = nullptr, *out = nullptr;
    const int64_t m_pad = (m + 63) & ~int64_t(63);
    int rc = ZF_OK;
    ZF_KEEP_FIRST(hipMalloc(&sv, sizeof(double) * 3 * m_pad));
    ZF_KEEP_FIRST(hipMalloc(&b, sizeof(double) * m_pad));
    ZF_KEEP_FIRST(hipMalloc(&part, sizeof(double) * 2 * ZF_SPMV_RESID_MAX_CHUNKS));
    ZF_KEEP_FIRST(hipMalloc(&out, sizeof(double) * 2));
    if (rc == ZF_OK) {
        const double* src[3] = {s_plus_host, s_k_host, s_km1_host};
        for (int k = 0; k < 3; ++k) ZF_KEEP_FIRST(hipMemcpyAsync(sv + k * m_pad, src[k], sizeof(double) * m, hipMemcpyHostToDevice, nullptr));
        ZF_KEEP_FIRST(hipMemsetAsync(b, 0, sizeof(double) * m_pad, nullptr));   // (f(x+) of the same kernels is not asked for here)
        const zf_ring3 sr = {{sv, sv + m_pad, sv + 2 * m_pad}};
        if (wide)
            zf_launch_spmv_resid_x_rem(nullptr, nullptr, sr.p[0], sr.p[1], sr.p[2], -1, b, scale, m, nesterov ? 1 : 0, beta, part,
                                       part + ZF_SPMV_RESID_MAX_CHUNKS, out + 0, out + 1);
        else
            hipLaunchKernelGGL(zf_resid_x_rem_kernel, dim3(1), dim3(RESID_BLOCK), 0, nullptr, nullptr, sr, -1, b, scale, m, out + 0,
                               nesterov ? 1 : 0, beta, out + 1);
        ZF_KEEP_FIRST(hipGetLastError());
        ZF_KEEP_FIRST(hipMemcpyAsync(r_out, out + 1, sizeof(double), hipMemcpyDeviceToHost, nullptr));
        ZF_KEEP_FIRST(hipStreamSynchronize(nullptr));
    }
    for (void* p : {(void*)sv, (void*)b, (void*)part, (void*)out})
        if (p) (void)hipFree(p);
    return rc;
}

// ---------------------------------------------------------------------------
// the evaluations outside the loop: a view of the caller's matrix (zf_matview.h) and a workspace of the call's own
// ---------------------------------------------------------------------------
// (adjoint false: what z = A x alone needs)
static int zf_sweep_ws_alloc(const zf_matview& V, bool adjoint, zf_sweep_ws* W) {
    int rc = ZF_OK;
    *W = zf_sweep_ws{nullptr, 1, V.m, nullptr, nullptr};
    if (V.csr) {
        if (V.h->A.nseg > 0) ZF_KEEP_FIRST(hipMalloc(&W->part_A, sizeof(double) * V.h->A.nseg * V.k));
        if (adjoint && V.h->At.nseg > 0) ZF_KEEP_FIRST(hipMalloc(&W->part_At, sizeof(double) * V.h->At.nseg * V.k));
    } else if (adjoint) {
        zf_view_slices(V, &W->slices, &W->rows_per_slice);
        ZF_KEEP_FIRST(hipMalloc(&W->slab, sizeof(double) * W->slices * zf_view_cols(V)));
    }
    return rc;
}
static void zf_sweep_ws_free(zf_sweep_ws* W) {
    for (void* p : {(void*)W->slab, (void*)W->part_A, (void*)W->part_At})
        if (p) (void)hipFree(p);
}

// The checks the three evaluation entries share (`who`: the entry's name; `io_ok`: its own host pointers), all before anything
// touches a device or reads through the handle: the descriptor and its size, the matrix, the pointers, the loss, the responses
// (which loss, response count and storage form exist together: the predicates of zf_solver_options.h, which a solver's setters ask too).
// Leaves the loss in *L.
static int zf_desc_args(const char* who, const zf_eval_desc* d, int64_t desc_bytes, bool io_ok, zf_loss* L) {
    if (!d || desc_bytes != (int64_t)sizeof(zf_eval_desc))
        return zf_fail(ZF_ERR_ARG, "%s: null descriptor, or desc_bytes differs from zf_sizeof_eval_desc()%s", who);
    if ((d->A != nullptr) + (d->A32 != nullptr) + (d->spmat != nullptr) != 1)
        return zf_fail(ZF_ERR_ARG, "%s: exactly one of A, A32 and spmat must be set%s", who);
    if (!(d->b && io_ok)) return zf_fail(ZF_ERR_ARG, "%s: null argument%s", who);
    const bool csr = d->spmat != nullptr;
    if (!csr && !(d->m_rows >= 1 && d->n >= 1)) return zf_fail(ZF_ERR_ARG, "%s: bad argument (m_rows and n must be >= 1)%s", who);
    if (!csr && !zf_aligned16(d->A32 ? (const void*)d->A32 : (const void*)d->A)) return zf_fail(ZF_ERR_ARG, "%s: A must be 16-byte aligned%s", who);
    if (!(d->K >= 1 && d->K <= ZF_MR_MAX_K)) return zf_fail(ZF_ERR_ARG, "%s: K must be 1 .. 16%s", who);
    if (d->K > 1 && !zf_loss_takes_responses(d->loss))
        return zf_fail(ZF_ERR_ARG, "%s: with K > 1 the loss must be ZF_LOSS_SQUARE or ZF_LOSS_LOGISTIC (or ZF_LOSS_MULTINOMIAL, whose rows couple the K responses)%s", who);
    if (d->loss == ZF_LOSS_MULTINOMIAL && !zf_multinomial_fits(d->K, d->A32 != nullptr))
        return zf_fail(ZF_ERR_ARG, "%s: ZF_LOSS_MULTINOMIAL needs K = 2 .. 16 responses on A or spmat, not a matrix stored in fp32 (the other codes: ZF_LOSS_SQUARE, "
                       "ZF_LOSS_LOGISTIC, ZF_LOSS_HUBER, ZF_LOSS_POISSON)%s", who);
    if (d->loss != ZF_LOSS_SQUARE && d->loss != ZF_LOSS_LOGISTIC && d->loss != ZF_LOSS_HUBER && d->loss != ZF_LOSS_POISSON &&
        d->loss != ZF_LOSS_MULTINOMIAL)
        return zf_fail(ZF_ERR_ARG, "%s: loss must be ZF_LOSS_SQUARE, ZF_LOSS_LOGISTIC, ZF_LOSS_HUBER, ZF_LOSS_POISSON or ZF_LOSS_MULTINOMIAL%s", who);
    if (d->loss == ZF_LOSS_MULTINOMIAL && !zf_aligned16(d->b)) return zf_fail(ZF_ERR_ARG, "%s: with ZF_LOSS_MULTINOMIAL b must be 16-byte aligned%s", who);
    if (d->loss == ZF_LOSS_HUBER && !(d->delta > 0.0 && d->delta <= DBL_MAX)) return zf_fail(ZF_ERR_ARG, "%s: delta must be finite and > 0%s", who);
    if (!zf_responses_fit_storage(d->K, d->A32 != nullptr)) return zf_fail(ZF_ERR_ARG, "%s: not with K > 1 and a matrix stored in fp32 (the K-response sweeps read an fp64 A)%s", who);
    *L = zf_loss{d->loss, d->loss == ZF_LOSS_HUBER ? d->delta : 0.0, d->w, d->K};
    return ZF_OK;
}
// the matrix of a checked descriptor as the sweeps see it (a handle knows its own sizes)
static zf_matview zf_view_of(const zf_eval_desc* d) {
    if (d->spmat) return zf_matview{nullptr, d->spmat->m, d->spmat->n, d->spmat, true, nullptr, d->K};
    return zf_matview{d->A, d->m_rows, d->n, nullptr, false, d->A32, d->K};
}
// ... and the two evaluations of the certificate add: the capacity of `out` and the three scalars of the penalty
static int zf_gap_args(const char* who, const zf_eval_desc* d, int64_t count, int64_t need) {
    if (count < need) return zf_fail(ZF_ERR_ARG, need == 8 ? "%s: the output buffer holds fewer than 8 doubles%s" : "%s: the output buffer holds fewer than 12 doubles%s", who);
    if (!(d->scale > 0.0 && d->lam >= 0.0 && d->l2 >= 0.0 && d->l2 <= DBL_MAX))
        return zf_fail(ZF_ERR_ARG, "%s: needs scale > 0, lam >= 0 and a finite l2 >= 0%s", who);
    return ZF_OK;
}

// ---------------------------------------------------------------------------
// f and grad f at a host point (callback contract, not the hot loop)
// ---------------------------------------------------------------------------
// f = scale sum w phi(A x) and (grad_out_host != NULL) grad = gfac A^T (w o psi(A x)), on the rows kernels and the sweeps a solver
// of this loss runs.  The column sweep of a dense A is always the VALU one (V.mfma stays false): jac_f has the same bits whatever n % 32 is.
static int zf_point_eval(const zf_matview& V, const double* b_dev, double scale, const zf_loss& L, const double* x_host, double* f_out,
                         double* grad_out_host) {
    const int64_t m = zf_view_rows(V), n = zf_view_cols(V);
    const bool own_rows = L.w || L.kind != ZF_LOSS_SQUARE;   // (zf_launch_loss_y / _x return true)
    double *x = nullptr, *z = nullptr, *grad = nullptr, *fdev = nullptr, *rho = nullptr, *part = nullptr;
    zf_sweep_ws W;
    int rc = zf_sweep_ws_alloc(V, grad_out_host != nullptr, &W);
    ZF_KEEP_FIRST(hipMalloc(&x, sizeof(double) * (n + 2)));   // (the dense rows kernel reads its two-wide tail; nothing reads the pad for CSR)
    ZF_KEEP_FIRST(hipMalloc(&z, sizeof(double) * (m + 2)));
    ZF_KEEP_FIRST(hipMalloc(&fdev, sizeof(double) * 2));
    if (own_rows) {
        ZF_KEEP_FIRST(hipMalloc(&part, sizeof(double) * ZF_SPMV_RESID_MAX_CHUNKS));
        if (grad_out_host) ZF_KEEP_FIRST(hipMalloc(&rho, sizeof(double) * m));
    }
    if (grad_out_host) ZF_KEEP_FIRST(hipMalloc(&grad, sizeof(double) * n));
    if (rc == ZF_OK) {
        ZF_KEEP_FIRST(hipMemcpyAsync(x, x_host, sizeof(double) * n, hipMemcpyHostToDevice, nullptr));
        zf_launch_apply(V, nullptr, nullptr, {{x, x, x}}, {{z, z, z}}, -1, W);
        const bool launched = grad_out_host ? zf_launch_loss_y(nullptr, nullptr, z, z, z, b_dev, L, rho, scale, m, 0, part, fdev)
                                            : zf_launch_loss_x(nullptr, nullptr, z, z, z, -1, b_dev, L, scale, m, part, fdev);
        if (!launched) {   // the unweighted squared loss: f from the residual kernel, then r = z - b in place for the sweep
            zf_ring3 sr = {{z, z, z}};
            hipLaunchKernelGGL(zf_resid_x_kernel, dim3(1), dim3(RESID_BLOCK), 0, nullptr, nullptr, sr, -1, b_dev, scale, m, fdev);
            if (grad_out_host) hipLaunchKernelGGL(zf_axmb_kernel, dim3(zf_grid_for(m)), dim3(ZF_BLOCK), 0, nullptr, z, b_dev, m);
        }
        if (grad_out_host) {
            zf_launch_adjoint(V, nullptr, nullptr, launched ? rho : z, grad, zf_gfac(L, scale), W);
            ZF_KEEP_FIRST(hipMemcpyAsync(grad_out_host, grad, sizeof(double) * n, hipMemcpyDeviceToHost, nullptr));
        }
        ZF_KEEP_FIRST(hipGetLastError());
        ZF_KEEP_FIRST(hipMemcpyAsync(f_out, fdev, sizeof(double), hipMemcpyDeviceToHost, nullptr));
        ZF_KEEP_FIRST(hipStreamSynchronize(nullptr));
    }
    zf_sweep_ws_free(&W);
    for (void* p : {(void*)x, (void*)z, (void*)grad, (void*)fdev, (void*)rho, (void*)part})
        if (p) (void)hipFree(p);
    return rc;
}

// the one entry: any storage, any loss, weighted or not, 1 .. 16 responses (reads neither lam, l2 nor p of the descriptor)
extern "C" int zf_margins_eval(const zf_eval_desc* d, int64_t desc_bytes, const double* x_host, double* f_out, double* grad_out_host) {
    zf_loss L;
    const int rc = zf_desc_args("zf_margins_eval", d, desc_bytes, x_host && f_out, &L);
    return rc ? rc : zf_point_eval(zf_view_of(d), d->b, d->scale, L, x_host, f_out, grad_out_host);
}

// out = out_scale * A in (transpose == 0: in holds n K, out m K doubles) or out_scale * A^T in (in m K, out n K), host vectors,
// response-interleaved: one sweep alone, outside any solve, for element-wise tests.  K = 1: zf_launch_spmv; 2 .. 16: zf_launch_spmm.
extern "C" int zf_spmat_mr_apply(const zf_spmat* h, int32_t transpose, int32_t K, double out_scale, const double* in_host, double* out_host) {
    ZF_REQUIRE(h && in_host && out_host, "zf_spmat_mr_apply: null argument");
    ZF_REQUIRE(K >= 1 && K <= ZF_SPMM_MAX_K, "zf_spmat_mr_apply: K must be 1 .. 16");
    const zf_spmv_mat& M = transpose ? h->At : h->A;
    const int64_t n_in = M.cols * K, n_out = M.rows * K;
    double *in = nullptr, *out = nullptr, *part = nullptr;
    int rc = ZF_OK;
    ZF_KEEP_FIRST(hipMalloc(&in, sizeof(double) * n_in));
    ZF_KEEP_FIRST(hipMalloc(&out, sizeof(double) * n_out));
    if (M.nseg > 0) ZF_KEEP_FIRST(hipMalloc(&part, sizeof(double) * M.nseg * K));
    if (rc == ZF_OK) {
        ZF_KEEP_FIRST(hipMemcpyAsync(in, in_host, sizeof(double) * n_in, hipMemcpyHostToDevice, nullptr));
        const zf_spmv_io io = {{in, in, in}, {out, out, out}};
        if (K == 1) zf_launch_spmv(M, nullptr, nullptr, false, io, -1, out_scale, part);
        else zf_launch_spmm(M, nullptr, nullptr, false, io, -1, out_scale, K, part);
        ZF_KEEP_FIRST(hipGetLastError());
        ZF_KEEP_FIRST(hipMemcpyAsync(out_host, out, sizeof(double) * n_out, hipMemcpyDeviceToHost, nullptr));
        ZF_KEEP_FIRST(hipStreamSynchronize(nullptr));
    }
    for (void* p : {(void*)in, (void*)out, (void*)part})
        if (p) (void)hipFree(p);
    return rc;
}

// f(x) = scale |B W^-1 x - b|^2 and (optionally) jac_f(x) = 2 scale W B (B W^-1 x - b) of the operator problem
// (zf_kernels_op.h; reference: examples/cameraman.ipynb cell 8) for a host vector: the callbacks of
// zfista_amd.problems.BlurHaarL1 outside the device-resident loop.  taps_dev: K x K, b_dev: H x W (device).
extern "C" int zf_op_eval(const double* taps_dev, int32_t k, const double* b_dev, int64_t h, int64_t w, double scale,
                          const double* x_host, double* f_out, double* grad_out_host) {
    ZF_REQUIRE(taps_dev && b_dev && x_host && f_out, "zf_op_eval: null argument");
    ZF_REQUIRE(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && k >= 1 && k % 2 == 1 && k <= ZF_OP_MAXK && k / 2 < h && k / 2 < w,
               "zf_op_eval: the image must be even-sized and the kernel odd, at most 15 wide");
    const int64_t n = h * w;
    zf_problem_desc d;
    memset(&d, 0, sizeof(d));
    d.op_h = h;
    d.op_w = w;
    d.op_k = k;
    d.op_taps = taps_dev;
    double *x = nullptr, *sv = nullptr, *grad = nullptr, *fdev = nullptr, *opbuf = nullptr;
    zf_op_plan pl;
    const double *taps = nullptr, *sep = nullptr;
    int rc = zf_op_prepare(zf_env_read(), taps_dev, (int)k, h, w, nullptr, &pl, &opbuf, &taps, &sep);
    if (rc) return rc;
    ZF_KEEP_FIRST(hipMalloc(&x, sizeof(double) * n));
    ZF_KEEP_FIRST(hipMalloc(&sv, sizeof(double) * n));
    ZF_KEEP_FIRST(hipMalloc(&fdev, sizeof(double) * 2));
    if (grad_out_host) ZF_KEEP_FIRST(hipMalloc(&grad, sizeof(double) * n));
    if (rc == ZF_OK) {
        ZF_KEEP_FIRST(hipMemcpyAsync(x, x_host, sizeof(double) * n, hipMemcpyHostToDevice, nullptr));
        zf_ring3 sr = {{sv, sv, sv}};
        zf_launch_op_apply(pl, nullptr, zf_op_of(d, nullptr, pl, taps, sep), x, x, x, sv, sv, sv, -1, zf_op_no_fuse());
        hipLaunchKernelGGL(zf_resid_x_kernel, dim3(1), dim3(RESID_BLOCK), 0, nullptr, nullptr, sr, -1, b_dev, scale, n, fdev);
        if (grad_out_host) {
            hipLaunchKernelGGL(zf_axmb_kernel, dim3(zf_grid_for(n)), dim3(ZF_BLOCK), 0, nullptr, sv, b_dev, n);
            zf_launch_op_adjoint(pl, nullptr, zf_op_of(d, nullptr, pl, taps, sep), sv, grad, 2 * scale, zf_op_no_fuse());
            ZF_KEEP_FIRST(hipMemcpyAsync(grad_out_host, grad, sizeof(double) * n, hipMemcpyDeviceToHost, nullptr));
        }
        ZF_KEEP_FIRST(hipGetLastError());
        ZF_KEEP_FIRST(hipMemcpyAsync(f_out, fdev, sizeof(double), hipMemcpyDeviceToHost, nullptr));
        ZF_KEEP_FIRST(hipStreamSynchronize(nullptr));
    }
    for (void* p : {(void*)x, (void*)sv, (void*)grad, (void*)fdev, (void*)opbuf})
        if (p) (void)hipFree(p);
    return rc;
}

// ---------------------------------------------------------------------------
// duality gap (zf_kernels_gap.h): standalone at a host point, and at x_k of a live solver
// ---------------------------------------------------------------------------
static int zf_gap_ws_alloc(zf_gap_ws* ws, int64_t m, int64_t n, const zf_loss& L) {
    int rc = ZF_OK;
    ZF_KEEP_FIRST(hipMalloc(&ws->rvec, sizeof(double) * m));
    ZF_KEEP_FIRST(hipMalloc(&ws->g, sizeof(double) * n));
    ZF_KEEP_FIRST(hipMalloc(&ws->part, sizeof(double) * zf_gap_part_len(L)));
    ZF_KEEP_FIRST(hipMalloc(&ws->scal, sizeof(double) * ZF_GAP_SCAL));
    return rc;
}
static void zf_gap_ws_free(zf_gap_ws* ws) {
    for (void* p : {(void*)ws->rvec, (void*)ws->g, (void*)ws->part, (void*)ws->scal})
        if (p) (void)hipFree(p);
    *ws = zf_gap_ws{nullptr, nullptr, nullptr, nullptr};
}

// The gap at a host point x: z = A x, the rows pass of the loss, g = grad f(x) by the column sweep a solver of this shape runs
// (dense: MFMA when n % 32 == 0 and ZF_GEMV_MFMA is not 0 - V.mfma is set here by that rule), the n-passes and the composition; l2 > 0: the elastic-net evaluation.
// scr != NULL (zf_margins_screen): the screen of zf_kernels_screen.h over the call's g behind the same sequence - its four
// scalars follow the eight outputs; scr->cnt and scr->scal are allocated here
// p_dev != NULL: penalty factors - g and the call's copy of x are scaled in place between step 2 and the tails
static int zf_gap_eval_impl(zf_matview V, const double* b_dev, double scale, double lam, double l2, const zf_loss& L,
                            const double* x_host, double* out, int64_t out_count, const zf_screen_req* scr, const double* p_dev = nullptr) {
    const int64_t m = zf_view_rows(V), n = zf_view_cols(V);
    zf_gap_ws ws = {nullptr, nullptr, nullptr, nullptr};
    zf_sweep_ws W = {nullptr, 1, m, nullptr, nullptr};
    double *x = nullptr, *z = nullptr, *scr_scal = nullptr;
    int32_t* scr_cnt = nullptr;
    int rc = zf_gap_ws_alloc(&ws, m, n, L);
    if (rc == ZF_OK) rc = zf_sweep_ws_alloc(V, true, &W);
    if (scr) {
        ZF_KEEP_FIRST(hipMalloc(&scr_scal, sizeof(double) * ZF_SCREEN_SCAL));
        ZF_KEEP_FIRST(hipMalloc(&scr_cnt, sizeof(int32_t) * (ZF_SCREEN_MAX_CHUNKS + 1)));
    }
    ZF_KEEP_FIRST(hipMalloc(&x, sizeof(double) * (n + 2)));
    ZF_KEEP_FIRST(hipMalloc(&z, sizeof(double) * (m + 2)));
    if (rc == ZF_OK) {
        V.mfma = !V.csr && V.k == 1 && n % 32 == 0 && zf_env_read().gemv_mfma;
        ZF_KEEP_FIRST(hipMemcpyAsync(x, x_host, sizeof(double) * n, hipMemcpyHostToDevice, nullptr));
        zf_launch_apply(V, nullptr, nullptr, {{x, x, x}}, {{z, z, z}}, -1, W);
        zf_launch_loss_gap_rows(nullptr, L, z, b_dev, m, scale, ws);
        zf_launch_adjoint(V, nullptr, nullptr, ws.rvec, ws.g, zf_gfac(L, scale), W);
        if (p_dev) zf_launch_gap_pf_scale(nullptr, ws.g, x, p_dev, x, n);
        const zf_gap_out res = zf_launch_loss_gap_tail(nullptr, L, z, b_dev, x, m, n, scale, lam, l2, ws, out_count);
        if (scr) {
            zf_screen_req rq = *scr;
            rq.cnt = scr_cnt;
            rq.scal = scr_scal;
            zf_launch_screen(nullptr, rq, ws.g, ws.scal + ZF_GS_OUT, ws.scal + ZF_GS_ASUM, ws.scal + ZF_GS_RR, m, n, scale, lam,
                             L.kind == ZF_LOSS_LOGISTIC);
        }
        ZF_KEEP_FIRST(hipGetLastError());
        ZF_KEEP_FIRST(hipMemcpyAsync(out, ws.scal + res.slot, sizeof(double) * res.count, hipMemcpyDeviceToHost, nullptr));
        if (scr) ZF_KEEP_FIRST(hipMemcpyAsync(out + 8, scr_scal, sizeof(double) * ZF_SCREEN_SCAL, hipMemcpyDeviceToHost, nullptr));
        ZF_KEEP_FIRST(hipStreamSynchronize(nullptr));
    }
    zf_gap_ws_free(&ws);
    zf_sweep_ws_free(&W);
    for (void* p : {(void*)x, (void*)z, (void*)scr_scal, (void*)scr_cnt})
        if (p) (void)hipFree(p);
    return rc;
}

// The certificate at a host point.  l2 = 0 runs the l1 evaluation - its kernels, its eight values - and writes [8] = [9] = 0 when the
// buffer holds ten; with penalty factors (l2 = 0 only) the tails run on g / p and p o x
extern "C" int zf_margins_gap(const zf_eval_desc* d, int64_t desc_bytes, const double* x_host, double* out, int64_t count) {
    const char* who = "zf_margins_gap";
    zf_loss L;
    int rc = zf_desc_args(who, d, desc_bytes, x_host && out, &L);
    if (rc == ZF_OK) rc = zf_gap_args(who, d, count, 8);
    if (rc) return rc;
    if (d->p && d->l2 > 0.0)
        return zf_fail(ZF_ERR_ARG, "%s: not with penalty factors and l2 > 0 together (the ridge term would need the factors too)%s", who);
    rc = zf_gap_eval_impl(zf_view_of(d), d->b, d->scale, d->lam, d->l2, L, x_host, out, count, nullptr, d->p);
    if (rc == ZF_OK && !(d->l2 > 0.0) && count >= 10) out[8] = out[9] = 0.0;
    return rc;
}

// the gap evaluation followed by the gap-safe screen of its g (zf_kernels_screen.h), l2 = 0 only: out[0 .. 8) as zf_margins_gap - the
// same kernels in the same order, the same bits - then [r, E, r_eff, kept count].  Huber's loss: the rule, the guard and the four
// screen launches are the least-squares kinds' - L = 2 scale, |c|_2 from sum c^2 where they read sum r^2 (the clip is exact and
// 1-Lipschitz; tests/huber_cases.py derives the guard line by line)
extern "C" int zf_margins_screen(const zf_eval_desc* d, int64_t desc_bytes, const double* x_host, double* out, int64_t count,
                                 const double* norms_dev, const double* stats_dev, int64_t max_row, int64_t max_col, uint8_t* keep_dev,
                                 int32_t* index_dev) {
    const char* who = "zf_margins_screen";
    zf_loss L;
    int rc = zf_desc_args(who, d, desc_bytes, x_host && out, &L);
    if (rc == ZF_OK) rc = zf_gap_args(who, d, count, 8 + ZF_SCREEN_SCAL);
    if (rc) return rc;
    // what the rule and its rounding guard are not built for
    if (d->loss == ZF_LOSS_POISSON) return zf_fail(ZF_ERR_ARG, "%s: not for ZF_LOSS_POISSON (exp is not globally Lipschitz: no gap-safe radius)%s", who);
    if (d->loss == ZF_LOSS_MULTINOMIAL) return zf_fail(ZF_ERR_ARG, "%s: not for ZF_LOSS_MULTINOMIAL (screening needs per-response gaps)%s", who);
    if (d->w) return zf_fail(ZF_ERR_ARG, "%s: not with row weights (w)%s", who);
    if (d->p) return zf_fail(ZF_ERR_ARG, "%s: not with penalty factors (p)%s", who);
    if (d->l2 > 0.0) return zf_fail(ZF_ERR_ARG, "%s: not with l2 > 0%s", who);
    if (d->A32) return zf_fail(ZF_ERR_ARG, "%s: not for a matrix stored in fp32 (A32)%s", who);
    if (d->K > 1) return zf_fail(ZF_ERR_ARG, "%s: not with K > 1 responses%s", who);
    if (!d->spmat && d->n > 0x7fffffffLL) return zf_fail(ZF_ERR_ARG, "%s: n must be below 2^31 (index_dev holds int32)%s", who);
    if (!(norms_dev && stats_dev && keep_dev && index_dev)) return zf_fail(ZF_ERR_ARG, "%s: null argument%s", who);
    if (d->spmat && (max_row < 0 || max_col < 0)) return zf_fail(ZF_ERR_ARG, "%s: the longest row and column must be >= 0%s", who);
    const zf_screen_req rq = {norms_dev, stats_dev, d->spmat ? max_row : d->n, d->spmat ? max_col : d->m_rows, keep_dev, index_dev, nullptr, nullptr};
    return zf_gap_eval_impl(zf_view_of(d), d->b, d->scale, d->lam, 0.0, L, x_host, out, 8, &rq);
}

// The gap at x_k of a live solver, on its stream: the margins A x_k are the ring's (no sweep over A), the dual candidate goes
// to the call's own m-vector, g = grad f(x_k) through the solver's column sweep to its own n-vector.  Reads the iterate and
// margin rings, A, b; writes only its workspace (and the scratch of a sweep - the slab, the segment sums of split rows -
// which holds nothing between two launches of a sweep): r, the gradient, ls_scal and the control block stay as they are,
// so a solve interrupted here - also between a rejected trial and its retry - continues bit for bit.
extern "C" int zf_solver_duality_gap(zf_solver* s, double* out, int64_t count) {
    ZF_REQUIRE(s && out, "zf_solver_duality_gap: null argument");
    ZF_REQUIRE(count >= 8, "zf_solver_duality_gap: the output buffer holds fewer than 8 doubles");
    const zf_problem_desc& d = s->desc;
    ZF_REQUIRE(zf_is_dense_mat(d.kind) || zf_is_sparse_mat(d.kind),
               "zf_solver_duality_gap: only for ZF_PROBLEM_LEAST_SQUARES_L1, ZF_PROBLEM_SPARSE_LS_L1, ZF_PROBLEM_LOGISTIC_L1 and "
               "ZF_PROBLEM_SPARSE_LOGISTIC_L1 (the dual of the other kinds is not built)");
    ZF_REQUIRE(d.world == 1, "zf_solver_duality_gap: not for a sharded solve (world > 1): the dual point needs the whole A^T grad phi");
    ZF_REQUIRE(!s->box, "zf_solver_duality_gap: not with a finite box (the dual of the boxed problem is another one)");
    ZF_REQUIRE(d.scale > 0.0, "zf_solver_duality_gap: needs scale > 0");
    if (!s->initialised) return zf_fail(ZF_ERR_STATE, "zf_solver_duality_gap: solver not initialised%s%s");
    const int64_t m = d.m_rows, n = d.n;
    const zf_loss loss = zf_loss_of(s);
    if (!s->gap.scal) {
        int rc = zf_gap_ws_alloc(&s->gap, m, n, loss);
        if (rc) {
            zf_gap_ws_free(&s->gap);
            return rc;
        }
    }
    if (s->o.pf && !s->gap_xp) ZF_HIP(hipMalloc(&s->gap_xp, sizeof(double) * n));
    zf_control c;
    ZF_HIP(hipMemcpyAsync(&c, s->ctl, sizeof(c), hipMemcpyDeviceToHost, s->stream));
    ZF_HIP(hipStreamSynchronize(s->stream));
    if (c.lag != 0 || c.cur < 0 || c.cur > 2) return zf_fail(ZF_ERR_STATE, "zf_solver_duality_gap: the iterate ring does not hold x_k%s%s");
    const double* x = s->xb[c.cur];
    const double* z = s->sring.p[c.cur];   // A x_k: every path of these kinds keeps it there (the fused small-matrix path too)
    const zf_gap_ws& ws = s->gap;
    zf_launch_loss_gap_rows(s->stream, loss, z, d.b, m, d.scale, ws);
    zf_launch_adjoint(zf_mat_of(s), s->stream, nullptr, ws.rvec, ws.g, zf_gfac(loss, d.scale), s->ws);
    if (s->o.pf) {   // (penalty factors: the tails run on g / p and p o x_k)
        zf_launch_gap_pf_scale(s->stream, ws.g, x, s->o.pf, s->gap_xp, n);
        x = s->gap_xp;
    }
    const zf_gap_out res = zf_launch_loss_gap_tail(s->stream, loss, z, d.b, x, m, n, d.scale, d.lam, s->o.l2, ws, count);
    ZF_HIP(hipGetLastError());
    ZF_HIP(hipMemcpyAsync(out, ws.scal + res.slot, sizeof(double) * res.count, hipMemcpyDeviceToHost, s->stream));
    ZF_HIP(hipStreamSynchronize(s->stream));
    return ZF_OK;
}
