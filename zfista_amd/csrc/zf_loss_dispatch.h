// zf_loss_dispatch.h - where the loss of a margins problem is chosen (gfx950 only; host code, no kernel in here).
//
// f(x) = scale sum_i w_i phi((A x)_i) with phi the squared, the logistic, Huber's or the Poisson loss of one margin, or the
// multinomial loss of the K margins of a row, with or without per-row weights w.
// Four places of a solve depend on which: the rows kernel that forms psi(y) and f(y), the one that forms f(x+), the one that
// forms the dual candidate of the duality gap, and the launches that compose the gap.  Each is ONE function below, over
// zf_kernels_loss.h, zf_kernels_gap.h and zf_kernels_softmax.h (include this header after those three); every site of
// zf_solver.hip calls these and names no loss.
//
// To add a loss that is a row function of one margin: one ZF_LOSS_* enumerator (include/zfista_hip.h), one arm of zf_loss_row
// and of zf_launch_loss_rows_of; for the certificate one rows kernel (an arm of zf_launch_gap_rows in zf_kernels_gap.h or of
// zf_launch_gap_alpha_rows below) and the choice of its composition kernel in zf_launch_loss_gap_tail.
// To add a loss that couples several margins of a row (the multinomial one is the model): zf_loss_row does not apply - the loss
// brings a rows kernel of its own with the ring, guard and shape logic of zf_loss_rows_kernel and a launcher over zf_rows_call
// (which carries the response count), and takes an arm of zf_launch_loss_rows_of, of zf_launch_loss_gap_rows (step 1 by the
// trial's rows kernel outside the loop), of zf_launch_gap_alpha_rows and of zf_gfac; zf_loss::K tells its kernels how many
// flattened entries make a row.
#pragma once

struct zf_loss {
    int kind;          // ZF_LOSS_SQUARE / ZF_LOSS_LOGISTIC / ZF_LOSS_HUBER / ZF_LOSS_POISSON / ZF_LOSS_MULTINOMIAL
    double delta;      // Huber's threshold; 0 for the others
    const double* w;   // per-row weights (device, m doubles), or NULL
    int K;             // the responses (1 .. 16): the margins a row of ZF_LOSS_MULTINOMIAL couples; unread by the other losses
};

// the losses whose rows need alpha and leave their two sums in ZF_GS_KL / ZF_GS_ENT: step 1 by the trial's rows kernel, the
// compositions' "logistic" arm
static inline bool zf_loss_kl_like(const zf_loss& L) {
    return L.kind == ZF_LOSS_LOGISTIC || L.kind == ZF_LOSS_POISSON || L.kind == ZF_LOSS_MULTINOMIAL;
}

// grad f = zf_gfac A^T psi: 2 scale for the squared and Huber's loss (psi = r, clip(r)), scale for the logistic (psi = rho), the
// Poisson (psi = exp(z) - b) and the multinomial one (psi = softmax(z) - y)
static inline double zf_gfac(const zf_loss& L, double scale) { return zf_loss_kl_like(L) ? scale : 2 * scale; }

template <int LOSS, int WHICH>
static inline void zf_launch_loss_rows_w(hipStream_t st, const zf_rows_call& c) {
    if (c.w) zf_launch_loss_rows<LOSS, true, WHICH>(st, c);
    else zf_launch_loss_rows<LOSS, false, WHICH>(st, c);
}

// the rows pass of a trial (WHICH 0: at y, 1: at x+) for the loss of L.
// false: the unweighted squared loss - it has no rows kernel of its own, nothing was launched and the site runs its own form.
template <int WHICH>
static inline bool zf_launch_loss_rows_of(hipStream_t st, const zf_loss& L, const zf_rows_call& c) {
    if (L.kind == ZF_LOSS_LOGISTIC) zf_launch_loss_rows_w<ZF_LOSS_LOGISTIC, WHICH>(st, c);
    else if (L.kind == ZF_LOSS_HUBER) zf_launch_loss_rows_w<ZF_LOSS_HUBER, WHICH>(st, c);
    else if (L.kind == ZF_LOSS_POISSON) zf_launch_loss_rows_w<ZF_LOSS_POISSON, WHICH>(st, c);
    else if (L.kind == ZF_LOSS_MULTINOMIAL) zf_launch_softmax_rows<WHICH>(st, c);
    else if (L.w) zf_launch_loss_rows<ZF_LOSS_SQUARE, true, WHICH>(st, c);
    else return false;
    return true;
}

// psi(y) -> r and f(y) -> *f_out, y = the extrapolated margins of the ring (ctl given) or s0 itself (ctl NULL); false as above
static inline bool zf_launch_loss_y(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2,
                                    const double* b, const zf_loss& L, double* r, double scale, int64_t m, int nesterov, double* part,
                                    double* f_out) {
    return zf_launch_loss_rows_of<0>(st, L, {ctl, ctl, s0, s1, s2, 0, b, L.w, r, scale, L.delta, m, nesterov, part, f_out, L.K});
}

// f(x+) -> *f_out from the margins in ring slot `slot` (-1: s0 as given, outside the loop); false as above
static inline bool zf_launch_loss_x(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2, int slot,
                                    const double* b, const zf_loss& L, double scale, int64_t m, double* part, double* f_out) {
    return zf_launch_loss_rows_of<1>(st, L, {ctl, slot >= 0 ? ctl : nullptr, s0, s1, s2, slot, b, L.w, nullptr, scale, L.delta, m, 0, part, f_out, L.K});
}

// doubles of chunk results a gap evaluation of this loss needs in zf_gap_ws::part (Huber's rows pass holds a fourth row)
static inline int zf_gap_part_len(const zf_loss& L) { return L.kind == ZF_LOSS_HUBER ? ZF_GAP_PART_HUBER : ZF_GAP_PART; }

// step 1 of a gap evaluation: the dual candidate (without its factor) -> ws.rvec and the row sums that need no alpha
static inline void zf_launch_loss_gap_rows(hipStream_t st, const zf_loss& L, const double* z, const double* b, int64_t m, double scale,
                                           const zf_gap_ws& ws) {
    if (zf_loss_kl_like(L))   // psi and f by the rows kernel of a trial, called outside the loop
        zf_launch_loss_y(st, nullptr, z, z, z, b, L, ws.rvec, scale, m, 0, ws.part + 2 * ZF_GAP_MAX_CHUNKS, ws.scal + ZF_GS_F);
    else zf_launch_gap_rows(st, L.kind == ZF_LOSS_HUBER, z, b, L.w, m, scale, L.delta, ws);
}

// step 5 of a gap evaluation: the rows pass that needs alpha - the logistic, the Poisson and the multinomial loss; none for the
// others, whose composition reads the sums of step 1
static inline void zf_launch_gap_alpha_rows(hipStream_t st, const zf_loss& L, const double* z, const double* b, int64_t m,
                                            const zf_gap_ws& ws) {
    const double* w = L.w;
    int chunks;
    if (L.kind == ZF_LOSS_MULTINOMIAL) chunks = zf_launch_gap_softmax(st, L.K, z, b, w, m, ws);
    else if (L.kind == ZF_LOSS_LOGISTIC)
        chunks = zf_launch_rows_shapes(st, w ? zf_gap_kl_kernel<ZF_ROWS_BLOCK, true> : zf_gap_kl_kernel<ZF_ROWS_BLOCK, false>,
                                       w ? zf_gap_kl_kernel<ZF_BLOCK, true> : zf_gap_kl_kernel<ZF_BLOCK, false>, m, z, b, w, m, ws.part, ws.scal);
    else if (L.kind == ZF_LOSS_POISSON)
        chunks = zf_launch_rows_shapes(st, w ? zf_gap_poisson_kernel<ZF_ROWS_BLOCK, true> : zf_gap_poisson_kernel<ZF_ROWS_BLOCK, false>,
                                       w ? zf_gap_poisson_kernel<ZF_BLOCK, true> : zf_gap_poisson_kernel<ZF_BLOCK, false>, m, z, b, w, m, ws.part,
                                       ws.scal);
    else return;
    if (chunks) zf_launch_gap_sum_finish(st, ws, chunks, ZF_GS_KL, ZF_GS_ENT);
}

// where the composition left the results in ws.scal, and how many of them a caller's buffer of out_count doubles takes
struct zf_gap_out {
    int slot, count;
};

// steps 3 .. 6, with g = grad f(x) in ws.g: the n-passes, the rows that need alpha, and the composition of the l1 (l2 = 0) or
// the elastic-net evaluation.  The Poisson and the multinomial rows leave their two sums where the logistic ones do: the same
// composition arm.
static inline zf_gap_out zf_launch_loss_gap_tail(hipStream_t st, const zf_loss& L, const double* z, const double* b, const double* x,
                                                 int64_t m, int64_t n, double scale, double lam, double l2, const zf_gap_ws& ws,
                                                 int64_t out_count) {
    const int enet = l2 > 0.0 ? 1 : 0, logistic = zf_loss_kl_like(L) ? 1 : 0;
    zf_launch_gap_npasses(st, x, n, lam, l2, ws);
    zf_launch_gap_alpha_rows(st, L, z, b, m, ws);
    if (L.kind == ZF_LOSS_HUBER) hipLaunchKernelGGL(zf_gap_compose_huber_kernel, dim3(1), dim3(64), 0, st, enet, scale, lam, l2, ws.scal);
    else if (enet) hipLaunchKernelGGL(zf_gap_compose_enet_kernel, dim3(1), dim3(64), 0, st, logistic, scale, lam, l2, ws.scal);
    else hipLaunchKernelGGL(zf_gap_compose_kernel, dim3(1), dim3(64), 0, st, logistic, scale, lam, ws.scal);
    if (enet) return zf_gap_out{ZF_GS_OUT_ENET, out_count >= 10 ? 10 : 8};   // (ten values when the caller's buffer holds them)
    return zf_gap_out{ZF_GS_OUT, 8};
}
