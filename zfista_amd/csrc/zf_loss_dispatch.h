// zf_loss_dispatch.h - where the loss of a margins problem is chosen (gfx950 only; host code, no kernel in here).
//
// f(x) = scale sum_i w_i phi((A x)_i) with phi the squared, the logistic, Huber's or the Poisson loss, with or without per-row weights w.
// Four places of a solve depend on which: the rows kernel that forms psi(y) and f(y), the one that forms f(x+), the one that
// forms the dual candidate of the duality gap, and the launches that compose the gap.  Each is ONE function below, over the
// launchers of zf_kernels_loss.h / zf_kernels_gap.h / zf_kernels_huber.h / zf_kernels_poisson.h / zf_kernels_wloss.h (include
// this header after those five); every site of zf_solver.hip calls these and names no loss.
//
// To add a loss: one ZF_LOSS_* enumerator (include/zfista_hip.h), its kernels, and one arm in each of the four launchers.
#pragma once

struct zf_loss {
    int kind;          // ZF_LOSS_SQUARE / ZF_LOSS_LOGISTIC / ZF_LOSS_HUBER / ZF_LOSS_POISSON
    double delta;      // Huber's threshold; 0 for the others
    const double* w;   // per-row weights (device, m doubles), or NULL
};

// grad f = zf_gfac A^T psi: 2 scale for the squared and Huber's loss (psi = r, clip(r)), scale for the logistic (psi = rho) and
// the Poisson one (psi = exp(z) - b)
static inline double zf_gfac(const zf_loss& L, double scale) {
    return L.kind == ZF_LOSS_LOGISTIC || L.kind == ZF_LOSS_POISSON ? scale : 2 * scale;
}

// psi(y) -> r and f(y) -> *f_out, y = the extrapolated margins of the ring (ctl given) or s0 itself (ctl NULL).
// false: the unweighted squared loss - it has no rows kernel of its own, nothing was launched and the site runs its own form.
static inline bool zf_launch_loss_y(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2,
                                    const double* b, const zf_loss& L, double* r, double scale, int64_t m, int nesterov, double* part,
                                    double* f_out) {
    if (L.w) zf_launch_wloss_y(st, ctl, s0, s1, s2, b, L.w, r, scale, L.kind, L.delta, m, nesterov, part, f_out);
    else if (L.kind == ZF_LOSS_LOGISTIC) zf_launch_logit_y(st, ctl, s0, s1, s2, b, r, scale, m, nesterov, part, f_out);
    else if (L.kind == ZF_LOSS_HUBER) zf_launch_huber_y(st, ctl, s0, s1, s2, b, r, scale, L.delta, m, nesterov, part, f_out);
    else if (L.kind == ZF_LOSS_POISSON) zf_launch_poisson_y(st, ctl, s0, s1, s2, b, r, scale, m, nesterov, part, f_out);
    else return false;
    return true;
}

// f(x+) -> *f_out from the margins in ring slot `slot` (-1: s0 as given, outside the loop); false as above
static inline bool zf_launch_loss_x(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2, int slot,
                                    const double* b, const zf_loss& L, double scale, int64_t m, double* part, double* f_out) {
    if (L.w) zf_launch_wloss_x(st, ctl, s0, s1, s2, slot, b, L.w, scale, L.kind, L.delta, m, part, f_out);
    else if (L.kind == ZF_LOSS_LOGISTIC) zf_launch_logit_x(st, ctl, s0, s1, s2, slot, b, scale, m, part, f_out);
    else if (L.kind == ZF_LOSS_HUBER) zf_launch_huber_x(st, ctl, s0, s1, s2, slot, b, scale, L.delta, m, part, f_out);
    else if (L.kind == ZF_LOSS_POISSON) zf_launch_poisson_x(st, ctl, s0, s1, s2, slot, b, scale, m, part, f_out);
    else return false;
    return true;
}

// doubles of chunk results a gap evaluation of this loss needs in zf_gap_ws::part (Huber's rows pass holds a fourth row)
static inline int zf_gap_part_len(const zf_loss& L) { return L.kind == ZF_LOSS_HUBER ? ZF_GAP_PART_HUBER : ZF_GAP_PART; }

// step 1 of a gap evaluation: the dual candidate (without its factor) -> ws.rvec and the row sums that need no alpha
static inline void zf_launch_loss_gap_rows(hipStream_t st, const zf_loss& L, const double* z, const double* b, int64_t m, double scale,
                                           const zf_gap_ws& ws) {
    if (L.w) zf_launch_gap_wrows(st, L.kind, z, b, L.w, m, scale, L.delta, ws);
    else if (L.kind == ZF_LOSS_HUBER) zf_launch_gap_huber_rows(st, z, b, m, scale, L.delta, ws);
    else if (L.kind == ZF_LOSS_POISSON)   // psi and f by the loss kernels of a trial, called outside the loop (as the logistic rows)
        zf_launch_poisson_y(st, nullptr, z, z, z, b, ws.rvec, scale, m, 0, ws.part + 2 * ZF_GAP_MAX_CHUNKS, ws.scal + ZF_GS_F);
    else zf_launch_gap_rows(st, L.kind == ZF_LOSS_LOGISTIC, z, b, m, scale, ws);
}

// where the composition left the results in ws.scal, and how many of them a caller's buffer of out_count doubles takes
struct zf_gap_out {
    int slot, count;
};

// steps 3 .. 6, with g = grad f(x) in ws.g: the n-passes and the composition of the l1 (l2 = 0) or the elastic-net evaluation
static inline zf_gap_out zf_launch_loss_gap_tail(hipStream_t st, const zf_loss& L, const double* z, const double* b, const double* x,
                                                 int64_t m, int64_t n, double scale, double lam, double l2, const zf_gap_ws& ws,
                                                 int64_t out_count) {
    const bool logistic = L.kind == ZF_LOSS_LOGISTIC;
    if (L.w) zf_launch_gap_wtail(st, L.kind, z, b, L.w, x, m, n, scale, lam, l2, ws);
    else if (L.kind == ZF_LOSS_HUBER) zf_launch_gap_tail_huber(st, x, n, scale, lam, l2, ws);
    else if (L.kind == ZF_LOSS_POISSON) zf_launch_gap_tail_poisson(st, z, b, nullptr, x, m, n, scale, lam, l2, ws);
    else if (l2 > 0.0) zf_launch_gap_tail_enet(st, logistic, z, b, x, m, n, scale, lam, l2, ws);
    else zf_launch_gap_tail(st, logistic, z, b, x, m, n, scale, lam, ws);
    if (l2 > 0.0) return zf_gap_out{ZF_GS_OUT_ENET, out_count >= 10 ? 10 : 8};   // (ten values when the caller's buffer holds them)
    return zf_gap_out{ZF_GS_OUT, 8};
}
