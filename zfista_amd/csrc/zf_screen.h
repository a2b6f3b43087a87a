// zf_screen.h - what the gap evaluation (zf_solver.hip) needs of gap-safe screening: the request a caller attaches to a
// gap evaluation and the launch that serves it.  The kernels are in zf_kernels_screen.h (included by zf_screen.hip only).
#pragma once
#include "zf_spmv.h"

constexpr int ZF_SCREEN_MAX_CHUNKS = 1024;   // as ZF_GAP_MAX_CHUNKS: the n-passes of a screen take the chunks of the gap's
constexpr int ZF_SCREEN_SCAL = 4;            // [r, E, r_eff = r + E, kept count]

// Screening behind a gap evaluation: keep_j = !(alpha |g_j| + r_eff |a_j|_2 < lam)  (zf_kernels_screen.h)
struct zf_screen_req {
    const double* norms;       // n: |a_j|_2                       (device)
    const double* stats;       // [sum_j |a_j|^2, max_j |a_j|]     (device)
    int64_t max_row, max_col;  // stored elements of the longest row and column of A (dense: n and m)
    uint8_t* keep;             // n: the mask                      (device, out)
    int32_t* index;            // n: its exclusive scan            (device, out)
    int32_t* cnt;              // ZF_SCREEN_MAX_CHUNKS + 1 of the evaluation
    double* scal;              // ZF_SCREEN_SCAL of the evaluation (device, out)
};

// g: grad f(x) (n); gap8: the eight outputs of the gap evaluation; asum: sum |x_j|; rr: sum r^2 (least squares; unused for
// the logistic loss).  Stream-ordered behind the gap's own kernels: four launches.
void zf_launch_screen(hipStream_t st, const zf_screen_req& rq, const double* g, const double* gap8, const double* asum, const double* rr,
                      int64_t m, int64_t n, double scale, double lam, bool logistic);
