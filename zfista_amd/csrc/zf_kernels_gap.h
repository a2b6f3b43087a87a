// zf_kernels_gap.h - the duality gap of  P(x) = sum_i phi_i(z_i) + lam |x|_1,  z = A x  (gfx950, fp64), for the two losses of
// the margins kinds:  phi_i(z) = scale (z - b_i)^2  and  phi_i(z) = scale softplus(-b_i z).
//
// Dual point: nu = alpha grad phi(z), g = A^T grad phi(z) = grad f(x), alpha = min(1, lam / |g|_inf) (1 when g = 0), so that
// |A^T nu|_inf <= lam and D = -sum_i phi_i^*(nu_i).  P - D is a difference of two numbers of the size of F; the gap is
// formed instead as the sum of the two Fenchel-Young gaps, every term of which is >= 0:
//   rows     least squares  scale (1 - alpha)^2 |r|^2,  r = z - b               (closed form, from sum r^2)
//            logistic       scale sum_i KL(alpha q_i || q_i),  q = sigma(t), t = -b z:
//                           KL = q (alpha log alpha) + (1 - alpha q) L,  L = log[(1 - alpha q) / (1 - q)]
//                              = log1p((1 - alpha) e^t)  (t <= 0)   |   t + log((1 - alpha) + e^-t)  (t > 0)
//                           with 1 - alpha q formed as (1 - q) + (1 - alpha) q - no subtraction anywhere; one e = exp(-|t|)
//                           per row as in zf_kernels_loss.h, finite for every finite margin; alpha = 1: every term exactly 0
//   columns  sum_j (lam |x_j| + alpha g_j x_j), term by term (each >= 0 because |alpha g_j| <= lam)
// 1 - alpha is max(0, (|g|_inf - lam) / |g|_inf), never 1 - (rounded alpha); alpha log alpha is alpha log1p(-(1 - alpha)).
// P and D are reported in their plain forms beside it:  least squares D = -scale (alpha^2 |r|^2 + 2 alpha b.r),
// logistic D = -scale sum_i [p log p + (1 - p) log(1 - p)], p = alpha q.
//
// One evaluation, given the margins z (a sweep over A, or the margin ring of a live solver) and x:
//   1  rows:   least squares zf_gap_ls_rows_kernel: r -> rvec, sum r^2, sum b r, f;  logistic: zf_launch_logit_y (ctl = NULL)
//   2  g = factor * A^T rvec by the caller's column sweep (zf_solver.hip)
//   3  zf_gap_ginf_kernel (+ finish): |g|_inf -> alpha, 1 - alpha, alpha log alpha, left in device memory
//   4  zf_gap_cols_kernel (+ finish): sum_j (lam |x_j| + alpha g_j x_j), sum |x_j|
//   5  logistic: zf_gap_kl_kernel (+ finish): sum KL, sum of the negative entropies
//   6  zf_gap_compose_kernel (one thread): [P, D, gap, alpha, |g|_inf, f, lam |x|_1, rows gap]
// Shapes: the n-vectors take ONE workgroup up to ZF_GAP_ONE_WG_MAX_N elements and zf_gap_chunks(n) workgroups on a
// contiguous chunk each beyond (chunk results combined in chunk order by one workgroup); the m-vectors the two shapes of
// zf_logit_wide(m) - so the dense and the sparse class sum the rows of the same m in the same order.  No atomics; every sum
// in an order fixed by m or n alone: two evaluations give the same bits.
// Non-finite input: v_max_f64 drops a NaN operand, so the maximum carries a flag beside it (any |g_j| that is not <= DBL_MAX)
// and |g|_inf, alpha and everything behind them are NaN then; the column pass turns a non-finite x_j into a NaN term.
// Bytes: 8 n (|g|_inf) + 16 n (columns) + 16 m (logistic rows; least squares: 24 m with the store of r).
// (included by zf_solver.hip alone)
#pragma once
#include <float.h>

#include "zf_common.h"
#include "zf_kernels_loss.h"

constexpr int64_t ZF_GAP_ONE_WG_MAX_N = 4096;   // n-vectors: one workgroup up to here
constexpr int64_t ZF_GAP_CHUNK_ELEMS = 2048;    // ... beyond: a workgroup per this many elements,
constexpr int ZF_GAP_MAX_CHUNKS = 1024;         // at most so many (longer chunks then)
constexpr int ZF_GAP_ROWS_BLOCK = 1024;         // m-vectors: the one-workgroup shape (as ZF_LOGIT_BLOCK / RESID_BLOCK)
constexpr int ZF_GAP_PART = 3 * ZF_GAP_MAX_CHUNKS;   // doubles of chunk results: two rows of the gap kernels + the loss kernels' one

// slots of the scalar block (device memory; ZF_GAP_SCAL doubles)
enum {
    ZF_GS_GINF = 0, ZF_GS_ALPHA, ZF_GS_OMA, ZF_GS_ALOGA,   // |g|_inf, alpha, 1 - alpha, alpha log alpha
    ZF_GS_F, ZF_GS_RR, ZF_GS_BR,                           // f(x); least squares: sum r^2, sum b r
    ZF_GS_COLS, ZF_GS_ASUM,                                // sum_j (lam |x_j| + alpha g_j x_j), sum |x_j|
    ZF_GS_KL, ZF_GS_ENT,                                   // logistic: sum KL(alpha q || q), sum [p log p + (1 - p) log(1 - p)]
    ZF_GS_OUT = 16,                                        // the eight output doubles
    ZF_GAP_SCAL = 24
};

static inline int zf_gap_chunks(int64_t n) {
    if (n <= ZF_GAP_ONE_WG_MAX_N) return 1;
    const int64_t c = (n + ZF_GAP_CHUNK_ELEMS - 1) / ZF_GAP_CHUNK_ELEMS;
    return (int)(c > ZF_GAP_MAX_CHUNKS ? ZF_GAP_MAX_CHUNKS : c);
}

// two sums (MAX: two maxima) of the workgroup at once: wave trees, then the wave results in wave order (every thread holds both)
template <int BLOCK, bool MAX>
__device__ __forceinline__ void zf_gap_block_pair(double& a, double& b, double* lds /* 2 * BLOCK / 64 */) {
    a = MAX ? zf_wave_max(a) : zf_wave_sum(a);
    b = MAX ? zf_wave_max(b) : zf_wave_sum(b);
    if ((threadIdx.x & 63) == 0) {
        lds[threadIdx.x >> 6] = a;
        lds[BLOCK / 64 + (threadIdx.x >> 6)] = b;
    }
    __syncthreads();
    double ta = lds[0], tb = lds[BLOCK / 64];
    for (int w = 1; w < BLOCK / 64; ++w) {
        ta = MAX ? fmax(ta, lds[w]) : ta + lds[w];
        tb = MAX ? fmax(tb, lds[BLOCK / 64 + w]) : tb + lds[BLOCK / 64 + w];
    }
    a = ta;
    b = tb;
}

// the chunk [lo, hi) of workgroup blockIdx.x of a vector of `len` elements
__device__ __forceinline__ void zf_gap_chunk_of(int64_t len, int64_t& lo, int64_t& hi) {
    const int64_t per = (len + gridDim.x - 1) / gridDim.x;
    lo = (int64_t)blockIdx.x * per;
    hi = lo + per < len ? lo + per : len;
}

// ---- rows, least squares: r = z - b -> rvec, sum r^2, sum b r; f = scale sqrt(sum r^2)^2 as zf_resid_x_kernel leaves it ----
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void zf_gap_ls_rows_kernel(const double* __restrict__ z, const double* __restrict__ b,
                                                               double* __restrict__ rvec, int64_t m, double scale,
                                                               double* __restrict__ part, double* __restrict__ scal) {
    __shared__ double lds[2 * BLOCK / 64];
    int64_t lo, hi;
    zf_gap_chunk_of(m, lo, hi);
    double rr = 0.0, br = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
        const double bi = b[i];
        const double rv = z[i] - bi;
        rvec[i] = rv;
        rr += rv * rv;
        br += bi * rv;
    }
    zf_gap_block_pair<BLOCK, false>(rr, br, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            const double nrm = sqrt(rr);
            scal[ZF_GS_RR] = rr;
            scal[ZF_GS_BR] = br;
            scal[ZF_GS_F] = scale * (nrm * nrm);
        } else {
            part[blockIdx.x] = rr;
            part[ZF_GAP_MAX_CHUNKS + blockIdx.x] = br;
        }
    }
}

// the two rows of chunk sums, each added in chunk order (thread t: chunks t, t + 256, ...) -> scal[dst0], scal[dst1];
// f_scale >= 0 (least-squares rows): also f = f_scale sqrt(first sum)^2
__global__ __launch_bounds__(ZF_BLOCK) void zf_gap_sum_finish_kernel(const double* __restrict__ part, int count, int dst0, int dst1,
                                                                     double f_scale, double* __restrict__ scal) {
    __shared__ double lds[2 * ZF_WAVES];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < count; i += ZF_BLOCK) {
        a += part[i];
        b += part[ZF_GAP_MAX_CHUNKS + i];
    }
    zf_gap_block_pair<ZF_BLOCK, false>(a, b, lds);
    if (threadIdx.x == 0) {
        scal[dst0] = a;
        scal[dst1] = b;
        if (f_scale >= 0.0) {
            const double nrm = sqrt(a);
            scal[ZF_GS_F] = f_scale * (nrm * nrm);
        }
    }
}

// ---- |g|_inf and the dual scaling -----------------------------------------------------------------------------------------
// gmax: the maximum of the finite |g_j|; bad > 0: some g_j is NaN or +-inf
__device__ __forceinline__ void zf_gap_alpha(double gmax, double bad, double lam, double* __restrict__ scal) {
    double ginf = gmax, alpha = 1.0, oma = 0.0, aloga = 0.0;
    if (bad > 0.0) {
        ginf = alpha = oma = aloga = NAN;
    } else if (ginf > lam) {   // (g = 0, and every lam >= |g|_inf: alpha = 1, nothing to scale)
        alpha = lam / ginf;
        oma = (ginf - lam) / ginf;
        aloga = alpha > 0.0 ? alpha * log1p(-oma) : 0.0;
    }
    scal[ZF_GS_GINF] = ginf;
    scal[ZF_GS_ALPHA] = alpha;
    scal[ZF_GS_OMA] = oma;
    scal[ZF_GS_ALOGA] = aloga;
}

__global__ __launch_bounds__(ZF_BLOCK) void zf_gap_ginf_kernel(const double* __restrict__ g, int64_t n, double lam,
                                                               double* __restrict__ part, double* __restrict__ scal) {
    __shared__ double lds[2 * ZF_WAVES];
    int64_t lo, hi;
    zf_gap_chunk_of(n, lo, hi);
    double mx = 0.0, bad = 0.0;
#pragma unroll 4
    for (int64_t j = lo + threadIdx.x; j < hi; j += ZF_BLOCK) {
        const double a = fabs(g[j]);
        if (!(a <= DBL_MAX)) bad = 1.0;   // NaN or inf (fmax below would drop the NaN)
        mx = fmax(mx, a);
    }
    zf_gap_block_pair<ZF_BLOCK, true>(mx, bad, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            zf_gap_alpha(mx, bad, lam, scal);
        } else {
            part[blockIdx.x] = mx;
            part[ZF_GAP_MAX_CHUNKS + blockIdx.x] = bad;
        }
    }
}

__global__ __launch_bounds__(ZF_BLOCK) void zf_gap_ginf_finish_kernel(const double* __restrict__ part, int count, double lam,
                                                                      double* __restrict__ scal) {
    __shared__ double lds[2 * ZF_WAVES];
    double mx = 0.0, bad = 0.0;
    for (int i = threadIdx.x; i < count; i += ZF_BLOCK) {
        mx = fmax(mx, part[i]);
        bad = fmax(bad, part[ZF_GAP_MAX_CHUNKS + i]);
    }
    zf_gap_block_pair<ZF_BLOCK, true>(mx, bad, lds);
    if (threadIdx.x == 0) zf_gap_alpha(mx, bad, lam, scal);
}

// ---- columns: sum_j (lam |x_j| + alpha g_j x_j) term by term, and sum |x_j| --------------------------------------------------
__global__ __launch_bounds__(ZF_BLOCK) void zf_gap_cols_kernel(const double* __restrict__ x, const double* __restrict__ g, int64_t n,
                                                               double lam, double* __restrict__ part, double* __restrict__ scal) {
    __shared__ double lds[2 * ZF_WAVES];
    const double alpha = scal[ZF_GS_ALPHA];
    int64_t lo, hi;
    zf_gap_chunk_of(n, lo, hi);
    double cs = 0.0, as = 0.0;
#pragma unroll 4
    for (int64_t j = lo + threadIdx.x; j < hi; j += ZF_BLOCK) {
        const double xj = x[j];
        const double ax = fabs(xj);
        double t = fma(alpha * g[j], xj, lam * ax);
        if (t < 0.0) t = 0.0;                 // (>= 0 but for the rounding of alpha g_j; a NaN stays: the comparison is false)
        if (!(ax <= DBL_MAX)) t = NAN;        // x_j = +-inf: lam inf + alpha g_j inf is inf or NaN by the sign of g_j - NaN always
        cs += t;
        as += ax;
    }
    zf_gap_block_pair<ZF_BLOCK, false>(cs, as, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            scal[ZF_GS_COLS] = cs;
            scal[ZF_GS_ASUM] = as;
        } else {
            part[blockIdx.x] = cs;
            part[ZF_GAP_MAX_CHUNKS + blockIdx.x] = as;
        }
    }
}

// ---- rows, logistic: sum_i KL(alpha q_i || q_i) and sum_i [p log p + (1 - p) log(1 - p)], p = alpha q -------------------------
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void zf_gap_kl_kernel(const double* __restrict__ z, const double* __restrict__ b, int64_t m,
                                                          double* __restrict__ part, double* __restrict__ scal) {
    __shared__ double lds[2 * BLOCK / 64];
    const double alpha = scal[ZF_GS_ALPHA], oma = scal[ZF_GS_OMA], aloga = scal[ZF_GS_ALOGA];
    int64_t lo, hi;
    zf_gap_chunk_of(m, lo, hi);
    double kl = 0.0, ent = 0.0;
#pragma unroll 2
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
        const double t = -b[i] * z[i];
        const double e = exp(-fabs(t));
        const double q = zf_sigmoid_of(t, e);
        const double q1 = (t >= 0.0 ? e : 1.0) / (1.0 + e);   // 1 - q = sigma(-t)
        const double omp = q1 + oma * q;                      // 1 - alpha q
        const double p = alpha * q;
        if (oma != 0.0) {   // (alpha = 1: KL(q || q) is exactly 0; a NaN alpha takes this branch)
            const double L = t <= 0.0 ? log1p(oma * e) : t + log(oma + e);
            double k = q * aloga + omp * L;
            if (k < 0.0) k = 0.0;
            kl += k;
        }
        ent += (p == 0.0 ? 0.0 : p * log(p)) + (omp == 0.0 ? 0.0 : omp * log(omp));
    }
    zf_gap_block_pair<BLOCK, false>(kl, ent, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            scal[ZF_GS_KL] = kl;
            scal[ZF_GS_ENT] = ent;
        } else {
            part[blockIdx.x] = kl;
            part[ZF_GAP_MAX_CHUNKS + blockIdx.x] = ent;
        }
    }
}

// ---- composition (one thread): [P, D, gap, alpha, |g|_inf, f, lam |x|_1, rows gap] ----------------------------------------------
__global__ void zf_gap_compose_kernel(int logistic, double scale, double lam, double* __restrict__ scal) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double alpha = scal[ZF_GS_ALPHA], oma = scal[ZF_GS_OMA];
    const double f = scal[ZF_GS_F], g1 = lam * scal[ZF_GS_ASUM];
    double dual, rows;
    if (logistic) {
        dual = -scale * scal[ZF_GS_ENT];
        rows = scale * scal[ZF_GS_KL];
    } else {
        const double rr = scal[ZF_GS_RR];
        dual = -scale * (alpha * alpha * rr + 2.0 * alpha * scal[ZF_GS_BR]);
        rows = scale * (oma * oma) * rr;
    }
    double* out = scal + ZF_GS_OUT;
    out[0] = f + g1;
    out[1] = dual;
    out[2] = rows + scal[ZF_GS_COLS];
    out[3] = alpha;
    out[4] = scal[ZF_GS_GINF];
    out[5] = f;
    out[6] = g1;
    out[7] = rows;
}

// ---- elastic net: g(x) = lam |x|_1 + (l2 / 2) |x|^2 ------------------------------------------------------------------------
// The ridge term is n more rows with phi(t) = (l2 / 2) t^2 at z = x: grad phi = l2 x, so the dual point is alpha times
// (grad phi(A x), l2 x) with alpha = min(1, lam / |gt|_inf), gt = grad f(x) + l2 x, and phi^*(alpha l2 x_j) = alpha^2 (l2 / 2) x_j^2:
//   P = f + lam |x|_1 + (l2 / 2) sum x^2            D = D_loss(alpha) - (l2 / 2) alpha^2 sum x^2
//   rows: the loss part as above                    ridge = (l2 / 2) (1 - alpha)^2 sum x^2
//   columns = sum_j (lam |x_j| + alpha gt_j x_j)    gap = rows + ridge + columns, every term >= 0 as before
// gt_j = fma(l2, x_j, g_j) is formed on the fly in both n-passes (16 n bytes each; the same expression, the same bits); the
// column pass also sums x^2 (a third row of chunk sums).  The eight outputs keep their meaning with |gt|_inf for |g|_inf;
// [8] = (l2 / 2) sum x^2, [9] = the ridge part of the gap.  The ten values lie in scal[ZF_GS_OUT_ENET ..], sum x^2 in
// scal[ZF_GS_XX]: slots that the l1 evaluation leaves unused - its kernels, launches and allocations are as they were.
enum { ZF_GS_XX = 11, ZF_GS_OUT_ENET = 14 };
static_assert(ZF_GS_ENT < ZF_GS_XX && ZF_GS_XX < ZF_GS_OUT_ENET && ZF_GS_OUT_ENET + 10 <= ZF_GAP_SCAL, "the scalar block holds the ten outputs");

__global__ __launch_bounds__(ZF_BLOCK) void zf_gap_ginf_enet_kernel(const double* __restrict__ g, const double* __restrict__ x, double l2,
                                                                    int64_t n, double lam, double* __restrict__ part,
                                                                    double* __restrict__ scal) {
    __shared__ double lds[2 * ZF_WAVES];
    int64_t lo, hi;
    zf_gap_chunk_of(n, lo, hi);
    double mx = 0.0, bad = 0.0;
#pragma unroll 4
    for (int64_t j = lo + threadIdx.x; j < hi; j += ZF_BLOCK) {
        const double a = fabs(fma(l2, x[j], g[j]));
        if (!(a <= DBL_MAX)) bad = 1.0;
        mx = fmax(mx, a);
    }
    zf_gap_block_pair<ZF_BLOCK, true>(mx, bad, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            zf_gap_alpha(mx, bad, lam, scal);
        } else {
            part[blockIdx.x] = mx;
            part[ZF_GAP_MAX_CHUNKS + blockIdx.x] = bad;
        }
    }
}

// columns: sum_j (lam |x_j| + alpha gt_j x_j) term by term, sum |x_j| and sum x_j^2
__global__ __launch_bounds__(ZF_BLOCK) void zf_gap_cols_enet_kernel(const double* __restrict__ x, const double* __restrict__ g, double l2,
                                                                    int64_t n, double lam, double* __restrict__ part,
                                                                    double* __restrict__ scal) {
    __shared__ double lds[2 * ZF_WAVES];
    const double alpha = scal[ZF_GS_ALPHA];
    int64_t lo, hi;
    zf_gap_chunk_of(n, lo, hi);
    double cs = 0.0, as = 0.0, xx = 0.0;
#pragma unroll 4
    for (int64_t j = lo + threadIdx.x; j < hi; j += ZF_BLOCK) {
        const double xj = x[j];
        const double ax = fabs(xj);
        double t = fma(alpha * fma(l2, xj, g[j]), xj, lam * ax);
        if (t < 0.0) t = 0.0;
        if (!(ax <= DBL_MAX)) t = NAN;
        cs += t;
        as += ax;
        xx = fma(xj, xj, xx);
    }
    zf_gap_block_pair<ZF_BLOCK, false>(cs, as, lds);
    __syncthreads();   // (the pair's LDS words are read by every thread: none may be rewritten before)
    double zero = 0.0;
    zf_gap_block_pair<ZF_BLOCK, false>(xx, zero, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            scal[ZF_GS_COLS] = cs;
            scal[ZF_GS_ASUM] = as;
            scal[ZF_GS_XX] = xx;
        } else {
            part[blockIdx.x] = cs;
            part[ZF_GAP_MAX_CHUNKS + blockIdx.x] = as;
            part[2 * ZF_GAP_MAX_CHUNKS + blockIdx.x] = xx;   // (the loss kernels' row: they are done - stream order)
        }
    }
}

// the third row of chunk sums, added in chunk order -> scal[dst]
__global__ __launch_bounds__(ZF_BLOCK) void zf_gap_sum_third_kernel(const double* __restrict__ part, int count, int dst,
                                                                    double* __restrict__ scal) {
    __shared__ double lds[2 * ZF_WAVES];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < count; i += ZF_BLOCK) a += part[2 * ZF_GAP_MAX_CHUNKS + i];
    zf_gap_block_pair<ZF_BLOCK, false>(a, b, lds);
    if (threadIdx.x == 0) scal[dst] = a;
}

// composition (one thread): [P, D, gap, alpha, |gt|_inf, f, lam |x|_1, rows gap, (l2 / 2) sum x^2, ridge gap]
__global__ void zf_gap_compose_enet_kernel(int logistic, double scale, double lam, double l2, double* __restrict__ scal) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double alpha = scal[ZF_GS_ALPHA], oma = scal[ZF_GS_OMA];
    const double f = scal[ZF_GS_F], g1 = lam * scal[ZF_GS_ASUM], g2 = (0.5 * l2) * scal[ZF_GS_XX];
    double dual, rows;
    if (logistic) {
        dual = -scale * scal[ZF_GS_ENT];
        rows = scale * scal[ZF_GS_KL];
    } else {
        const double rr = scal[ZF_GS_RR];
        dual = -scale * (alpha * alpha * rr + 2.0 * alpha * scal[ZF_GS_BR]);
        rows = scale * (oma * oma) * rr;
    }
    const double ridge = (oma * oma) * g2;
    double* out = scal + ZF_GS_OUT_ENET;
    out[0] = (f + g1) + g2;
    out[1] = dual - (alpha * alpha) * g2;
    out[2] = (rows + ridge) + scal[ZF_GS_COLS];
    out[3] = alpha;
    out[4] = scal[ZF_GS_GINF];
    out[5] = f;
    out[6] = g1;
    out[7] = rows;
    out[8] = g2;
    out[9] = ridge;
}

// ---- launches -------------------------------------------------------------------------------------------------------------
// the workspace of one evaluation: rvec (m doubles: r or rho), g (n), part (ZF_GAP_PART), scal (ZF_GAP_SCAL)
struct zf_gap_ws {
    double *rvec, *g, *part, *scal;
};

// step 1: the dual candidate grad phi(z) (without its factor: r, or rho) -> ws.rvec, and the row sums that need no alpha
static inline void zf_launch_gap_rows(hipStream_t st, bool logistic, const double* z, const double* b, int64_t m, double scale,
                                      const zf_gap_ws& ws) {
    if (logistic) {   // rho and f by the loss kernels of a trial, called outside the loop
        zf_launch_logit_y(st, nullptr, z, z, z, b, ws.rvec, scale, m, 0, ws.part + 2 * ZF_GAP_MAX_CHUNKS, ws.scal + ZF_GS_F);
        return;
    }
    if (!zf_logit_wide(m)) {
        hipLaunchKernelGGL(zf_gap_ls_rows_kernel<ZF_GAP_ROWS_BLOCK>, dim3(1), dim3(ZF_GAP_ROWS_BLOCK), 0, st, z, b, ws.rvec, m, scale,
                           ws.part, ws.scal);
        return;
    }
    const int chunks = zf_spmv_resid_chunks(m);
    hipLaunchKernelGGL(zf_gap_ls_rows_kernel<ZF_BLOCK>, dim3(chunks), dim3(ZF_BLOCK), 0, st, z, b, ws.rvec, m, scale, ws.part, ws.scal);
    hipLaunchKernelGGL(zf_gap_sum_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, chunks, (int)ZF_GS_RR, (int)ZF_GS_BR, scale, ws.scal);
}

// Penalty factors p > 0 (g(x) = lam sum p_j |x_j|, dual constraint |a_j^T theta| <= lam p_j): with g'_j = g_j / p_j and
// x'_j = x_j p_j every quantity of the certificate is that of the unfactored problem at (g', x') - alpha = min(1, lam / |g'|_inf),
// columns = sum (lam |x'_j| + alpha g'_j x'_j), lam |x'|_1 = g(x).  One n-pass between step 2 and the tails: an IEEE division and a
// multiplication per element; g is scaled in place, xp may be x itself (32 n bytes).  The tails then run unchanged.
__global__ __launch_bounds__(ZF_BLOCK) void zf_gap_pf_scale_kernel(double* g, const double* x, const double* __restrict__ p, double* xp,
                                                                   int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * ZF_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * ZF_BLOCK + threadIdx.x; i < n; i += stride) {
        const double pj = p[i];
        g[i] = g[i] / pj;
        xp[i] = x[i] * pj;
    }
}
static inline void zf_launch_gap_pf_scale(hipStream_t st, double* g, const double* x, const double* p, double* xp, int64_t n) {
    hipLaunchKernelGGL(zf_gap_pf_scale_kernel, dim3(zf_grid_for(n)), dim3(ZF_BLOCK), 0, st, g, x, p, xp, n);
}

// steps 3 .. 6, with g = grad f(x) in ws.g; the eight results are left in ws.scal + ZF_GS_OUT
static inline void zf_launch_gap_tail(hipStream_t st, bool logistic, const double* z, const double* b, const double* x, int64_t m,
                                      int64_t n, double scale, double lam, const zf_gap_ws& ws) {
    const int nc = zf_gap_chunks(n);
    hipLaunchKernelGGL(zf_gap_ginf_kernel, dim3(nc), dim3(ZF_BLOCK), 0, st, ws.g, n, lam, ws.part, ws.scal);
    if (nc > 1) hipLaunchKernelGGL(zf_gap_ginf_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, nc, lam, ws.scal);
    hipLaunchKernelGGL(zf_gap_cols_kernel, dim3(nc), dim3(ZF_BLOCK), 0, st, x, ws.g, n, lam, ws.part, ws.scal);
    if (nc > 1)
        hipLaunchKernelGGL(zf_gap_sum_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, nc, (int)ZF_GS_COLS, (int)ZF_GS_ASUM, -1.0, ws.scal);
    if (logistic) {
        if (!zf_logit_wide(m)) {
            hipLaunchKernelGGL(zf_gap_kl_kernel<ZF_GAP_ROWS_BLOCK>, dim3(1), dim3(ZF_GAP_ROWS_BLOCK), 0, st, z, b, m, ws.part, ws.scal);
        } else {
            const int chunks = zf_spmv_resid_chunks(m);
            hipLaunchKernelGGL(zf_gap_kl_kernel<ZF_BLOCK>, dim3(chunks), dim3(ZF_BLOCK), 0, st, z, b, m, ws.part, ws.scal);
            hipLaunchKernelGGL(zf_gap_sum_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, chunks, (int)ZF_GS_KL, (int)ZF_GS_ENT, -1.0, ws.scal);
        }
    }
    hipLaunchKernelGGL(zf_gap_compose_kernel, dim3(1), dim3(64), 0, st, logistic ? 1 : 0, scale, lam, ws.scal);
}

// steps 3 .. 6 of the elastic-net evaluation (l2 > 0), with g = grad f(x) in ws.g; the ten results are left in ws.scal + ZF_GS_OUT_ENET
static inline void zf_launch_gap_tail_enet(hipStream_t st, bool logistic, const double* z, const double* b, const double* x, int64_t m,
                                           int64_t n, double scale, double lam, double l2, const zf_gap_ws& ws) {
    const int nc = zf_gap_chunks(n);
    hipLaunchKernelGGL(zf_gap_ginf_enet_kernel, dim3(nc), dim3(ZF_BLOCK), 0, st, ws.g, x, l2, n, lam, ws.part, ws.scal);
    if (nc > 1) hipLaunchKernelGGL(zf_gap_ginf_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, nc, lam, ws.scal);
    hipLaunchKernelGGL(zf_gap_cols_enet_kernel, dim3(nc), dim3(ZF_BLOCK), 0, st, x, ws.g, l2, n, lam, ws.part, ws.scal);
    if (nc > 1) {
        hipLaunchKernelGGL(zf_gap_sum_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, nc, (int)ZF_GS_COLS, (int)ZF_GS_ASUM, -1.0, ws.scal);
        hipLaunchKernelGGL(zf_gap_sum_third_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, nc, (int)ZF_GS_XX, ws.scal);
    }
    if (logistic) {
        if (!zf_logit_wide(m)) {
            hipLaunchKernelGGL(zf_gap_kl_kernel<ZF_GAP_ROWS_BLOCK>, dim3(1), dim3(ZF_GAP_ROWS_BLOCK), 0, st, z, b, m, ws.part, ws.scal);
        } else {
            const int chunks = zf_spmv_resid_chunks(m);
            hipLaunchKernelGGL(zf_gap_kl_kernel<ZF_BLOCK>, dim3(chunks), dim3(ZF_BLOCK), 0, st, z, b, m, ws.part, ws.scal);
            hipLaunchKernelGGL(zf_gap_sum_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, chunks, (int)ZF_GS_KL, (int)ZF_GS_ENT, -1.0, ws.scal);
        }
    }
    hipLaunchKernelGGL(zf_gap_compose_enet_kernel, dim3(1), dim3(64), 0, st, logistic ? 1 : 0, scale, lam, l2, ws.scal);
}
