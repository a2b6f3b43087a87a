// zf_kernels_gap.h - the duality gap of  P(x) = sum_i w_i phi_i(z_i) + lam |x|_1 (+ (l2 / 2) |x|^2),  z = A x  (gfx950, fp64), for
// the four losses of the margins kinds (zf_kernels_loss.h), with or without row weights w: every certificate kernel and launcher.
//
// Dual point: nu = alpha grad phi(z), g = A^T grad phi(z) = grad f(x), alpha = min(1, lam / |g|_inf) (1 when g = 0), so that
// |A^T nu|_inf <= lam and D = -sum_i phi_i^*(nu_i).  P - D is a difference of two numbers of the size of F; the gap is
// formed instead as the sum of the two Fenchel-Young gaps, every term of which is >= 0:
//   rows     least squares  scale (1 - alpha)^2 |r|^2,  r = z - b               (closed form, from sum r^2)
//            logistic       scale sum_i KL(alpha q_i || q_i),  q = sigma(t), t = -b z          (at zf_gap_kl_kernel)
//            Huber          scale (1 - alpha) ((1 - alpha) sum c^2 + 2 T)                      (at zf_gap_huber_rows_kernel)
//            Poisson        scale sum_i [e^z - v + v (log v - z)],  v = alpha e^z + (1 - alpha) b   (at zf_poisson_gap_row)
//   columns  sum_j (lam |x_j| + alpha g_j x_j), term by term (each >= 0 because |alpha g_j| <= lam)
// 1 - alpha is max(0, (|g|_inf - lam) / |g|_inf), never 1 - (rounded alpha); alpha log alpha is alpha log1p(-(1 - alpha)).
// P and D are reported in their plain forms beside it.  Row weights: (w phi)^*(w u) = w phi^*(u), so every row term is taken
// times w_i (zf_wterm: w_i == 0 is a row that is not there) into the same scalar slots, rvec receives w o psi - the caller's
// column sweep yields the weighted gradient - and the n-passes and the composition kernels do not know of w.
//
// One evaluation, given the margins z (a sweep over A, or the margin ring of a live solver) and x:
//   1  rows (zf_launch_gap_rows):  psi -> rvec and the row sums that need no alpha - least squares zf_gap_ls_rows_kernel /
//      zf_gap_wls_rows_kernel, Huber zf_gap_huber_rows_kernel; logistic and Poisson: the rows kernel of a trial (ctl = NULL)
//   2  g = factor * A^T rvec by the caller's column sweep (zf_solver.hip); penalty factors: zf_gap_pf_scale_kernel
//   3  zf_gap_ginf[_enet]_kernel (+ finish): |g|_inf -> alpha, 1 - alpha, alpha log alpha, left in device memory
//   4  zf_gap_cols[_enet]_kernel (+ finish): sum_j (lam |x_j| + alpha g_j x_j), sum |x_j| (, sum x_j^2)   (3, 4: zf_launch_gap_npasses)
//   5  the rows that need alpha (zf_launch_gap_alpha_rows in zf_loss_dispatch.h): logistic zf_gap_kl_kernel, Poisson zf_gap_poisson_kernel, multinomial
//      zf_gap_softmax_kernel of zf_kernels_softmax.h (+ finish)
//   6  composition (one thread): zf_gap_compose_kernel / _enet_kernel / _huber_kernel
// Shapes: the n-vectors take ONE workgroup up to ZF_GAP_ONE_WG_MAX_N elements and zf_gap_chunks(n) workgroups on a
// contiguous chunk each beyond (chunk results combined in chunk order by one workgroup); the m-vectors the two shapes of
// zf_launch_rows_shapes - so the dense and the sparse class sum the rows of the same m in the same order.  No atomics; every
// sum in an order fixed by m or n alone: two evaluations give the same bits.
// Non-finite input: v_max_f64 drops a NaN operand, so the maximum carries a flag beside it (any |g_j| that is not <= DBL_MAX)
// and |g|_inf, alpha and everything behind them are NaN then; the column pass turns a non-finite x_j into a NaN term.
// Bytes: 8 n (|g|_inf) + 16 n (columns) + 16 m (the rows of step 5; step 1: 24 m with the store of psi), 8 m more per rows pass
// with weights.
// (included by zf_solver.hip alone)
#pragma once
#include <float.h>

#include "zf_common.h"
#include "zf_kernels_loss.h"

constexpr int64_t ZF_GAP_ONE_WG_MAX_N = 4096;   // n-vectors: one workgroup up to here
constexpr int64_t ZF_GAP_CHUNK_ELEMS = 2048;    // ... beyond: a workgroup per this many elements,
constexpr int ZF_GAP_MAX_CHUNKS = 1024;         // at most so many (longer chunks then)
constexpr int ZF_GAP_PART = 3 * ZF_GAP_MAX_CHUNKS;   // doubles of chunk results: two rows of the gap kernels + the loss kernels' one
constexpr int ZF_GAP_PART_HUBER = 4 * ZF_GAP_MAX_CHUNKS;   // Huber's rows pass holds a fourth row: its workspace is longer by it

// slots of the scalar block (device memory; ZF_GAP_SCAL doubles)
enum {
    ZF_GS_GINF = 0, ZF_GS_ALPHA, ZF_GS_OMA, ZF_GS_ALOGA,   // |g|_inf, alpha, 1 - alpha, alpha log alpha
    ZF_GS_F, ZF_GS_RR, ZF_GS_BR,                           // f(x); least squares: sum r^2, sum b r
    ZF_GS_COLS, ZF_GS_ASUM,                                // sum_j (lam |x_j| + alpha g_j x_j), sum |x_j|
    ZF_GS_KL, ZF_GS_ENT,                                   // logistic: sum KL(alpha q || q), sum [p log p + (1 - p) log(1 - p)]
    ZF_GS_OUT = 16,                                        // the eight output doubles
    ZF_GAP_SCAL = 24
};
// Huber: sum c^2 and sum b c where the least-squares rows leave sum r^2 and sum b r (the dual and the screen's |c|_2 read them
// there), sum H and T in the two slots of the logistic rows.  Poisson: its two sums in the slots of the logistic rows.
enum { ZF_GS_HSUM = ZF_GS_KL, ZF_GS_HT = ZF_GS_ENT };

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

// the same rows with weights: w r -> rvec, sum w r^2, sum w b r; f = scale sum w r^2, the PLAIN form (beyond one workgroup by
// zf_rows_finish_kernel over the first row of chunk sums).  A kernel of its own: the two differ in their f and in the unroll
// of the loop, which one template would have to carry as two more switches.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void zf_gap_wls_rows_kernel(const double* __restrict__ z, const double* __restrict__ b,
                                                                const double* __restrict__ w, double* __restrict__ rvec, int64_t m,
                                                                double scale, double* __restrict__ part, double* __restrict__ scal) {
    __shared__ double lds[2 * BLOCK / 64];
    int64_t lo, hi;
    zf_gap_chunk_of(m, lo, hi);
    double rr = 0.0, br = 0.0;
#pragma unroll 2
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
        const double bi = b[i], wi = w[i];
        const double rv = z[i] - bi;
        const bool on = wi != 0.0;
        rvec[i] = on ? wi * rv : 0.0;
        rr += on ? wi * (rv * rv) : 0.0;
        br += on ? wi * (bi * rv) : 0.0;
    }
    zf_gap_block_pair<BLOCK, false>(rr, br, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            scal[ZF_GS_RR] = rr;
            scal[ZF_GS_BR] = br;
            scal[ZF_GS_F] = scale * rr;
        } else {
            part[blockIdx.x] = rr;
            part[ZF_GAP_MAX_CHUNKS + blockIdx.x] = br;
        }
    }
}

// ---- rows, Huber: c -> cvec and four sums that need no alpha -------------------------------------------------------------------
//   sum H,  sum c^2,  sum b c,  T = sum |c| (|r| - |c|)          (every term of T >= 0, exactly 0 on an unclipped row)
//   D = -scale (alpha^2 sum c^2 + 2 alpha sum b c)      rows gap = scale (1 - alpha) ((1 - alpha) sum c^2 + 2 T)
// chunk sums: four rows of ZF_GAP_MAX_CHUNKS (ZF_GAP_PART_HUBER)
template <int BLOCK, bool W>
__global__ __launch_bounds__(BLOCK) void zf_gap_huber_rows_kernel(const double* __restrict__ z, const double* __restrict__ b,
                                                                  const double* __restrict__ w, double* __restrict__ cvec, int64_t m,
                                                                  double scale, double delta, double* __restrict__ part,
                                                                  double* __restrict__ scal) {
    __shared__ double lds[2 * BLOCK / 64];
    int64_t lo, hi;
    zf_gap_chunk_of(m, lo, hi);
    double hs = 0.0, cc = 0.0, bc = 0.0, tt = 0.0;
#pragma unroll 2
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
        const double bi = b[i], wi = W ? w[i] : 1.0;
        const double rv = z[i] - bi;
        const double c = zf_huber_clip(rv, delta);
        const double ac = fabs(c);
        const bool on = wi != 0.0;
        cvec[i] = zf_wterm<W>(on, wi, c);
        hs += zf_wterm<W>(on, wi, zf_huber_of(rv, c));
        cc += zf_wterm<W>(on, wi, c * c);
        bc += zf_wterm<W>(on, wi, bi * c);
        tt += zf_wterm<W>(on, wi, ac * (fabs(rv) - ac));
    }
    zf_gap_block_pair<BLOCK, false>(hs, tt, lds);
    __syncthreads();   // (the pair's LDS words are read by every thread: none may be rewritten before)
    zf_gap_block_pair<BLOCK, false>(cc, bc, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            scal[ZF_GS_HSUM] = hs;
            scal[ZF_GS_HT] = tt;
            scal[ZF_GS_RR] = cc;
            scal[ZF_GS_BR] = bc;
            scal[ZF_GS_F] = scale * hs;
        } else {
            part[blockIdx.x] = cc;
            part[ZF_GAP_MAX_CHUNKS + blockIdx.x] = bc;
            part[2 * ZF_GAP_MAX_CHUNKS + blockIdx.x] = hs;
            part[3 * ZF_GAP_MAX_CHUNKS + blockIdx.x] = tt;
        }
    }
}

// rows 2 and 3 of the chunk sums, each added in chunk order -> sum H, T and f = scale sum H
__global__ __launch_bounds__(ZF_BLOCK) void zf_gap_huber_finish_kernel(const double* __restrict__ part, int count, double scale,
                                                                       double* __restrict__ scal) {
    __shared__ double lds[2 * ZF_WAVES];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < count; i += ZF_BLOCK) {
        a += part[2 * ZF_GAP_MAX_CHUNKS + i];
        b += part[3 * ZF_GAP_MAX_CHUNKS + i];
    }
    zf_gap_block_pair<ZF_BLOCK, false>(a, b, lds);
    if (threadIdx.x == 0) {
        scal[ZF_GS_HSUM] = a;
        scal[ZF_GS_HT] = b;
        scal[ZF_GS_F] = scale * a;
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

// ---- rows, logistic: sum_i w_i KL(alpha q_i || q_i) and sum_i w_i [p log p + (1 - p) log(1 - p)], p = alpha q ------------------
//   KL = q (alpha log alpha) + (1 - alpha q) L,  L = log[(1 - alpha q) / (1 - q)]
//      = log1p((1 - alpha) e^t)  (t <= 0)   |   t + log((1 - alpha) + e^-t)  (t > 0)
// with 1 - alpha q formed as (1 - q) + (1 - alpha) q - no subtraction anywhere; one e = exp(-|t|) per row as in zf_loss_row,
// finite for every finite margin; alpha = 1: every term exactly 0.  D = -scale [the second sum].
template <int BLOCK, bool W>
__global__ __launch_bounds__(BLOCK) void zf_gap_kl_kernel(const double* __restrict__ z, const double* __restrict__ b,
                                                          const double* __restrict__ w, int64_t m, double* __restrict__ part,
                                                          double* __restrict__ scal) {
    __shared__ double lds[2 * BLOCK / 64];
    const double alpha = scal[ZF_GS_ALPHA], oma = scal[ZF_GS_OMA], aloga = scal[ZF_GS_ALOGA];
    int64_t lo, hi;
    zf_gap_chunk_of(m, lo, hi);
    double kl = 0.0, ent = 0.0;
#pragma unroll 2
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
        const double wi = W ? w[i] : 1.0;
        const bool on = wi != 0.0;
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
            kl += zf_wterm<W>(on, wi, k);
        }
        const double en = (p == 0.0 ? 0.0 : p * log(p)) + (omp == 0.0 ? 0.0 : omp * log(omp));
        ent += zf_wterm<W>(on, wi, en);
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

// ---- rows, Poisson ------------------------------------------------------------------------------------------------------------
// h(z) = e^z - b z has the conjugate h^*(u) = v log v - v, v = u + b >= 0 (0 log 0 = 0); the dual point nu = alpha grad phi(z)
// gives v = alpha e^z + (1 - alpha) b >= 0 always: feasible for every alpha in [0, 1].
//   D = -scale sum_i (v_i log v_i - v_i)
//   rows = scale sum_i [e^z - v + v (log v - z)],  each term = e^z ((1 + d) log1p(d) - d),  d = (1 - alpha)(b - e^z) / e^z >= -1
// every term >= 0 and exactly 0 at alpha = 1.  1 - alpha and alpha log alpha are read from device memory (zf_gap_alpha), never
// formed from a rounded alpha.  The three forms of a row:
//   b = 0:            e (alpha log alpha + (1 - alpha))                            (v = alpha e)
//   d <= 1:           e ((alpha + (1 - alpha) b / e) log1p(d) - d)                 (1 + d as a sum of two terms >= 0)
//   d > 1, e = 0:     (e - v) + v (log v - z)   - the direct form: no cancellation there (log v - z >= log 2), and finite
//                     where b / e overflows (z = -700) or e has underflowed to 0
// finite for every |z| <= 700 and every count b < 1e300.
// the Fenchel-Young gap of one row (>= 0) and v log v - v; oma != 0 (the caller skips alpha = 1)
__device__ __forceinline__ void zf_poisson_gap_row(double z, double bi, double alpha, double oma, double aloga, double& gap, double& ent) {
    const double e = exp(z);
    const double v = alpha * e + oma * bi;
    double t;
    if (bi == 0.0) {
        t = e * (aloga + oma);
    } else {
        const double d = oma * (bi - e) / e;   // (e = 0: +inf; a NaN margin: NaN - both take the direct form)
        if (d <= 1.0) t = e * ((alpha + oma * (bi / e)) * log1p(d) - d);
        else t = (e - v) + v * (log(v) - z);
    }
    if (t < 0.0) t = 0.0;   // (>= 0 but for rounding; a NaN stays: the comparison is false)
    gap = t;
    ent = v == 0.0 ? 0.0 : v * log(v) - v;
}

// sum_i w_i [row gap] -> ZF_GS_KL and sum_i w_i (v log v - v) -> ZF_GS_ENT: the slots, shapes and chunk rows of zf_gap_kl_kernel,
// so the composition kernels' logistic arm - rows = scale [KL slot], D = -scale [ENT slot] - serves this loss too.
// alpha = 1 (oma == 0): v = e exactly and every row gap is exactly 0 - not formed.
template <int BLOCK, bool W>
__global__ __launch_bounds__(BLOCK) void zf_gap_poisson_kernel(const double* __restrict__ z, const double* __restrict__ b,
                                                               const double* __restrict__ w, int64_t m, double* __restrict__ part,
                                                               double* __restrict__ scal) {
    __shared__ double lds[2 * BLOCK / 64];
    const double alpha = scal[ZF_GS_ALPHA], oma = scal[ZF_GS_OMA], aloga = scal[ZF_GS_ALOGA];
    int64_t lo, hi;
    zf_gap_chunk_of(m, lo, hi);
    double gs = 0.0, ent = 0.0;
#pragma unroll 2
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
        const double wi = W ? w[i] : 1.0;
        const bool on = wi != 0.0;
        const double zi = z[i];
        double k = 0.0, en;
        if (oma != 0.0) {   // (a NaN alpha takes this branch)
            zf_poisson_gap_row(zi, b[i], alpha, oma, aloga, k, en);
        } else {
            const double e = exp(zi);
            en = e == 0.0 ? 0.0 : e * log(e) - e;
        }
        gs += zf_wterm<W>(on, wi, k);
        ent += zf_wterm<W>(on, wi, en);
    }
    zf_gap_block_pair<BLOCK, false>(gs, ent, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            scal[ZF_GS_KL] = gs;
            scal[ZF_GS_ENT] = ent;
        } else {
            part[blockIdx.x] = gs;
            part[ZF_GAP_MAX_CHUNKS + blockIdx.x] = ent;
        }
    }
}

// ---- composition (one thread): [P, D, gap, alpha, |g|_inf, f, lam |x|_1, rows gap] ----------------------------------------------
// least squares: D = -scale (alpha^2 |r|^2 + 2 alpha b.r); `logistic` (and Poisson): the two sums of the rows pass of step 5
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

// Huber's composition (one thread).  enet == 0: the eight values of zf_gap_compose_kernel at ZF_GS_OUT; else the ten of
// zf_gap_compose_enet_kernel at ZF_GS_OUT_ENET.  Every factor >= 0: the rows part is a sum of non-negative terms.
__global__ void zf_gap_compose_huber_kernel(int enet, double scale, double lam, double l2, double* __restrict__ scal) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double alpha = scal[ZF_GS_ALPHA], oma = scal[ZF_GS_OMA];
    const double f = scal[ZF_GS_F], g1 = lam * scal[ZF_GS_ASUM];
    const double cc = scal[ZF_GS_RR];
    const double dual = -scale * (alpha * alpha * cc + 2.0 * alpha * scal[ZF_GS_BR]);
    const double rows = scale * oma * (oma * cc + 2.0 * scal[ZF_GS_HT]);
    if (!enet) {
        double* out = scal + ZF_GS_OUT;
        out[0] = f + g1;
        out[1] = dual;
        out[2] = rows + scal[ZF_GS_COLS];
        out[3] = alpha;
        out[4] = scal[ZF_GS_GINF];
        out[5] = f;
        out[6] = g1;
        out[7] = rows;
        return;
    }
    const double g2 = (0.5 * l2) * scal[ZF_GS_XX];
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

// ---- launches -------------------------------------------------------------------------------------------------------------
// the workspace of one evaluation: rvec (m doubles: psi), g (n), part (ZF_GAP_PART; Huber: ZF_GAP_PART_HUBER), scal (ZF_GAP_SCAL)
struct zf_gap_ws {
    double *rvec, *g, *part, *scal;
};

// the finish of a chunked pass: the two rows of chunk sums -> ws.scal[dst0], ws.scal[dst1] (f_scale: zf_gap_sum_finish_kernel)
static inline void zf_launch_gap_sum_finish(hipStream_t st, const zf_gap_ws& ws, int chunks, int dst0, int dst1, double f_scale = -1.0) {
    hipLaunchKernelGGL(zf_gap_sum_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, chunks, dst0, dst1, f_scale, ws.scal);
}

// step 1 for the squared loss and Huber's (w: the row weights or NULL): psi (without its factor: r, or c) -> ws.rvec and the
// row sums that need no alpha.  The logistic and the Poisson loss take the rows kernel of a trial instead (zf_loss_dispatch.h).
static inline void zf_launch_gap_rows(hipStream_t st, bool huber, const double* z, const double* b, const double* w, int64_t m,
                                      double scale, double delta, const zf_gap_ws& ws) {
    if (huber) {
        const int chunks = zf_launch_rows_shapes(st, w ? zf_gap_huber_rows_kernel<ZF_ROWS_BLOCK, true> : zf_gap_huber_rows_kernel<ZF_ROWS_BLOCK, false>,
                                                 w ? zf_gap_huber_rows_kernel<ZF_BLOCK, true> : zf_gap_huber_rows_kernel<ZF_BLOCK, false>, m, z, b, w,
                                                 ws.rvec, m, scale, delta, ws.part, ws.scal);
        if (!chunks) return;
        zf_launch_gap_sum_finish(st, ws, chunks, ZF_GS_RR, ZF_GS_BR);
        hipLaunchKernelGGL(zf_gap_huber_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, chunks, scale, ws.scal);
    } else if (w) {
        const int chunks = zf_launch_rows_shapes(st, zf_gap_wls_rows_kernel<ZF_ROWS_BLOCK>, zf_gap_wls_rows_kernel<ZF_BLOCK>, m, z, b, w, ws.rvec,
                                                 m, scale, ws.part, ws.scal);
        if (!chunks) return;
        zf_launch_gap_sum_finish(st, ws, chunks, ZF_GS_RR, ZF_GS_BR);
        // f = scale * (the first row of chunk sums, added in the same order): the plain form, no sqrt()^2
        hipLaunchKernelGGL(zf_rows_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, nullptr, 0, ws.part, chunks, scale, ws.scal + ZF_GS_F);
    } else {
        const int chunks = zf_launch_rows_shapes(st, zf_gap_ls_rows_kernel<ZF_ROWS_BLOCK>, zf_gap_ls_rows_kernel<ZF_BLOCK>, m, z, b, ws.rvec, m,
                                                 scale, ws.part, ws.scal);
        if (chunks) zf_launch_gap_sum_finish(st, ws, chunks, ZF_GS_RR, ZF_GS_BR, scale);
    }
}

static inline void zf_launch_gap_pf_scale(hipStream_t st, double* g, const double* x, const double* p, double* xp, int64_t n) {
    hipLaunchKernelGGL(zf_gap_pf_scale_kernel, dim3(zf_grid_for(n)), dim3(ZF_BLOCK), 0, st, g, x, p, xp, n);
}

// steps 3 and 4, with g = grad f(x) in ws.g: the n-passes of the l1 (l2 = 0) or the elastic-net evaluation
static inline void zf_launch_gap_npasses(hipStream_t st, const double* x, int64_t n, double lam, double l2, const zf_gap_ws& ws) {
    const int nc = zf_gap_chunks(n);
    const bool enet = l2 > 0.0;
    if (enet) hipLaunchKernelGGL(zf_gap_ginf_enet_kernel, dim3(nc), dim3(ZF_BLOCK), 0, st, ws.g, x, l2, n, lam, ws.part, ws.scal);
    else hipLaunchKernelGGL(zf_gap_ginf_kernel, dim3(nc), dim3(ZF_BLOCK), 0, st, ws.g, n, lam, ws.part, ws.scal);
    if (nc > 1) hipLaunchKernelGGL(zf_gap_ginf_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, nc, lam, ws.scal);
    if (enet) hipLaunchKernelGGL(zf_gap_cols_enet_kernel, dim3(nc), dim3(ZF_BLOCK), 0, st, x, ws.g, l2, n, lam, ws.part, ws.scal);
    else hipLaunchKernelGGL(zf_gap_cols_kernel, dim3(nc), dim3(ZF_BLOCK), 0, st, x, ws.g, n, lam, ws.part, ws.scal);
    if (nc > 1) {
        zf_launch_gap_sum_finish(st, ws, nc, ZF_GS_COLS, ZF_GS_ASUM);
        if (enet) hipLaunchKernelGGL(zf_gap_sum_third_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, nc, (int)ZF_GS_XX, ws.scal);
    }
}
