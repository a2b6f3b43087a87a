// zf_kernels_loss.h - the losses of the margins s = A x (gfx950, fp64):
//   f(x) = scale * sum_i w_i phi(z_i, b_i),   grad f = gfac * A^T (w o psi(z)),   z = A x,  w = 1 without row weights
// One row function (zf_loss_row<LOSS>) forms psi and phi of a row for the four losses, one kernel body
// (zf_loss_rows_kernel<LOSS, W, WHICH, BLOCK>) walks the rows, one launcher picks its shape.  The two places of a trial where
// the loss enters - everything else of the trial is the least-squares kinds' (zf_launch_trial), the A^T sweep called with gfac:
//   at y  (WHICH 0, only when ctl->need_grad): z = s_k + beta (s_k - s_{k-1}) by linearity, w o psi -> the residual buffer, f(y)
//   at x+ (WHICH 1, every trial):              f(x+) from s+ = A x+
// The unweighted squared loss alone is not served here: it keeps zf_resid_y_kernel / zf_resid_x_kernel / zf_spmv_resid_* and
// the sqrt()^2 form of its f (that mirrors numpy.linalg.norm(.)**2 of the reference's closures).  Every sum in here is a plain
// sum, multiplied by scale once at the end.
//
// Two shapes, chosen by m alone (zf_rows_wide) for both storage forms, so the dense and the sparse class sum a loss of the
// same m in the same order:
//   one workgroup of 1024 threads, thread t takes rows t, t + 1024, ... in that order, and writes f itself - the shape of
//     zf_resid_y_kernel / zf_resid_x_kernel, for the row counts of the dense class;
//   above ZF_SPMV_WIDE_RESID_MIN_ROWS rows zf_spmv_resid_chunks(m) workgroups of 256 threads on a contiguous chunk each
//     -> part[chunk], then ONE workgroup adds the chunk sums in chunk order (zf_rows_finish_kernel) - the shape of
//     zf_spmv_resid_kernel.
// Two rows per thread are in flight (unroll 2: two independent chains), their sums added in row order.  No atomics, no scratch,
// no LDS beyond the block sum, every sum in an order fixed by m: two solves give the same bits.  Guards and ring indices are
// zf_resid_y_kernel's / zf_resid_x_kernel's; ctl == NULL (WHICH 0) or slot < 0 (WHICH 1): a plain call outside the loop on
// ring index 0 (no momentum).
// Bytes: 32 m at y (s_k, s_{k-1}, b, psi), 16 m at x+ - the residual kernels' own - and 8 m more at each place with weights.
// Cost of the logistic rows: fp64 exp and log1p are polynomial code on the VALU (no hardware transcendental in fp64) and the
// division at y is a Newton sequence: on the order of 10^2 instructions per row where the residual kernels spend three.  One
// workgroup is one CU: 14.3 + 12.6 us at 8192 rows and 27.0 + 21.5 us at 16384 (y + x+, kernel trace) where the
// residual kernels take 6.2 + 4.7 and 11.4 + 6.6 us - 2 % of a dense 16384 x 65536 trial, but 16 us of an 88 us sparse trial
// at 8192 rows (DESIGN 9 lists a lower wide threshold for these kernels).  Beyond 32768 rows - sparse problems have
// 10^5 .. 10^7 - the rows go to up to 1024 workgroups of 256 threads: 6.5 + 5.5 us at 200 000 rows beside the residual
// kernels' 4.8 + 4.5, plus the same 4.9 us finish each.
// (included by zf_solver.hip alone)
#pragma once
#include "zf_common.h"
#include "zf_spmv.h"

constexpr int ZF_ROWS_BLOCK = 1024;   // the one-workgroup shape of every rows pass (here and in zf_kernels_gap.h)

// ---- the row functions ------------------------------------------------------------------------------------------------------
// (include/zfista_hip.h: ZF_LOSS_SQUARE = 0, ZF_LOSS_LOGISTIC = 1, ZF_LOSS_HUBER = 2, ZF_LOSS_POISSON = 3)
//
// Logistic: phi = softplus(t), psi = rho = -b sigma(t), t = -b z, b in {-1, +1}; gfac = scale.  ONE e = exp(-|t|) <= 1 per row
// feeds both outputs -
//   softplus(t) = max(t, 0) + log1p(e),   sigma(t) = t >= 0 ? 1 / (1 + e) : e / (1 + e)
// - nothing overflows for any finite margin (|t| = 750: e = 0, softplus = max(t, 0), sigma in {0, 1}), and -b z is exact.
__device__ __forceinline__ double zf_softplus_of(double t, double e) { return fmax(t, 0.0) + log1p(e); }
__device__ __forceinline__ double zf_sigmoid_of(double t, double e) { return (t >= 0.0 ? 1.0 : e) / (1.0 + e); }

// Huber: phi = H(r) = r^2 (|r| <= delta) | delta (2 |r| - delta) (beyond), psi = c = clip(r, -delta, delta), r = z - b;
// gfac = 2 scale.  The same branch-free arithmetic in every kernel (and in the NumPy restatement of the tests):
//   c = copysign(min(|r|, delta), r)      no rounding beyond the one of r = z - b
//   H = c * (2 r - c)                     two roundings, never negative; an unclipped row gives r * r
// A NaN margin: v_min_f64 drops the NaN operand, so c alone would be +-delta - but 2 r - c is NaN and so are H and f.
__device__ __forceinline__ double zf_huber_clip(double r, double delta) { return copysign(fmin(fabs(r), delta), r); }
__device__ __forceinline__ double zf_huber_of(double r, double c) { return c * (2.0 * r - c); }

// Poisson with a log link: phi = exp(z) - b z, psi = exp(z) - b, counts b >= 0 (the constant log b! is dropped); gfac = scale:
//   e   = exp(z)          ONE exp per row - no log1p, no division
//   psi = e - b           one rounding
//   phi = e - b * z       two roundings (contraction is off)
// A margin beyond the range of exp gives e = +inf, phi = +inf and f = +inf - never NaN (inf - finite) - which the acceptance
// test rejects, so the line search backtracks out of an overflowing trial.  A NaN margin gives a NaN f.
//
// Square (with row weights only): psi = r = z - b, phi = r * r; gfac = 2 scale.
//
// psi and phi of one row; b is read only here, so a zero-weight row's b never reaches an output
template <int LOSS>
__device__ __forceinline__ void zf_loss_row(double z, double bi, double delta, double& psi, double& phi) {
    if (LOSS == ZF_LOSS_LOGISTIC) {
        const double t = -bi * z;
        const double e = exp(-fabs(t));
        psi = -bi * zf_sigmoid_of(t, e);
        phi = zf_softplus_of(t, e);
    } else if (LOSS == ZF_LOSS_HUBER) {
        const double rv = z - bi;
        psi = zf_huber_clip(rv, delta);
        phi = zf_huber_of(rv, psi);
    } else if (LOSS == ZF_LOSS_POISSON) {
        const double e = exp(z);
        psi = e - bi;
        phi = e - bi * z;
    } else {
        psi = z - bi;
        phi = psi * psi;
    }
}

// Row weights (W): ONE product for each output, rho_i = w_i * psi_i and acc += w_i * phi_i (-ffp-contract=off: two roundings per
// row, which NumPy reproduces bit for bit).  w_i == 0 is a row that is not there: rho_i = +0 and its term +0 by a select,
// whatever b_i holds (NaN and Inf included), so a fold may carry unlabeled rows.  A NaN margin on a row with w_i > 0 gives NaN
// f; a NaN weight is refused before it gets here (it would count as a row that is there).  !W: the term itself - no load of w,
// no select.  `on` is w_i != 0.
template <bool W>
__device__ __forceinline__ double zf_wterm(bool on, double wi, double t) {
    return W ? (on ? wi * t : 0.0) : t;
}

// ---- the rows kernel ------------------------------------------------------------------------------------------------------------
// the workgroup's sum: wave trees, then the wave sums in wave order (every thread holds it)
template <int BLOCK>
__device__ __forceinline__ double zf_rows_block_sum(double acc, double* lds) {
    acc = zf_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    double t = lds[0];
    for (int w = 1; w < BLOCK / 64; ++w) t += lds[w];
    return t;
}

// WHICH 0: at y - w o psi stored into r, sum of w phi; skipped unless the gradient is due.  WHICH 1: at s[(cur + slot) % 3].
// gridDim.x == 1: *f_out = scale * sum.  Otherwise part[blockIdx.x] = the chunk's sum (zf_rows_finish_kernel follows).
// !W: w is not read (NULL).  delta: Huber's threshold, unused by the other losses.
template <int LOSS, bool W, int WHICH, int BLOCK>
__global__ __launch_bounds__(BLOCK) void zf_loss_rows_kernel(const zf_control* ctl, const double* s0, const double* s1, const double* s2,
                                                             int slot, const double* __restrict__ b, const double* __restrict__ w,
                                                             double* __restrict__ r, int64_t m, int nesterov, double scale, double delta,
                                                             double* __restrict__ part, double* f_out) {
    __shared__ double lds[BLOCK / 64];
    const double* sr[3] = {s0, s1, s2};
    int cur = 0;
    double beta = 0.0;
    if (WHICH == 0) {
        if (ctl) {
            if (ctl->status != ZF_RUNNING || !ctl->need_grad) return;
            cur = ctl->cur;
            beta = nesterov ? ctl->beta_next : 0.0;
        } else {
            nesterov = 0;
        }
    } else if (slot >= 0) {
        if (ctl->status != ZF_RUNNING) return;
        cur = (ctl->cur + slot) % 3;
    }
    const double* __restrict__ sk = cur == 0 ? sr[0] : cur == 1 ? sr[1] : sr[2];
    const int o = (cur + 2) % 3;
    const double* __restrict__ so = o == 0 ? sr[0] : o == 1 ? sr[1] : sr[2];
    const int64_t per = (m + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < m ? lo + per : m;
    double acc = 0.0;
#pragma unroll 2
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
        double z = sk[i];
        if (WHICH == 0 && nesterov) z = z + beta * (z - so[i]);
        const double wi = W ? w[i] : 1.0;
        double psi, phi;
        zf_loss_row<LOSS>(z, b[i], delta, psi, phi);
        const bool on = wi != 0.0;
        if (WHICH == 0) r[i] = zf_wterm<W>(on, wi, psi);
        acc += zf_wterm<W>(on, wi, phi);
    }
    const double t = zf_rows_block_sum<BLOCK>(acc, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) *f_out = scale * t;
        else part[blockIdx.x] = t;
    }
}

// f = scale * (part[0] + part[1] + ...): thread t adds chunks t, t + 256, ... in that order, then the block sum
__global__ __launch_bounds__(ZF_BLOCK) void zf_rows_finish_kernel(const zf_control* ctl, int grad_guard, const double* __restrict__ part,
                                                                  int count, double scale, double* f_out) {
    __shared__ double lds[ZF_WAVES];
    if (ctl) {
        if (ctl->status != ZF_RUNNING) return;
        if (grad_guard && !ctl->need_grad) return;
    }
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += ZF_BLOCK) acc += part[i];
    const double t = zf_rows_block_sum<ZF_BLOCK>(acc, lds);
    if (threadIdx.x == 0) *f_out = scale * t;
}

// ---- the launcher ---------------------------------------------------------------------------------------------------------------
static inline bool zf_rows_wide(int64_t m) { return m > ZF_SPMV_WIDE_RESID_MIN_ROWS; }

// The two shapes of a rows pass over m rows, for the kernels here and the rows kernels of zf_kernels_gap.h: `narrow` is the
// ZF_ROWS_BLOCK instantiation, `wide` the ZF_BLOCK one, both called with args.  Returns 0 after the one-workgroup launch - the
// kernel has written its results itself - else the number of chunks whose sums the caller's finish kernel has to add.
template <typename K, typename... A>
static inline int zf_launch_rows_shapes(hipStream_t st, K narrow, K wide, int64_t m, A... args) {
    if (!zf_rows_wide(m)) {
        hipLaunchKernelGGL(narrow, dim3(1), dim3(ZF_ROWS_BLOCK), 0, st, args...);
        return 0;
    }
    const int chunks = zf_spmv_resid_chunks(m);   // (>= 33 here: never the one-workgroup branch of a kernel)
    hipLaunchKernelGGL(wide, dim3(chunks), dim3(ZF_BLOCK), 0, st, args...);
    return chunks;
}

// the arguments of one trial-side rows pass.  fin_ctl: the guard of the finish kernel (at y: ctl; at x+: ctl inside the loop,
// NULL for slot < 0, where ctl is not read); part: zf_spmv_resid_chunks(m) doubles of the caller (used above
// ZF_SPMV_WIDE_RESID_MIN_ROWS rows only; may be NULL below)
struct zf_rows_call {
    const zf_control *ctl, *fin_ctl;
    const double *s0, *s1, *s2;
    int slot;
    const double *b, *w;
    double* r;
    double scale, delta;
    int64_t m;
    int nesterov;
    double *part, *f_out;
    int K;   // the responses a row of the multinomial loss couples (zf_kernels_softmax.h); unread by the row losses here
};

template <int LOSS, bool W, int WHICH>
static inline void zf_launch_loss_rows(hipStream_t st, const zf_rows_call& c) {
    const int chunks = zf_launch_rows_shapes(st, zf_loss_rows_kernel<LOSS, W, WHICH, ZF_ROWS_BLOCK>, zf_loss_rows_kernel<LOSS, W, WHICH, ZF_BLOCK>,
                                             c.m, c.ctl, c.s0, c.s1, c.s2, c.slot, c.b, c.w, c.r, c.m, c.nesterov, c.scale, c.delta, c.part,
                                             c.f_out);
    if (chunks)
        hipLaunchKernelGGL(zf_rows_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, c.fin_ctl, WHICH == 0 ? 1 : 0, c.part, chunks, c.scale,
                           c.f_out);
}
