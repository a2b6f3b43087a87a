// zf_kernels_poisson.h - the Poisson loss with a log link on the margins s = A x (gfx950, fp64), switched on for the two
// least-squares kinds by zf_solver_set_poisson:
//   f(x) = scale * sum_i (exp(z_i) - b_i z_i),  z = A x,  counts b_i >= 0 (the constant log b! is dropped);
//   grad f = scale * A^T psi,  psi_i = exp(z_i) - b_i
// The same arithmetic in every kernel (and in the NumPy restatement of the tests):
//   e   = exp(z)          ONE exp per row - no log1p, no division
//   psi = e - b           one rounding
//   phi = e - b * z       two roundings (contraction is off)
// A margin beyond the range of exp gives e = +inf, phi = +inf and f = +inf - never NaN (inf - finite) - which the acceptance
// test rejects, so the line search backtracks out of an overflowing trial.  A NaN margin gives a NaN f.
// The sum is a plain sum, multiplied by scale once.
//
// The two places of a trial (everything else of it is the least-squares kinds' own, the A^T sweep with `scale` for `2 scale`):
//   at y  (only when ctl->need_grad): z = s_k + beta (s_k - s_{k-1}) by linearity, psi -> the residual buffer, f(y)
//   at x+ (every trial):              f(x+) from s+ = A x+
// Shapes, guards, ring indices, the row_part layout and the order of every sum are zf_logit_kernel's (zf_kernels_loss.h):
// one workgroup of 1024 threads up to ZF_SPMV_WIDE_RESID_MIN_ROWS rows, beyond it zf_spmv_resid_chunks(m) workgroups of 256
// threads on a contiguous chunk each and zf_logit_finish_kernel in chunk order - chosen by m alone for both storage forms,
// so the dense and the sparse class sum a loss of the same m in the same order.  No atomics, no scratch, two rows in
// flight per thread, no LDS beyond the block sum.  Bytes: 32 m at y (s_k, s_{k-1}, b, psi), 16 m at x+ - the residual kernels' own.
//
// The duality gap.  h(z) = e^z - b z has the conjugate h^*(u) = v log v - v, v = u + b >= 0 (0 log 0 = 0); the dual point
// nu = alpha grad phi(z) gives v = alpha e^z + (1 - alpha) b >= 0 always: feasible for every alpha in [0, 1].
//   D = -scale sum_i (v_i log v_i - v_i)
//   rows = scale sum_i [e^z - v + v (log v - z)],  each term = e^z ((1 + d) log1p(d) - d),  d = (1 - alpha)(b - e^z) / e^z >= -1
// every term >= 0 and exactly 0 at alpha = 1 (the pass is skipped, as zf_gap_kl_kernel's).  The row terms depend on alpha, so
// - as for the logistic loss - a second rows pass follows the n-passes (zf_gap_poisson_kernel); it leaves its two sums in the
// slots of the logistic rows (ZF_GS_KL, ZF_GS_ENT), and the composition kernels' logistic arm - rows = scale [KL slot],
// D = -scale [ENT slot] - writes the eight or ten outputs.  1 - alpha and alpha log alpha are read from device memory
// (zf_gap_alpha), never formed from a rounded alpha.  Per row:
//   b = 0:            e (alpha log alpha + (1 - alpha))                            (v = alpha e)
//   d <= 1:           e ((alpha + (1 - alpha) b / e) log1p(d) - d)                 (1 + d as a sum of two terms >= 0)
//   d > 1, e = 0:     (e - v) + v (log v - z)   - the direct form: no cancellation there (log v - z >= log 2), and finite
//                     where b / e overflows (z = -700) or e has underflowed to 0
// finite for every |z| <= 700 and every count b < 1e300.  Weighted evaluation (w != NULL): every row term times w_i, a row with
// w_i = 0 contributes +0 whatever b_i holds.
// (included by zf_solver.hip alone, behind zf_kernels_gap.h; zf_kernels_wloss.h reads zf_poisson_row)
#pragma once
#include "zf_kernels_gap.h"
#include "zf_kernels_loss.h"

// psi and phi of one row from the ONE exp
__device__ __forceinline__ void zf_poisson_row(double z, double bi, double& psi, double& phi) {
    const double e = exp(z);
    psi = e - bi;
    phi = e - bi * z;
}

// WHICH 0: at y - psi stored into r, sum of phi; skipped unless the gradient is due.  WHICH 1: at s[(cur + slot) % 3].
// gridDim.x == 1: *f_out = scale * sum.  Otherwise part[blockIdx.x] = the chunk's sum (zf_logit_finish_kernel follows).
template <int WHICH, int BLOCK>
__global__ __launch_bounds__(BLOCK) void zf_poisson_kernel(const zf_control* ctl, const double* s0, const double* s1, const double* s2,
                                                           int slot, const double* __restrict__ b, double* __restrict__ r, int64_t m,
                                                           int nesterov, double scale, double* __restrict__ part, double* f_out) {
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
        double psi, phi;
        zf_poisson_row(z, b[i], psi, phi);
        if (WHICH == 0) r[i] = psi;
        acc += phi;
    }
    const double t = zf_logit_block_sum<BLOCK>(acc, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) *f_out = scale * t;
        else part[blockIdx.x] = t;
    }
}

// psi(y) -> r and f(y) -> *f_out.  ctl != NULL: inside the loop (guards, ring, momentum); NULL: psi and f at the margins s0.
// part: zf_spmv_resid_chunks(m) doubles of the caller (read beyond ZF_SPMV_WIDE_RESID_MIN_ROWS rows only)
static inline void zf_launch_poisson_y(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2,
                                       const double* b, double* r, double scale, int64_t m, int nesterov, double* part, double* f_out) {
    if (!zf_logit_wide(m)) {
        hipLaunchKernelGGL((zf_poisson_kernel<0, ZF_LOGIT_BLOCK>), dim3(1), dim3(ZF_LOGIT_BLOCK), 0, st, ctl, s0, s1, s2, 0, b, r, m, nesterov,
                           scale, part, f_out);
        return;
    }
    const int chunks = zf_spmv_resid_chunks(m);   // (>= 33 here: never the one-workgroup branch of the kernel)
    hipLaunchKernelGGL((zf_poisson_kernel<0, ZF_BLOCK>), dim3(chunks), dim3(ZF_BLOCK), 0, st, ctl, s0, s1, s2, 0, b, r, m, nesterov, scale,
                       part, f_out);
    hipLaunchKernelGGL(zf_logit_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ctl, 1, part, chunks, scale, f_out);
}

// f at the margins s[(cur + slot) % 3] (slot >= 0: inside the loop) or s0 (slot < 0: ctl is not read) -> *f_out
static inline void zf_launch_poisson_x(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2, int slot,
                                       const double* b, double scale, int64_t m, double* part, double* f_out) {
    if (!zf_logit_wide(m)) {
        hipLaunchKernelGGL((zf_poisson_kernel<1, ZF_LOGIT_BLOCK>), dim3(1), dim3(ZF_LOGIT_BLOCK), 0, st, ctl, s0, s1, s2, slot, b, nullptr, m, 0,
                           scale, part, f_out);
        return;
    }
    const int chunks = zf_spmv_resid_chunks(m);
    hipLaunchKernelGGL((zf_poisson_kernel<1, ZF_BLOCK>), dim3(chunks), dim3(ZF_BLOCK), 0, st, ctl, s0, s1, s2, slot, b, nullptr, m, 0, scale,
                       part, f_out);
    hipLaunchKernelGGL(zf_logit_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, slot >= 0 ? ctl : nullptr, 0, part, chunks, scale, f_out);
}

// ---- duality gap: the second rows pass ------------------------------------------------------------------------------------
// the Fenchel-Young gap of one row (>= 0) and v log v - v, v = alpha e + (1 - alpha) b; oma != 0 (the caller skips alpha = 1)
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

// sum_i w_i [row gap] -> ZF_GS_KL and sum_i w_i (v log v - v) -> ZF_GS_ENT (w == NULL: every w_i = 1), in the two shapes and the
// chunk rows of zf_gap_kl_kernel.  alpha = 1 (oma == 0): v = e exactly and every row gap is exactly 0 - not formed.
template <int BLOCK>
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
        const double wi = w ? w[i] : 1.0;
        const bool on = wi != 0.0;
        const double zi = z[i];
        double k = 0.0, en;
        if (oma != 0.0) {   // (a NaN alpha takes this branch)
            zf_poisson_gap_row(zi, b[i], alpha, oma, aloga, k, en);
        } else {
            const double e = exp(zi);
            en = e == 0.0 ? 0.0 : e * log(e) - e;
        }
        if (w) {
            gs += on ? wi * k : 0.0;
            ent += on ? wi * en : 0.0;
        } else {
            gs += k;
            ent += en;
        }
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

// steps 3 .. 6 of a Poisson evaluation with g = grad f(x) in ws.g: the n-passes of the l1 / elastic-net evaluation unchanged, the
// second rows pass (w: the row weights or NULL), then the composition kernels' logistic arm (its two sums lie in those slots)
static inline void zf_launch_gap_tail_poisson(hipStream_t st, const double* z, const double* b, const double* w, const double* x, int64_t m,
                                              int64_t n, double scale, double lam, double l2, const zf_gap_ws& ws) {
    const int nc = zf_gap_chunks(n);
    if (l2 > 0.0) {
        hipLaunchKernelGGL(zf_gap_ginf_enet_kernel, dim3(nc), dim3(ZF_BLOCK), 0, st, ws.g, x, l2, n, lam, ws.part, ws.scal);
        if (nc > 1) hipLaunchKernelGGL(zf_gap_ginf_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, nc, lam, ws.scal);
        hipLaunchKernelGGL(zf_gap_cols_enet_kernel, dim3(nc), dim3(ZF_BLOCK), 0, st, x, ws.g, l2, n, lam, ws.part, ws.scal);
        if (nc > 1) {
            hipLaunchKernelGGL(zf_gap_sum_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, nc, (int)ZF_GS_COLS, (int)ZF_GS_ASUM, -1.0, ws.scal);
            hipLaunchKernelGGL(zf_gap_sum_third_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, nc, (int)ZF_GS_XX, ws.scal);
        }
    } else {
        hipLaunchKernelGGL(zf_gap_ginf_kernel, dim3(nc), dim3(ZF_BLOCK), 0, st, ws.g, n, lam, ws.part, ws.scal);
        if (nc > 1) hipLaunchKernelGGL(zf_gap_ginf_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, nc, lam, ws.scal);
        hipLaunchKernelGGL(zf_gap_cols_kernel, dim3(nc), dim3(ZF_BLOCK), 0, st, x, ws.g, n, lam, ws.part, ws.scal);
        if (nc > 1)
            hipLaunchKernelGGL(zf_gap_sum_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, nc, (int)ZF_GS_COLS, (int)ZF_GS_ASUM, -1.0, ws.scal);
    }
    if (!zf_logit_wide(m)) {
        hipLaunchKernelGGL(zf_gap_poisson_kernel<ZF_GAP_ROWS_BLOCK>, dim3(1), dim3(ZF_GAP_ROWS_BLOCK), 0, st, z, b, w, m, ws.part, ws.scal);
    } else {
        const int chunks = zf_spmv_resid_chunks(m);
        hipLaunchKernelGGL(zf_gap_poisson_kernel<ZF_BLOCK>, dim3(chunks), dim3(ZF_BLOCK), 0, st, z, b, w, m, ws.part, ws.scal);
        hipLaunchKernelGGL(zf_gap_sum_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, chunks, (int)ZF_GS_KL, (int)ZF_GS_ENT, -1.0, ws.scal);
    }
    if (l2 > 0.0) hipLaunchKernelGGL(zf_gap_compose_enet_kernel, dim3(1), dim3(64), 0, st, 1, scale, lam, l2, ws.scal);
    else hipLaunchKernelGGL(zf_gap_compose_kernel, dim3(1), dim3(64), 0, st, 1, scale, lam, ws.scal);
}
