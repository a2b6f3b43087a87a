// zf_kernels_wloss.h - per-row sample weights on the three losses of the margins s = A x (gfx950, fp64), switched on for the
// four margins kinds by zf_solver_set_row_weights:
//   f(x) = scale * sum_i w_i phi_i(z_i),   grad f = gfac * A^T (w o psi(z)),   gfac = 2 scale (square, Huber) | scale (logistic)
// phi and psi per row exactly as the unweighted kernels form them:
//   ZF_LOSS_SQUARE    r = z - b              psi = r                          phi = r * r
//   ZF_LOSS_HUBER     r = z - b              psi = c = zf_huber_clip(r)       phi = zf_huber_of(r, c) = c (2 r - c)
//   ZF_LOSS_LOGISTIC  t = -b z, e = exp(-|t|) psi = -b zf_sigmoid_of(t, e)     phi = zf_softplus_of(t, e)
//   ZF_LOSS_POISSON   e = exp(z)             psi = e - b                      phi = e - b z       (zf_poisson_row)
// then ONE product for each output: rho_i = w_i * psi_i and acc += w_i * phi_i (-ffp-contract=off: two roundings per row,
// which NumPy reproduces bit for bit).  The sum is a plain sum, multiplied by scale once at the end - not the sqrt()^2 of the
// unweighted squared loss.  w_i == 0 is a row that is not there: rho_i = +0 and its term +0 by a select, whatever b_i holds
// (NaN and Inf included), so a fold may carry unlabeled rows.  A NaN margin on a row with w_i > 0 gives NaN f.
//
// zf_wloss_kernel<LOSS, WHICH, BLOCK> is zf_logit_kernel (zf_kernels_loss.h) with one more read stream: guards, ring indices,
// momentum by linearity, two rows in flight per thread, thread-to-row order, the gridDim.x == 1 / chunk-sum split and
// zf_logit_block_sum are its own; beyond ZF_SPMV_WIDE_RESID_MIN_ROWS rows zf_logit_finish_kernel follows, unchanged.  Shapes by m
// alone (zf_logit_wide) for both storage forms.  No atomics, no scratch, no LDS beyond the block sum.
// Bytes: 40 m at y (s_k, s_{k-1}, b, w, rho), 24 m at x+ (s+, b, w) - 8 m more than the unweighted kernels at each place.
//
// The rows passes of the duality gap: every row term of zf_gap_ls_rows_kernel / zf_gap_huber_rows_kernel / zf_gap_kl_kernel
// times w_i, in the same two shapes, into the same scalar slots - (w phi)^*(w u) = w phi^*(u), so the dual point
// nu = alpha grad phi(z), the n-passes and the three composition kernels are reused unchanged; rvec receives w o psi, so the
// caller's column sweep yields the weighted gradient and alpha = min(1, lam / |g|_inf) needs no change:
//   square    sum w r^2, sum w b r                       f = scale sum w r^2
//   Huber     sum w H, sum w c^2, sum w b c, sum w |c| (|r| - |c|)
//   logistic  sum w KL(alpha q || q), sum w [p log p + (1 - p) log(1 - p)]
//   Poisson   sum w [row gap], sum w (v log v - v)       (zf_gap_poisson_kernel with w, zf_kernels_poisson.h)
// (included by zf_solver.hip alone, behind zf_kernels_huber.h)
#pragma once
#include "zf_kernels_huber.h"
#include "zf_kernels_poisson.h"

// (include/zfista_hip.h: ZF_LOSS_SQUARE = 0, ZF_LOSS_LOGISTIC = 1, ZF_LOSS_HUBER = 2, ZF_LOSS_POISSON = 3)

// psi and phi of one row; b is read only here, so a zero-weight row's b never reaches an output
template <int LOSS>
__device__ __forceinline__ void zf_wloss_row(double z, double bi, double delta, double& psi, double& phi) {
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
        zf_poisson_row(z, bi, psi, phi);
    } else {
        psi = z - bi;
        phi = psi * psi;
    }
}

// WHICH 0: at y - w o psi stored into r, sum of w phi; skipped unless the gradient is due.  WHICH 1: at s[(cur + slot) % 3].
// gridDim.x == 1: *f_out = scale * sum.  Otherwise part[blockIdx.x] = the chunk's sum (zf_logit_finish_kernel follows).
template <int LOSS, int WHICH, int BLOCK>
__global__ __launch_bounds__(BLOCK) void zf_wloss_kernel(const zf_control* ctl, const double* s0, const double* s1, const double* s2,
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
        const double wi = w[i];
        double psi, phi;
        zf_wloss_row<LOSS>(z, b[i], delta, psi, phi);
        const bool on = wi != 0.0;   // (a NaN weight is refused before it gets here; it would count as a row that is there)
        if (WHICH == 0) r[i] = on ? wi * psi : 0.0;
        acc += on ? wi * phi : 0.0;
    }
    const double t = zf_logit_block_sum<BLOCK>(acc, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) *f_out = scale * t;
        else part[blockIdx.x] = t;
    }
}

template <int LOSS, int WHICH>
static inline void zf_launch_wloss_shape(hipStream_t st, const zf_control* ctl, const zf_control* fin_ctl, const double* s0, const double* s1,
                                         const double* s2, int slot, const double* b, const double* w, double* r, double scale,
                                         double delta, int64_t m, int nesterov, double* part, double* f_out) {
    if (!zf_logit_wide(m)) {
        hipLaunchKernelGGL((zf_wloss_kernel<LOSS, WHICH, ZF_LOGIT_BLOCK>), dim3(1), dim3(ZF_LOGIT_BLOCK), 0, st, ctl, s0, s1, s2, slot, b, w, r,
                           m, nesterov, scale, delta, part, f_out);
        return;
    }
    const int chunks = zf_spmv_resid_chunks(m);   // (>= 33 here: never the one-workgroup branch of the kernel)
    hipLaunchKernelGGL((zf_wloss_kernel<LOSS, WHICH, ZF_BLOCK>), dim3(chunks), dim3(ZF_BLOCK), 0, st, ctl, s0, s1, s2, slot, b, w, r, m,
                       nesterov, scale, delta, part, f_out);
    hipLaunchKernelGGL(zf_logit_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, fin_ctl, WHICH == 0 ? 1 : 0, part, chunks, scale, f_out);
}

// w o psi(y) -> r and f(y) -> *f_out.  ctl != NULL: inside the loop (guards, ring, momentum); NULL: at the margins s0.
// part: zf_spmv_resid_chunks(m) doubles of the caller (read beyond ZF_SPMV_WIDE_RESID_MIN_ROWS rows only)
static inline void zf_launch_wloss_y(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2,
                                     const double* b, const double* w, double* r, double scale, int loss, double delta, int64_t m,
                                     int nesterov, double* part, double* f_out) {
    if (loss == ZF_LOSS_LOGISTIC)
        zf_launch_wloss_shape<ZF_LOSS_LOGISTIC, 0>(st, ctl, ctl, s0, s1, s2, 0, b, w, r, scale, delta, m, nesterov, part, f_out);
    else if (loss == ZF_LOSS_HUBER)
        zf_launch_wloss_shape<ZF_LOSS_HUBER, 0>(st, ctl, ctl, s0, s1, s2, 0, b, w, r, scale, delta, m, nesterov, part, f_out);
    else if (loss == ZF_LOSS_POISSON)
        zf_launch_wloss_shape<ZF_LOSS_POISSON, 0>(st, ctl, ctl, s0, s1, s2, 0, b, w, r, scale, delta, m, nesterov, part, f_out);
    else
        zf_launch_wloss_shape<ZF_LOSS_SQUARE, 0>(st, ctl, ctl, s0, s1, s2, 0, b, w, r, scale, delta, m, nesterov, part, f_out);
}

// f at the margins s[(cur + slot) % 3] (slot >= 0: inside the loop) or s0 (slot < 0: ctl is not read) -> *f_out
static inline void zf_launch_wloss_x(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2, int slot,
                                     const double* b, const double* w, double scale, int loss, double delta, int64_t m, double* part,
                                     double* f_out) {
    const zf_control* fin = slot >= 0 ? ctl : nullptr;
    if (loss == ZF_LOSS_LOGISTIC)
        zf_launch_wloss_shape<ZF_LOSS_LOGISTIC, 1>(st, ctl, fin, s0, s1, s2, slot, b, w, nullptr, scale, delta, m, 0, part, f_out);
    else if (loss == ZF_LOSS_HUBER)
        zf_launch_wloss_shape<ZF_LOSS_HUBER, 1>(st, ctl, fin, s0, s1, s2, slot, b, w, nullptr, scale, delta, m, 0, part, f_out);
    else if (loss == ZF_LOSS_POISSON)
        zf_launch_wloss_shape<ZF_LOSS_POISSON, 1>(st, ctl, fin, s0, s1, s2, slot, b, w, nullptr, scale, delta, m, 0, part, f_out);
    else
        zf_launch_wloss_shape<ZF_LOSS_SQUARE, 1>(st, ctl, fin, s0, s1, s2, slot, b, w, nullptr, scale, delta, m, 0, part, f_out);
}

// ---- duality gap: the weighted rows passes ------------------------------------------------------------------------------------
// square: w r -> rvec, sum w r^2, sum w b r; f = scale sum w r^2 (plain)
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

// Huber: w c -> cvec and the four weighted sums, in the slots and chunk rows of zf_gap_huber_rows_kernel
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void zf_gap_whuber_rows_kernel(const double* __restrict__ z, const double* __restrict__ b,
                                                                   const double* __restrict__ w, double* __restrict__ cvec, int64_t m,
                                                                   double scale, double delta, double* __restrict__ part,
                                                                   double* __restrict__ scal) {
    __shared__ double lds[2 * BLOCK / 64];
    int64_t lo, hi;
    zf_gap_chunk_of(m, lo, hi);
    double hs = 0.0, cc = 0.0, bc = 0.0, tt = 0.0;
#pragma unroll 2
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
        const double bi = b[i], wi = w[i];
        const double rv = z[i] - bi;
        const double c = zf_huber_clip(rv, delta);
        const double ac = fabs(c);
        const bool on = wi != 0.0;
        cvec[i] = on ? wi * c : 0.0;
        hs += on ? wi * zf_huber_of(rv, c) : 0.0;
        cc += on ? wi * (c * c) : 0.0;
        bc += on ? wi * (bi * c) : 0.0;
        tt += on ? wi * (ac * (fabs(rv) - ac)) : 0.0;
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

// logistic: sum_i w_i KL(alpha q_i || q_i) and sum_i w_i [p log p + (1 - p) log(1 - p)] - zf_gap_kl_kernel's row, times w_i
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void zf_gap_wkl_kernel(const double* __restrict__ z, const double* __restrict__ b,
                                                           const double* __restrict__ w, int64_t m, double* __restrict__ part,
                                                           double* __restrict__ scal) {
    __shared__ double lds[2 * BLOCK / 64];
    const double alpha = scal[ZF_GS_ALPHA], oma = scal[ZF_GS_OMA], aloga = scal[ZF_GS_ALOGA];
    int64_t lo, hi;
    zf_gap_chunk_of(m, lo, hi);
    double kl = 0.0, ent = 0.0;
#pragma unroll 2
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
        const double wi = w[i];
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
            kl += on ? wi * k : 0.0;
        }
        const double en = (p == 0.0 ? 0.0 : p * log(p)) + (omp == 0.0 ? 0.0 : omp * log(omp));
        ent += on ? wi * en : 0.0;
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

// step 1 of a weighted evaluation: w o psi -> ws.rvec and the row sums that need no alpha (ws.part: ZF_GAP_PART doubles,
// ZF_GAP_PART_HUBER for Huber's loss)
static inline void zf_launch_gap_wrows(hipStream_t st, int loss, const double* z, const double* b, const double* w, int64_t m, double scale,
                                       double delta, const zf_gap_ws& ws) {
    if (loss == ZF_LOSS_LOGISTIC || loss == ZF_LOSS_POISSON) {   // w psi and f by the loss kernels of a trial, called outside the loop
        zf_launch_wloss_y(st, nullptr, z, z, z, b, w, ws.rvec, scale, loss, 0.0, m, 0, ws.part + 2 * ZF_GAP_MAX_CHUNKS,
                          ws.scal + ZF_GS_F);
        return;
    }
    const bool wide = zf_logit_wide(m);
    const int chunks = wide ? zf_spmv_resid_chunks(m) : 1;
    if (loss == ZF_LOSS_HUBER) {
        if (!wide) {
            hipLaunchKernelGGL(zf_gap_whuber_rows_kernel<ZF_GAP_ROWS_BLOCK>, dim3(1), dim3(ZF_GAP_ROWS_BLOCK), 0, st, z, b, w, ws.rvec, m, scale,
                               delta, ws.part, ws.scal);
            return;
        }
        hipLaunchKernelGGL(zf_gap_whuber_rows_kernel<ZF_BLOCK>, dim3(chunks), dim3(ZF_BLOCK), 0, st, z, b, w, ws.rvec, m, scale, delta, ws.part,
                           ws.scal);
        hipLaunchKernelGGL(zf_gap_sum_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, chunks, (int)ZF_GS_RR, (int)ZF_GS_BR, -1.0, ws.scal);
        hipLaunchKernelGGL(zf_gap_huber_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, chunks, scale, ws.scal);
        return;
    }
    if (!wide) {
        hipLaunchKernelGGL(zf_gap_wls_rows_kernel<ZF_GAP_ROWS_BLOCK>, dim3(1), dim3(ZF_GAP_ROWS_BLOCK), 0, st, z, b, w, ws.rvec, m, scale,
                           ws.part, ws.scal);
        return;
    }
    hipLaunchKernelGGL(zf_gap_wls_rows_kernel<ZF_BLOCK>, dim3(chunks), dim3(ZF_BLOCK), 0, st, z, b, w, ws.rvec, m, scale, ws.part, ws.scal);
    hipLaunchKernelGGL(zf_gap_sum_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, chunks, (int)ZF_GS_RR, (int)ZF_GS_BR, -1.0, ws.scal);
    // f = scale * (the first row of chunk sums, added in the same order): the plain form, no sqrt()^2
    hipLaunchKernelGGL(zf_logit_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, nullptr, 0, ws.part, chunks, scale, ws.scal + ZF_GS_F);
}

// steps 3 .. 6 of a weighted evaluation with g = grad f(x) in ws.g: the n-passes and the composition kernels of the unweighted
// evaluation, the weighted KL rows for the logistic loss
static inline void zf_launch_gap_wtail(hipStream_t st, int loss, const double* z, const double* b, const double* w, const double* x,
                                       int64_t m, int64_t n, double scale, double lam, double l2, const zf_gap_ws& ws) {
    if (loss == ZF_LOSS_HUBER) {   // (no row pass behind the n-passes: its composition reads the four sums of step 1)
        zf_launch_gap_tail_huber(st, x, n, scale, lam, l2, ws);
        return;
    }
    if (loss == ZF_LOSS_POISSON) {   // (its second rows pass takes the weights itself)
        zf_launch_gap_tail_poisson(st, z, b, w, x, m, n, scale, lam, l2, ws);
        return;
    }
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
    const bool logistic = loss == ZF_LOSS_LOGISTIC;
    if (logistic) {
        if (!zf_logit_wide(m)) {
            hipLaunchKernelGGL(zf_gap_wkl_kernel<ZF_GAP_ROWS_BLOCK>, dim3(1), dim3(ZF_GAP_ROWS_BLOCK), 0, st, z, b, w, m, ws.part, ws.scal);
        } else {
            const int chunks = zf_spmv_resid_chunks(m);
            hipLaunchKernelGGL(zf_gap_wkl_kernel<ZF_BLOCK>, dim3(chunks), dim3(ZF_BLOCK), 0, st, z, b, w, m, ws.part, ws.scal);
            hipLaunchKernelGGL(zf_gap_sum_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, chunks, (int)ZF_GS_KL, (int)ZF_GS_ENT, -1.0, ws.scal);
        }
    }
    if (l2 > 0.0) hipLaunchKernelGGL(zf_gap_compose_enet_kernel, dim3(1), dim3(64), 0, st, logistic ? 1 : 0, scale, lam, l2, ws.scal);
    else hipLaunchKernelGGL(zf_gap_compose_kernel, dim3(1), dim3(64), 0, st, logistic ? 1 : 0, scale, lam, ws.scal);
}
