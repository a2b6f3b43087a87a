// zf_kernels_huber.h - Huber's loss of the margins s = A x (gfx950, fp64), switched on for the two least-squares kinds by
// zf_solver_set_huber:
//   f(x) = scale * sum_i H(r_i),  r = A x - b,  H(r) = r^2 (|r| <= delta) | delta (2 |r| - delta) (beyond);
//   grad f = 2 scale A^T c,  c = clip(r, -delta, delta)
// The same branch-free arithmetic in every kernel (and in the NumPy restatement of the tests):
//   c = copysign(min(|r|, delta), r)      no rounding beyond the one of r = z - b
//   H = c * (2 r - c)                     two roundings, never negative; an unclipped row gives r * r
// A NaN margin: v_min_f64 drops the NaN operand, so c alone would be +-delta - but 2 r - c is NaN and so are H and f.
// The sum is a plain sum (not sqrt()^2 as the squared loss: that mirrors numpy.linalg.norm(.)**2 of its closures).
//
// The two places of a trial (everything else of it is the least-squares kinds' own, the A^T sweep with the same 2 scale):
//   at y  (only when ctl->need_grad): z = s_k + beta (s_k - s_{k-1}) by linearity, c -> the residual buffer, f(y)
//   at x+ (every trial):              f(x+) from s+ = A x+
// Shapes, guards, ring indices, the row_part layout and the order of every sum are zf_logit_kernel's (zf_kernels_loss.h):
// one workgroup of 1024 threads up to ZF_SPMV_WIDE_RESID_MIN_ROWS rows, beyond it zf_spmv_resid_chunks(m) workgroups of 256
// threads on a contiguous chunk each and zf_logit_finish_kernel in chunk order - chosen by m alone for both storage forms,
// so the dense and the sparse class sum a loss of the same m in the same order.  No atomics, no scratch, two rows in
// flight per thread.  Bytes: 32 m at y (s_k, s_{k-1}, b, c), 16 m at x+ - the residual kernels' own.
//
// The rows pass of the duality gap (zf_gap_huber_rows_kernel) stores c and returns four sums that need no alpha:
//   sum H,  sum c^2,  sum b c,  T = sum |c| (|r| - |c|)          (every term of T >= 0, exactly 0 on an unclipped row)
//   D = -scale (alpha^2 sum c^2 + 2 alpha sum b c)      rows gap = scale (1 - alpha) ((1 - alpha) sum c^2 + 2 T)
// (included by zf_solver.hip alone, behind zf_kernels_gap.h)
#pragma once
#include "zf_kernels_gap.h"
#include "zf_kernels_loss.h"

__device__ __forceinline__ double zf_huber_clip(double r, double delta) { return copysign(fmin(fabs(r), delta), r); }
__device__ __forceinline__ double zf_huber_of(double r, double c) { return c * (2.0 * r - c); }

// WHICH 0: at y - c stored into r, sum of H; skipped unless the gradient is due.  WHICH 1: at s[(cur + slot) % 3].
// gridDim.x == 1: *f_out = scale * sum.  Otherwise part[blockIdx.x] = the chunk's sum (zf_logit_finish_kernel follows).
template <int WHICH, int BLOCK>
__global__ __launch_bounds__(BLOCK) void zf_huber_kernel(const zf_control* ctl, const double* s0, const double* s1, const double* s2,
                                                         int slot, const double* __restrict__ b, double* __restrict__ r, int64_t m,
                                                         int nesterov, double scale, double delta, double* __restrict__ part,
                                                         double* f_out) {
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
        const double rv = z - b[i];
        const double c = zf_huber_clip(rv, delta);
        if (WHICH == 0) r[i] = c;
        acc += zf_huber_of(rv, c);
    }
    const double t = zf_logit_block_sum<BLOCK>(acc, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) *f_out = scale * t;
        else part[blockIdx.x] = t;
    }
}

// c(y) -> r and f(y) -> *f_out.  ctl != NULL: inside the loop (guards, ring, momentum); NULL: c and f at the margins s0.
// part: zf_spmv_resid_chunks(m) doubles of the caller (read beyond ZF_SPMV_WIDE_RESID_MIN_ROWS rows only)
static inline void zf_launch_huber_y(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2,
                                     const double* b, double* r, double scale, double delta, int64_t m, int nesterov, double* part,
                                     double* f_out) {
    if (!zf_logit_wide(m)) {
        hipLaunchKernelGGL((zf_huber_kernel<0, ZF_LOGIT_BLOCK>), dim3(1), dim3(ZF_LOGIT_BLOCK), 0, st, ctl, s0, s1, s2, 0, b, r, m, nesterov,
                           scale, delta, part, f_out);
        return;
    }
    const int chunks = zf_spmv_resid_chunks(m);   // (>= 33 here: never the one-workgroup branch of the kernel)
    hipLaunchKernelGGL((zf_huber_kernel<0, ZF_BLOCK>), dim3(chunks), dim3(ZF_BLOCK), 0, st, ctl, s0, s1, s2, 0, b, r, m, nesterov, scale,
                       delta, part, f_out);
    hipLaunchKernelGGL(zf_logit_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ctl, 1, part, chunks, scale, f_out);
}

// f at the margins s[(cur + slot) % 3] (slot >= 0: inside the loop) or s0 (slot < 0: ctl is not read) -> *f_out
static inline void zf_launch_huber_x(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2, int slot,
                                     const double* b, double scale, double delta, int64_t m, double* part, double* f_out) {
    if (!zf_logit_wide(m)) {
        hipLaunchKernelGGL((zf_huber_kernel<1, ZF_LOGIT_BLOCK>), dim3(1), dim3(ZF_LOGIT_BLOCK), 0, st, ctl, s0, s1, s2, slot, b, nullptr, m, 0,
                           scale, delta, part, f_out);
        return;
    }
    const int chunks = zf_spmv_resid_chunks(m);
    hipLaunchKernelGGL((zf_huber_kernel<1, ZF_BLOCK>), dim3(chunks), dim3(ZF_BLOCK), 0, st, ctl, s0, s1, s2, slot, b, nullptr, m, 0, scale,
                       delta, part, f_out);
    hipLaunchKernelGGL(zf_logit_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, slot >= 0 ? ctl : nullptr, 0, part, chunks, scale, f_out);
}

// ---- duality gap: the rows pass -----------------------------------------------------------------------------------------------
// scalar slots: sum c^2 and sum b c where the least-squares rows leave sum r^2 and sum b r (the dual and the screen's |c|_2
// read them there), sum H and T in the two slots of the logistic rows (unused by a least-squares kind)
enum { ZF_GS_HSUM = ZF_GS_KL, ZF_GS_HT = ZF_GS_ENT };
// chunk sums: four rows of ZF_GAP_MAX_CHUNKS - one more than ZF_GAP_PART: the workspace of a Huber evaluation is longer by it
constexpr int ZF_GAP_PART_HUBER = 4 * ZF_GAP_MAX_CHUNKS;

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void zf_gap_huber_rows_kernel(const double* __restrict__ z, const double* __restrict__ b,
                                                                  double* __restrict__ cvec, int64_t m, double scale, double delta,
                                                                  double* __restrict__ part, double* __restrict__ scal) {
    __shared__ double lds[2 * BLOCK / 64];
    int64_t lo, hi;
    zf_gap_chunk_of(m, lo, hi);
    double hs = 0.0, cc = 0.0, bc = 0.0, tt = 0.0;
#pragma unroll 2
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
        const double bi = b[i];
        const double rv = z[i] - bi;
        const double c = zf_huber_clip(rv, delta);
        const double ac = fabs(c);
        cvec[i] = c;
        hs += zf_huber_of(rv, c);
        cc += c * c;
        bc += bi * c;
        tt += ac * (fabs(rv) - ac);
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

// composition (one thread).  enet == 0: the eight values of zf_gap_compose_kernel at ZF_GS_OUT; else the ten of
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

// step 1 of a Huber evaluation: c -> ws.rvec and the four row sums (ws.part: ZF_GAP_PART_HUBER doubles)
static inline void zf_launch_gap_huber_rows(hipStream_t st, const double* z, const double* b, int64_t m, double scale, double delta,
                                            const zf_gap_ws& ws) {
    if (!zf_logit_wide(m)) {
        hipLaunchKernelGGL(zf_gap_huber_rows_kernel<ZF_GAP_ROWS_BLOCK>, dim3(1), dim3(ZF_GAP_ROWS_BLOCK), 0, st, z, b, ws.rvec, m, scale,
                           delta, ws.part, ws.scal);
        return;
    }
    const int chunks = zf_spmv_resid_chunks(m);
    hipLaunchKernelGGL(zf_gap_huber_rows_kernel<ZF_BLOCK>, dim3(chunks), dim3(ZF_BLOCK), 0, st, z, b, ws.rvec, m, scale, delta, ws.part,
                       ws.scal);
    hipLaunchKernelGGL(zf_gap_sum_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, chunks, (int)ZF_GS_RR, (int)ZF_GS_BR, -1.0, ws.scal);
    hipLaunchKernelGGL(zf_gap_huber_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ws.part, chunks, scale, ws.scal);
}

// steps 3 .. 6 with g = grad f(x) in ws.g: the n-passes of the l1 / elastic-net evaluation unchanged, then the Huber composition
static inline void zf_launch_gap_tail_huber(hipStream_t st, const double* x, int64_t n, double scale, double lam, double l2,
                                            const zf_gap_ws& ws) {
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
    hipLaunchKernelGGL(zf_gap_compose_huber_kernel, dim3(1), dim3(64), 0, st, l2 > 0.0 ? 1 : 0, scale, lam, l2, ws.scal);
}
