// zf_kernels_loss.h - the logistic loss of the margins s = A x (gfx950, fp64):
//   f(x) = scale * sum_i softplus(t_i),  t_i = -b_i s_i,  b_i in {-1, +1};   grad f = scale * A^T rho,  rho_i = -b_i sigma(t_i)
// the two places of a trial where the loss enters (ZF_PROBLEM_LOGISTIC_L1, ZF_PROBLEM_SPARSE_LOGISTIC_L1) - everything
// else of the trial is the least-squares kinds' (zf_launch_trial), with the sweeps called with `scale` for their `2 scale`:
//   at y  (only when ctl->need_grad): z = s_k + beta (s_k - s_{k-1}) by linearity, rho -> the residual buffer, f(y)
//   at x+ (every trial):              f(x+) from s+ = A x+
// Numerics: ONE e = exp(-|t|) <= 1 per element feeds both outputs -
//   softplus(t) = max(t, 0) + log1p(e),   sigma(t) = t >= 0 ? 1 / (1 + e) : e / (1 + e)
// - nothing overflows for any finite margin (|t| = 750: e = 0, softplus = max(t, 0), sigma in {0, 1}), and -b z is exact.
// The sum is NOT passed through sqrt()^2 as the squared loss is (that mirrors numpy.linalg.norm(.)**2 of the reference's
// closures; the reference form of this loss is a plain sum).
//
// Two shapes, one kernel body (zf_logit_kernel<WHICH, BLOCK>):
//   one workgroup of 1024 threads, thread t takes rows t, t + 1024, ... in that order, and writes f itself - the shape of
//     zf_resid_y_kernel / zf_resid_x_kernel, for the row counts of the dense class;
//   zf_spmv_resid_chunks(m) workgroups of 256 threads on a contiguous chunk each -> part[chunk], then ONE workgroup adds
//     the chunk sums in chunk order (zf_logit_finish_kernel) - the shape of zf_spmv_resid_kernel, above
//     ZF_SPMV_WIDE_RESID_MIN_ROWS rows, for EITHER storage form: the shape is a function of m alone, so the dense and the
//     sparse class sum a loss of the same m in the same order.
// Cost: fp64 exp and log1p are polynomial code on the VALU (no hardware transcendental in fp64) and the division at y is
// a Newton sequence: on the order of 10^2 instructions per row where the residual kernels spend three.  One workgroup is one
// CU: 14.3 + 12.6 us at 8192 rows and 27.0 + 21.5 us at 16384 (y + x+, kernel trace) where the residual
// kernels take 6.2 + 4.7 and 11.4 + 6.6 us - 2 % of a dense 16384 x 65536 trial, but 16 us of an 88 us sparse trial at
// 8192 rows (DESIGN 9 lists a lower wide threshold for these kernels).  Beyond 32768 rows - sparse problems have
// 10^5 .. 10^7 - the rows go to up to 1024 workgroups of 256 threads: 6.5 + 5.5 us at 200 000 rows beside the residual
// kernels' 4.8 + 4.5, plus the same 4.9 us finish each.  Two rows per thread are in
// flight (unroll 2: two independent polynomial chains), their sums added in row order.
// No atomics, every sum in an order fixed by m: two solves give the same bits.  Guards and ring indices are
// zf_resid_y_kernel's / zf_resid_x_kernel's; ctl == NULL (WHICH 0) or slot < 0 (WHICH 1): a plain call outside the loop on
// ring index 0 (no momentum).
// (included by zf_solver.hip alone)
#pragma once
#include "zf_common.h"
#include "zf_spmv.h"

constexpr int ZF_LOGIT_BLOCK = 1024;   // the one-workgroup form

__device__ __forceinline__ double zf_softplus_of(double t, double e) { return fmax(t, 0.0) + log1p(e); }
__device__ __forceinline__ double zf_sigmoid_of(double t, double e) { return (t >= 0.0 ? 1.0 : e) / (1.0 + e); }

// the workgroup's sum: wave trees, then the wave sums in wave order (every thread holds it)
template <int BLOCK>
__device__ __forceinline__ double zf_logit_block_sum(double acc, double* lds) {
    acc = zf_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    double t = lds[0];
    for (int w = 1; w < BLOCK / 64; ++w) t += lds[w];
    return t;
}

// WHICH 0: at y - rho stored into r, sum of softplus; skipped unless the gradient is due.  WHICH 1: at s[(cur + slot) % 3].
// gridDim.x == 1: *f_out = scale * sum.  Otherwise part[blockIdx.x] = the chunk's sum (zf_logit_finish_kernel follows).
template <int WHICH, int BLOCK>
__global__ __launch_bounds__(BLOCK) void zf_logit_kernel(const zf_control* ctl, const double* s0, const double* s1, const double* s2,
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
        const double bi = b[i];
        const double t = -bi * z;
        const double e = exp(-fabs(t));
        if (WHICH == 0) r[i] = -bi * zf_sigmoid_of(t, e);
        acc += zf_softplus_of(t, e);
    }
    const double t = zf_logit_block_sum<BLOCK>(acc, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) *f_out = scale * t;
        else part[blockIdx.x] = t;
    }
}

// f = scale * (part[0] + part[1] + ...): thread t adds chunks t, t + 256, ... in that order, then the block sum
__global__ __launch_bounds__(ZF_BLOCK) void zf_logit_finish_kernel(const zf_control* ctl, int grad_guard, const double* __restrict__ part,
                                                                   int count, double scale, double* f_out) {
    __shared__ double lds[ZF_WAVES];
    if (ctl) {
        if (ctl->status != ZF_RUNNING) return;
        if (grad_guard && !ctl->need_grad) return;
    }
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += ZF_BLOCK) acc += part[i];
    const double t = zf_logit_block_sum<ZF_BLOCK>(acc, lds);
    if (threadIdx.x == 0) *f_out = scale * t;
}

// part: zf_spmv_resid_chunks(m) doubles of the caller (used above ZF_SPMV_WIDE_RESID_MIN_ROWS rows only; may be NULL below)
static inline bool zf_logit_wide(int64_t m) { return m > ZF_SPMV_WIDE_RESID_MIN_ROWS; }

// rho(y) -> r and f(y) -> *f_out.  ctl != NULL: inside the loop (guards, ring, momentum); NULL: rho and f at the margins s0
static inline void zf_launch_logit_y(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2,
                                     const double* b, double* r, double scale, int64_t m, int nesterov, double* part, double* f_out) {
    if (!zf_logit_wide(m)) {
        hipLaunchKernelGGL((zf_logit_kernel<0, ZF_LOGIT_BLOCK>), dim3(1), dim3(ZF_LOGIT_BLOCK), 0, st, ctl, s0, s1, s2, 0, b, r, m, nesterov,
                           scale, part, f_out);
        return;
    }
    const int chunks = zf_spmv_resid_chunks(m);   // (>= 33 here: never the one-workgroup branch of the kernel)
    hipLaunchKernelGGL((zf_logit_kernel<0, ZF_BLOCK>), dim3(chunks), dim3(ZF_BLOCK), 0, st, ctl, s0, s1, s2, 0, b, r, m, nesterov, scale,
                       part, f_out);
    hipLaunchKernelGGL(zf_logit_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ctl, 1, part, chunks, scale, f_out);
}

// f at the margins s[(cur + slot) % 3] (slot >= 0: inside the loop) or s0 (slot < 0: ctl is not read) -> *f_out
static inline void zf_launch_logit_x(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2, int slot,
                                     const double* b, double scale, int64_t m, double* part, double* f_out) {
    if (!zf_logit_wide(m)) {
        hipLaunchKernelGGL((zf_logit_kernel<1, ZF_LOGIT_BLOCK>), dim3(1), dim3(ZF_LOGIT_BLOCK), 0, st, ctl, s0, s1, s2, slot, b, nullptr, m, 0,
                           scale, part, f_out);
        return;
    }
    const int chunks = zf_spmv_resid_chunks(m);
    hipLaunchKernelGGL((zf_logit_kernel<1, ZF_BLOCK>), dim3(chunks), dim3(ZF_BLOCK), 0, st, ctl, s0, s1, s2, slot, b, nullptr, m, 0, scale,
                       part, f_out);
    hipLaunchKernelGGL(zf_logit_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, slot >= 0 ? ctl : nullptr, 0, part, chunks, scale, f_out);
}
