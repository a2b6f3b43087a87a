// zf_kernels_softmax.h - the multinomial (softmax) loss on the K-response margins (gfx950, fp64): the one loss whose row couples
// K margins, which zf_loss_row (one margin) cannot express.
//   f(X) = scale sum_i w_i [logsumexp(z_i) - <y_i, z_i>],  z_i = (A X)_i in R^K,  grad f = scale A^T (w o (softmax(Z) - Y))
// The margins, Y and psi are the K-response vectors of zf_kernels_mr.h / zf_kernels_spmm.h: s[i K + k], m K doubles, `m` below is
// that flattened count and a ROW of this loss is K consecutive entries.  One row, the same arithmetic in every kernel here and in
// the NumPy restatement of the tests (tests/multinomial_cases.py):
//   mx = max_k z_k (k order)    d_k = z_k - mx <= 0    e_k = exp(d_k)    S = sum_k e_k (k order), in [1, K]
//   rS = 1 / S (ONE division per row)    p_k = e_k rS    psi_k = p_k - y_k    phi = log S + sum_k y_k (-d_k)   (k order)
// every term of phi >= 0; K exps, one log and one division per row; nothing overflows for finite margins.  The maximum is
// v_max_f64, which drops a NaN operand - but d_k = NaN - mx is NaN, and so are S, phi and f; a +inf margin gives d = inf - inf = NaN.
// A -inf margin: y_k * inf - NaN where y_k = 0, +inf where y_k > 0 (f = +inf: the acceptance test rejects the trial).
// phi = logsumexp - <y, z> because sum_k y_k = 1 (the caller's check).
// Row weights: the library holds one weight per flattened entry (zf_solver_set_row_weights: m doubles) and a row of this loss has
// one weight, read at w[i K]; it multiplies the K entries of psi and phi once each, and w_i == 0 is a row that is not there
// (zf_wterm: +0 outputs whatever y_i holds).
//
// Lanes: ONE LANE PER ROW.  Lane t of a workgroup takes rows lo + t, lo + t + BLOCK, ...: a wave's 64 rows are 64 K 8 contiguous
// bytes, so every line a wave touches is consumed whole by that wave's K loads (the k-th load of the unrolled loop re-reads the
// lines the first one fetched from the vector L1), and the K margins of a row sit in one lane's registers - max, sum and phi need
// no cross-lane step.  Even K: a row starts on a 16-byte boundary (the buffers are 16-byte aligned: hipMalloc's, and b is checked),
// so a row is read and psi stored as K / 2 16-byte accesses; odd K: 8-byte accesses, rows at odd i are not 16-byte aligned.  A few
// lanes per row would make each access contiguous across lanes, but leaves K not dividing 64 with idle lanes and puts shuffles into
// max and sum.  The simple map stays on the SUPPOSITION that the rows pass (m K entries) is small beside the two sweeps of a trial
// (nnz K or m n K multiply-adds) and that the later loads of a row hit the vector L1; neither is measured yet.
// Shapes, sums and guards are zf_loss_rows_kernel's: one workgroup of 1024 threads up to ZF_SPMV_WIDE_RESID_MIN_ROWS flattened
// entries, else zf_spmv_resid_chunks(m) workgroups of 256 on a contiguous chunk of WHOLE rows each -> part[chunk] and
// zf_rows_finish_kernel.  A lane adds its rows in row order, then the block sum: an order fixed by (m, K) alone.  No atomics, no
// scratch, no LDS beyond the block sum; every device write is a plain vector store.
// (included by zf_solver.hip alone, after zf_kernels_gap.h)
#pragma once
#include "zf_kernels_gap.h"
#include "zf_kernels_mr.h"

// the K doubles of row i of v (even K: 16-byte loads)
template <int K>
__device__ __forceinline__ void zf_softmax_load(const double* __restrict__ v, int64_t i, double (&out)[K]) {
    if (K % 2 == 0) {
        const double2* __restrict__ p = reinterpret_cast<const double2*>(v + i * K);
#pragma unroll
        for (int k = 0; k < K / 2; ++k) {
            const double2 t = p[k];
            out[2 * k] = t.x;
            out[2 * k + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = v[i * K + k];
    }
}

template <int K>
__device__ __forceinline__ void zf_softmax_store(double* __restrict__ v, int64_t i, const double (&in)[K]) {
    if (K % 2 == 0) {
        double2* __restrict__ p = reinterpret_cast<double2*>(v + i * K);
#pragma unroll
        for (int k = 0; k < K / 2; ++k) p[k] = make_double2(in[2 * k], in[2 * k + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) v[i * K + k] = in[k];
    }
}

// z (in) -> d = z - mx (in place), e = exp(d); returns S
template <int K>
__device__ __forceinline__ double zf_softmax_row(double (&z)[K], double (&e)[K]) {
    double mx = z[0];
#pragma unroll
    for (int k = 1; k < K; ++k) mx = fmax(mx, z[k]);
    double S = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        z[k] = z[k] - mx;
        e[k] = exp(z[k]);
        S += e[k];
    }
    return S;
}

// the rows [lo, hi) of workgroup blockIdx.x out of `rows`: whole rows, a function of (rows, gridDim.x) alone
__device__ __forceinline__ void zf_softmax_chunk_of(int64_t rows, int64_t& lo, int64_t& hi) {
    const int64_t per = (rows + gridDim.x - 1) / gridDim.x;
    lo = (int64_t)blockIdx.x * per;
    if (lo > rows) lo = rows;
    hi = lo + per < rows ? lo + per : rows;
}

// WHICH 0: at y - w o psi stored into r, sum of w phi; skipped unless the gradient is due.  WHICH 1: at s[(cur + slot) % 3].
// gridDim.x == 1: *f_out = scale * sum.  Otherwise part[blockIdx.x] = the chunk's sum (zf_rows_finish_kernel follows).
// m: the flattened count (rows K).  !W: w is not read (NULL).
template <int K, bool W, int WHICH, int BLOCK>
__global__ __launch_bounds__(BLOCK) void zf_softmax_rows_kernel(const zf_control* ctl, const double* s0, const double* s1, const double* s2,
                                                                int slot, const double* __restrict__ b, const double* __restrict__ w,
                                                                double* __restrict__ r, int64_t m, int nesterov, double scale,
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
    int64_t lo, hi;
    zf_softmax_chunk_of(m / K, lo, hi);
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
        double z[K], e[K], y[K];
        zf_softmax_load<K>(sk, i, z);
        if (WHICH == 0 && nesterov) {
            zf_softmax_load<K>(so, i, e);
#pragma unroll
            for (int k = 0; k < K; ++k) z[k] = z[k] + beta * (z[k] - e[k]);
        }
        zf_softmax_load<K>(b, i, y);
        const double wi = W ? w[i * K] : 1.0;
        const bool on = wi != 0.0;
        const double S = zf_softmax_row<K>(z, e);
        double phi = log(S);
#pragma unroll
        for (int k = 0; k < K; ++k) phi += y[k] * (-z[k]);
        if (WHICH == 0) {
            const double rS = 1.0 / S;
#pragma unroll
            for (int k = 0; k < K; ++k) e[k] = zf_wterm<W>(on, wi, e[k] * rS - y[k]);
            zf_softmax_store<K>(r, i, e);
        }
        acc += zf_wterm<W>(on, wi, phi);
    }
    const double t = zf_rows_block_sum<BLOCK>(acc, lds);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) *f_out = scale * t;
        else part[blockIdx.x] = t;
    }
}

// ---- the certificate rows ---------------------------------------------------------------------------------------------------
// The conjugate of logsumexp(z) - <y, z> at theta is sum_k v_k log v_k, v = theta + y on the simplex; theta = alpha psi gives
// v = alpha p + (1 - alpha) y: a convex combination, feasible for every alpha in [0, 1].
//   ZF_GS_ENT  sum_i w_i sum_k v_ik log v_ik  (0 log 0 = 0)                  D = -scale [ENT]
//   ZF_GS_KL   sum_i w_i KL(v_i || p_i) = sum_k v_k (log v_k - log p_k)      rows = scale [KL]
// log p_k = d_k - log S, never a quotient of underflowed numbers: finite for every finite margin, also where p_k has underflowed
// to 0 and y_k > 0.  The row term is clamped at 0 and not formed when 1 - alpha (read from scal, never from a rounded alpha) is
// exactly 0: alpha = 1 gives a rows gap of exactly 0 (a NaN alpha takes the branch).  Slots, shapes and chunk rows of
// zf_gap_kl_kernel: the compositions' logistic arm serves this loss.
template <int K, bool W, int BLOCK>
__global__ __launch_bounds__(BLOCK) void zf_gap_softmax_kernel(const double* __restrict__ zv, const double* __restrict__ b,
                                                               const double* __restrict__ w, int64_t m, double* __restrict__ part,
                                                               double* __restrict__ scal) {
    __shared__ double lds[2 * BLOCK / 64];
    const double alpha = scal[ZF_GS_ALPHA], oma = scal[ZF_GS_OMA];
    int64_t lo, hi;
    zf_softmax_chunk_of(m / K, lo, hi);
    double kl = 0.0, ent = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
        double z[K], e[K];
        zf_softmax_load<K>(zv, i, z);
        const double wi = W ? w[i * K] : 1.0;
        const bool on = wi != 0.0;
        const double S = zf_softmax_row<K>(z, e);
        const double rS = 1.0 / S, lS = log(S);
        double kr = 0.0, er = 0.0;
        // y is streamed, a pair (even K: 16 bytes) or an entry at a time: d, e and y of a row are never all in registers
        // (3 K doubles: 96 VGPRs at K = 16 would spill in the 1024-thread shape)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double yk;
            if (K % 2 == 0) {
                const double2 t = reinterpret_cast<const double2*>(b + i * K)[k / 2];
                yk = k % 2 ? t.y : t.x;
            } else {
                yk = b[i * K + k];
            }
            const double v = alpha * (e[k] * rS) + oma * yk;
            const double lv = log(v);
            er += v == 0.0 ? 0.0 : v * lv;
            if (oma != 0.0) kr += v == 0.0 ? 0.0 : v * (lv - (z[k] - lS));
        }
        if (kr < 0.0) kr = 0.0;   // (>= 0 but for rounding; a NaN stays: the comparison is false)
        kl += zf_wterm<W>(on, wi, kr);
        ent += zf_wterm<W>(on, wi, er);
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

// ---- launchers ------------------------------------------------------------------------------------------------------------------
template <int K, bool W, int WHICH>
static inline void zf_launch_softmax_rows_k(hipStream_t st, const zf_rows_call& c) {
    const int chunks = zf_launch_rows_shapes(st, zf_softmax_rows_kernel<K, W, WHICH, ZF_ROWS_BLOCK>, zf_softmax_rows_kernel<K, W, WHICH, ZF_BLOCK>,
                                             c.m, c.ctl, c.s0, c.s1, c.s2, c.slot, c.b, c.w, c.r, c.m, c.nesterov, c.scale, c.part, c.f_out);
    if (chunks)
        hipLaunchKernelGGL(zf_rows_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, c.fin_ctl, WHICH == 0 ? 1 : 0, c.part, chunks, c.scale,
                           c.f_out);
}

// the trial-side rows pass for the response count of the call (2 .. 16: the setter and the entry points admit no other)
template <int WHICH>
static inline void zf_launch_softmax_rows(hipStream_t st, const zf_rows_call& c) {
    switch (c.K) {
#define ZF_SM_CASE(k)                                                   \
    case k:                                                             \
        if (c.w) zf_launch_softmax_rows_k<k, true, WHICH>(st, c);       \
        else zf_launch_softmax_rows_k<k, false, WHICH>(st, c);          \
        break;
        ZF_MR_EACH_K(ZF_SM_CASE)
#undef ZF_SM_CASE
        default: break;
    }
}

template <int K>
static inline int zf_launch_gap_softmax_k(hipStream_t st, const double* z, const double* b, const double* w, int64_t m, const zf_gap_ws& ws) {
    return zf_launch_rows_shapes(st, w ? zf_gap_softmax_kernel<K, true, ZF_ROWS_BLOCK> : zf_gap_softmax_kernel<K, false, ZF_ROWS_BLOCK>,
                                 w ? zf_gap_softmax_kernel<K, true, ZF_BLOCK> : zf_gap_softmax_kernel<K, false, ZF_BLOCK>, m, z, b, w, m, ws.part,
                                 ws.scal);
}

// step 5 of a gap evaluation; returns the chunks whose two rows of sums the caller's finish has to add (0: written)
static inline int zf_launch_gap_softmax(hipStream_t st, int K, const double* z, const double* b, const double* w, int64_t m,
                                        const zf_gap_ws& ws) {
    switch (K) {
#define ZF_SM_CASE(k) case k: return zf_launch_gap_softmax_k<k>(st, z, b, w, m, ws);
        ZF_MR_EACH_K(ZF_SM_CASE)
#undef ZF_SM_CASE
        default: return 0;
    }
}
