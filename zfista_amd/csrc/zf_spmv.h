// zf_spmv.h - what the solver needs of the sparse kind: the device view of a CSR matrix and its plan, the matrix handle,
// and the launches of zf_spmv.hip.  The kernels themselves are in zf_kernels_spmv.h (included by zf_spmv.hip only).
#pragma once
#include "zf_common.h"

constexpr int ZF_SPMV_MIN_LANES = 4;
constexpr int ZF_SPMV_MAX_LANES = 64;
// row groups beyond that many workgroups are walked with the grid's stride (fewer, longer-lived workgroups measured
// slower at 2e5 rows of ~40: 2048 workgroups 4 870 it/s, 8192 4 960, one per 8 rows 5 090)
constexpr int64_t ZF_SPMV_MAX_ROW_BLOCKS = int64_t(1) << 20;

// one CSR matrix and its plan, as the kernels take it (device pointers)
struct zf_spmv_mat {
    const int64_t* indptr;      // rows + 1
    const int32_t* indices;     // nnz (NULL when nnz == 0)
    const double* values;       // nnz
    int64_t rows, cols, nnz;
    int lanes;                  // L
    int64_t threshold;          // rows longer than this are split
    int64_t nsplit, nseg;       // split rows / their segments
    const int64_t* split_row;   // nsplit: the row
    const int64_t* split_first; // nsplit + 1: its first segment
    const int64_t* seg_start;   // nseg: first element of the segment (it ends `threshold` on, or with its row)
    const int64_t* seg_row;     // nseg
};

// the matrix handle of the C ABI (zf_spmat_create): A, A^T and the device copies of their plans.  Immutable once created:
// solvers and evaluations that share a handle - on any streams, at the same time - write nothing through it (the segment
// sums of split rows go to an array of the CALLER of zf_launch_spmv: one per solver and matrix, one per evaluation)
struct zf_spmat {
    zf_spmv_mat A, At;
    int64_t m, n, nnz;
    void* owned[8];
    int n_owned;
};

// the three vectors of a ring (zf_solver: x / A x slots); slot -1 uses index 0 (a plain call outside the loop)
struct zf_spmv_io {
    const double* in[3];
    double* out[3];
};

// out = out_scale * M in (one launch; two when M has split rows), stream-ordered.  partial: M.nseg doubles of the caller
// (the segment sums of this sweep; NULL when M has no split row) - never shared between sweeps that may run at once.
void zf_launch_spmv(const zf_spmv_mat& M, hipStream_t st, const zf_control* ctl, bool grad_guard, const zf_spmv_io& io, int slot,
                    double out_scale, double* partial);

// The same sweep against K response-interleaved columns (zf_kernels_spmm.h, zf_spmm.hip): in holds M.cols K doubles, out M.rows K,
// out[i K + k] = out_scale * sum_e values[e] * in[indices[e] K + k].  Response k is summed exactly as zf_launch_spmv sums a vector:
// column k of out is bit-equal to that sweep on column k of in.  2 <= K <= ZF_SPMM_MAX_K (the caller checks); the same plan, the
// same grid and launch count; partial: M.nseg K doubles of the caller (NULL when M has no split row).
constexpr int ZF_SPMM_MAX_K = 16;
void zf_launch_spmm(const zf_spmv_mat& M, hipStream_t st, const zf_control* ctl, bool grad_guard, const zf_spmv_io& io, int slot,
                    double out_scale, int K, double* partial);

// ---- residuals of LONG vectors --------------------------------------------------------------------------------------
// r = A y - b by linearity with f(y), and f(x+) from s+ = A x+, as zf_resid_y_kernel / zf_resid_x_kernel compute them - but
// those walk the m rows with ONE workgroup (dense matrices have at most a few 10^4 rows), and a sparse problem has 10^5 ..
// 10^7: at m = 2e5 the two took 112 + 60 us of a 367 us trial.  Here zf_spmv_resid_chunks(m) workgroups take a contiguous
// chunk each -> part[chunk]; a second launch adds the chunk sums in chunk order and finishes f = scale * sqrt(sum)^2.
// Chunk count and chunk length are functions of m alone.  Used when m > ZF_SPMV_WIDE_RESID_MIN_ROWS.
constexpr int64_t ZF_SPMV_WIDE_RESID_MIN_ROWS = int64_t(1) << 15;
constexpr int ZF_SPMV_RESID_MAX_CHUNKS = 1024;
int zf_spmv_resid_chunks(int64_t m);
// (ctl never NULL: these run inside the loop only; the guards and ring indices are zf_resid_y_kernel's / zf_resid_x_kernel's)
void zf_launch_spmv_resid_y(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2, const double* b,
                            double* r, double scale, int64_t m, int nesterov, double* part, double* f_out);
void zf_launch_spmv_resid_x(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2, int slot,
                            const double* b, double scale, int64_t m, double* part, double* f_out);
// ZF_ACCEPT_REMAINDER: f(x+) exactly as zf_launch_spmv_resid_x leaves it, and beside it R = scale sum (s+ - s_y)^2 with
// s_y = s_k + beta (s_k - s_{k-1}) (zf_resid_x_rem_kernel, zf_kernels_gemv.h), chunk by chunk in the same order; still two
// launches.  part, part_r: zf_spmv_resid_chunks(m) doubles each.  slot < 0: a plain call outside the loop (ctl unused) on
// s+ = s0, s_k = s1, s_{k-1} = s2 with beta = beta_plain.
void zf_launch_spmv_resid_x_rem(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2, int slot,
                                const double* b, double scale, int64_t m, int nesterov, double beta_plain, double* part, double* part_r,
                                double* f_out, double* r_out);
