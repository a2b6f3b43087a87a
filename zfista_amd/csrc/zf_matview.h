// zf_matview.h - the design matrix of a margins problem as its two sweeps see it, and the two sweeps (gfx950 only; host code, no
// kernel in here).
//
// Every margins problem class rests on z = A x (rows) and g = factor * A^T r (columns), over five storage forms of A: dense fp64
// on the VALU or on MFMA (zf_kernels_gemv.h), dense fp32 (zf_kernels_gemv_f32.h), dense with K responses (zf_kernels_mr.h), CSR
// with one response or K (zf_spmv.h).  Which form runs is chosen HERE and nowhere else: the solver's loop (ctl given, a ring
// slot) and the evaluations outside it (ctl NULL, slot -1) call the same two launchers, so the same matrix takes the same
// kernel, grid and summation order in both - what "resume equals the uninterrupted solve" and "the live gap equals the
// standalone gap" rest on.
#pragma once
#include "zf_kernels_gemv.h"
#include "zf_kernels_gemv_f32.h"
#include "zf_kernels_mr.h"
#include "zf_spmv.h"

struct zf_matview {
    const double* A;     // dense: m x n row-major (device), 16-byte aligned; NULL for CSR
    int64_t m, n;        // (CSR: the handle's)
    const zf_spmat* h;   // CSR: A and A^T with their plans; NULL for dense
    bool csr;
    const float* A32;    // dense, stored in fp32 (zf_kernels_gemv_f32.h): m x n row-major (device), 16-byte aligned - A is NULL then; NULL otherwise
    int k = 1;           // responses (zf_kernels_mr.h for dense fp64, zf_kernels_spmm.h for CSR): m and n stay the matrix's, the vectors hold m k and n k doubles
    bool mfma = false;   // dense fp64, k = 1, n % 32 == 0: the column sweep runs on v_mfma_f64_16x16x4 - fixed when the view is built (the two sum in different orders)
};
static inline int64_t zf_view_rows(const zf_matview& V) { return V.m * V.k; }   // length of a margins vector
static inline int64_t zf_view_cols(const zf_matview& V) { return V.n * V.k; }   // length of a decision vector

// what the sweeps write between their launches: the slab of the dense column sweep and its slices, or the segment sums of the
// split rows of A / A^T (a call's own, or a solver's: the handle is shared with live solvers on other streams)
struct zf_sweep_ws {
    double* slab;        // slices * zf_view_cols doubles
    int slices;
    int64_t rows_per_slice;
    double *part_A, *part_At;
};

// row slices of a dense column sweep whose threads own V columns: enough that panels x slices fills the chip (>= ~2048
// workgroups), at most 64, at least 8 rows each
static inline void zf_col_slices(int64_t m, int64_t n, int V, int* slices_out, int64_t* rows_per_slice) {
    const int64_t panels = (n / V + ZF_BLOCK - 1) / ZF_BLOCK;
    int64_t slices = (ZF_MAX_GRID + panels - 1) / panels;
    if (slices > (m + 7) / 8) slices = (m + 7) / 8;
    if (slices < 1) slices = 1;
    if (slices > 64) slices = 64;
    *rows_per_slice = (m + slices - 1) / slices;
    *slices_out = (int)((m + *rows_per_slice - 1) / *rows_per_slice);
}
// ... of a dense view: fp64 threads own 2 columns or 1 by the parity of n, fp32 threads up to 4 (so a given n has up to half the
// panels and takes up to twice the slices); K responses: the fp64 rule on the matrix's own m and n (the panels are A's columns)
static inline void zf_view_slices(const zf_matview& V, int* slices_out, int64_t* rows_per_slice) {
    zf_col_slices(V.m, V.n, V.A32 ? zf_f32_width(V.n) : (V.n % 2 == 0) ? 2 : 1, slices_out, rows_per_slice);
}

// sr = A xr.  Inside the loop: ctl given, the ring index is (ctl->cur + slot) % 3; outside: ctl NULL, slot -1, index 0 (the
// callers pass three equal pointers).
static inline void zf_launch_apply(const zf_matview& V, hipStream_t st, const zf_control* ctl, zf_ring3 xr, zf_ring3 sr, int slot,
                                   const zf_sweep_ws& W) {
    if (V.csr) {
        const zf_spmv_io io = {{xr.p[0], xr.p[1], xr.p[2]}, {sr.p[0], sr.p[1], sr.p[2]}};
        if (V.k > 1) zf_launch_spmm(V.h->A, st, ctl, false, io, slot, 1.0, V.k, W.part_A);
        else zf_launch_spmv(V.h->A, st, ctl, false, io, slot, 1.0, W.part_A);
    } else if (V.A32) {
        zf_launch_rows_f32(st, ctl, V.A32, xr, sr, slot, V.m, V.n);
    } else if (V.k > 1) {
        zf_launch_mr_rows(st, ctl, V.A, xr, sr, slot, V.m, V.n, V.k);
    } else {
        int gr = (int)((V.m + GEMV_ROWS - 1) / GEMV_ROWS);
        if (gr > 8 * ZF_MAX_GRID) gr = 8 * ZF_MAX_GRID;
        if (V.n % 2 == 0) hipLaunchKernelGGL(zf_gemv_rows_kernel<2>, dim3(gr), dim3(ZF_BLOCK), 0, st, ctl, V.A, xr, sr, slot, V.m, V.n);
        else hipLaunchKernelGGL(zf_gemv_rows_kernel<1>, dim3(gr), dim3(ZF_BLOCK), 0, st, ctl, V.A, xr, sr, slot, V.m, V.n);
    }
}

// g = factor * A^T r.  CSR: the row sums of the stored A^T, guarded as a gradient inside the loop (ctl given).  Dense: the
// column sweep over W's slices, then the slice combine over zf_view_cols entries.  combine_guarded false (row-sharded least
// squares: g is this rank's part, the rest of the trial follows the exchange): the combine runs with ctl NULL, the partial
// sweep keeps ctl.
static inline void zf_launch_adjoint(const zf_matview& V, hipStream_t st, const zf_control* ctl, const double* r, double* g, double factor,
                                     const zf_sweep_ws& W, bool combine_guarded = true) {
    if (V.csr) {
        const zf_spmv_io io = {{r, r, r}, {g, g, g}};
        if (V.k > 1) zf_launch_spmm(V.h->At, st, ctl, ctl != nullptr, io, -1, factor, V.k, W.part_At);
        else zf_launch_spmv(V.h->At, st, ctl, ctl != nullptr, io, -1, factor, W.part_At);
        return;
    }
    const int64_t m = V.m, n = V.n;
    if (V.A32) {   // (no MFMA form: that sweep reads fp64 A)
        zf_launch_cols_f32(st, ctl, V.A32, r, W.slab, m, n, W.slices, W.rows_per_slice);
    } else if (V.k > 1) {   // (nor here)
        zf_launch_mr_cols(st, ctl, V.A, r, W.slab, m, n, V.k, W.slices, W.rows_per_slice);
    } else if (V.mfma) {
        const dim3 gM((unsigned)((n + GEMVT_MFMA_COLS - 1) / GEMVT_MFMA_COLS), (unsigned)W.slices);
        hipLaunchKernelGGL(zf_gemvT_partial_mfma_kernel, gM, dim3(ZF_BLOCK), 0, st, ctl, V.A, r, W.slab, m, n, W.rows_per_slice);
    } else {
        const int vw = (n % 2 == 0) ? 2 : 1;
        const dim3 gT((unsigned)((n / vw + ZF_BLOCK - 1) / ZF_BLOCK), (unsigned)W.slices);
        if (vw == 2) hipLaunchKernelGGL(zf_gemvT_partial_kernel<2>, gT, dim3(ZF_BLOCK), 0, st, ctl, V.A, r, W.slab, m, n, W.rows_per_slice);
        else hipLaunchKernelGGL(zf_gemvT_partial_kernel<1>, gT, dim3(ZF_BLOCK), 0, st, ctl, V.A, r, W.slab, m, n, W.rows_per_slice);
    }
    const int64_t nk = zf_view_cols(V);
    hipLaunchKernelGGL(zf_gemvT_combine_kernel, dim3(zf_grid_for(nk)), dim3(ZF_BLOCK), 0, st, combine_guarded ? ctl : nullptr, W.slab, g,
                       factor, nk, W.slices);
}
