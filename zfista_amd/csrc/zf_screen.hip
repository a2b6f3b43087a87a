// zf_screen.hip - instantiations of the screening kernels (zf_kernels_screen.h), the launch behind a gap evaluation and the
// entry points of the C ABI for column norms, mask scans and the restriction of a matrix to its kept columns
#include <vector>

#include "zf_kernels_screen.h"

#define ZF_SCR_TRY(expr)                                                          \
    do {                                                                          \
        hipError_t _e = (expr);                                                   \
        if (_e != hipSuccess && rc == ZF_OK)                                      \
            rc = zf_fail(ZF_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e));     \
    } while (0)

// the grid of a kernel shaped like zf_spmv_rows_kernel: row workgroups, then one wave per segment
static inline dim3 zf_scr_rows_grid(const zf_spmv_mat& M, int* row_blocks_out) {
    const int rpb = ZF_BLOCK / M.lanes;
    int64_t row_blocks = (M.rows + rpb - 1) / rpb;
    if (row_blocks > ZF_SPMV_MAX_ROW_BLOCKS) row_blocks = ZF_SPMV_MAX_ROW_BLOCKS;
    const int64_t seg_blocks = (M.nseg + ZF_WAVES - 1) / ZF_WAVES;
    *row_blocks_out = (int)row_blocks;
    return dim3((unsigned)(row_blocks + seg_blocks));
}

#define ZF_SCR_BY_LANES(M, KERNEL, grid, st, ...)                                                                   \
    switch ((M).lanes) {                                                                                            \
        case 4: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(ZF_BLOCK), 0, st, __VA_ARGS__); break;                     \
        case 8: hipLaunchKernelGGL(KERNEL<8>, grid, dim3(ZF_BLOCK), 0, st, __VA_ARGS__); break;                     \
        case 16: hipLaunchKernelGGL(KERNEL<16>, grid, dim3(ZF_BLOCK), 0, st, __VA_ARGS__); break;                   \
        case 32: hipLaunchKernelGGL(KERNEL<32>, grid, dim3(ZF_BLOCK), 0, st, __VA_ARGS__); break;                   \
        default: hipLaunchKernelGGL(KERNEL<64>, grid, dim3(ZF_BLOCK), 0, st, __VA_ARGS__); break;                   \
    }

// ---- the screen behind a gap evaluation ----------------------------------------------------------------------------------
// keep (n) -> index (its exclusive scan), cnt[chunks] = the kept count (also to *total_out): three launches
static void zf_launch_mask_scan(hipStream_t st, bool screen, const double* g, const double* norms, const double* gap8, const double* sscal,
                                int64_t n, double lam, uint8_t* keep, int32_t* index, int32_t* cnt, double* total_out) {
    const int nc = zf_scr_chunks(n);
    if (screen) hipLaunchKernelGGL(zf_scr_mask_kernel<true>, dim3(nc), dim3(ZF_BLOCK), 0, st, g, norms, gap8, sscal, n, lam, keep, cnt);
    else hipLaunchKernelGGL(zf_scr_mask_kernel<false>, dim3(nc), dim3(ZF_BLOCK), 0, st, g, norms, gap8, sscal, n, lam, keep, cnt);
    hipLaunchKernelGGL(zf_scr_offsets_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, cnt, nc, total_out);
    hipLaunchKernelGGL(zf_scr_scan_kernel, dim3(nc), dim3(ZF_BLOCK), 0, st, keep, n, cnt, index);
}

void zf_launch_screen(hipStream_t st, const zf_screen_req& rq, const double* g, const double* gap8, const double* asum, const double* rr,
                      int64_t m, int64_t n, double scale, double lam, bool logistic) {
    hipLaunchKernelGGL(zf_scr_radius_kernel, dim3(1), dim3(64), 0, st, gap8, asum, rr, rq.stats, m, rq.max_row, rq.max_col, scale, lam,
                       logistic ? 1 : 0, rq.scal);
    zf_launch_mask_scan(st, true, g, rq.norms, gap8, rq.scal, n, lam, rq.keep, rq.index, rq.cnt, rq.scal + 3);
}

// ---- column norms --------------------------------------------------------------------------------------------------------
// stats = [sum norms^2, max norm]
static int zf_norm_stats(const double* norms_dev, int64_t n, double* stats_dev) {
    int rc = ZF_OK;
    const int nc = zf_scr_chunks(n);
    double* part = nullptr;
    if (nc > 1) ZF_SCR_TRY(hipMalloc(&part, sizeof(double) * 2 * ZF_SCREEN_MAX_CHUNKS));
    if (rc == ZF_OK) {
        hipLaunchKernelGGL(zf_scr_stats_kernel<false>, dim3(nc), dim3(ZF_BLOCK), 0, nullptr, norms_dev, n, part, stats_dev);
        if (nc > 1) hipLaunchKernelGGL(zf_scr_stats_kernel<true>, dim3(1), dim3(ZF_BLOCK), 0, nullptr, part, (int64_t)nc, part, stats_dev);
        ZF_SCR_TRY(hipGetLastError());
        ZF_SCR_TRY(hipStreamSynchronize(nullptr));
    }
    if (part) (void)hipFree(part);
    return rc;
}

extern "C" int zf_spmat_col_norms(const zf_spmat* h, double* norms_dev, double* stats_dev) {
    ZF_REQUIRE(h && norms_dev && stats_dev, "zf_spmat_col_norms: null argument");
    int rc = ZF_OK;
    const zf_spmv_mat& M = h->At;
    double* partial = nullptr;
    if (M.nseg > 0) ZF_SCR_TRY(hipMalloc(&partial, sizeof(double) * M.nseg));
    if (rc == ZF_OK) {
        int rb = 0;
        const dim3 grid = zf_scr_rows_grid(M, &rb);
        ZF_SCR_BY_LANES(M, zf_scr_norms_rows_kernel, grid, nullptr, M, rb, norms_dev, partial);
        if (M.nsplit > 0)
            hipLaunchKernelGGL(zf_scr_norms_tail_kernel, dim3(zf_grid_for(M.nsplit)), dim3(ZF_BLOCK), 0, nullptr, M, norms_dev, partial);
        ZF_SCR_TRY(hipGetLastError());
        if (rc == ZF_OK) rc = zf_norm_stats(norms_dev, h->n, stats_dev);
    }
    if (partial) (void)hipFree(partial);
    return rc;
}

extern "C" int zf_dense_col_norms(const double* A_dev, int64_t m_rows, int64_t n, double* norms_dev, double* stats_dev) {
    ZF_REQUIRE(A_dev && norms_dev && stats_dev, "zf_dense_col_norms: null argument");
    ZF_REQUIRE(m_rows >= 1 && n >= 1, "zf_dense_col_norms: m and n must be >= 1");
    hipLaunchKernelGGL(zf_scr_norms_dense_kernel, dim3(zf_grid_for(n)), dim3(ZF_BLOCK), 0, nullptr, A_dev, m_rows, n, norms_dev);
    ZF_HIP(hipGetLastError());
    return zf_norm_stats(norms_dev, n, stats_dev);
}

// ---- the scan of a caller's mask -------------------------------------------------------------------------------------------
static int zf_mask_scan_sync(const uint8_t* keep_dev, int64_t n, int32_t* index_dev, int64_t* count_out) {
    int rc = ZF_OK;
    int32_t* cnt = nullptr;
    const int nc = zf_scr_chunks(n);
    ZF_SCR_TRY(hipMalloc(&cnt, sizeof(int32_t) * (ZF_SCREEN_MAX_CHUNKS + 1)));
    if (rc == ZF_OK) {
        int32_t total = 0;
        zf_launch_mask_scan(nullptr, false, nullptr, nullptr, nullptr, nullptr, n, 0.0, const_cast<uint8_t*>(keep_dev), index_dev, cnt, nullptr);
        ZF_SCR_TRY(hipGetLastError());
        ZF_SCR_TRY(hipMemcpy(&total, cnt + nc, sizeof(int32_t), hipMemcpyDeviceToHost));
        *count_out = total;
    }
    if (cnt) (void)hipFree(cnt);
    return rc;
}

extern "C" int zf_screen_scan(const uint8_t* keep_dev, int64_t n, int32_t* index_dev, int64_t* count_out) {
    ZF_REQUIRE(keep_dev && index_dev && count_out, "zf_screen_scan: null argument");
    ZF_REQUIRE(n >= 1 && n <= 0x7fffffffLL, "zf_screen_scan: n must be in [1, 2^31)");
    return zf_mask_scan_sync(keep_dev, n, index_dev, count_out);
}

// ---- restriction -------------------------------------------------------------------------------------------------------------
extern "C" int zf_spmat_restrict_count(const zf_spmat* h, const uint8_t* keep_dev, int32_t* index_dev, int64_t* len_dev, int64_t* t_len_dev,
                                       int32_t* seg_off_dev, int64_t* count_out) {
    ZF_REQUIRE(h && keep_dev && index_dev && len_dev && t_len_dev && count_out, "zf_spmat_restrict_count: null argument");
    ZF_REQUIRE(h->A.nseg == 0 || seg_off_dev, "zf_spmat_restrict_count: seg_off is required when A has split rows");
    int rc = zf_mask_scan_sync(keep_dev, h->n, index_dev, count_out);
    if (rc) return rc;
    int rb = 0;
    const dim3 grid = zf_scr_rows_grid(h->A, &rb);
    ZF_SCR_BY_LANES(h->A, zf_scr_rcount_kernel, grid, nullptr, h->A, rb, keep_dev, len_dev, seg_off_dev);
    if (h->A.nsplit > 0)
        hipLaunchKernelGGL(zf_scr_rcount_tail_kernel, dim3(zf_grid_for(h->A.nsplit)), dim3(ZF_BLOCK), 0, nullptr, h->A, len_dev, seg_off_dev);
    hipLaunchKernelGGL(zf_scr_tlen_kernel, dim3(zf_grid_for(h->n)), dim3(ZF_BLOCK), 0, nullptr, h->At.indptr, h->n, keep_dev, index_dev, t_len_dev);
    ZF_HIP(hipGetLastError());
    ZF_HIP(hipStreamSynchronize(nullptr));
    return ZF_OK;
}

extern "C" int zf_spmat_restrict_fill(const zf_spmat* h, const uint8_t* keep_dev, const int32_t* index_dev, const int32_t* seg_off_dev,
                                      int64_t k, int64_t nnz_new, const int64_t* indptr_dev, int32_t* indices_dev, double* values_dev,
                                      const int64_t* t_indptr_dev, int32_t* t_indices_dev, double* t_values_dev) {
    ZF_REQUIRE(h && keep_dev && index_dev && indptr_dev && t_indptr_dev, "zf_spmat_restrict_fill: null argument");
    ZF_REQUIRE(h->A.nseg == 0 || seg_off_dev, "zf_spmat_restrict_fill: seg_off is required when A has split rows");
    ZF_REQUIRE(k >= 1 && k <= h->n && nnz_new >= 0 && nnz_new <= h->nnz, "zf_spmat_restrict_fill: k must be in [1, n] and nnz_new in [0, nnz]");
    ZF_REQUIRE(nnz_new == 0 || (indices_dev && values_dev && t_indices_dev && t_values_dev),
               "zf_spmat_restrict_fill: indices and values are required when nnz_new > 0");
    // the row pointers the kernels write by must end where the caller's arrays end
    int64_t last = -1, t_last = -1;
    ZF_HIP(hipMemcpy(&last, indptr_dev + h->m, sizeof(int64_t), hipMemcpyDeviceToHost));
    ZF_HIP(hipMemcpy(&t_last, t_indptr_dev + k, sizeof(int64_t), hipMemcpyDeviceToHost));
    ZF_REQUIRE(last == nnz_new && t_last == nnz_new, "zf_spmat_restrict_fill: both row pointer arrays must end at nnz_new");
    if (nnz_new == 0) return ZF_OK;
    int rb = 0;
    dim3 grid = zf_scr_rows_grid(h->A, &rb);
    ZF_SCR_BY_LANES(h->A, zf_scr_fill_A_kernel, grid, nullptr, h->A, rb, keep_dev, index_dev, indptr_dev, seg_off_dev, indices_dev, values_dev);
    grid = zf_scr_rows_grid(h->At, &rb);
    ZF_SCR_BY_LANES(h->At, zf_scr_fill_At_kernel, grid, nullptr, h->At, rb, keep_dev, index_dev, t_indptr_dev, t_indices_dev, t_values_dev);
    ZF_HIP(hipGetLastError());
    ZF_HIP(hipStreamSynchronize(nullptr));
    return ZF_OK;
}

extern "C" int zf_dense_restrict(const double* A_dev, int64_t m_rows, int64_t n, const uint8_t* keep_dev, int32_t* index_dev, int64_t k,
                                 double* out_dev) {
    ZF_REQUIRE(A_dev && keep_dev && index_dev && out_dev, "zf_dense_restrict: null argument");
    ZF_REQUIRE(m_rows >= 1 && n >= 1 && n <= 0x7fffffffLL, "zf_dense_restrict: m must be >= 1 and n in [1, 2^31)");
    int64_t count = 0;
    int rc = zf_mask_scan_sync(keep_dev, n, index_dev, &count);
    if (rc) return rc;
    ZF_REQUIRE(count == k && k >= 1, "zf_dense_restrict: k must be the number of kept columns, at least 1");
    const dim3 grid((unsigned)((n + ZF_BLOCK - 1) / ZF_BLOCK), (unsigned)(m_rows < 1024 ? m_rows : 1024));
    hipLaunchKernelGGL(zf_scr_gather_dense_kernel, grid, dim3(ZF_BLOCK), 0, nullptr, A_dev, m_rows, n, keep_dev, index_dev, k, out_dev);
    ZF_HIP(hipGetLastError());
    ZF_HIP(hipStreamSynchronize(nullptr));
    return ZF_OK;
}
