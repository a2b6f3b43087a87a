// zf_spmm.hip - instantiations of the K-response CSR row-sum kernels (zf_kernels_spmm.h): K = 2 .. 16 times the five lane
// widths of a plan
#include "zf_kernels_spmm.h"

template <int K>
static void zf_spmm_launch_k(const zf_spmv_mat& M, hipStream_t st, const zf_control* ctl, int g, const zf_spmv_io& io, int slot,
                             double out_scale, const dim3 grid, int rb, double* partial) {
    const dim3 block(ZF_BLOCK);
    switch (M.lanes) {
        case 4: hipLaunchKernelGGL((zf_spmm_rows_kernel<4, K>), grid, block, 0, st, M, ctl, g, io, slot, out_scale, rb, partial); break;
        case 8: hipLaunchKernelGGL((zf_spmm_rows_kernel<8, K>), grid, block, 0, st, M, ctl, g, io, slot, out_scale, rb, partial); break;
        case 16: hipLaunchKernelGGL((zf_spmm_rows_kernel<16, K>), grid, block, 0, st, M, ctl, g, io, slot, out_scale, rb, partial); break;
        case 32: hipLaunchKernelGGL((zf_spmm_rows_kernel<32, K>), grid, block, 0, st, M, ctl, g, io, slot, out_scale, rb, partial); break;
        default: hipLaunchKernelGGL((zf_spmm_rows_kernel<64, K>), grid, block, 0, st, M, ctl, g, io, slot, out_scale, rb, partial); break;
    }
    if (M.nsplit > 0)
        hipLaunchKernelGGL(zf_spmm_tail_kernel<K>, dim3(zf_grid_for(M.nsplit * K)), block, 0, st, M, ctl, g, io, slot, out_scale, partial);
}

// the grid of zf_launch_spmv: the row workgroups and the segment workgroups depend on the matrix and its plan alone
void zf_launch_spmm(const zf_spmv_mat& M, hipStream_t st, const zf_control* ctl, bool grad_guard, const zf_spmv_io& io, int slot,
                    double out_scale, int K, double* partial) {
    const int rpb = ZF_BLOCK / M.lanes;
    int64_t row_blocks = (M.rows + rpb - 1) / rpb;
    if (row_blocks > ZF_SPMV_MAX_ROW_BLOCKS) row_blocks = ZF_SPMV_MAX_ROW_BLOCKS;
    const int64_t seg_blocks = (M.nseg + ZF_WAVES - 1) / ZF_WAVES;
    const dim3 grid((unsigned)(row_blocks + seg_blocks));
    const int g = grad_guard ? 1 : 0, rb = (int)row_blocks;
#define ZF_SPMM_CASE(k) \
    case k: zf_spmm_launch_k<k>(M, st, ctl, g, io, slot, out_scale, grid, rb, partial); break;
    switch (K) {
        ZF_SPMM_CASE(2) ZF_SPMM_CASE(3) ZF_SPMM_CASE(4) ZF_SPMM_CASE(5) ZF_SPMM_CASE(6) ZF_SPMM_CASE(7) ZF_SPMM_CASE(8) ZF_SPMM_CASE(9)
        ZF_SPMM_CASE(10) ZF_SPMM_CASE(11) ZF_SPMM_CASE(12) ZF_SPMM_CASE(13) ZF_SPMM_CASE(14) ZF_SPMM_CASE(15) ZF_SPMM_CASE(16)
        default: break;   // (every caller has checked 2 <= K <= ZF_SPMM_MAX_K)
    }
#undef ZF_SPMM_CASE
}
