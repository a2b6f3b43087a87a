// zf_kernels_spmv.h - fp64 row sums of a CSR matrix against a gathered vector (gfx950):
//   out[i] = out_scale * sum_k values[k] * in[indices[k]],  k in [indptr[i], indptr[i + 1])
// the two sweeps of a sparse least-squares trial (ZF_PROBLEM_SPARSE_LS_L1):
//   s+ = A x+                  CSR of A,   gathered x+ (n),         every trial
//   grad = 2 scale A^T r       CSR of A^T, gathered r = A y - b (m), only when y changed (ctl->need_grad)
// A^T is STORED (24 B per stored element for the pair) instead of scattered into: a float atomic sum depends on the
// arrival order, and every decision of a solve is a function of the problem alone.
//
// Summation order - fixed by the matrix and its plan, never by the grid or by timing:
//  * a row of at most `threshold` elements: L lanes (a power of two, 4 .. 64, chosen once from the mean row length),
//    lane l adds elements l, l + L, l + 2L, ... of the row in that order, then ONE shuffle tree (offsets L/2 .. 1)
//    whose lane 0 holds the row sum;
//  * a longer row (an intercept column is a dense row of A^T; a bag-of-words matrix has rows thousands of times the
//    median) is cut into segments of `threshold` elements.  One wave per segment sums it as a row with L = 64 into
//    partial[segment] (an array of the sweep's caller); the tail kernel adds the partials of a row in segment order.
//    The segment list comes from the host (zfista_amd.sparse.plan_rows), built from indptr when the problem is created.
// Streaming operands (values 8 B + indices 4 B per element) are read once per sweep, coalesced across the L lanes of
// a row and nontemporal, so that the gathered vector keeps its place in L2 / the memory-side cache.  No LDS, no atomics.
// The product and the sum of an element are two roundings (-ffp-contract=off).
// (structs and launch declarations: zf_spmv.h; this file is included by zf_spmv.hip alone)
#pragma once
#include "zf_spmv.h"

__device__ __forceinline__ int32_t zf_spmv_ld_stream(const int32_t* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ double zf_spmv_ld_stream(const double* p) { return __builtin_nontemporal_load(p); }

// elements lo + lane, lo + lane + L, ... < hi in that order; up to four loads of each stream in flight
template <int L>
__device__ __forceinline__ double zf_spmv_lane_sum(const int32_t* __restrict__ idx, const double* __restrict__ val,
                                                   const double* __restrict__ in, int64_t lo, int64_t hi, int lane) {
    double acc = 0.0;
    int64_t k = lo + lane;
    for (; k + 3 * L < hi; k += 4 * L) {
        int32_t j[4];
        double a[4], v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            j[u] = zf_spmv_ld_stream(idx + k + u * L);
            a[u] = zf_spmv_ld_stream(val + k + u * L);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = in[j[u]];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += a[u] * v[u];
    }
    // the last one to three elements of the lane: their loads go out together as well (predicated), the sums stay in order
    int32_t j[3];
    double a[3], v[3];
    bool p[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        p[u] = k + u * L < hi;
        j[u] = p[u] ? zf_spmv_ld_stream(idx + k + u * L) : 0;
        a[u] = p[u] ? zf_spmv_ld_stream(val + k + u * L) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) v[u] = p[u] ? in[j[u]] : 0.0;
#pragma unroll
    for (int u = 0; u < 3; ++u)
        if (p[u]) acc += a[u] * v[u];
    return acc;
}

// the fixed tree over the L lanes of a row: lane 0 of the group holds the sum
template <int L>
__device__ __forceinline__ double zf_spmv_group_sum(double v) {
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) v += __shfl_down(v, off, L);
    return v;
}

// Workgroups [0, row_blocks): rows of at most `threshold` elements, ZF_BLOCK / L rows per workgroup and round.
// Workgroups behind them: one wave per segment of the longer rows -> partial[segment].
// ctl != NULL: leave at once unless the solve is running (and, grad_guard, unless the gradient is due); slot >= 0: the
// ring index (ctl->cur + slot) % 3, as zf_gemv_rows_kernel.
template <int L>
__global__ __launch_bounds__(ZF_BLOCK) void zf_spmv_rows_kernel(zf_spmv_mat M, const zf_control* ctl, int grad_guard, zf_spmv_io io,
                                                                int slot, double out_scale, int row_blocks, double* __restrict__ partial) {
    int ring = 0;
    if (ctl) {
        if (ctl->status != ZF_RUNNING) return;
        if (grad_guard && !ctl->need_grad) return;
        if (slot >= 0) ring = (ctl->cur + slot) % 3;
    }
    const double* __restrict__ in = io.in[ring];
    double* __restrict__ out = io.out[ring];
    if ((int)blockIdx.x >= row_blocks) {
        const int lane = threadIdx.x & 63;
        const int64_t seg = (int64_t)(blockIdx.x - row_blocks) * ZF_WAVES + (threadIdx.x >> 6);
        if (seg >= M.nseg) return;   // (wave-uniform)
        const int64_t lo = M.seg_start[seg];
        const int64_t row_end = M.indptr[M.seg_row[seg] + 1];
        const int64_t hi = lo + M.threshold < row_end ? lo + M.threshold : row_end;
        const double t = zf_spmv_group_sum<64>(zf_spmv_lane_sum<64>(M.indices, M.values, in, lo, hi, lane));
        if (lane == 0) partial[seg] = t;
        return;
    }
    constexpr int RPB = ZF_BLOCK / L;
    const int lane = threadIdx.x & (L - 1);
    const int sub = threadIdx.x / L;
    for (int64_t base = (int64_t)blockIdx.x * RPB; base < M.rows; base += (int64_t)row_blocks * RPB) {
        const int64_t row = base + sub;
        const bool live = row < M.rows;
        int64_t lo = 0, hi = 0;
        if (live) {
            lo = M.indptr[row];
            hi = M.indptr[row + 1];
        }
        const bool split = hi - lo > M.threshold;   // (its segments and the tail kernel write this row)
        if (split) hi = lo;
        const double t = zf_spmv_group_sum<L>(zf_spmv_lane_sum<L>(M.indices, M.values, in, lo, hi, lane));
        if (live && !split && lane == 0) out[row] = out_scale * t;
    }
}

// out[row] = out_scale * (partial[first] + partial[first + 1] + ...) for every split row: segment order
__global__ __launch_bounds__(ZF_BLOCK) void zf_spmv_tail_kernel(zf_spmv_mat M, const zf_control* ctl, int grad_guard, zf_spmv_io io, int slot,
                                                                double out_scale, const double* __restrict__ partial) {
    int ring = 0;
    if (ctl) {
        if (ctl->status != ZF_RUNNING) return;
        if (grad_guard && !ctl->need_grad) return;
        if (slot >= 0) ring = (ctl->cur + slot) % 3;
    }
    double* __restrict__ out = io.out[ring];
    const int64_t stride = (int64_t)gridDim.x * ZF_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * ZF_BLOCK + threadIdx.x; j < M.nsplit; j += stride) {
        const int64_t s0 = M.split_first[j], s1 = M.split_first[j + 1];
        // added in segment order; eight loads in flight at a time (a 10^6-element row has 245 partials: one load latency
        // each took 22 us)
        double t = partial[s0];
        int64_t s = s0 + 1;
        for (; s + 8 <= s1; s += 8) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = partial[s + k];
#pragma unroll
            for (int k = 0; k < 8; ++k) t += v[k];
        }
        for (; s < s1; ++s) t += partial[s];
        out[M.split_row[j]] = out_scale * t;
    }
}
