// zf_kernels_spmm.h - fp64 row sums of a CSR matrix against K gathered, response-interleaved columns (gfx950):
//   out[i K + k] = out_scale * sum_e values[e] * in[indices[e] K + k],  e in [indptr[i], indptr[i + 1]),  k = 0 .. K - 1
// the two sweeps of a sparse trial with K responses (zf_solver_create_sparse_responses): S+ = A X+ on the CSR of A, G = gfac A^T R
// on the stored CSR of A^T, as zf_spmv_rows_kernel serves both for one response.
//
// THE RULE: response k is summed exactly as zf_kernels_spmv.h sums a vector.  The same L from the handle's plan; lane l adds
// elements l, l + L, l + 2L, ... of the row in that order; product and sum are two roundings (-ffp-contract=off); ONE shuffle tree
// (offsets L/2 .. 1); out_scale applied once; rows longer than `threshold` cut into the handle's segments, one wave (L = 64) per
// segment into partial[seg K + k], the tail kernel adding a row's partials in segment order.  So column k of the output is
// bit-equal to the plain sweep on column k of the input, the handle (zf_spmat) is used as it is - no new plan - and the only
// array that grows is the caller's segment sums: nseg K doubles.  No LDS, no atomics: equal input columns give bit-equal output
// columns, and a non-finite value in one column leaves the bits of the others.
//
// What one stored element costs: 12 B of stream (index + value, nontemporal, coalesced over the L lanes) and ONE gathered line
// for all K responses - its K values are K 8 contiguous bytes (K / 2 16-byte loads when K is even: in + idx K is 16-byte aligned
// then; scalar loads when K is odd).  A lane holds K accumulators.  Elements in flight per lane: 4 for K <= 4, 2 beyond
// (zf_spmm_depth: 2 K gathered registers per element in flight; chosen so that no instantiation spills - DESIGN 4.5n has the
// registers of every one); the remainder loads (up to depth - 1) go out together, predicated, and the sums stay in order.
// indices[e] K + k and row K + k are 64-bit: n < 2^31, n K is not.
// (launch declaration: zf_spmv.h; this file is included by zf_spmm.hip alone)
#pragma once
#include "zf_spmv.h"

__device__ __forceinline__ int32_t zf_spmm_ld_stream(const int32_t* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ double zf_spmm_ld_stream(const double* p) { return __builtin_nontemporal_load(p); }

template <int K>
struct zf_spmm_depth {
    static constexpr int U = K <= 4 ? 4 : 2;
};

// v[k] = in[j K + k]
template <int K>
__device__ __forceinline__ void zf_spmm_gather(const double* __restrict__ in, int32_t j, double (&v)[K]) {
    const double* __restrict__ p = in + (int64_t)j * K;
    if constexpr (K % 2 == 0) {
        const double2* __restrict__ p2 = reinterpret_cast<const double2*>(p);
#pragma unroll
        for (int q = 0; q < K / 2; ++q) {
            const double2 t = p2[q];
            v[2 * q] = t.x;
            v[2 * q + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = p[k];
    }
}

// p[k] = v[k], k < K (p + K doubles in bounds; 16-byte aligned when K is even)
template <int K>
__device__ __forceinline__ void zf_spmm_store(double* __restrict__ p, const double (&v)[K]) {
    if constexpr (K % 2 == 0) {
        double2* __restrict__ p2 = reinterpret_cast<double2*>(p);
#pragma unroll
        for (int q = 0; q < K / 2; ++q) p2[q] = make_double2(v[2 * q], v[2 * q + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) p[k] = v[k];
    }
}

// elements lo + lane, lo + lane + L, ... < hi in that order, for every response
template <int L, int K>
__device__ __forceinline__ void zf_spmm_lane_sum(const int32_t* __restrict__ idx, const double* __restrict__ val,
                                                 const double* __restrict__ in, int64_t lo, int64_t hi, int lane, double (&acc)[K]) {
    constexpr int U = zf_spmm_depth<K>::U;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    int64_t e = lo + lane;
    for (; e + (U - 1) * L < hi; e += U * L) {
        int32_t j[U];
        double a[U], v[U][K];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            j[u] = zf_spmm_ld_stream(idx + e + u * L);
            a[u] = zf_spmm_ld_stream(val + e + u * L);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) zf_spmm_gather<K>(in, j[u], v[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] += a[u] * v[u][k];
    }
    // the last one to U - 1 elements of the lane: their loads go out together as well (predicated), the sums stay in order
    int32_t j[U - 1];
    double a[U - 1], v[U - 1][K];
    bool p[U - 1];
#pragma unroll
    for (int u = 0; u < U - 1; ++u) {
        p[u] = e + u * L < hi;
        j[u] = p[u] ? zf_spmm_ld_stream(idx + e + u * L) : 0;
        a[u] = p[u] ? zf_spmm_ld_stream(val + e + u * L) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U - 1; ++u) {
        if (p[u]) {
            zf_spmm_gather<K>(in, j[u], v[u]);
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) v[u][k] = 0.0;
        }
    }
#pragma unroll
    for (int u = 0; u < U - 1; ++u)
        if (p[u]) {
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] += a[u] * v[u][k];
        }
}

// zf_spmv_group_sum for every response: lane 0 of the group holds the K sums
template <int L, int K>
__device__ __forceinline__ void zf_spmm_group_sum(double (&v)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int off = L / 2; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, L);
    }
}

// zf_spmv_rows_kernel with K columns: the same workgroups, the same rows per workgroup and round, the same early exits and ring
// index.  partial: M.nseg K doubles.
template <int L, int K>
__global__ __launch_bounds__(ZF_BLOCK) void zf_spmm_rows_kernel(zf_spmv_mat M, const zf_control* ctl, int grad_guard, zf_spmv_io io, int slot,
                                                                double out_scale, int row_blocks, double* __restrict__ partial) {
    int ring = 0;
    if (ctl) {
        if (ctl->status != ZF_RUNNING) return;
        if (grad_guard && !ctl->need_grad) return;
        if (slot >= 0) ring = (ctl->cur + slot) % 3;
    }
    const double* __restrict__ in = io.in[ring];
    double* __restrict__ out = io.out[ring];
    double t[K];
    if ((int)blockIdx.x >= row_blocks) {
        const int lane = threadIdx.x & 63;
        const int64_t seg = (int64_t)(blockIdx.x - row_blocks) * ZF_WAVES + (threadIdx.x >> 6);
        if (seg >= M.nseg) return;   // (wave-uniform)
        const int64_t lo = M.seg_start[seg];
        const int64_t row_end = M.indptr[M.seg_row[seg] + 1];
        const int64_t hi = lo + M.threshold < row_end ? lo + M.threshold : row_end;
        zf_spmm_lane_sum<64, K>(M.indices, M.values, in, lo, hi, lane, t);
        zf_spmm_group_sum<64, K>(t);
        if (lane == 0) zf_spmm_store<K>(partial + seg * K, t);
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
        zf_spmm_lane_sum<L, K>(M.indices, M.values, in, lo, hi, lane, t);
        zf_spmm_group_sum<L, K>(t);
        if (live && !split && lane == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) t[k] = out_scale * t[k];
            zf_spmm_store<K>(out + row * K, t);
        }
    }
}

// out[row K + k] = out_scale * (partial[first K + k] + partial[(first + 1) K + k] + ...) for every split row and response:
// segment order, one thread per (row, response) - consecutive threads read consecutive doubles
template <int K>
__global__ __launch_bounds__(ZF_BLOCK) void zf_spmm_tail_kernel(zf_spmv_mat M, const zf_control* ctl, int grad_guard, zf_spmv_io io, int slot,
                                                                double out_scale, const double* __restrict__ partial) {
    int ring = 0;
    if (ctl) {
        if (ctl->status != ZF_RUNNING) return;
        if (grad_guard && !ctl->need_grad) return;
        if (slot >= 0) ring = (ctl->cur + slot) % 3;
    }
    double* __restrict__ out = io.out[ring];
    const int64_t stride = (int64_t)gridDim.x * ZF_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * ZF_BLOCK + threadIdx.x; i < M.nsplit * K; i += stride) {
        const int64_t j = i / K;
        const int k = (int)(i - j * K);
        const int64_t s0 = M.split_first[j], s1 = M.split_first[j + 1];
        const double* __restrict__ pk = partial + k;
        double t = pk[s0 * K];
        int64_t s = s0 + 1;
        for (; s + 8 <= s1; s += 8) {   // (eight loads in flight at a time, as zf_spmv_tail_kernel)
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = pk[(s + q) * K];
#pragma unroll
            for (int q = 0; q < 8; ++q) t += v[q];
        }
        for (; s < s1; ++s) t += pk[s * K];
        out[M.split_row[j] * K + k] = out_scale * t;
    }
}
