// zf_kernels_screen.h - gap-safe screening of the l1 margins problems and the restriction of a matrix to the kept columns
// (gfx950 wave64, fp64; no atomics, no scratch, every sum and every output order fixed by the matrix and the mask alone).
//
// The rule.  P(x) = sum_i phi_i(z_i) + lam |x|_1, z = A x, phi_i' L-Lipschitz (least squares L = 2 scale, logistic L = scale / 4):
// the dual is (1/L)-strongly concave, so every feasible nu lies within r = sqrt(2 L gap) of the dual optimum, and
//     alpha |g_j| + r |a_j|_2 < lam   ==>   x_j = 0 at every optimum           (g = grad f(x), nu = alpha grad phi(z))
// In fp64 the radius is widened to r_eff = r + E; E |a_j| bounds, by Cauchy-Schwarz, everything the evaluation of the left
// side loses (first order, u = 2^-53, with the factor 2 of the project's element-wise bounds):
//     R, C     stored elements of the longest row / column of A;  S1 = sum |x_j|;  |A|_F = sqrt(sum_j |a_j|^2);  amax = max_j |a_j|
//     margins  |dz|_2 <= R u |A|_F S1
//     dual candidate (c = r or rho, without its factor)
//              least squares  |dc|_2 <= |dz|_2 + u |r|_2,  |c|_2 = |r|_2 = sqrt(sum r^2)
//              logistic       |dc|_2 <= |dz|_2 / 4 + 5 u sqrt(m),  |c|_2 <= sqrt(m)            (|rho_i| <= 1)
//     g_j      dg_j <= |a_j| Eg,  Eg = gfac (|dc|_2 + (C + 2) u |c|_2),  gfac = 2 scale | scale;   |g_j| <= gfac |c|_2 |a_j|
//     alpha    d(alpha) <= Eg amax / lam + u   (alpha = min(1, lam / |g|_inf), |g|_inf within Eg amax)
//     left side, its own three roundings and the norm's (C / 2 + 2) u:
//              X = Eg (1 + gfac |c|_2 amax / lam) + u (4 gfac |c|_2 + (C / 2 + 4) r)
//     gap      relative error below 2^-20 (asserted by the tests from the gap's own bound; a gap so close to its rounding
//              error certifies nothing anyway): dr <= 2^-21 r
//     E = 2 X + 2^-20 r
// A non-finite gap, alpha or E makes r_eff = +inf and a non-finite g_j fails the comparison: everything is kept.
//
// Kernels:
//   column norms   sparse: row sums of squares over the stored CSR of A^T with the plan's lanes and the segment / tail scheme
//                  of zf_kernels_spmv.h;  dense: one thread per column, rows in order.  Then sum |a_j|^2 and max |a_j|.
//   screen         zf_scr_radius_kernel (one thread): r, E, r_eff;  zf_scr_mask_kernel: keep_j and the kept count of each
//                  chunk;  zf_scr_offsets_kernel: chunk counts -> chunk offsets, in chunk order;  zf_scr_scan_kernel: the
//                  exclusive scan of the mask (the new column index).  Chunks as the gap's n-passes: one workgroup up to
//                  4096 elements, contiguous chunks of 2048 (at most 1024, longer then) beyond.
//   restrict       sparse: zf_scr_rcount_kernel (kept elements per row of A; per segment for split rows, turned into
//                  offsets by the tail), zf_scr_tlen_kernel (lengths of the kept rows of A^T); the row pointers are scans of
//                  those lengths (the caller's); zf_scr_fill_A_kernel writes every row of A with its kept elements in stored
//                  order - ballot plus prefix popcount over the L lanes of a row (64 for a segment) - and renumbered
//                  columns, zf_scr_fill_At_kernel copies the kept rows of A^T whole.  Values and indices are streamed
//                  (nontemporal) as in the SpMV kernels.  dense: zf_scr_gather_dense_kernel, A[:, keep] row-major.
// (launch declarations: zf_screen.h; this file is included by zf_screen.hip alone)
#pragma once
#include <float.h>

#include "zf_screen.h"

constexpr int64_t ZF_SCR_ONE_WG_MAX_N = 4096;   // = ZF_GAP_ONE_WG_MAX_N
constexpr int64_t ZF_SCR_CHUNK_ELEMS = 2048;    // = ZF_GAP_CHUNK_ELEMS

static inline int zf_scr_chunks(int64_t n) {
    if (n <= ZF_SCR_ONE_WG_MAX_N) return 1;
    const int64_t c = (n + ZF_SCR_CHUNK_ELEMS - 1) / ZF_SCR_CHUNK_ELEMS;
    return (int)(c > ZF_SCREEN_MAX_CHUNKS ? ZF_SCREEN_MAX_CHUNKS : c);
}

__device__ __forceinline__ void zf_scr_chunk_of(int64_t len, int64_t& lo, int64_t& hi) {
    const int64_t per = (len + gridDim.x - 1) / gridDim.x;
    lo = (int64_t)blockIdx.x * per;
    if (lo > len) lo = len;
    hi = lo + per < len ? lo + per : len;
}

__device__ __forceinline__ int32_t zf_scr_ld(const int32_t* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ double zf_scr_ld(const double* p) { return __builtin_nontemporal_load(p); }

template <int L>
__device__ __forceinline__ double zf_scr_group_sum(double v) {
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) v += __shfl_down(v, off, L);
    return v;
}
template <int L>
__device__ __forceinline__ int zf_scr_group_sum_int(int v) {
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) v += __shfl_down(v, off, L);
    return v;
}

// the workgroup's integer sum (every thread holds it)
__device__ __forceinline__ int zf_scr_block_sum_int(int v, int* lds /* ZF_WAVES */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    for (int w = 0; w < ZF_WAVES; ++w) t += lds[w];
    __syncthreads();
    return t;
}

// ---- column norms, sparse: sqrt of the row sums of squares of the CSR of A^T ---------------------------------------------------
// elements lo + lane, lo + lane + L, ... < hi in that order, four loads in flight
template <int L>
__device__ __forceinline__ double zf_scr_lane_sumsq(const double* __restrict__ val, int64_t lo, int64_t hi, int lane) {
    double acc = 0.0;
    int64_t k = lo + lane;
    for (; k + 3 * L < hi; k += 4 * L) {
        double a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = zf_scr_ld(val + k + u * L);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += a[u] * a[u];
    }
    for (; k < hi; k += L) {
        const double a = zf_scr_ld(val + k);
        acc += a * a;
    }
    return acc;
}

// workgroups [0, row_blocks): rows of at most `threshold` elements, ZF_BLOCK / L rows per workgroup and round; behind them
// one wave per segment of the longer rows -> partial[segment]   (the shape of zf_spmv_rows_kernel)
template <int L>
__global__ __launch_bounds__(ZF_BLOCK) void zf_scr_norms_rows_kernel(zf_spmv_mat M, int row_blocks, double* __restrict__ out,
                                                                     double* __restrict__ partial) {
    if ((int)blockIdx.x >= row_blocks) {
        const int lane = threadIdx.x & 63;
        const int64_t seg = (int64_t)(blockIdx.x - row_blocks) * ZF_WAVES + (threadIdx.x >> 6);
        if (seg >= M.nseg) return;   // (wave-uniform)
        const int64_t lo = M.seg_start[seg];
        const int64_t row_end = M.indptr[M.seg_row[seg] + 1];
        const int64_t hi = lo + M.threshold < row_end ? lo + M.threshold : row_end;
        const double t = zf_scr_group_sum<64>(zf_scr_lane_sumsq<64>(M.values, lo, hi, lane));
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
        const bool split = hi - lo > M.threshold;
        if (split) hi = lo;
        const double t = zf_scr_group_sum<L>(zf_scr_lane_sumsq<L>(M.values, lo, hi, lane));
        if (live && !split && lane == 0) out[row] = sqrt(t);
    }
}

__global__ __launch_bounds__(ZF_BLOCK) void zf_scr_norms_tail_kernel(zf_spmv_mat M, double* __restrict__ out, const double* __restrict__ partial) {
    const int64_t stride = (int64_t)gridDim.x * ZF_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * ZF_BLOCK + threadIdx.x; j < M.nsplit; j += stride) {
        const int64_t s0 = M.split_first[j], s1 = M.split_first[j + 1];
        double t = partial[s0];
        for (int64_t s = s0 + 1; s < s1; ++s) t += partial[s];   // segment order
        out[M.split_row[j]] = sqrt(t);
    }
}

// ---- column norms, dense row-major: one thread per column, rows in order ----------------------------------------------------------
__global__ __launch_bounds__(ZF_BLOCK) void zf_scr_norms_dense_kernel(const double* __restrict__ A, int64_t m, int64_t n, double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * ZF_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * ZF_BLOCK + threadIdx.x; j < n; j += stride) {
        const double* __restrict__ col = A + j;
        double acc = 0.0;
        int64_t i = 0;
        for (; i + 4 <= m; i += 4) {
            double a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = col[(i + u) * n];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += a[u] * a[u];
        }
        for (; i < m; ++i) {
            const double a = col[i * n];
            acc += a * a;
        }
        out[j] = sqrt(acc);
    }
}

// ---- sum_j |a_j|^2 and max_j |a_j|: chunk results, then in chunk order ---------------------------------------------------------------
__device__ __forceinline__ void zf_scr_block_sum_max(double& s, double& mx, double* lds /* 2 * ZF_WAVES */) {
    s = zf_wave_sum(s);
    mx = zf_wave_max(mx);
    if ((threadIdx.x & 63) == 0) {
        lds[threadIdx.x >> 6] = s;
        lds[ZF_WAVES + (threadIdx.x >> 6)] = mx;
    }
    __syncthreads();
    double ts = lds[0], tm = lds[ZF_WAVES];
    for (int w = 1; w < ZF_WAVES; ++w) {
        ts += lds[w];
        tm = fmax(tm, lds[ZF_WAVES + w]);
    }
    s = ts;
    mx = tm;
}

// FINISH = false: the chunk of the workgroup of `v` = norms -> part (or stats, one workgroup); true: the chunk results -> stats
template <bool FINISH>
__global__ __launch_bounds__(ZF_BLOCK) void zf_scr_stats_kernel(const double* __restrict__ v, int64_t len, double* __restrict__ part,
                                                                double* __restrict__ stats) {
    __shared__ double lds[2 * ZF_WAVES];
    double s = 0.0, mx = 0.0;
    if (FINISH) {
        for (int64_t i = threadIdx.x; i < len; i += ZF_BLOCK) {
            s += v[i];
            mx = fmax(mx, v[ZF_SCREEN_MAX_CHUNKS + i]);
        }
    } else {
        int64_t lo, hi;
        zf_scr_chunk_of(len, lo, hi);
        for (int64_t j = lo + threadIdx.x; j < hi; j += ZF_BLOCK) {
            const double a = v[j];
            s += a * a;
            mx = fmax(mx, a);
        }
    }
    zf_scr_block_sum_max(s, mx, lds);
    if (threadIdx.x == 0) {
        if (FINISH || gridDim.x == 1) {
            stats[0] = s;
            stats[1] = mx;
        } else {
            part[blockIdx.x] = s;
            part[ZF_SCREEN_MAX_CHUNKS + blockIdx.x] = mx;
        }
    }
}

// ---- the radius (one thread) ---------------------------------------------------------------------------------------------------------
__global__ void zf_scr_radius_kernel(const double* __restrict__ gap8, const double* __restrict__ asum, const double* __restrict__ rr,
                                     const double* __restrict__ stats, int64_t m, int64_t max_row, int64_t max_col, double scale,
                                     double lam, int logistic, double* __restrict__ sscal) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double u = 0x1p-53;
    const double gap = gap8[2], alpha = gap8[3];
    const double lip = logistic ? 0.25 * scale : 2.0 * scale;
    const double gfac = logistic ? scale : 2.0 * scale;
    const double r = sqrt(2.0 * lip * gap);
    const double fro = sqrt(stats[0]), amax = stats[1];
    const double dz = (double)max_row * u * fro * asum[0];
    double cn, dc;
    if (logistic) {
        cn = sqrt((double)m);
        dc = 0.25 * dz + 5.0 * u * cn;
    } else {
        cn = sqrt(rr[0]);
        dc = dz + u * cn;
    }
    const double eg = gfac * (dc + (double)(max_col + 2) * u * cn) + (logistic ? (double)m * 0x1p-1022 : 0.0);
    const double x = eg * (1.0 + gfac * cn * amax / lam) + u * (4.0 * gfac * cn + (0.5 * (double)max_col + 4.0) * r);
    const double e = 2.0 * x + 0x1p-20 * r;
    double reff = r + e;
    if (!(reff <= DBL_MAX) || !(fabs(alpha) <= DBL_MAX)) reff = INFINITY;   // non-finite gap, alpha or E (lam = 0): keep everything
    sscal[0] = r;
    sscal[1] = e;
    sscal[2] = reff;
}

// ---- the mask and the kept count of each chunk -----------------------------------------------------------------------------------------
// SCREEN: keep_j = !(alpha |g_j| + r_eff |a_j| < lam), written; else: the caller's mask, counted
template <bool SCREEN>
__global__ __launch_bounds__(ZF_BLOCK) void zf_scr_mask_kernel(const double* __restrict__ g, const double* __restrict__ norms,
                                                               const double* __restrict__ gap8, const double* __restrict__ sscal, int64_t n,
                                                               double lam, uint8_t* __restrict__ keep, int32_t* __restrict__ cnt) {
    __shared__ int lds[ZF_WAVES];
    double alpha = 0.0, reff = 0.0;
    if (SCREEN) {
        alpha = gap8[3];
        reff = sscal[2];
    }
    int64_t lo, hi;
    zf_scr_chunk_of(n, lo, hi);
    int c = 0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += ZF_BLOCK) {
        int k;
        if (SCREEN) {
            const double t = alpha * fabs(g[j]) + reff * norms[j];
            k = !(t < lam);   // (a NaN - a non-finite g_j, inf * 0 - keeps the column)
            keep[j] = (uint8_t)k;
        } else {
            k = keep[j] != 0;
        }
        c += k;
    }
    c = zf_scr_block_sum_int(c, lds);
    if (threadIdx.x == 0) cnt[blockIdx.x] = c;
}

// cnt[0 .. count) -> their exclusive scan in place, cnt[count] = the total (also to *total_out as a double): one workgroup,
// thread t takes the entries 4 t .. 4 t + 3
__global__ __launch_bounds__(ZF_BLOCK) void zf_scr_offsets_kernel(int32_t* __restrict__ cnt, int count, double* __restrict__ total_out) {
    __shared__ int lds[ZF_WAVES];
    static_assert(4 * ZF_BLOCK >= ZF_SCREEN_MAX_CHUNKS, "four chunk counts per thread");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int v[4], mine = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = 4 * (int)threadIdx.x + q;
        v[q] = i < count ? cnt[i] : 0;
        mine += v[q];
    }
    int inc = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < ZF_WAVES; ++w) {
        if (w < wave) base += lds[w];
        total += lds[w];
    }
    int run = base + inc - mine;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = 4 * (int)threadIdx.x + q;
        if (i < count) cnt[i] = run;
        run += v[q];
    }
    if (threadIdx.x == 0) {
        cnt[count] = total;
        if (total_out) *total_out = (double)total;
    }
}

// index_j = off[chunk] + the kept elements of the chunk before j: tiles of ZF_BLOCK in order, ballot + prefix popcount per wave
__global__ __launch_bounds__(ZF_BLOCK) void zf_scr_scan_kernel(const uint8_t* __restrict__ keep, int64_t n, const int32_t* __restrict__ off,
                                                               int32_t* __restrict__ index) {
    __shared__ int lds[ZF_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t lo, hi;
    zf_scr_chunk_of(n, lo, hi);
    int run = off[blockIdx.x];
    for (int64_t t0 = lo; t0 < hi; t0 += ZF_BLOCK) {   // (uniform over the workgroup)
        const int64_t j = t0 + threadIdx.x;
        const bool f = j < hi && keep[j] != 0;
        const unsigned long long bal = __ballot(f);
        if (lane == 0) lds[wave] = __popcll(bal);
        __syncthreads();
        int base = 0, total = 0;
        for (int w = 0; w < ZF_WAVES; ++w) {
            if (w < wave) base += lds[w];
            total += lds[w];
        }
        if (j < hi) index[j] = run + base + __popcll(bal & ((1ull << lane) - 1ull));
        run += total;
        __syncthreads();
    }
}

// ---- restriction, sparse: counts ---------------------------------------------------------------------------------------------------------
// the kept elements of every row of A -> len_out[row]; of every segment of a split row -> seg_cnt[segment]
template <int L>
__global__ __launch_bounds__(ZF_BLOCK) void zf_scr_rcount_kernel(zf_spmv_mat M, int row_blocks, const uint8_t* __restrict__ keep,
                                                                 int64_t* __restrict__ len_out, int32_t* __restrict__ seg_cnt) {
    if ((int)blockIdx.x >= row_blocks) {
        const int lane = threadIdx.x & 63;
        const int64_t seg = (int64_t)(blockIdx.x - row_blocks) * ZF_WAVES + (threadIdx.x >> 6);
        if (seg >= M.nseg) return;   // (wave-uniform)
        const int64_t lo = M.seg_start[seg];
        const int64_t row_end = M.indptr[M.seg_row[seg] + 1];
        const int64_t hi = lo + M.threshold < row_end ? lo + M.threshold : row_end;
        int c = 0;
        for (int64_t k = lo + lane; k < hi; k += 64) c += keep[zf_scr_ld(M.indices + k)] != 0;
        c = zf_scr_group_sum_int<64>(c);
        if (lane == 0) seg_cnt[seg] = c;
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
        const bool split = hi - lo > M.threshold;
        if (split) hi = lo;
        int c = 0;
        for (int64_t k = lo + lane; k < hi; k += L) c += keep[zf_scr_ld(M.indices + k)] != 0;
        c = zf_scr_group_sum_int<L>(c);
        if (live && !split && lane == 0) len_out[row] = c;
    }
}

// split rows: the segment counts -> their offsets inside the row (segment order), the row's kept length
__global__ __launch_bounds__(ZF_BLOCK) void zf_scr_rcount_tail_kernel(zf_spmv_mat M, int64_t* __restrict__ len_out, int32_t* __restrict__ seg_cnt) {
    const int64_t stride = (int64_t)gridDim.x * ZF_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * ZF_BLOCK + threadIdx.x; j < M.nsplit; j += stride) {
        int64_t run = 0;
        for (int64_t s = M.split_first[j]; s < M.split_first[j + 1]; ++s) {
            const int c = seg_cnt[s];
            seg_cnt[s] = (int32_t)run;
            run += c;
        }
        len_out[M.split_row[j]] = run;
    }
}

// the lengths of the kept rows of A^T, at their new row numbers
__global__ __launch_bounds__(ZF_BLOCK) void zf_scr_tlen_kernel(const int64_t* __restrict__ t_indptr, int64_t n, const uint8_t* __restrict__ keep,
                                                               const int32_t* __restrict__ index, int64_t* __restrict__ len_out) {
    const int64_t stride = (int64_t)gridDim.x * ZF_BLOCK;
    for (int64_t j = (int64_t)blockIdx.x * ZF_BLOCK + threadIdx.x; j < n; j += stride)
        if (keep[j]) len_out[index[j]] = t_indptr[j + 1] - t_indptr[j];
}

// ---- restriction, sparse: fill -------------------------------------------------------------------------------------------------------------
// the kept elements of the W lanes [first, first + W) of this wave, one element per lane, to dst .. in lane order; returns
// how many there were.  Every lane of the wave calls it (f = false where it has no element).
template <int W>
__device__ __forceinline__ int zf_scr_emit(bool f, int lane_in_group, int first, int64_t dst, int32_t col, double a,
                                           int32_t* __restrict__ out_idx, double* __restrict__ out_val) {
    unsigned long long bal = __ballot(f);
    if (W < 64) bal = (bal >> first) & ((1ull << (W & 63)) - 1ull);
    if (f) {
        const int64_t p = dst + __popcll(bal & ((1ull << lane_in_group) - 1ull));
        out_idx[p] = col;
        out_val[p] = a;
    }
    return __popcll(bal);
}

// new_ptr: the row pointers of the restricted A; seg_off: zf_scr_rcount_tail_kernel's offsets
template <int L>
__global__ __launch_bounds__(ZF_BLOCK) void zf_scr_fill_A_kernel(zf_spmv_mat M, int row_blocks, const uint8_t* __restrict__ keep,
                                                                 const int32_t* __restrict__ index, const int64_t* __restrict__ new_ptr,
                                                                 const int32_t* __restrict__ seg_off, int32_t* __restrict__ out_idx,
                                                                 double* __restrict__ out_val) {
    if ((int)blockIdx.x >= row_blocks) {
        const int lane = threadIdx.x & 63;
        const int64_t seg = (int64_t)(blockIdx.x - row_blocks) * ZF_WAVES + (threadIdx.x >> 6);
        if (seg >= M.nseg) return;   // (wave-uniform)
        const int64_t row = M.seg_row[seg];
        const int64_t lo = M.seg_start[seg];
        const int64_t row_end = M.indptr[row + 1];
        const int64_t hi = lo + M.threshold < row_end ? lo + M.threshold : row_end;
        int64_t dst = new_ptr[row] + seg_off[seg];
        for (int64_t k0 = lo; k0 < hi; k0 += 64) {   // (wave-uniform)
            const int64_t k = k0 + lane;
            const bool act = k < hi;
            const int32_t j = act ? zf_scr_ld(M.indices + k) : 0;
            const double a = act ? zf_scr_ld(M.values + k) : 0.0;
            const bool f = act && keep[j] != 0;
            dst += zf_scr_emit<64>(f, lane, 0, dst, f ? index[j] : 0, a, out_idx, out_val);
        }
        return;
    }
    constexpr int RPB = ZF_BLOCK / L;
    const int lane = threadIdx.x & (L - 1);
    const int sub = threadIdx.x / L;
    const int first = (threadIdx.x & 63) - lane;   // the group's first lane in its wave
    for (int64_t base = (int64_t)blockIdx.x * RPB; base < M.rows; base += (int64_t)row_blocks * RPB) {
        const int64_t row = base + sub;
        const bool live = row < M.rows;
        int64_t lo = 0, hi = 0, dst = 0;
        if (live) {
            lo = M.indptr[row];
            hi = M.indptr[row + 1];
        }
        if (hi - lo > M.threshold) hi = lo;   // (its segments write this row)
        if (hi > lo) dst = new_ptr[row];
        // rounds of L elements, as many as the longest row of the wave needs: every lane of the wave takes part in the ballot
        int rounds = (int)((hi - lo + L - 1) / L);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(rounds, off, 64);
            rounds = o > rounds ? o : rounds;
        }
        for (int r = 0; r < rounds; ++r) {
            const int64_t k = lo + (int64_t)r * L + lane;
            const bool act = k < hi;
            const int32_t j = act ? zf_scr_ld(M.indices + k) : 0;
            const double a = act ? zf_scr_ld(M.values + k) : 0.0;
            const bool f = act && keep[j] != 0;
            dst += zf_scr_emit<L>(f, lane, first, dst, f ? index[j] : 0, a, out_idx, out_val);
        }
    }
}

// the kept rows of A^T (M), whole, to their new places; new_ptr: the row pointers of the restricted A^T
template <int L>
__global__ __launch_bounds__(ZF_BLOCK) void zf_scr_fill_At_kernel(zf_spmv_mat M, int row_blocks, const uint8_t* __restrict__ keep,
                                                                  const int32_t* __restrict__ index, const int64_t* __restrict__ new_ptr,
                                                                  int32_t* __restrict__ out_idx, double* __restrict__ out_val) {
    if ((int)blockIdx.x >= row_blocks) {
        const int lane = threadIdx.x & 63;
        const int64_t seg = (int64_t)(blockIdx.x - row_blocks) * ZF_WAVES + (threadIdx.x >> 6);
        if (seg >= M.nseg) return;
        const int64_t row = M.seg_row[seg];
        if (!keep[row]) return;
        const int64_t lo = M.seg_start[seg];
        const int64_t row_end = M.indptr[row + 1];
        const int64_t hi = lo + M.threshold < row_end ? lo + M.threshold : row_end;
        const int64_t shift = new_ptr[index[row]] - M.indptr[row];
        for (int64_t k = lo + lane; k < hi; k += 64) {
            out_idx[k + shift] = zf_scr_ld(M.indices + k);
            out_val[k + shift] = zf_scr_ld(M.values + k);
        }
        return;
    }
    constexpr int RPB = ZF_BLOCK / L;
    const int lane = threadIdx.x & (L - 1);
    const int sub = threadIdx.x / L;
    for (int64_t base = (int64_t)blockIdx.x * RPB; base < M.rows; base += (int64_t)row_blocks * RPB) {
        const int64_t row = base + sub;
        if (row >= M.rows || !keep[row]) continue;
        const int64_t lo = M.indptr[row], hi = M.indptr[row + 1];
        if (hi - lo > M.threshold) continue;   // (its segments copy this row)
        const int64_t shift = new_ptr[index[row]] - lo;
        for (int64_t k = lo + lane; k < hi; k += L) {
            out_idx[k + shift] = zf_scr_ld(M.indices + k);
            out_val[k + shift] = zf_scr_ld(M.values + k);
        }
    }
}

// ---- restriction, dense: out (m x k, row-major) = A[:, keep] -------------------------------------------------------------------------------
__global__ __launch_bounds__(ZF_BLOCK) void zf_scr_gather_dense_kernel(const double* __restrict__ A, int64_t m, int64_t n,
                                                                       const uint8_t* __restrict__ keep, const int32_t* __restrict__ index,
                                                                       int64_t k, double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * ZF_BLOCK + threadIdx.x;
    if (j >= n || !keep[j]) return;
    const int64_t c = index[j];
    for (int64_t i = blockIdx.y; i < m; i += gridDim.y) out[i * k + c] = A[i * n + j];
}
