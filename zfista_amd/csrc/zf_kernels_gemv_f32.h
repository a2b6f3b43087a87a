// zf_kernels_gemv_f32.h - the two dense sweeps of zf_kernels_gemv.h over a matrix STORED in fp32 (zf_solver_set_matrix_f32):
//   s = A x (rows) and slab[slice][j] = sum_{i in slice} A[i][j] r[i] (columns), A row-major m_rows x n floats in HBM.
// Both sweeps are bound by streaming A, so half the bytes per element is the whole point; everything else stays double:
// x, r, the accumulators, the slab, the outputs.  An element is widened in a register ((double)a: every float is a double,
// the conversion is exact), so the kernels compute in fp64 on float64(A) - the fp64 problem of that matrix, summed in
// another order.  Fixed-order reductions, no atomics: bit-reproducible.  A is loaded nontemporally (zf_ld_stream).
// V floats per load: 4 when n % 4 == 0 (rows are 16-byte aligned: one 16-byte load, the rate the fp64 sweeps stream at),
// 2 when n % 4 == 2 (8-byte loads), 1 for odd n.  V = 4 is the path that matters; 2 and 1 exist for correctness at every n.
#pragma once
#include "zf_kernels_gemv.h"

// Rows per workgroup of the row sweep.  Every workgroup re-reads x from L2 / Infinity Cache: (m / rows) n 8 bytes beside the
// m n 4 bytes of A.  With the 2 rows of the fp64 sweep that is as many bytes of x as of A (fp64: half as many); 4 rows restore
// the fp64 sweep's ratio.  Measured on 16384 x 65536 (rocprofv3 kernel trace, one sweep = 4.29 GB): 2 rows 0.716 ms = 6.00 TB/s,
// 4 rows 0.621 ms = 6.91 TB/s (the fp64 sweep in the same trace: 1.256 ms = 6.84 TB/s).
#ifndef ZF_GEMV_ROWS_F32
#define ZF_GEMV_ROWS_F32 4
#endif
constexpr int GEMV_ROWS_F32 = ZF_GEMV_ROWS_F32;
typedef float zf_f32x2 __attribute__((ext_vector_type(2)));
typedef float zf_f32x4 __attribute__((ext_vector_type(4)));
template <int V> struct zf_f32vec;
template <> struct zf_f32vec<1> { using type = float; };
template <> struct zf_f32vec<2> { using type = zf_f32x2; };
template <> struct zf_f32vec<4> { using type = zf_f32x4; };
static inline int zf_f32_width(int64_t n) { return (n % 4 == 0) ? 4 : (n % 2 == 0) ? 2 : 1; }

// x[V*j .. V*j + V) as doubles (16-byte loads where V allows: x is 16-byte aligned like every vector of the solver)
template <int V> struct zf_xvec { double v[V]; };
template <int V> __device__ __forceinline__ zf_xvec<V> zf_ld_x(const double* __restrict__ x, int64_t j);
template <> __device__ __forceinline__ zf_xvec<1> zf_ld_x<1>(const double* __restrict__ x, int64_t j) { return {{x[j]}}; }
template <> __device__ __forceinline__ zf_xvec<2> zf_ld_x<2>(const double* __restrict__ x, int64_t j) {
    const double2 a = reinterpret_cast<const double2*>(x)[j];
    return {{a.x, a.y}};
}
template <> __device__ __forceinline__ zf_xvec<4> zf_ld_x<4>(const double* __restrict__ x, int64_t j) {
    const double2 a = reinterpret_cast<const double2*>(x)[2 * j], b = reinterpret_cast<const double2*>(x)[2 * j + 1];
    return {{a.x, a.y, b.x, b.y}};
}
// sum_v (double)a[v] * x[v], left to right as zf_dot_row
__device__ __forceinline__ double zf_dot_f32(float a, const zf_xvec<1>& x) { return (double)a * x.v[0]; }
__device__ __forceinline__ double zf_dot_f32(zf_f32x2 a, const zf_xvec<2>& x) { return (double)a.x * x.v[0] + (double)a.y * x.v[1]; }
__device__ __forceinline__ double zf_dot_f32(zf_f32x4 a, const zf_xvec<4>& x) {
    return (double)a.x * x.v[0] + (double)a.y * x.v[1] + (double)a.z * x.v[2] + (double)a.w * x.v[3];
}
// acc[v] += (double)a[v] * s
__device__ __forceinline__ void zf_fma_f32(double (&acc)[1], float a, double s) { acc[0] += (double)a * s; }
__device__ __forceinline__ void zf_fma_f32(double (&acc)[2], zf_f32x2 a, double s) {
    acc[0] += (double)a.x * s;
    acc[1] += (double)a.y * s;
}
__device__ __forceinline__ void zf_fma_f32(double (&acc)[4], zf_f32x4 a, double s) {
    acc[0] += (double)a.x * s;
    acc[1] += (double)a.y * s;
    acc[2] += (double)a.z * s;
    acc[3] += (double)a.w * s;
}

// ---- s_out = A x_in  (row dot products) ------------------------------------
// zf_gemv_rows_kernel with float rows: GEMV_ROWS_F32 rows per workgroup, row groups in a grid-stride loop once the grid is
// capped, `slot` / `ctl` as there.  A thread's V-wide unit j covers columns [V j, V j + V): n / V units cover the row.
template <int V>
__global__ __launch_bounds__(ZF_BLOCK) void zf_gemv_rows_f32_kernel(const zf_control* ctl, const float* __restrict__ A,
                                                                    zf_ring3 xr, zf_ring3 sr, int slot, int64_t m_rows,
                                                                    int64_t n) {
    using AT = typename zf_f32vec<V>::type;
    __shared__ double lds[ZF_WAVES * GEMV_ROWS_F32];
    int idx = 0;
    if (slot >= 0) {
        if (ctl->status != ZF_RUNNING) return;
        idx = (ctl->cur + slot) % 3;
    }
    const double* __restrict__ x = xr.p[idx];
    double* __restrict__ s = sr.p[idx];
    const int64_t nv = n / V;
    for (int64_t row0 = (int64_t)blockIdx.x * GEMV_ROWS_F32; row0 < m_rows; row0 += (int64_t)gridDim.x * GEMV_ROWS_F32) {
        double acc[GEMV_ROWS_F32];
#pragma unroll
        for (int r = 0; r < GEMV_ROWS_F32; ++r) acc[r] = 0.0;
        for (int64_t j = threadIdx.x; j < nv; j += ZF_BLOCK) {
            const zf_xvec<V> xj = zf_ld_x<V>(x, j);
#pragma unroll
            for (int r = 0; r < GEMV_ROWS_F32; ++r) {
                if (row0 + r < m_rows) {
                    const AT a = zf_ld_stream(reinterpret_cast<const AT*>(A + (row0 + r) * n) + j);
                    acc[r] += zf_dot_f32(a, xj);
                }
            }
        }
        const double maxs[1] = {0.0};
        double out = 0.0;
        zf_block_reduce<GEMV_ROWS_F32, 0, ZF_WAVES>(acc, maxs, lds, out);
        if (threadIdx.x < GEMV_ROWS_F32 && row0 + threadIdx.x < m_rows) s[row0 + threadIdx.x] = out;
        __syncthreads();
    }
}

// ---- slab[slice][j] = sum_{i in slice} A[i][j] r[i]  (column sums) ----------
// zf_gemvT_partial_kernel with float rows: grid (column panels of ZF_BLOCK * V, row slices - zf_view_slices, zf_matview.h); each
// thread owns V adjacent columns, walks its row slice with GEMVT_UNROLL loads in flight and writes V doubles of the slab
// [slices][n], which zf_gemvT_combine_kernel adds in slice order.
template <int V>
__global__ __launch_bounds__(ZF_BLOCK) void zf_gemvT_partial_f32_kernel(const zf_control* ctl, const float* __restrict__ A,
                                                                        const double* __restrict__ r,
                                                                        double* __restrict__ slab, int64_t m_rows, int64_t n,
                                                                        int64_t rows_per_slice) {
    using AT = typename zf_f32vec<V>::type;
    if (ctl && (ctl->status != ZF_RUNNING || !ctl->need_grad)) return;   // ctl == NULL: plain call
    const int64_t colv = (int64_t)blockIdx.x * ZF_BLOCK + threadIdx.x;  // V-wide unit
    const int64_t nv = n / V;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_slice;
    int64_t r1 = r0 + rows_per_slice;
    if (r1 > m_rows) r1 = m_rows;
    if (colv >= nv) return;
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0;
    const AT* __restrict__ Ac = reinterpret_cast<const AT*>(A) + colv;
    int64_t i = r0;
    for (; i + GEMVT_UNROLL <= r1; i += GEMVT_UNROLL) {
        AT a[GEMVT_UNROLL];
#pragma unroll
        for (int u = 0; u < GEMVT_UNROLL; ++u) a[u] = zf_ld_stream(Ac + (i + u) * nv);
#pragma unroll
        for (int u = 0; u < GEMVT_UNROLL; ++u) zf_fma_f32(acc, a[u], r[i + u]);
    }
    for (; i < r1; ++i) zf_fma_f32(acc, zf_ld_stream(Ac + i * nv), r[i]);
    double* out = slab + (int64_t)blockIdx.y * n + colv * V;
#pragma unroll
    for (int v = 0; v < V; ++v) out[v] = acc[v];
}

// ---- launches ---------------------------------------------------------------
// sr = A xr (slot / ctl as zf_gemv_rows_kernel) ...
static void zf_launch_rows_f32(hipStream_t st, const zf_control* ctl, const float* A32, zf_ring3 xr, zf_ring3 sr, int slot, int64_t m,
                               int64_t n) {
    int gr = (int)((m + GEMV_ROWS_F32 - 1) / GEMV_ROWS_F32);
    if (gr > 8 * ZF_MAX_GRID) gr = 8 * ZF_MAX_GRID;
    const int V = zf_f32_width(n);
    if (V == 4) hipLaunchKernelGGL(zf_gemv_rows_f32_kernel<4>, dim3(gr), dim3(ZF_BLOCK), 0, st, ctl, A32, xr, sr, slot, m, n);
    else if (V == 2) hipLaunchKernelGGL(zf_gemv_rows_f32_kernel<2>, dim3(gr), dim3(ZF_BLOCK), 0, st, ctl, A32, xr, sr, slot, m, n);
    else hipLaunchKernelGGL(zf_gemv_rows_f32_kernel<1>, dim3(gr), dim3(ZF_BLOCK), 0, st, ctl, A32, xr, sr, slot, m, n);
}
// ... and the slice partials of A^T r (slices / rows_per_slice: zf_view_slices; zf_gemvT_combine_kernel follows)
static void zf_launch_cols_f32(hipStream_t st, const zf_control* ctl, const float* A32, const double* r, double* slab, int64_t m,
                               int64_t n, int slices, int64_t rows_per_slice) {
    const int V = zf_f32_width(n);
    const dim3 gT((unsigned)((n / V + ZF_BLOCK - 1) / ZF_BLOCK), (unsigned)slices);
    if (V == 4) hipLaunchKernelGGL(zf_gemvT_partial_f32_kernel<4>, gT, dim3(ZF_BLOCK), 0, st, ctl, A32, r, slab, m, n, rows_per_slice);
    else if (V == 2) hipLaunchKernelGGL(zf_gemvT_partial_f32_kernel<2>, gT, dim3(ZF_BLOCK), 0, st, ctl, A32, r, slab, m, n, rows_per_slice);
    else hipLaunchKernelGGL(zf_gemvT_partial_f32_kernel<1>, gT, dim3(ZF_BLOCK), 0, st, ctl, A32, r, slab, m, n, rows_per_slice);
}
