// zf_kernels_mr.h - the two dense fp64 sweeps of zf_kernels_gemv.h for K responses at once (zf_solver_set_responses):
//   S[i][k] = sum_j A[i][j] X[j][k]  (rows)   and   slab[slice][j][k] = sum_{i in slice} A[i][j] R[i][k]  (columns),
// A row-major m x n doubles in HBM, read ONCE per sweep whatever K is.  Every vector is response-interleaved -
// x[j K + k] = X[j][k], s[i K + k] = S[i][k], the C order of the caller's 2-D arrays - so the problem is the margins problem
// of A (x) I_K and everything element-wise around the sweeps (loss kernels, prox step, certificate passes) runs unchanged on
// vectors of m K and n K entries.
// K = 2 .. 16 is a template parameter (one instantiation per K: every loop over k unrolls, no padded response is computed);
// V = 2 (16-byte nontemporal loads of A, even n) or 1 (odd n: rows are not 16-byte aligned).
// Every sum has an order fixed by (m, n, K); the operations of response k are those of every other response on its own
// operands, so equal columns of X / R give bit-equal columns of S / the slab.  No atomics, fused multiply-adds throughout
// (__builtin_fma: the build runs with -ffp-contract=off).
#pragma once
#include "zf_kernels_gemv.h"

constexpr int ZF_MR_MAX_K = 16;

// ---- S = A X  (row dot products) -------------------------------------------------------------
// A workgroup of MR_ROWS_BLOCK threads (8 waves) owns 8 RT consecutive rows: wave w the RT rows from row0 + w RT, its lanes
// the V-wide column units of a chunk of 64 V columns.  The chunk's X values - 64 V K doubles - are staged ONCE per workgroup
// in LDS, transposed to xs[k][column] (row stride 64 V + 2: the transposing stores of consecutive k land in different banks;
// the reads of consecutive lanes are consecutive doubles), so a workgroup reads X once from L2 / Infinity Cache:
//   X bytes / A bytes = K / (8 RT),  RT = 2 (K <= 8), 3 (K <= 12), 4 (K <= 16)  ->  at most 1/2 for every K.
// Register tile of a lane: RT rows x V columns of A (and the next chunk's, loaded before the current one is used: the loads
// stay in flight across the barriers) against RT x K accumulators (at most 64 doubles).  The RT K sums of a wave are
// wave-reduced by the butterfly of zf_wave_sum; lane 0 stores them.  `slot` / `ctl` as zf_gemv_rows_kernel.
constexpr int MR_ROWS_BLOCK = 512;
constexpr int MR_ROWS_WAVES = MR_ROWS_BLOCK / 64;
constexpr int zf_mr_rt(int K) { return K <= 8 ? 2 : K <= 12 ? 3 : 4; }
static inline int zf_mr_rows_per_wg(int K) { return MR_ROWS_WAVES * zf_mr_rt(K); }

template <int K, int V>
__global__ __launch_bounds__(MR_ROWS_BLOCK) void zf_mr_rows_kernel(const zf_control* ctl, const double* __restrict__ A,
                                                                   zf_ring3 xr, zf_ring3 sr, int slot, int64_t m_rows,
                                                                   int64_t n) {
    using RT_ = typename zf_rowvec<V>::type;
    constexpr int RT = zf_mr_rt(K);
    constexpr int CH = 64 * V;      // columns per chunk
    constexpr int LD = CH + 2;      // row stride of the staged chunk
    __shared__ double xs[K * LD];
    int idx = 0;
    if (slot >= 0) {
        if (ctl->status != ZF_RUNNING) return;
        idx = (ctl->cur + slot) % 3;
    }
    const double* __restrict__ x = xr.p[idx];
    double* __restrict__ s = sr.p[idx];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane * V;       // first column of this lane's unit inside a chunk
    for (int64_t row0 = (int64_t)blockIdx.x * (MR_ROWS_WAVES * RT); row0 < m_rows;
         row0 += (int64_t)gridDim.x * (MR_ROWS_WAVES * RT)) {
        const int64_t rw = row0 + wave * RT;
        double acc[RT][K];
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int k = 0; k < K; ++k) acc[r][k] = 0.0;
        double a_cur[RT][V], a_nxt[RT][V];
        // (n % V == 0 and every chunk starts at a multiple of V: a unit is inside the row or outside it as a whole)
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            RT_ a = {};
            if (rw + r < m_rows && col < n) a = zf_ld_stream(reinterpret_cast<const RT_*>(A + (rw + r) * n + col));
            if constexpr (V == 2) { a_cur[r][0] = a.x; a_cur[r][1] = a.y; } else { a_cur[r][0] = a; }
        }
        for (int64_t c0 = 0; c0 < n; c0 += CH) {
            const int64_t cw = n - c0 < CH ? n - c0 : CH;   // columns of this chunk
            __syncthreads();   // the chunk before has been read by every wave
            for (int64_t e = threadIdx.x; e < cw * K; e += MR_ROWS_BLOCK) xs[(e % K) * LD + e / K] = x[c0 * K + e];
            __syncthreads();
            const int64_t cn = c0 + CH + col;   // this lane's unit of the next chunk
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                RT_ a = {};
                if (rw + r < m_rows && cn < n) a = zf_ld_stream(reinterpret_cast<const RT_*>(A + (rw + r) * n + cn));
                if constexpr (V == 2) { a_nxt[r][0] = a.x; a_nxt[r][1] = a.y; } else { a_nxt[r][0] = a; }
            }
            if (col < cw) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const double xv = xs[k * LD + col + v];
#pragma unroll
                        for (int r = 0; r < RT; ++r) acc[r][k] = __builtin_fma(a_cur[r][v], xv, acc[r][k]);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int v = 0; v < V; ++v) a_cur[r][v] = a_nxt[r][v];
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double t = zf_wave_sum(acc[r][k]);
                if (lane == 0 && rw + r < m_rows) s[(rw + r) * K + k] = t;
            }
        }
    }
}

// ---- slab[slice][j][k] = sum_{i in slice} A[i][j] R[i][k]  (column sums) ------------------------
// zf_gemvT_partial_kernel with K right-hand sides: grid (column panels of ZF_BLOCK V columns, row slices); a thread owns V
// adjacent columns and V K accumulators, walks its row slice with MR_COLS_UNROLL loads of A in flight and multiplies each
// element into the K values of that row of R - the same K addresses for every lane, so they are read through the scalar
// cache.  The slab is [slices][n K] in the interleaved layout; zf_gemvT_combine_kernel adds it in slice order over n K entries.
constexpr int MR_COLS_UNROLL = 4;
template <int K, int V>
__global__ __launch_bounds__(ZF_BLOCK) void zf_mr_cols_partial_kernel(const zf_control* ctl, const double* __restrict__ A,
                                                                      const double* __restrict__ r,
                                                                      double* __restrict__ slab, int64_t m_rows, int64_t n,
                                                                      int64_t rows_per_slice) {
    using RT_ = typename zf_rowvec<V>::type;
    if (ctl && (ctl->status != ZF_RUNNING || !ctl->need_grad)) return;   // ctl == NULL: plain call
    const int64_t colv = (int64_t)blockIdx.x * ZF_BLOCK + threadIdx.x;  // V-wide unit
    const int64_t nv = n / V;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_slice;
    int64_t r1 = r0 + rows_per_slice;
    if (r1 > m_rows) r1 = m_rows;
    if (colv >= nv) return;
    double acc[V][K];
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[v][k] = 0.0;
    const RT_* __restrict__ Ac = reinterpret_cast<const RT_*>(A) + colv;
    int64_t i = r0;
    for (; i + MR_COLS_UNROLL <= r1; i += MR_COLS_UNROLL) {
        double a[MR_COLS_UNROLL][V];
#pragma unroll
        for (int u = 0; u < MR_COLS_UNROLL; ++u) {
            const RT_ t = zf_ld_stream(Ac + (i + u) * nv);
            if constexpr (V == 2) { a[u][0] = t.x; a[u][1] = t.y; } else { a[u][0] = t; }
        }
#pragma unroll
        for (int u = 0; u < MR_COLS_UNROLL; ++u)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double rv = r[(i + u) * K + k];
#pragma unroll
                for (int v = 0; v < V; ++v) acc[v][k] = __builtin_fma(a[u][v], rv, acc[v][k]);
            }
    }
    for (; i < r1; ++i) {   // fewer than MR_COLS_UNROLL rows left in the slice
        const RT_ t = zf_ld_stream(Ac + i * nv);
        double a[V];
        if constexpr (V == 2) { a[0] = t.x; a[1] = t.y; } else { a[0] = t; }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double rv = r[i * K + k];
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v][k] = __builtin_fma(a[v], rv, acc[v][k]);
        }
    }
    double* out = slab + ((int64_t)blockIdx.y * n + colv * V) * K;
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int k = 0; k < K; ++k) out[v * K + k] = acc[v][k];
}

// ---- launches -------------------------------------------------------------------------------
template <int K>
static void zf_mr_rows_k(hipStream_t st, const zf_control* ctl, const double* A, zf_ring3 xr, zf_ring3 sr, int slot, int64_t m, int64_t n) {
    const int per = zf_mr_rows_per_wg(K);
    int64_t gr = (m + per - 1) / per;
    if (gr > ZF_MAX_GRID) gr = ZF_MAX_GRID;   // (beyond: row groups in a grid-stride loop)
    if (n % 2 == 0)
        hipLaunchKernelGGL((zf_mr_rows_kernel<K, 2>), dim3((unsigned)gr), dim3(MR_ROWS_BLOCK), 0, st, ctl, A, xr, sr, slot, m, n);
    else
        hipLaunchKernelGGL((zf_mr_rows_kernel<K, 1>), dim3((unsigned)gr), dim3(MR_ROWS_BLOCK), 0, st, ctl, A, xr, sr, slot, m, n);
}

template <int K>
static void zf_mr_cols_k(hipStream_t st, const zf_control* ctl, const double* A, const double* r, double* slab, int64_t m, int64_t n,
                         int slices, int64_t rows_per_slice) {
    const int V = (n % 2 == 0) ? 2 : 1;
    const dim3 g((unsigned)((n / V + ZF_BLOCK - 1) / ZF_BLOCK), (unsigned)slices);
    if (V == 2)
        hipLaunchKernelGGL((zf_mr_cols_partial_kernel<K, 2>), g, dim3(ZF_BLOCK), 0, st, ctl, A, r, slab, m, n, rows_per_slice);
    else
        hipLaunchKernelGGL((zf_mr_cols_partial_kernel<K, 1>), g, dim3(ZF_BLOCK), 0, st, ctl, A, r, slab, m, n, rows_per_slice);
}

#define ZF_MR_EACH_K(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

// sr = A xr for K responses (m x n: the matrix; the vectors hold n K and m K doubles); slot / ctl as zf_gemv_rows_kernel
static void zf_launch_mr_rows(hipStream_t st, const zf_control* ctl, const double* A, zf_ring3 xr, zf_ring3 sr, int slot, int64_t m, int64_t n,
                       int K) {
    switch (K) {
#define ZF_MR_CASE(k) case k: zf_mr_rows_k<k>(st, ctl, A, xr, sr, slot, m, n); break;
        ZF_MR_EACH_K(ZF_MR_CASE)
#undef ZF_MR_CASE
        default: break;   // (zf_solver_set_responses and the entry points admit 2 .. 16 only)
    }
}

// the slice partials of A^T R (zf_gemvT_combine_kernel over n K entries follows)
static void zf_launch_mr_cols(hipStream_t st, const zf_control* ctl, const double* A, const double* r, double* slab, int64_t m, int64_t n, int K,
                       int slices, int64_t rows_per_slice) {
    switch (K) {
#define ZF_MR_CASE(k) case k: zf_mr_cols_k<k>(st, ctl, A, r, slab, m, n, slices, rows_per_slice); break;
        ZF_MR_EACH_K(ZF_MR_CASE)
#undef ZF_MR_CASE
        default: break;
    }
}
