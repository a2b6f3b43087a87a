// zf_spmv.hip - instantiations of the CSR row-sum kernels (zf_kernels_spmv.h) and the matrix handle of the C ABI
#include <new>
#include <vector>

#include "zf_kernels_spmv.h"

void zf_launch_spmv(const zf_spmv_mat& M, hipStream_t st, const zf_control* ctl, bool grad_guard, const zf_spmv_io& io, int slot,
                    double out_scale, double* partial) {
    const int rpb = ZF_BLOCK / M.lanes;
    int64_t row_blocks = (M.rows + rpb - 1) / rpb;
    if (row_blocks > ZF_SPMV_MAX_ROW_BLOCKS) row_blocks = ZF_SPMV_MAX_ROW_BLOCKS;
    const int64_t seg_blocks = (M.nseg + ZF_WAVES - 1) / ZF_WAVES;
    const dim3 grid((unsigned)(row_blocks + seg_blocks)), block(ZF_BLOCK);
    const int g = grad_guard ? 1 : 0, rb = (int)row_blocks;
    switch (M.lanes) {
        case 4: hipLaunchKernelGGL(zf_spmv_rows_kernel<4>, grid, block, 0, st, M, ctl, g, io, slot, out_scale, rb, partial); break;
        case 8: hipLaunchKernelGGL(zf_spmv_rows_kernel<8>, grid, block, 0, st, M, ctl, g, io, slot, out_scale, rb, partial); break;
        case 16: hipLaunchKernelGGL(zf_spmv_rows_kernel<16>, grid, block, 0, st, M, ctl, g, io, slot, out_scale, rb, partial); break;
        case 32: hipLaunchKernelGGL(zf_spmv_rows_kernel<32>, grid, block, 0, st, M, ctl, g, io, slot, out_scale, rb, partial); break;
        default: hipLaunchKernelGGL(zf_spmv_rows_kernel<64>, grid, block, 0, st, M, ctl, g, io, slot, out_scale, rb, partial); break;
    }
    if (M.nsplit > 0)
        hipLaunchKernelGGL(zf_spmv_tail_kernel, dim3(zf_grid_for(M.nsplit)), block, 0, st, M, ctl, g, io, slot, out_scale, partial);
}

// ---- residuals of long vectors (zf_kernels_spmv.h) -----------------------------------------------------------------
int zf_spmv_resid_chunks(int64_t m) {
    int64_t chunks = (m + 1023) / 1024;
    if (chunks < 1) chunks = 1;
    if (chunks > ZF_SPMV_RESID_MAX_CHUNKS) chunks = ZF_SPMV_RESID_MAX_CHUNKS;
    return (int)chunks;
}

// the workgroup's sum: wave trees, then the four wave sums in wave order (thread 0 holds it)
__device__ __forceinline__ double zf_spmv_block_sum(double acc, double* lds) {
    acc = zf_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    double t = lds[0];
    for (int w = 1; w < ZF_WAVES; ++w) t += lds[w];
    return t;
}

// WHICH: 0 = r = (s_k + beta (s_k - s_{k-1})) - b at y, stored, only when the gradient is due; 1 = s[(cur + slot) % 3] - b
template <int WHICH>
__global__ __launch_bounds__(ZF_BLOCK) void zf_spmv_resid_kernel(const zf_control* ctl, const double* s0, const double* s1, const double* s2,
                                                                 int slot, const double* __restrict__ b, double* __restrict__ r, int64_t m,
                                                                 int nesterov, double* __restrict__ part) {
    __shared__ double lds[ZF_WAVES];
    if (ctl->status != ZF_RUNNING) return;
    if (WHICH == 0 && !ctl->need_grad) return;
    const double* sr[3] = {s0, s1, s2};
    const int cur = ctl->cur;
    const int64_t per = (m + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < m ? lo + per : m;
    double acc = 0.0;
    if (WHICH == 0) {
        const double beta = nesterov ? ctl->beta_next : 0.0;
        const double* __restrict__ sk = cur == 0 ? sr[0] : cur == 1 ? sr[1] : sr[2];
        const int o = (cur + 2) % 3;
        const double* __restrict__ so = o == 0 ? sr[0] : o == 1 ? sr[1] : sr[2];
        for (int64_t i = lo + threadIdx.x; i < hi; i += ZF_BLOCK) {
            double ay = sk[i];
            if (nesterov) ay = ay + beta * (ay - so[i]);
            const double rv = ay - b[i];
            r[i] = rv;
            acc += rv * rv;
        }
    } else {
        const int k = (cur + slot) % 3;
        const double* __restrict__ sv = k == 0 ? sr[0] : k == 1 ? sr[1] : sr[2];
        for (int64_t i = lo + threadIdx.x; i < hi; i += ZF_BLOCK) {
            const double rv = sv[i] - b[i];
            acc += rv * rv;
        }
    }
    const double t = zf_spmv_block_sum(acc, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// f = scale * sqrt(part[0] + part[1] + ...)^2: thread t adds chunks t, t + 256, ... in that order, then the block sum
__global__ __launch_bounds__(ZF_BLOCK) void zf_spmv_resid_finish_kernel(const zf_control* ctl, int grad_guard, const double* __restrict__ part,
                                                                        int count, double scale, double* f_out) {
    __shared__ double lds[ZF_WAVES];
    if (ctl->status != ZF_RUNNING) return;
    if (grad_guard && !ctl->need_grad) return;
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += ZF_BLOCK) acc += part[i];
    const double t = zf_spmv_block_sum(acc, lds);
    if (threadIdx.x == 0) {
        const double nrm = sqrt(t);
        *f_out = scale * (nrm * nrm);
    }
}

void zf_launch_spmv_resid_y(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2, const double* b,
                            double* r, double scale, int64_t m, int nesterov, double* part, double* f_out) {
    const int chunks = zf_spmv_resid_chunks(m);
    hipLaunchKernelGGL(zf_spmv_resid_kernel<0>, dim3(chunks), dim3(ZF_BLOCK), 0, st, ctl, s0, s1, s2, 0, b, r, m, nesterov, part);
    hipLaunchKernelGGL(zf_spmv_resid_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ctl, 1, part, chunks, scale, f_out);
}

void zf_launch_spmv_resid_x(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2, int slot,
                            const double* b, double scale, int64_t m, double* part, double* f_out) {
    const int chunks = zf_spmv_resid_chunks(m);
    hipLaunchKernelGGL(zf_spmv_resid_kernel<1>, dim3(chunks), dim3(ZF_BLOCK), 0, st, ctl, s0, s1, s2, slot, b, nullptr, m, 0, part);
    hipLaunchKernelGGL(zf_spmv_resid_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, ctl, 0, part, chunks, scale, f_out);
}

// ZF_ACCEPT_REMAINDER (zf_spmv.h): zf_spmv_resid_kernel<1>'s chunk sums of (s+ - b)^2 and, beside them, those of (s+ - s_y)^2
__global__ __launch_bounds__(ZF_BLOCK) void zf_spmv_resid_rem_kernel(const zf_control* ctl, const double* s0, const double* s1, const double* s2,
                                                                     int slot, const double* __restrict__ b, int64_t m, int nesterov,
                                                                     double beta_plain, double* __restrict__ part, double* __restrict__ part_r) {
    __shared__ double lds[ZF_WAVES];
    __shared__ double lds_r[ZF_WAVES];
    const double* sr[3] = {s0, s1, s2};
    int ip = 0, ik = 1, io = 2;
    double beta = nesterov ? beta_plain : 0.0;
    if (slot >= 0) {
        if (ctl->status != ZF_RUNNING) return;
        const int cur = ctl->cur;
        ip = (cur + slot) % 3;
        ik = cur;
        io = (cur + 2) % 3;
        beta = nesterov ? ctl->beta_next : 0.0;
    }
    const double* __restrict__ sv = ip == 0 ? sr[0] : ip == 1 ? sr[1] : sr[2];
    const double* __restrict__ sk = ik == 0 ? sr[0] : ik == 1 ? sr[1] : sr[2];
    const double* __restrict__ so = io == 0 ? sr[0] : io == 1 ? sr[1] : sr[2];
    const int64_t per = (m + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < m ? lo + per : m;
    double acc = 0.0, acc_r = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += ZF_BLOCK) {
        const double sp = sv[i];
        const double rv = sp - b[i];
        acc += rv * rv;
        double ay = sk[i];
        if (nesterov) ay = ay + beta * (ay - so[i]);
        const double dv = sp - ay;
        acc_r += dv * dv;
    }
    const double t = zf_spmv_block_sum(acc, lds);
    const double tr = zf_spmv_block_sum(acc_r, lds_r);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = t;
        part_r[blockIdx.x] = tr;
    }
}

// both chunk sums in zf_spmv_resid_finish_kernel's order: f = scale * sqrt(sum part)^2, R = scale * sum part_r
__global__ __launch_bounds__(ZF_BLOCK) void zf_spmv_resid_rem_finish_kernel(const zf_control* ctl, const double* __restrict__ part,
                                                                            const double* __restrict__ part_r, int count, double scale,
                                                                            double* f_out, double* r_out) {
    __shared__ double lds[ZF_WAVES];
    __shared__ double lds_r[ZF_WAVES];
    if (ctl && ctl->status != ZF_RUNNING) return;
    double acc = 0.0, acc_r = 0.0;
    for (int i = threadIdx.x; i < count; i += ZF_BLOCK) {
        acc += part[i];
        acc_r += part_r[i];
    }
    const double t = zf_spmv_block_sum(acc, lds);
    const double tr = zf_spmv_block_sum(acc_r, lds_r);
    if (threadIdx.x == 0) {
        const double nrm = sqrt(t);
        *f_out = scale * (nrm * nrm);
        *r_out = scale * tr;
    }
}

void zf_launch_spmv_resid_x_rem(hipStream_t st, const zf_control* ctl, const double* s0, const double* s1, const double* s2, int slot,
                                const double* b, double scale, int64_t m, int nesterov, double beta_plain, double* part, double* part_r,
                                double* f_out, double* r_out) {
    const int chunks = zf_spmv_resid_chunks(m);
    hipLaunchKernelGGL(zf_spmv_resid_rem_kernel, dim3(chunks), dim3(ZF_BLOCK), 0, st, ctl, s0, s1, s2, slot, b, m, nesterov, beta_plain, part,
                       part_r);
    hipLaunchKernelGGL(zf_spmv_resid_rem_finish_kernel, dim3(1), dim3(ZF_BLOCK), 0, st, slot >= 0 ? ctl : nullptr, part, part_r, chunks, scale,
                       f_out, r_out);
}

// ---- the matrix handle ---------------------------------------------------------------------------------------------
static int zf_spmat_free(zf_spmat* h) {
    for (int k = 0; k < h->n_owned; ++k)
        if (h->owned[k]) (void)hipFree(h->owned[k]);
    delete h;
    return ZF_OK;
}

// the plan of one matrix: checked on the host against the sizes AND against the row pointers (one copy of indptr to the
// host: the rows kernel decides "split" from indptr itself and leaves those rows to the plan's segments - the two must name
// the same rows, and a row's segments must start with the row), then uploaded
static int zf_spmat_plan(zf_spmat* h, zf_spmv_mat* M, int64_t rows, int64_t cols, int64_t nnz, const int64_t* indptr_dev,
                         const int32_t* indices_dev, const double* values_dev, const zf_spmv_plan* p) {
    ZF_REQUIRE(p->lanes == 4 || p->lanes == 8 || p->lanes == 16 || p->lanes == 32 || p->lanes == 64,
               "zf_spmat_create: lanes per row must be a power of two from 4 to 64");
    ZF_REQUIRE(p->threshold >= 1, "zf_spmat_create: the split threshold must be >= 1");
    ZF_REQUIRE(p->nsplit >= 0 && p->nsplit <= rows && p->nseg >= 2 * p->nsplit && p->nseg <= nnz,
               "zf_spmat_create: bad number of split rows or segments");
    ZF_REQUIRE(p->nsplit == 0 ? p->nseg == 0 : (p->split_row && p->split_first && p->seg_start),
               "zf_spmat_create: a plan with split rows needs split_row, split_first and seg_start");
    std::vector<int64_t> indptr((size_t)rows + 1);
    ZF_HIP(hipMemcpy(indptr.data(), indptr_dev, sizeof(int64_t) * (rows + 1), hipMemcpyDeviceToHost));
    ZF_REQUIRE(indptr[0] == 0 && indptr[(size_t)rows] == nnz, "zf_spmat_create: indptr must start at 0 and end at nnz");
    int64_t longer = 0;
    for (int64_t i = 0; i < rows; ++i) {
        ZF_REQUIRE(indptr[(size_t)i + 1] >= indptr[(size_t)i], "zf_spmat_create: indptr must not decrease");
        if (indptr[(size_t)i + 1] - indptr[(size_t)i] > p->threshold) longer += 1;
    }
    ZF_REQUIRE(longer == p->nsplit, "zf_spmat_create: split_row must list exactly the rows longer than the threshold");
    std::vector<int64_t> seg_row((size_t)p->nseg);
    for (int64_t j = 0; j < p->nsplit; ++j) {
        const int64_t s0 = p->split_first[j], s1 = p->split_first[j + 1];
        ZF_REQUIRE(p->split_row[j] >= 0 && p->split_row[j] < rows && (j == 0 || p->split_row[j] > p->split_row[j - 1]),
                   "zf_spmat_create: split rows must be increasing row numbers");
        ZF_REQUIRE((j == 0 ? s0 == 0 : true) && s1 >= s0 + 2 && s1 <= p->nseg, "zf_spmat_create: split_first must start at 0 and give every split row two segments or more");
        {
            const int64_t lo = indptr[(size_t)p->split_row[j]], len = indptr[(size_t)p->split_row[j] + 1] - lo;
            ZF_REQUIRE(len > p->threshold, "zf_spmat_create: split_row names a row that is not longer than the threshold");
            ZF_REQUIRE(p->seg_start[s0] == lo && s1 - s0 == (len + p->threshold - 1) / p->threshold,
                       "zf_spmat_create: the segments of a split row must start with the row and cover it");
        }
        for (int64_t s = s0; s < s1; ++s) {
            ZF_REQUIRE(p->seg_start[s] >= 0 && p->seg_start[s] < nnz && (s == 0 || p->seg_start[s] > p->seg_start[s - 1]),
                       "zf_spmat_create: segment starts must be increasing element numbers below nnz");
            ZF_REQUIRE(s == s0 || p->seg_start[s] == p->seg_start[s - 1] + p->threshold,
                       "zf_spmat_create: the segments of a row must be `threshold` elements apart");
            seg_row[(size_t)s] = p->split_row[j];
        }
    }
    ZF_REQUIRE(p->nsplit == 0 || p->split_first[p->nsplit] == p->nseg, "zf_spmat_create: split_first must end at nseg");
    M->indptr = indptr_dev;
    M->indices = indices_dev;
    M->values = values_dev;
    M->rows = rows;
    M->cols = cols;
    M->nnz = nnz;
    M->lanes = p->lanes;
    M->threshold = p->threshold;
    M->nsplit = p->nsplit;
    M->nseg = p->nseg;
    M->split_row = M->split_first = M->seg_start = M->seg_row = nullptr;
    if (p->nsplit == 0) return ZF_OK;
    const struct {
        const int64_t* host;
        int64_t count;
        const int64_t** dev;
    } up[4] = {{p->split_row, p->nsplit, &M->split_row},
               {p->split_first, p->nsplit + 1, &M->split_first},
               {p->seg_start, p->nseg, &M->seg_start},
               {seg_row.data(), p->nseg, &M->seg_row}};
    for (const auto& u : up) {
        void* d = nullptr;
        ZF_HIP(hipMalloc(&d, sizeof(int64_t) * u.count));
        h->owned[h->n_owned++] = d;
        ZF_HIP(hipMemcpy(d, u.host, sizeof(int64_t) * u.count, hipMemcpyHostToDevice));
        *u.dev = static_cast<const int64_t*>(d);
    }
    return ZF_OK;
}

extern "C" int zf_spmat_create(zf_spmat** out, int64_t m, int64_t n, int64_t nnz, const int64_t* indptr_dev, const int32_t* indices_dev,
                               const double* values_dev, const zf_spmv_plan* plan, const int64_t* t_indptr_dev, const int32_t* t_indices_dev,
                               const double* t_values_dev, const zf_spmv_plan* t_plan, int64_t plan_bytes) {
    ZF_REQUIRE(out && plan && t_plan && indptr_dev && t_indptr_dev, "zf_spmat_create: null argument");
    ZF_REQUIRE(plan_bytes == (int64_t)sizeof(zf_spmv_plan), "zf_spmat_create: plan_bytes differs from sizeof(zf_spmv_plan)");
    ZF_REQUIRE(m >= 1 && n >= 1 && m <= 0x7fffffffLL && n <= 0x7fffffffLL && nnz >= 0,
               "zf_spmat_create: m and n must be in [1, 2^31) (32-bit column indices) and nnz >= 0");
    ZF_REQUIRE(nnz == 0 || (indices_dev && values_dev && t_indices_dev && t_values_dev), "zf_spmat_create: indices and values are required when nnz > 0");
    zf_spmat* h = new (std::nothrow) zf_spmat();
    if (!h) return zf_fail(ZF_ERR_ARG, "zf_spmat_create: out of host memory");
    h->m = m;
    h->n = n;
    h->nnz = nnz;
    h->n_owned = 0;
    int rc = zf_spmat_plan(h, &h->A, m, n, nnz, indptr_dev, indices_dev, values_dev, plan);
    if (rc == ZF_OK) rc = zf_spmat_plan(h, &h->At, n, m, nnz, t_indptr_dev, t_indices_dev, t_values_dev, t_plan);
    if (rc != ZF_OK) {
        zf_spmat_free(h);
        return rc;
    }
    *out = h;
    return ZF_OK;
}

extern "C" int zf_spmat_destroy(zf_spmat* h) {
    if (!h) return ZF_OK;
    (void)hipDeviceSynchronize();
    return zf_spmat_free(h);
}
