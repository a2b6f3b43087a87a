"""The case table of the fp32-matrix tests (tests/test_f32_cases.py on the CPU, tests/test_gpu_f32_matrix.py on the GPU).

A dense margins problem with ``matrix_dtype="float32"`` keeps A in HBM as floats and sweeps it with
csrc/zf_kernels_gemv_f32.h: V floats per load, V = 4 when n % 4 == 0 (16-byte loads), 2 when n % 4 == 2, 1 for odd n; the
column sweep splits the rows into slices by the rule of zf_view_slices for an fp32 view (panels of 256 V columns, at most 64 slices of
at least 8 rows); the row sweep (4 rows per workgroup) loops over row groups once m > 65536; no small-matrix path.  float32 -> float64 is exact,
so such a solve is the fp64 solve on A64 = float64(float32(A)) with sums in another order: every reference here gets A64.

Matrices come from oracle.problems_ref.make_plasso and are rounded once.  A seed is part of a case (one that does not separate
gets another): the CPU test checks,
per case, that rounding A moves the oracle's iterates by far more than the tolerance of the GPU comparison - a GPU test
could not otherwise tell the fp32 path from one that silently kept fp64 A."""
import numpy as np

TOL = 1e-10
U = 2.0 ** -53

COLS_V4, COLS_V2, COLS_V1 = 6, 7, 8    # zf_solver_ls_plan out[0]: zf_gemvT_partial_f32_kernel<4>, <2>, <1>
ROWS_V4, ROWS_V2, ROWS_V1 = 4, 5, 6    # out[1]: zf_gemv_rows_f32_kernel<4>, <2>, <1>
ROW_LOOP_MIN_M = 4 * 8 * 2048          # GEMV_ROWS_F32 rows per workgroup, at most 8 * ZF_MAX_GRID workgroups: beyond, row groups loop

# (m, n), scale, seed, expected ls_plan (column form, row form, slices, rows per slice), what the case reaches
CASES = [
    ((1, 1), 0.5, 11, (COLS_V1, ROWS_V1, 1, 1), "smallest problem"),
    ((1, 7), 0.5, 11, (COLS_V1, ROWS_V1, 1, 1), "one row"),
    ((7, 1), 1 / 6, 11, (COLS_V1, ROWS_V1, 1, 7), "one column"),
    ((129, 1000), 1 / 6, 11, (COLS_V4, ROWS_V4, 17, 8), "V4, one panel with idle lanes, last slice 1 row"),
    ((3000, 4096), 0.5, 11, (COLS_V4, ROWS_V4, 64, 47), "V4, 40 unrolled + 7 tail rows per slice, last slice 39"),
    ((1200, 4002), 0.5, 11, (COLS_V2, ROWS_V2, 64, 19), "V2: n % 4 == 2, rows only 8-byte aligned; last slice 3"),
    ((1201, 4001), 0.5, 11, (COLS_V1, ROWS_V1, 64, 19), "V1, last slice 4"),
    ((70000, 4), 1 / 6, 13, (COLS_V4, ROWS_V4, 64, 1094), "V4, one unit per row, the row sweep loops, 1094 rows per slice"),
    ((70003, 33), 0.5, 11, (COLS_V1, ROWS_V1, 64, 1094), "V1, the row sweep loops (its last group: 3 of 4 rows), last slice 1081"),
    ((2, 2097184), 0.5, 11, (COLS_V4, ROWS_V4, 1, 2), "V4, one slice, tail only, 2049 column panels"),
    ((5, 4128), 0.5, 11, (COLS_V4, ROWS_V4, 1, 5), "the fp64 class takes the fused small-matrix path here; fp32 the general one"),
]


def case_id(case):
    (m, n) = case[0]
    return f"{m}x{n}"


IDS = [case_id(c) for c in CASES]
BY_SHAPE = {c[0]: c for c in CASES}


def width(n):
    return 4 if n % 4 == 0 else 2 if n % 2 == 0 else 1


def dispatch_f32(m, n):
    """zf_solver_set_matrix_f32's plan (zfista_amd/csrc: zf_view_slices in zf_matview.h, zf_solver_ls_plan), restated:
    the table above must agree."""
    V = width(n)
    panels = -(-(n // V) // 256)                 # column panels: ZF_BLOCK threads x V columns
    slices = max(1, min(-(-2048 // panels), -(-m // 8), 64))
    rps = -(-m // slices)
    slices = -(-m // rps)
    return {4: COLS_V4, 2: COLS_V2, 1: COLS_V1}[V], {4: ROWS_V4, 2: ROWS_V2, 1: ROWS_V1}[V], slices, rps


class Dense:
    """One shape's data: A as make_plasso made it, A32 = float32(A) and A64 = float64(A32), b, lam, ||A64||_2^2."""

    def __init__(self, m, n, seed):
        from oracle import problems_ref as P

        self.A, self.b, self.lam = P.make_plasso(m, n, seed=seed, n_informative=max(1, min(20, n // 4)))
        self.A32 = np.ascontiguousarray(self.A.astype(np.float32))
        self.A64 = self.A32.astype(np.float64)
        G = self.A64 @ self.A64.T if m <= n else self.A64.T @ self.A64
        self.sigma2 = float(np.linalg.eigvalsh(G)[-1])

    def L(self, scale):
        return 2 * scale * self.sigma2


def make(case):
    (m, n), _, seed, _, _ = case
    return Dense(m, n, seed)


def fista_iters(m, n):
    """30 iterations; 10 for tall A, which is well conditioned: its FISTA is at rounding level soon after, and the line
    search would then decide on rounding noise (tests/test_gpu_dense_ls_paths.py)."""
    return 30 if m <= n else 10


def fista_kw(D, m, n, scale, variant="dense"):
    """dense: lr = 1 with backtracking on small shapes (rejected trials occur), 0.9 / L on large ones (no marginal trial).
    near-lam-max: 0.9 / L and decay_rate = 1, which accepts every trial (no line search) - there f is |b|^2 / 2 up to a part
    in 1e3 or less, so the sufficient-decrease test of a short step compares differences of f far below the rounding of f and
    would decide on rounding noise (the oracle and the GPU then part ways by a halved lr, not by an error of a sweep)."""
    if variant == "near-lam-max":
        return dict(lr=0.9 / D.L(scale), decay_rate=1, nesterov=True, tol=0.0, max_iter=fista_iters(m, n), return_all=True)
    lr = 1.0 if m * n <= 1 << 18 else 0.9 / D.L(scale)
    return dict(lr=lr, nesterov=True, tol=0.0, max_iter=fista_iters(m, n), return_all=True)


def fista_x0(m, n):
    return 0.1 * np.random.default_rng(n * 31 + m).standard_normal(n)


# The short FISTA solve runs in two variants.
#   "dense":       x0 random, lam = make_plasso's (0.1 max |A^T b|): dense iterates, every column of A takes part in A x.  But
#                  rounding A to fp32 (relative error <= 2^-24 per element, random in sign, averaged over a row or a column by
#                  every sum) moves these iterates by only 4e-11 ... 1e-8 relative (measured on the CPU oracle, per shape) -
#                  from 0.4 to 100 times TOL: this variant alone could not tell fp32 storage from fp64 storage.
#   "near-lam-max": x0 = 0, no line search, lam = NEAR_LAM_MAX * lam_max with lam_max = 2 scale max |A^T b|: the soft threshold takes the
#                  difference of two nearly equal numbers, so a relative change e of A^T b becomes e / (1 - NEAR_LAM_MAX) in the
#                  iterate: the variant in which rounding is material (tests/test_f32_cases.py asserts > 1e3 TOL per case).
NEAR_LAM_MAX = 0.999
VARIANTS = ("near-lam-max", "dense")


def fista_problem(D, m, n, scale, variant):
    """(lam, x0) of a variant; lam_max is taken on the unrounded A, so both sides of a rounding comparison get one lam."""
    if variant == "dense":
        return D.lam, fista_x0(m, n)
    return NEAR_LAM_MAX * 2 * scale * float(np.max(np.abs(D.A.T @ D.b))), np.zeros(n)
