"""Seeded option sweep of the four dense margins classes with the matrix stored in fp32 (``matrix_dtype="float32"``,
``with_matrix_dtype``): the case table shared by tests/test_f32_fuzz_cases.py (CPU: the table is sound) and
tests/test_gpu_fuzz_f32.py (GPU: the fp32 classes against the oracle on it).  No test in here.

Built on tests/margins_fuzz_ext_cases.py (``X``), imported and not copied: a case is (loss, seed) over X.LOSSES; factor kind,
weights kind, l2, box, deprecated, decay rate and run kind are X.layout's; scale, start and solver options are X.draw's (the
same seed bases: a case here and the case of X with its seed differ in the matrix only); the oracle, the stagnation cut, the
second evaluation and the acceptance criteria are X.oracle, X.other_form and X.accepted with ``cases=`` this module.

What differs:

  shapes   X's six with two swapped, so that every load width of csrc/zf_kernels_gemv_f32.h occurs and V2 twice - the index
           into SHAPES is X's, so the layout stays a bijection of shape and factor kind on 24 seeds:
             300 x 1000     V4 (n % 4 == 0: four floats per load)
             1000 x 257     V1 (odd n)
             64 x 4098      V2 (n % 4 == 2: two floats per load), in place of 64 x 4099 - same density and seed
             48 x 96        V4; the fp64 class would take the fused small-matrix form here, fp32 has none
             4097 x 66      V2, in place of 4097 x 64 - same density and seed
             40000 x 500    V4; the loss kernels in their many-workgroup shape (m > 32768), 64 slices in the column sweep
  matrix   float32 -> float64 is exact and the fp32 sweeps compute in fp64, so an fp32 solve is the fp64 solve on
           A64 = float64(float32(A)) with sums in another order (tests/f32_cases.py).  ``build`` therefore gives the case the
           CSR form of A64 - every closure of the oracle is X.ExtRef over it, the second evaluation over the dense A64 with the
           rows of (A64, b, w) reversed - while ``make_problem`` hands the library the dense matrix AS GENERATED (unrounded
           fp64): the library rounds.  b, lam and delta are those of the unrounded problem.
  storage  only the dense fp32 form runs on the GPU; CSR is not part of this table.

The device problem.  HuberL1, LeastSquaresL1 and PoissonL1 take ``matrix_dtype="float32"`` with l2, weights and factors as
keywords.  LogisticL1 is built in fp64 and takes ``with_matrix_dtype("float32")`` - after its other siblings (with_penalty,
with_sample_weight, with_penalty_factor) on even seeds, before them on odd ones.

PLANS restates zf_solver_ls_plan for the six shapes (column form, row form, slices, rows per slice);
tests/test_f32_fuzz_cases.py proves it against f32_cases.dispatch_f32."""
import functools
import sys

import numpy as np
import scipy.sparse as sp

import f32_cases as F
import margins_fuzz_ext_cases as X
from margins_fuzz_ext_cases import FACTORS, LOSSES, WEIGHTS, Case, Spec, disagreement, ending, outside_box, run_ref   # noqa: F401

V2_WIDE = (64, 4098, 0.03, 4)      # in place of X.SHAPES[2] = (64, 4099, 0.03, 4)
V2_TALL = (4097, 66, 0.05, 6)      # in place of X.SHAPES[4] = (4097, 64, 0.05, 6)
SHAPES = [X.SHAPES[0], X.SHAPES[1], V2_WIDE, X.SHAPES[3], V2_TALL, X.SHAPES[5]]
FORMS = ("dense",)
BLOCK = X.BLOCK
# zf_solver_ls_plan of an fp32 view, by (m, n): (column form, row form, slices, rows per slice)
PLANS = {
    (300, 1000): (F.COLS_V4, F.ROWS_V4, 38, 8),
    (1000, 257): (F.COLS_V1, F.ROWS_V1, 63, 16),
    (64, 4098): (F.COLS_V2, F.ROWS_V2, 8, 8),
    (48, 96): (F.COLS_V4, F.ROWS_V4, 6, 8),
    (4097, 66): (F.COLS_V2, F.ROWS_V2, 64, 65),
    (40000, 500): (F.COLS_V4, F.ROWS_V4, 64, 625),
}
FORM_NAMES = {F.COLS_V4: "f32v4", F.COLS_V2: "f32v2", F.COLS_V1: "f32v1"}

# The fixed table: the first BLOCK seeds per loss, counted from 0, that tests/test_f32_fuzz_cases.py accepts (X.accepted's
# criteria on A64).  A seed is replaced only for failing that CPU test - never for anything seen on a GPU.  REPLACED maps each
# replaced seed to what X.accepted said of it.  211 seeds were examined and 19 replaced (square 2 of 50, logistic 9 of 57, huber 6
# of 54, poisson 2 of 50: each inside the cap of one in four).  None of the 19 was decided differently by the two CPU
# evaluations: 18 have one iterate that differs by 3.1e-15 .. 1.1e-13 of its norm between the two, beyond the 3e-15 the table
# asks for, and Poisson's seed 12 loses its run to the stagnation cut at x0 (as in X).  Fifteen of the 19 are replaced in X too.
REPLACED = {
    "square": {10: "iterate 1: 3.78e-15", 22: "iterate 1: 4.17e-15"},
    "logistic": {6: "iterate 6: 4.49e-15", 12: "iterate 7: 3.13e-15", 22: "iterate 3: 9.26e-15", 25: "iterate 4: 1.05e-13",
                 28: "iterate 2: 6.17e-15", 37: "iterate 11: 4.1e-15", 39: "iterate 1: 4.81e-15", 49: "iterate 21: 3.08e-15",
                 51: "iterate 1: 3.58e-15"},
    "huber": {2: "iterate 9: 1.85e-14", 12: "iterate 2: 3.18e-15", 18: "iterate 10: 1.99e-14", 22: "iterate 2: 6.51e-15",
              28: "iterate 1: 1.09e-14", 51: "iterate 1: 3.23e-15"},
    "poisson": {12: "no run left", 25: "iterate 1: 8.48e-15"},
}
EXAMINED = {loss: BLOCK + len(REPLACED[loss]) for loss in LOSSES}
SEEDS = {loss: [s for s in range(EXAMINED[loss]) if s not in REPLACED[loss]] for loss in LOSSES}
TABLE = [(loss, seed) for loss in LOSSES for seed in SEEDS[loss]]


def layout(seed):
    """X.layout with this module's shape at X's index."""
    lay = X.layout(seed)
    return dict(lay, shape=SHAPES[X.SHAPES.index(lay["shape"])])


def draw(loss, seed):
    """X.draw's case (layout, scale, start, options) on this module's shape."""
    spec = X.draw(loss, seed)
    return spec._replace(shape=SHAPES[X.SHAPES.index(spec.shape)])


def width(spec):
    return F.width(spec.shape[1])


def plan(spec):
    return PLANS[spec.shape[:2]]


def dense_form(spec):
    """The column form of the case's fp32 view (zf_solver_ls_plan out[0]): what _check_storage compares plan[0] with."""
    return plan(spec)[0]


def case_id(spec):
    """loss - seed - shape - column form - weights - factors - box - l2"""
    tags = ([f"w{spec.weights}"] * (spec.weights is not None) + [f"p{spec.factors}"] * (spec.factors is not None)
            + ["box"] * (spec.bounds is not None) + ["l2"] * (spec.l2fac > 0))
    return "-".join([spec.loss, f"s{spec.seed:02d}", f"{spec.shape[0]}x{spec.shape[1]}", FORM_NAMES[dense_form(spec)]] + tags)


def round_f32(A):
    """float64(float32(A)), element by element, for a dense array or a CSR matrix (a zero stays a zero)."""
    if sp.issparse(A):
        A = sp.csr_matrix(A, dtype=np.float64)
        return sp.csr_matrix((A.data.astype(np.float32).astype(np.float64), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    return np.asarray(A, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def data(loss, shape):
    """(A64 csr, b, lam, delta): X.data with the matrix rounded to fp32 and widened again - read-only."""
    A, b, lam, delta = X.data(loss, shape)
    return round_f32(A), b, lam, delta


def generated(loss, shape):
    """The dense matrix as generated (unrounded fp64): what the device problem is built from."""
    return X.dense(loss, shape)


@functools.lru_cache(maxsize=None)
def dense(loss, shape):
    return data(loss, shape)[0].toarray()


@functools.lru_cache(maxsize=None)
def dense_reversed(loss, shape):
    return np.ascontiguousarray(dense(loss, shape)[::-1])


def build(spec):
    """X.build's case with A64 (CSR) in place of the matrix."""
    return X.build(spec)._replace(A=data(spec.loss, spec.shape)[0])


def make_problem(case, storage="dense"):
    """The fp32 device problem of a case, from the matrix as generated (module docstring)."""
    from zfista_amd import problems as Z

    assert storage == "dense", "only the dense fp32 form is part of this table"
    sp_ = case.spec
    A = generated(sp_.loss, sp_.shape)
    if sp_.loss == "logistic":
        prob = Z.LogisticL1(A, case.b, case.lam, scale=sp_.scale, bounds=sp_.bounds)
        if sp_.seed % 2:
            prob = prob.with_matrix_dtype("float32")
        if case.l2 > 0:
            prob = prob.with_penalty(case.lam, case.l2)
        if case.w is not None:
            prob = prob.with_sample_weight(case.w)
        if case.p is not None:
            prob = prob.with_penalty_factor(case.p)
        return prob if sp_.seed % 2 else prob.with_matrix_dtype("float32")
    cls = {"square": Z.LeastSquaresL1, "huber": Z.HuberL1, "poisson": Z.PoissonL1}[sp_.loss]
    lead = (A, case.b, case.lam, case.delta) if sp_.loss == "huber" else (A, case.b, case.lam)
    return cls(*lead, scale=sp_.scale, bounds=sp_.bounds, l2=case.l2, sample_weight=case.w, penalty_factor=case.p,
               matrix_dtype="float32")


_ORACLE = {}
_THIS = sys.modules[__name__]


def oracle(spec):
    """X.oracle on this table: (case, options after the stagnation cut, the oracle's result on A64, non-finite returns of f)."""
    return X.oracle(spec, cases=_THIS)


def other_form(spec):
    return X.other_form(spec, cases=_THIS)


def accepted(spec):
    """X.accepted's criteria, unchanged, on A64."""
    return X.accepted(spec, cases=_THIS)


def resume_cases():
    return X.resume_cases(cases=_THIS)


def extra_block(k):
    return X.extra_block(k, cases=_THIS)
