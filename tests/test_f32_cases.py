"""CPU: the case table of the fp32-matrix tests agrees with the dispatch rule, rounding the matrix to fp32 is material in
every case, and the host-side refusals of ``matrix_dtype`` come before anything touches a device."""
import warnings

import numpy as np
import pytest

import f32_cases as F
from conftest import rel_err


def test_case_table_follows_the_dispatch_rules():
    for case in F.CASES:
        (m, n), _, _, plan, _ = case
        assert F.dispatch_f32(m, n) == plan, F.case_id(case)
    # every form of both sweeps, the row-group loop and its absence, one slice and the slice cap
    assert {c[3][0] for c in F.CASES} == {F.COLS_V4, F.COLS_V2, F.COLS_V1}
    assert {c[3][1] for c in F.CASES} == {F.ROWS_V4, F.ROWS_V2, F.ROWS_V1}
    for form in (F.ROWS_V4, F.ROWS_V1):
        assert any(c[3][1] == form and c[0][0] > F.ROW_LOOP_MIN_M for c in F.CASES), "the row sweep must loop in a V4 and a V1 case"
    assert any(c[3][2] == 1 and c[0][0] > 1 for c in F.CASES) and any(c[3][2] == 64 for c in F.CASES)
    # a slice shorter than the others, an unrolled main loop with a tail, and a slice that is tail only
    assert any(m % rps not in (0,) and s > 1 for (m, _), _, _, (_, _, s, rps), _ in F.CASES)
    assert any(rps > 8 and rps % 8 for _, _, _, (_, _, _, rps), _ in F.CASES) and any(rps < 8 for _, _, _, (_, _, _, rps), _ in F.CASES)
    # more than 2000 column panels in one case; one case the fp64 class sends to its fused small-matrix path
    assert any(-(-(n // F.width(n)) // 256) > 2000 for (_, n), *_ in F.CASES)
    assert any(n % 32 == 0 and m <= 4096 and m * n <= 1 << 22 for (m, n), *_ in F.CASES)


def test_width_rule():
    assert [F.width(n) for n in (1, 2, 3, 4, 6, 8, 33, 4001, 4002, 4096)] == [1, 2, 1, 4, 2, 4, 1, 1, 2, 4]


@pytest.mark.parametrize("case", F.CASES, ids=F.IDS)
def test_rounding_is_material(case):
    """The oracle's FISTA iterates on A as generated and on A64 = float64(float32(A)), after the case's iterations of the
    near-lam-max variant, differ by more than 1e3 TOL: a GPU solve that silently kept fp64 A would miss the oracle on A64 by
    three orders of magnitude more than the comparison allows."""
    from oracle import cpu_ref, problems_ref as P

    (m, n), scale, _, _, _ = case
    D = F.make(case)
    assert D.A32.dtype == np.float32 and np.array_equal(D.A64.astype(np.float32), D.A32) and not np.array_equal(D.A64, D.A)
    lam, x0 = F.fista_problem(D, m, n, scale, "near-lam-max")
    kw = F.fista_kw(D, m, n, scale, "near-lam-max")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full = cpu_ref.minimize_proximal_gradient(*P.LeastSquaresL1Ref(D.A, D.b, lam, scale=scale).callbacks(), x0, **kw)
        rounded = cpu_ref.minimize_proximal_gradient(*P.LeastSquaresL1Ref(D.A64, D.b, lam, scale=scale).callbacks(), x0, **kw)
    assert full.nit == rounded.nit == F.fista_iters(m, n)
    assert np.any(rounded.allvecs[-1] != 0), "the iterate must not be thresholded to zero"
    sep = rel_err(full.allvecs[-1], rounded.allvecs[-1])
    print(f"{F.case_id(case)}: rounding moves x_K by {sep:.3g} relative")
    assert sep > 1e3 * F.TOL, sep


class _Group:
    """Stands in for a process group: the refusal must come before anything looks at it."""


# (the bare object gets a fixed id: its repr carries an address, another one in every run)
@pytest.mark.parametrize("bad", ["float16", "double", "f32", 32, np.float16, np.int32, pytest.param(object(), id="object()")], ids=repr)
def test_a_bad_matrix_dtype_is_refused_on_the_host(bad):
    from zfista_amd.problems import HuberL1, LeastSquaresL1, PoissonL1

    A, b = np.ones((3, 2)), np.ones(3)
    for make in (lambda: LeastSquaresL1(A, b, 0.1, matrix_dtype=bad), lambda: HuberL1(A, b, 0.1, 1.0, matrix_dtype=bad),
                 lambda: PoissonL1(A, b, 0.1, matrix_dtype=bad)):
        with pytest.raises(ValueError, match="matrix_dtype"):
            make()


def test_matrix_dtype_names():
    import torch

    from zfista_amd.problems import _matrix_dtype

    for v in (None, "float64", np.float64, np.dtype("float64"), torch.float64):
        assert _matrix_dtype(v) == "float64"
    for v in ("float32", np.float32, np.dtype("float32"), torch.float32):
        assert _matrix_dtype(v) == "float32"


def test_group_with_an_fp32_matrix_is_refused_on_the_host():
    from zfista_amd.problems import LeastSquaresL1

    with pytest.raises(ValueError, match="group="):
        LeastSquaresL1(np.ones((3, 2)), np.ones(3), 0.1, group=_Group(), matrix_dtype="float32")
    with pytest.raises(ValueError, match="group="):
        LeastSquaresL1(np.ones((3, 2)), np.ones(3), 0.1, group=_Group(), shard="rows", matrix_dtype=np.float32)


def test_the_logistic_constructor_keeps_its_parameter_list():
    import inspect

    from zfista_amd.problems import LogisticL1, SparseLeastSquaresL1

    assert list(inspect.signature(LogisticL1.__init__).parameters) == ["self", "A", "b", "lam", "scale", "bounds"]
    assert "matrix_dtype" not in inspect.signature(SparseLeastSquaresL1.__init__).parameters
    assert hasattr(LogisticL1, "with_matrix_dtype")
