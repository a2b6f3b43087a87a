"""GPU: SparseLeastSquaresL1 - the CSR row-sum kernels (csrc/zf_kernels_spmv.h) element by element, and device-resident
solves against the CPU oracle, the reference's fixture and the dense class.

A sweep sums a row with L lanes (a power of two from 4 to 64, the largest that is at most the mean row length); rows
longer than sparse.SPLIT_THRESHOLD are cut into segments summed by a wave each and added in segment order.  One case
table drives the kernel checks; every case asserts the plan it claims (zf_solver_ls_plan: 5, L of the sweep over A, L
of the sweep over A^T, split rows of both).  Element checks are against a longdouble evaluation with the a-priori
bound of an fp64 evaluation in any order (oracle.problems_ref.ls_longdouble)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import sparse_cases as S
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-10
T = 4096   # sparse.SPLIT_THRESHOLD, restated (test_case_table_follows_the_plan_rules checks it)


def _rand(m, n, nnz, seed):
    rng = np.random.default_rng(seed)
    flat = rng.choice(m * n, size=nnz, replace=False)
    return sp.csr_matrix((rng.standard_normal(nnz), (flat // n, flat % n)), shape=(m, n))


def _with_rows(A, dense_rows=(), row_fill=(), dense_cols=(), empty_rows=(), empty_cols=(), seed=0):
    """A with whole rows / columns made dense, rows given an exact number of elements, rows / columns emptied."""
    rng = np.random.default_rng(seed)
    A = A.tolil()
    m, n = A.shape
    for i in dense_rows:
        A[i, :] = rng.standard_normal(n)
    for i, count in row_fill:
        A[i, :] = 0
        A[i, rng.choice(n, count, replace=False)] = rng.standard_normal(count)
    for j in dense_cols:
        A[:, j] = rng.standard_normal(m).reshape(-1, 1)
    for i in empty_rows:
        A[i, :] = 0
    for j in empty_cols:
        A[:, j] = 0
    A = A.tocsr()
    A.eliminate_zeros()
    return A


# name -> (builder, claimed plan (5, L of A, L of A^T, split rows), what the case reaches)
CASES = {
    "L4-L4": (lambda: _rand(600, 600, 3600, 1), (5, 4, 4, 0), "mean 6 / 6: the fewest lanes on both sweeps"),
    "L8-L4": (lambda: _rand(500, 1000, 6000, 2), (5, 8, 4, 0), "mean 12 / 6"),
    "L4-L8": (lambda: _rand(1000, 500, 6000, 3), (5, 4, 8, 0), "mean 6 / 12"),
    "L32-L16": (lambda: _rand(400, 800, 16000, 4), (5, 32, 16, 0), "mean 40 / 20"),
    "L16-L32": (lambda: _rand(2000, 1000, 40000, 5), (5, 16, 32, 0), "mean 20 / 40"),
    "L64-L16": (lambda: _rand(300, 1200, 28800, 6), (5, 64, 16, 0), "mean 96 / 24: one wave per row"),
    "L16-L64": (lambda: _rand(1200, 300, 28800, 7), (5, 16, 64, 0), "mean 24 / 96"),
    "L64-L64": (lambda: _rand(333, 301, 30000, 8), (5, 64, 64, 0), "mean 90 / 99, m and n odd: partial row groups"),
    "dense-row-40000": (lambda: _with_rows(_rand(8, 40000, 400, 9), dense_rows=[3]), (5, 64, 4, 1),
                        "a row of 40000 > 2 T: 10 segments, the last one short"),
    "dense-col-10000": (lambda: _with_rows(_rand(10000, 16, 3000, 10), dense_cols=[5]), (5, 4, 64, 1),
                        "a column of 10000 > 2 T: 3 segments in the sweep over A^T"),
    "rows-at-T": (lambda: _with_rows(_rand(6, 9001, 50, 11), row_fill=[(0, T), (2, T + 1), (4, 2 * T), (5, 2 * T + 1)]),
                  (5, 64, 4, 3), "rows of exactly T (not split), T + 1 (T + 1), 2 T (two full segments), 2 T + 1"),
    "cols-at-T": (lambda: _with_rows(_rand(6, 9001, 50, 12), row_fill=[(0, T), (2, T + 1), (4, 2 * T), (5, 2 * T + 1)], seed=1).T.tocsr(),
                  (5, 4, 64, 3), "the same as columns: the sweep over A^T splits"),
    "empty-rows-cols": (lambda: _with_rows(_rand(200, 300, 3000, 13), empty_rows=[0, 77, 199], empty_cols=[0, 150, 299]),
                        (5, 8, 8, 0), "empty first / middle / last rows and columns"),
    "1x1": (lambda: sp.csr_matrix(np.array([[2.5]])), (5, 4, 4, 0), "smallest problem"),
    "m1": (lambda: _with_rows(sp.csr_matrix((1, 777)), dense_rows=[0]), (5, 64, 4, 0), "one row; every row of A^T holds one element"),
    "n1": (lambda: _with_rows(sp.csr_matrix((513, 1)), dense_cols=[0]), (5, 4, 64, 0), "one column"),
    "nnz0": (lambda: sp.csr_matrix((5, 9)), (5, 4, 4, 0), "no stored element"),
    "one-per-row": (lambda: sp.csr_matrix((np.random.default_rng(14).standard_normal(1001),
                                           (np.arange(1001), np.random.default_rng(15).integers(0, 640, 1001))), shape=(1001, 640)),
                    (5, 4, 4, 0), "every row has one element; n even, m odd"),
    "small-case-2": (lambda: S.make_sparse(*S.SMALL[1])[0], (5, 32, 16, 1), "2000 x 5000: a row of 4999 splits, a column of 1999 does not"),
    "small-case-4": (lambda: S.make_sparse(*S.SMALL[3])[0], (5, 64, 4, 1), "64 x 4099, n odd: a row of 4098 splits"),
}
IDS = list(CASES)


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(name):
        if name not in cache:
            A = CASES[name][0]()
            A.sum_duplicates()
            A.sort_indices()
            rng = np.random.default_rng(len(name) * 131 + A.shape[1])
            cache[name] = (A, rng.standard_normal(A.shape[0]))
        return cache[name]

    yield get
    cache.clear()


def _plan_of(prob):
    from zfista_amd.engine import DeviceSolver

    fields, keep = prob._descriptor()
    solver = DeviceSolver(fields, dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=1, max_backtrack_iter=10),
                          keepalive=keep)
    plan = solver.ls_plan()
    solver.close()
    return plan


def test_case_table_follows_the_plan_rules(built):
    """The rule restated: L = the largest power of two in [4, 64] at most nnz / rows; split rows = rows longer than T."""
    from zfista_amd import sparse

    assert sparse.SPLIT_THRESHOLD == T
    for name, (_, plan, _) in CASES.items():
        A, _ = built(name)
        got = [5]
        for M in (A, A.T.tocsr()):
            mean = M.nnz / M.shape[0]
            got.append(max(4, min(64, 2 ** int(np.floor(np.log2(max(mean, 1)))))))
        got.append(int(np.sum(np.diff(A.indptr) > T) + np.sum(np.diff(A.T.tocsr().indptr) > T)))
        assert tuple(got) == plan, name
    # (b): every L on both sweeps, splits on both sweeps, the edge shapes
    assert {c[1][1] for c in CASES.values()} == {c[1][2] for c in CASES.values()} == {4, 8, 16, 32, 64}
    A, _ = built("dense-row-40000")
    assert np.diff(A.indptr).max() == 40000 > 2 * T
    A, _ = built("dense-col-10000")
    assert np.diff(A.T.tocsr().indptr).max() == 10000 > 2 * T
    A, _ = built("rows-at-T")
    assert sorted(np.diff(A.indptr))[-4:] == [T, T + 1, 2 * T, 2 * T + 1]
    A, _ = built("one-per-row")
    assert np.all(np.diff(A.indptr) == 1)


@pytest.mark.parametrize("scale", [0.5, 1 / 6], ids=["half", "sixth"])
@pytest.mark.parametrize("name", IDS)
def test_f_and_jac_f_element_by_element(name, scale, built):
    """(a) prob.f / prob.jac_f - both sweeps, the segment partials and their tail - against the longdouble value, for a
    random x and for x = 0."""
    from oracle import problems_ref as P
    from zfista_amd.problems import SparseLeastSquaresL1

    A, b = built(name)
    m, n = A.shape
    prob = SparseLeastSquaresL1(A, b, 0.1, scale=scale)
    assert _plan_of(prob) == CASES[name][1]
    dense = A.toarray()
    empty_cols = np.flatnonzero(np.diff(A.T.tocsr().indptr) == 0)
    for x in (np.random.default_rng(m + 3 * n).standard_normal(n), np.zeros(n)):
        f, g, f_bound, g_bound = P.ls_longdouble(dense, b, x, scale)
        fv, gv = prob.f(x), prob.jac_f(x)
        print(f"{name} scale {scale:.3g}: f error / bound {float(abs(np.longdouble(fv) - f)) / max(f_bound, 1e-300):.3g}", end="")
        assert abs(np.longdouble(fv) - f) <= f_bound, (float(fv), float(f), f_bound)
        err = np.abs(gv.astype(np.longdouble) - g).astype(np.float64)
        print(f", grad error / bound up to {np.max(err / np.maximum(g_bound, 1e-300)):.3g}")
        bad = np.flatnonzero(err > g_bound)
        assert bad.size == 0, f"{bad.size} of {n} gradient elements outside the fp64 bound, first {bad[:8]}"
        # an empty column is an empty row of A^T: exactly +0.0
        assert np.all(gv[empty_cols] == 0.0) and not np.signbit(gv[empty_cols]).any()
    if A.nnz:
        # the bound means something: without the last stored element of the longest row (where tails and last segments
        # go wrong) that element's gradient entry would miss it by orders of magnitude
        x = np.random.default_rng(m + 3 * n).standard_normal(n)
        _, _, _, g_bound = P.ls_longdouble(dense, b, x, scale)
        i = int(np.argmax(np.diff(A.indptr)))
        k = A.indptr[i + 1] - 1
        assert abs(2 * scale * A.data[k] * float(dense[i] @ x - b[i])) > 100 * g_bound[A.indices[k]]


@pytest.fixture
def solve(monkeypatch):
    """minimize_proximal_gradient on the native path; returns (result, trace rows of every accepted iteration, ls_plan)."""
    from zfista_amd import minimize_proximal_gradient, proximal_gradient as pg

    seen = []

    class _Recorded(pg.NativeRun):
        def __init__(self, *a, **k):
            self.rows = []
            super().__init__(*a, **k)
            self.plan = self.solver.ls_plan()
            seen.append(self)

        def collect(self):
            rows = super().collect()
            self.rows.append(rows)
            return rows

    monkeypatch.setattr(pg, "NativeRun", _Recorded)

    def run(prob, x0, **kw):
        del seen[:]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = minimize_proximal_gradient(*prob.callbacks(), x0, **kw)
        assert len(seen) == 1, "the solve did not run on the native path"
        return res, np.concatenate(seen[0].rows), seen[0].plan

    return run


def _oracle(ref, x0, **kw):
    from oracle import cpu_ref

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cpu_ref.minimize_proximal_gradient(*ref.callbacks(), x0, **kw)


def _check_errs(got, want, vecs):
    """allerrs entry by entry: err_k = max |x+ - y| is a difference of two iterates that are each held to TOL of their
    norm, so an entry may be off by 2 TOL |x| whatever its own size (towards convergence it is orders of magnitude smaller
    than either iterate); beyond that, TOL of itself."""
    xnorm = max(float(np.linalg.norm(v)) for v in vecs)
    np.testing.assert_allclose(got, want, rtol=TOL, atol=2 * TOL * xnorm)


def _check_solve(res, rows, exp):
    """Iterates 1e-10 (norm-relative, rel_err), equal nit, status and trial / lr sequences, allfuns 1e-10 element by
    element; allerrs 1e-10 by rel_err over the sequence and element by element (_check_errs)."""
    from zfista_amd import _lib

    assert res.nit == exp.nit and bool(res.success) == bool(exp.success)
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), np.asarray(exp.alltrials, np.int64))
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float))
    assert rel_err(res.x, exp.x) <= TOL
    assert len(res.allvecs) == len(exp.allvecs) == exp.nit + 1
    worst = max(rel_err(a, e) for a, e in zip(res.allvecs, exp.allvecs))
    print(f"nit {res.nit}, trials {int(rows[:, _lib.TR_TRIALS].sum())}: iterates within {worst:.3g}, "
          f"allerrs within {rel_err(res.allerrs, exp.allerrs):.3g}")
    assert worst <= TOL
    np.testing.assert_allclose(res.allfuns, exp.allfuns, rtol=TOL, atol=0)
    assert rel_err(res.allerrs, exp.allerrs) <= TOL
    _check_errs(res.allerrs, exp.allerrs, exp.allvecs)


VARIANTS = {
    "ista": dict(nesterov=False),
    "fista": dict(nesterov=True),
    "momentum-half-16th": dict(nesterov=True, nesterov_ratio=(0.5, 1 / 16)),
    "scale-sixth": dict(nesterov=True, scale=1 / 6),
    "deprecated": dict(nesterov=True, deprecated=True),
    "box": dict(nesterov=True, bounds=(-0.05, 0.3)),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", S.SMALL + [S.TALL], ids=lambda c: f"{c[0]}x{c[1]}")
def test_solve_vs_oracle(case, variant, solve):
    """(c) 80 iterations from lr = 1 (7 - 12 backtracking trials at the start) against the oracle on SciPy-sparse
    closures, every iterate.  The tall case (40000 rows; checked on the CPU like the others: both summation orders take
    the same trials in every variant) runs the many-workgroup residual kernels and splits a column."""
    from zfista_amd.problems import SparseLeastSquaresL1

    m, n, density, seed = case
    A, b, lam = S.make_sparse(m, n, density, seed)
    kw = dict(VARIANTS[variant])
    pk = dict(scale=kw.pop("scale", 0.5), bounds=kw.pop("bounds", None))
    kw.update(lr=1, tol=0.0, max_iter=80, return_all=True)
    res, rows, plan = solve(SparseLeastSquaresL1(A, b, lam, **pk), np.zeros(n), **kw)
    assert plan[0] == 5
    exp = _oracle(S.SparseLeastSquaresL1Ref(A, b, lam, **pk), np.zeros(n), **kw)
    assert exp.nit == 80 and sum(exp.alltrials) > 80
    _check_solve(res, rows, exp)
    if pk["bounds"] is not None:
        lo, hi = pk["bounds"]
        assert res.x.min() >= lo and res.x.max() <= hi and np.count_nonzero((res.x == lo) | (res.x == hi)) >= 10


@pytest.mark.parametrize("case,nit", list(zip(S.SMALL, (371, 711, 246, 1802))), ids=lambda v: str(v))
def test_solve_to_termination_vs_oracle(case, nit, solve):
    """(c) tol = 1e-6 to termination: the same iteration count as the oracle, status 1."""
    from zfista_amd.problems import SparseLeastSquaresL1

    m, n, density, seed = case
    A, b, lam = S.make_sparse(m, n, density, seed)
    kw = dict(lr=1, tol=1e-6, nesterov=True, max_iter=5000, return_all=True)
    res, rows, _ = solve(SparseLeastSquaresL1(A, b, lam), np.zeros(n), **kw)
    exp = _oracle(S.SparseLeastSquaresL1Ref(A, b, lam), np.zeros(n), **kw)
    assert exp.nit == nit and exp.success and res.status == 1
    _check_solve(res, rows, exp)


@pytest.mark.parametrize("tag", list(S.GOLDEN_VARIANTS))
@pytest.mark.parametrize("ci", S.GOLDEN_CASES)
def test_solve_vs_reference_fixture(golden, ci, tag, solve):
    """(c) the same solves against what the REFERENCE solver produced (tests/golden/make_golden_sparse.py)."""
    from zfista_amd import _lib
    from zfista_amd.problems import SparseLeastSquaresL1

    G = golden("g14_sparse_lasso.npz")
    m, n, density, seed = S.SMALL[ci]
    A, b, lam = S.make_sparse(m, n, density, seed)
    assert lam == float(G(f"c{ci}.lam"))
    res, rows, _ = solve(SparseLeastSquaresL1(A, b, lam), np.zeros(n), **S.GOLDEN_KW, **S.GOLDEN_VARIANTS[tag])
    pre = f"c{ci}.{tag}"
    assert res.nit == int(G(f"{pre}.nit")) == 80
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), G(f"{pre}.alltrials"))
    assert np.array_equal(rows[:, _lib.TR_LR], G(f"{pre}.alllrs"))
    assert rel_err(res.x, G(f"{pre}.x")) <= TOL
    assert abs(np.linalg.norm(res.x) - float(G(f"{pre}.xnorm"))) <= TOL * float(G(f"{pre}.xnorm"))
    for k, v in zip(G(f"{pre}.kept"), G(f"{pre}.vecs")):
        assert rel_err(res.allvecs[k][::S.GOLDEN_STRIDE], v) <= TOL, k
    np.testing.assert_allclose(res.allfuns, G(f"{pre}.allfuns"), rtol=TOL, atol=0)
    assert rel_err(res.allerrs, G(f"{pre}.allerrs")) <= TOL
    np.testing.assert_allclose(res.allerrs, G(f"{pre}.allerrs"), rtol=TOL, atol=2 * TOL * float(G(f"{pre}.xnorm")))


@pytest.mark.parametrize("tag,nest", [("ista", False), ("fista", True)])
def test_matrix_without_stored_elements(golden, tag, nest, solve):
    """(c) the reference's own first LASSO test, A = 0: x0 = 0.3, scale 1/6, b = (-1, 0, 1), lam 0.1 -> x = 0."""
    from zfista_amd.problems import SparseLeastSquaresL1

    G = golden("g14_sparse_lasso.npz")
    A, b, lam, scale, x0 = S.azero_problem()
    prob = SparseLeastSquaresL1(A, b, lam, scale=scale)
    assert prob.nnz == 0 and prob.f(x0) == pytest.approx(2 / 6, rel=1e-15) and np.array_equal(prob.jac_f(x0), [0.0])
    res, rows, plan = solve(prob, x0, return_all=True, nesterov=nest)
    assert plan == (5, 4, 4, 0)
    assert np.array_equal(res.x, [0.0]) and res.status == 1 and res.nit == int(G(f"azero.{tag}.nit"))
    np.testing.assert_allclose(res.allfuns, G(f"azero.{tag}.allfuns"), rtol=TOL, atol=0)
    np.testing.assert_allclose(res.allerrs, G(f"azero.{tag}.allerrs"), rtol=TOL, atol=1e-16)
    np.testing.assert_allclose(np.asarray(res.allvecs), G(f"azero.{tag}.vecs"), rtol=TOL, atol=1e-16)


@pytest.mark.parametrize("case", S.SMALL + [S.TALL], ids=lambda c: f"{c[0]}x{c[1]}")
def test_same_trials_as_the_dense_class(case, solve):
    """(d) LeastSquaresL1 on the densified matrix and the sparse problem take the same trial sequence, 1e-10 apart."""
    from zfista_amd import _lib
    from zfista_amd.problems import LeastSquaresL1, SparseLeastSquaresL1

    m, n, density, seed = case
    A, b, lam = S.make_sparse(m, n, density, seed)
    kw = dict(lr=1, tol=0.0, max_iter=80, nesterov=True, return_all=True)
    rs, rows_s, plan_s = solve(SparseLeastSquaresL1(A, b, lam), np.zeros(n), **kw)
    rd, rows_d, plan_d = solve(LeastSquaresL1(A.toarray(), b, lam), np.zeros(n), **kw)
    assert plan_s[0] == 5 and plan_d[0] in (1, 2, 3, 4)
    assert rs.nit == rd.nit == 80
    assert np.array_equal(rows_s[:, _lib.TR_TRIALS], rows_d[:, _lib.TR_TRIALS])
    assert np.array_equal(rows_s[:, _lib.TR_LR], rows_d[:, _lib.TR_LR])
    assert max(rel_err(a, e) for a, e in zip(rs.allvecs, rd.allvecs)) <= TOL
    np.testing.assert_allclose(rs.allfuns, rd.allfuns, rtol=TOL, atol=0)


def test_large_case_vs_oracle(solve):
    """(e) 200 000 x 1 000 003 with 8 draws per column (nnz 7 999 888, row lengths 16 .. 77), 60 FISTA iterations from
    lr = 1 (66 trials, final lr 2^-6) against the oracle on SciPy closures."""
    from zfista_amd import _lib
    from zfista_amd.problems import SparseLeastSquaresL1

    m, n, per_col, seed = S.BIG
    A, b, lam = S.make_sparse_big(m, n, per_col, seed)
    assert A.nnz == 7_999_888
    kw = dict(lr=1, tol=0.0, max_iter=60, nesterov=True)
    res, rows, plan = solve(SparseLeastSquaresL1(A, b, lam), np.zeros(n), **kw)
    assert plan == (5, 32, 4, 0)
    exp = _oracle(S.SparseLeastSquaresL1Ref(A, b, lam), np.zeros(n), **kw)
    assert exp.nit == res.nit == 60 and sum(exp.alltrials) == 66
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), np.asarray(exp.alltrials, np.int64))
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float)) and rows[-1, _lib.TR_LR] == 2.0 ** -6
    print(f"large case: x within {rel_err(res.x, exp.x):.3g}, {np.count_nonzero(res.x)} non-zeros")
    assert rel_err(res.x, exp.x) <= TOL and np.count_nonzero(res.x) == np.count_nonzero(exp.x)


def test_bit_reproducible(solve):
    """(f) no atomics, every sum in a fixed order: two solves give the same bits - x, every iterate, every trace row."""
    from zfista_amd.problems import SparseLeastSquaresL1

    A, b, lam = S.make_sparse(*S.SMALL[1])   # (split rows in the sweep over A)
    kw = dict(lr=1, tol=0.0, max_iter=60, nesterov=True, return_all=True)
    (r1, rows1, p1), (r2, rows2, p2) = [solve(SparseLeastSquaresL1(A, b, lam), np.zeros(A.shape[1]), **kw) for _ in range(2)]
    assert p1 == p2 == (5, 32, 16, 1)
    assert np.array_equal(r1.x, r2.x) and np.array_equal(rows1, rows2)
    assert np.array_equal(np.asarray(r1.allvecs), np.asarray(r2.allvecs))
    x = np.random.default_rng(0).standard_normal(A.shape[1])
    p, q = SparseLeastSquaresL1(A, b, lam), SparseLeastSquaresL1(A.tocoo(), b, lam)
    assert p.f(x) == q.f(x) and np.array_equal(p.jac_f(x), q.jac_f(x))


def _split_both():
    """9000 x 9000 with a dense row and a dense column: split rows in the sweep over A and in the sweep over A^T."""
    A = _with_rows(_rand(9000, 9000, 90000, 21), dense_rows=[5], dense_cols=[7], seed=3)
    A.sum_duplicates()
    A.sort_indices()
    rng = np.random.default_rng(22)
    x_true = np.zeros(9000)
    x_true[:20] = rng.standard_normal(20)
    b = A @ x_true + 0.01 * rng.standard_normal(9000)
    return A, b, 0.1 * np.max(np.abs(A.T @ b))


@pytest.mark.parametrize("which", ["split-both", "tall"])
def test_solves_of_one_problem_on_streams_equal_the_solves_alone(which):
    """Several solves of ONE SparseLeastSquaresL1 at the same time (zfista_amd.replicas.solve_on_streams: a host thread and
    a HIP stream each) while another thread evaluates prob.f / prob.jac_f: the matrix handle is shared, the segment sums of
    split rows are not - every result is bit for bit the one the same call gives alone."""
    import threading

    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.problems import SparseLeastSquaresL1
    from zfista_amd.replicas import solve_on_streams

    A, b, lam = _split_both() if which == "split-both" else S.make_sparse(*S.TALL)
    n = A.shape[1]
    prob = SparseLeastSquaresL1(A, b, lam)
    plan = _plan_of(prob)
    assert plan[0] == 5 and plan[3] == (2 if which == "split-both" else 1)
    ratios = [(0, 0.25), (0.5, 1 / 16), (0.75, 0.25), (0.25, 1 / 64), (1 / 6, 1 / 144), (0.1, 0.2)]
    kws = [dict(lr=1, tol=0.0, max_iter=150, nesterov=True, nesterov_ratio=r, return_all=(k % 2 == 0)) for k, r in enumerate(ratios)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alone = [minimize_proximal_gradient(*prob.callbacks(), np.zeros(n), **kw) for kw in kws]
    xs = [np.random.default_rng(k).standard_normal(n) for k in range(3)]
    want = [(prob.f(x), prob.jac_f(x)) for x in xs]
    stop, seen, wrong = threading.Event(), [0], []

    def evaluate():
        while not stop.is_set():
            for x, (f, g) in zip(xs, want):
                if prob.f(x) != f or not np.array_equal(prob.jac_f(x), g):
                    wrong.append(seen[0])
                seen[0] += 1

    t = threading.Thread(target=evaluate)
    t.start()
    try:
        together = solve_on_streams([(prob, np.zeros(n), kw) for kw in kws], streams=6)
        again = solve_on_streams([(prob, np.zeros(n), kw) for kw in kws], streams=3)
    finally:
        stop.set()
        t.join()
    assert seen[0] >= 3 and not wrong, f"{len(wrong)} of {seen[0]} evaluations beside running solves differ from the value alone"
    for a, c, d in zip(alone, together, again):
        assert a.nit == c.nit == d.nit == 150
        assert np.array_equal(a.x, c.x) and np.array_equal(a.x, d.x) and a.fun == c.fun == d.fun
        if a.allfuns is not None:
            assert np.array_equal(np.asarray(a.allfuns), np.asarray(c.allfuns)) and np.array_equal(np.asarray(a.allerrs), np.asarray(c.allerrs))
            assert np.array_equal(np.asarray(a.allvecs), np.asarray(c.allvecs))


def test_a_plan_that_does_not_fit_the_row_pointers_is_refused():
    """zf_spmat_create checks the caller's plan against indptr: the rows kernel leaves exactly the rows longer than the
    threshold to the plan's segments, so a plan that names other rows, or starts a row's segments elsewhere, is an error."""
    from zfista_amd import _lib, sparse
    from zfista_amd.problems import _SpmatHandle

    A, _ = _split_both()[0], None
    good = sparse.prepare(A)
    assert good["plan"]["split_row"].size == 1 and good["t_plan"]["split_row"].size == 1
    _SpmatHandle(good)   # (the plan as built is accepted)

    def broken(key, **change):
        p = dict(good)
        p[key] = dict(good[key], **change)
        return p

    none = sparse.plan_rows(np.zeros(A.shape[0] + 1, dtype=np.int64))
    shifted = good["plan"]["seg_start"].copy()
    shifted[0] += 1
    other_row = good["t_plan"]["split_row"] + 1
    short = dict(split_first=np.array([0, 2]), seg_start=good["plan"]["seg_start"][:2].copy())
    for p in (broken("plan", split_row=none["split_row"], split_first=none["split_first"], seg_start=none["seg_start"]),
              broken("plan", seg_start=shifted), broken("t_plan", split_row=other_row), broken("plan", **short),
              broken("t_plan", threshold=2048)):
        with pytest.raises(_lib.ZfError):
            _SpmatHandle(p)


def test_snapshot_resume_is_bit_identical(tmp_path):
    """(f) a solve interrupted by snapshot() / from_snapshot continues bit for bit (A x_k, A x_{k-1} are recomputed by the
    sweep that produced them)."""
    from zfista_amd import _lib
    from zfista_amd.problems import SparseLeastSquaresL1
    from zfista_amd.proximal_gradient import NativeRun

    A, b, lam = S.make_sparse(*S.SMALL[0])
    prob = SparseLeastSquaresL1(A, b, lam)
    o = dict(lr=1, tol=0.0, tol_internal=1e-12, max_iter=70, max_iter_internal=100000, max_backtrack_iter=100, warm_start=False,
             decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False, deprecated=False)

    def drain(run):
        rows = [np.zeros((0, _lib.ZF_TRACE_COLS))]
        while run.status == _lib.ZF_RUNNING:
            rows.append(run.advance(5))
        return np.concatenate(rows)

    whole = NativeRun(prob, np.zeros(prob.n_features), o)
    ref_rows, ref_x = drain(whole), whole.solver.get_x()
    whole.solver.close()
    for stop_after in (3, 20):   # inside the backtracking phase, and behind it
        first = NativeRun(prob, np.zeros(prob.n_features), o)
        head = [first.advance(1) for _ in range(stop_after)]
        state = first.snapshot()
        first.solver.close()
        np.savez(tmp_path / "ckpt.npz", **state)
        run = NativeRun.from_snapshot(prob, dict(np.load(tmp_path / "ckpt.npz")), o)
        rows = np.concatenate(head + [drain(run)])
        assert np.array_equal(rows, ref_rows) and np.array_equal(run.solver.get_x(), ref_x), stop_after
        run.solver.close()


def test_callbacks_as_opaque_callables_and_keywords():
    """(g) the callbacks handed to the oracle's solver as opaque callables (the generic use) reproduce case 1;
    acceptance="resolved" is refused as for every non-separable problem; there is no group= keyword."""
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.problems import NativeProblem, SparseLeastSquaresL1, match_native

    m, n, density, seed = S.SMALL[0]
    A, b, lam = S.make_sparse(m, n, density, seed)
    prob = SparseLeastSquaresL1(A, b, lam)
    assert isinstance(prob, NativeProblem) and match_native(*prob.callbacks()) is prob
    kw = dict(lr=1, tol=0.0, max_iter=80, nesterov=True, return_all=True)
    got = _oracle(prob, np.zeros(n), **kw)
    exp = _oracle(S.SparseLeastSquaresL1Ref(A, b, lam), np.zeros(n), **kw)
    assert got.nit == exp.nit == 80 and np.array_equal(got.alltrials, exp.alltrials)
    assert max(rel_err(a, e) for a, e in zip(got.allvecs, exp.allvecs)) <= TOL
    with pytest.raises(ValueError):
        minimize_proximal_gradient(*prob.callbacks(), np.zeros(n), acceptance="resolved")
    with pytest.raises(TypeError):
        SparseLeastSquaresL1(A, b, lam, group=None)
    with pytest.raises(ValueError):
        prob.f(np.zeros(n + 1))
    # the method form, and the result fields of the dense class
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = prob.minimize_proximal_gradient(np.zeros(n), nesterov=True, tol=1e-6, lr=1)
    assert res.success and res.status == 1 and res.nit == 371 and rel_err(res.x, _oracle(
        S.SparseLeastSquaresL1Ref(A, b, lam), np.zeros(n), nesterov=True, tol=1e-6, lr=1).x) <= TOL
