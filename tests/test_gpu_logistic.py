"""GPU: LogisticL1 / SparseLogisticL1 - the loss kernels (csrc/zf_kernels_loss.h) element by element through the evaluation
entry points, device-resident solves against the CPU oracle and the reference's fixture G15, the two classes against each
other, the MFMA column sweep against the VALU one, and the shared machinery (return_all, snapshots, streams) on the new
kinds.

The element-wise bound (test_f_and_jac_f_element_by_element), with u = 2^-53, gamma_k = k u / (1 - k u), c = |A| |x|:

  margins   s_i = (A x)_i summed in ANY order in fp64:  ds_i = |s^_i - s_i| <= gamma_n c_i  (Higham 3.1; what the sparse tests
            use for the same sweeps).  t_i = -b_i s_i is exact (b_i = +-1).
  e         e^ = exp(-|t^|) (1 + eps), |eps| <= 2 u: HIP documents 1 ulp for the double-precision exp, and 1 ulp <= 2 u relative.
  softplus  l^ = log1p(e^) (1 + eps), |eps| <= 2 u (log1p: 1 ulp as well).  |log1p(e^) - log1p(e)| <= |e^ - e| <= 2 u e and
            e <= log1p(e) / ln 2 on (0, 1], so |l^ - l| <= (2 / ln 2 + 2) u l < 5 u l; max(t, 0) is exact, the addition rounds
            once: |sp^ - softplus(t^)| <= 6 u softplus(t^) (+ O(u^2)).  |softplus'| <= 1 carries the margin's error:
                |sp^_i - softplus(t_i)| <= ds_i + 6 u softplus_i
            f = scale * sum: m non-negative terms in any order, gamma_(m-1) of their sum, and one rounding for the factor:
                |f^ - f| <= scale ( sum_i ds_i + (6 u + gamma_m) sum_i softplus_i )              -> gamma_(m+7)
  sigma     1 + e^ carries u + 2 u e / (1 + e) <= 2 u, the numerator (1 or e^) at most 2 u, the division u: 5 u relative;
            |sigma'| <= 1/4 carries the margin's error:   drho_i = |rho^_i - rho_i| <= ds_i / 4 + 5 u sigma_i  (-b_i: exact)
  gradient  scale * sum_i a_ij rho^_i over m terms in any order, one rounding for the factor:
                |g^_j - g_j| <= scale ( (|A|^T drho)_j + gamma_(m+1) (|A|^T |rho|)_j )
  underflow e below 2^-1022 loses its relative accuracy (exp(-750) = 0 on the device, 1e-326 in longdouble): m * 2^-1022 is
            added to both bounds.
Both bounds carry the safety factor 2 of oracle.problems_ref.ls_longdouble (second-order terms, the bound's own rounding).
The reference values are np.longdouble (64 mantissa bits: expl / log1pl), summed over the stored elements only.

ZF_LOGISTIC_BOUNDS_RECORD=1 appends the worst error-to-bound ratio of every case to profiles/logistic_kernel_bounds.jsonl
(any other value: to that path) - records for the next change of these kernels to compare with, not thresholds."""
import json
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import logistic_cases as L
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-10
WIDE = 1 << 15   # ZF_SPMV_WIDE_RESID_MIN_ROWS, restated: beyond it the loss kernels take many workgroups


def _classes():
    from zfista_amd.problems import LogisticL1, SparseLogisticL1

    return {"csr": SparseLogisticL1, "dense": LogisticL1}


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


# ---- (1) the kernels, element by element ---------------------------------------------------------------------------------
def _rand(m, n, nnz, seed):
    rng = np.random.default_rng(seed)
    flat = rng.choice(m * n, size=nnz, replace=False)
    A = sp.csr_matrix((rng.standard_normal(nnz), (flat // n, flat % n)), shape=(m, n))
    A.sort_indices()
    return A


def _labels(m, seed):
    return np.where(np.random.default_rng(seed).random(m) < 0.5, -1.0, 1.0)


def _case_small(i):
    def build():
        A, b, _ = L.make_logistic(*L.SMALL[i])
        return A, b, np.random.default_rng(i).standard_normal(A.shape[1])
    return build


def _case_tall():
    A, b, _ = L.make_logistic(*L.TALL)
    return A, b, np.random.default_rng(9).standard_normal(A.shape[1])


def _case_rows(m, n=64, per_row=3):
    def build():
        return _rand(m, n, per_row * m, m), _labels(m, m + 1), np.random.default_rng(m + 2).standard_normal(n)
    return build


def _case_margins_750():
    """Rows 0 .. 3 hold the single element +-750 against x_0 = 1 under both labels: t = +-750 in all four combinations;
    the other rows are ordinary.  n odd."""
    A = _rand(40, 33, 300, 17).tolil()
    for i, v in enumerate((750.0, 750.0, -750.0, -750.0)):
        A[i, :] = 0
        A[i, 0] = v
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    b = _labels(40, 18)
    b[:4] = (1.0, -1.0, 1.0, -1.0)
    x = np.random.default_rng(19).standard_normal(33)
    x[0] = 1.0
    return A, b, x


# name -> (builder of (A csr, labels, x), residual shape: "one" workgroup or "wide", what the case reaches)
CASES = {
    "small-300x1000": (_case_small(0), "one", "n even; a dense row and column, an empty row and column"),
    "small-2000x5000": (_case_small(1), "one", "n even; a split row in the CSR sweep"),
    "small-1000x257": (_case_small(2), "one", "n odd, m < 1024: threads without a row"),
    "small-64x4099": (_case_small(3), "one", "n odd, m = 64: one wave of the workgroup has rows"),
    "tall-40000x500": (_case_tall, "wide", "40 chunks of 1000 rows; a column of 39 999 splits in the sweep over A^T"),
    "rows-32768": (_case_rows(WIDE), "one", "the last row count of the one-workgroup form: 32 rows per thread"),
    "rows-32769": (_case_rows(WIDE + 1), "wide", "the first of the wide form: 33 chunks of 993, the last one of 993"),
    "rows-70001": (_case_rows(70001, n=31), "wide", "69 chunks of 1015, the last one shorter; n odd"),
    "margins-750": (_case_margins_750, "one", "t = +-750: exp underflows, softplus = max(t, 0), sigma in {0, 1}"),
    "m1-n777": (lambda: (sp.csr_matrix(np.random.default_rng(20).standard_normal((1, 777))), np.array([-1.0]),
                         np.random.default_rng(21).standard_normal(777)), "one", "one row, n odd"),
    "m1-n2": (lambda: (sp.csr_matrix(np.array([[0.5, -2.0]])), np.array([1.0]), np.array([3.0, 1.0])), "one", "one row, n even"),
    "1x1": (lambda: (sp.csr_matrix(np.array([[2.5]])), np.array([1.0]), np.array([-0.7])), "one", "smallest problem"),
    "nnz0": (lambda: (sp.csr_matrix((5, 9)), _labels(5, 22), np.random.default_rng(23).standard_normal(9)), "one",
             "no stored element: every margin 0, f = 5 ln 2, gradient exactly 0"),
}


def logistic_longdouble(A, b, x, scale):
    """(f, grad, f_bound, grad_bound) of the module docstring for a canonical CSR A: values in np.longdouble, bounds float64."""
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError("np.longdouble carries fewer than 63 mantissa bits here: an fp64 evaluation cannot be checked against it")
    ld = np.longdouble
    m, n = A.shape
    rows = np.repeat(np.arange(m), np.diff(A.indptr))
    data, xl = A.data.astype(ld), np.asarray(x, np.float64).astype(ld)
    s = np.zeros(m, dtype=ld)
    np.add.at(s, rows, data * xl[A.indices])
    t = -np.asarray(b, np.float64).astype(ld) * s
    e = np.exp(-np.abs(t))
    soft = np.maximum(t, ld(0)) + np.log1p(e)
    sigma = np.where(t >= 0, ld(1), e) / (ld(1) + e)
    rho = -np.asarray(b, np.float64).astype(ld) * sigma
    f = ld(scale) * np.sum(soft)
    g = np.zeros(n, dtype=ld)
    np.add.at(g, A.indices, data * rho[rows])
    g *= ld(scale)
    u = 2.0 ** -53
    gamma = lambda k: k * u / (1 - k * u)
    absA = abs(A)
    ds = gamma(n) * (absA @ np.abs(np.asarray(x, np.float64)))
    tiny = m * 2.0 ** -1022
    f_bound = 2 * (scale * (ds.sum() + gamma(m + 7) * float(np.sum(soft))) + tiny)
    drho = ds / 4 + 5 * u * sigma.astype(np.float64)
    g_bound = 2 * (scale * (absA.T @ drho + gamma(m + 1) * (absA.T @ np.abs(rho).astype(np.float64))) + tiny)
    return f, g, f_bound, g_bound


def _record(**rec):
    where = os.environ.get("ZF_LOGISTIC_BOUNDS_RECORD", "")
    if where in ("", "0"):
        return
    path = os.path.join(ROOT, "profiles", "logistic_kernel_bounds.jsonl") if where == "1" else where
    with open(path, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


def test_case_table_reaches_what_it_claims():
    for name, (build, shape, _) in CASES.items():
        A, b, x = build()
        assert (A.shape[0] > WIDE) == (shape == "wide"), name
        assert set(np.unique(b)) <= {-1.0, 1.0} and b.shape == (A.shape[0],) and x.shape == (A.shape[1],)
    assert {CASES[k][0]()[0].shape[1] % 2 for k in CASES} == {0, 1}
    A, b, x = CASES["margins-750"][0]()
    assert sorted((-b * (A @ x))[:4]) == [-750.0, -750.0, 750.0, 750.0]
    A = CASES["small-300x1000"][0]()[0]
    assert np.diff(A.indptr).min() == 0 and np.diff(A.T.tocsr().indptr).min() == 0, "an empty row and an empty column"


@pytest.mark.parametrize("storage", ["csr", "dense"])
@pytest.mark.parametrize("name", list(CASES))
def test_f_and_jac_f_element_by_element(name, storage):
    """prob.f / prob.jac_f (zf_logistic_eval / zf_spmat_logistic_eval: the sweeps and the loss kernels the solver runs) against
    the longdouble value inside the derived bound, at scale 1 and 1 / 3, for x and for x = 0."""
    build, shape, _ = CASES[name]
    A, b, x = build()
    m, n = A.shape
    M = A if storage == "csr" else A.toarray()
    empty_cols = np.flatnonzero(np.diff(A.T.tocsr().indptr) == 0)
    for scale in (1.0, 1 / 3):
        prob = _classes()[storage](M, b, 0.1, scale=scale)
        for xv in (x, np.zeros(n)):
            f, g, f_bound, g_bound = logistic_longdouble(A, b, xv, scale)
            fv, gv = prob.f(xv), prob.jac_f(xv)
            assert np.isfinite(fv) and np.isfinite(gv).all()
            f_ratio = float(abs(np.longdouble(fv) - f)) / f_bound
            err = np.abs(gv.astype(np.longdouble) - g).astype(np.float64)
            g_ratio = float(np.max(err / g_bound))
            print(f"{name} {storage} scale {scale:.3g}: f error / bound {f_ratio:.3g}, grad error / bound up to {g_ratio:.3g}")
            _record(case=name, storage=storage, shape=[m, n], resid=shape, scale=scale, x_zero=bool(not xv.any()),
                    f_err_over_bound=f_ratio, grad_err_over_bound=g_ratio)
            assert abs(np.longdouble(fv) - f) <= f_bound, (float(fv), float(f), f_bound)
            bad = np.flatnonzero(err > g_bound)
            assert bad.size == 0, f"{bad.size} of {n} gradient elements outside the fp64 bound, first {bad[:8]}"
            if storage == "csr":   # an empty column is an empty row of A^T: exactly +0.0
                assert np.all(gv[empty_cols] == 0.0) and not np.signbit(gv[empty_cols]).any()
            else:
                assert np.all(gv[empty_cols] == 0.0)
            if not xv.any():   # every margin 0: softplus = ln 2, sigma = 1/2 exactly
                assert abs(fv - scale * m * np.log(2.0)) <= 2 * m * 2.0 ** -53 * scale * m * np.log(2.0)
    if name == "margins-750":
        prob = _classes()[storage](M, b, 0.1)
        # f - the four saturated rows hold exactly 1500 of it; their rho is 0, -+1: the gradient of x_0 through them is exact
        rest = A[4:]
        only = _classes()[storage](A[:4] if storage == "csr" else A[:4].toarray(), b[:4], 0.1)
        assert only.f(x) == 1500.0 and np.array_equal(only.jac_f(x)[1:], np.zeros(n - 1))
        assert only.jac_f(x)[0] == 750.0 * 1.0 + (-750.0) * (-1.0)   # rows 1 and 2: rho = +1 with a = 750, rho = -1 with a = -750
        assert prob.f(x) > 1500.0 and rest.nnz > 0
    t = -b * (A @ x)
    live = (np.abs(t) < 5) & (np.diff(A.indptr) > 0)   # (a saturated row has sigma = 0 or 1 whatever its elements)
    if live.any():
        # the bound means something: without the largest stored element of the longest unsaturated row that element's
        # gradient entry would miss it by orders of magnitude
        g_bound = logistic_longdouble(A, b, x, 1.0)[3]
        i = int(np.argmax(np.where(live, np.diff(A.indptr), -1)))
        k = A.indptr[i] + int(np.argmax(np.abs(A.data[A.indptr[i]:A.indptr[i + 1]])))
        assert abs(A.data[k]) / (1.0 + np.exp(-t[i])) > 100 * g_bound[A.indices[k]]


# ---- (2) solves -----------------------------------------------------------------------------------------------------------
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
        res = _quiet(minimize_proximal_gradient, *prob.callbacks(), x0, **kw)
        assert len(seen) == 1, "the solve did not run on the native path"
        return res, np.concatenate(seen[0].rows), seen[0].plan

    return run


_ORACLE = {}


def _oracle(case, variant, **kw):
    """The CPU oracle on the stable closures over the CSR matrix (one run per case and variant, shared by both storage forms)."""
    from oracle import cpu_ref

    key = (case, variant)
    if key not in _ORACLE:
        A, b, lam = L.make_logistic(*case)
        okw = dict(kw)
        ref = L.LogisticL1Ref(A, b, lam, scale=okw.pop("scale", 1.0), bounds=okw.pop("bounds", None))
        _ORACLE[key] = _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), np.zeros(A.shape[1]), **okw)
    return _ORACLE[key]


def _check_solve(res, rows, exp):
    """Iterates 1e-10 (norm-relative), equal nit, status and trial / lr sequences, allfuns 1e-10 element by element, allerrs
    1e-10 over the sequence and element by element (an entry is a difference of two iterates held to TOL of their norm each)."""
    from zfista_amd import _lib

    assert res.nit == exp.nit and bool(res.success) == bool(exp.success)
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), np.asarray(exp.alltrials, np.int64))
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float))
    assert rel_err(res.x, exp.x) <= TOL
    assert len(res.allvecs) == len(exp.allvecs) == exp.nit + 1
    worst = max(rel_err(a, e) for a, e in zip(res.allvecs, exp.allvecs))
    print(f"nit {res.nit}, trials {int(rows[:, _lib.TR_TRIALS].sum())}: iterates within {worst:.3g}, "
          f"allfuns within {np.max(np.abs(np.asarray(res.allfuns) - exp.allfuns) / np.abs(exp.allfuns)):.3g}, "
          f"allerrs within {rel_err(res.allerrs, exp.allerrs):.3g}")
    assert worst <= TOL
    np.testing.assert_allclose(res.allfuns, exp.allfuns, rtol=TOL, atol=0)
    assert rel_err(res.allerrs, exp.allerrs) <= TOL
    xnorm = max(float(np.linalg.norm(v)) for v in exp.allvecs)
    np.testing.assert_allclose(res.allerrs, exp.allerrs, rtol=TOL, atol=2 * TOL * xnorm)


VARIANTS = {
    "ista": dict(nesterov=False),
    "fista": dict(nesterov=True),
    "momentum-half-16th": dict(nesterov=True, nesterov_ratio=(0.5, 1 / 16)),
    "box": dict(nesterov=True, bounds=(-0.05, 0.3)),
    "scale-third": dict(nesterov=True, scale=1 / 3),
}
# (every variant was run on the CPU with both evaluation forms of logistic_cases.LogisticL1Ref on both storage forms before it
#  was fixed: equal trial and lr sequences, iterates within 3e-15.  ISTA with scale 1/3 inside the box is NOT here: on the
#  tall case the oracle's own line search collapses - trial counts of 8 in mid-solve, lr towards 1e-15 - which compares
#  rounding noise, not solvers.)


@pytest.mark.parametrize("storage", ["csr", "dense"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", L.SMALL + [L.TALL], ids=lambda c: f"{c[0]}x{c[1]}")
def test_solve_vs_oracle(case, variant, storage, solve):
    """80 iterations from lr = 1 (the line search backtracks at the start) against the oracle on the stable closures, every
    iterate, on both classes.  The tall case runs the many-workgroup loss kernels."""
    A, b, lam = L.make_logistic(*case)
    n = A.shape[1]
    kw = dict(VARIANTS[variant], lr=1, tol=0.0, max_iter=80, return_all=True)
    exp = _oracle(case, variant, **kw)
    pk = dict(scale=kw.pop("scale", 1.0), bounds=kw.pop("bounds", None))
    res, rows, plan = solve(_classes()[storage](L.golden_matrix(A, storage), b, lam, **pk), np.zeros(n), **kw)
    assert plan[0] == 5 if storage == "csr" else plan[0] in (2, 3, 4) and plan[1] in (2, 3)
    assert exp.nit == 80 and sum(exp.alltrials) > 80
    _check_solve(res, rows, exp)
    if pk["bounds"] is not None:
        lo, hi = pk["bounds"]
        assert res.x.min() >= lo and res.x.max() <= hi and np.count_nonzero((res.x == lo) | (res.x == hi)) >= 10


@pytest.mark.parametrize("storage", L.GOLDEN_FORMS)
@pytest.mark.parametrize("tag", list(L.GOLDEN_VARIANTS))
@pytest.mark.parametrize("ci", L.GOLDEN_CASES)
def test_solve_vs_reference_fixture(golden, ci, tag, storage, solve):
    """The same solves against what the REFERENCE solver produced (tests/golden/make_golden_logistic.py)."""
    from zfista_amd import _lib

    G = golden("g15_logistic_l1.npz")
    A, b, lam = L.make_logistic(*L.SMALL[ci])
    n = A.shape[1]
    assert lam == float(G(f"c{ci}.lam"))
    res, rows, _ = solve(_classes()[storage](L.golden_matrix(A, storage), b, lam), np.zeros(n), **L.GOLDEN_KW, **L.GOLDEN_VARIANTS[tag])
    pre = f"c{ci}.{storage}.{tag}"
    assert res.nit == int(G(f"{pre}.nit")) == 80
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), G(f"{pre}.alltrials"))
    assert np.array_equal(rows[:, _lib.TR_LR], G(f"{pre}.alllrs"))
    assert rel_err(res.x, G(f"{pre}.x")) <= TOL
    assert abs(np.linalg.norm(res.x) - float(G(f"{pre}.xnorm"))) <= TOL * float(G(f"{pre}.xnorm"))
    for k, v in zip(G(f"{pre}.kept"), G(f"{pre}.vecs")):
        assert rel_err(res.allvecs[k][::L.GOLDEN_STRIDE], v) <= TOL, k
    np.testing.assert_allclose(res.allfuns, G(f"{pre}.allfuns"), rtol=TOL, atol=0)
    assert rel_err(res.allerrs, G(f"{pre}.allerrs")) <= TOL
    np.testing.assert_allclose(res.allerrs, G(f"{pre}.allerrs"), rtol=TOL, atol=2 * TOL * float(G(f"{pre}.xnorm")))


@pytest.mark.parametrize("case", L.SMALL + [L.TALL], ids=lambda c: f"{c[0]}x{c[1]}")
def test_dense_and_sparse_classes_take_the_same_trials(case, solve):
    """LogisticL1 on the densified matrix and SparseLogisticL1 take the same trial sequence, 1e-10 apart."""
    from zfista_amd import _lib

    A, b, lam = L.make_logistic(*case)
    n = A.shape[1]
    kw = dict(lr=1, tol=0.0, max_iter=80, nesterov=True, return_all=True)
    rs, rows_s, plan_s = solve(_classes()["csr"](A, b, lam), np.zeros(n), **kw)
    rd, rows_d, plan_d = solve(_classes()["dense"](A.toarray(), b, lam), np.zeros(n), **kw)
    assert plan_s[0] == 5 and plan_d[0] in (2, 3, 4), "the dense logistic kind never takes the small-matrix path"
    assert rs.nit == rd.nit == 80
    assert np.array_equal(rows_s[:, _lib.TR_TRIALS], rows_d[:, _lib.TR_TRIALS])
    assert np.array_equal(rows_s[:, _lib.TR_LR], rows_d[:, _lib.TR_LR])
    assert max(rel_err(a, e) for a, e in zip(rs.allvecs, rd.allvecs)) <= TOL
    np.testing.assert_allclose(rs.allfuns, rd.allfuns, rtol=TOL, atol=0)


def _mfma_case():
    """300 x 1024 (n % 32 == 0: the MFMA column sweep is eligible), small enough for the least-squares kind's fused path."""
    A = _rand(300, 1024, 6000, 31)
    rng = np.random.default_rng(32)
    x_true = np.zeros(1024)
    x_true[:20] = rng.standard_normal(20)
    b = np.sign(A @ x_true + 0.1 * rng.standard_normal(300))
    b[b == 0] = 1.0
    return A.toarray(), b, 0.1 * np.max(np.abs(A.T @ (b / 2)))


def test_mfma_and_valu_column_sweeps_take_the_same_decisions(solve, monkeypatch):
    """ZF_GEMV_MFMA=0 against the default on a matrix the least-squares kind would run on its fused small-matrix kernels:
    the logistic kind takes the general path (plan 2 / 3), equal trial and lr sequences, iterates within 1e-10."""
    from zfista_amd import _lib
    from zfista_amd.problems import LeastSquaresL1

    A, b, lam = _mfma_case()
    kw = dict(lr=1, tol=0.0, max_iter=80, nesterov=True, return_all=True)
    r1, rows1, plan1 = solve(_classes()["dense"](A, b, lam), np.zeros(1024), **kw)
    _, _, plan_ls = solve(LeastSquaresL1(A, b, lam), np.zeros(1024), **dict(kw, max_iter=2))
    monkeypatch.setenv("ZF_GEMV_MFMA", "0")
    r0, rows0, plan0 = solve(_classes()["dense"](A, b, lam), np.zeros(1024), **kw)
    assert plan_ls[0] == 1 and plan1[:2] == (2, 2) and plan0[:2] == (3, 2)
    assert r0.overrides.get("ZF_GEMV_MFMA") == "0" and "ZF_GEMV_MFMA" not in (getattr(r1, "overrides", None) or {})
    assert r1.nit == r0.nit == 80 and rows1[:, _lib.TR_TRIALS].sum() > 80
    assert np.array_equal(rows1[:, _lib.TR_TRIALS], rows0[:, _lib.TR_TRIALS]) and np.array_equal(rows1[:, _lib.TR_LR], rows0[:, _lib.TR_LR])
    assert max(rel_err(a, e) for a, e in zip(r1.allvecs, r0.allvecs)) <= TOL


# ---- (3) shared machinery on the new kinds --------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["csr", "dense"])
def test_bit_reproducible_and_sub_iters_and_return_all(storage, solve):
    """No atomics, every sum in a fixed order: two solves give the same bits - x, every iterate, every trace row; sub_iters
    (chains exist for separable f only) changes nothing; a solve without return_all ends at the same bits."""
    A, b, lam = L.make_logistic(*L.SMALL[1])
    n = A.shape[1]
    M = L.golden_matrix(A, storage)
    kw = dict(lr=1, tol=0.0, max_iter=60, nesterov=True, return_all=True)
    r1, rows1, p1 = solve(_classes()[storage](M, b, lam), np.zeros(n), **kw)
    assert len(r1.allvecs) == 61 and len(r1.allfuns) == 61 and np.array_equal(r1.allvecs[-1], r1.x) and np.array_equal(r1.allvecs[0], np.zeros(n))
    for extra in ({}, dict(sub_iters=1), dict(sub_iters=4), dict(sub_iters=16), dict(return_all=False)):
        r2, rows2, p2 = solve(_classes()[storage](M, b, lam), np.zeros(n), **dict(kw, **extra))
        assert p1 == p2 and np.array_equal(r1.x, r2.x) and np.array_equal(rows1, rows2) and r1.fun == r2.fun, extra
        if dict(kw, **extra)["return_all"]:
            assert np.array_equal(np.asarray(r1.allvecs), np.asarray(r2.allvecs)) and np.array_equal(r1.allfuns, r2.allfuns)
    x = np.random.default_rng(0).standard_normal(n)
    p, q = _classes()[storage](M, b, lam), _classes()[storage](M.copy(), b.copy(), lam)
    assert p.f(x) == q.f(x) and np.array_equal(p.jac_f(x), q.jac_f(x))


@pytest.mark.parametrize("storage", ["csr", "dense"])
def test_snapshot_resume_is_bit_identical(storage, tmp_path):
    """A solve interrupted by snapshot() / from_snapshot continues bit for bit (A x_k, A x_{k-1} are recomputed by the sweep
    that produced them; the loss kernels read them as before)."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    A, b, lam = L.make_logistic(*L.SMALL[0])
    prob = _classes()[storage](L.golden_matrix(A, storage), b, lam)
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
    assert len(ref_rows) == 70 and ref_rows[:, _lib.TR_TRIALS].sum() > 70
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


@pytest.mark.parametrize("which", ["small", "tall"])
def test_concurrent_solves_of_one_sparse_problem_equal_the_solves_alone(which):
    """Two (and more) solves of ONE SparseLogisticL1 at the same time (zfista_amd.replicas.solve_on_streams): the matrix
    handle is shared, the chunk sums of the loss and the segment sums are each solver's - bit for bit the solves alone."""
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.replicas import solve_on_streams

    A, b, lam = L.make_logistic(*(L.SMALL[1] if which == "small" else L.TALL))
    n = A.shape[1]
    prob = _classes()["csr"](A, b, lam)
    ratios = [(0, 0.25), (0.5, 1 / 16), (0.75, 0.25), (0.25, 1 / 64)]
    kws = [dict(lr=1, tol=0.0, max_iter=120, nesterov=True, nesterov_ratio=r, return_all=(k % 2 == 0)) for k, r in enumerate(ratios)]
    alone = [_quiet(minimize_proximal_gradient, *prob.callbacks(), np.zeros(n), **kw) for kw in kws]
    two = solve_on_streams([(prob, np.zeros(n), kw) for kw in kws[:2]], streams=2)
    four = solve_on_streams([(prob, np.zeros(n), kw) for kw in kws], streams=4)
    for a, c in list(zip(alone, two)) + list(zip(alone, four)):
        assert a.nit == c.nit == 120
        assert np.array_equal(a.x, c.x) and a.fun == c.fun
        if a.allfuns is not None:
            assert np.array_equal(np.asarray(a.allfuns), np.asarray(c.allfuns)) and np.array_equal(np.asarray(a.allerrs), np.asarray(c.allerrs))
            assert np.array_equal(np.asarray(a.allvecs), np.asarray(c.allvecs))


# ---- (4) the public interface and the refusals ----------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["csr", "dense"])
def test_callbacks_as_opaque_callables_and_keywords(storage):
    """The callbacks handed to the oracle's solver as opaque callables (the generic use) reproduce the oracle on the closures;
    acceptance="resolved" is refused as for every non-separable problem; the bound method form works."""
    from oracle import cpu_ref
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.problems import NativeProblem, match_native

    A, b, lam = L.make_logistic(*L.SMALL[0])
    n = A.shape[1]
    prob = _classes()[storage](L.golden_matrix(A, storage), b, lam)
    assert isinstance(prob, NativeProblem) and match_native(*prob.callbacks()) is prob
    kw = dict(lr=1, tol=0.0, max_iter=80, nesterov=True, return_all=True)
    got = _quiet(cpu_ref.minimize_proximal_gradient, *prob.callbacks(), np.zeros(n), **kw)
    exp = _quiet(cpu_ref.minimize_proximal_gradient, *L.LogisticL1Ref(A, b, lam).callbacks(), np.zeros(n), **kw)
    assert got.nit == exp.nit == 80 and np.array_equal(got.alltrials, exp.alltrials)
    assert max(rel_err(a, e) for a, e in zip(got.allvecs, exp.allvecs)) <= TOL
    with pytest.raises(ValueError):
        minimize_proximal_gradient(*prob.callbacks(), np.zeros(n), acceptance="resolved")
    with pytest.raises(ValueError):
        prob.f(np.zeros(n + 1))
    with pytest.raises(ValueError):
        prob.minimize_proximal_gradient(np.zeros(n + 1))
    boxed = _classes()[storage](L.golden_matrix(A, storage), b, lam, bounds=(-0.05, 0.3))
    assert boxed.g(np.full(n, 0.4)) == np.inf and boxed.g(np.full(n, 0.1)) == pytest.approx(lam * 0.1 * n, rel=1e-14)
    assert np.array_equal(boxed.prox_wsum_g(2.0, np.array([1.0] + [0.0] * (n - 1)))[:2], [min(max(1.0 - 2 * lam, 0.0), 0.3), 0.0])
    # the method form, and the result fields of the least-squares classes
    res = _quiet(prob.minimize_proximal_gradient, np.zeros(n), nesterov=True, tol=1e-6, lr=1)
    want = _quiet(cpu_ref.minimize_proximal_gradient, *L.LogisticL1Ref(A, b, lam).callbacks(), np.zeros(n), nesterov=True, tol=1e-6, lr=1)
    assert res.success and res.status == 1 and res.nit == want.nit and rel_err(res.x, want.x) <= TOL
    for field in ("x", "fun", "success", "status", "message", "nit", "nfev", "njev", "nit_internal", "time"):
        assert hasattr(res, field) == hasattr(want, field), field
    # a CUDA tensor as A / b, as for LeastSquaresL1
    if storage == "dense":
        import torch

        t = _classes()["dense"](torch.from_numpy(A.toarray()).cuda(), torch.from_numpy(b).cuda(), lam)
        x = np.random.default_rng(1).standard_normal(n)
        assert t.f(x) == prob.f(x) and np.array_equal(t.jac_f(x), prob.jac_f(x))
        with pytest.raises(ValueError):
            _classes()["dense"](torch.from_numpy(A.toarray()).cuda(), torch.from_numpy(np.abs(b) * 0.5).cuda(), lam)


def test_the_library_refuses_resolved_acceptance_and_kind_creator_mismatches():
    from zfista_amd import _lib
    from zfista_amd.engine import DeviceSolver

    A, b, lam = L.make_logistic(*L.SMALL[0])
    options = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=1, max_backtrack_iter=10)
    sparse_prob, dense_prob = _classes()["csr"](A, b, lam), _classes()["dense"](A.toarray(), b, lam)
    for prob in (sparse_prob, dense_prob):
        fields, keep = prob._descriptor()
        DeviceSolver(fields, options, keepalive=keep).close()   # (the descriptor as built is accepted)
        with pytest.raises(_lib.ZfError, match="accept_mode"):
            DeviceSolver(fields, dict(options, accept_mode=_lib.ZF_ACCEPT_RESOLVED), keepalive=keep)
    fields, keep = sparse_prob._descriptor()
    with pytest.raises(_lib.ZfError, match="zf_solver_create_sparse"):   # kind 5 to zf_solver_create_sparse
        DeviceSolver(dict(fields, kind=_lib.ZF_PROBLEM_LOGISTIC_L1), options, keepalive=keep)
    fields, keep = dense_prob._descriptor()
    with pytest.raises(_lib.ZfError, match="zf_solver_create_sparse"):   # kind 6 to zf_solver_create
        DeviceSolver(dict(fields, kind=_lib.ZF_PROBLEM_SPARSE_LOGISTIC_L1), options, keepalive=keep)
    # the least-squares handle of the same matrix serves the logistic kind (one handle type), and the other way round
    from zfista_amd.problems import SparseLeastSquaresL1

    ls = SparseLeastSquaresL1(A, b, lam)
    f2, k2 = ls._descriptor()
    s = DeviceSolver(dict(f2, kind=_lib.ZF_PROBLEM_SPARSE_LOGISTIC_L1), options, keepalive=k2)
    assert s.ls_plan()[0] == 5
    s.close()
