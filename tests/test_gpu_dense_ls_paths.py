"""GPU: every dense least-squares kernel path at the shapes where it is most likely to go wrong.

zf_solver_create picks one of four forms of the gradient A^T r by shape (zf_solver_ls_plan reports which):

  small   zf_ls_small_step_kernel + zf_ls_small_rows_kernel  world 1, n % 32 == 0, m <= 4096, m n <= 2^22
  MFMA    zf_gemvT_partial_mfma_kernel                       n % 32 == 0 otherwise (ZF_GEMV_MFMA=0: VALU)
  VALU2   zf_gemvT_partial_kernel<2>                         n even
  VALU1   zf_gemvT_partial_kernel<1>                         n odd

The column sweeps split the rows into `slices` of `rows_per_slice` rows; the row sweep zf_gemv_rows_kernel loops over
rows once m > 32768.  One case table drives every test here, and every case asserts the form, the slice count and the
rows per slice it claims.  The checks are element by element against a longdouble evaluation with an a-priori fp64
error bound (oracle.problems_ref.ls_longdouble), and iterate by iterate against the CPU oracle."""
import math
import warnings

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-10
U = 2.0 ** -53

SMALL, MFMA, VALU2, VALU1 = 1, 2, 3, 4          # zf_solver_ls_plan out[0]
ROWS_SMALL, ROWS_V2, ROWS_V1 = 1, 2, 3          # out[1]
SWITCHES = ("ZF_LS_SMALL", "ZF_GEMV_MFMA")

# (m, n), scale, switches, expected ls_plan (column form, row form, slices, rows per slice), what the case reaches
CASES = [
    ((5, 4128), 0.5, {}, (SMALL, ROWS_SMALL, 1, 5), "few rows, 129 workgroups"),
    ((1500, 128), 1 / 6, {}, (SMALL, ROWS_SMALL, 63, 24), "row groups: 8-row unroll plus tail"),
    ((4096, 1024), 0.5, {}, (SMALL, ROWS_SMALL, 64, 64), "m and m n exactly at the limit (s_r full)"),
    ((3, 1048576), 0.5, {}, (SMALL, ROWS_SMALL, 1, 3), "32768 workgroups, one row wave"),
    ((4097, 1024), 0.5, {}, (MFMA, ROWS_V2, 64, 65), "one row past the small limit: 64 + 1, last slice 2"),
    ((4096, 1056), 1 / 6, {}, (MFMA, ROWS_V2, 64, 64), "m n just past 2^22"),
    ((3000, 4096), 0.5, {}, (MFMA, ROWS_V2, 64, 47), "32 main + 15 tail rows, last slice 39"),
    ((1200, 4000), 0.5, {}, (MFMA, ROWS_V2, 64, 19), "16 main + 3 tail rows, last slice 3"),
    ((1000, 8192), 0.5, {}, (MFMA, ROWS_V2, 63, 16), "16 rows per slice, last slice 8 (tail only)"),
    ((40000, 64), 1 / 6, {}, (MFMA, ROWS_V2, 64, 625), "624 main + 1 tail rows; the row sweep loops"),
    ((2, 2097184), 0.5, {}, (MFMA, ROWS_V2, 1, 2), "one slice, tail only, 16385 column panels"),
    ((100, 65536), 0.5, {}, (MFMA, ROWS_V2, 13, 8), "the element cap rejects the small form; tail only"),
    ((33, 64), 0.5, {"ZF_LS_SMALL": "0"}, (MFMA, ROWS_V2, 5, 7), "a small shape forced onto the general path"),
    ((3000, 4096), 0.5, {"ZF_GEMV_MFMA": "0"}, (VALU2, ROWS_V2, 64, 47), "8-row unroll + 7-row tail at n % 32 == 0"),
    ((40000, 2), 0.5, {}, (VALU2, ROWS_V2, 64, 625), "the row sweep loops"),
    ((129, 1000), 1 / 6, {}, (VALU2, ROWS_V2, 17, 8), "VALU 16-B, last slice 1"),
    ((40003, 33), 0.5, {}, (VALU1, ROWS_V1, 64, 626), "the row sweep loops, last slice 565"),
    ((1201, 4001), 0.5, {}, (VALU1, ROWS_V1, 64, 19), "VALU scalar, last slice 4"),
    ((1, 1), 0.5, {}, (VALU1, ROWS_V1, 1, 1), "smallest problem"),
]


def _id(case):
    (m, n), _, env, _, _ = case
    return f"{m}x{n}" + "".join(f"-{k}={v}" for k, v in env.items())


IDS = [_id(c) for c in CASES]
# one wide shape of each form for the box tests (tall problems reach rounding level within a few iterations: below)
BOX_CASES = [c for c in CASES if _id(c) in ("5x4128", "1200x4000", "129x1000", "1201x4001")]


def dispatch(m, n, env):
    """zf_solver_create's choice for world 1 (zfista_amd/csrc/zf_solver.hip), restated: the table above must agree."""
    V = 2 if n % 2 == 0 else 1
    panels = -(-(n // V) // 256)                 # column panels of the VALU sweep (ZF_BLOCK threads x V columns)
    slices = max(1, min(-(-2048 // panels), -(-m // 8), 64))
    rps = -(-m // slices)
    slices = -(-m // rps)
    small = n % 32 == 0 and m <= 4096 and m * n <= 1 << 22 and env.get("ZF_LS_SMALL") != "0"
    mfma = n % 32 == 0 and env.get("ZF_GEMV_MFMA") != "0"
    form = SMALL if small else MFMA if mfma else VALU2 if V == 2 else VALU1
    rows = ROWS_SMALL if small else ROWS_V2 if V == 2 else ROWS_V1
    return form, rows, slices, rps


def test_case_table_follows_the_dispatch_rules():
    for case in CASES:
        (m, n), _, env, plan, _ = case
        assert dispatch(m, n, env) == plan, _id(case)
    # every form and every row sweep is in the table
    assert {c[3][0] for c in CASES} == {SMALL, MFMA, VALU2, VALU1}
    assert {c[3][1] for c in CASES} == {ROWS_SMALL, ROWS_V2, ROWS_V1}


class _Dense:
    def __init__(self, m, n):
        import torch

        from oracle import problems_ref as P

        self.A, self.b, self.lam = P.make_plasso(m, n, seed=11, n_informative=max(1, min(20, n // 4)))
        self.A_dev = torch.from_numpy(self.A).cuda()
        self.b_dev = torch.from_numpy(self.b).cuda()
        # ||A||_2^2 as the largest eigenvalue of the smaller Gram matrix (exact to rounding: the step sizes below
        # must lie on the right side of 1/L)
        G = self.A @ self.A.T if m <= n else self.A.T @ self.A
        self.sigma2 = float(np.linalg.eigvalsh(G)[-1])

    def L(self, scale):
        return 2 * scale * self.sigma2


@pytest.fixture(scope="module")
def dense():
    """A, b on the host and the device, once per shape for the whole file (module scope: the ~0.6 GB are given back
    when the file is done)."""
    cache = {}

    def get(m, n):
        if (m, n) not in cache:
            cache[(m, n)] = _Dense(m, n)
        return cache[(m, n)]

    yield get
    cache.clear()


@pytest.fixture
def switches(monkeypatch):
    """Set exactly the case's ZF_* switches (the others unset, whatever the environment holds)."""

    def apply(env):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)

    return apply


@pytest.fixture
def solve(monkeypatch):
    """minimize_proximal_gradient on the native path; returns (result, ls_plan of the solver that ran it)."""
    from zfista_amd import minimize_proximal_gradient, proximal_gradient as pg

    plans = []

    class _Recorded(pg.NativeRun):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            plans.append(self.solver.ls_plan())

    monkeypatch.setattr(pg, "NativeRun", _Recorded)

    def run(prob, x0, **kw):
        del plans[:]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = minimize_proximal_gradient(*prob.callbacks(), x0, **kw)
        assert len(plans) == 1, "the solve did not run on the native path"
        return res, plans[0]

    return run


def _ld_ref(A, b, x, scale, grad=True):
    from oracle import problems_ref as P

    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip(f"np.longdouble has only {np.finfo(np.longdouble).nmant} mantissa bits on this host: no reference "
                    "more exact than the fp64 kernels")
    return P.ls_longdouble(A, b, x, scale, grad=grad)


def _fista_lr(D, m, n, scale):
    """lr = 1 with backtracking on small shapes, 0.9 / L on large ones (no marginal trial)."""
    return 1.0 if m * n <= 1 << 18 else 0.9 / D.L(scale)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_gradient_element_by_element(case, dense, switches, solve):
    """ISTA, lam = 0, one iteration with lr = 2^-k <= 1/(2L): the first trial is accepted and x1 = x0 - lr grad f(x0)
    with a single rounding, so (x0 - x1) / lr is the column sweep's gradient.  It, f(x0) (the initial row sweep) and
    f(x1) (the row sweep inside the loop) are each checked against the longdouble value within the a-priori bound of
    an fp64 evaluation."""
    from zfista_amd.problems import LeastSquaresL1

    (m, n), scale, env, plan, _ = case
    D = dense(m, n)
    switches(env)
    x0 = np.random.default_rng(m * 7919 + n).standard_normal(n)
    lr = 2.0 ** -math.ceil(math.log2(2 * D.L(scale)))
    assert lr <= 1 / (2 * D.L(scale))
    prob = LeastSquaresL1(D.A_dev, D.b_dev, 0.0, scale=scale)
    res, got = solve(prob, x0, lr=lr, tol=0.0, max_iter=1, nesterov=False, return_all=True)
    assert got == plan
    assert res.nit == 1 and len(res.allvecs) == 2 and len(res.allfuns) == 2
    assert np.array_equal(res.allvecs[0], x0)
    x1 = np.asarray(res.allvecs[1])

    f0, g0, f0_bound, g0_bound = _ld_ref(D.A, D.b, x0, scale)
    x0l, x1l = x0.astype(np.longdouble), x1.astype(np.longdouble)
    g_kernel = (x0l - x1l) / np.longdouble(lr)
    bound = g0_bound + U * (np.abs(x0) + np.abs(x1)) / lr   # + the rounding of x0 - lr grad
    # the bound means something here: leaving one row out of one column (the last row: where tails go wrong) would
    # exceed it by orders of magnitude in almost every column
    r_last = float(D.A[-1] @ x0 - D.b[-1])
    drop = 2 * scale * np.abs(D.A[-1] * r_last)
    assert np.median(drop / bound) > 1e3
    err = np.abs(g_kernel - g0).astype(np.float64)
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, (f"{bad.size} of {n} gradient elements outside the fp64 bound, first {bad[:8]}: "
                           f"error / bound up to {np.max(err / bound):.3g}")

    assert abs(np.longdouble(res.allfuns[0]) - f0) <= f0_bound, (float(res.allfuns[0]), float(f0), f0_bound)
    f1, _, f1_bound, _ = _ld_ref(D.A, D.b, x1, scale, grad=False)
    assert abs(np.longdouble(res.allfuns[1]) - f1) <= f1_bound, (float(res.allfuns[1]), float(f1), f1_bound)


def _check_against_oracle(res, exp, max_iter):
    assert res.nit == exp.nit == max_iter
    assert len(res.allvecs) == len(exp.allvecs)
    for k, (a, e) in enumerate(zip(res.allvecs, exp.allvecs)):
        assert rel_err(a, e) <= TOL, k
    np.testing.assert_allclose(res.allfuns, exp.allfuns, rtol=TOL)
    # err = max|x+ - y|: a difference of two iterates, each within TOL of the oracle's
    xmax = max(float(np.max(np.abs(e))) for e in exp.allvecs)
    np.testing.assert_allclose(res.allerrs, exp.allerrs, rtol=1e-9, atol=2 * TOL * xmax)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_short_fista_solve_vs_oracle(case, dense, switches, solve):
    """FISTA with lam > 0 against the CPU oracle, every iterate: A y by linearity from the cached A x_k, A x_{k-1}
    (the s ring) on top of both sweeps.  30 iterations; 10 for tall A, which is well conditioned: its FISTA reaches
    rounding level within 11 - 25 iterations here, and the line search would then decide on rounding noise."""
    from oracle import cpu_ref, problems_ref as P
    from zfista_amd.problems import LeastSquaresL1

    (m, n), scale, env, plan, _ = case
    D = dense(m, n)
    switches(env)
    x0 = 0.1 * np.random.default_rng(n * 31 + m).standard_normal(n)
    K = 30 if m <= n else 10
    kw = dict(lr=_fista_lr(D, m, n, scale), nesterov=True, tol=0.0, max_iter=K, return_all=True)
    res, got = solve(LeastSquaresL1(D.A_dev, D.b_dev, D.lam, scale=scale), x0, **kw)
    assert got == plan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = cpu_ref.minimize_proximal_gradient(*P.LeastSquaresL1Ref(D.A, D.b, D.lam, scale=scale).callbacks(), x0,
                                                 **kw)
    _check_against_oracle(res, exp, K)


@pytest.mark.parametrize("bounds", [(-0.05, 0.08), (0.01, 0.5)], ids=["active", "excludes-0"])
@pytest.mark.parametrize("nesterov", [False, True], ids=["ista", "fista"])
@pytest.mark.parametrize("case", BOX_CASES, ids=[_id(c) for c in BOX_CASES])
def test_box_vs_oracle(case, nesterov, bounds, dense, switches, solve):
    """A least-squares problem with a box, one shape of each form (the small form: both BOX=true instances of its step
    kernel).  (-0.05, 0.08) is active on many coordinates; (0.01, 0.5) excludes 0, so a soft-thresholded 0 is clipped
    up to 0.01.  x0 lies inside the box (the oracle's g is inf outside it)."""
    from oracle import cpu_ref, problems_ref as P
    from zfista_amd.problems import LeastSquaresL1

    (m, n), scale, env, plan, _ = case
    D = dense(m, n)
    switches(env)
    lo, hi = bounds
    x0 = np.random.default_rng(n + 5).uniform(lo, hi, n)
    K = 25
    kw = dict(lr=_fista_lr(D, m, n, scale), nesterov=nesterov, tol=0.0, max_iter=K, return_all=True)
    res, got = solve(LeastSquaresL1(D.A_dev, D.b_dev, D.lam, scale=scale, bounds=bounds), x0, **kw)
    assert got == plan
    ref = P.LeastSquaresL1Ref(D.A, D.b, D.lam, scale=scale, bounds=bounds)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = cpu_ref.minimize_proximal_gradient(*ref.callbacks(), x0, **kw)
    _check_against_oracle(res, exp, K)
    X = np.asarray(res.allvecs)
    assert X.min() >= lo and X.max() <= hi
    assert np.count_nonzero((X[1:] == lo) | (X[1:] == hi)) >= 30, "the box should be active"
    if lo > 0:
        assert np.count_nonzero(X[1:] == lo) >= 30, "soft-thresholded zeros should be clipped up to lo"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bit_reproducible(case, dense, switches, solve):
    """No atomics in any sweep, and every reduction in a fixed order: the same solve twice gives the same bits."""
    from zfista_amd.problems import LeastSquaresL1

    (m, n), scale, env, plan, _ = case
    D = dense(m, n)
    switches(env)
    x0 = 0.1 * np.random.default_rng(n * 31 + m).standard_normal(n)
    kw = dict(lr=_fista_lr(D, m, n, scale), nesterov=True, tol=0.0, max_iter=20, return_all=True)
    runs = [solve(LeastSquaresL1(D.A_dev, D.b_dev, D.lam, scale=scale), x0, **kw) for _ in range(2)]
    (r1, p1), (r2, p2) = runs
    assert p1 == p2 == plan
    assert r1.nit == r2.nit == 20
    assert np.array_equal(np.asarray(r1.allvecs), np.asarray(r2.allvecs))
    assert np.array_equal(np.asarray(r1.allfuns), np.asarray(r2.allfuns))
    assert np.array_equal(r1.x, r2.x)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (40003, 33), (40000, 2), (3000, 4096), (2, 2097184)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_ls_eval_vs_longdouble(shape, dense):
    """prob.f / prob.jac_f (zf_ls_eval: the VALU row sweep, r = s - b, the VALU column sweep and the slice combine)
    element by element against the longdouble value."""
    from zfista_amd.problems import LeastSquaresL1

    m, n = shape
    D = dense(m, n)
    x = np.random.default_rng(m + 3 * n).standard_normal(n)
    prob = LeastSquaresL1(D.A_dev, D.b_dev, D.lam, scale=0.5)
    f, g, f_bound, g_bound = _ld_ref(D.A, D.b, x, 0.5)
    fv = prob.f(x)
    assert abs(np.longdouble(fv) - f) <= f_bound, (float(fv), float(f), f_bound)
    gv = prob.jac_f(x)
    err = np.abs(gv.astype(np.longdouble) - g).astype(np.float64)
    bad = np.flatnonzero(err > g_bound)
    assert bad.size == 0, f"{bad.size} of {n} elements outside the fp64 bound, first {bad[:8]}"
