"""GPU: dense margins problems whose matrix is stored in fp32 (``matrix_dtype="float32"``, ``with_matrix_dtype``).

The fp32 sweeps (csrc/zf_kernels_gemv_f32.h) widen every element exactly and compute in fp64, so an fp32 problem is the
fp64 problem on A64 = float64(float32(A)) with sums in another order: everything that pins the fp64 sweeps applies with A64
on the reference side - the CPU oracle at 1e-10, the a-priori longdouble bounds of oracle.problems_ref.ls_longdouble.  One
case table (tests/f32_cases.py) drives the tests; every case asserts the kernel forms, the slice count and the rows per
slice it claims.  The problems are built from the matrix AS GENERATED (unrounded fp64): the library rounds, and
tests/test_f32_cases.py shows that an implementation which kept the fp64 matrix would miss these references by 1e3 TOL."""
import math
import warnings

import numpy as np
import pytest

import f32_cases as F
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL, U = F.TOL, F.U
BASE = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=100000, max_backtrack_iter=100, nesterov=True,
            nesterov_ratio=(0, 0.25), deprecated=False, return_all=False, verbose=False)


class _Case:
    def __init__(self, case):
        import torch

        from zfista_amd.problems import LeastSquaresL1

        (self.m, self.n), self.scale, _, self.plan, _ = case
        self.D = D = F.make(case)
        self.b_dev = torch.from_numpy(D.b).cuda()
        # rounded by the library, once per shape; every test takes with_lam siblings of this problem
        self.prob = LeastSquaresL1(D.A, self.b_dev, D.lam, scale=self.scale, matrix_dtype="float32")


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(case):
        if case[0] not in cache:
            cache[case[0]] = _Case(case)
        return cache[case[0]]

    yield get
    cache.clear()


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


def _walk(prob, passes, opts=None, resume=None, snapshot_at=None, x0=None):
    """`passes` chunks of ONE pass each: (nit, lr, trials) after every pass, the final x, the plan, a snapshot."""
    from zfista_amd.proximal_gradient import NativeRun

    o = dict(BASE, **(opts or {}))
    x0 = np.zeros(prob.n_features) if x0 is None else x0
    run = NativeRun(prob, x0, o) if resume is None else NativeRun.from_snapshot(prob, resume, o)
    seq, state = [], None
    for k in range(passes):
        run.advance(1)
        ctl = run.solver.ctl
        seq.append((int(ctl.nit), float(ctl.lr), int(ctl.total_trials)))
        if snapshot_at == k:
            state = run.snapshot()
    ctl, _ = run.solver.poll()
    return dict(seq=seq, x=run.solver.get_x(), F=float(ctl.F_old), plan=run.solver.ls_plan(), state=state)


# ---- (1) one gradient ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", F.CASES, ids=F.IDS)
def test_one_gradient_element_by_element(case, cases, solve):
    """ISTA, lam = 0, one iteration with lr = 2^-k <= 1/(2L): the first trial is accepted and x1 = x0 - lr grad f(x0) with a
    single rounding, so (x0 - x1) / lr is the fp32 column sweep's gradient.  It, f(x0) (the initial fp32 row sweep) and f(x1)
    (the row sweep inside the loop) are each inside the a-priori bound of an fp64 evaluation on A64."""
    from oracle import problems_ref as P

    C = cases(case)
    D, m, n, scale = C.D, C.m, C.n, C.scale
    x0 = np.random.default_rng(m * 7919 + n).standard_normal(n)
    lr = 2.0 ** -math.ceil(math.log2(2 * D.L(scale)))
    assert lr <= 1 / (2 * D.L(scale))
    res, got = solve(C.prob.with_lam(0.0), x0, lr=lr, tol=0.0, max_iter=1, nesterov=False, return_all=True)
    assert got == C.plan
    assert res.nit == 1 and len(res.allvecs) == 2 and len(res.allfuns) == 2
    assert np.array_equal(res.allvecs[0], x0)
    x1 = np.asarray(res.allvecs[1])

    f0, g0, f0_bound, g0_bound = P.ls_longdouble(D.A64, D.b, x0, scale)
    x0l, x1l = x0.astype(np.longdouble), x1.astype(np.longdouble)
    g_kernel = (x0l - x1l) / np.longdouble(lr)
    bound = g0_bound + U * (np.abs(x0) + np.abs(x1)) / lr   # + the rounding of x0 - lr grad
    # the bound means something here: leaving one row out of one column (the last row: where tails go wrong) would exceed it
    # by orders of magnitude in almost every column
    r_last = float(D.A64[-1] @ x0 - D.b[-1])
    drop = 2 * scale * np.abs(D.A64[-1] * r_last)
    assert np.median(drop / bound) > 1e3
    err = np.abs(g_kernel - g0).astype(np.float64)
    bad = np.flatnonzero(err > bound)
    print(f"{F.case_id(case)}: gradient error / bound up to {np.max(err / bound):.3g}")
    assert bad.size == 0, (f"{bad.size} of {n} gradient elements outside the fp64 bound, first {bad[:8]}: "
                           f"error / bound up to {np.max(err / bound):.3g}")
    assert abs(np.longdouble(res.allfuns[0]) - f0) <= f0_bound, (float(res.allfuns[0]), float(f0), f0_bound)
    f1, _, f1_bound, _ = P.ls_longdouble(D.A64, D.b, x1, scale, grad=False)
    assert abs(np.longdouble(res.allfuns[1]) - f1) <= f1_bound, (float(res.allfuns[1]), float(f1), f1_bound)


# ---- (2) FISTA against the oracle ------------------------------------------------------------------------------------------------
def _check_against_oracle(res, exp, max_iter):
    assert res.nit == exp.nit == max_iter
    assert len(res.allvecs) == len(exp.allvecs)
    worst = 0.0
    for k, (a, e) in enumerate(zip(res.allvecs, exp.allvecs)):
        worst = max(worst, rel_err(a, e))
        assert rel_err(a, e) <= TOL, (k, rel_err(a, e))
    np.testing.assert_allclose(res.allfuns, exp.allfuns, rtol=TOL)
    # err = max|x+ - y|: a difference of two iterates, each within TOL of the oracle's
    xmax = max(float(np.max(np.abs(e))) for e in exp.allvecs)
    np.testing.assert_allclose(res.allerrs, exp.allerrs, rtol=1e-9, atol=2 * TOL * xmax)
    return worst


@pytest.mark.parametrize("variant", F.VARIANTS)
@pytest.mark.parametrize("case", F.CASES, ids=F.IDS)
def test_short_fista_solve_vs_oracle(case, variant, cases, solve):
    """FISTA with lam > 0 against the CPU oracle ON A64, every iterate, in both variants of tests/f32_cases.py: near-lam-max -
    in which an unrounded matrix would miss by 1e3 TOL - and dense (every column takes part in A x)."""
    from oracle import cpu_ref, problems_ref as P

    C = cases(case)
    D, m, n, scale = C.D, C.m, C.n, C.scale
    lam, x0 = F.fista_problem(D, m, n, scale, variant)
    kw = F.fista_kw(D, m, n, scale, variant)
    res, got = solve(C.prob.with_lam(lam), x0, **kw)
    assert got == C.plan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = cpu_ref.minimize_proximal_gradient(*P.LeastSquaresL1Ref(D.A64, D.b, lam, scale=scale).callbacks(), x0, **kw)
    worst = _check_against_oracle(res, exp, kw["max_iter"])
    print(f"{F.case_id(case)} {variant}: worst rel_err {worst:.3g}")


# ---- (3) bit reproducibility -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", F.CASES, ids=F.IDS)
def test_bit_reproducible(case, cases, solve):
    """No atomics in either fp32 sweep, every reduction in a fixed order: the same solve twice gives the same bits."""
    C = cases(case)
    D, m, n, scale = C.D, C.m, C.n, C.scale
    kw = dict(F.fista_kw(D, m, n, scale), max_iter=20)
    (r1, p1), (r2, p2) = [solve(C.prob, F.fista_x0(m, n), **kw) for _ in range(2)]
    assert p1 == p2 == C.plan
    assert r1.nit == r2.nit == 20
    assert np.array_equal(np.asarray(r1.allvecs), np.asarray(r2.allvecs))
    assert np.array_equal(np.asarray(r1.allfuns), np.asarray(r2.allfuns))
    assert np.array_equal(r1.x, r2.x)


# ---- (4) f / jac_f ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (70003, 33), (70000, 4), (3000, 4096)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_f32_eval_vs_longdouble(shape, cases):
    """prob.f / prob.jac_f (zf_f32_eval: the fp32 row sweep, r = s - b, the fp32 column sweep and the slice combine) element by
    element against the longdouble value on A64."""
    from oracle import problems_ref as P

    C = cases(F.BY_SHAPE[shape])
    D, (m, n) = C.D, shape
    x = np.random.default_rng(m + 3 * n).standard_normal(n)
    prob = C.prob.with_lam(D.lam)
    prob.scale = 0.5
    f, g, f_bound, g_bound = P.ls_longdouble(D.A64, D.b, x, 0.5)
    fv = prob.f(x)
    assert abs(np.longdouble(fv) - f) <= f_bound, (float(fv), float(f), f_bound)
    gv = prob.jac_f(x)
    err = np.abs(gv.astype(np.longdouble) - g).astype(np.float64)
    bad = np.flatnonzero(err > g_bound)
    assert bad.size == 0, f"{bad.size} of {n} elements outside the fp64 bound, first {bad[:8]}"


# ---- (5) the other losses ---------------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(129, 1000), (1201, 4001)]   # V4, V1


def _loss_data(C, loss):
    """(A as generated, A64, b) for a loss on a case's matrix.  Poisson: the matrix times 2^-k (exact in both formats), so
    that the margins stay in the range of exp; counts drawn from the model."""
    D, n = C.D, C.n
    if loss == "logistic":
        return D.A, D.A64, np.where(D.b >= 0, 1.0, -1.0)
    if loss == "huber":
        return D.A, D.A64, D.b
    s = 2.0 ** -math.ceil(math.log2(math.sqrt(n) / 4))   # (margins of the model: standard deviation about 1)
    rng = np.random.default_rng(n + 17)
    xt = np.where(rng.random(n) < 0.05, rng.standard_normal(n), 0.0)
    return D.A * s, D.A64 * s, rng.poisson(np.exp((D.A64 * s) @ xt)).astype(np.float64)


def _loss_pair(loss, A, A64, b, lam, **kw):
    """(the fp32 problem built from A as generated, its fp64 class on A64)."""
    from zfista_amd import problems as Z

    if loss == "logistic":
        return Z.LogisticL1(A, b, lam, **kw).with_matrix_dtype("float32"), Z.LogisticL1(A64, b, lam, **kw)
    if loss == "huber":
        delta = 0.5 * float(np.std(b))
        return Z.HuberL1(A, b, lam, delta, matrix_dtype="float32", **kw), Z.HuberL1(A64, b, lam, delta, **kw)
    return Z.PoissonL1(A, b, lam, matrix_dtype="float32", **kw), Z.PoissonL1(A64, b, lam, **kw)


def _compare_walks(p32, p64, plan, passes=12, opts=None):
    assert p32.matrix_dtype == "float32" and p64.matrix_dtype == "float64"
    a, e = _walk(p32, passes, opts), _walk(p64, passes, opts)
    assert a["plan"] == plan and e["plan"][0] in (2, 3, 4)
    assert a["seq"] == e["seq"], "the accepted iterations, step sizes and trial counts must agree pass by pass"
    assert a["seq"][-1][2] > a["seq"][-1][0] > 0, "the case must backtrack and accept"
    assert np.any(e["x"] != 0)
    assert rel_err(a["x"], e["x"]) <= TOL, rel_err(a["x"], e["x"])
    assert abs(a["F"] - e["F"]) <= TOL * abs(e["F"])
    return a, e


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("loss", ["logistic", "huber", "poisson"])
def test_other_losses_vs_their_fp64_class(loss, shape, cases):
    """LogisticL1(...).with_matrix_dtype("float32"), HuberL1 and PoissonL1 with the keyword against their own fp64 class built
    on A64: the same accept / reject sequence, iterates to 1e-10, f and jac_f (zf_f32_eval) to 1e-10."""
    C = cases(F.BY_SHAPE[shape])
    A, A64, b = _loss_data(C, loss)
    lam0 = _loss_pair(loss, A, A64, b, 1.0)[1].lam_max()
    p32, p64 = _loss_pair(loss, A, A64, b, 0.3 * float(lam0))
    # (the logistic sibling is made on the device from the fp64 upload of A: the same rounding as the host's)
    assert np.array_equal(p32.A.cpu().numpy().astype(np.float64), A64)
    a, _ = _compare_walks(p32, p64, C.plan)
    x = a["x"]
    assert abs(p32.f(x) - p64.f(x)) <= TOL * abs(p64.f(x))
    assert rel_err(p32.jac_f(x), p64.jac_f(x)) <= TOL


def test_weights_factors_and_box_together(cases):
    """sample_weight (with zeros), penalty_factor (an unpenalised column) and a box on one fp32 Huber problem."""
    C = cases(F.BY_SHAPE[(1201, 4001)])
    A, A64, b = _loss_data(C, "huber")
    rng = np.random.default_rng(5)
    w = np.where(rng.random(C.m) < 0.1, 0.0, rng.uniform(0.5, 2.0, C.m))
    p = rng.uniform(0.5, 2.0, C.n)
    p[0] = 0.0
    kw = dict(sample_weight=w, penalty_factor=p, bounds=(-0.05, 0.08))
    p32, p64 = _loss_pair("huber", A, A64, b, C.D.lam, **kw)
    a, _ = _compare_walks(p32, p64, C.plan)
    assert a["x"].min() >= -0.05 and a["x"].max() <= 0.08 and np.count_nonzero((a["x"] == -0.05) | (a["x"] == 0.08)) > 0
    sib = p32.with_lam(0.5 * C.D.lam)
    assert sib.matrix_dtype == "float32" and sib.A is p32.A and sib._w is p32._w and sib._pf is p32._pf


def test_elastic_net(cases):
    """l2 > 0 on an fp32 Poisson problem and on a logistic sibling (with_penalty), and the ten-value certificate."""
    C = cases(F.BY_SHAPE[(129, 1000)])
    for loss in ("poisson", "logistic"):
        A, A64, b = _loss_data(C, loss)
        lam0 = float(_loss_pair(loss, A, A64, b, 1.0)[1].lam_max())
        p32, p64 = _loss_pair(loss, A, A64, b, 0.3 * lam0)
        p32, p64 = p32.with_penalty(0.3 * lam0, 0.05), p64.with_penalty(0.3 * lam0, 0.05)
        a, _ = _compare_walks(p32, p64, C.plan)
        g32, g64 = p32.duality_gap(a["x"]), p64.duality_gap(a["x"])
        assert g64.g_l2 > 0
        for key in ("primal", "dual", "g_l2", "ridge_gap"):
            assert abs(getattr(g32, key) - getattr(g64, key)) <= TOL * abs(getattr(g64, key)), key
        assert abs(g32.gap - g64.gap) <= TOL * abs(g64.primal)


# ---- (6) the duality gap ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(129, 1000), (1200, 4002), (1201, 4001)], ids=lambda s: f"{s[0]}x{s[1]}")   # V4, V2, V1
def test_duality_gap_lam_max_and_gap_tol(shape, cases):
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.problems import LeastSquaresL1

    C = cases(F.BY_SHAPE[shape])
    D = C.D
    p32 = C.prob
    p64 = LeastSquaresL1(D.A64, C.b_dev, D.lam, scale=C.scale)
    assert abs(p32.lam_max() - p64.lam_max()) <= TOL * p64.lam_max()
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=400, gap_tol=1e-4 * float(p64.f(np.zeros(C.n))), gap_every=5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r32 = minimize_proximal_gradient(*p32.callbacks(), np.zeros(C.n), **kw)
        r64 = minimize_proximal_gradient(*p64.callbacks(), np.zeros(C.n), **kw)
    assert r32.dual_gap_checks == r64.dual_gap_checks >= 1 and r32.nit == r64.nit
    assert r32.dual_gap <= kw["gap_tol"] and r32.success
    assert rel_err(r32.x, r64.x) <= TOL
    for x in (r32.x, np.random.default_rng(3).standard_normal(C.n) * 0.01):
        g32, g64 = p32.duality_gap(x), p64.duality_gap(x)
        for key in ("primal", "dual", "f", "g_l1", "grad_inf", "alpha"):
            assert abs(getattr(g32, key) - getattr(g64, key)) <= TOL * abs(getattr(g64, key)), (key, g32, g64)
        assert abs(g32.gap - g64.gap) <= TOL * abs(g64.primal), (g32, g64)
        assert g32.gap >= 0
    # the live solver's certificate is the standalone evaluation's, bit for bit (the same fp32 sweeps in the same order)
    from zfista_amd.proximal_gradient import NativeRun

    run = NativeRun(p32, np.zeros(C.n), dict(BASE))
    run.advance(3)
    live, alone = run.duality_gap(), p32.duality_gap(run.solver.get_x())
    assert all(getattr(live, k) == getattr(alone, k) for k in live.__slots__), (live, alone)


# ---- (7) storage ------------------------------------------------------------------------------------------------------------------
def test_storage_and_siblings(cases):
    import torch

    from zfista_amd.problems import HuberL1, LeastSquaresL1, LogisticL1

    C = cases(F.BY_SHAPE[(129, 1000)])
    D = C.D
    assert C.prob.A.dtype == torch.float32 and C.prob.matrix_dtype == "float32"
    assert np.array_equal(C.prob.A.cpu().numpy(), D.A32), "an fp64 host matrix is rounded to nearest"
    t = torch.from_numpy(D.A32).cuda()
    for dt in ("float32", np.float32, torch.float32):
        adopted = LeastSquaresL1(t, C.b_dev, D.lam, matrix_dtype=dt)
        assert adopted.A.data_ptr() == t.data_ptr() and adopted.A.dtype == torch.float32, "a float32 CUDA tensor is taken as it is"
    from_dev64 = HuberL1(torch.from_numpy(D.A).cuda(), C.b_dev, D.lam, 1.0, matrix_dtype="float32")
    assert torch.equal(from_dev64.A, t), "an fp64 device tensor is rounded to nearest"
    for dt in (None, "float64", np.float64, torch.float64):
        p64 = LeastSquaresL1(D.A64, C.b_dev, D.lam, matrix_dtype=dt)
        assert p64.matrix_dtype == "float64" and p64.A.dtype == torch.float64
    w = np.linspace(0.5, 1.5, C.m)
    for sib in (adopted.with_lam(0.1), adopted.with_sample_weight(w), adopted.with_penalty(0.1, 0.2),
                adopted.with_penalty_factor(np.ones(C.n)), adopted.with_matrix_dtype("float32")):
        assert sib.matrix_dtype == "float32" and sib.A is adopted.A and sib._descriptor()[0]["matrix_f32"] == t.data_ptr()
    wide = adopted.with_sample_weight(w).with_matrix_dtype("float64")
    assert wide.matrix_dtype == "float64" and wide.A.dtype == torch.float64 and np.array_equal(wide.A.cpu().numpy(), D.A64)
    assert wide._w is not None and "matrix_f32" not in wide._descriptor()[0]
    log64 = LogisticL1(D.A, np.where(D.b >= 0, 1.0, -1.0), 0.1)
    log32 = log64.with_matrix_dtype(torch.float32)
    assert log32.matrix_dtype == "float32" and log32.b is log64.b and log32.A.dtype == torch.float32 and log64.A.dtype == torch.float64
    assert log32.A.data_ptr() != log64.A.data_ptr() and torch.equal(log32.A, t)


def test_snapshot_resumes_to_the_bits(cases):
    C = cases(F.BY_SHAPE[(129, 1000)])
    plain = _walk(C.prob, 12, snapshot_at=5)
    assert plain["plan"] == C.plan and plain["seq"][-1][2] > plain["seq"][-1][0] > 0
    resumed = _walk(C.prob, 6, resume=plain["state"])
    assert resumed["plan"] == C.plan
    assert np.array_equal(resumed["x"], plain["x"]) and resumed["seq"] == plain["seq"][6:] and resumed["F"] == plain["F"]


def test_remainder_acceptance_and_l1_path(cases):
    """acceptance="remainder" and l1_path run through siblings and the descriptor: against the fp64 class on A64."""
    from zfista_amd.path import l1_path
    from zfista_amd.problems import LeastSquaresL1

    C = cases(F.BY_SHAPE[(129, 1000)])
    p64 = LeastSquaresL1(C.D.A64, C.b_dev, C.D.lam, scale=C.scale)
    _compare_walks(C.prob, p64, C.plan, opts=dict(acceptance="remainder"))
    lams = [0.5 * float(p64.lam_max()), 0.2 * float(p64.lam_max())]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        path32 = l1_path(C.prob, lams, gap_tol=1e-6, max_iter=300)
        path64 = l1_path(p64, lams, gap_tol=1e-6, max_iter=300)
    for a, e in zip(path32, path64):
        assert a.nit == e.nit and rel_err(a.x, e.x) <= TOL


# ---- (8) refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(cases):
    import torch

    from zfista_amd import _lib
    from zfista_amd.path import l1_path
    from zfista_amd.problems import HuberL1, LeastSquaresL1, LogisticL1, PoissonL1
    from zfista_amd.screening import solve_screened

    C = cases(F.BY_SHAPE[(129, 1000)])
    D, p32 = C.D, C.prob
    x = np.zeros(C.n)
    for call in (p32.column_norms, lambda: p32.screen(x), lambda: p32.restrict(np.arange(10)),
                 lambda: solve_screened(p32, x, 1e-6), lambda: l1_path(p32, [D.lam], screen=True)):
        with pytest.raises(ValueError, match="fp32"):
            call()
    log32 = LogisticL1(D.A32.astype(np.float64), np.where(D.b >= 0, 1.0, -1.0), 0.1).with_matrix_dtype("float32")
    with pytest.raises(ValueError, match="fp32"):
        log32.column_norms()
    t32 = torch.from_numpy(D.A32).cuda()
    for make in (lambda: LeastSquaresL1(t32, C.b_dev, D.lam), lambda: HuberL1(t32, C.b_dev, D.lam, 1.0),
                 lambda: PoissonL1(t32, np.ones(C.m), D.lam), lambda: LogisticL1(t32, np.ones(C.m), D.lam)):
        with pytest.raises(TypeError, match="float64"):
            make()
    with pytest.raises(ValueError, match="matrix_dtype"):
        LeastSquaresL1(D.A, C.b_dev, D.lam, matrix_dtype="float16")
    with pytest.raises(ValueError, match="matrix_dtype"):
        p32.with_matrix_dtype("bfloat16")
    with pytest.raises(ValueError, match="group="):
        LeastSquaresL1(D.A, C.b_dev, D.lam, group=object(), matrix_dtype="float32")
    # a value that is not finite after the rounding: found on the host for a host matrix, on the device for a device one
    big = D.A.copy()
    big[3, 5] = 1e39
    nan = D.A32.copy()
    nan[0, 0] = np.nan
    for bad in (big, torch.from_numpy(big).cuda(), torch.from_numpy(nan).cuda(), nan):
        with pytest.raises(ValueError, match="finite"):
            LeastSquaresL1(bad, C.b_dev, D.lam, matrix_dtype="float32")
    with pytest.raises(ValueError, match="finite"):
        LeastSquaresL1(big, C.b_dev, D.lam).with_matrix_dtype("float32")
    # the C entry refuses what it is documented to refuse
    lib = _lib.require_gpu()
    import ctypes as Ct

    import evaldesc as E

    out, xz = np.zeros(10), np.zeros(C.n)
    fields = dict(A32=p32.A.data_ptr(), b=C.b_dev.data_ptr(), m_rows=C.m, n=C.n, scale=0.5, lam=0.1)
    rc = E.gap(E.desc(**fields, p=C.b_dev.data_ptr(), l2=0.5), Ct.c_void_p(_lib.ptr(xz)), Ct.c_void_p(_lib.ptr(out)), 10)
    assert rc == -2 and b"zf_margins_gap" in lib.zf_last_error() and b"penalty factors and l2" in lib.zf_last_error()
    f = Ct.c_double(0.0)
    rc = E.point(E.desc(**{**fields, "A32": p32.A.data_ptr() + 4}), Ct.c_void_p(_lib.ptr(xz)), Ct.byref(f))
    assert rc == -2 and b"aligned" in lib.zf_last_error()
    rc = E.point(E.desc(**fields, loss=7), Ct.c_void_p(_lib.ptr(xz)), Ct.byref(f))
    assert rc == -2 and b"ZF_LOSS" in lib.zf_last_error()


def test_the_setter_refuses_what_it_must(cases):
    """zf_solver_set_matrix_f32: ZF_ERR_ARG for a NULL or misaligned pointer, another kind, and an initialised solver."""
    import ctypes as Ct

    from zfista_amd.engine import DeviceSolver
    from zfista_amd.problems import DiagQuadL1
    from zfista_amd.proximal_gradient import NativeRun

    C = cases(F.BY_SHAPE[(129, 1000)])
    p64 = C.prob.with_matrix_dtype("float64")
    a32 = C.prob.A.data_ptr()
    options = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=10, max_backtrack_iter=10, nesterov=1, deprecated=0,
                   accept_mode=0, sub_iters=0)
    run = NativeRun(p64, np.zeros(C.n), dict(BASE))
    lib = run.solver.lib
    assert lib.zf_solver_set_matrix_f32(run.solver.handle, Ct.c_void_p(a32)) == -2 and b"before zf_solver_enqueue_init" in lib.zf_last_error()
    assert run.solver.ls_plan()[0] in (2, 3, 4)
    fields, keep = DiagQuadL1(np.ones(64), np.zeros(64), 0.1)._descriptor()
    diag = DeviceSolver(fields, options, keepalive=keep)
    assert lib.zf_solver_set_matrix_f32(diag.handle, Ct.c_void_p(a32)) == -2 and b"only for" in lib.zf_last_error()
    fields, keep = p64._descriptor()
    fresh = DeviceSolver(fields, options, keepalive=keep + (C.prob.A,))
    assert lib.zf_solver_set_matrix_f32(fresh.handle, None) == -2
    assert lib.zf_solver_set_matrix_f32(fresh.handle, Ct.c_void_p(a32 + 4)) == -2 and b"aligned" in lib.zf_last_error()
    assert fresh.ls_plan()[0] in (2, 3, 4)
    assert lib.zf_solver_set_matrix_f32(fresh.handle, Ct.c_void_p(a32)) == 0
    assert fresh.ls_plan() == C.plan


# ---- (9) the fp64 classes run what they ran ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 4128), (129, 1000), (3000, 4096)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_fp64_solves_are_untouched(shape, cases, solve):
    """matrix_dtype=None: the same ls_plan as the fp64 rule gives and the same bits before and after the fp32 path ran."""
    from zfista_amd.problems import LeastSquaresL1

    C = cases(F.BY_SHAPE[shape])
    D, (m, n) = C.D, shape
    kw = dict(F.fista_kw(D, m, n, C.scale), max_iter=15)
    x0 = F.fista_x0(m, n)
    p64 = LeastSquaresL1(D.A64, C.b_dev, D.lam, scale=C.scale)
    before, plan_before = solve(p64, x0, **kw)
    small = n % 32 == 0 and m <= 4096 and m * n <= 1 << 22
    assert plan_before[0] == (1 if small else 2 if n % 32 == 0 else 3), plan_before
    r32, plan32 = solve(C.prob, x0, **kw)
    assert plan32 == C.plan and C.prob.f(x0) > 0 and C.prob.duality_gap(x0).gap >= 0
    after, plan_after = solve(LeastSquaresL1(D.A64, C.b_dev, D.lam, scale=C.scale, matrix_dtype=None), x0, **kw)
    assert plan_after == plan_before
    assert np.array_equal(np.asarray(before.allvecs), np.asarray(after.allvecs))
    assert np.array_equal(np.asarray(before.allfuns), np.asarray(after.allfuns))
    assert rel_err(r32.x, before.x) <= 1e-8   # (the same problem, summed otherwise)
