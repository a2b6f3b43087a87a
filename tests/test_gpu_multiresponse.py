"""GPU: K responses on one dense matrix (csrc/zf_kernels_mr.h, zf_solver_set_responses, MultiResponseLeastSquaresL1 /
MultiResponseLogisticL1, l1_cv_lockstep).

(1) The two sweeps element-wise: f and every element of jac_f against oracle.problems_ref.ls_longdouble per response, inside its
    a-priori bound, for EVERY K = 2 .. 16 (each is a kernel instantiation of its own) on every load width and remainder path
    (multiresponse_cases.sweep_shapes), the kernel forms asserted through zf_solver_ls_plan.  ZF_MR_BOUNDS_RECORD=1 appends the worst error / bound ratios to
    profiles/multiresponse_bounds.jsonl (any other value: to that path).
(2) Response symmetry: equal columns of B give bit-equal columns of jac_f and of every iterate of a 30-iteration FISTA solve.
(3) Response independence, every K: another column k of B changes no bit of the other columns; inf in X[:, k] leaves the others finite.
(4) Solves against the CPU oracle on the Kronecker matrix at 1e-10, the lr and trial sequences exactly (multiresponse_cases.CASES and
    ENDINGS; TALL: m K > 32768, the wide residual kernels), against the existing
    device class on the same Kronecker matrix, with and without return_all, advanced three passes at a time, and resumed from a
    snapshot.  multiresponse_cases.ALL_K: one 30-iteration solve per loss and per K = 2 .. 16 through the solver's ring-indexed
    launches, each K under both load widths - oracle, sequences, sub_iters, the Kronecker class and the certificate.
(5) The certificate against the existing class's on the Kronecker matrix; the live solver's; gap_tol; every response's own gap.
(6) l1_cv_lockstep: fold ids and every fold's certificate for both losses; the score bound and lam_best against l1_cv for the squared
    loss only (the bound needs strong convexity in x).  (7) K = 1, with_responses, streams.  (8) Refusals at the C level in both call orders."""
import contextlib
import functools
import io
import json
import os
import warnings

import numpy as np
import pytest

import gap_cases as GC
import multiresponse_cases as M
from conftest import ROOT, rel_err
from oracle import problems_ref as P

pytestmark = pytest.mark.gpu
TOL = 1e-10
U = 2.0 ** -53


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with contextlib.redirect_stdout(io.StringIO()):
            return fn(*a, **k)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _record(row):
    where = os.environ.get("ZF_MR_BOUNDS_RECORD")
    if not where:
        return
    path = os.path.join(ROOT, "profiles", "multiresponse_bounds.jsonl") if where == "1" else where
    with open(path, "a") as fh:
        fh.write(json.dumps(row) + "\n")


def _cls(loss, multi=True):
    from zfista_amd import problems as Z

    if multi:
        return Z.MultiResponseLogisticL1 if loss == "logistic" else Z.MultiResponseLeastSquaresL1
    return Z.LogisticL1 if loss == "logistic" else Z.LeastSquaresL1


def _problem(case):
    """The multi-response problem of a case."""
    A, B, lam, Wt, Pf, l2 = case.data()
    return _cls(case.loss)(A, B, lam, M.SCALE[case.loss], case.box, l2, sample_weight=Wt, penalty_factor=Pf)


def _kron_problem(case):
    """The same case on the EXISTING device class over np.kron(A, I_K)."""
    A, B, lam, Wt, Pf, l2 = case.data()
    K = case.K
    big, b = np.kron(A, np.eye(K)), B.reshape(-1)
    if case.loss == "logistic":
        p = _cls("logistic", False)(big, b, lam, M.SCALE["logistic"], case.box)
        if l2 > 0:
            p = p.with_penalty(lam, l2)
    else:
        p = _cls("square", False)(big, b, lam, M.SCALE["square"], case.box, l2=l2)
    if Wt is not None:
        p = p.with_sample_weight(M.wide(Wt, case.m, K).reshape(-1))
    if Pf is not None:
        p = p.with_penalty_factor(M.wide(Pf, case.n, K).reshape(-1))
    return p


@functools.lru_cache(maxsize=None)
def _oracle(idx, table="CASES"):
    """The reference solver on the Kronecker closures - computed once per case, shared, left unchanged."""
    from oracle import cpu_ref

    case = getattr(M, table)[idx]
    return _quiet(cpu_ref.minimize_proximal_gradient, *M.kron_ref(case).callbacks(), case.x0(), return_all=True, **case.opts)


# ---- (1) the sweeps, element-wise ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", M.KS)
def test_sweeps_elementwise_within_the_longdouble_bounds(K):
    from zfista_amd.engine import DeviceSolver

    worst_f = worst_g = 0.0
    for m, n in M.sweep_shapes(K):
        rng = np.random.default_rng(1000 * K + m + n)
        A, X, B = rng.standard_normal((m, n)), rng.standard_normal((n, K)), rng.standard_normal((m, K))
        prob = _cls("square")(A, B, 0.1, 0.5)
        # the kernel forms this shape takes
        fields, keep = prob._descriptor()
        s = DeviceSolver(fields, dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=3, max_backtrack_iter=10), keepalive=keep)
        slices, rps = M.slices_of(m, n)
        assert s.ls_plan() == ((10, 8) if n % 2 else (9, 7)) + (slices, rps), (m, n, s.ls_plan())
        assert s.responses_plan() == (K, M.rows_per_wg(K))
        s.close()
        f = prob.f(X)
        G = prob.jac_f(X.reshape(-1)).reshape(n, K)
        f_ref, f_bound = np.longdouble(0), 0.0
        for k in range(K):
            fk, gk, fb, gb = P.ls_longdouble(A, B[:, k], X[:, k], 0.5)
            err = np.abs((G[:, k].astype(np.longdouble) - gk).astype(np.float64))
            assert np.all(err <= gb), (K, m, n, k, float(np.max(err / gb)))
            worst_g = max(worst_g, float(np.max(err / gb)))
            f_ref, f_bound = f_ref + fk, f_bound + fb
        # f is ONE sum of m K squares: ls_longdouble's bound for response k carries gamma_(m + 2n + 6) for its m terms; the joint sum
        # has m K terms, so each response's bound is scaled by (m K + 2 n + 6) / (m + 2 n + 6) (first order in u, as the bound itself)
        f_bound *= (m * K + 2 * n + 6) / (m + 2 * n + 6)
        ferr = abs(float(np.longdouble(f) - f_ref))
        assert ferr <= f_bound, (K, m, n, ferr / f_bound)
        worst_f = max(worst_f, ferr / f_bound)
    print(f"K={K}: worst f error / bound {worst_f:.3g}, worst gradient element error / bound {worst_g:.3g}")
    _record(dict(test="sweeps", K=K, f_ratio=worst_f, grad_ratio=worst_g))


# ---- (2) response symmetry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["square", "logistic"])
@pytest.mark.parametrize("K", [3, 16])
def test_equal_columns_give_bit_equal_columns(K, loss):
    from zfista_amd import minimize_proximal_gradient

    m, n = 100, 131
    A, B1, lam = M.make(loss, m, n, 1, 77)
    B = np.repeat(B1, K, axis=1)
    w = M.make_weights(m, K, 77, "real")
    p = M.make_factors(n, 1, 77, "pos").reshape(-1)
    prob = _cls(loss)(A, B, lam, M.SCALE[loss], sample_weight=w, penalty_factor=p)
    x = np.repeat(np.random.default_rng(5).standard_normal((n, 1)), K, axis=1)
    G = prob.jac_f(x).reshape(n, K)
    assert all(np.array_equal(_bits(G[:, 0]), _bits(G[:, k])) for k in range(1, K)) and np.abs(G).max() > 0
    res = _quiet(minimize_proximal_gradient, *prob.callbacks(), np.zeros(n * K), lr=1.0, tol=0.0, max_iter=30, nesterov=True, return_all=True)
    assert res.nit == 30
    for it, xv in enumerate(res.allvecs):
        Xv = np.asarray(xv).reshape(n, K)
        assert all(np.array_equal(_bits(Xv[:, 0]), _bits(Xv[:, k])) for k in range(1, K)), it
    assert np.abs(prob.coef(res.x)).max() > 0


# ---- (3) response independence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", M.KS)
def test_a_response_touches_no_other(K):
    m, n = 65, 130
    rng = np.random.default_rng(K)
    A, X, B = rng.standard_normal((m, n)), rng.standard_normal((n, K)), rng.standard_normal((m, K))
    G = _cls("square")(A, B, 0.1).jac_f(X).reshape(n, K)
    for k in (0, K - 1):
        B2 = B.copy()
        B2[:, k] = rng.standard_normal(m)
        G2 = _cls("square")(A, B2, 0.1).jac_f(X).reshape(n, K)
        others = [j for j in range(K) if j != k]
        assert np.array_equal(_bits(G[:, others]), _bits(G2[:, others])) and not np.array_equal(G[:, k], G2[:, k])
        # inf (not NaN: v_max_f64 would drop a NaN operand) in X[:, k]: the other margins, hence the other gradient columns, stay finite
        X2 = X.copy()
        X2[3, k] = np.inf
        with np.errstate(invalid="ignore"):
            G3 = _cls("square")(A, B, 0.1).jac_f(X2).reshape(n, K)
        assert np.all(np.isfinite(G3[:, others])) and np.array_equal(_bits(G3[:, others]), _bits(G[:, others]))
        assert not np.all(np.isfinite(G3[:, k]))


# ---- (4) solves against the oracle ---------------------------------------------------------------------------------------------
def _compare(res, exp, case):
    assert res.nit == exp.nit and res.success == exp.success, (res.nit, exp.nit, res.message, exp.message)
    assert res.message == exp.message
    assert len(res.allvecs) == len(exp.allvecs)
    worst = 0.0
    for a, b in zip(res.allvecs, exp.allvecs):
        worst = max(worst, rel_err(a, b) if np.any(b) else float(np.max(np.abs(a))))
    fa, fb = np.asarray(res.allfuns, float).reshape(-1), np.asarray(exp.allfuns, float).reshape(-1)
    fin = np.isfinite(fb)
    assert np.array_equal(fin, np.isfinite(fa))
    ferr = float(np.max(np.abs(fa[fin] - fb[fin]) / np.abs(fb[fin]))) if fin.any() else 0.0
    ea, eb = np.asarray(res.allerrs, float), np.asarray(exp.allerrs, float)
    # (err is a norm of a difference of two iterates: 1e-10 of the iterates' size, not of its own, is what two solves within 1e-10 imply)
    size = max(1.0, max(float(np.max(np.abs(v))) for v in exp.allvecs))
    eerr = float(np.max(np.abs(ea - eb))) / size if len(eb) else 0.0
    print(f"{case.id}: nit {res.nit}, iterates {worst:.2e}, F {ferr:.2e}, err {eerr:.2e}")
    assert worst <= TOL and ferr <= TOL and eerr <= TOL


_OPTS = dict(lr=1.0, tol=0.0, tol_internal=1e-12, max_iter=60, max_iter_internal=100000, max_backtrack_iter=100, warm_start=False,
             decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False, deprecated=False)


def _drain(prob, case, step, **extra):
    """The trace rows of every accepted iteration of the case's solve, advanced `step` passes at a time, and its final x."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    run = NativeRun(prob, case.x0(), dict(_OPTS, **case.opts, **extra))
    rows = [np.zeros((0, _lib.ZF_TRACE_COLS))]
    while run.status == _lib.ZF_RUNNING:
        rows.append(run.advance(step))
    x = run.solver.get_x()
    run.solver.close()
    return np.concatenate(rows), x


def _check_sequences(rows, exp):
    """The line search decided as the oracle's: the step after, and the trials of, every accepted iteration - exactly."""
    from zfista_amd import _lib

    assert len(rows) == exp.nit
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), np.asarray(exp.alltrials, np.int64))
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float))


@pytest.mark.parametrize("idx", range(len(M.CASES)), ids=[c.id for c in M.CASES])
def test_solve_vs_oracle_and_the_existing_class_on_the_kronecker_matrix(idx):
    from zfista_amd import _lib, minimize_proximal_gradient

    case = M.CASES[idx]
    exp = _oracle(idx)
    prob = _problem(case)
    kw = dict(case.opts, gap_tol=None)
    res = _quiet(minimize_proximal_gradient, *prob.callbacks(), case.x0(), return_all=True, **kw)
    _compare(res, exp, case)
    # without return_all: chunks of doubling length - the same bits
    plain = _quiet(minimize_proximal_gradient, *prob.callbacks(), case.x0(), **kw)
    assert plain.nit == res.nit and np.array_equal(_bits(plain.x), _bits(res.x)) and plain.fun == res.fun
    # three passes at a time, and sub_iters 1 / 16 (a margins solver runs one trial per pass whatever is asked)
    for sub in (1, 16):
        rows, x = _drain(prob, case, 3, sub_iters=sub)
        assert np.array_equal(_bits(x), _bits(res.x)) and len(rows) == res.nit, sub
        assert np.array_equal(rows[:, _lib.TR_F], np.asarray(res.allfuns[1:], float).reshape(-1))
        _check_sequences(rows, exp)
    # the existing device class on the Kronecker matrix
    kr = _quiet(minimize_proximal_gradient, *_kron_problem(case).callbacks(), case.x0(), return_all=True, **kw)
    assert kr.nit == res.nit and rel_err(res.x, kr.x) <= TOL and abs(res.fun - kr.fun) <= TOL * abs(kr.fun)


@pytest.mark.parametrize("idx", range(len(M.ENDINGS)), ids=[c.id for c in M.ENDINGS])
def test_every_ending_as_the_oracle(idx):
    from zfista_amd import minimize_proximal_gradient

    case = M.ENDINGS[idx]
    exp = _oracle(idx, "ENDINGS")
    prob = _problem(case)
    res = _quiet(minimize_proximal_gradient, *prob.callbacks(), case.x0(), return_all=True, **case.opts)
    _compare(res, exp, case)
    rows, x = _quiet(_drain, prob, case, 2)
    _check_sequences(rows, exp)
    assert np.array_equal(_bits(x), _bits(res.x))


@functools.lru_cache(maxsize=None)
def _tall_oracle(idx):
    """The reference solver on the per-response closures (which the CPU file proves equal to the Kronecker ones on this table too: the
    Kronecker matrix of these cases is 50 MB, the closures of A @ X need none)."""
    from oracle import cpu_ref

    case = M.TALL[idx]
    return _quiet(cpu_ref.minimize_proximal_gradient, *M.MRRef(case).callbacks(), case.x0(), return_all=True, **case.opts)


@pytest.mark.parametrize("nesterov", [True, False], ids=["fista", "ista"])
@pytest.mark.parametrize("idx", range(len(M.TALL)), ids=[c.id for c in M.TALL])
def test_more_than_32768_rows_of_margins_take_the_wide_residual_kernels(idx, nesterov, tmp_path):
    """m K > 32768 with the unweighted squared loss: r(y), f(y) and f(x+) of a trial come from the many-workgroup residual kernels and
    their chunk sums.  Against the oracle (iterates, F, err at 1e-10, the lr and trial sequences exactly), F of the first and last
    iterate against long double per response, K plain solves on the columns of B, and a resume across a snapshot."""
    from zfista_amd import _lib, minimize_proximal_gradient
    from zfista_amd.proximal_gradient import NativeRun

    case = M.TALL[idx]
    assert case.m * case.K > 32768 and case.weights is None
    A, B, lam, _, _, _ = case.data()
    prob = _problem(case)
    if nesterov:
        exp = _tall_oracle(idx)
        opts = dict(case.opts)
    else:
        from oracle import cpu_ref

        opts = dict(case.opts, nesterov=False)
        exp = _quiet(cpu_ref.minimize_proximal_gradient, *M.MRRef(case).callbacks(), case.x0(), return_all=True, **opts)
    res = _quiet(minimize_proximal_gradient, *prob.callbacks(), case.x0(), return_all=True, **opts)
    _compare(res, exp, case)
    run = NativeRun(prob, case.x0(), dict(_OPTS, **opts))
    rows = [run.advance(1) for _ in range(14)]   # (the first iteration alone takes 13 trials from lr = 1)
    state = run.snapshot()
    run.solver.close()
    np.savez(tmp_path / "ckpt.npz", **state)
    run = NativeRun.from_snapshot(prob, dict(np.load(tmp_path / "ckpt.npz")), dict(_OPTS, **opts))
    while run.status == _lib.ZF_RUNNING:
        rows.append(run.advance(2))
    rows = np.concatenate(rows)
    _check_sequences(rows, exp)
    assert int(rows[:, _lib.TR_TRIALS].sum()) > exp.nit, "the case must reject trials"
    assert np.array_equal(_bits(run.solver.get_x()), _bits(res.x)), "resumed across a snapshot: the same bits"
    assert np.array_equal(rows[:, _lib.TR_F], np.asarray(res.allfuns[1:], float).reshape(-1))
    run.solver.close()
    # F = f + g of the trace at the device's own iterates, against long double per response: ls_longdouble's f bound as in the sweep
    # test (one sum of m K squares) plus n K u g for the l1 sum
    m, n, K = case.m, case.n, case.K
    for it in (1, res.nit):
        X = np.asarray(res.allvecs[it]).reshape(n, K)
        f_ref, f_bound = np.longdouble(0), 0.0
        for k in range(K):
            fk, _, fb, _ = P.ls_longdouble(A, B[:, k], X[:, k], M.SCALE["square"], grad=False)
            f_ref, f_bound = f_ref + fk, f_bound + fb
        f_bound *= (m * K + 2 * n + 6) / (m + 2 * n + 6)
        g = np.longdouble(lam) * np.sum(np.abs(X.astype(np.longdouble)))
        bound = f_bound + 2 * n * K * U * float(g) + 2 * U * float(f_ref + g)
        Fdev = float(np.asarray(res.allfuns[it]).reshape(-1)[0])
        assert abs(float(np.longdouble(Fdev) - (f_ref + g))) <= bound, (it, Fdev, float(f_ref + g), bound)
    # K plain solves, each with its own line search: the same minimisers (the plain class is the yardstick), compared where both have
    # converged - eight iterations reach 1e-9 here, so the tolerance is that of the solves, not of the arithmetic
    if nesterov:
        plain = _cls("square", False)(A, B[:, 0].copy(), lam, M.SCALE["square"])
        long = _quiet(minimize_proximal_gradient, *prob.callbacks(), case.x0(), lr=1.0, tol=0.0, nesterov=True, max_iter=14)
        Xl = prob.coef(long.x)
        for k in (0, K - 1):
            import torch

            q = plain.with_lam(lam)
            q.b = torch.from_numpy(np.ascontiguousarray(B[:, k])).cuda()
            one = _quiet(minimize_proximal_gradient, *q.callbacks(), np.zeros(n), lr=1.0, tol=0.0, nesterov=True, max_iter=14)
            assert rel_err(Xl[:, k], one.x) <= 1e-7, (k, rel_err(Xl[:, k], one.x))


@pytest.mark.parametrize("idx", M.SNAPSHOT_CASES, ids=[M.CASES[i].id for i in M.SNAPSHOT_CASES])
def test_snapshot_and_resume_across_the_last_chunk(idx, tmp_path):
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    case = M.CASES[idx]
    prob = _problem(case)
    opts = dict(lr=1.0, tol=0.0, tol_internal=1e-12, max_iter=60, max_iter_internal=100000, max_backtrack_iter=100, warm_start=False,
                decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False, deprecated=False)

    def drain(run):
        rows = [np.zeros((0, _lib.ZF_TRACE_COLS))]
        while run.status == _lib.ZF_RUNNING:
            rows.append(run.advance(5))
        return np.concatenate(rows)

    whole = NativeRun(prob, case.x0(), opts)
    ref_rows, ref_x = drain(whole), whole.solver.get_x()
    whole.solver.close()
    assert len(ref_rows) == 60
    first = NativeRun(prob, case.x0(), opts)
    head = [first.advance(1) for _ in range(57)]
    state = first.snapshot()
    first.solver.close()
    np.savez(tmp_path / "ckpt.npz", **state)
    run = NativeRun.from_snapshot(prob, dict(np.load(tmp_path / "ckpt.npz")), opts)
    assert run.solver.responses_plan()[0] == case.K
    rows = np.concatenate(head + [drain(run)])
    assert np.array_equal(rows, ref_rows) and np.array_equal(_bits(run.solver.get_x()), _bits(ref_x))
    run.solver.close()


# ---- (5) the certificate -----------------------------------------------------------------------------------------------------
GAP_CASES = [i for i, c in enumerate(M.CASES) if c.box is None and c.factors != "zero"]


def _gap_reference(case, x):
    """(values, bounds) of the certificate at x in long double on the Kronecker matrix: weight_cases.gap_longdouble (unit weights where
    the case has none: a product by 1 is exact, the bound is the unweighted one widened by the u of that product) or, with factors,
    penalty_cases.gap_longdouble - unchanged."""
    import penalty_cases as PC
    import scipy.sparse as sp
    import weight_cases as W

    A, B, lam, Wt, Pf, l2 = case.data()
    K = case.K
    big, b = sp.csr_matrix(np.kron(A, np.eye(K))), B.reshape(-1)
    w = np.ones(b.size) if Wt is None else M.wide(Wt, case.m, K).reshape(-1)
    if Pf is not None:
        vals, bounds, _ = PC.gap_longdouble(big, b, M.wide(Pf, case.n, K).reshape(-1), x, lam, case.loss, scale=M.SCALE[case.loss], w=w)
    else:
        vals, bounds, _ = W.gap_longdouble(big, b, w, x, lam, case.loss, 0.0, M.SCALE[case.loss], l2)
    return vals, bounds


@pytest.mark.parametrize("idx", GAP_CASES, ids=[M.CASES[i].id for i in GAP_CASES])
def test_the_certificate_is_the_existing_class_on_the_kronecker_matrix(idx):
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.proximal_gradient import NativeRun

    case = M.CASES[idx]
    prob, kron = _problem(case), _kron_problem(case)
    keys = GC.KEYS + (("g_l2", "ridge_gap") if case.l2fac else ())
    exp = _oracle(idx)
    pts = [np.zeros(case.n * case.K), np.asarray(exp.allvecs[20]), None]
    long = _quiet(minimize_proximal_gradient, *prob.callbacks(), case.x0(), **dict(case.opts, max_iter=300))
    pts[2] = long.x
    import weight_cases as W

    worst = 0.0
    for x in pts:
        a, b = prob.duality_gap(x), kron.duality_gap(x)
        vals, bounds = _gap_reference(case, x)
        ra, rb = W.worst_ratio(a, vals, bounds), W.worst_ratio(b, vals, bounds)
        assert max(ra.values()) <= 1.0 and max(rb.values()) <= 1.0, (ra, rb)
        worst = max(worst, max(ra.values()))
        for key in vals:   # two evaluations inside the same bound of the same value
            assert abs(float(getattr(a, key)) - float(getattr(b, key))) <= 2 * bounds[key], key
        assert a.gap >= 0
    print(f"{case.id}: worst certificate error / bound {worst:.3g}")
    _record(dict(test="certificate", case=case.id, ratio=worst))
    joint_bound = _gap_reference(case, long.x)[1]["gap"]
    # the live solver's certificate is the standalone one, bit for bit
    opts = dict(lr=1.0, tol=0.0, tol_internal=1e-12, max_iter=100000, max_iter_internal=100000, max_backtrack_iter=100, warm_start=False,
                decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False, deprecated=False)
    run = NativeRun(prob, case.x0(), opts)
    for _ in range(20):
        run.advance(1)
    live, alone = run.duality_gap(), prob.duality_gap(run.solver.get_x())
    run.solver.close()
    assert all(np.array_equal(_bits(getattr(live, k)), _bits(getattr(alone, k))) for k in keys), (live, alone)
    # every response's own certificate (the plain class, its weights) is at most the joint gap: the joint alpha is feasible for it
    A, B, lam, Wt, Pf, l2 = case.data()
    if Pf is None:
        X = prob.coef(long.x)
        joint = prob.duality_gap(long.x)
        plain = _cls(case.loss, False)(A, B[:, 0].copy(), lam, M.SCALE[case.loss])
        if l2 > 0:
            plain = plain.with_penalty(lam, l2)
        total = 0.0
        for k in range(case.K):
            import torch

            q = plain.with_sample_weight(None if Wt is None else M.wide(Wt, case.m, case.K)[:, k].copy())
            q.b = torch.from_numpy(np.ascontiguousarray(B[:, k])).cuda()
            gk = q.duality_gap(np.ascontiguousarray(X[:, k]))
            assert gk.gap <= joint.gap + joint_bound, (k, gk.gap, joint.gap)
            total += float(gk.gap)
        assert total <= float(joint.gap) + case.K * joint_bound


@pytest.mark.parametrize("loss", ["square", "logistic"])
def test_gap_tol_stops_where_a_hand_run_probe_predicts(loss):
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.proximal_gradient import NativeRun

    case = M.CASES[0 if loss == "square" else 9]
    prob = _problem(case)
    P0 = float(prob.duality_gap(np.zeros(prob.n_features)).primal)
    gap_tol = 1e-3 * P0
    opts = dict(lr=1.0, tol=0.0, tol_internal=1e-12, max_iter=4000, max_iter_internal=100000, max_backtrack_iter=100, warm_start=False,
                decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False, deprecated=False)
    run = NativeRun(prob, case.x0(), opts)
    checks = 0
    while True:
        run.advance(16)   # gap_every, as passed below
        checks += 1
        if run.duality_gap().gap <= gap_tol or checks > 400:
            break
    x_probe, nit_probe = run.solver.get_x(), run.nit_seen
    run.solver.close()
    res = _quiet(minimize_proximal_gradient, *prob.callbacks(), case.x0(), lr=1.0, tol=0.0, nesterov=True, max_iter=4000, gap_tol=gap_tol, gap_every=16)
    assert res.success and res.message == "Duality gap reached gap_tol" and res.dual_gap_checks == checks and res.nit == nit_probe
    assert np.array_equal(_bits(res.x), _bits(x_probe)) and 0 <= res.dual_gap <= gap_tol


@pytest.mark.parametrize("idx", range(len(M.ALL_K)), ids=[c.id for c in M.ALL_K])
def test_every_k_solves_through_the_solvers_own_launches(idx):
    """multiresponse_cases.ALL_K: every K = 2 .. 16 under both losses, m one row into the second workgroup of the row sweep, n = 67
    (V = 1) under one loss and 130 (V = 2) under the other.  The comparisons are those of the tests above, unchanged: the oracle on
    the Kronecker closures at TOL (iterates, F, err), the lr and trial sequences exactly, sub_iters 1 / 16 three passes at a time
    bit-equal to the plain solve, the existing class on np.kron(A, I_K) at TOL, the certificate at the final iterate inside the
    long-double bounds of _gap_reference, the live solver's certificate bit-equal to the standalone one."""
    import weight_cases as W
    from zfista_amd import _lib, minimize_proximal_gradient
    from zfista_amd.proximal_gradient import NativeRun

    case = M.ALL_K[idx]
    exp = _oracle(idx, "ALL_K")
    prob, kron = _problem(case), _kron_problem(case)
    kw = dict(case.opts, gap_tol=None)
    res = _quiet(minimize_proximal_gradient, *prob.callbacks(), case.x0(), return_all=True, **kw)
    _compare(res, exp, case)
    assert res.nit == 30 and np.abs(prob.coef(res.x)).max() > 0
    for sub in (1, 16):
        rows, x = _drain(prob, case, 3, sub_iters=sub)
        assert np.array_equal(_bits(x), _bits(res.x)) and len(rows) == res.nit, sub
        assert np.array_equal(rows[:, _lib.TR_F], np.asarray(res.allfuns[1:], float).reshape(-1))
        _check_sequences(rows, exp)
        assert int(rows[:, _lib.TR_TRIALS].sum()) > res.nit, "the case must reject trials"
    kr = _quiet(minimize_proximal_gradient, *kron.callbacks(), case.x0(), return_all=True, **kw)
    assert kr.nit == res.nit and rel_err(res.x, kr.x) <= TOL and abs(res.fun - kr.fun) <= TOL * abs(kr.fun)
    # the certificate at the final iterate: inside the long-double bounds, as the existing class's
    a, b = prob.duality_gap(res.x), kron.duality_gap(res.x)
    vals, bounds = _gap_reference(case, res.x)
    ra, rb = W.worst_ratio(a, vals, bounds), W.worst_ratio(b, vals, bounds)
    print(f"{case.id}: worst certificate error / bound {max(ra.values()):.3g}")
    assert max(ra.values()) <= 1.0 and max(rb.values()) <= 1.0, (ra, rb)
    assert a.gap >= 0
    _record(dict(test="certificate", case=case.id, ratio=max(ra.values())))
    # the live solver's certificate is the standalone one, bit for bit
    run = NativeRun(prob, case.x0(), dict(_OPTS, max_iter=100000))
    for _ in range(20):
        run.advance(1)
    live, alone = run.duality_gap(), prob.duality_gap(run.solver.get_x())
    assert run.solver.responses_plan() == (case.K, M.rows_per_wg(case.K))
    run.solver.close()
    assert all(np.array_equal(_bits(getattr(live, k)), _bits(getattr(alone, k))) for k in GC.KEYS), (live, alone)


# ---- (6) l1_cv_lockstep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["square", "logistic"])
def test_l1_cv_lockstep_certifies_every_fold(loss):
    from zfista_amd.path import cv_fold_ids, l1_cv, l1_cv_lockstep

    m, n, folds = 120, 66, 4
    A, B, lam = M.make(loss, m, n, 1, 901)
    b = B[:, 0].copy()
    prob = _cls(loss, False)(A, b, lam, M.SCALE[loss])
    lmax = float(prob.lam_max())
    lams = [0.5 * lmax, 0.2 * lmax, 0.05 * lmax]
    P0 = float(prob.duality_gap(np.zeros(n)).primal)
    gap_tol = 1e-6 * P0
    kw = dict(lr=1.0, tol=0.0, nesterov=True, max_iter=20000)
    cv = _quiet(l1_cv_lockstep, prob, lams, folds=folds, seed=3, gap_tol=gap_tol, refit=False, **kw)
    assert np.array_equal(cv.fold_ids, cv_fold_ids(m, folds, 3)) and cv.folds == list(range(folds))
    joint = cv.problems[0]
    assert joint.A.data_ptr() == prob.A.data_ptr() and joint.n_responses == folds
    ids = cv.fold_ids
    slack = 1e-11 * max(P0, 1.0)
    gaps = np.zeros((folds, len(lams)))
    for l, res in enumerate(cv.paths[0]):
        assert res.success and res.dual_gap <= gap_tol
        X = joint.coef(res.x)
        for k in range(folds):
            train = prob.with_lam(lams[l]).with_sample_weight((ids != k).astype(float))
            gk = train.duality_gap(np.ascontiguousarray(X[:, k]))
            assert gk.gap <= gap_tol + slack, (l, k, float(gk.gap), gap_tol)
            gaps[k, l] = float(gk.gap)
            score = prob.with_sample_weight((ids == k).astype(float)).f(np.ascontiguousarray(X[:, k])) / float((ids == k).sum())
            assert score == cv.scores[k, l]
    # against l1_cv, fold by fold (squared loss: the bound below needs strong convexity in x, which the logistic loss has not).
    # f_train(x) = 0.5 |A_tr x - b_tr|^2 with m_train > n is mu-strongly convex in x, mu = sigma_min(A_tr)^2, and so is P: a point with
    # duality gap G lies within sqrt(2 G / mu) of the minimiser, two such points within dx = sqrt(2 Ga / mu) + sqrt(2 Gb / mu).  The
    # held-out score 0.5 |r|^2 / m_te, r = A_te x - b_te, then moves by at most 0.5 (|ra| + |rb|) |A_te|_2 dx / m_te.
    ref = _quiet(l1_cv, prob, lams, folds=folds, seed=3, gap_tol=gap_tol, refit=False, return_paths=True, **kw)
    assert np.array_equal(ref.fold_ids, cv.fold_ids)
    if loss == "square":
        bounds = np.zeros((folds, len(lams)))
        for k in range(folds):
            te = ids == k
            mu = float(np.linalg.svd(A[~te], compute_uv=False)[-1]) ** 2
            for l in range(len(lams)):
                xa, xb = np.ascontiguousarray(joint.coef(cv.paths[0][l].x)[:, k]), ref.paths[k][l].x
                gb = float(ref.problems[k].with_lam(lams[l]).duality_gap(xb).gap)
                dx = np.sqrt(2 * gaps[k, l] / mu) + np.sqrt(2 * gb / mu)
                assert np.linalg.norm(xa - xb) <= dx + 1e-12, (k, l)
                ra, rb = A[te] @ xa - b[te], A[te] @ xb - b[te]
                bounds[k, l] = 0.5 * (np.linalg.norm(ra) + np.linalg.norm(rb)) * np.linalg.norm(A[te], 2) * dx / te.sum()
                assert abs(cv.scores[k, l] - ref.scores[k, l]) <= bounds[k, l] + 1e-12 * abs(ref.scores[k, l]), (k, l)
        order = np.sort(ref.mean)
        assert order[1] - order[0] > 2 * bounds.mean(axis=0).max(), "the case must separate the runner-up by more than the bound"
        assert cv.lam_best == ref.lam_best


# ---- (7) K = 1, with_responses, streams ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["square", "logistic"])
def test_one_response_is_the_plain_class_bit_for_bit(loss):
    from zfista_amd import minimize_proximal_gradient

    A, B, lam = M.make(loss, 100, 130, 1, 55)
    plain = _cls(loss, False)(A, B[:, 0].copy(), lam, M.SCALE[loss])
    one = _cls(loss)(A, B, lam, M.SCALE[loss])
    assert one.n_responses == 1 and "responses" not in one._descriptor()[0]
    x = np.random.default_rng(1).standard_normal(130)
    assert one.f(x) == plain.f(x) and np.array_equal(_bits(one.jac_f(x)), _bits(plain.jac_f(x)))
    assert one.duality_gap(x).gap == plain.duality_gap(x).gap
    kw = dict(lr=1.0, tol=0.0, max_iter=40, nesterov=True)
    a = _quiet(minimize_proximal_gradient, *one.callbacks(), np.zeros(130), **kw)
    b = _quiet(minimize_proximal_gradient, *plain.callbacks(), np.zeros(130), **kw)
    assert a.nit == b.nit == 40 and np.array_equal(_bits(a.x), _bits(b.x)) and a.fun == b.fun


def test_with_responses_shares_the_matrix_and_streams_give_the_same_bits():
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.replicas import solve_on_streams

    case = M.CASES[2]
    A, B, lam, Wt, Pf, l2 = case.data()
    base = _cls("square", False)(A, B[:, 0].copy(), lam, 0.5)
    sib = base.with_responses(B)
    assert sib.A.data_ptr() == base.A.data_ptr() and sib.n_responses == case.K and sib.n_features == case.n * case.K
    direct = _cls("square")(A, B, lam, 0.5)
    n = sib.n_features
    kw = dict(lr=1.0, tol=0.0, max_iter=40, nesterov=True)
    alone = [_quiet(minimize_proximal_gradient, *p.callbacks(), np.zeros(n), **kw) for p in (sib, direct)]
    assert np.array_equal(_bits(alone[0].x), _bits(alone[1].x))
    X0 = np.zeros((case.n, case.K))
    shaped = _quiet(minimize_proximal_gradient, *sib.callbacks(), X0, **kw)
    assert np.array_equal(_bits(shaped.x), _bits(alone[0].x)) and shaped.x.shape == (n,)
    both = solve_on_streams([(p, np.zeros(n), kw) for p in (sib, direct)], streams=2)
    for a, c in zip(alone, both):
        assert a.nit == c.nit == 40 and np.array_equal(_bits(a.x), _bits(c.x)) and a.fun == c.fun


# ---- (8) refusals at the C level -----------------------------------------------------------------------------------------------
def test_the_setter_refuses_in_both_call_orders_and_composes():
    import ctypes as C

    import torch

    from zfista_amd import _lib
    from zfista_amd.engine import DeviceSolver
    from zfista_amd.problems import DiagQuadL1, LeastSquaresL1

    A, b, lam = P.make_plasso(512, 1024, seed=0)
    options = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=3, max_backtrack_iter=10)
    fields, keep = LeastSquaresL1(A, b, lam)._descriptor()
    s = DeviceSolver(fields, options, keepalive=keep)
    lib = s.lib
    assert s.ls_plan()[0] == 1 and s.responses_plan() == (1, 0)
    for bad in (1, 0, -1, 17):
        assert lib.zf_solver_set_responses(s.handle, bad) == -2 and b"2 .. 16" in lib.zf_last_error()
    assert lib.zf_solver_set_responses(s.handle, 3) == -2 and b"multiples of K" in lib.zf_last_error()
    assert lib.zf_solver_set_responses(None, 2) == -2
    assert s.ls_plan()[0] == 1, "a refused call leaves the solver as it was"
    # composition in any order with l2 / weights / factors
    wd = torch.ones(512, dtype=torch.float64, device="cuda")
    pd = torch.ones(1024, dtype=torch.float64, device="cuda")
    assert lib.zf_solver_set_row_weights(s.handle, C.c_void_p(wd.data_ptr())) == 0
    assert lib.zf_solver_set_responses(s.handle, 4) == 0 and s.ls_plan()[:2] == (9, 7) and s.responses_plan() == (4, 16)
    assert lib.zf_solver_set_penalty_factors(s.handle, C.c_void_p(pd.data_ptr())) == 0
    assert lib.zf_solver_set_responses(s.handle, 4) == -2 and b"already" in lib.zf_last_error()
    # ... and the setters it excludes, after it
    a32 = torch.zeros(8, dtype=torch.float32, device="cuda")
    assert lib.zf_solver_set_huber(s.handle, 0.5) == -2 and b"responses" in lib.zf_last_error()
    assert lib.zf_solver_set_poisson(s.handle) == -2 and b"responses" in lib.zf_last_error()
    assert lib.zf_solver_set_matrix_f32(s.handle, C.c_void_p(a32.data_ptr())) == -2 and b"responses" in lib.zf_last_error()
    x0 = torch.zeros(1024, dtype=torch.float64, device="cuda")
    s.init(x0.data_ptr())
    s.close()
    # ... and before it
    for first, word in ((lambda h: lib.zf_solver_set_huber(h, 0.5), b"Huber"), (lambda h: lib.zf_solver_set_poisson(h), b"Poisson")):
        s = DeviceSolver(fields, options, keepalive=keep)
        assert first(s.handle) == 0 and lib.zf_solver_set_responses(s.handle, 2) == -2 and word in lib.zf_last_error()
        s.close()
    A32 = torch.zeros(512 * 1024, dtype=torch.float32, device="cuda")
    s = DeviceSolver(fields, options, keepalive=keep)
    assert lib.zf_solver_set_matrix_f32(s.handle, C.c_void_p(A32.data_ptr())) == 0
    assert lib.zf_solver_set_responses(s.handle, 2) == -2 and b"fp32" in lib.zf_last_error()
    s.close()
    # after init: ZF_ERR_STATE
    s = DeviceSolver(fields, options, keepalive=keep)
    s.init(x0.data_ptr())
    assert lib.zf_solver_set_responses(s.handle, 2) == -3 and b"before" in lib.zf_last_error()
    s.close()
    # ZF_ACCEPT_REMAINDER, another kind, world > 1
    s = DeviceSolver(fields, dict(options, accept_mode=_lib.ZF_ACCEPT_REMAINDER), keepalive=keep)
    assert lib.zf_solver_set_responses(s.handle, 2) == -2 and b"ZF_ACCEPT_REMAINDER" in lib.zf_last_error()
    s.close()
    d, c, lam_d = P.make_pdiag(1000, seed=1)
    f2, k2 = DiagQuadL1(d, c, lam_d)._descriptor()
    s = DeviceSolver(f2, options, keepalive=k2)
    assert lib.zf_solver_set_responses(s.handle, 2) == -2 and b"only for" in lib.zf_last_error()
    s.close()
    dd, o, h = _lib.ProblemDesc(), _lib.Options(), C.c_void_p()
    for k, v in dict(fields, world=2, rank=0).items():
        setattr(dd, k, v)
    for k, v in options.items():
        setattr(o, k, v)
    assert lib.zf_solver_create(C.byref(h), C.byref(dd), C.byref(o), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert lib.zf_solver_set_responses(h, 2) == -2 and b"world > 1" in lib.zf_last_error()
    assert lib.zf_solver_destroy(h) == 0


def test_a_plain_solver_launches_what_it_launched(monkeypatch):
    """A multi-response solve in between changes nothing for the plain classes: the same plan, launch counts and bits."""
    from zfista_amd import minimize_proximal_gradient, proximal_gradient as pg
    from zfista_amd.problems import LeastSquaresL1

    seen = []

    class _Recorded(pg.NativeRun):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.plan = self.solver.ls_plan() + self.solver.responses_plan()
            seen.append(self)

        def collect(self):
            rows = super().collect()
            self.counts = self.solver.launch_counts()
            return rows

    monkeypatch.setattr(pg, "NativeRun", _Recorded)
    A, b, lam = P.make_plasso(64, 128, seed=0)
    kw = dict(lr=1.0, tol=0.0, max_iter=30, nesterov=True)
    before = _quiet(minimize_proximal_gradient, *LeastSquaresL1(A, b, lam).callbacks(), np.zeros(128), **kw)
    case = M.CASES[1]
    _quiet(minimize_proximal_gradient, *_problem(case).callbacks(), case.x0(), **case.opts)
    after = _quiet(minimize_proximal_gradient, *LeastSquaresL1(A, b, lam).callbacks(), np.zeros(128), **kw)
    assert before.nit == after.nit and np.array_equal(_bits(before.x), _bits(after.x)) and before.fun == after.fun
    assert len(seen) == 3 and seen[1].plan[4] == case.K
    assert seen[0].plan == seen[2].plan and seen[0].plan[0] == 1 and seen[0].plan[4:] == (1, 0), "the fused small-matrix path, no responses"
    assert seen[0].counts == seen[2].counts
