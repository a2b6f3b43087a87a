"""GPU: K responses on one CSR matrix (csrc/zf_kernels_spmm.h, zf_solver_create_sparse_responses,
SparseMultiResponseLeastSquaresL1 / SparseMultiResponseLogisticL1, l1_cv_lockstep on sparse problems).

The yardstick is EXACT: row i K + k of sp.kron(A, I_K) holds the elements of row i of A in the same order at columns j K + k, the
plans agree per response (tests/test_sparse_multiresponse_cases.py), and the K-response sweeps sum response k as the plain sweeps
sum a vector - so the existing sparse classes on the Kronecker matrix perform the same floating-point operations in the same
order, and every comparison against them below is bit for bit.  The CPU oracle on the SciPy closures of the Kronecker matrix is
the independent reference, at the project's parity tolerance 1e-10.

(1) Both sweeps element-wise: zf_spmat_mr_apply(K)[:, k] == zf_spmat_mr_apply(K = 1) on column k, for EVERY K = 2 .. 16 (each is a
    kernel instantiation of its own, per lane width), on the SMALL and TALL matrices and on hand-built ones: every remainder of a
    lane per lane width, nnz = 0, one row, one column, the split threshold from both sides, 300 split rows (K in {2, 4, 7, 16}).
(2) Equal columns give bit-equal columns (jac_f, 30 FISTA iterates); inf in one column leaves the others' bits.
(3) f, jac_f, duality_gap: the Kronecker class's bits, inside the long-double bounds on the Kronecker CSR.
(4) Solves: the Kronecker class bit for bit (nit, status, message, iterates, F, err, lr and trial columns; sub_iters 1 / 16; three
    passes at a time), the oracle at 1e-10; every ending; sparse_multiresponse_cases.ALL_K: one solve per loss and per K = 2 .. 16
    through the solver's own launches.  (5) TALL with K = 8: FISTA and ISTA, a resume across a snapshot.
(6) gap_tol, the live certificate, l1_cv_lockstep on sparse problems.  (7) K = 1, with_responses, streams, the creator's
    refusals, the plain sparse solver's launch count."""
import contextlib
import functools
import hashlib
import io
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import gap_cases as GC
import multiresponse_cases as M
import sparse_cases as S
import sparse_multiresponse_cases as SM
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-10


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with contextlib.redirect_stdout(io.StringIO()):
            return fn(*a, **k)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _cls(loss, multi=True):
    from zfista_amd import problems as Z

    if multi:
        return Z.SparseMultiResponseLogisticL1 if loss == "logistic" else Z.SparseMultiResponseLeastSquaresL1
    return Z.SparseLogisticL1 if loss == "logistic" else Z.SparseLeastSquaresL1


def _build(loss, A, B, lam, Wt, Pf, l2, box, K):
    """(the K-response problem, the EXISTING sparse class on sp.kron(A, I_K)) of one set of inputs."""
    m, n = A.shape
    new = _cls(loss)(A, B, lam, SM.SCALE[loss], box, l2, sample_weight=Wt, penalty_factor=Pf)
    big, b = SM.kron(A, K), B.reshape(-1)
    if loss == "logistic":
        kr = _cls("logistic", False)(big, b, lam, SM.SCALE["logistic"], box)
        if l2 > 0:
            kr = kr.with_penalty(lam, l2)
    else:
        kr = _cls("square", False)(big, b, lam, SM.SCALE["square"], box, l2=l2)
    if Wt is not None:
        kr = kr.with_sample_weight(M.wide(Wt, m, K).reshape(-1))
    if Pf is not None:
        kr = kr.with_penalty_factor(M.wide(Pf, n, K).reshape(-1))
    return new, kr


def _problems(case):
    A, B, lam, Wt, Pf, l2 = case.data()
    return _build(case.loss, A, B, lam, Wt, Pf, l2, case.box, case.K)


@functools.lru_cache(maxsize=None)
def _oracle(idx, table="CASES"):
    """The reference solver on the SciPy-sparse closures of the Kronecker matrix - once per case, shared, left unchanged."""
    from oracle import cpu_ref

    case = getattr(SM, table)[idx]
    return _quiet(cpu_ref.minimize_proximal_gradient, *SM.kron_ref(case).callbacks(), case.x0(), return_all=True, **case.opts)


# ---- (1) the sweeps, element-wise ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sweep_inputs():
    mats = [(f"small{i}", S.make_sparse(*c)[0]) for i, c in enumerate(S.SMALL)]
    mats.append(("tall", S.make_sparse(*S.TALL)[0]))
    return tuple(mats + SM.sweep_matrices())


def _apply(lib, h, transpose, K, scale, x):
    import ctypes as C

    from zfista_amd import _lib

    rows = h.shape[1] if transpose else h.shape[0]
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.full(rows * K, np.nan)
    _lib.check(lib.zf_spmat_mr_apply(h.value, int(transpose), K, scale, C.c_void_p(_lib.ptr(x)), C.c_void_p(_lib.ptr(out))), "zf_spmat_mr_apply")
    return out.reshape(rows, K)


@functools.lru_cache(maxsize=None)
def _handle(name):
    from zfista_amd import problems, sparse

    A = dict(_sweep_inputs())[name]
    prep = sparse.prepare(A)
    h = problems._SpmatHandle(prep)
    h.shape = A.shape
    h.lanes = (prep["plan"]["lanes"], prep["t_plan"]["lanes"])
    return h


SWEEP_NAMES = [f"small{i}" for i in range(len(S.SMALL))] + ["tall"] + [n for n, _ in SM.sweep_matrices()]


@pytest.mark.parametrize("name", SWEEP_NAMES)
def test_every_column_of_a_sweep_is_the_plain_sweep_on_that_column(name):
    """Every K = 2 .. 16 on every matrix but `many-split` (1.2e6 elements per sweep), which takes K in (2, 4, 7, 16): the 16-byte and
    the scalar gather, each at four and at two elements in flight."""
    from zfista_amd import _lib

    lib = _lib.require_gpu()
    h = _handle(name)
    A = sp.csr_matrix(dict(_sweep_inputs())[name])
    absA = abs(A)
    scale = 0.3
    ks = SM.MANY_SPLIT_KS if name == "many-split" else SM.KS
    assert tuple(SM.KS) == tuple(range(2, 17))
    for transpose in (0, 1):
        Mx, absM = (A.T, absA.T) if transpose else (A, absA)
        cols = Mx.shape[1]
        rng = np.random.default_rng(31 + transpose)
        Xall = rng.standard_normal((cols, 16))
        ones = {k: _apply(lib, h, transpose, 1, scale, Xall[:, k])[:, 0] for k in range(16)}
        # the plain sweep itself against SciPy: gamma_len |M| |x| per element, first order, with a factor 2
        longest = int(np.diff(sp.csr_matrix(Mx).indptr).max(initial=0))
        for k in (0, 15):
            bound = 2 * (longest + 2) * 2.0 ** -53 * scale * (absM @ np.abs(Xall[:, k])) + 1e-300
            assert np.all(np.abs(ones[k] - scale * (Mx @ Xall[:, k])) <= bound), (name, transpose, k)
        for K in ks:
            out = _apply(lib, h, transpose, K, scale, Xall[:, :K])
            for k in range(K):
                assert _same(out[:, k], ones[k]), (name, transpose, K, k, h.lanes)


# ---- (2) symmetry and independence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["square", "logistic"])
@pytest.mark.parametrize("K", [3, 16])
def test_equal_columns_give_bit_equal_columns(K, loss):
    from zfista_amd import minimize_proximal_gradient

    A, B1, lam = SM.make(loss, "a", 1, 77)
    m, n = A.shape
    B = np.repeat(B1, K, axis=1)
    w = M.make_weights(m, K, 77, "real")
    p = M.make_factors(n, 1, 77, "pos").reshape(-1)
    prob = _cls(loss)(A, B, lam, SM.SCALE[loss], sample_weight=w, penalty_factor=p)
    x = np.repeat(np.random.default_rng(5).standard_normal((n, 1)), K, axis=1)
    G = prob.jac_f(x).reshape(n, K)
    assert all(_same(G[:, 0], G[:, k]) for k in range(1, K)) and np.abs(G).max() > 0
    res = _quiet(minimize_proximal_gradient, *prob.callbacks(), np.zeros(n * K), lr=1.0, tol=0.0, max_iter=30, nesterov=True, return_all=True)
    assert res.nit == 30
    for it, xv in enumerate(res.allvecs):
        Xv = np.asarray(xv).reshape(n, K)
        assert all(_same(Xv[:, 0], Xv[:, k]) for k in range(1, K)), it
    assert np.abs(prob.coef(res.x)).max() > 0


@pytest.mark.parametrize("K", SM.KS)
def test_a_response_touches_no_other(K):
    A, B, lam = SM.make("square", "d", K, 78)
    m, n = A.shape
    rng = np.random.default_rng(K)
    X = rng.standard_normal((n, K))
    base = _cls("square", False)(A, B[:, 0].copy(), lam)
    prob = base.with_responses(B)
    G = prob.jac_f(X).reshape(n, K)
    for k in (0, K - 1):
        others = [j for j in range(K) if j != k]
        B2 = B.copy()
        B2[:, k] = rng.standard_normal(m)
        G2 = base.with_responses(B2).jac_f(X).reshape(n, K)
        assert _same(G[:, others], G2[:, others]) and not np.array_equal(G[:, k], G2[:, k])
        X2 = X.copy()
        X2[3, k] = np.inf   # (row 3 of X meets column 3 of A: not the empty column n // 2)
        with np.errstate(invalid="ignore"):
            G3 = prob.jac_f(X2).reshape(n, K)
        assert np.all(np.isfinite(G3[:, others])) and _same(G3[:, others], G[:, others])
        assert not np.all(np.isfinite(G3[:, k]))


# ---- (3) f, jac_f, duality_gap ----------------------------------------------------------------------------------------------------
GAP_CASES = [i for i, c in enumerate(SM.CASES) if c.box is None and c.factors != "zero"]


def _gap_reference(case, x):
    import penalty_cases as PC
    import weight_cases as W

    A, B, lam, Wt, Pf, l2 = case.data()
    K = case.K
    big, b = SM.kron(A, K), B.reshape(-1)
    w = np.ones(b.size) if Wt is None else M.wide(Wt, case.m, K).reshape(-1)
    if Pf is not None:
        vals, bounds, _ = PC.gap_longdouble(big, b, M.wide(Pf, case.n, K).reshape(-1), x, lam, case.loss, scale=SM.SCALE[case.loss], w=w)
    else:
        vals, bounds, _ = W.gap_longdouble(big, b, w, x, lam, case.loss, 0.0, SM.SCALE[case.loss], l2)
    return vals, bounds


@pytest.mark.parametrize("idx", range(len(SM.CASES)), ids=[c.id for c in SM.CASES])
def test_f_jac_f_and_the_certificate_are_the_kronecker_class_bit_for_bit(idx):
    import weight_cases as W
    from zfista_amd.proximal_gradient import NativeRun

    case = SM.CASES[idx]
    new, kr = _problems(case)
    assert new.n_responses == case.K and new.n_features == kr.n_features == case.n * case.K and new.m_rows == kr.m_rows
    exp = _oracle(idx)
    keys = GC.KEYS + (("g_l2", "ridge_gap") if case.l2fac else ())
    for x in (np.zeros(case.n * case.K), np.asarray(exp.allvecs[20]), np.random.default_rng(idx).standard_normal(case.n * case.K)):
        assert _same(new.f(x), kr.f(x)), (new.f(x), kr.f(x))
        assert _same(new.jac_f(x), kr.jac_f(x))
        assert _same(new.jac_f(x.reshape(case.n, case.K)), kr.jac_f(x)), "x as (n, K)"
        if idx in GAP_CASES:
            a, b = new.duality_gap(x), kr.duality_gap(x)
            assert all(_same(getattr(a, k), getattr(b, k)) for k in keys), (a, b)
            vals, bounds = _gap_reference(case, x)
            ratio = W.worst_ratio(a, vals, bounds)
            assert max(ratio.values()) <= 1.0, ratio
            assert a.gap >= 0
    if idx in GAP_CASES:   # the live solver's certificate is the standalone one, bit for bit
        run = NativeRun(new, case.x0(), dict(_OPTS, max_iter=100000))
        for _ in range(20):
            run.advance(1)
        live, alone = run.duality_gap(), new.duality_gap(run.solver.get_x())
        assert run.solver.responses_plan() == (case.K, 0)
        run.solver.close()
        assert all(_same(getattr(live, k), getattr(alone, k)) for k in keys), (live, alone)
    else:
        with pytest.raises(ValueError, match="duality_gap is not available"):
            new.duality_gap(np.zeros(case.n * case.K))
    lmax = new.with_penalty_factor(None).lam_max() if case.factors == "zero" else new.lam_max()
    assert _same(lmax, kr.with_penalty_factor(None).lam_max() if case.factors == "zero" else kr.lam_max())


# ---- (4) solves -------------------------------------------------------------------------------------------------------------------
_OPTS = dict(lr=1.0, tol=0.0, tol_internal=1e-12, max_iter=60, max_iter_internal=100000, max_backtrack_iter=100, warm_start=False,
             decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False, deprecated=False)


def _compare_oracle(res, exp, case):
    assert res.nit == exp.nit and res.success == exp.success, (res.nit, exp.nit, res.message, exp.message)
    assert res.message == exp.message and len(res.allvecs) == len(exp.allvecs)
    worst = 0.0
    for a, b in zip(res.allvecs, exp.allvecs):
        worst = max(worst, rel_err(a, b) if np.any(b) else float(np.max(np.abs(a))))
    fa, fb = np.asarray(res.allfuns, float).reshape(-1), np.asarray(exp.allfuns, float).reshape(-1)
    fin = np.isfinite(fb)
    assert np.array_equal(fin, np.isfinite(fa))
    ferr = float(np.max(np.abs(fa[fin] - fb[fin]) / np.abs(fb[fin]))) if fin.any() else 0.0
    ea, eb = np.asarray(res.allerrs, float), np.asarray(exp.allerrs, float)
    size = max(1.0, max(float(np.max(np.abs(v))) for v in exp.allvecs))   # (err is a norm of a difference of two iterates)
    eerr = float(np.max(np.abs(ea - eb))) / size if len(eb) else 0.0
    print(f"{case.id}: nit {res.nit}, iterates {worst:.2e}, F {ferr:.2e}, err {eerr:.2e}")
    assert worst <= TOL and ferr <= TOL and eerr <= TOL


def _compare_exact(res, kr):
    assert res.nit == kr.nit and res.get("status") == kr.get("status") and res.success == kr.success and res.message == kr.message
    assert len(res.allvecs) == len(kr.allvecs) and all(_same(a, b) for a, b in zip(res.allvecs, kr.allvecs))
    assert _same(np.asarray(res.allfuns, float).reshape(-1), np.asarray(kr.allfuns, float).reshape(-1))
    assert _same(res.allerrs, kr.allerrs) and _same(res.x, kr.x) and _same(res.fun, kr.fun)


def _drain(prob, x0, opts, step):
    """The trace rows of every accepted iteration of a solve advanced `step` passes at a time, its final x and status."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    run = NativeRun(prob, x0, opts)
    rows = [np.zeros((0, _lib.ZF_TRACE_COLS))]
    while run.status == _lib.ZF_RUNNING:
        rows.append(run.advance(step))
    x, status = run.solver.get_x(), run.status
    run.solver.close()
    return np.concatenate(rows), x, status


def _solve_both_ways(case, exp):
    from zfista_amd import minimize_proximal_gradient

    new, kr = _problems(case)
    kw = dict(case.opts, gap_tol=None)
    res = _quiet(minimize_proximal_gradient, *new.callbacks(), case.x0(), return_all=True, **kw)
    ref = _quiet(minimize_proximal_gradient, *kr.callbacks(), case.x0(), return_all=True, **kw)
    _compare_exact(res, ref)
    _compare_oracle(res, exp, case)
    return new, kr, res


@pytest.mark.parametrize("idx", range(len(SM.CASES)), ids=[c.id for c in SM.CASES])
def test_solve_is_the_kronecker_class_bit_for_bit_and_the_oracle_to_1e_10(idx):
    from zfista_amd import minimize_proximal_gradient

    case = SM.CASES[idx]
    new, kr, res = _solve_both_ways(case, _oracle(idx))
    plain = _quiet(minimize_proximal_gradient, *new.callbacks(), case.x0(), **dict(case.opts, gap_tol=None))
    assert plain.nit == res.nit and _same(plain.x, res.x) and plain.fun == res.fun, "without return_all: the same bits"
    # every trace column - F, err, lr, trials among them - for sub_iters 1 / 16, three passes at a time
    for sub in (1, 16):
        opts = dict(_OPTS, **case.opts, sub_iters=sub)
        rows, x, status = _drain(new, case.x0(), opts, 3)
        rows_k, x_k, status_k = _drain(kr, case.x0(), opts, 3)
        assert len(rows) == res.nit and status == status_k and _same(x, x_k) and _same(x, res.x), sub
        assert _same(rows, rows_k), sub


@pytest.mark.parametrize("idx", range(len(SM.ENDINGS)), ids=[c.id for c in SM.ENDINGS])
def test_every_ending_is_the_kronecker_class_and_the_oracle(idx):
    from zfista_amd import _lib

    case = SM.ENDINGS[idx]
    exp = _oracle(idx, "ENDINGS")
    new, kr, res = _solve_both_ways(case, exp)
    opts = dict(_OPTS, **case.opts)
    rows, x, status = _quiet(_drain, new, case.x0(), opts, 2)
    rows_k, x_k, status_k = _quiet(_drain, kr, case.x0(), opts, 2)
    assert status == status_k and _same(rows, rows_k) and _same(x, x_k) and _same(x, res.x)
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), np.asarray(exp.alltrials, np.int64))
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float))


@pytest.mark.parametrize("idx", range(len(SM.ALL_K)), ids=[c.id for c in SM.ALL_K])
def test_every_k_solves_through_the_solvers_own_launches(idx):
    """sparse_multiresponse_cases.ALL_K: every K = 2 .. 16 under both losses, the shape (hence the lane widths of both sweeps) by K % 4.
    The Kronecker class bit for bit - nit, status, message, every iterate, F, err (return_all) and every trace column, lr and trials
    among them; the oracle at 1e-10 and its lr / trial sequences exactly; f, jac_f and the certificate at x = 0 and at the final
    iterate bit for bit."""
    from zfista_amd import _lib

    case = SM.ALL_K[idx]
    exp = _oracle(idx, "ALL_K")
    new, kr, res = _solve_both_ways(case, exp)
    assert res.nit == 30 and np.abs(new.coef(res.x)).max() > 0
    opts = dict(_OPTS, **case.opts)
    rows, x, status = _drain(new, case.x0(), opts, 3)
    rows_k, x_k, status_k = _drain(kr, case.x0(), opts, 3)
    assert len(rows) == res.nit and status == status_k and _same(rows, rows_k) and _same(x, x_k) and _same(x, res.x)
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), np.asarray(exp.alltrials, np.int64))
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float))
    assert int(rows[:, _lib.TR_TRIALS].sum()) > res.nit, "the case must reject trials"
    assert _responses_plan(new, case) == (case.K, 0)
    for xp in (np.zeros(case.n * case.K), np.asarray(res.x)):
        assert _same(new.f(xp), kr.f(xp)), (new.f(xp), kr.f(xp))
        assert _same(new.jac_f(xp), kr.jac_f(xp))
        a, b = new.duality_gap(xp), kr.duality_gap(xp)
        assert all(_same(getattr(a, k), getattr(b, k)) for k in GC.KEYS), (a, b)
        assert a.gap >= 0


def _responses_plan(prob, case):
    """responses_plan() of a solver of the problem: (K, 0) for the sparse kind."""
    from zfista_amd.proximal_gradient import NativeRun

    run = NativeRun(prob, case.x0(), dict(_OPTS, **case.opts))
    plan = run.solver.responses_plan()
    run.solver.close()
    return plan


@pytest.mark.parametrize("idx", SM.SNAPSHOT_CASES, ids=[SM.CASES[i].id for i in SM.SNAPSHOT_CASES])
def test_snapshot_and_resume_across_the_last_chunk(idx, tmp_path):
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    case = SM.CASES[idx]
    new, _ = _problems(case)
    ref_rows, ref_x, _ = _drain(new, case.x0(), dict(_OPTS), 5)
    assert len(ref_rows) == 60
    first = NativeRun(new, case.x0(), dict(_OPTS))
    head = [first.advance(1) for _ in range(57)]
    state = first.snapshot()
    first.solver.close()
    np.savez(tmp_path / "ckpt.npz", **state)
    run = NativeRun.from_snapshot(new, dict(np.load(tmp_path / "ckpt.npz")), dict(_OPTS))
    assert run.solver.responses_plan()[0] == case.K
    while run.status == _lib.ZF_RUNNING:
        head.append(run.advance(5))
    assert _same(np.concatenate(head), ref_rows) and _same(run.solver.get_x(), ref_x)
    run.solver.close()


# ---- (5) TALL with K = 8 ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tall():
    A, B, lam = SM.make_tall()
    return (A, B, lam) + _build("square", A, B, lam, None, None, 0.0, None, SM.TALL_K)


@pytest.mark.parametrize("nesterov", [True, False], ids=["fista", "ista"])
def test_tall_with_eight_responses_is_the_kronecker_class_bit_for_bit(nesterov, tmp_path):
    """320 000 rows of margins: the wide residual kernels; a column of 39 999 elements: a split row of A^T, ten segments of K sums."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    A, B, lam, new, kr = _tall()
    K, n = SM.TALL_K, A.shape[1]
    assert A.shape[0] * K > 32768 and new.plan[1]["split_row"].size >= 1
    opts = dict(_OPTS, max_iter=12, nesterov=nesterov)
    x0 = np.zeros(n * K)
    rows, x, status = _drain(new, x0, opts, 1)
    rows_k, x_k, status_k = _drain(kr, x0, opts, 1)
    assert len(rows) == 12 and status == status_k and _same(rows, rows_k) and _same(x, x_k)
    assert int(rows[:, _lib.TR_TRIALS].sum()) > 12, "the case must reject trials"
    assert len({tuple(c) for c in new.coef(x).T.tolist()}) == K and np.abs(x).max() > 0, "distinct responses, a solve that moved"
    # resumed across a snapshot: the same bits
    run = NativeRun(new, x0, opts)
    head = [run.advance(1) for _ in range(7)]
    state = run.snapshot()
    run.solver.close()
    np.savez(tmp_path / "ckpt.npz", **state)
    run = NativeRun.from_snapshot(new, dict(np.load(tmp_path / "ckpt.npz")), opts)
    while run.status == _lib.ZF_RUNNING:
        head.append(run.advance(2))
    assert _same(np.concatenate(head), rows) and _same(run.solver.get_x(), x)
    run.solver.close()
    if nesterov:   # the oracle on the SciPy closures of the Kronecker matrix
        from oracle import cpu_ref

        ref = S.SparseLeastSquaresL1Ref(SM.kron(A, K), B.reshape(-1), lam, scale=0.5)
        exp = _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), x0, lr=1.0, tol=0.0, max_iter=12, nesterov=True)
        assert exp.nit == 12 and rel_err(x, exp.x) <= TOL


# ---- (6) the certificate in a solve, lockstep cross-validation -----------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["square", "logistic"])
def test_gap_tol_stops_where_a_hand_run_probe_predicts(loss):
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.proximal_gradient import NativeRun

    case = SM.CASES[0 if loss == "square" else 9]
    new, kr = _problems(case)
    P0 = float(new.duality_gap(np.zeros(new.n_features)).primal)
    gap_tol = 1e-3 * P0
    run = NativeRun(new, case.x0(), dict(_OPTS, max_iter=4000))
    checks = 0
    while True:
        run.advance(16)   # gap_every, as passed below
        checks += 1
        if run.duality_gap().gap <= gap_tol or checks > 400:
            break
    x_probe, nit_probe = run.solver.get_x(), run.nit_seen
    run.solver.close()
    kw = dict(lr=1.0, tol=0.0, nesterov=True, max_iter=4000, gap_tol=gap_tol, gap_every=16)
    res = _quiet(minimize_proximal_gradient, *new.callbacks(), case.x0(), **kw)
    assert res.success and res.message == "Duality gap reached gap_tol" and res.dual_gap_checks == checks and res.nit == nit_probe
    assert _same(res.x, x_probe) and 0 <= res.dual_gap <= gap_tol
    ref = _quiet(minimize_proximal_gradient, *kr.callbacks(), case.x0(), **kw)
    assert ref.nit == res.nit and _same(ref.x, res.x) and _same(ref.dual_gap, res.dual_gap)


@pytest.mark.parametrize("loss", ["square", "logistic"])
def test_l1_cv_lockstep_on_sparse_problems_certifies_every_fold(loss):
    from zfista_amd.path import cv_fold_ids, l1_cv, l1_cv_lockstep

    folds = 4
    A, B, lam = SM.make(loss, (120, 40, 0.3), 1, 901)
    m, n = A.shape
    b = B[:, 0].copy()
    prob = _cls(loss, False)(A, b, lam, SM.SCALE[loss])
    lmax = float(prob.lam_max())
    lams = [0.5 * lmax, 0.2 * lmax, 0.05 * lmax]
    P0 = float(prob.duality_gap(np.zeros(n)).primal)
    gap_tol = 1e-6 * P0
    kw = dict(lr=1.0, tol=0.0, nesterov=True, max_iter=20000)
    cv = _quiet(l1_cv_lockstep, prob, lams, folds=folds, seed=3, gap_tol=gap_tol, refit=False, **kw)
    assert np.array_equal(cv.fold_ids, cv_fold_ids(m, folds, 3)) and cv.folds == list(range(folds))
    joint = cv.problems[0]
    assert joint._spmat is prob._spmat and joint.n_responses == folds and isinstance(joint, _cls(loss))
    ids = cv.fold_ids
    slack = 1e-11 * max(P0, 1.0)
    for l, res in enumerate(cv.paths[0]):
        assert res.success and res.dual_gap <= gap_tol
        X = joint.coef(res.x)
        for k in range(folds):
            train = prob.with_lam(lams[l]).with_sample_weight((ids != k).astype(float))
            gk = train.duality_gap(np.ascontiguousarray(X[:, k]))
            assert gk.gap <= gap_tol + slack, (l, k, float(gk.gap), gap_tol)
            score = prob.with_sample_weight((ids == k).astype(float)).f(np.ascontiguousarray(X[:, k])) / float((ids == k).sum())
            assert score == cv.scores[k, l]
    if loss == "square":
        ref = _quiet(l1_cv, prob, lams, folds=folds, seed=3, gap_tol=gap_tol, refit=False, **kw)
        assert np.array_equal(ref.fold_ids, cv.fold_ids)
        order = np.sort(ref.mean)
        assert order[1] - order[0] > 1e-3 * order[0], "the case must separate the runner-up"
        assert cv.lam_best == ref.lam_best


# ---- (7) interface ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["square", "logistic"])
def test_one_response_is_the_plain_sparse_class_bit_for_bit(loss):
    from zfista_amd import minimize_proximal_gradient

    A, B, lam = SM.make(loss, "a", 1, 55)
    n = A.shape[1]
    plain = _cls(loss, False)(A, B[:, 0].copy(), lam, SM.SCALE[loss])
    one = _cls(loss)(A, B, lam, SM.SCALE[loss])
    assert one.n_responses == 1 and "responses" not in one._descriptor()[0]
    x = np.random.default_rng(1).standard_normal(n)
    assert one.f(x) == plain.f(x) and _same(one.jac_f(x), plain.jac_f(x))
    assert one.duality_gap(x).gap == plain.duality_gap(x).gap
    kw = dict(lr=1.0, tol=0.0, max_iter=40, nesterov=True)
    a = _quiet(minimize_proximal_gradient, *one.callbacks(), np.zeros(n), **kw)
    b = _quiet(minimize_proximal_gradient, *plain.callbacks(), np.zeros(n), **kw)
    assert a.nit == b.nit == 40 and _same(a.x, b.x) and a.fun == b.fun


def test_with_responses_shares_the_handle_and_streams_give_the_same_bits():
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.replicas import solve_on_streams

    case = SM.CASES[2]
    A, B, lam, Wt, Pf, l2 = case.data()
    base = _cls("square", False)(A, B[:, 0].copy(), lam, 0.5)
    sib = base.with_responses(B)
    assert sib._spmat is base._spmat and sib.n_responses == case.K and sib.n_features == case.n * case.K
    assert sib.with_lam(0.5 * lam)._spmat is base._spmat
    direct = _cls("square")(A, B, lam, 0.5)
    n = sib.n_features
    kw = dict(lr=1.0, tol=0.0, max_iter=40, nesterov=True)
    alone = [_quiet(minimize_proximal_gradient, *p.callbacks(), np.zeros(n), **kw) for p in (sib, direct)]
    assert _same(alone[0].x, alone[1].x)
    shaped = _quiet(minimize_proximal_gradient, *sib.callbacks(), np.zeros((case.n, case.K)), **kw)
    assert _same(shaped.x, alone[0].x) and shaped.x.shape == (n,)
    both = solve_on_streams([(p, np.zeros(n), kw) for p in (sib, direct)], streams=2)
    for a, c in zip(alone, both):
        assert a.nit == c.nit == 40 and _same(a.x, c.x) and a.fun == c.fun
    path = _quiet(__import__("zfista_amd.path", fromlist=["l1_path"]).l1_path, sib, [0.5 * lam, 0.2 * lam], gap_tol=None, **kw)
    assert len(path) == 2 and all(r.x.shape == (n,) for r in path)


def test_the_creator_refuses_and_the_setter_still_refuses_the_sparse_kinds():
    import ctypes as C

    import torch

    from zfista_amd import _lib
    from zfista_amd.engine import DeviceSolver

    case = SM.CASES[0]
    A, B, lam, _, _, _ = case.data()
    K, (m, n) = case.K, A.shape
    new = _cls("square")(A, B, lam)
    fields, keep = new._descriptor()
    assert fields["responses"] == K and fields["m_rows"] == m * K and fields["n"] == n * K and fields["A"] is None
    options = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=3, max_backtrack_iter=10)
    lib = _lib.require_gpu()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def create(K_arg, opts=options, **over):
        d, o, h = _lib.ProblemDesc(), _lib.Options(), C.c_void_p()
        for k, v in dict(fields, **over).items():
            if k not in ("spmat", "responses"):
                setattr(d, k, v)
        for k, v in opts.items():
            setattr(o, k, v)
        rc = lib.zf_solver_create_sparse_responses(C.byref(h), C.byref(d), C.c_void_p(fields["spmat"]), K_arg, C.byref(o), stream)
        msg = lib.zf_last_error()
        if rc == 0:
            assert lib.zf_solver_destroy(h) == 0
        return rc, msg

    assert create(K)[0] == 0
    for bad in (1, 0, -1, 17):
        rc, msg = create(bad)
        assert rc == -2 and b"2 .. 16" in msg
    rc, msg = create(K + 1)
    assert rc == -2 and b"K times the matrix handle's" in msg
    rc, msg = create(K, m_rows=m)
    assert rc == -2 and b"K times the matrix handle's" in msg
    rc, msg = create(K, kind=_lib.ZF_PROBLEM_LEAST_SQUARES_L1)
    assert rc == -2 and b"ZF_PROBLEM_SPARSE_LS_L1" in msg
    rc, msg = create(K, world=2)
    assert rc == -2 and b"world > 1" in msg
    for mode in (_lib.ZF_ACCEPT_REMAINDER, _lib.ZF_ACCEPT_RESOLVED):
        rc, msg = create(K, dict(options, accept_mode=mode))
        assert rc == -2 and b"ZF_ACCEPT_REMAINDER" in msg
    # the plain creator keeps its dimension check; the setter keeps refusing both sparse kinds
    d, o, h = _lib.ProblemDesc(), _lib.Options(), C.c_void_p()
    for k, v in fields.items():
        if k not in ("spmat", "responses"):
            setattr(d, k, v)
    for k, v in options.items():
        setattr(o, k, v)
    assert lib.zf_solver_create_sparse(C.byref(h), C.byref(d), C.c_void_p(fields["spmat"]), C.byref(o), stream) == -2
    assert b"differ from the matrix handle's" in lib.zf_last_error()
    for loss in ("square", "logistic"):
        plain = _cls(loss, False)(A, np.sign(B[:, 0]) if loss == "logistic" else B[:, 0].copy(), lam)
        f1, k1 = plain._descriptor()
        s = DeviceSolver(f1, options, keepalive=k1)
        assert lib.zf_solver_set_responses(s.handle, 2) == -2 and b"only for" in lib.zf_last_error()
        assert s.responses_plan() == (1, 0) and s.ls_plan()[0] == 5
        s.close()
    # a solver of the new creator: the plain sparse plan, K in slot 4; the setters it excludes; those it composes with
    s = DeviceSolver(fields, options, keepalive=keep)
    plain = _cls("square", False)(A, B[:, 0].copy(), lam)
    f1, k1 = plain._descriptor()
    s1 = DeviceSolver(f1, options, keepalive=k1)
    assert s.ls_plan() == s1.ls_plan() and s.ls_plan()[:3] == (5,) + SM.SHAPE_LANES[case.shape] and s.responses_plan() == (K, 0)
    s1.close()
    assert lib.zf_solver_set_huber(s.handle, 0.5) == -2 and b"responses" in lib.zf_last_error()
    assert lib.zf_solver_set_poisson(s.handle) == -2 and b"responses" in lib.zf_last_error()
    assert lib.zf_solver_set_responses(s.handle, K) == -2
    wd = torch.ones(m * K, dtype=torch.float64, device="cuda")
    pd = torch.ones(n * K, dtype=torch.float64, device="cuda")
    assert lib.zf_solver_set_row_weights(s.handle, C.c_void_p(wd.data_ptr())) == 0
    assert lib.zf_solver_set_penalty_factors(s.handle, C.c_void_p(pd.data_ptr())) == 0
    x0 = torch.zeros(n * K, dtype=torch.float64, device="cuda")
    s.init(x0.data_ptr())
    s.close()
    # the standalone entries' argument checks
    P = C.c_void_p(_lib.ptr(np.zeros(4)))
    f = C.c_double(0.0)
    import evaldesc as E

    H = new._spmat.value
    for bad in (17,):
        assert E.point(E.sparse(P, spmat=H, K=bad), P, C.byref(f)) == -2 and b"K must be 1 .. 16" in lib.zf_last_error()
        assert E.gap(E.sparse(P, spmat=H, K=bad), P, P, 10) == -2
    assert E.point(E.sparse(P, spmat=H, K=2, loss=2, delta=1.0), P, C.byref(f)) == -2 and b"ZF_LOSS_SQUARE or ZF_LOSS_LOGISTIC" in lib.zf_last_error()
    assert E.point(E.sparse(P, spmat=None, K=2), P, C.byref(f)) == -2
    assert E.gap(E.sparse(P, spmat=H, K=2, p=P, l2=0.25), P, P, 10) == -2 and b"penalty factors and l2" in lib.zf_last_error()
    assert lib.zf_spmat_mr_apply(new._spmat.value, 0, 17, 1.0, P, P) == -2 and lib.zf_spmat_mr_apply(None, 0, 2, 1.0, P, P) == -2


# zf_solver_launch_counts of the fixed plain solve below on the build of the commit before this feature, from a run of that build:
# (trial steps issued, shape-specific trial kernels launched).  Both count the chained trial kernels of the separable kind and are 0
# for a sparse solver there - and must stay so: a plain sparse solver launches what it launched.
PARENT_LAUNCH_COUNTS = (0, 0)
# ... and computes what it computed: nit, F and the first 16 hex digits of sha256(x) of that solve on that build
PARENT_SOLVE = (30, "0x1.3ca72c9e3b0b4p+4", "d8aec96d94283713")


def test_a_plain_sparse_solver_launches_what_the_parent_commit_launched():
    from zfista_amd import minimize_proximal_gradient

    A, b, lam = S.make_sparse(*S.SMALL[0])
    n = A.shape[1]
    plain = _cls("square", False)(A, b, lam)
    opts = dict(_OPTS, max_iter=30)

    def counts():
        from zfista_amd import _lib
        from zfista_amd.proximal_gradient import NativeRun

        run = NativeRun(plain, np.zeros(n), opts)
        while run.status == _lib.ZF_RUNNING:
            run.advance(4)
        out = run.solver.launch_counts(), run.solver.ls_plan(), run.solver.responses_plan(), run.solver.get_x()
        solve = (run.nit_seen, float(run.solver.ctl.F_old).hex(), hashlib.sha256(np.ascontiguousarray(out[3]).tobytes()).hexdigest()[:16])
        run.solver.close()
        return out + (solve,)

    before = counts()
    case = SM.CASES[1]
    _quiet(minimize_proximal_gradient, *_problems(case)[0].callbacks(), case.x0(), **case.opts)
    after = counts()
    print("plain sparse launch counts:", before[0])
    assert before[0] == after[0] == PARENT_LAUNCH_COUNTS and before[1] == after[1] and before[2] == after[2] == (1, 0)
    assert _same(before[3], after[3]) and before[4] == after[4] == PARENT_SOLVE, before[4]
