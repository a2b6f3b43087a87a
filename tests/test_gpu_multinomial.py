"""GPU: multinomial (softmax) regression on the K-response sweeps (csrc/zf_kernels_softmax.h, zf_solver_set_multinomial,
MultinomialL1 / SparseMultinomialL1).

(1) The row kernels and the certificate element-wise against the long-double restatement of multinomial_cases, inside its a-priori
    bounds, through zf_margins_eval / zf_margins_gap: every K = 2 .. 16 (each is a kernel instantiation of its own), the row counts
    of multinomial_cases.eval_rows (both shapes of a rows pass, the last narrow and the first wide count, a short last chunk),
    n in {5, 66}, dense and sparse, with and without weights.  ZF_MN_BOUNDS_RECORD=1 appends the worst error / bound ratios to
    profiles/multinomial_bounds.jsonl (any other value: to that path).
(2) Margins at +-700 and past exp's underflow stay finite, a NaN or infinite margin gives a NaN f (-inf on a class with y > 0: +inf); rows that are not there give +0 bits; rows are independent.
(3) Every case, ending and ALL_K entry against the CPU oracle at 1e-10 with the lr and trial sequences exactly; sub_iters, return_all,
    passes three at a time, snapshots; dense and sparse take the same trials.
(4) The certificate: bounds at final iterates, zero rows gap at alpha = 1, the live solver's, gap_tol.
(5) lam_max, K = 2 against LogisticL1, l1_path, with_classes, streams, unchanged defaults, refusals at the C level."""
import contextlib
import ctypes as C
import functools
import hashlib
import io
import json
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import multinomial_cases as MC
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-10
FORMS = ("dense", "csr")


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with contextlib.redirect_stdout(io.StringIO()):
            return fn(*a, **k)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _record(row):
    where = os.environ.get("ZF_MN_BOUNDS_RECORD")
    if not where:
        return
    path = os.path.join(ROOT, "profiles", "multinomial_bounds.jsonl") if where == "1" else where
    with open(path, "a") as fh:
        fh.write(json.dumps(row) + "\n")


def _make(storage, A, Y, lam, **kw):
    from zfista_amd import problems as Z

    if storage == "csr":
        return Z.SparseMultinomialL1(sp.csr_matrix(A), Y, lam, **kw)
    return Z.MultinomialL1(A.toarray() if sp.issparse(A) else A, Y, lam, **kw)


def _problem(case, storage="dense"):
    A, Y, lam, w, Pf, l2 = case.data()
    return _make(storage, A, Y, lam, scale=MC.SCALE, bounds=case.box, l2=l2, sample_weight=w, penalty_factor=Pf)


@functools.lru_cache(maxsize=None)
def _oracle(idx, table="CASES"):
    """The reference solver on the per-row closures - computed once per case, shared, left unchanged."""
    from oracle import cpu_ref

    case = getattr(MC, table)[idx]
    return _quiet(cpu_ref.minimize_proximal_gradient, *case.ref().callbacks(), case.x0(), return_all=True, **case.opts)


# ---- (1) the row kernels and the certificate, element-wise -----------------------------------------------------------------------
def _gapdict(got, keys):
    return {k: getattr(got, k) for k in keys}


@pytest.mark.parametrize("K", MC.KS)
def test_row_kernels_and_certificate_within_the_longdouble_bounds(K):
    worst = dict(f=0.0, grad=0.0, gap=0.0)
    for j, m in enumerate(MC.eval_rows(K)):
        n = 66 if m <= 65 else 5
        rng = np.random.default_rng(1000 * K + m)
        A = rng.standard_normal((m, n))
        X = 0.7 * rng.standard_normal((n, K))
        Y = rng.dirichlet(np.ones(K), m) if j % 2 else MC.one_hot(rng.integers(0, K, m), K)
        w = None if j % 3 else np.where(rng.random(m) < 0.2, 0.0, 0.25 + 2 * rng.random(m))
        if w is not None:
            w[0] = 1.0
        vals0, _, _ = MC.gap_longdouble(A, Y, X, 1.0, w=w)
        lam = 0.3 * float(vals0["grad_inf"])   # (alpha = 0.3: the rows that need alpha are formed)
        vals, bounds, extra = MC.gap_longdouble(A, Y, X, lam, w=w)
        for storage in FORMS:
            prob = _make(storage, A, Y, lam, sample_weight=w)
            f = prob.f(X)
            G = prob.jac_f(X).reshape(n, K)
            ferr = abs(float(np.longdouble(f) - vals["f"])) / bounds["f"]
            gerr = float(np.max(np.abs((G.astype(np.longdouble) - extra["grad"]).astype(np.float64)) / extra["dgrad"]))
            ratios = MC.worst_ratio(_gapdict(prob.duality_gap(X), MC.KEYS8), vals, bounds)
            assert ferr <= 1.0 and gerr <= 1.0 and max(ratios.values()) <= 1.0, (K, m, storage, ferr, gerr, ratios)
            worst = dict(f=max(worst["f"], ferr), grad=max(worst["grad"], gerr), gap=max(worst["gap"], max(ratios.values())))
    print(f"K={K}: worst error / bound: f {worst['f']:.3g}, gradient element {worst['grad']:.3g}, certificate {worst['gap']:.3g}")
    _record(dict(test="rows", K=K, rows=MC.eval_rows(K), **worst))


# ---- (2) edges of a row ----------------------------------------------------------------------------------------------------------------
def _identity(storage, m):
    return sp.identity(m, format="csr", dtype=np.float64) if storage == "csr" else np.eye(m)


@pytest.mark.parametrize("storage", FORMS)
@pytest.mark.parametrize("K,m", [(2, 65), (3, 1025), (16, 2049), (7, 2049)])
def test_margins_at_700_stay_finite_and_a_nan_or_infinite_margin_gives_nan(K, m, storage):
    """A = I: the margins are the rows of X.  One class at +700 / -700 in two rows (p underflows to 0 where y > 0): f, psi and the
    certificate stay finite and inside their bounds.  A NaN, +inf or -inf margin on a class the row does not have: f is NaN.  On
    the row's own class (y_k > 0) NaN and +inf give NaN and -inf gives f = +inf: phi = log S + y_k (-d_k) = +inf with every other
    term finite (include/zfista_hip.h says so)."""
    rng = np.random.default_rng(K + m)
    Z = rng.uniform(-3, 3, (m, K))
    lab = rng.integers(0, K, m)
    Z[m // 2, (lab[m // 2] + 1) % K] = 700.0
    Z[m // 3, lab[m // 3]] = -700.0
    Y = MC.one_hot(lab, K)
    prob = _make(storage, _identity(storage, m), Y, 0.1)
    f, G = prob.f(Z), prob.jac_f(Z).reshape(m, K)
    fl, fb, psi, pb = MC.loss_longdouble(Z, Y)
    assert np.isfinite(f) and np.isfinite(G).all() and abs(float(np.longdouble(f) - fl)) <= fb
    assert np.all(np.abs((G.astype(np.longdouble) - psi).astype(np.float64)) <= pb), "scale = 1 and A = I: the gradient is psi itself"
    assert abs(G[m // 2, lab[m // 2]] + 1.0) <= 1e-15 and abs(G[m // 3, lab[m // 3]] + 1.0) <= 1e-15
    got = prob.duality_gap(Z)
    vals, bounds, _ = MC.gap_longdouble(_identity("dense", m), Y, Z, 0.1)
    assert all(np.isfinite(getattr(got, k)) for k in MC.KEYS8) and got.rows_gap > 0
    assert max(MC.worst_ratio(_gapdict(got, MC.KEYS8), vals, bounds).values()) <= 1.0
    for bad in (np.nan, np.inf, -np.inf):
        Zb = Z.copy()
        Zb[m - 1, (lab[m - 1] + 1) % K] = bad   # (a class the row does not have: 0 * inf for -inf)
        with np.errstate(invalid="ignore"):
            assert np.isnan(prob.f(Zb)), bad
        Zb = Z.copy()
        Zb[m - 1, lab[m - 1]] = bad   # (the row's own class: y_k = 1)
        with np.errstate(invalid="ignore"):
            got = prob.f(Zb)
        # (the dense identity multiplies the infinity by its zeros: every margin of that column is NaN before the loss sees it)
        assert got == np.inf if bad == -np.inf and storage == "csr" else np.isnan(got), (bad, got)


@pytest.mark.parametrize("storage", FORMS)
@pytest.mark.parametrize("K,m", [(2, 65), (3, 1025), (16, 2049)])
def test_margins_past_the_underflow_of_exp_stay_finite(K, m, storage):
    """exp(-700) is still a normal number; exp(-5000) is 0.  The LAST class at +5000 in two rows: every other p_k of those rows is
    exactly 0.  In row r1 the label is the last class (p_k = 0 where y_k = 0: v_k = 0, the 0 log 0 of ZF_GS_ENT), in row r2 it is
    class 0 (p_k = 0 where y_k > 0: log p_k from d_k - log S).  A maximum that misses the last class overflows exp here."""
    rng = np.random.default_rng(11 * K + m)
    Z = rng.uniform(-3, 3, (m, K))
    lab = rng.integers(0, K, m)
    r1, r2 = m // 2, m // 3
    Z[r1, K - 1] = Z[r2, K - 1] = 5000.0
    lab[r1], lab[r2] = K - 1, 0
    Y = MC.one_hot(lab, K)
    prob = _make(storage, _identity(storage, m), Y, 0.1)
    f, G = prob.f(Z), prob.jac_f(Z).reshape(m, K)
    fl, fb, psi, pb = MC.loss_longdouble(Z, Y)
    assert np.isfinite(f) and np.isfinite(G).all() and abs(float(np.longdouble(f) - fl)) <= fb
    assert np.all(np.abs((G.astype(np.longdouble) - psi).astype(np.float64)) <= pb)
    assert not G[r1].any() and G[r2, 0] == -1.0 and G[r2, K - 1] == 1.0 and not G[r2, 1:K - 1].any()
    vals0, _, _ = MC.gap_longdouble(_identity("dense", m), Y, Z, 1.0)
    for lam in (0.3 * float(vals0["grad_inf"]), 2.0 * float(vals0["grad_inf"])):   # alpha = 0.3, and alpha = 1 (v = p)
        got = prob.with_lam(lam).duality_gap(Z)
        vals, bounds, _ = MC.gap_longdouble(_identity("dense", m), Y, Z, lam)
        assert all(np.isfinite(getattr(got, k)) for k in MC.KEYS8), got
        assert max(MC.worst_ratio(_gapdict(got, MC.KEYS8), vals, bounds).values()) <= 1.0
        assert (got.alpha == 1.0 and _bits(got.rows_gap) == 0) if lam > float(vals0["grad_inf"]) else got.rows_gap > 0


# (an identity of 16385 rows is 2 GB in dense storage: the sparse class alone takes that count)
@pytest.mark.parametrize("K,m,storage", [(K, m, st) for K, m in [(2, 1), (5, 65), (3, 1025), (16, 2049), (2, 16385)] for st in FORMS
                                         if st == "csr" or m <= 2049])
def test_rows_that_are_not_there_give_plus_zero_bits(K, m, storage):
    """Rows with w_i = 0 hold NaN in y (and, under the sparse identity, one a NaN margin): psi is +0 there bit for bit and f is the long-double f of the other
    rows; in both shapes of the rows pass (16 x 2049 and 2 x 16385 entries take the wide one)."""
    rng = np.random.default_rng(3 * K + m)
    Z = rng.uniform(-4, 4, (m, K))
    Y = rng.dirichlet(np.ones(K), m)
    w = np.where(rng.random(m) < 0.3, 0.0, 0.5 + rng.random(m))
    w[0] = 0.0 if m > 1 else 1.0
    w[m - 1] = 1.0
    off = w == 0
    Y[off] = np.nan
    prob = _make(storage, _identity(storage, m), Y, 0.1, sample_weight=w)
    Zn = Z.copy()
    if off.any() and storage == "csr":   # (a dense identity would carry the NaN into every row: 0 * NaN)
        Zn[np.flatnonzero(off)[0], 0] = np.nan
    f, G = prob.f(Zn), prob.jac_f(Zn).reshape(m, K)
    assert not _bits(G[off]).any(), "+0 bits"
    fl, fb, psi, pb = MC.loss_longdouble(Z, Y, w=w)
    assert abs(float(np.longdouble(f) - fl)) <= fb and np.all(np.abs((G.astype(np.longdouble) - psi).astype(np.float64)) <= pb)
    # the weight of a row is read at w[i K], once: psi_i = w_i psi_i(unweighted) in one product
    G1 = _make(storage, _identity(storage, m), np.where(off[:, None], 1.0 / K, Y), 0.1).jac_f(Z).reshape(m, K)
    assert np.array_equal(_bits(G[~off]), _bits(w[~off, None] * G1[~off]))


@pytest.mark.parametrize("K", MC.KS)
def test_a_row_touches_no_other(K):
    m = 2049 if K == 16 else 131   # (16 x 2049 entries: the wide shape, chunks of whole rows)
    rng = np.random.default_rng(K)
    Z = rng.uniform(-4, 4, (m, K))
    Y = rng.dirichlet(np.ones(K), m)
    prob = _make("csr", _identity("csr", m), Y, 0.1)
    G = prob.jac_f(Z).reshape(m, K)
    for i in (0, m // 2, m - 1):
        Z2 = Z.copy()
        Z2[i] = rng.uniform(-4, 4, K)
        G2 = prob.jac_f(Z2).reshape(m, K)
        others = np.arange(m) != i
        assert np.array_equal(_bits(G[others]), _bits(G2[others])) and not np.array_equal(G[i], G2[i])
    assert np.max(np.abs(G.sum(axis=1))) <= 4 * K * MC.U, "softmax and y sum to 1 in every row"


# ---- (3) solves against the oracle -------------------------------------------------------------------------------------------------
def _compare(res, exp, case):
    assert res.nit == exp.nit and res.success == exp.success, (res.nit, exp.nit, res.message, exp.message)
    assert res.message == exp.message
    assert len(res.allvecs) == len(exp.allvecs)
    worst = 0.0
    for a, b in zip(res.allvecs, exp.allvecs):
        worst = max(worst, rel_err(a, b) if np.any(b) else float(np.max(np.abs(a))))
    fa, fb = np.asarray(res.allfuns, float).reshape(-1), np.asarray(exp.allfuns, float).reshape(-1)
    ferr = float(np.max(np.abs(fa - fb) / np.abs(fb)))
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


def _solve_and_check(case, exp, with_subs):
    from zfista_amd import _lib, minimize_proximal_gradient

    kw = dict(case.opts, gap_tol=None)
    prob = _problem(case, "dense")
    res = _quiet(minimize_proximal_gradient, *prob.callbacks(), case.x0(), return_all=True, **kw)
    _compare(res, exp, case)
    # without return_all: chunks of doubling length - the same bits
    plain = _quiet(minimize_proximal_gradient, *prob.callbacks(), case.x0(), **kw)
    assert plain.nit == res.nit and np.array_equal(_bits(plain.x), _bits(res.x)) and plain.fun == res.fun
    # three passes at a time, and sub_iters 1 / 16 (a margins solver runs one trial per pass whatever is asked)
    for sub in (1, 16) if with_subs else (1,):
        rows, x = _drain(prob, case, 3, sub_iters=sub)
        assert np.array_equal(_bits(x), _bits(res.x)) and len(rows) == res.nit, sub
        assert np.array_equal(rows[:, _lib.TR_F], np.asarray(res.allfuns[1:], float).reshape(-1))
        _check_sequences(rows, exp)
    # the sparse class on the same data: the oracle again, the same trials, the same F to the last digits of the sweeps
    sres = _quiet(minimize_proximal_gradient, *_problem(case, "csr").callbacks(), case.x0(), return_all=True, **kw)
    _compare(sres, exp, case)
    srows, _ = _drain(_problem(case, "csr"), case, 3)
    _check_sequences(srows, exp)
    assert np.array_equal(srows[:, _lib.TR_TRIALS], rows[:, _lib.TR_TRIALS]) and np.array_equal(srows[:, _lib.TR_LR], rows[:, _lib.TR_LR])
    return prob, res


@pytest.mark.parametrize("idx", range(len(MC.CASES)), ids=[c.id for c in MC.CASES])
def test_solve_vs_oracle_dense_and_sparse(idx):
    case = MC.CASES[idx]
    prob, res = _solve_and_check(case, _oracle(idx), True)
    assert np.any(res.x != 0)
    if not case.box and case.factors != "zero":   # the certificate at the final iterate, inside its bounds
        A, Y, lam, w, Pf, l2 = case.data()
        vals, bounds, _ = MC.gap_longdouble(A, Y, res.x, lam, MC.SCALE, l2, w, Pf)
        keys = MC.KEYS10 if l2 > 0 else MC.KEYS8
        for storage in FORMS:
            got = _problem(case, storage).duality_gap(res.x)
            ratios = MC.worst_ratio(_gapdict(got, keys), vals, bounds)
            assert max(ratios.values()) <= 1.0 and got.gap >= 0 and got.rows_gap >= 0, (storage, ratios)
            assert got.primal - got.dual >= -bounds["primal"] - bounds["dual"], "P - D >= 0"
        _record(dict(test="final", case=case.id, ratio=max(ratios.values())))


@pytest.mark.parametrize("idx", range(len(MC.ENDINGS)), ids=[c.id for c in MC.ENDINGS])
def test_every_ending_as_the_oracle(idx):
    _solve_and_check(MC.ENDINGS[idx], _oracle(idx, "ENDINGS"), False)


@pytest.mark.parametrize("storage", FORMS)
@pytest.mark.parametrize("idx", range(len(MC.ALL_K)), ids=[c.id for c in MC.ALL_K])
def test_all_k_solves(idx, storage):
    """One 30-iteration solve per K through the solver's ring-indexed launches (the rows kernels inside the loop: ctl, cur, slot, the
    extrapolation at y), against the oracle with the sequences exactly."""
    from zfista_amd import _lib, minimize_proximal_gradient

    case = MC.ALL_K[idx]
    exp = _oracle(idx, "ALL_K")
    prob = _problem(case, storage)
    res = _quiet(minimize_proximal_gradient, *prob.callbacks(), case.x0(), return_all=True, **case.opts)
    _compare(res, exp, case)
    for sub in (1, 16):
        rows, x = _drain(prob, case, 3, sub_iters=sub)
        _check_sequences(rows, exp)
        assert np.array_equal(_bits(x), _bits(res.x))
        assert np.array_equal(rows[:, _lib.TR_F], np.asarray(res.allfuns[1:], float).reshape(-1))
    assert int(rows[:, _lib.TR_TRIALS].sum()) > res.nit, "the case must reject trials"


@pytest.mark.parametrize("storage", FORMS)
@pytest.mark.parametrize("idx", MC.SNAPSHOT_CASES, ids=[MC.CASES[i].id for i in MC.SNAPSHOT_CASES])
def test_snapshot_and_resume_across_the_last_chunk_is_bit_identical(idx, storage, tmp_path):
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    case = MC.CASES[idx]
    prob = _problem(case, storage)
    rows, x = _drain(prob, case, 4)
    opts = dict(_OPTS, **case.opts)
    run = NativeRun(prob, case.x0(), opts)
    got = [run.advance(1) for _ in range(len(rows) - 3)]   # (at least one pass per iteration: stops inside the last chunk)
    assert run.status == _lib.ZF_RUNNING
    state = run.snapshot()
    run.solver.close()
    np.savez(tmp_path / "ckpt.npz", **state)
    run = NativeRun.from_snapshot(_problem(case, storage), dict(np.load(tmp_path / "ckpt.npz")), opts)
    while run.status == _lib.ZF_RUNNING:
        got.append(run.advance(2))
    assert np.array_equal(np.concatenate(got), rows) and np.array_equal(_bits(run.solver.get_x()), _bits(x))
    run.solver.close()


@pytest.mark.parametrize("storage", FORMS)
@pytest.mark.parametrize("ci", range(len(MC.GOLDEN_CASES)), ids=[c.id for c in MC.GOLDEN_CASES])
def test_solve_vs_the_reference_fixture(ci, storage, golden):
    """tests/golden/g20_multinomial.npz: what the reference's solver returned on the per-row closures for three small problems."""
    from zfista_amd import _lib, minimize_proximal_gradient

    G, pre, case = golden("g20_multinomial.npz"), MC.golden_prefix(ci), MC.GOLDEN_CASES[ci]
    prob = _problem(case, storage)
    assert float(G(f"{pre}.lam")) == prob.lam
    res = _quiet(minimize_proximal_gradient, *prob.callbacks(), case.x0(), return_all=True, **case.opts)
    rows, x = _drain(prob, case, 3)
    assert res.nit == int(G(f"{pre}.nit")) == 60 and res.status == int(G(f"{pre}.status")) and np.array_equal(_bits(x), _bits(res.x))
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), G(f"{pre}.alltrials")) and rows[:, _lib.TR_TRIALS].sum() > 60
    assert np.array_equal(rows[:, _lib.TR_LR], G(f"{pre}.alllrs"))
    assert rel_err(res.x, G(f"{pre}.x")) <= TOL
    for k, v in zip(G(f"{pre}.kept"), G(f"{pre}.vecs")):
        if np.any(v):
            assert rel_err(res.allvecs[k][::MC.GOLDEN_STRIDE], v) <= TOL, k
    np.testing.assert_allclose(res.allfuns, G(f"{pre}.allfuns"), rtol=TOL, atol=0)
    np.testing.assert_allclose(res.allerrs, G(f"{pre}.allerrs"), rtol=TOL, atol=2 * TOL * float(G(f"{pre}.xnorm")))


def test_a_tall_solve_takes_the_wide_shape_inside_the_loop():
    """m K > 32768: every rows pass of a trial runs many workgroups on chunks of whole rows and the finish kernel, with its guards."""
    from zfista_amd import _lib, minimize_proximal_gradient
    from oracle import cpu_ref

    for K, m in ((16, 2100), (3, 11000)):
        case = MC.Case(K, m, 6, 800 + K, weights="real" if K == 3 else None, opts=dict(max_iter=8))
        assert m * K > MC.WIDE
        exp = _quiet(cpu_ref.minimize_proximal_gradient, *case.ref().callbacks(), case.x0(), return_all=True, **case.opts)
        for storage in FORMS:
            prob = _problem(case, storage)
            res = _quiet(minimize_proximal_gradient, *prob.callbacks(), case.x0(), return_all=True, **case.opts)
            _compare(res, exp, case)
            rows, x = _drain(prob, case, 2)
            _check_sequences(rows, exp)
            assert np.array_equal(_bits(x), _bits(res.x)) and int(rows[:, _lib.TR_TRIALS].sum()) > exp.nit


# ---- (4) the certificate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", FORMS)
@pytest.mark.parametrize("K,m", [(2, 300), (5, 1025), (16, 2100)])
def test_the_rows_gap_is_exactly_zero_at_alpha_one(K, m, storage):
    A, Y, _ = MC.make(m, 40, K, 50 + K, labels="soft")
    for w in (None, MC.make_weights(m, 50 + K, "real")):
        prob0 = _make(storage, A, Y, 1.0, sample_weight=w)
        big = 2.0 * float(prob0.lam_max())
        got = prob0.with_lam(big).duality_gap(np.zeros(40 * K))
        assert got.alpha == 1.0 and _bits(got.rows_gap) == 0 and got.gap == 0.0
        mass = float(m if w is None else w.sum()) * np.log(K)   # f(0) = sum w log K; D = -sum w sum_k p log p at p = 1 / K: the same
        assert abs(float(got.primal) - mass) <= 1e-12 * mass and abs(float(got.dual) - mass) <= 1e-12 * mass


_BASE = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=100000, max_backtrack_iter=100, nesterov=True,
             nesterov_ratio=(0, 0.25), deprecated=False, return_all=False, verbose=False)


def _walk(prob, passes, gap_after=()):
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    run = NativeRun(prob, np.zeros(prob.n_features), dict(_BASE))
    rows, gaps = [np.zeros((0, _lib.ZF_TRACE_COLS))], {}
    for k in range(passes):
        rows.append(run.advance(1))
        if k in gap_after:
            gaps[k] = run.duality_gap()
    ctl, _ = run.solver.poll()
    out = dict(rows=np.concatenate(rows), x=run.solver.get_x(), nit=int(ctl.nit), lr=ctl.lr, F=ctl.F_old, trials=int(ctl.total_trials), gaps=gaps)
    run.solver.close()
    return out


@pytest.mark.parametrize("variant", ["l1", "l2", "weights", "factors"])
@pytest.mark.parametrize("storage", FORMS)
def test_the_gap_of_a_live_solve_is_the_standalone_certificate(storage, variant):
    K, m, n = 5, 300, 1100   # n K = 5500: more than one chunk of the n-passes
    A, Y, lam = MC.make(m, n, K, 61, labels="soft", density=0.1)
    kw = dict(l2=lam / 100 if variant == "l2" else 0.0, sample_weight=MC.make_weights(m, 61, "real") if variant == "weights" else None,
              penalty_factor=MC.make_factors(n, K, 61, "pos") if variant == "factors" else None)
    prob = _make(storage, A, Y, lam, **kw)
    keys = MC.KEYS10 if variant == "l2" else MC.KEYS8
    passes = 25
    plain = _walk(prob, passes)
    assert plain["trials"] > plain["nit"] > 0, "the case must backtrack and accept"
    probed = _walk(prob, passes, gap_after=range(passes))
    assert (plain["nit"], plain["lr"], plain["F"], plain["trials"]) == (probed["nit"], probed["lr"], probed["F"], probed["trials"])
    assert np.array_equal(plain["rows"], probed["rows"]) and np.array_equal(plain["x"], probed["x"]), "a probed solve is the solve"
    live, alone = probed["gaps"][passes - 1], prob.duality_gap(probed["x"])
    assert np.array_equal(_bits([getattr(live, k) for k in keys]), _bits([getattr(alone, k) for k in keys])), (live, alone)
    vals, bounds, _ = MC.gap_longdouble(A, Y, probed["x"], lam, MC.SCALE, kw["l2"], kw["sample_weight"], kw["penalty_factor"])
    ratios = MC.worst_ratio(_gapdict(live, keys), vals, bounds)
    assert max(ratios.values()) <= 1.0 and live.gap >= 0 and 0 < live.alpha <= 1, ratios


@pytest.mark.parametrize("storage", FORMS)
def test_gap_tol_stops_where_a_hand_run_probe_predicts_with_a_valid_certificate(storage):
    from zfista_amd import minimize_proximal_gradient as solve
    from zfista_amd.proximal_gradient import NativeRun

    case = MC.GAP_CASE
    A, Y, _, _, _, _ = case.data()
    n = case.n * case.K
    prob0 = _make(storage, A, Y, 1.0)
    lam = 0.5 * float(prob0.lam_max())
    prob = prob0.with_lam(lam)
    P0 = float(MC.gap_longdouble(A, Y, np.zeros(n), lam)[0]["primal"])
    gap_tol = 1e-7 * P0
    kw = dict(lr=1.0, nesterov=True, tol=0.0)
    # by hand: gap_every passes at a time, the standalone certificate after each - the first check at which it is small enough
    run = NativeRun(prob, np.zeros(n), dict(_BASE, max_iter=3000))
    checks = 0
    while True:
        run.advance(16)   # gap_every, as passed below
        checks += 1
        probe = prob.duality_gap(run.solver.get_x())
        assert np.array_equal(_bits(run.duality_gap().gap), _bits(probe.gap)), "the live solver's certificate is the standalone one"
        if probe.gap <= gap_tol or checks > 200:
            break
    x_probe, nit_probe = run.solver.get_x(), run.nit_seen
    run.solver.close()
    assert 1 < checks <= 200, "the first check must not stop the solve, and one must"
    res = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=3000, gap_tol=gap_tol, gap_every=16, **kw)
    assert res.success and res.status == 1 and res.message == "Duality gap reached gap_tol" and res.nit < 3000
    assert (res.dual_gap_checks, res.nit) == (checks, nit_probe) and np.array_equal(_bits(res.x), _bits(x_probe))
    assert 0 <= res.dual_gap <= gap_tol and res.dual_gap == prob.duality_gap(res.x).gap
    plain = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=res.nit, **kw)
    assert plain.nit == res.nit and np.array_equal(plain.x, res.x) and plain.fun == res.fun, "the keyword does not alter the iterates"
    vals, bounds, extra = MC.gap_longdouble(A, Y, res.x, lam)
    print(f"{storage}: stopped at nit {res.nit}, gap {float(res.dual_gap):.3g} <= {gap_tol:.3g}; long double {float(vals['gap']):.3g}")
    assert float(vals["gap"]) <= gap_tol * (1 + 1e-6) and float(extra["gap_pd"]) >= -1e-15 * P0, "P - D >= 0"
    for bad in ("remainder", "resolved"):
        with pytest.raises(ValueError, match="acceptance="):
            solve(*prob.callbacks(), np.zeros(n), acceptance=bad, max_iter=3)


# ---- (5) the public interface --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", FORMS)
def test_lam_max_returns_zero_and_just_below_it_does_not(storage):
    from zfista_amd import minimize_proximal_gradient as solve

    case = MC.GAP_CASE
    A, Y, _, _, _, _ = case.data()
    K, n = case.K, case.n
    for w, pf in ((None, None), (MC.make_weights(case.m, 5, "real"), None), (None, MC.make_factors(n, K, 5, "pos"))):
        prob0 = _make(storage, A, Y, 1.0, sample_weight=w, penalty_factor=pf)
        lmax = float(prob0.lam_max())
        wv = np.ones(case.m) if w is None else w
        ref = np.abs(A.T @ (wv[:, None] * (1.0 / K - Y))) / (1.0 if pf is None else pf)
        assert abs(lmax - float(ref.max())) <= 1e-12 * lmax
        at = _quiet(solve, *prob0.with_lam(lmax * (1 + 1e-9)).callbacks(), np.zeros(n * K), lr=1.0, tol=0.0, max_iter=30, nesterov=True)
        assert not at.x.any(), "x = 0 is returned at lam_max"
        below = _quiet(solve, *prob0.with_lam(0.99 * lmax).callbacks(), np.zeros(n * K), lr=1.0, tol=0.0, max_iter=30, nesterov=True)
        assert below.x.any(), "x = 0 is left at 0.99 lam_max"


@pytest.mark.parametrize("storage", FORMS)
def test_two_classes_are_logistic_regression_on_the_difference_of_columns(storage):
    """Softmax with K = 2 is the logistic model of beta = x_1 - x_0, and min |x_0| + |x_1| over x_1 - x_0 = beta is |beta|: the two
    problems have the same optimal value and the same fitted probabilities.  f at matched points to 1e-12; the fitted probabilities of
    two gap-certified solves within sqrt(gap / 2) each: F(x) - F* >= the Bregman divergence of f at the optimal margins, which is
    sum_i KL(p*_i || p_i) >= 2 sum_i (p_i - p*_i)^2 (Pinsker), so |p_i - p*_i| <= sqrt(gap / 2) for either solve (scale = 1)."""
    from zfista_amd import minimize_proximal_gradient as solve
    from zfista_amd import problems as Z

    m, n = 200, 30
    A, Y, _ = MC.make(m, n, 2, 77)
    lab = Y[:, 1].astype(int)
    b = 2.0 * lab - 1.0
    As = sp.csr_matrix(A) if storage == "csr" else A
    logi = (Z.SparseLogisticL1 if storage == "csr" else Z.LogisticL1)(As, b, 1.0)
    mn = logi.with_classes(lab)
    assert type(mn) is (Z.SparseMultinomialL1 if storage == "csr" else Z.MultinomialL1)
    rng = np.random.default_rng(3)
    for _ in range(3):
        beta = rng.standard_normal(n)
        X = np.stack([np.zeros(n), beta], axis=1)
        fm, fl = float(mn.f(X)), float(logi.f(beta))
        assert abs(fm - fl) <= 1e-12 * abs(fl)
        shift = rng.standard_normal(n)
        assert abs(float(mn.f(X + shift[:, None])) - fl) <= 1e-12 * abs(fl) * (1 + np.abs(shift).max()), "a common shift of both columns changes nothing"
    lam = 0.1 * float(logi.lam_max())
    assert abs(float(mn.lam_max()) - float(logi.lam_max()) / 1.0) <= 1e-12 * float(logi.lam_max()), "|A^T (1/2 - y)|_inf on both sides"
    gap_tol = 1e-9 * m * np.log(2.0)
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=20000, gap_tol=gap_tol)
    rl = _quiet(solve, *logi.with_lam(lam).callbacks(), np.zeros(n), **kw)
    rm = _quiet(solve, *mn.with_lam(lam).callbacks(), np.zeros(2 * n), **kw)
    assert rl.success and rm.success and rl.dual_gap <= gap_tol and rm.dual_gap <= gap_tol
    pl = 1.0 / (1.0 + np.exp(-(A @ rl.x)))
    pm = mn.predict_proba(rm.x)
    assert pm.shape == (m, 2) and np.allclose(pm.sum(axis=1), 1.0, atol=1e-15)
    assert np.array_equal(pm, mn.predict_proba(rm.x, A=As)), "the problem's own matrix, copied from the device"
    bound = np.sqrt(rl.dual_gap / 2) + np.sqrt(rm.dual_gap / 2)
    print(f"{storage}: max |p_multinomial - p_logistic| {np.abs(pm[:, 1] - pl).max():.3g} <= {bound:.3g}; nit {rm.nit} / {rl.nit}")
    assert np.abs(pm[:, 1] - pl).max() <= bound
    assert abs(float(rm.fun) - float(rl.fun)) <= 2 * gap_tol, "the same optimal value"
    assert np.array_equal(mn.classes, [0, 1]) and mn.coef(rm.x).shape == (n, 2)


@pytest.mark.parametrize("storage", FORMS)
def test_l1_path_equals_the_same_solves_made_problem_by_problem(storage):
    from zfista_amd import minimize_proximal_gradient as solve
    from zfista_amd.path import l1_path

    case = MC.GAP_CASE
    A, Y, _, _, _, _ = case.data()
    n = case.n * case.K
    w = MC.make_weights(case.m, 9, "real")
    prob = _make(storage, A, Y, 1.0, sample_weight=w)
    lmax = float(prob.lam_max())
    lams = [lmax * f for f in (1.0000001, 0.5, 0.25, 0.15)]
    gap_tol = 1e-6 * float(MC.gap_longdouble(A, Y, np.zeros(n), lams[-1], w=w)[0]["primal"])
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=4000)
    pth = _quiet(l1_path, prob, lams, gap_tol=gap_tol, **kw)
    assert not pth[0].x.any() and len(pth) == 4
    x = np.zeros(n)
    for lam_k, r in zip(lams, pth):
        sib = prob.with_lam(lam_k)
        assert sib.b.data_ptr() == prob.b.data_ptr()
        one = _quiet(solve, *sib.callbacks(), x, gap_tol=gap_tol, **kw)
        assert r.success and r.dual_gap <= gap_tol and r["lam"] == lam_k
        assert one.nit == r.nit and np.array_equal(one.x, r.x) and one.dual_gap == r.dual_gap
        assert float(MC.gap_longdouble(A, Y, r.x, lam_k, w=w)[0]["gap"]) <= gap_tol * (1 + 1e-6)
        x = r.x
    assert np.count_nonzero(pth[-1].x) > np.count_nonzero(pth[1].x) > 0
    with pytest.raises(ValueError, match="several responses"):
        l1_path(prob.with_sample_weight(None), lams, screen=True)


def test_with_classes_shares_the_resident_matrix_and_labels_expand():
    from zfista_amd import problems as Z

    A, Y, lam = MC.make(60, 20, 4, 21)
    lab = Y.argmax(axis=1)
    b = np.where(lab == 0, 1.0, -1.0)
    dense = Z.LogisticL1(A, b, lam)
    mn = dense.with_classes(lab, sample_weight=np.ones(60))
    assert mn.A.data_ptr() == dense.A.data_ptr() and mn.n_responses == 4 and np.array_equal(mn.classes, np.arange(4))
    assert (mn.lam, mn.scale) == (dense.lam, dense.scale) and mn.sample_weight.shape == (60,)
    own = Z.MultinomialL1(A, Y, lam)
    x = np.random.default_rng(0).standard_normal(80)
    assert own.f(x) == dense.with_classes(lab).f(x) == dense.with_classes(Y).f(x), "labels expand to the one-hot rows"
    five = Z.MultinomialL1(A, lab, lam, n_classes=5)
    assert five.n_responses == 5 and five.n_features == 100 and not five.b.cpu().numpy().reshape(60, 5)[:, 4].any()
    sparse = Z.SparseLogisticL1(sp.csr_matrix(A), b, lam)
    smn = sparse.with_classes(lab)
    assert smn._spmat is sparse._spmat and smn.f(x) == pytest.approx(own.f(x), rel=1e-13)
    for prob in (own, smn):
        with pytest.raises(ValueError, match="sample_weight must be a vector of 60"):
            prob.with_sample_weight(np.ones((60, 4)))
        assert prob.with_sample_weight(np.ones(60)).sample_weight.shape == (60,)
        assert prob.with_penalty_factor(np.ones(20)).penalty_factor.shape == (80,)
        assert prob.with_penalty_factor(np.ones((20, 4))).b.data_ptr() == prob.b.data_ptr()


def test_two_solves_on_two_streams_agree_with_the_solves_alone():
    from zfista_amd import minimize_proximal_gradient as solve
    from zfista_amd.replicas import solve_on_streams

    case = MC.CASES[4]
    prob = _problem(case)
    kws = [dict(lr=1.0, tol=0.0, max_iter=40, nesterov=True), dict(lr=0.5, tol=0.0, max_iter=40, nesterov=False)]
    alone = [_quiet(solve, *prob.callbacks(), case.x0(), **kw) for kw in kws]
    two = solve_on_streams([(prob, case.x0(), kw) for kw in kws], streams=2)
    for a, b in zip(alone, two):
        assert a.nit == b.nit and np.array_equal(_bits(a.x), _bits(b.x)) and a.fun == b.fun


# What solvers that never call zf_solver_set_multinomial launched, planned and computed with the parent commit's library: the values
# tests/test_gpu_poisson.py holds for the plain classes (its PARENT table, asserted there against every later library), and for the
# K-response classes the solver's own launch counts and plan before and after multinomial solves on the same device.
PARENT = {
    "ls_small": [[0, 0], [1, 1, 64, 8], "140644d478064c34d9df6bf34441bbf3ed3161eee13154280815f0feb95de89c"],
    "ls_general": [[0, 0], [3, 2, 60, 10], "cdcc96d756b64be74285e8a105cc62bbf0ee1545c5a76059df1a6a25c1ba22ad"],
    "logistic": [[0, 0], [2, 2, 64, 8], "36ad5e3411402a8cdb0d1ac8c00ecf505878ea31b151144902baaf8e67c690f5"],
    "sparse": [[0, 0], [5, 16, 4, 0], "be38efb83e1d4dedd6671d89c8eeab69984bb8d45afbb4e87989a9ee7145f779"],
}


def _default_solves():
    import sparse_cases as S
    from oracle import problems_ref as P
    from zfista_amd import problems as Z

    A, b, lam = P.make_plasso(512, 1024, seed=0)
    A2, b2, lam2 = P.make_plasso(600, 3000, seed=1)
    Sm, bs, lams = S.make_sparse(*S.SMALL[0])
    Am, Bm, lamm = MC.make(33, 130, 5, 1)
    return {
        "ls_small": lambda: Z.LeastSquaresL1(A, b, lam),
        "ls_general": lambda: Z.LeastSquaresL1(A2, b2, lam2),
        "logistic": lambda: Z.LogisticL1(A, np.where(b > 0, 1.0, -1.0), lam),
        "sparse": lambda: Z.SparseLeastSquaresL1(Sm, bs, lams),
        "mr_logistic": lambda: Z.MultiResponseLogisticL1(Am, 2.0 * Bm - 1.0, lamm),
        "mr_sparse_ls": lambda: Z.SparseMultiResponseLeastSquaresL1(sp.csr_matrix(Am), Bm, lamm),
    }


@pytest.fixture
def recorded(monkeypatch):
    """minimize_proximal_gradient on the native path; returns (result, ls_plan, launch counts) - the recording of tests/test_gpu_poisson.py."""
    from zfista_amd import minimize_proximal_gradient, proximal_gradient as pg

    seen = []

    class _Recorded(pg.NativeRun):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.plan = self.solver.ls_plan()
            seen.append(self)

        def collect(self):
            rows = super().collect()
            self.counts = self.solver.launch_counts()
            return rows

    monkeypatch.setattr(pg, "NativeRun", _Recorded)

    def run(prob, x0, **kw):
        del seen[:]
        res = _quiet(minimize_proximal_gradient, *prob.callbacks(), x0, **kw)
        assert len(seen) == 1, "the solve did not run on the native path"
        return res, seen[0].plan, seen[0].counts

    return run


def _fingerprint(run, make):
    prob = make()
    res, plan, counts = run(prob, np.zeros(prob.n_features), lr=1, tol=0.0, max_iter=40, nesterov=True)
    assert res.nit == 40
    return [list(map(int, counts)), list(map(int, plan)), hashlib.sha256(np.ascontiguousarray(res.x).tobytes()).hexdigest()]


@pytest.mark.parametrize("name", ["ls_small", "ls_general", "logistic", "sparse", "mr_logistic", "mr_sparse_ls"])
def test_solvers_that_never_asked_launch_what_the_parent_library_launched(name, recorded):
    from zfista_amd import minimize_proximal_gradient as solve

    make = _default_solves()[name]
    got = _fingerprint(recorded, make)
    print(name, json.dumps(got))
    for storage in FORMS:
        case = MC.ALL_K[3]
        _quiet(solve, *_problem(case, storage).callbacks(), case.x0(), **case.opts)
    assert _fingerprint(recorded, make) == got, "multinomial solves in between do not disturb the other classes"
    if name in PARENT:
        assert got[:2] == PARENT[name][:2], "launch counts and plan of the parent library"
        assert got[2] == PARENT[name][2], "the bits of x_40 of the parent library"


def test_refusals_at_the_c_level_in_both_call_orders():
    import torch

    from oracle import problems_ref as P
    from zfista_amd import _lib
    from zfista_amd import problems as Z
    from zfista_amd.engine import DeviceSolver

    A, Y, lam = MC.make(64, 128, 4, 3)
    options = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=3, max_backtrack_iter=10)
    plain = Z.MultiResponseLeastSquaresL1(A, Y, lam)   # (the least-squares kind with 4 responses: the setter is ours to call)
    fields, keep = plain._descriptor()
    K = fields.pop("responses")
    w = torch.ones(64 * 4, dtype=torch.float64, device="cuda")
    pf = torch.ones(128 * 4, dtype=torch.float64, device="cuda")
    # the reverse order: the multinomial setter before the responses
    s = DeviceSolver(fields, options, keepalive=keep)
    lib = s.lib
    assert lib.zf_solver_set_multinomial(s.handle) == -2 and b"zf_solver_set_responses" in lib.zf_last_error() and b"BEFORE" in lib.zf_last_error()
    assert lib.zf_solver_set_responses(s.handle, K) == 0 and lib.zf_solver_set_multinomial(s.handle) == 0
    assert lib.zf_solver_set_multinomial(s.handle) == -2 and b"already" in lib.zf_last_error(), "a second call"
    assert lib.zf_solver_set_huber(s.handle, 0.5) == -2 and lib.zf_solver_set_poisson(s.handle) == -2 and b"multinomial" in lib.zf_last_error()
    # composes with l2 and the weights in any order; the factors not with l2 (as everywhere)
    assert lib.zf_solver_set_l2(s.handle, 0.25) == 0 and lib.zf_solver_set_row_weights(s.handle, w.data_ptr()) == 0
    x0 = torch.zeros(128 * 4, dtype=torch.float64, device="cuda")
    s.init(x0.data_ptr())
    assert lib.zf_solver_set_multinomial(s.handle) == -3 and b"before" in lib.zf_last_error()   # ZF_ERR_STATE
    s.close()
    s = DeviceSolver(fields, options, keepalive=keep)
    assert lib.zf_solver_set_row_weights(s.handle, w.data_ptr()) == 0 and lib.zf_solver_set_penalty_factors(s.handle, pf.data_ptr()) == 0
    assert lib.zf_solver_set_responses(s.handle, K) == 0 and lib.zf_solver_set_multinomial(s.handle) == 0
    s.close()
    for first, word in ((lambda h: lib.zf_solver_set_huber(h, 0.5), b"responses"), (lambda h: lib.zf_solver_set_poisson(h), b"responses")):
        s = DeviceSolver(fields, options, keepalive=keep)
        assert first(s.handle) == 0
        assert lib.zf_solver_set_multinomial(s.handle) == -2   # (Huber / Poisson: refused whichever check comes first)
        s.close()
    # the acceptance modes, other kinds, a sparse solver from the plain creator
    s = DeviceSolver(fields, dict(options, accept_mode=_lib.ZF_ACCEPT_REMAINDER), keepalive=keep)
    assert lib.zf_solver_set_multinomial(s.handle) == -2 and b"ZF_ACCEPT_REMAINDER" in lib.zf_last_error()
    s.close()
    with pytest.raises(_lib.ZfError, match="accept_mode"):   # (ZF_ACCEPT_RESOLVED never reaches the setter: the kind refuses it at creation)
        DeviceSolver(fields, dict(options, accept_mode=_lib.ZF_ACCEPT_RESOLVED), keepalive=keep)
    d, c, lam_d = P.make_pdiag(1000, seed=1)
    for prob in (Z.DiagQuadL1(d, c, lam_d), Z.MultiResponseLogisticL1(A, 2 * Y - 1, lam)):
        f2, k2 = prob._descriptor()
        s = DeviceSolver(f2, options, keepalive=k2)
        assert lib.zf_solver_set_multinomial(s.handle) == -2 and b"only for" in lib.zf_last_error()
        s.close()
    f3, k3 = Z.SparseLeastSquaresL1(sp.csr_matrix(A), Y[:, 0].copy(), lam)._descriptor()
    s = DeviceSolver(f3, options, keepalive=k3)
    assert lib.zf_solver_set_multinomial(s.handle) == -2 and b"zf_solver_create_sparse_responses" in lib.zf_last_error()
    s.close()
    f4, k4 = Z.SparseMultiResponseLeastSquaresL1(sp.csr_matrix(A), Y, lam)._descriptor()
    s = DeviceSolver(f4, options, keepalive=k4)
    assert lib.zf_solver_set_multinomial(s.handle) == 0, "a sparse solver from zf_solver_create_sparse_responses has its responses"
    assert lib.zf_solver_set_multinomial(s.handle) == -2 and b"already" in lib.zf_last_error()
    s.close()
    # the evaluation entries with K = 1 on live device pointers, and the Python refusals with a device
    prob = Z.MultinomialL1(A, Y, lam)
    d1 = prob._eval_desc()
    d1.K = 1
    f = C.c_double(-7.0)
    x = np.zeros(128 * 4)
    assert lib.zf_margins_eval(C.byref(d1), C.sizeof(d1), C.c_void_p(_lib.ptr(x)), C.byref(f), None) == -2 and f.value == -7.0
    for call in (prob.column_norms, lambda: prob.screen(x), lambda: prob.restrict(np.arange(5))):
        with pytest.raises(ValueError, match="several responses"):
            call()
    with pytest.raises(ValueError, match="bounds are set"):
        Z.MultinomialL1(A, Y, lam, bounds=(-1.0, 1.0)).duality_gap(x)
    with pytest.raises(ValueError, match="unpenalised column"):
        Z.MultinomialL1(A, Y, lam, penalty_factor=np.r_[0.0, np.ones(127)]).duality_gap(x)
