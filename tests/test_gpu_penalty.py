"""GPU: per-column penalty factors on the eight margins classes - g(x) = lam sum_j p_j |x_j| (zf_trial_pf_kernel, zf_eval_pf_kernel,
zf_gap_pf_scale_kernel; csrc/zf_kernels_step.h, zf_kernels_gap.h).

(1) Element bits.  A the sparse identity and scale = 1/2 make the gradient y - b exactly, so every iterate of a short solve is
    NumPy's expression bit for bit (the oracle on penalty_cases.PenaltyRef): with and without momentum (the third iterate has
    beta != 0), with and without an active box, at every n where the kernel changes path; p = 0 entries come through unthresholded.
    A NaN iterate ends a solve before its x+ can be read, so NaN and +-inf at p = 0 are checked on the host-pointer restatement
    zf_host_prox_pf_box (the same expression), with zf_host_pf_g inside its bound.
(2) p = 1 is the plain class bit for bit: iterates, allfuns, lr and trial traces of 80 FISTA iterations, the eight certificate
    outputs; the unfactored solve before and after launches the same.
(3) Parity against G19 and against the oracle on PenaltyRef: all four losses, both storages, with and without row weights.
(4) The certificate with positive factors inside its derived bounds, the live solver's, gap_tol, lam_max.
(5) The factored problem on A against the plain problem on A diag(1 / p).
(6) Intercepts.  (7) Snapshots, streams, l1_cv, the refusals of the C level.

The tolerance of (5).  Both solves stop at a certified gap <= G = 1e-10.  phi (the loss as a function of the margins) has an
L-Lipschitz gradient (squared loss: L = 2 scale), so for the common optimum z* of the margins, P(x) - P* >= |grad phi(z) - grad
phi(z*)|^2 / (2 L): the two margin vectors differ by at most (sqrt(2 L g1) + sqrt(2 L g2)) / (2 scale) in the 2-norm - no strong
convexity of f is used.  p o x - x' lives on the joint support S of the two solutions, so it is bounded by the same number over
sigma_min(A'_S), A' = A diag(1 / p), computed by the test (the whole 1000 x 257 matrix has dependent columns); the rounding of
A / p and x p (relative u per factor) adds 4 u |A'|_F |x'|.

Measured on an MI355X when these tests were written (figures, not thresholds): iterates within 8.0e-15 of the oracle over all (3)
solves; the worst certificate output at 0.0054 of its derived bound; (5): the two optimal values equal to the last digit printed
(140.335966373), |A'(p o x - x')| = 7.0e-11 against a bound of 2.5e-5, |p o x - x'| = 3.8e-11; (6): lam_max with an intercept
2.5e-12 from the long-double value, 1.3e-9 allowed, and |grad f(x)_0| <= 9.3e-9 on the Poisson path where 6.1e-5 to 1.4e-4 is
allowed."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import penalty_cases as PF
import poisson_cases as PC
import sparse_cases as S
import weight_cases as W
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-10
U = PF.U
_id = lambda c: f"{c[0]}x{c[1]}"
KW80 = dict(lr=1, tol=0.0, max_iter=80, nesterov=True, return_all=True)


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _gap_bits(gp):
    return np.array([getattr(gp, k) for k in PF.KEYS8]).view(np.uint64)


def _cls(loss, storage):
    from zfista_amd import problems as Z

    return {("square", "csr"): Z.SparseLeastSquaresL1, ("square", "dense"): Z.LeastSquaresL1,
            ("logistic", "csr"): Z.SparseLogisticL1, ("logistic", "dense"): Z.LogisticL1,
            ("huber", "csr"): Z.SparseHuberL1, ("huber", "dense"): Z.HuberL1,
            ("poisson", "csr"): Z.SparsePoissonL1, ("poisson", "dense"): Z.PoissonL1}[loss, storage]


def _make(loss, storage, A, b, lam, delta=0.0, p=None, w=None, bounds=None):
    """The class of (loss, storage) at penalty_cases.SCALE; factors and weights through the sibling form all eight share."""
    M = PF.matrix(A, storage) if sp.issparse(A) else A
    cls, scale = _cls(loss, storage), PF.SCALE[loss]
    prob = cls(M, b, lam, delta, scale=scale, bounds=bounds) if loss == "huber" else cls(M, b, lam, scale=scale, bounds=bounds)
    if w is not None:
        prob = prob.with_sample_weight(w)
    return prob if p is None else prob.with_penalty_factor(p)


@functools.lru_cache(maxsize=None)
def _data(case, loss):
    return PF.make_problem(case, loss)


@functools.lru_cache(maxsize=None)
def _factors(case, kind):
    p = PF.make_factors(case[1], case[3], kind)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _weights(case, loss):
    w = PC.case_weights(case) if loss == "poisson" else W.make_weights(case[0], case[3], "real")
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _oracle(case, loss, weighted):
    """80 FISTA iterations of the oracle solver on PenaltyRef with the ``real`` factors - computed once, shared, left unchanged."""
    from oracle import cpu_ref

    A, b, lam, delta = _data(case, loss)
    ref = PF.PenaltyRef(A, b, lam, _factors(case, "real"), loss, delta, w=_weights(case, loss) if weighted else None)
    return _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), np.zeros(A.shape[1]), **KW80)


@pytest.fixture
def solve(monkeypatch):
    """minimize_proximal_gradient on the native path; returns (result, trace rows of every accepted iteration, ls_plan, counts)."""
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
            self.counts = self.solver.launch_counts()
            return rows

    monkeypatch.setattr(pg, "NativeRun", _Recorded)

    def run(prob, x0, **kw):
        del seen[:]
        res = _quiet(minimize_proximal_gradient, *prob.callbacks(), x0, **kw)
        assert len(seen) == 1, "the solve did not run on the native path"
        return res, np.concatenate(seen[0].rows), seen[0].plan, seen[0].counts

    return run


def _check_solve(res, rows, exp, what=""):
    """The suite's criteria: equal nit, status and trial / lr sequences; iterates, allfuns, allerrs to 1e-10."""
    from zfista_amd import _lib

    assert res.nit == exp.nit and bool(res.success) == bool(exp.success)
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), np.asarray(exp.alltrials, np.int64))
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float))
    assert len(res.allvecs) == len(exp.allvecs) == exp.nit + 1
    worst = max(rel_err(a, e) for a, e in zip(res.allvecs[1:], exp.allvecs[1:]))
    print(f"{what}: nit {res.nit}, trials {int(rows[:, _lib.TR_TRIALS].sum())}: iterates within {worst:.3g}")
    assert worst <= TOL and rel_err(res.x, exp.x) <= TOL
    np.testing.assert_allclose(res.allfuns, exp.allfuns, rtol=TOL, atol=0)
    np.testing.assert_allclose(res.allerrs, exp.allerrs, rtol=1e-8, atol=1e-14)


# ---- (1) element bits ----------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 255, 257, 1023, 1024, 1025, 2049, 4099]


@pytest.mark.parametrize("boxed", [False, True], ids=["free", "box"])
@pytest.mark.parametrize("nesterov", [False, True], ids=["ista", "fista"])
@pytest.mark.parametrize("n", SIZES)
def test_step_kernel_element_bits(n, nesterov, boxed, solve):
    from oracle import cpu_ref
    from zfista_amd import _lib
    from zfista_amd.problems import SparseLeastSquaresL1

    rng = np.random.default_rng(100 + n)
    x0 = 0.5 * rng.standard_normal(n)
    b = rng.standard_normal(n)
    p = PF.make_factors(n, n, "real")
    if n >= 3:
        p[1], p[n - 1] = 0.0, 0.0   # an unpenalised coordinate in the first unit and at the very end (the scalar tail of an odd n)
    lam, bounds = 0.4, ((-0.3, 0.6) if boxed else None)
    kw = dict(lr=0.5, tol=0.0, max_iter=3, nesterov=nesterov, return_all=True)
    prob = SparseLeastSquaresL1(sp.identity(n, format="csr"), b, lam, scale=0.5, bounds=bounds, penalty_factor=p)
    if boxed:
        x0 = np.clip(x0, *bounds)
    ref = PF.PenaltyRef(sp.identity(n, format="csr"), b, lam, p, "square", bounds=bounds)
    exp = _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), x0, **kw)
    res, rows, plan, _ = solve(prob, x0, **kw)
    assert res.nit == exp.nit == 3 and rows[:, _lib.TR_TRIALS].tolist() == [float(t) for t in exp.alltrials]
    for k in range(1, 4):
        got, want = np.asarray(res.allvecs[k]), np.asarray(exp.allvecs[k])
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, (k, bad[:8], got[bad[:8]], want[bad[:8]])
    # the first iterate by hand: y = x0, v = x0 - lr (x0 - b); p = 0 carries v through, p > 0 thresholds at (lam lr) p_j
    v = x0 - 0.5 * (x0 - b)
    x1 = np.asarray(res.allvecs[1])
    free = p == 0
    want0 = v[free] if not boxed else np.clip(v[free], *bounds)
    assert np.array_equal(_bits(x1[free]), _bits(want0)), "an unpenalised coordinate is not thresholded"
    if n >= 255:
        assert np.count_nonzero(x1 == 0.0) >= 5 and np.count_nonzero(x1) >= 5, "the threshold must be active and inactive"
        if boxed:
            assert np.count_nonzero(x1 == bounds[0]) >= 3 and np.count_nonzero(x1 == bounds[1]) >= 3, "the box must be active"
    # F of the trace is f + lam sum p |x| (the pack scale stays lam)
    F1 = float(PF.primal_longdouble(sp.identity(n, format="csr"), b, p, x1, lam, "square", scale=0.5))
    assert abs(float(res.allfuns[1]) - F1) <= 1e-12 * max(abs(F1), 1e-300) + 1e-300


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_host_restatements_equal_numpy_bits(n):
    from zfista_amd import _lib
    from zfista_amd.problems import SparseLeastSquaresL1

    lib = _lib.require_gpu()
    rng = np.random.default_rng(3 + n)
    v = 0.05 * rng.standard_normal(n)
    p = PF.make_factors(n, n, "real")
    special = [0.0, -0.0, np.nan, np.inf, -np.inf, 1e-320, -1e-320, 1e300, -1e300, np.nan, np.inf, -0.0]
    pspec = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0, 0.0, 1.0, 1.5, 0.5, 3.0]
    k = min(n, len(special))
    v[:k], p[:k] = special[:k], pspec[:k]
    for t in (0.37, 2.0 ** -20, 0.0):
        for bounds in (None, (-0.02, 0.03)):
            with np.errstate(invalid="ignore"):
                want = PF.prox_pf(v, t, p, bounds)
            got = np.empty_like(v)
            lo, hi = (-np.inf, np.inf) if bounds is None else bounds
            assert lib.zf_host_prox_pf_box(C.c_void_p(_lib.ptr(got)), C.c_void_p(_lib.ptr(v)), C.c_void_p(_lib.ptr(p)), t, lo, hi, n) == 0
            same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
            assert same.all() and np.array_equal(np.isnan(got), np.isnan(want)), (t, bounds, np.flatnonzero(~same)[:8])
    if n >= 12:   # the class method is that call: p = 0 keeps NaN and +-inf
        prob = SparseLeastSquaresL1(sp.identity(n, format="csr"), np.zeros(n), 0.37, penalty_factor=p)
        out = prob.prox_wsum_g(1.0, v)
        assert np.isnan(out[2]) and out[3] == np.inf and out[4] == -np.inf and out[5] == 1e-320 and out[7] == 1e300
        assert out[0] == 0.0 and not np.signbit(out[0])
    # g: n fused multiply-adds in some order: (n + 2) u relative to the sum (every term >= 0), one product with lam
    x = 0.05 * rng.standard_normal(n)
    pf = np.where(np.isfinite(p), p, 1.0)
    s = C.c_double(-1.0)
    assert lib.zf_host_pf_g(C.c_void_p(_lib.ptr(x)), C.c_void_p(_lib.ptr(pf)), n, 0.3, C.byref(s)) == 0
    exact = np.longdouble(0.3) * np.sum(pf.astype(np.longdouble) * np.abs(x.astype(np.longdouble)))
    assert abs(float(np.longdouble(s.value) - exact)) <= (n + 3) * U * float(exact)


# ---- (2) p = 1 ---------------------------------------------------------------------------------------------------------------------------
ONES = [("logistic", "dense", PF.GPU_SMALL[0]), ("huber", "csr", PF.GPU_SMALL[1]), ("poisson", "dense", PF.GPU_SMALL[1]),
        ("square", "csr", PF.GPU_SMALL[2]), ("square", "dense", PF.GPU_SMALL[1]), ("poisson", "csr", PF.GPU_SMALL[0])]


@pytest.mark.parametrize("loss,storage,case", ONES, ids=[f"{l}-{s}-{_id(c)}" for l, s, c in ONES])
def test_unit_factors_are_the_plain_class_bit_for_bit(loss, storage, case, solve, monkeypatch):
    from zfista_amd import _lib

    if (loss, storage) == ("square", "dense"):
        monkeypatch.setenv("ZF_LS_SMALL", "0")   # (the plain class on the general path: the fused small-matrix kernels sum otherwise)
    A, b, lam, delta = _data(case, loss)
    n = A.shape[1]
    plain = _make(loss, storage, A, b, lam, delta)
    ones = plain.with_penalty_factor(np.ones(n))
    assert (ones._spmat is plain._spmat) if storage == "csr" else (ones.A.data_ptr() == plain.A.data_ptr()), "the sibling shares the matrix"
    r0, rows0, plan0, counts0 = solve(plain, np.zeros(n), **KW80)
    r1, rows1, plan1, counts1 = solve(ones, np.zeros(n), **KW80)
    assert r1.nit == r0.nit == 80 and plan1[0] != 1 and rows1[:, _lib.TR_TRIALS].sum() > 80
    assert np.array_equal(rows1, rows0), "trial, lr and F traces"
    assert np.array_equal(_bits(r1.x), _bits(r0.x)) and np.array_equal(_bits(r1.allfuns), _bits(r0.allfuns))
    assert np.array_equal(_bits(np.asarray(r1.allvecs)), _bits(np.asarray(r0.allvecs)))
    assert np.array_equal(_bits(r1.allerrs), _bits(r0.allerrs))
    for v in (np.zeros(n), np.asarray(r0.x)):
        assert np.array_equal(_gap_bits(ones.duality_gap(v)), _gap_bits(plain.duality_gap(v)))
    assert _bits(ones.lam_max()) == _bits(plain.lam_max())
    # a warm start: g(x0) of the init kernel, x0 != 0
    w0, _, _, _ = solve(plain, np.asarray(r0.allvecs[40]), **dict(KW80, max_iter=5))
    w1, _, _, _ = solve(ones, np.asarray(r0.allvecs[40]), **dict(KW80, max_iter=5))
    assert np.array_equal(_bits(w1.allfuns), _bits(w0.allfuns)) and np.array_equal(_bits(w1.x), _bits(w0.x))
    # the unfactored solve afterwards launches what it launched before
    r2, rows2, plan2, counts2 = solve(plain, np.zeros(n), **KW80)
    assert plan2 == plan0 and counts2 == counts0 and np.array_equal(rows2, rows0) and np.array_equal(_bits(r2.x), _bits(r0.x))
    assert counts1 == counts0, "a factored trial is one launch where the plain trial is one"


def test_a_small_dense_matrix_keeps_its_fused_path_and_its_factored_sibling_leaves_it(solve):
    from oracle import problems_ref as P
    from zfista_amd.problems import LeastSquaresL1

    A, b, lam = P.make_plasso(512, 1024, seed=0)
    kw = dict(lr=1, tol=0.0, max_iter=40, nesterov=True)
    plain = LeastSquaresL1(A, b, lam)
    r0, rows0, plan0, counts0 = solve(plain, np.zeros(1024), **kw)
    assert plan0[:2] == (1, 1), "the fused small-matrix path"
    r1, _, plan1, _ = solve(plain.with_penalty_factor(np.ones(1024)), np.zeros(1024), **kw)
    assert plan1[:2] == (2, 2) and r1.nit == 40 and rel_err(r1.x, r0.x) <= 1e-12
    again = plain.with_penalty_factor(np.ones(1024)).with_penalty_factor(None)
    r2, rows2, plan2, counts2 = solve(again, np.zeros(1024), **kw)
    assert plan2 == plan0 and counts2 == counts0 and np.array_equal(rows2, rows0) and np.array_equal(r2.x, r0.x)


# ---- (3) parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,ci,storage,tag", PF.GOLDEN_SOLVES)
def test_solve_vs_reference_fixture(golden, loss, ci, storage, tag, solve):
    from zfista_amd import _lib

    G = golden("g19_penalty.npz")
    case = S.SMALL[ci]
    A, b, lam, delta = _data(case, loss)
    assert lam == float(G(f"penalty.{loss}.c{ci}.lam"))
    prob = _make(loss, storage, A, b, lam, delta, p=_factors(case, "real"))
    res, rows, _, _ = solve(prob, np.zeros(A.shape[1]), **PF.GOLDEN_KW, **PF.GOLDEN_VARIANTS[tag])
    pre = PF.golden_prefix(loss, ci, storage, tag)
    assert res.nit == int(G(f"{pre}.nit")) == 80
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), G(f"{pre}.alltrials")), "decisions"
    assert np.array_equal(rows[:, _lib.TR_LR], G(f"{pre}.alllrs"))
    assert rel_err(res.x, G(f"{pre}.x")) <= TOL and abs(np.linalg.norm(res.x) - float(G(f"{pre}.xnorm"))) <= TOL * float(G(f"{pre}.xnorm"))
    got = np.stack([np.asarray(res.allvecs[k])[::PF.GOLDEN_STRIDE] for k in G(f"{pre}.kept")])
    assert max(rel_err(a, e) for a, e in zip(got[1:], G(f"{pre}.vecs")[1:])) <= TOL
    np.testing.assert_allclose(res.allfuns, G(f"{pre}.allfuns"), rtol=TOL, atol=0)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("storage", PF.FORMS)
@pytest.mark.parametrize("loss", PF.LOSSES)
@pytest.mark.parametrize("case", PF.GPU_SMALL, ids=_id)
def test_solve_vs_oracle(case, loss, storage, weighted, solve):
    A, b, lam, delta = _data(case, loss)
    p = _factors(case, "real")
    prob = _make(loss, storage, A, b, lam, delta, p=p, w=_weights(case, loss) if weighted else None)
    res, rows, plan, _ = solve(prob, np.zeros(A.shape[1]), **KW80)
    assert plan[0] != 1
    _check_solve(res, rows, _oracle(case, loss, weighted), f"{_id(case)} {loss} {storage} {'w' if weighted else '-'}")
    assert np.count_nonzero(np.asarray(res.x)[p == 0]) > 0, "unpenalised columns move"


def test_the_constructor_keyword_is_the_sibling(solve):
    case = PF.GPU_SMALL[1]
    p = _factors(case, "real")
    for loss, storage in (("square", "dense"), ("huber", "csr"), ("poisson", "csr")):
        A, b, lam, delta = _data(case, loss)
        cls, M = _cls(loss, storage), PF.matrix(A, storage)
        extra = (delta,) if loss == "huber" else ()
        kw = dict(lr=1, tol=0.0, max_iter=20, nesterov=True)
        a, _, _, _ = solve(cls(M, b, lam, *extra, scale=PF.SCALE[loss], penalty_factor=p), np.zeros(A.shape[1]), **kw)
        c, _, _, _ = solve(_make(loss, storage, A, b, lam, delta, p=p), np.zeros(A.shape[1]), **kw)
        assert a.nit == c.nit == 20 and np.array_equal(_bits(a.x), _bits(c.x)) and a.fun == c.fun


# ---- (4) the certificate ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _xhat(case, loss, weighted):
    """The factored problem (``positive`` factors) solved to 1e-12: (P(x^) in long double, x^)."""
    from zfista_amd import minimize_proximal_gradient

    A, b, lam, delta = _data(case, loss)
    p, w = _factors(case, "positive"), (_weights(case, loss) if weighted else None)
    prob = _make(loss, "csr", A, b, lam, delta, p=p, w=w)
    res = _quiet(minimize_proximal_gradient, *prob.callbacks(), np.zeros(A.shape[1]), lr=1, tol=1e-12, max_iter=20000, nesterov=True)
    return PF.primal_longdouble(A, b, p, res.x, lam, loss, delta, w=w), np.asarray(res.x)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("storage", PF.FORMS)
@pytest.mark.parametrize("loss", PF.LOSSES)
def test_every_output_within_its_rounding_bound(loss, storage, weighted, solve):
    """duality_gap(x) at x = 0 and at the iterates 20 and 300 of a FISTA solve: all eight outputs inside the bounds of
    tests/penalty_cases.py; gap >= 0 and gap >= P(x) - P(x^)."""
    case = PF.GPU_SMALL[1]   # 1000 x 257
    A, b, lam, delta = _data(case, loss)
    n = A.shape[1]
    p, w = _factors(case, "positive"), (_weights(case, loss) if weighted else None)
    prob = _make(loss, storage, A, b, lam, delta, p=p, w=w)
    res, _, _, _ = solve(prob, np.zeros(n), lr=1, tol=0.0, max_iter=300, nesterov=True, return_all=True)
    assert res.nit == 300
    P_hat, _ = _xhat(case, loss, weighted)
    gaps = []
    for k in (0, 20, 300):
        x = np.asarray(res.allvecs[k])
        vals, bounds, _ = PF.gap_longdouble(A, b, p, x, lam, loss, delta, w=w)
        got = prob.duality_gap(x)
        ratios = PF.worst_ratio(got, vals, bounds)
        worst = max(ratios, key=ratios.get)
        print(f"{loss} {storage} {'w' if weighted else '-'}, x_{k}: worst error / bound {ratios[worst]:.3g} ({worst}); gap {float(got.gap):.6g} "
              f"alpha {float(got.alpha):.6g}")
        assert all(np.isfinite(getattr(got, key)) for key in PF.KEYS8), got
        assert ratios[worst] <= 1.0, (k, worst, ratios, got)
        assert got.gap >= 0 and got.rows_gap >= 0
        Px = PF.primal_longdouble(A, b, p, x, lam, loss, delta, w=w)
        assert np.longdouble(got.gap) + bounds["gap"] + bounds["primal"] >= Px - P_hat, "P(x) - min P <= gap"
        # slot [4] is max_j |g_j| / p_j, slot [6] is g(x) itself
        ref = PF.PenaltyRef(A, b, lam, p, loss, delta, w=w)
        assert abs(float(got.grad_inf) - np.max(np.abs(ref.jac_f(x)) / p)) <= 1e-11 * float(got.grad_inf)
        assert abs(float(got.g_l1) - float(prob.g(x))) <= 4 * n * U * float(got.g_l1)
        gaps.append(float(got.gap))
    assert gaps[2] < gaps[0]
    x = np.asarray(res.allvecs[300])
    assert np.array_equal(_gap_bits(prob.duality_gap(x)), _gap_bits(prob.duality_gap(x))), "two evaluations: the same bits"


_BASE = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=100000, max_backtrack_iter=100, nesterov=True,
             nesterov_ratio=(0, 0.25), deprecated=False, return_all=False, verbose=False)


def _walk(prob, passes, gap_after=()):
    """`passes` chunks of ONE pass each; a gap call after the chunks listed in gap_after."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    run = NativeRun(prob, np.zeros(prob.n_features), dict(_BASE))
    rows, gaps = [np.zeros((0, _lib.ZF_TRACE_COLS))], {}
    for k in range(passes):
        rows.append(run.advance(1))
        if k in gap_after:
            gaps[k] = run.duality_gap()
    ctl, _ = run.solver.poll()
    out = dict(rows=np.concatenate(rows), x=run.solver.get_x(), nit=int(ctl.nit), lr=ctl.lr, F=ctl.F_old, trials=int(ctl.total_trials),
               gaps=gaps, counts=run.solver.launch_counts())
    run.solver.close()
    return out


@pytest.mark.parametrize("storage", PF.FORMS)
@pytest.mark.parametrize("loss", PF.LOSSES)
def test_the_gap_of_a_live_solve(loss, storage):
    """NativeRun.duality_gap() honours the solver's factors: it equals the standalone evaluation at get_x() bit for bit, inside the
    derived bounds; a solve probed after every pass is the solve that was never asked, bit for bit."""
    case = PF.GPU_SMALL[2]   # n = 4099: the n-passes go beyond one workgroup
    A, b, lam, delta = _data(case, loss)
    p = _factors(case, "positive")
    prob = _make(loss, storage, A, b, lam, delta, p=p, w=_weights(case, loss) if loss == "huber" else None)
    w = _weights(case, loss) if loss == "huber" else None
    passes = 24
    plain = _walk(prob, passes)
    assert plain["trials"] > plain["nit"] > 0, "the case must backtrack and accept"
    probed = _walk(prob, passes, gap_after=range(passes))
    assert (plain["nit"], plain["lr"], plain["F"], plain["trials"]) == (probed["nit"], probed["lr"], probed["F"], probed["trials"])
    assert np.array_equal(plain["rows"], probed["rows"]) and np.array_equal(plain["x"], probed["x"])
    assert plain["counts"] == probed["counts"]
    live, alone = probed["gaps"][passes - 1], prob.duality_gap(probed["x"])
    assert np.array_equal(_gap_bits(live), _gap_bits(alone)), (live, alone)
    vals, bounds, _ = PF.gap_longdouble(A, b, p, probed["x"], lam, loss, delta, w=w)
    ratios = PF.worst_ratio(live, vals, bounds)
    assert max(ratios.values()) <= 1.0, ratios
    assert live.gap < probed["gaps"][0].gap


@pytest.mark.parametrize("storage", PF.FORMS)
@pytest.mark.parametrize("loss", PF.LOSSES)
def test_gap_tol_stops_where_the_unkeyworded_solve_says(loss, storage):
    from zfista_amd import minimize_proximal_gradient as solve

    case = PF.GPU_SMALL[1]
    A, b, lam, delta = _data(case, loss)
    n = A.shape[1]
    p = _factors(case, "positive")
    prob = _make(loss, storage, A, b, lam, delta, p=p)
    P0 = float(PF.primal_longdouble(A, b, p, np.zeros(n), lam, loss, delta))
    gap_tol = 1e-4 * P0
    kw = dict(lr=1.0, nesterov=True, tol=0.0)
    res = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=4000, gap_tol=gap_tol, gap_every=1, **kw)
    assert res.success and res.status == 1 and res.message == "Duality gap reached gap_tol" and res.nit < 4000
    assert 0 <= res.dual_gap <= gap_tol and res.dual_gap == prob.duality_gap(res.x).gap
    plain = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=res.nit, return_all=True, **kw)
    assert plain.nit == res.nit and np.array_equal(plain.x, res.x) and plain.fun == res.fun, "the keyword does not alter the iterates"
    if res.nit > 1:   # checked at every iteration: the iterate before was not yet there
        assert prob.duality_gap(np.asarray(plain.allvecs[res.nit - 1])).gap > gap_tol
    print(f"{loss} {storage}: stopped at nit {res.nit}, gap {float(res.dual_gap):.3g} <= {gap_tol:.3g}")


@pytest.mark.parametrize("storage", PF.FORMS)
@pytest.mark.parametrize("loss", PF.LOSSES)
def test_lam_max_with_positive_factors(loss, storage, solve):
    case = PF.GPU_SMALL[1]
    A, b, lam, delta = _data(case, loss)
    n = A.shape[1]
    p = _factors(case, "positive")
    prob = _make(loss, storage, A, b, lam, delta, p=p)
    lmax = float(prob.lam_max())
    A1, _ = PF.scaled(A, p)
    exact = PC.lam_max(A1, b) if loss == "poisson" else W.lam_max(A1, b, np.ones(A.shape[0]), loss, delta)
    assert abs(lmax - exact) <= 1e-12 * exact
    top = prob.with_lam(lmax * (1 + 1e-9))
    assert np.array_equal(top.penalty_factor, p)
    res, _, _, _ = solve(top, np.zeros(n), lr=1, tol=0.0, max_iter=30, nesterov=True)
    assert not res.x.any(), "at lam_max the solution is 0"
    gp = top.duality_gap(np.zeros(n))
    assert gp.alpha == 1.0 and gp.gap == 0.0, "x = 0 is certified optimal at lam_max"
    low = prob.with_lam(0.99 * lmax)
    gl = low.duality_gap(np.zeros(n))
    assert gl.alpha < 1.0 and gl.gap > 0.0
    below, _, _, _ = solve(low, np.zeros(n), lr=1, tol=0.0, max_iter=200, nesterov=True)
    Pl = PF.primal_longdouble(A, b, p, below.x, 0.99 * lmax, loss, delta)
    assert below.x.any() and Pl < PF.primal_longdouble(A, b, p, np.zeros(n), 0.99 * lmax, loss, delta), "x = 0 is not optimal at 0.99 lam_max"


# ---- (5) the factored problem on A is the plain problem on A diag(1 / p) -----------------------------------------------------------------
@pytest.mark.parametrize("storage", PF.FORMS)
def test_optimum_equivalence(storage):
    from zfista_amd import minimize_proximal_gradient as solve

    case, loss = PF.GPU_SMALL[1], "square"   # 1000 x 257: full column rank
    A, b, lam, delta = _data(case, loss)
    m, n = A.shape
    scale = PF.SCALE[loss]
    p = _factors(case, "positive")
    A1, _ = PF.scaled(A, p)
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=200000, gap_tol=1e-10, gap_every=10)
    fac = _make(loss, storage, A, b, lam, delta, p=p)
    un = _make(loss, storage, A1, b, lam, delta)
    r1 = _quiet(solve, *fac.callbacks(), np.zeros(n), **kw)
    r2 = _quiet(solve, *un.callbacks(), np.zeros(n), **kw)
    assert r1.success and r2.success and r1.dual_gap <= 1e-10 and r2.dual_gap <= 1e-10
    P1 = float(PF.primal_longdouble(A, b, p, r1.x, lam, loss, delta))
    P2 = float(PF.primal_longdouble(A1, b, np.ones(n), r2.x, lam, loss, delta))
    assert abs(P1 - P2) <= 2e-10 * max(P1, 1.0), (P1, P2)
    # margins: |grad phi(z1) - grad phi(z2)| <= sqrt(2 L g1) + sqrt(2 L g2), grad phi = 2 scale (z - b), L = 2 scale (module docstring)
    x1p, x2 = np.asarray(r1.x) * p, np.asarray(r2.x)
    L = 2 * scale
    dz_bound = (np.sqrt(2 * L * float(r1.dual_gap)) + np.sqrt(2 * L * float(r2.dual_gap))) / (2 * scale)
    A1d = A1.toarray()
    rounding = 4 * U * np.linalg.norm(A1d) * max(np.linalg.norm(x1p), np.linalg.norm(x2))   # (A / p and x p: one rounding per factor)
    dz = np.linalg.norm(A1 @ x1p - A1 @ x2)
    # p o x - x' lives on the joint support S; where A'_S has full column rank, |p o x - x'| <= |A'(p o x - x')| / sigma_min(A'_S)
    S_ = np.flatnonzero((x1p != 0) | (x2 != 0))
    smin = float(np.linalg.svd(A1d[:, S_], compute_uv=False)[-1])
    assert S_.size > 0 and smin > 1e-8 * np.linalg.norm(A1d, 2), "the columns of the joint support must be independent"
    dx = np.linalg.norm(x1p - x2)
    print(f"{storage}: P {P1:.12g} / {P2:.12g} (diff {abs(P1 - P2):.3g}); |A'(p o x - x')| {dz:.3g} <= {dz_bound + rounding:.3g}; "
          f"|p o x - x'| {dx:.3g} <= {(dz_bound + rounding) / smin:.3g} (sigma_min of the {S_.size} support columns {smin:.3g}); nit {r1.nit} / {r2.nit}")
    assert dz <= dz_bound + rounding
    assert dx <= (dz_bound + rounding) / smin


# ---- (6) intercepts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", PF.FORMS)
def test_least_squares_intercept(storage, solve):
    """lam_max() of least squares with an intercept is max_j |a_j^T (b - mean b)| 2 scale.  The allowed difference: the solve for the
    intercept alone stops when |x+ - y|_inf < tol; on the unpenalised coordinate x+_0 - y_0 = -lr f'(y_0) = -lr L (y_0 - c*) with
    L = 2 scale m and c* = mean b, and x+_0 - c* = (1 - lr L)(y_0 - c*); backtracking from lr = 1 by halves accepts at the latest when
    lr L <= 1 and a step is a descent only for lr L < 2, so lr L lies in (1/2, 2) and |x+_0 - c*| = |1 - lr L| / (lr L) |x+_0 - y_0| <= tol.
    grad f(c, 0, ...)_j = 2 scale a_j^T (c 1 - b) then moves by at most 2 scale |a_j^T 1| tol."""
    from zfista_amd.problems import add_intercept

    case = PF.GPU_SMALL[0]
    A, b, lam, _ = _data(case, "square")
    b = b + 0.7   # (a mean that matters)
    m, n = A.shape
    scale, tol = 0.5, 1e-10
    A1, p = add_intercept(A if storage == "csr" else A.toarray())
    assert p.tolist() == [0.0] + [1.0] * n
    prob = _cls("square", storage)(A1, b, lam, scale=scale, penalty_factor=p)
    lmax = float(prob.lam_max(tol=tol, lr=1.0, nesterov=True))
    ld = np.longdouble
    Al = sp.csr_matrix(A)
    bl = b.astype(ld)
    r = bl - np.sum(bl) / ld(m)
    rows = np.repeat(np.arange(m), np.diff(Al.indptr))
    g = np.zeros(n, dtype=ld)
    np.add.at(g, Al.indices, Al.data.astype(ld) * r[rows])
    exact = float(np.max(np.abs(g)) * 2 * ld(scale))
    allowed = 2 * scale * float(np.max(np.abs(np.asarray(Al.sum(axis=0)).ravel()))) * tol + 1e-12 * exact
    print(f"{storage}: lam_max {lmax:.15g}, exact {exact:.15g}, diff {abs(lmax - exact):.3g} <= {allowed:.3g}")
    assert abs(lmax - exact) <= allowed
    with pytest.raises(ValueError, match=r"unpenalised column.*gap_tol=None"):
        prob.duality_gap(np.zeros(n + 1))
    with pytest.raises(ValueError, match=r"gap_tol is not available.*gap_tol=None"):
        solve(prob, np.zeros(n + 1), gap_tol=1e-6)
    top, _, plan, _ = solve(prob.with_lam(lmax * (1 + 1e-9)), np.zeros(n + 1), lr=1.0, tol=1e-13, max_iter=5000, nesterov=True)
    assert plan[0] != 1 and not top.x[1:].any() and abs(top.x[0] - b.mean()) <= 1e-11 * max(1.0, abs(b.mean())), (top.x[0], b.mean())
    low, _, _, _ = solve(prob.with_lam(0.9 * lmax), np.zeros(n + 1), lr=1.0, tol=1e-13, max_iter=5000, nesterov=True)
    assert low.x[1:].any()


@pytest.mark.parametrize("storage", PF.FORMS)
def test_poisson_intercept_path_with_exposure(storage):
    """|grad f(x)_0| at the end of a solve that stopped on |x+ - y|_inf < tol: the unpenalised coordinate moved by lr |grad f(y)_0| < tol,
    and grad f moves by at most L_up |x+ - y|_2 <= L_up sqrt(n) tol between y and x+, L_up = 2 scale sigma_max(A)^2 max_i w_i exp(z_i)
    (twice the curvature bound at x+; y lies within tol of it).  lr >= the smallest step of the solve, recorded per point."""
    from zfista_amd import _lib, minimize_proximal_gradient, proximal_gradient as pg
    from zfista_amd.path import l1_path
    from zfista_amd.problems import add_intercept

    case = PC.GAP_CASE
    A, b, lam = PC.make_poisson(*case)
    m, n = A.shape
    t = 0.5 + np.random.default_rng(11).random(m)   # exposure: the rate b / t with sample_weight = t
    A1, p = add_intercept(A if storage == "csr" else A.toarray())
    prob = _cls("poisson", storage)(A1, b / t, lam, sample_weight=t, penalty_factor=p)
    lmax = float(prob.lam_max(lr=1.0, nesterov=True))
    lams = [lmax * f for f in (0.8, 0.5, 0.3, 0.15)]
    tol = 1e-9
    kw = dict(lr=1.0, nesterov=True, tol=tol, max_iter=20000)
    with pytest.raises(ValueError, match=r"unpenalised column.*gap_tol=None"):
        l1_path(prob, lams, **kw)
    out = _quiet(l1_path, prob, lams, gap_tol=None, **kw)
    assert len(out) == 4 and [r.lam for r in out] == lams
    smax = float(np.linalg.norm(A1.toarray() if sp.issparse(A1) else A1, 2))
    x = np.zeros(n + 1)
    for r, lam_k in zip(out, lams):
        assert r.success and r.x[0] != 0.0 and "dual_gap" not in r
        # the same point alone, from the same start: the same bits, and its smallest step
        run = pg.NativeRun(prob.with_lam(lam_k), x, dict(_BASE, tol=tol, max_iter=20000))
        rows = []
        while run.status == _lib.ZF_RUNNING:
            rows.append(run.advance(50))
        lr_min = float(np.concatenate(rows)[:, _lib.TR_LR].min())
        assert np.array_equal(run.solver.get_x(), r.x)
        run.solver.close()
        sib = prob.with_lam(lam_k)
        g0 = abs(float(sib.jac_f(r.x)[0]))
        z = A1 @ r.x
        L_up = 2 * 1.0 * smax ** 2 * float(np.max(t * np.exp(z)))
        bound = tol / lr_min + L_up * np.sqrt(n + 1) * tol
        print(f"{storage} lam {lam_k:.4g}: nit {r.nit}, x0 {r.x[0]:.6g}, nnz {np.count_nonzero(r.x[1:])}, |grad_0| {g0:.3g} <= {bound:.3g}")
        assert g0 <= bound
        x = r.x
    assert np.count_nonzero(out[-1].x[1:]) > np.count_nonzero(out[0].x[1:])


# ---- (7) plumbing ------------------------------------------------------------------------------------------------------------------------
_OPTS = dict(lr=1, tol=0.0, tol_internal=1e-12, max_iter=70, max_iter_internal=100000, max_backtrack_iter=100, warm_start=False,
             decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False, deprecated=False)


def _drain(run, step=5):
    from zfista_amd import _lib

    rows = [np.zeros((0, _lib.ZF_TRACE_COLS))]
    while run.status == _lib.ZF_RUNNING:
        rows.append(run.advance(step))
    return np.concatenate(rows)


@pytest.mark.parametrize("storage", PF.FORMS)
@pytest.mark.parametrize("loss", PF.LOSSES)
def test_snapshot_resume_is_bit_identical(loss, storage, tmp_path):
    """from_snapshot recreates the solver from the problem - which sets the factors again - and continues bit for bit."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    case = PF.GPU_SMALL[0]
    A, b, lam, delta = _data(case, loss)
    prob = _make(loss, storage, A, b, lam, delta, p=_factors(case, "real"))
    whole = NativeRun(prob, np.zeros(prob.n_features), _OPTS)
    ref_rows, ref_x = _drain(whole), whole.solver.get_x()
    whole.solver.close()
    assert len(ref_rows) == 70 and ref_rows[:, _lib.TR_TRIALS].sum() > 70
    for stop_after in (3, 20):
        first = NativeRun(prob, np.zeros(prob.n_features), _OPTS)
        head = [first.advance(1) for _ in range(stop_after)]
        state = first.snapshot()
        first.solver.close()
        np.savez(tmp_path / "ckpt.npz", **state)
        run = NativeRun.from_snapshot(prob, dict(np.load(tmp_path / "ckpt.npz")), _OPTS)
        rows = np.concatenate(head + [_drain(run)])
        assert np.array_equal(rows, ref_rows) and np.array_equal(run.solver.get_x(), ref_x), stop_after
        run.solver.close()


def test_factored_siblings_on_streams_equal_the_solves_alone():
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.replicas import solve_on_streams

    case = PF.GPU_SMALL[0]
    A, b, lam, delta = _data(case, "logistic")
    n = A.shape[1]
    prob = _make("logistic", "csr", A, b, lam)
    sibs = [prob.with_penalty_factor(_factors(case, k)) for k in ("real", "positive", "ones")] + [prob]
    kw = dict(lr=1, tol=0.0, max_iter=60, nesterov=True)
    alone = [_quiet(minimize_proximal_gradient, *q.callbacks(), np.zeros(n), **kw) for q in sibs]
    both = solve_on_streams([(q, np.zeros(n), kw) for q in sibs], streams=4)
    for a, c in zip(alone, both):
        assert a.nit == c.nit == 60 and np.array_equal(a.x, c.x) and a.fun == c.fun
    assert not np.array_equal(alone[0].x, alone[1].x) and np.array_equal(alone[2].x, alone[3].x)


@pytest.mark.parametrize("storage", PF.FORMS)
def test_l1_cv_shares_one_matrix(storage):
    from zfista_amd.path import l1_cv

    case = PF.GPU_SMALL[1]
    A, b, lam, delta = _data(case, "square")
    m, n = A.shape
    p = _factors(case, "positive")
    prob = _make("square", storage, A, b, lam, p=p)
    gap_tol = 1e-4 * float(PF.primal_longdouble(A, b, p, np.zeros(n), lam, "square"))
    cv = _quiet(l1_cv, prob, [lam, 0.5 * lam, 0.25 * lam], folds=3, seed=3, gap_tol=gap_tol, return_paths=True, lr=1.0, nesterov=True, tol=0.0,
                max_iter=4000)
    assert cv.scores.shape == (3, 3) and np.isfinite(cv.scores).all() and (cv.nnz > 0).all() and len(cv.problems) == 4
    for q in cv.problems:
        assert (q._spmat is prob._spmat) if storage == "csr" else (q.A.data_ptr() == prob.A.data_ptr()), "one resident matrix"
        assert q._pf.data_ptr() == prob._pf.data_ptr() and np.array_equal(q.penalty_factor, p)
    assert all(r.success and r.dual_gap <= gap_tol for r in cv.path)
    # with an unpenalised column the default gap_tol is refused, gap_tol=None runs
    zed = prob.with_penalty_factor(_factors(case, "real"))
    with pytest.raises(ValueError, match=r"unpenalised column.*gap_tol=None"):
        l1_cv(zed, [lam], folds=3)
    cz = _quiet(l1_cv, zed, [lam, 0.5 * lam], folds=3, gap_tol=None, refit=False, lr=1.0, nesterov=True, tol=1e-8, max_iter=4000)
    assert cz.scores.shape == (3, 2) and np.isfinite(cz.scores).all()


def test_refusals_of_the_python_classes_on_the_device():
    from zfista_amd.path import l1_path
    from zfista_amd.screening import solve_screened

    case = PF.GPU_SMALL[1]
    for loss in PF.LOSSES:
        A, b, lam, delta = _data(case, loss)
        n = A.shape[1]
        for storage in PF.FORMS:
            prob = _make(loss, storage, A, b, lam, delta, p=_factors(case, "positive"))
            for call in (lambda: prob.screen(np.zeros(n)), lambda: prob.column_norms(), lambda: prob.restrict(np.arange(3)),
                         lambda: solve_screened(prob, np.zeros(n), 1e-6), lambda: l1_path(prob, [lam], screen=True)):
                with pytest.raises(ValueError, match="penalty_factor|Poisson"):
                    call()
            for call in (lambda: prob.with_penalty(lam, 0.1), lambda: l1_path(prob, [lam], l2=0.1)):
                with pytest.raises(ValueError, match="l2 > 0 is not available with penalty_factor"):
                    call()
            for bad in (np.full(n, np.nan), -np.ones(n), np.ones(n + 1)):
                with pytest.raises(ValueError, match="penalty_factor"):
                    prob.with_penalty_factor(bad)
            if loss != "logistic":
                with pytest.raises(ValueError, match="l2 > 0"):
                    extra = (delta,) if loss == "huber" else ()
                    _cls(loss, storage)(PF.matrix(A, storage), b, lam, *extra, l2=0.1, penalty_factor=np.ones(n))
    with pytest.raises(ValueError, match="group="):
        _cls("square", "dense")(np.eye(3), np.zeros(3), 0.1, group=object(), penalty_factor=np.ones(3))


def test_refusals_at_the_c_level_and_composition():
    import torch

    from oracle import problems_ref as P
    from zfista_amd import _lib
    from zfista_amd.engine import DeviceSolver
    from zfista_amd.problems import DiagQuadL1, LeastSquaresL1

    A, b, lam = P.make_plasso(512, 1024, seed=0)
    options = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=3, max_backtrack_iter=10)
    fields, keep = LeastSquaresL1(A, b, lam)._descriptor()
    pd = torch.ones(1026, dtype=torch.float64, device="cuda")
    wd = torch.ones(512, dtype=torch.float64, device="cuda")
    pp, wp = C.c_void_p(pd.data_ptr()), C.c_void_p(wd.data_ptr())
    s = DeviceSolver(fields, options, keepalive=keep)
    lib = s.lib
    assert s.ls_plan()[0] == 1, "the fused small-matrix path"
    assert lib.zf_solver_set_penalty_factors(s.handle, None) == -2 and b"null" in lib.zf_last_error()
    assert lib.zf_solver_set_penalty_factors(s.handle, C.c_void_p(pd.data_ptr() + 8)) == -2 and b"16-byte" in lib.zf_last_error()
    assert s.ls_plan()[0] == 1, "a refused call leaves the solver as it was"
    assert lib.zf_solver_set_penalty_factors(s.handle, pp) == 0 and s.ls_plan()[0] == 2, "factors switch the small-matrix path off"
    # with l2 > 0: refused in either call order; l2 = 0 is no elastic net
    assert lib.zf_solver_set_l2(s.handle, 0.25) == -2 and b"penalty factors" in lib.zf_last_error()
    assert lib.zf_solver_set_l2(s.handle, 0.0) == 0
    # any order with the losses and the row weights
    assert lib.zf_solver_set_huber(s.handle, 0.5) == 0 and lib.zf_solver_set_row_weights(s.handle, wp) == 0
    assert lib.zf_solver_set_penalty_factors(s.handle, pp) == 0
    x0 = torch.zeros(1024, dtype=torch.float64, device="cuda")
    s.init(x0.data_ptr())
    assert lib.zf_solver_set_penalty_factors(s.handle, pp) == -3 and b"before" in lib.zf_last_error()   # ZF_ERR_STATE
    s.close()
    s = DeviceSolver(fields, options, keepalive=keep)
    assert lib.zf_solver_set_l2(s.handle, 0.25) == 0
    assert lib.zf_solver_set_penalty_factors(s.handle, pp) == -2 and b"l2 > 0" in lib.zf_last_error()
    s.close()
    s = DeviceSolver(fields, options, keepalive=keep)
    assert lib.zf_solver_set_poisson(s.handle) == 0 and lib.zf_solver_set_penalty_factors(s.handle, pp) == 0 and s.ls_plan()[0] == 2
    s.close()
    # a diag kind
    d, c, lam_d = P.make_pdiag(1000, seed=1)
    f2, k2 = DiagQuadL1(d, c, lam_d)._descriptor()
    s = DeviceSolver(f2, options, keepalive=k2)
    assert lib.zf_solver_set_penalty_factors(s.handle, pp) == -2 and b"only for" in lib.zf_last_error()
    s.close()
    # ZF_ACCEPT_REMAINDER touches f only: it composes
    s = DeviceSolver(fields, dict(options, accept_mode=_lib.ZF_ACCEPT_REMAINDER), keepalive=keep)
    assert lib.zf_solver_set_penalty_factors(s.handle, pp) == 0
    s.close()
    # world > 1: the descriptor of one rank of two (no communicator is needed to create the solver)
    d, o, h = _lib.ProblemDesc(), _lib.Options(), C.c_void_p()
    for k, v in dict(fields, world=2, rank=0).items():
        setattr(d, k, v)
    for k, v in options.items():
        setattr(o, k, v)
    assert lib.zf_solver_create(C.byref(h), C.byref(d), C.byref(o), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert lib.zf_solver_set_penalty_factors(h, pp) == -2 and b"world > 1" in lib.zf_last_error()
    assert lib.zf_solver_destroy(h) == 0


def test_acceptance_remainder_with_factors(solve):
    """ZF_ACCEPT_REMAINDER replaces the acceptance test on f only, so it composes with the factors: p = 1 under it is the plain class
    under it bit for bit, and a factored solve under it ends inside what the certificate of the reference test's solve allows:
    P* >= P(x_ref) - gap(x_ref), hence P(x_rem) >= P(x_ref) - gap(x_ref) (minus the two rounding bounds), and P(x_rem) < P(0)."""
    case = PF.GPU_SMALL[0]
    A, b, lam, _ = _data(case, "square")
    n = A.shape[1]
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=300, acceptance="remainder")
    plain = _make("square", "csr", A, b, lam)
    r0, rows0, _, _ = solve(plain, np.zeros(n), **kw)
    r1, rows1, _, _ = solve(plain.with_penalty_factor(np.ones(n)), np.zeros(n), **kw)
    assert r0["acceptance"] == r1["acceptance"] == "remainder" and r0.nit == r1.nit == 300
    assert np.array_equal(rows0, rows1) and np.array_equal(_bits(r0.x), _bits(r1.x))
    p = _factors(case, "positive")
    prob = plain.with_penalty_factor(p)
    rem, _, _, _ = solve(prob, np.zeros(n), **kw)
    ref, _, _, _ = solve(prob, np.zeros(n), **dict(kw, acceptance="reference"))
    assert rem.nit == ref.nit == 300 and rem["acceptance"] == "remainder"
    gp = prob.duality_gap(ref.x)
    _, bounds, _ = PF.gap_longdouble(A, b, p, ref.x, lam, "square")
    P_rem = PF.primal_longdouble(A, b, p, rem.x, lam, "square")
    P_ref = PF.primal_longdouble(A, b, p, ref.x, lam, "square")
    assert P_rem >= P_ref - np.longdouble(gp.gap) - bounds["gap"] - bounds["primal"]
    assert P_rem < PF.primal_longdouble(A, b, p, np.zeros(n), lam, "square")
