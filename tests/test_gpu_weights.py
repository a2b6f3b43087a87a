"""GPU: per-row sample weights on the six margins classes (csrc/zf_kernels_wloss.h) and K-fold l1_cv on one resident matrix.

(1) Element bits of the weighted loss kernels: A the sparse identity (and the same matrix densified where that fits; the m x 2
    matrix [z, 0] beyond) makes the margins exact, scale makes gfac 1: the squared and Huber gradients are NumPy's w * psi bit
    for bit, the logistic gradient w * the unweighted class's; f inside its derived bound and with equal bits from both
    storage forms at every m; zero-weight rows with b = NaN / Inf leave f finite; a NaN margin on a row that is there gives NaN.
(2) w = 1: logistic and Huber are the unweighted classes bit for bit (f, jac_f, certificate, an 80-iteration solve); least
    squares in its gradient bits and, for F(x_1), to the 1e-11 of two summation forms.
(3) Solves against the CPU oracle on weight_cases.WeightedRef.
(4) 0 / 1 weights against the EXISTING unweighted classes on A[rows], b[rows].
(5) The certificate: every output inside its derived bound; the live solver's; lam_max.
(6) gap_tol.  (7) l1_cv.  (8) snapshots, streams, refusals, and that unweighted solves launch what they launched.

Measured on an MI355X when these tests were written (figures, not thresholds): the worst error of f and of the certificate
outputs is 0.026 of its derived bound; the worst iterate deviation from the oracle over all (3) solves is 6.7e-15, that of x_80
from the existing class on the row subset 1.5e-15."""
import copy
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import weight_cases as W
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-10
U = W.U
_id = lambda c: f"{c[0]}x{c[1]}"
KW80 = dict(lr=1, tol=0.0, max_iter=80, nesterov=True, return_all=True)


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _cls(loss, storage):
    from zfista_amd import problems as Z

    return {("square", "csr"): Z.SparseLeastSquaresL1, ("square", "dense"): Z.LeastSquaresL1,
            ("logistic", "csr"): Z.SparseLogisticL1, ("logistic", "dense"): Z.LogisticL1,
            ("huber", "csr"): Z.SparseHuberL1, ("huber", "dense"): Z.HuberL1}[loss, storage]


def _make(loss, storage, A, b, lam, delta=0.0, w=None, l2=0.0):
    """The class of (loss, storage) at weight_cases.SCALE; weights through with_sample_weight (the one form all six share)."""
    M = W.matrix(A, storage) if sp.issparse(A) else A
    cls, scale = _cls(loss, storage), W.SCALE[loss]
    if loss == "huber":
        p = cls(M, b, lam, delta, scale=scale, l2=l2)
    elif loss == "square":
        p = cls(M, b, lam, scale=scale, l2=l2)
    else:
        p = cls(M, b, lam, scale=scale)
        if l2 > 0:
            p = p.with_penalty(lam, l2)
    return p if w is None else p.with_sample_weight(w)


def _with_b(prob, b):
    """The same problem object on another right-hand side in HBM (rows that are not there may hold anything: the logistic
    constructors accept only -1 / +1, so their unlabeled rows get here this way)."""
    import torch

    q = copy.copy(prob)
    q.b = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64)).cuda()
    return q


@functools.lru_cache(maxsize=None)
def _data(case, loss):
    return W.make_problem(case, loss)


@functools.lru_cache(maxsize=None)
def _weights(case, kind):
    w = W.make_weights(case[0], case[3], kind)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _oracle(case, loss, kind="real"):
    """80 FISTA iterations of the REFERENCE solver on WeightedRef - computed once, shared, left unchanged."""
    from oracle import cpu_ref

    A, b, lam, delta = _data(case, loss)
    ref = W.WeightedRef(A, b, lam, _weights(case, kind), loss, delta)
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


# ---- (1) element bits ----------------------------------------------------------------------------------------------------------------
DELTA = 0.75
ROWS = [1, 63, 64, 65, 1023, 1024, 1025, 2049, 32768, 32769, 40000]
DENSE_IDENTITY_MAX = 2049


def _margins(m, loss, seed):
    """(z, b valid everywhere, b with NaN / Inf on zero-weight rows, w): margins and right-hand side on a grid of 2^-6 (z - b and
    -b z are exact), weights from {0, 0.5, 1, 3, 1e-3 random}; row 0 always carries weight 1."""
    rng = np.random.default_rng(seed)
    if loss == "logistic":
        b = rng.choice([-1.0, 1.0], m)
        z = rng.integers(-640, 641, m) / 64.0
    else:
        b = rng.integers(-128, 129, m) / 64.0
        r = rng.integers(-120, 121, m) / 64.0
        r[::7] = rng.choice([-1.0, 1.0], r[::7].size) * DELTA
        r[3::11] = 0.0
        z = b + r
    w = rng.choice([0.0, 0.5, 1.0, 3.0, -1.0], m)
    w = np.where(w < 0, 1e-3 * rng.random(m), w)
    w[0] = 1.0
    if m > 4:
        w[1] = 0.0
    bad = b.copy()
    off = np.flatnonzero(w == 0)
    bad[off[0::3]], bad[off[1::3]], bad[off[2::3]] = np.nan, np.inf, -np.inf
    z = np.where(z == 0.0, 0.0, z)
    return z, b, bad, w


def _problems_at(m, loss, z, b, bad, w):
    """{storage: (weighted problem on `bad`, unweighted problem on `b`, the x that makes the margins z, whether A is an identity)}"""
    I = sp.identity(m, format="csr", dtype=np.float64)
    out = {"csr": (_with_b(_make(loss, "csr", I, b, 0.1, DELTA, w=w), bad), _make(loss, "csr", I, b, 0.1, DELTA), z, True)}
    if m <= DENSE_IDENTITY_MAX:
        out["dense"] = (_with_b(_make(loss, "dense", np.eye(m), b, 0.1, DELTA, w=w), bad), _make(loss, "dense", np.eye(m), b, 0.1, DELTA), z, True)
    else:
        M = np.stack([z, np.zeros(m)], axis=1)
        out["dense"] = (_with_b(_make(loss, "dense", M, b, 0.1, DELTA, w=w), bad), _make(loss, "dense", M, b, 0.1, DELTA),
                        np.array([1.0, 0.0]), False)
    return out


@pytest.mark.parametrize("loss", W.LOSSES)
@pytest.mark.parametrize("m", ROWS)
def test_loss_kernels_element_bits(m, loss):
    z, b, bad, w = _margins(m, loss, seed=m)
    assert m < 8 or ((w == 0).sum() >= 1 and np.isnan(bad).any() == ((w == 0).sum() >= 1))
    with np.errstate(invalid="ignore", over="ignore"):
        psi, _ = W.row_terms(z, bad, loss, DELTA)
    want = W.weighted(w, psi)   # NumPy's w * psi, +0 where w == 0
    assert np.isfinite(want).all()
    f_exact, f_bound, _, _ = W.loss_longdouble(z, bad, w, loss, DELTA)
    got = {}
    for storage, (pw, pu, x, ident) in _problems_at(m, loss, z, b, bad, w).items():
        f = pw.f(x)
        err = abs(float(np.longdouble(f) - f_exact))
        ratio = 0.0 if err == 0.0 else err / f_bound
        print(f"m={m} {loss} {storage}: f {float(f):.17g}, error / bound {ratio:.3g}")
        assert np.isfinite(f) and f >= 0 and ratio <= 1.0, (storage, f, float(f_exact), f_bound)
        got[storage] = f
        if ident:   # gfac = 1: the gradient is w o psi itself
            grad = pw.jac_f(x)
            if loss == "logistic":
                ref = w * pu.jac_f(x)   # w * the unweighted class's gradient at the same margins (valid labels on every row)
                ref[w == 0] = 0.0
            else:
                ref = want
            nz = ref != 0.0
            wrong = np.flatnonzero(_bits(grad)[nz] != _bits(ref)[nz])
            assert wrong.size == 0, (storage, wrong[:8], grad[nz][wrong[:8]], ref[nz][wrong[:8]])
            assert (grad[~nz] == 0.0).all() and np.isfinite(grad).all()
            if loss == "logistic":   # (NumPy's exp is not the device's: the stable form agrees to rounding, not in its bits)
                np.testing.assert_allclose(ref[nz], want[nz], rtol=8 * U, atol=0)
    assert _bits(got["csr"]) == _bits(got["dense"]), "both storage forms sum a loss of the same m in the same order"


@pytest.mark.parametrize("loss", W.LOSSES)
@pytest.mark.parametrize("m", [65, 2049, 32769])
def test_a_nan_margin_on_a_row_that_is_there_gives_a_nan_f(m, loss):
    z, b, bad, w = _margins(m, loss, seed=m + 1)
    on, off = np.flatnonzero(w > 0), np.flatnonzero(w == 0)
    I = sp.identity(m, format="csr", dtype=np.float64)
    sparse = _with_b(_make(loss, "csr", I, b, 0.1, DELTA, w=w), bad)
    e1 = np.array([1.0, 0.0])
    f_of = {"csr": lambda v: sparse.f(v),
            "dense": lambda v: _with_b(_make(loss, "dense", np.stack([v, np.zeros(m)], axis=1), b, 0.1, DELTA, w=w), bad).f(e1)}
    for storage, f in f_of.items():
        assert np.isfinite(f(z)), storage
        for k in (on[0], on[on.size // 2], on[-1]):
            v = z.copy()
            v[k] = np.nan
            assert np.isnan(f(v)), (storage, k)
        v = z.copy()
        v[off[0]] = np.nan   # a row that is not there: its margin does not matter either
        assert _bits(f(v)) == _bits(f(z)), storage


# ---- (2) w = 1 -----------------------------------------------------------------------------------------------------------------------
def _gap_bits(gp, keys):
    return np.array([getattr(gp, k) for k in keys]).view(np.uint64)


@pytest.mark.parametrize("storage", W.FORMS)
@pytest.mark.parametrize("fac", [0.0, 1.0], ids=["l1", "l2=lam"])
@pytest.mark.parametrize("loss", ["logistic", "huber"])
@pytest.mark.parametrize("case", [W.SMALL[0], W.TALL], ids=_id)
def test_unit_weights_are_the_unweighted_class_bit_for_bit(case, loss, fac, storage, solve):
    from zfista_amd import _lib

    A, b, lam, delta = _data(case, loss)
    m, n = A.shape
    l2 = fac * lam
    keys = W.KEYS10 if l2 > 0 else W.KEYS8
    plain = _make(loss, storage, A, b, lam, delta, l2=l2)
    ones = plain.with_sample_weight(np.ones(m))
    assert (ones._spmat is plain._spmat) if storage == "csr" else (ones.A is plain.A), "the sibling shares the matrix"
    rng = np.random.default_rng(3)
    x = np.zeros(n)
    x[rng.choice(n, 30, replace=False)] = 0.05 * rng.standard_normal(30)
    for v in (np.zeros(n), x):
        assert _bits(ones.f(v)) == _bits(plain.f(v))
        assert np.array_equal(_bits(ones.jac_f(v)), _bits(plain.jac_f(v)))
        assert np.array_equal(_gap_bits(ones.duality_gap(v), keys), _gap_bits(plain.duality_gap(v), keys))
    assert _bits(ones.lam_max()) == _bits(plain.lam_max())
    r1, rows1, plan1, _ = solve(ones, np.zeros(n), **KW80)
    r0, rows0, plan0, _ = solve(plain, np.zeros(n), **KW80)
    assert r1.nit == r0.nit == 80 and plan1 == plan0 and rows1[:, _lib.TR_TRIALS].sum() > 80
    assert np.array_equal(rows1, rows0), "trial, lr and F traces"
    assert np.array_equal(_bits(r1.x), _bits(r0.x)) and np.array_equal(_bits(r1.allfuns), _bits(r0.allfuns))
    assert np.array_equal(np.asarray(r1.allvecs), np.asarray(r0.allvecs))


@pytest.mark.parametrize("storage", W.FORMS)
@pytest.mark.parametrize("case", [W.SMALL[2], W.SMALL[3], W.TALL], ids=_id)
def test_unit_weights_on_least_squares(case, storage, solve):
    """The gradient bits are the unweighted class's; F(x_1) is the same number from two summation forms (plain against sqrt()^2)."""
    from zfista_amd import _lib

    A, b, lam, _ = _data(case, "square")
    m, n = A.shape
    plain = _make("square", storage, A, b, lam)
    ones = plain.with_sample_weight(np.ones(m))
    rng = np.random.default_rng(4)
    x = np.zeros(n)
    x[rng.choice(n, 30, replace=False)] = 0.05 * rng.standard_normal(30)
    for v in (np.zeros(n), x):
        assert np.array_equal(_bits(ones.jac_f(v)), _bits(plain.jac_f(v)))
        assert abs(float(ones.f(v)) - float(plain.f(v))) <= 1e-11 * float(plain.f(v))
    kw = dict(lr=2.0 ** -12, tol=0.0, max_iter=1, nesterov=True)
    base, rows0, plan0, _ = solve(plain, np.zeros(n), **kw)
    res, rows, plan, _ = solve(ones, np.zeros(n), **kw)
    assert plan[0] != 1, "a weighted problem never takes the fused small-matrix path"
    assert rows[:, _lib.TR_TRIALS].tolist() == rows0[:, _lib.TR_TRIALS].tolist() == [1.0]
    if plan0[0] != 1:   # (the sibling's sums are the general path's: the same gradient, the same step)
        assert np.array_equal(_bits(res.x), _bits(base.x))
    assert rel_err(res.x, base.x) <= 1e-13 and np.count_nonzero(res.x) > 0
    assert abs(float(res.fun) - float(base.fun)) <= 1e-11 * abs(float(base.fun)), "F(x_1): the same number from two summation forms"


# ---- (3) solves against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", W.FORMS)
@pytest.mark.parametrize("loss", W.LOSSES)
@pytest.mark.parametrize("case", W.GPU_SMALL + [W.TALL], ids=_id)
def test_weighted_solve_vs_oracle(case, loss, storage, solve):
    """Real-valued weights with about 20 % zeros: every iterate of 80 against the CPU oracle on WeightedRef."""
    from zfista_amd import _lib

    A, b, lam, delta = _data(case, loss)
    w = _weights(case, "real")
    assert 0.1 <= np.mean(w == 0) <= 0.3 and (w[w > 0] != 1).all()
    exp = _oracle(case, loss)
    res, rows, plan, _ = solve(_make(loss, storage, A, b, lam, delta, w=w), np.zeros(A.shape[1]), **KW80)
    assert plan[0] == 5 if storage == "csr" else plan[0] in (2, 3, 4)
    assert exp.nit == 80 and sum(exp.alltrials) > exp.nit, "rejected trials must be present"
    assert res.nit == exp.nit
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), np.asarray(exp.alltrials, np.int64))
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float))
    worst = max(rel_err(a, e) for a, e in zip(res.allvecs, exp.allvecs))
    print(f"{_id(case)} {loss} {storage}: trials {int(rows[:, _lib.TR_TRIALS].sum())}, worst iterate deviation {worst:.3g}")
    assert worst <= TOL
    np.testing.assert_allclose(res.allfuns, exp.allfuns, rtol=TOL, atol=0)
    assert rel_err(res.allerrs, exp.allerrs) <= TOL


def test_the_constructor_keyword_is_the_sibling(solve):
    A, b, lam, delta = _data(W.SMALL[2], "huber")
    w = _weights(W.SMALL[2], "real")
    from zfista_amd import problems as Z

    for storage in W.FORMS:
        M = W.matrix(A, storage)
        for built, sib in ((_cls("huber", storage)(M, b, lam, delta, sample_weight=w), _make("huber", storage, A, b, lam, delta, w=w)),
                           (_cls("square", storage)(M, b, lam, sample_weight=w), _make("square", storage, A, b, lam, w=w))):
            assert np.array_equal(built.sample_weight, w) and np.array_equal(sib.sample_weight, w)
            x = 0.01 * np.random.default_rng(1).standard_normal(A.shape[1])
            assert _bits(built.f(x)) == _bits(sib.f(x)) and np.array_equal(_bits(built.jac_f(x)), _bits(sib.jac_f(x)))
    assert Z.LeastSquaresL1(W.matrix(A, "dense"), b, lam).sample_weight is None


# ---- (4) 0 / 1 weights against the existing classes on the row subset --------------------------------------------------------------------
@pytest.mark.parametrize("storage", W.FORMS)
@pytest.mark.parametrize("loss", W.LOSSES)
@pytest.mark.parametrize("case", [W.SMALL[0], W.SMALL[2], W.TALL], ids=_id)
def test_zero_one_weights_are_the_existing_class_on_the_row_subset(case, loss, storage, solve):
    A, b, lam, delta = _data(case, loss)
    n = A.shape[1]
    w = _weights(case, "mask")
    rows = np.flatnonzero(w > 0)
    assert 0.5 * w.size < rows.size < 0.9 * w.size
    fold = _make(loss, storage, A, b, lam, delta, w=w)
    sub = _make(loss, storage, A[rows], b[rows], lam, delta)
    rw, _, _, _ = solve(fold, np.zeros(n), **KW80)
    rs, _, _, _ = solve(sub, np.zeros(n), **KW80)
    assert rw.nit == rs.nit == 80
    print(f"{_id(case)} {loss} {storage}: x_80 deviation {rel_err(rw.x, rs.x):.3g}")
    assert rel_err(rw.x, rs.x) <= TOL
    for k in (5, 80):
        x = np.asarray(rw.allvecs[k])
        gw, gs = fold.duality_gap(x), sub.duality_gap(x)
        for key in W.KEYS8:   # (absolute, in units of P: D and the gap are differences of sums of that size)
            assert abs(float(getattr(gw, key)) - float(getattr(gs, key))) <= 1e-11 * max(float(gs.primal), 1.0), (k, key, gw, gs)


# ---- (5) the certificate -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", W.FORMS)
@pytest.mark.parametrize("fac", [0.0, 1.0], ids=["l1", "l2=lam"])
@pytest.mark.parametrize("loss", W.LOSSES)
@pytest.mark.parametrize("case", [W.SMALL[2], W.TALL], ids=_id)
def test_every_output_within_its_rounding_bound(case, loss, fac, storage, solve):
    """duality_gap(x) at x = 0 and at the iterates 20 and 300 of a FISTA solve: all eight / ten outputs inside the bounds of
    tests/weight_cases.py; gap >= 0 and gap >= F(x) - F(x_300)."""
    A, b, lam, delta = _data(case, loss)
    n = A.shape[1]
    w = _weights(case, "real")
    l2 = fac * lam
    keys = W.KEYS10 if l2 > 0 else W.KEYS8
    prob = _make(loss, storage, A, b, lam, delta, w=w, l2=l2)
    res, _, _, _ = solve(prob, np.zeros(n), lr=1, tol=0.0, max_iter=300, nesterov=True, return_all=True)
    assert res.nit == 300
    P_hat = W.primal_longdouble(A, b, w, np.asarray(res.allvecs[300]), lam, loss, delta, l2=l2)
    gaps = []
    for k in (0, 20, 300):
        x = np.asarray(res.allvecs[k])
        vals, bounds, _ = W.gap_longdouble(A, b, w, x, lam, loss, delta, l2=l2)
        got = prob.duality_gap(x)
        ratios = W.worst_ratio(got, vals, bounds)
        worst = max(ratios, key=ratios.get)
        print(f"{_id(case)} {loss} {storage} l2 = {fac} lam, x_{k}: worst error / bound {ratios[worst]:.3g} ({worst}); gap {float(got.gap):.6g} "
              f"alpha {float(got.alpha):.6g}")
        assert all(np.isfinite(getattr(got, key)) for key in keys), got
        assert ratios[worst] <= 1.0, (k, worst, ratios, got)
        assert got.gap >= 0 and got.rows_gap >= 0 and got.ridge_gap >= 0
        assert np.longdouble(got.gap) + bounds["gap"] + bounds["primal"] >= vals["primal"] - P_hat, "P(x) - min P <= gap"
        if l2 == 0:
            assert got.g_l2 == 0.0 and got.ridge_gap == 0.0
        gaps.append(float(got.gap))
    assert gaps[2] < gaps[0]
    x = np.asarray(res.allvecs[300])
    assert np.array_equal(_gap_bits(prob.duality_gap(x), keys), _gap_bits(prob.duality_gap(x), keys)), "two evaluations: the same bits"


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


@pytest.mark.parametrize("fac", [0.0, 1.0], ids=["l1", "l2=lam"])
@pytest.mark.parametrize("storage", W.FORMS)
@pytest.mark.parametrize("loss", W.LOSSES)
def test_the_gap_of_a_live_solve(loss, storage, fac):
    """NativeRun.duality_gap() equals the standalone evaluation at get_x() bit for bit (a weighted solve is always on the general
    path), and a solve probed after every pass is the solve that was never asked, bit for bit."""
    case = W.SMALL[1]   # n = 5000: more than one gap chunk
    A, b, lam, delta = _data(case, loss)
    l2 = fac * lam
    keys = W.KEYS10 if l2 > 0 else W.KEYS8
    prob = _make(loss, storage, A, b, lam, delta, w=_weights(case, "real"), l2=l2)
    passes = 24
    plain = _walk(prob, passes)
    assert plain["trials"] > plain["nit"] > 0, "the case must backtrack and accept"
    probed = _walk(prob, passes, gap_after=range(passes))
    assert (plain["nit"], plain["lr"], plain["F"], plain["trials"]) == (probed["nit"], probed["lr"], probed["F"], probed["trials"])
    assert np.array_equal(plain["rows"], probed["rows"]) and np.array_equal(plain["x"], probed["x"])
    assert plain["counts"] == probed["counts"]
    live, alone = probed["gaps"][passes - 1], prob.duality_gap(probed["x"])
    assert np.array_equal(_gap_bits(live, keys), _gap_bits(alone, keys)), (live, alone)
    assert live.gap < probed["gaps"][0].gap and (live.g_l2 > 0) == (l2 > 0)


@pytest.mark.parametrize("storage", W.FORMS)
@pytest.mark.parametrize("loss", W.LOSSES)
def test_lam_max(loss, storage, solve):
    case = W.SMALL[2]
    A, b, lam, delta = _data(case, loss)
    n = A.shape[1]
    w = _weights(case, "real")
    prob = _make(loss, storage, A, b, lam, delta, w=w)
    lmax = float(prob.lam_max())
    ref = W.WeightedRef(A, b, lam, w, loss, delta)
    numpy_lmax = float(np.max(np.abs(ref.jac_f(np.zeros(n)))))
    assert abs(lmax - numpy_lmax) <= 1e-12 * numpy_lmax and abs(lmax - W.lam_max(A, b, w, loss, delta)) <= 1e-12 * lmax
    top = prob.with_lam(lmax * (1 + 1e-9))
    assert np.array_equal(top.sample_weight, w)
    res, _, _, _ = solve(top, np.zeros(n), lr=1, tol=0.0, max_iter=30, nesterov=True)
    assert not res.x.any(), "at lam_max the solution is 0"
    gp = top.duality_gap(np.zeros(n))
    assert gp.alpha == 1.0 and gp.gap == 0.0
    below, _, _, _ = solve(prob.with_lam(0.9 * lmax), np.zeros(n), lr=1, tol=0.0, max_iter=30, nesterov=True)
    assert below.x.any()


# ---- (6) gap_tol -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", W.FORMS)
@pytest.mark.parametrize("loss", W.LOSSES)
def test_gap_tol_stops_the_solve_with_a_certificate_the_subset_class_confirms(loss, storage):
    from zfista_amd import minimize_proximal_gradient as solve

    case = W.SMALL[2]
    A, b, lam, delta = _data(case, loss)
    n = A.shape[1]
    w = _weights(case, "mask")
    rows = np.flatnonzero(w > 0)
    prob = _make(loss, storage, A, b, lam, delta, w=w)
    P0 = float(W.primal_longdouble(A, b, w, np.zeros(n), lam, loss, delta))
    gap_tol = 1e-4 * P0   # (the target of the l1_path test of tests/test_gpu_duality_gap.py: within reach of every loss here)
    kw = dict(lr=1.0, nesterov=True, tol=0.0)
    res = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=4000, gap_tol=gap_tol, **kw)
    assert res.success and res.status == 1 and res.message == "Duality gap reached gap_tol" and res.nit < 4000
    assert 0 <= res.dual_gap <= gap_tol and res.dual_gap == prob.duality_gap(res.x).gap
    sub = _make(loss, storage, A[rows], b[rows], lam, delta).duality_gap(res.x)
    print(f"{loss} {storage}: stopped at nit {res.nit}, gap {float(res.dual_gap):.3g} <= {gap_tol:.3g}; the subset class's {float(sub.gap):.3g}")
    assert sub.gap <= gap_tol + 1e-11 * max(float(sub.primal), 1.0)
    plain = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=res.nit, **kw)
    assert plain.nit == res.nit and np.array_equal(plain.x, res.x) and plain.fun == res.fun, "the keyword does not alter the iterates"


# ---- (7) l1_cv -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", W.FORMS)
@pytest.mark.parametrize("loss", W.LOSSES)
def test_l1_cv_against_the_oracles_warm_started_chains(loss, storage):
    from oracle import cpu_ref
    from zfista_amd.path import cv_summary, l1_cv

    case = W.SMALL[0]   # 300 x 1000
    A, b, lam, delta = _data(case, loss)
    m, n = A.shape
    ids = np.random.default_rng(17).integers(0, 3, m)
    w_base = _weights(case, "real") if loss == "huber" else None   # one loss runs on a problem that carries weights of its own
    wb = np.ones(m) if w_base is None else w_base
    prob = _make(loss, storage, A, b, lam, delta, w=w_base)
    lams = [2.0 * lam, lam, 0.5 * lam]
    kw = dict(lr=1, tol=0.0, max_iter=40, nesterov=True)
    cv = _quiet(l1_cv, prob, lams, folds=ids, gap_tol=None, return_paths=True, **kw)
    assert np.array_equal(cv.fold_ids, ids) and cv.folds == [0, 1, 2] and cv.scores.shape == cv.nnz.shape == (3, 3)
    assert len(cv.paths) == 3 and len(cv.path) == 3 and len(cv.problems) == 4
    for k in range(3):
        w_train, w_test = wb * (ids != k), wb * (ids == k)
        x = np.zeros(n)
        for l, lam_l in enumerate(lams):   # the oracle's chain: each point from the one before
            ref = W.WeightedRef(A, b, lam_l, w_train, loss, delta)
            exp = _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), x, **kw)
            got = cv.paths[k][l]
            assert got.nit == exp.nit == 40 and got["lam"] == lam_l
            assert rel_err(got.x, exp.x) <= TOL, (k, l, rel_err(got.x, exp.x))
            x = exp.x
            held = W.WeightedRef(A, b, lam_l, w_test, loss, delta).f(got.x) / w_test.sum()
            assert abs(cv.scores[k, l] - held) <= 1e-12 * abs(held), (k, l)
            assert cv.nnz[k, l] == np.count_nonzero(got.x)
    mean, se, best, lam_best, lam_1se = cv_summary(lams, cv.scores)
    assert np.array_equal(cv.mean, cv.scores.mean(0)) and np.allclose(cv.se, cv.scores.std(0, ddof=1) / np.sqrt(3), rtol=1e-15)
    assert cv.best == int(np.argmin(cv.mean)) == best and cv.lam_best == lams[cv.best] == lam_best
    assert cv.lam_1se == max(l for l, v in zip(lams, cv.mean) if v <= cv.mean[cv.best] + cv.se[cv.best]) == lam_1se
    # one resident matrix: the K training siblings and the problem of the refit
    if storage == "dense":
        assert len({p.A.data_ptr() for p in cv.problems}) == 1 and cv.problems[0].A.data_ptr() == prob.A.data_ptr()
    else:
        assert len({p._spmat.value.value for p in cv.problems}) == 1 and cv.problems[0]._spmat is prob._spmat
    assert len({p.b.data_ptr() for p in cv.problems}) == 1
    for k, p in enumerate(cv.problems[:3]):
        assert np.array_equal(p.sample_weight, wb * (ids != k))
    full = cv.path[-1]
    ref = W.WeightedRef(A, b, lams[-1], wb, loss, delta)
    chain = np.zeros(n)
    for lam_l in lams:
        chain = _quiet(cpu_ref.minimize_proximal_gradient, *W.WeightedRef(A, b, lam_l, wb, loss, delta).callbacks(), chain, **kw).x
    assert rel_err(full.x, chain) <= TOL and ref.f(full.x) > 0
    none = _quiet(l1_cv, prob, lams[:2], folds=ids, gap_tol=None, refit=False, **kw)
    assert none.path is None and none.paths is None and np.array_equal(none.scores, cv.scores[:, :2])


def test_l1_cv_with_drawn_folds_and_a_gap_tol():
    from zfista_amd.path import l1_cv

    case = W.SMALL[2]
    A, b, lam, delta = _data(case, "square")
    m, n = A.shape
    prob = _make("square", "csr", A, b, lam)
    gap_tol = 1e-4 * float(W.primal_longdouble(A, b, np.ones(m), np.zeros(n), lam, "square"))
    cv = _quiet(l1_cv, prob, [lam, 0.5 * lam], folds=4, seed=3, gap_tol=gap_tol, refit=False, lr=1.0, nesterov=True, tol=0.0, max_iter=4000)
    assert np.array_equal(cv.fold_ids, W.fold_ids(m, 4, 3)) and cv.scores.shape == (4, 2) and np.isfinite(cv.scores).all()
    assert cv.lam_best in (lam, 0.5 * lam) and cv.lam_1se >= cv.lam_best and (cv.nnz > 0).all()


# ---- (8) snapshots, streams, refusals, nothing moved -----------------------------------------------------------------------------------------
_OPTS = dict(lr=1, tol=0.0, tol_internal=1e-12, max_iter=70, max_iter_internal=100000, max_backtrack_iter=100, warm_start=False,
             decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False, deprecated=False)


def _drain(run, step=5):
    from zfista_amd import _lib

    rows = [np.zeros((0, _lib.ZF_TRACE_COLS))]
    while run.status == _lib.ZF_RUNNING:
        rows.append(run.advance(step))
    return np.concatenate(rows)


@pytest.mark.parametrize("storage", W.FORMS)
@pytest.mark.parametrize("loss", W.LOSSES)
def test_snapshot_resume_is_bit_identical(loss, storage, tmp_path):
    """from_snapshot recreates the solver from the problem - which sets the weights again - and continues bit for bit."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    case = W.SMALL[0]
    A, b, lam, delta = _data(case, loss)
    prob = _make(loss, storage, A, b, lam, delta, w=_weights(case, "real"))
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


@pytest.mark.parametrize("which", ["small", "tall"])
def test_two_folds_on_streams_equal_the_solves_alone(which):
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.replicas import solve_on_streams

    case = W.SMALL[1] if which == "small" else W.TALL
    A, b, lam, delta = _data(case, "logistic")
    m, n = A.shape
    prob = _make("logistic", "csr", A, b, lam)
    ids = W.fold_ids(m, 2, 0)
    folds = [prob.with_sample_weight((ids != k).astype(float)) for k in range(2)]
    kw = dict(lr=1, tol=0.0, max_iter=60, nesterov=True)
    alone = [_quiet(minimize_proximal_gradient, *p.callbacks(), np.zeros(n), **kw) for p in folds]
    both = solve_on_streams([(p, np.zeros(n), kw) for p in folds], streams=2)
    for a, c in zip(alone, both):
        assert a.nit == c.nit == 60 and np.array_equal(a.x, c.x) and a.fun == c.fun
    assert not np.array_equal(alone[0].x, alone[1].x)


def test_refusals_of_the_python_classes(monkeypatch):
    from zfista_amd import minimize_proximal_gradient as solve
    from zfista_amd.path import l1_path
    from zfista_amd.screening import solve_screened

    case = W.SMALL[2]
    for loss in W.LOSSES:
        A, b, lam, delta = _data(case, loss)
        n = A.shape[1]
        for storage in W.FORMS:
            prob = _make(loss, storage, A, b, lam, delta, w=_weights(case, "real"))
            for call in (lambda: prob.screen(np.zeros(n)), lambda: prob.column_norms(), lambda: prob.restrict(np.arange(3)),
                         lambda: solve_screened(prob, np.zeros(n), 1e-6), lambda: l1_path(prob, [lam], screen=True)):
                with pytest.raises(ValueError, match="sample_weight"):
                    call()
            for bad in ("remainder", "resolved"):
                with pytest.raises(ValueError, match="sample_weight"):
                    solve(*prob.callbacks(), np.zeros(n), acceptance=bad, max_iter=3)
            for bad_w in (np.full(A.shape[0], np.nan), -np.ones(A.shape[0]), np.zeros(A.shape[0]), np.ones(A.shape[0] + 1)):
                with pytest.raises(ValueError, match="sample_weight"):
                    prob.with_sample_weight(bad_w)
    with pytest.raises(ValueError, match="group="):
        _cls("square", "dense")(np.eye(3), np.zeros(3), 0.1, group=object(), sample_weight=np.ones(3))
    # ZF_ACCEPT in the environment falls back to the reference's test, as for Huber
    A, b, lam, _ = _data(case, "square")
    prob = _make("square", "csr", A, b, lam, w=_weights(case, "real"))
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=40)
    plain = _quiet(solve, *prob.callbacks(), np.zeros(A.shape[1]), **kw)
    for mode in ("remainder", "resolved"):
        monkeypatch.setenv("ZF_ACCEPT", mode)
        env = _quiet(solve, *prob.callbacks(), np.zeros(A.shape[1]), **kw)
        assert np.array_equal(env.x, plain.x) and env.nit == plain.nit == 40 and "acceptance" not in env
    monkeypatch.delenv("ZF_ACCEPT")
    rem = _quiet(solve, *prob.with_sample_weight(None).callbacks(), np.zeros(A.shape[1]), acceptance="remainder", **kw)
    assert rem.nit == 40 and rem["acceptance"] == "remainder", "the unweighted sibling keeps its Taylor-remainder test"


def test_refusals_at_the_c_level_and_composition():
    import ctypes as C

    import torch

    from oracle import problems_ref as P
    from zfista_amd import _lib
    from zfista_amd.engine import DeviceSolver
    from zfista_amd.problems import DiagQuadL1, LeastSquaresL1

    A, b, lam = P.make_plasso(512, 1024, seed=0)
    options = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=3, max_backtrack_iter=10)
    fields, keep = LeastSquaresL1(A, b, lam)._descriptor()
    wd = torch.ones(512, dtype=torch.float64, device="cuda")
    wp = C.c_void_p(wd.data_ptr())
    s = DeviceSolver(fields, options, keepalive=keep)
    lib = s.lib
    assert s.ls_plan()[0] == 1, "the fused small-matrix path"
    assert lib.zf_solver_set_row_weights(s.handle, None) == -2 and b"null" in lib.zf_last_error()
    assert s.ls_plan()[0] == 1, "a refused call leaves the solver as it was"
    # any order with zf_solver_set_huber and zf_solver_set_l2
    assert lib.zf_solver_set_row_weights(s.handle, wp) == 0 and s.ls_plan()[0] == 2, "weights switch the small-matrix path off"
    assert lib.zf_solver_set_huber(s.handle, 0.5) == 0 and lib.zf_solver_set_l2(s.handle, 0.25) == 0 and lib.zf_solver_set_row_weights(s.handle, wp) == 0
    x0 = torch.zeros(1024, dtype=torch.float64, device="cuda")
    s.init(x0.data_ptr())
    assert lib.zf_solver_set_row_weights(s.handle, wp) == -3 and b"before" in lib.zf_last_error()   # ZF_ERR_STATE
    s.close()
    s = DeviceSolver(fields, options, keepalive=keep)
    assert lib.zf_solver_set_huber(s.handle, 0.75) == 0 and lib.zf_solver_set_row_weights(s.handle, wp) == 0 and s.ls_plan()[0] == 2
    s.close()
    # a diag kind
    d, c, lam_d = P.make_pdiag(1000, seed=1)
    f2, k2 = DiagQuadL1(d, c, lam_d)._descriptor()
    s = DeviceSolver(f2, options, keepalive=k2)
    assert lib.zf_solver_set_row_weights(s.handle, wp) == -2 and b"only for" in lib.zf_last_error()
    s.close()
    # ZF_ACCEPT_REMAINDER
    s = DeviceSolver(fields, dict(options, accept_mode=_lib.ZF_ACCEPT_REMAINDER), keepalive=keep)
    assert lib.zf_solver_set_row_weights(s.handle, wp) == -2 and b"ZF_ACCEPT_REMAINDER" in lib.zf_last_error()
    s.close()
    # world > 1: the descriptor of one rank of two (no communicator is needed to create the solver)
    d, o, h = _lib.ProblemDesc(), _lib.Options(), C.c_void_p()
    for k, v in dict(fields, world=2, rank=0).items():
        setattr(d, k, v)
    for k, v in options.items():
        setattr(o, k, v)
    assert lib.zf_solver_create(C.byref(h), C.byref(d), C.byref(o), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert lib.zf_solver_set_row_weights(h, wp) == -2 and b"world > 1" in lib.zf_last_error()
    assert lib.zf_solver_destroy(h) == 0


def test_a_weighted_solve_in_between_does_not_disturb_the_unweighted_classes(solve):
    """Each class solved before and after a weighted solve on the same data: the same plan, launch counts and bits; the small
    least-squares matrix still takes the fused path and its weighted sibling does not."""
    from oracle import problems_ref as P
    from zfista_amd.problems import HuberL1, LeastSquaresL1, LogisticL1

    A, b, lam = P.make_plasso(512, 1024, seed=0)
    labels = np.where(b > 0, 1.0, -1.0)
    w = W.make_weights(512, 0, "real")
    kw = dict(lr=1, tol=0.0, max_iter=40, nesterov=True)
    makers = {"square": lambda: LeastSquaresL1(A, b, lam), "huber": lambda: HuberL1(A, b, lam, float(np.median(np.abs(b)))),
              "logistic": lambda: LogisticL1(A, labels, lam)}
    before = {k: solve(mk(), np.zeros(1024), **kw) for k, mk in makers.items()}
    assert before["square"][2][:2] == (1, 1), "the fused small-matrix path"
    weighted = {}
    for k, mk in makers.items():
        res, _, plan, _ = solve(mk().with_sample_weight(w), np.zeros(1024), **kw)
        assert plan[:2] == (2, 2) and res.nit == 40 and not np.array_equal(res.x, before[k][0].x)
        weighted[k] = res
    for k, mk in makers.items():
        r0, rows0, plan0, counts0 = before[k]
        r1, rows1, plan1, counts1 = solve(mk(), np.zeros(1024), **kw)
        assert plan0 == plan1 and counts0 == counts1 and np.array_equal(rows0, rows1) and np.array_equal(r0.x, r1.x), k
        same = mk()
        again = same.with_sample_weight(w).with_sample_weight(None)
        r2, rows2, plan2, counts2 = solve(again, np.zeros(1024), **kw)
        assert plan0 == plan2 and counts0 == counts2 and np.array_equal(rows0, rows2) and np.array_equal(r0.x, r2.x), k
