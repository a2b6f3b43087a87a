"""GPU: the rows passes of the margins family beyond the chunk cap.  Every loss kernel (the instantiations of
zf_loss_rows_kernel for the four losses, weighted and not, and zf_spmv_resid_kernel, with their finish kernels) and every gap rows kernel is launched on
zf_spmv_resid_chunks(m) = min(ceil(m / 1024), 1024) workgroups of 256 threads.  Up to m = 2^20 a thread makes at most four
trips of its `#pragma unroll 2` loop; beyond it the chunks grow, threads make five trips and more, and the last chunk is short.
The sizes (tests/row_chunk_cases.py; tests/test_row_chunk_cases.py proves them on the CPU): M0 = 2^20 (the last size before the
cap: 1024 chunks of 1024), M1 = 2^20 + 1 (per = 1025: a fifth trip for thread 0 only, a last chunk of two rows), M2 = 2^21 + 3
(per = 2049: nine trips, a last chunk of 1028 rows).

The sparse class runs on scipy.sparse.identity(m) at x = z, the dense class on the m x 2 matrix [z, 0] at (1, 0): the margins are
z exactly.  No tolerance is new: f and every gradient element inside the a-priori bounds of the existing long-double
restatements, the certificate inside those of gap_cases / huber_cases / poisson_cases / weight_cases, the solves at the 1e-10
of every solve test.  Each test prints its worst error / bound ratio.

Measured on an MI355X when these tests were written (figures, not thresholds): f at most 7.2e-7 of its bound (exactly the
long-double value for the unweighted squared and Huber loss, whose terms are exact on the grid), gradient elements at most 0.46
of theirs (Poisson, weighted), the certificate at most 3.2e-7, the iterates of the solves within 8.9e-15 of the oracle's.  The
bounds of f are wide because the restatements carry gamma_m of an m-term sum; tests/test_row_chunk_cases.py shows that a walk
that misses rows still leaves them by a factor of 1e5 and more.  A kernel whose walk stopped at lo + 1024 failed these tests; a
cap of 1023 chunks instead of 1024 did not, and cannot: every kernel takes `per` from its own grid, so it computes the same
sums in another order (tests/test_row_chunk_cases.py pins the cap against the source instead)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import gap_cases as GC
import huber_cases as H
import logistic_cases as L
import poisson_cases as PC
import row_chunk_cases as R
import sparse_cases as S
import weight_cases as W
from conftest import rel_err
from test_gpu_fuzz_margins import default_switches, solve   # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
TOL = 1e-10
E1 = np.array([1.0, 0.0])


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _make(loss, storage, A, b, lam=0.1, w=None):
    from zfista_amd import problems as Z

    cls = {("square", "csr"): Z.SparseLeastSquaresL1, ("square", "dense"): Z.LeastSquaresL1,
           ("logistic", "csr"): Z.SparseLogisticL1, ("logistic", "dense"): Z.LogisticL1,
           ("huber", "csr"): Z.SparseHuberL1, ("huber", "dense"): Z.HuberL1,
           ("poisson", "csr"): Z.SparsePoissonL1, ("poisson", "dense"): Z.PoissonL1}[loss, storage]
    lead = (A, b, lam, R.DELTA) if loss == "huber" else (A, b, lam)
    prob = cls(*lead, scale=R.SCALE[loss])
    return prob if w is None else prob.with_sample_weight(w)


def _spoil(prob, off):
    """NaN into b on the rows that are switched off, in device memory (the constructors refuse such a b)."""
    import torch

    prob.b[torch.from_numpy(np.flatnonzero(off)).to(prob.b.device)] = float("nan")
    return prob


# ---- the loss rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("m", R.SIZES)
def test_loss_rows_within_their_bounds(m, loss, weighted):
    z, b = R.margins(loss, m)
    w = R.weights(m) if weighted else None
    off = np.zeros(m, bool) if w is None else w == 0
    f_exact, f_bound, rho, rho_bound = R.loss_reference(loss, z, b, w)
    sparse = _make(loss, "csr", sp.identity(m, format="csr", dtype=np.float64), b, w=w)
    dense = _make(loss, "dense", np.stack([z, np.zeros(m)], axis=1), b, w=w)
    if weighted:
        _spoil(sparse, off), _spoil(dense, off)
    got = {"csr": sparse.f(z), "dense": dense.f(E1)}
    worst_f = 0.0
    for storage, f in got.items():
        err = abs(float(np.longdouble(f) - f_exact))
        worst_f = max(worst_f, 0.0 if err == 0.0 else err / f_bound)
        assert np.isfinite(f) and err <= f_bound, (storage, float(f), float(f_exact), f_bound)
    assert _bits(got["csr"]) == _bits(got["dense"]), "both classes sum a loss of the same m in the same order"
    grad = sparse.jac_f(z)   # gfac = 1 on the identity: w o psi itself, row by row
    gerr = np.abs((grad.astype(np.longdouble) - rho).astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratios = np.where(gerr == 0.0, 0.0, gerr / rho_bound)
    worst_g = float(ratios.max())
    print(f"m={m} {loss} {'weighted' if weighted else 'plain'}: f {float(got['csr']):.17g}, error / bound {worst_f:.3g}; "
          f"gradient elements up to {worst_g:.3g} of theirs")
    assert worst_g <= 1.0, (int(np.argmax(ratios)), worst_g)
    if weighted:
        assert off[-1] and (_bits(grad[off]) == 0).all(), "+0 on a row with w = 0, the last row among them"
    at = R.special_rows(m)
    assert np.signbit(z[at["neg_zero"]]) and abs(z[at["last"]]) == R.BIG and abs(z[at["fifth"]]) == R.BIG


@pytest.mark.parametrize("m", [R.M1, R.M2])
def test_an_overflowing_margin_in_the_last_chunk_gives_inf_and_a_nan_margin_nan(m):
    z, b = R.margins("poisson", m)
    lo_last = R.chunk_range(m, R.chunks(m) - 1)[0]
    sparse = _make("poisson", "csr", sp.identity(m, format="csr", dtype=np.float64), b)
    f_of = {"csr": sparse.f, "dense": lambda v: _make("poisson", "dense", np.stack([v, np.zeros(m)], axis=1), b).f(E1)}
    for storage, f in f_of.items():
        assert np.isfinite(f(z)), storage
        for k in (lo_last, m - 1, R.special_rows(m)["fifth"]):
            big = z.copy()
            big[k] = 800.0
            assert f(big) == np.inf, (storage, k, "exp overflows: inf - b z is inf, not NaN")
            bad = z.copy()
            bad[k] = np.nan
            assert np.isnan(f(bad)), (storage, k)


# ---- the gap rows --------------------------------------------------------------------------------------------------------------------
GAP_CASES = [("square", False), ("logistic", False), ("huber", False), ("poisson", False), ("logistic", True)]


@pytest.mark.parametrize("loss,weighted", GAP_CASES, ids=[f"{l}{'-weighted' if w else ''}" for l, w in GAP_CASES])
def test_gap_rows_beyond_the_cap_within_their_bounds(loss, weighted):
    """duality_gap(x) on the identity at M1 and an alpha < 1: all eight outputs inside the bounds of the long-double restatements."""
    m = R.M1
    z, b = R.margins(loss, m, heavy=False)
    w = R.weights(m) if weighted else None
    I = sp.identity(m, format="csr", dtype=np.float64)
    scale = R.SCALE[loss]

    def reference(lam):
        if weighted:
            return W.gap_longdouble(I, b, w, z, lam, loss, R.DELTA, scale)
        if loss == "poisson":
            return PC.gap_longdouble(I, b, z, lam, scale=scale)
        if loss == "huber":
            return H.gap_longdouble(I, b, z, lam, R.DELTA, scale=scale)
        return GC.gap_longdouble(I, b, z, lam, scale, loss == "logistic")

    lam = 0.25 * float(reference(1.0)[0]["grad_inf"])
    vals, bounds, _ = reference(lam)
    vals, bounds = {k: vals[k] for k in GC.KEYS}, {k: bounds[k] for k in GC.KEYS}
    assert 0 < float(vals["alpha"]) < 1
    got = _make(loss, "csr", I, b, lam=lam, w=w).duality_gap(z)
    ratios = W.worst_ratio(got, vals, bounds)
    worst = max(ratios, key=ratios.get)
    print(f"m={m} {loss} weighted {weighted}: worst error / bound {ratios[worst]:.3g} ({worst}); gap {float(got.gap):.6g} "
          f"alpha {float(got.alpha):.6g} rows {float(got.rows_gap):.6g}")
    assert all(np.isfinite(getattr(got, k)) for k in GC.KEYS), got
    assert ratios[worst] <= 1.0, (worst, ratios)
    assert got.gap >= 0 and got.rows_gap > 0


# ---- in the loop ---------------------------------------------------------------------------------------------------------------------
LOOP_CASES = [("square", False), ("logistic", False), ("huber", False), ("poisson", False), ("huber", True)]


def _loop_ref(loss, A, b, lam, delta, w):
    if w is not None:
        return W.WeightedRef(A, b, lam, w, loss, delta, R.SCALE[loss])
    if loss == "poisson":
        return PC.PoissonRef(A, b, lam, R.SCALE[loss])
    if loss == "huber":
        return H.HuberRef(A, b, lam, delta, R.SCALE[loss])
    if loss == "logistic":
        return L.LogisticL1Ref(A, b, lam, R.SCALE[loss])
    return S.SparseLeastSquaresL1Ref(A, b, lam, R.SCALE[loss])


@pytest.mark.parametrize("loss,weighted", LOOP_CASES, ids=[f"{l}{'-weighted' if w else ''}" for l, w in LOOP_CASES])
def test_three_fista_iterations_beyond_the_cap_against_the_oracle(loss, weighted, solve):
    """M1 x 64, two stored elements per row, from x0 = 0.1 N(0, 1): the momentum form and the ring slots of the same kernels."""
    from oracle import cpu_ref
    from zfista_amd import _lib

    A, b, lam, delta = R.loop_problem(loss)
    m, n = A.shape
    w = R.weights(m) if weighted else None
    x0 = 0.1 * np.random.default_rng(11).standard_normal(n)
    kw = dict(lr=1.0, tol=0.0, max_iter=3, nesterov=True, nesterov_ratio=(0, 0.25), return_all=True)
    with np.errstate(all="ignore"):
        exp = _quiet(cpu_ref.minimize_proximal_gradient, *_loop_ref(loss, A, b, lam, delta, w).callbacks(), x0, **kw)
    assert exp.nit == 3 and np.isfinite(exp.allfuns).all()
    lead = (A, b, lam, delta) if loss == "huber" else (A, b, lam)
    from zfista_amd import problems as Z

    cls = {"square": Z.SparseLeastSquaresL1, "logistic": Z.SparseLogisticL1, "huber": Z.SparseHuberL1, "poisson": Z.SparsePoissonL1}[loss]
    prob = cls(*lead, scale=R.SCALE[loss])
    if w is not None:
        prob = prob.with_sample_weight(w)
    res, rows, _ = solve(prob, x0, **kw)
    assert res.nit == 3 and len(rows) == 3
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float))
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), np.asarray(exp.alltrials, np.int64)) and sum(exp.alltrials) > 3
    worst = max(rel_err(a, e) for a, e in zip(res.allvecs, exp.allvecs))
    print(f"m={m} {loss} weighted {weighted}: trials {list(exp.alltrials)}, iterates within {worst:.3g}, "
          f"F within {np.max(np.abs(np.asarray(res.allfuns) / np.asarray(exp.allfuns) - 1)):.3g}")
    assert worst <= TOL and rel_err(res.x, exp.x) <= TOL
    np.testing.assert_allclose(res.allfuns, exp.allfuns, rtol=TOL, atol=0)
