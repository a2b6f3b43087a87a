"""CPU: the weighted closures of tests/weight_cases.py under the reference's solver, and the long-double restatements.

The two exact equivalences that stand in for a reference implementation of sample weights (the reference project has none):
    0 / 1 weights       are  the unweighted problem on the rows with w = 1
    integer weights     are  the unweighted problem with row i repeated w_i times
Both pairs differ only in the order and grouping of their row sums, so under the oracle solver they must take the same
accept / reject decisions and agree to the project's TOL.  On sparse_cases.SMALL and TALL, all three losses, 80 FISTA
iterations from lr = 1: decisions equal in all 30 combinations, worst iterate deviation 2e-14 (weight_cases.make_weights
says how the integer weights were chosen)."""
import warnings

import numpy as np
import pytest

import gap_cases as GC
import huber_cases as H
import weight_cases as W
from conftest import rel_err
from oracle import cpu_ref

TOL = 1e-10
KW = dict(lr=1, tol=0.0, max_iter=80, nesterov=True, return_all=True)
CASES = list(W.SMALL) + [W.TALL]
_id = lambda c: f"{c[0]}x{c[1]}"


def _solve(ref, n):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cpu_ref.minimize_proximal_gradient(*ref.callbacks(), np.zeros(n), **KW)


@pytest.mark.parametrize("kind", ["mask", "int"])
@pytest.mark.parametrize("loss", W.LOSSES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_integer_weights_are_repeated_rows_under_the_oracle_solver(case, loss, kind):
    A, b, lam, delta = W.make_problem(case, loss)
    n = A.shape[1]
    w = W.make_weights(A.shape[0], case[3], kind)
    assert (w == 0).any() and (kind == "mask" or (w > 1).any())
    weighted = _solve(W.WeightedRef(A, b, lam, w, loss, delta), n)
    sub, rows = W.subset_ref(A, b, lam, w, loss, delta)
    assert rows.size == int(w.sum())
    plain = _solve(sub, n)
    assert weighted.nit == plain.nit == 80
    assert list(weighted.alltrials) == list(plain.alltrials) and list(weighted.alllrs) == list(plain.alllrs)
    worst = max(rel_err(a, e) for a, e in zip(weighted.allvecs, plain.allvecs))
    print(f"{_id(case)} {loss} {kind}: trials {sum(weighted.alltrials)}, worst iterate deviation {worst:.3g}")
    assert worst <= TOL
    np.testing.assert_allclose(weighted.allfuns, plain.allfuns, rtol=TOL, atol=0)


@pytest.mark.parametrize("loss", W.LOSSES)
def test_zero_weight_rows_are_not_there_whatever_b_holds(loss):
    A, b, lam, delta = W.make_problem(W.SMALL[0], loss)
    w = W.make_weights(A.shape[0], 3, "real")
    off = np.flatnonzero(w == 0)
    assert off.size >= 20
    bad = b.copy()
    bad[off[0::3]], bad[off[1::3]], bad[off[2::3]] = np.nan, np.inf, -np.inf
    x = 0.01 * np.random.default_rng(0).standard_normal(A.shape[1])
    good, ugly = W.WeightedRef(A, b, lam, w, loss, delta), W.WeightedRef(A, bad, lam, w, loss, delta)
    assert np.isfinite(ugly.f(x)) and ugly.f(x) == good.f(x) and np.array_equal(ugly.jac_f(x), good.jac_f(x))
    rho = W.weighted(w, W.row_terms(A @ x, bad, loss, delta)[0])
    assert not np.signbit(rho[off]).any() and (rho[off] == 0).all()
    for storage_b in (b, bad):
        f, bound, _, _ = W.loss_longdouble(A @ x, storage_b, w, loss, delta)
        assert abs(float(np.longdouble(good.f(x)) - f)) <= bound


@pytest.mark.parametrize("l2fac", [0.0, 1.0])
@pytest.mark.parametrize("loss", W.LOSSES)
def test_the_long_double_certificate(loss, l2fac):
    """With unit weights the values are those of tests/gap_cases.py / tests/huber_cases.py; with 0 / 1 weights those of the row
    subset; gap = P - D in long double; the fp64 closures lie inside the bound of f."""
    ld = np.longdouble
    A, b, lam, delta = W.make_problem(W.SMALL[2], loss)
    m, n = A.shape
    l2 = l2fac * lam
    rng = np.random.default_rng(5)
    x = np.zeros(n)
    x[rng.choice(n, 25, replace=False)] = 0.05 * rng.standard_normal(25)
    ones, _, _ = W.gap_longdouble(A, b, np.ones(m), x, lam, loss, delta, l2=l2)
    if loss == "huber":
        old, _, _ = H.gap_longdouble(A, b, x, lam, delta, l2=l2)
    elif l2 == 0:
        old, _, _ = GC.gap_longdouble(A, b, x, lam, W.SCALE[loss], loss == "logistic")
    else:
        import enet_cases as E

        old = E.gap_longdouble(A, b, x, lam, l2, W.SCALE[loss], loss == "logistic")[0]
    for k in old:
        assert abs(float(ones[k] - old[k])) <= 1e-17 * max(1.0, abs(float(old[k]))), k
    for kind in ("mask", "real"):
        w = W.make_weights(m, 11, kind)
        vals, bounds, extra = W.gap_longdouble(A, b, w, x, lam, loss, delta, l2=l2)
        assert abs(float(vals["gap"] - extra["gap_pd"])) <= 1e-15 * abs(float(vals["primal"])), "gap = P - D"
        assert all(v > 0 for k, v in bounds.items() if k not in ("alpha", "g_l2", "ridge_gap")) and vals["gap"] >= 0
        ref = W.WeightedRef(A, b, lam, w, loss, delta, l2=l2)
        assert abs(float(ld(ref.f(x)) - vals["f"])) <= bounds["f"]
        assert abs(float(ld(np.max(np.abs(ref.jac_f(x) + l2 * x))) - vals["grad_inf"])) <= bounds["grad_inf"]
        if kind == "mask":
            keep = w > 0
            sub, _, _ = W.gap_longdouble(A[keep], b[keep], np.ones(int(keep.sum())), x, lam, loss, delta, l2=l2)
            for k in vals:
                assert abs(float(vals[k] - sub[k])) <= 1e-16 * max(1.0, abs(float(sub[k]))), k


def test_fold_ids():
    ids = W.fold_ids(7, 3, seed=0)
    perm = np.random.default_rng(0).permutation(7)
    assert sorted(np.bincount(ids).tolist()) == [2, 2, 3] and all(ids[perm[k]] == k % 3 for k in range(7))
