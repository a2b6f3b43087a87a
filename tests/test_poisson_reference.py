"""CPU: the case table and the restatements of tests/poisson_cases.py - the closures are the stated expressions; two summation
orders of the loss decide alike on every case; the overflowing first trial is where it is claimed; the long-double certificate
is P - D, every row and column term of it is >= 0, its rows part is exactly 0 at alpha = 1; and every bound is far smaller
than the quantity it guards."""
import warnings

import numpy as np
import pytest

import poisson_cases as PC
from oracle import cpu_ref

ALL = PC.SMALL + [PC.TALL]
_id = lambda c: f"{c[0]}x{c[1]}"
_CASES = {}


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _case(case):
    """(A, b, lam, {k: x_k of backtracking FISTA}) - one run per case, shared and left unchanged."""
    if case not in _CASES:
        A, b, lam = PC.make_poisson(*case)
        _, kept = PC.fista(A, b, lam, np.zeros(A.shape[1]), 80, record=(20, 80))
        kept[0] = np.zeros(A.shape[1])
        _CASES[case] = (A, b, lam, kept)
    return _CASES[case]


def test_the_closures_are_the_stated_expressions():
    A, b, lam = PC.make_poisson(*PC.GAP_CASE)
    rng = np.random.default_rng(0)
    x = 0.05 * rng.standard_normal(A.shape[1])
    z = A @ x
    w = PC.case_weights(PC.GAP_CASE)
    for storage in PC.FORMS:
        ref = PC.PoissonRef(PC.matrix(A, storage), b, lam)
        assert abs(ref.f(x) - np.sum(np.exp(z) - b * z)) <= 1e-13 * abs(ref.f(x))
        np.testing.assert_allclose(ref.jac_f(x), A.T @ (np.exp(z) - b), rtol=1e-12, atol=1e-12)
        g = ref.jac_f(x)
        for j in rng.choice(A.shape[1], 5, replace=False):   # the gradient is the derivative (central differences)
            e = np.zeros_like(x)
            e[j] = 1e-6
            assert abs((ref.f(x + e) - ref.f(x - e)) / 2e-6 - g[j]) <= 1e-5 * max(1.0, abs(g[j]))
        # exposure is exactly a sample weight: counts c ~ Poisson(t exp(z)) have the loss t exp(z) - c z = t (exp(z) - (c / t) z)
        t = 0.5 + rng.random(b.size)
        direct = np.sum(t * np.exp(z) - b * z)
        assert abs(PC.PoissonRef(PC.matrix(A, storage), b / t, lam, sample_weight=t).f(x) - direct) <= 1e-13 * abs(direct)
        # a row with w = 0 is a row that is not there, whatever its count holds
        bad = b.copy()
        bad[w == 0] = np.nan
        assert PC.PoissonRef(PC.matrix(A, storage), bad, lam, sample_weight=w).f(x) == PC.PoissonRef(PC.matrix(A, storage), b, lam, sample_weight=w).f(x)
        assert np.array_equal(PC.PoissonRef(PC.matrix(A, storage), bad, lam, sample_weight=w).jac_f(x),
                              PC.PoissonRef(PC.matrix(A, storage), b, lam, sample_weight=w).jac_f(x))
    # overflow and NaN: +inf, never NaN, from a margin beyond the range of exp; NaN from a NaN margin
    psi, phi = PC.poisson_terms(np.array([800.0, -800.0, np.nan, 0.0, -0.0]), np.array([3.0, 3.0, 1.0, 0.0, 2.0]))
    assert phi[0] == np.inf and psi[0] == np.inf and phi[1] == 2400.0 and psi[1] == -3.0 and np.isnan(phi[2]) and np.isnan(psi[2])
    assert phi[3] == 1.0 and phi[4] == 1.0 and psi[4] == -1.0
    assert np.sum(phi[[0, 1, 3]]) == np.inf


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_the_case_table(case):
    """What the recipe is claimed to give: counts up to 5 - 8, 34 - 47 % zero counts, lam = 0.1 lam_max."""
    A, b, lam = PC.make_poisson(*case)
    assert (b >= 0).all() and (b == np.round(b)).all() and 3 <= b.max() <= 8
    assert 0.34 <= np.mean(b == 0) <= 0.47
    assert abs(lam - 0.1 * PC.lam_max(A, b)) <= 1e-13 * lam


@pytest.mark.parametrize("tag", sorted(PC.GOLDEN_VARIANTS))
@pytest.mark.parametrize("case", ALL, ids=_id)
def test_two_summation_orders_decide_alike(case, tag):
    """80 iterations from lr = 1 on the closures and on the closures over the reversed rows: the same trial sequence, 9 - 16
    rejected trials at the start, iterates within 3e-15."""
    A, b, lam = PC.make_poisson(*case)
    x0 = np.zeros(A.shape[1])
    kw = dict(PC.GOLDEN_KW, **PC.GOLDEN_VARIANTS[tag])
    fwd = _quiet(cpu_ref.minimize_proximal_gradient, *PC.PoissonRef(A, b, lam).callbacks(), x0, **kw)
    rev = _quiet(cpu_ref.minimize_proximal_gradient, *PC.PoissonRef(A, b, lam, reverse=True).callbacks(), x0, **kw)
    assert fwd.nit == rev.nit == 80
    assert list(fwd.alltrials) == list(rev.alltrials) and list(fwd.alllrs) == list(rev.alllrs)
    assert 9 <= sum(fwd.alltrials) - 80 <= 16, "rejected trials"
    assert fwd.alltrials[0] >= 9, "the line search starts with a run of rejections from lr = 1"
    worst = max(np.linalg.norm(a - c) / np.linalg.norm(c) for a, c in zip(fwd.allvecs[1:], rev.allvecs[1:]))
    print(_id(case), tag, "trials", sum(fwd.alltrials), "iterates within", worst)
    assert worst <= 3e-15
    if sp_dense_fits(case):
        dense = _quiet(cpu_ref.minimize_proximal_gradient, *PC.PoissonRef(A.toarray(), b, lam).callbacks(), x0, **kw)
        assert list(dense.alltrials) == list(fwd.alltrials), "the dense closures take the same trials"


def sp_dense_fits(case):
    return case[0] * case[1] <= 10_000_000


def test_the_overflow_trial_is_where_it_is_claimed():
    """The first trial of the 2000 x 5000 case from lr = 1: its largest margin is beyond the range of exp, f(x+) = +inf (not
    NaN), the trial is rejected and the solve goes on."""
    A, b, lam = PC.make_poisson(*PC.OVERFLOW_CASE)
    ref = PC.PoissonRef(A, b, lam)
    x0 = np.zeros(A.shape[1])
    x1 = ref.prox_wsum_g(1.0, x0 - 1.0 * ref.jac_f(x0))
    zmax = float(np.max(A @ x1))
    print("largest margin of the first trial:", zmax)
    assert 1000 < zmax < 1025 and zmax > 709.8
    with np.errstate(over="ignore"):
        assert ref.f(x1) == np.inf
    res = _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), x0, **PC.GOLDEN_KW, nesterov=True)
    assert res.alltrials[0] > 1 and res.nit == 80 and np.isfinite(res.allfuns).all()
    for case in PC.SMALL:   # no other SMALL case overflows on its first trial
        if case != PC.OVERFLOW_CASE:
            A2, b2, lam2 = PC.make_poisson(*case)
            r2 = PC.PoissonRef(A2, b2, lam2)
            z2 = A2 @ r2.prox_wsum_g(1.0, -r2.jac_f(np.zeros(A2.shape[1])))
            assert np.max(z2) < 709


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("fac", [0.0, 1.0], ids=["l1", "l2=lam"])
@pytest.mark.parametrize("case", ALL, ids=_id)
def test_restatement_gap_is_p_minus_d_with_non_negative_terms(case, fac, weighted):
    A, b, lam, xs = _case(case)
    w = PC.case_weights(case) if weighted else None
    l2 = fac * lam
    for k in sorted(xs):
        vals, bounds, extra = PC.gap_longdouble(A, b, xs[k], lam, l2=l2, w=w)
        scale_of = max(abs(float(vals["primal"])), abs(float(vals["dual"])), 1.0)
        assert abs(float(vals["gap"] - extra["gap_pd"])) <= 1e-12 * scale_of, "rows + columns (+ ridge) = P - D"
        assert (extra["terms"] >= 0).all() and (extra["col_terms"] >= -1e-18).all(), "every row and column term is >= 0"
        assert vals["gap"] >= 0 and vals["rows_gap"] >= 0 and 0 < vals["alpha"] <= 1
        assert all(np.isfinite(v) and v >= 0 for v in bounds.values())
        assert set(vals) == set(PC.KEYS10 if l2 > 0 else PC.KEYS8)
        assert 0.3 <= extra["zero_share"] <= 0.6, "rows with b = 0 are there (weighted: the switched-off rows count as such)"
    if not weighted and fac == 0.0:
        assert float(PC.gap_longdouble(A, b, xs[80], lam)[0]["gap"]) < float(PC.gap_longdouble(A, b, xs[0], lam)[0]["gap"])


def test_the_direct_form_and_the_stable_form_of_a_row_gap_agree():
    """e - v + v (log v - z) against e ((1 + d) log1p(d) - d) in longdouble, on both sides of the branch point d = 1, at
    b = 0 and at the ends of |z| <= 700."""
    ld = np.longdouble
    z = np.array([-700.0, -30.0, -1.0, 0.0, 0.5, 3.0, 30.0, 700.0] * 3).astype(ld)
    b = np.repeat([0.0, 2.0, 7.0], 8).astype(ld)
    for alpha in (ld(0.999), ld(0.5), ld(1e-3)):
        oma = 1 - alpha
        t, d, v = PC.row_gap_longdouble(np.exp(z), z, b, alpha, oma, alpha * np.log(alpha))
        e = np.exp(z)
        with np.errstate(divide="ignore", invalid="ignore"):
            direct = (e - v) + v * (np.log(np.where(v > 0, v, ld(1))) - z)
        assert np.isfinite(t).all() and (t >= 0).all() and (d >= -1).all()
        assert (d > 1).any() and (d <= 1).any()
        size = np.abs(e) + np.abs(v) * (1 + np.abs(np.log(np.where(v > 0, v, ld(1)))) + np.abs(z))   # (log v and z round separately)
        assert (np.abs(t - direct) <= 64 * ld(2.0) ** -63 * size).all()


def test_rows_part_is_exactly_zero_at_alpha_one():
    A, b, lam, xs = _case(PC.SMALL[0])
    big = 2.0 * PC.lam_max(A, b)
    vals, bounds, extra = PC.gap_longdouble(A, b, np.zeros(A.shape[1]), big)
    assert vals["alpha"] == 1 and vals["rows_gap"] == 0 and bounds["rows_gap"] == 0.0 and bounds["alpha"] == 0.0
    assert vals["gap"] == 0 and vals["primal"] == vals["f"], "x = 0 is optimal at lam >= lam_max"
    assert abs(float(vals["primal"] - vals["dual"])) <= 1e-15 * float(vals["primal"]), "D = -sum (1 log 1 - 1) = m = f(0)"
    assert float(vals["f"]) == A.shape[0]


def test_every_bound_is_far_below_what_it_guards():
    """On the 1000 x 257 case after 80 iterations: the bound of f, of the largest gradient element and of each certificate
    output is at least 100 x smaller than the quantity itself."""
    A, b, lam, xs = _case(PC.GAP_CASE)
    x = xs[80]
    z = A @ x
    f, f_bound, psi, psi_bound = PC.loss_longdouble(z, b, PC.SCALE)
    assert 100 * f_bound <= abs(float(f))
    k = int(np.argmax(np.abs(psi)))
    assert 100 * psi_bound[k] <= abs(float(psi[k]))
    for l2 in (0.0, lam):
        vals, bounds, _ = PC.gap_longdouble(A, b, x, lam, l2=l2, w=PC.case_weights(PC.GAP_CASE))
        for key in vals:
            assert 100 * bounds[key] <= abs(float(vals[key])), (key, bounds[key], float(vals[key]))
