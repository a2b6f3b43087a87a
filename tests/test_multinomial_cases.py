"""CPU: the multinomial case module is honest.  The two closures (per row / Kronecker) agree with each other and with the
scipy.special forms to a few ulps; the oracle solves every case, ending and ALL_K entry alike on both; the long-double restatement
agrees with the fp64 closures inside its own bounds; every row gap is >= 0 and exactly 0 at alpha = 1; D <= P at random points; the
gradient passes a finite-difference check."""
import contextlib
import io
import warnings

import numpy as np
import pytest
import scipy.special as ssp

import multinomial_cases as MC
from oracle import cpu_ref

U = MC.U


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with contextlib.redirect_stdout(io.StringIO()):
            return fn(*a, **k)


def test_the_tables_cover_what_they_say():
    assert MC.REPLACED == 0, "no seed had to be replaced when the tables were drawn"
    assert {c.K for c in MC.CASES} == {2, 3, 5, 8, 12, 16}
    assert {c.weights for c in MC.CASES} == {None, "real", "nan"} and {c.factors for c in MC.CASES} == {None, "pos", "zero"}
    assert {bool(c.l2fac) for c in MC.CASES} == {False, True} and any(c.box for c in MC.CASES)
    assert {c.labels for c in MC.CASES} == {"hot", "soft"} and any(c.absent for c in MC.CASES)
    assert len({c.id for c in MC.CASES + MC.ENDINGS + MC.ALL_K}) == len(MC.CASES + MC.ENDINGS + MC.ALL_K)
    assert [c.K for c in MC.ALL_K] == list(range(2, 17)) and all(c.m == 33 and c.n in (67, 130) and c.opts["max_iter"] == 30 for c in MC.ALL_K)
    assert {c.n for c in MC.ALL_K} == {67, 130}
    assert sorted(c.tag for c in MC.ENDINGS) == sorted(["tol", "fail0", "one"] * 3)
    for c in MC.CASES:
        A, Y, lam, w, Pf, l2 = c.data()
        there = np.ones(c.m, bool) if w is None else w != 0
        assert np.all(np.abs(Y[there].sum(axis=1) - 1) <= 1e-12) and np.all(Y[there] >= 0)
        if c.weights == "nan":
            assert np.isnan(Y[~there]).all() and (~there).sum() >= 1
        if c.weights:
            assert (w == 0).sum() >= 1 and (w > 0).sum() >= 1
        if c.absent:
            assert not Y[there][:, -1].any(), "the last class never occurs"
        if c.labels == "hot" and c.weights != "nan":
            assert set(np.unique(Y)) == {0.0, 1.0}
        if c.factors == "zero":
            assert Pf[0] == 0.0 and np.all(Pf[1:] > 0)
    for K in (2, 16):
        rows = MC.eval_rows(K)
        first = MC.WIDE // K + 1
        assert first in rows and first - 1 in rows and first * K > MC.WIDE >= (first - 1) * K


def test_row_terms_match_the_scipy_forms_to_a_few_ulps():
    rng = np.random.default_rng(0)
    for K in MC.KS:
        Z = 5.0 * rng.standard_normal((200, K))
        Y = rng.dirichlet(np.ones(K), 200)
        psi, phi = MC.row_terms(Z, Y)
        ref_phi = ssp.logsumexp(Z, axis=1) - np.sum(Y * Z, axis=1)
        ref_psi = ssp.softmax(Z, axis=1) - Y
        size = np.abs(ssp.logsumexp(Z, axis=1)) + np.sum(np.abs(Y * Z), axis=1)   # the scipy form cancels: its own terms
        assert np.all(np.abs(phi - ref_phi) <= (K + 8) * U * size), K
        assert np.all(np.abs(psi - ref_psi) <= 8 * U), K
        assert np.all(phi >= 0)
    # one class at +-700: finite; a NaN or an infinite margin: NaN
    Z = np.zeros((4, 3))
    Z[0, 1], Z[1, 1] = 700.0, -700.0
    Z[2, 0], Z[3, 2] = np.nan, np.inf
    psi, phi = MC.row_terms(Z, MC.one_hot([0, 1, 1, 0], 3))
    assert np.isfinite(phi[:2]).all() and np.isfinite(psi[:2]).all() and phi[0] == 700.0 and abs(phi[1] - (700.0 + np.log(2.0))) < 1e-12
    assert np.isnan(phi[2]) and np.isnan(phi[3])


def test_a_row_that_is_not_there_gives_plus_zero_whatever_it_holds():
    Z = np.array([[1.0, 2.0, 3.0], [0.5, np.nan, 1.0], [1.0, 1.0, 1.0]])
    Y = np.array([[1.0, 0.0, 0.0], [np.nan, np.nan, np.nan], [0.0, 1.0, 0.0]])
    w = np.array([2.0, 0.0, 0.5])
    psi, phi = MC.weighted(w, *MC.row_terms(Z, Y))
    assert not np.signbit(psi[1]).any() and (psi[1] == 0).all() and phi[1] == 0 and not np.signbit(phi[1])
    p0, f0 = MC.row_terms(Z[[0, 2]], Y[[0, 2]])
    assert np.array_equal(psi[[0, 2]], w[[0, 2], None] * p0) and np.array_equal(phi[[0, 2]], w[[0, 2]] * f0)


ALL = [("CASES", i) for i in range(len(MC.CASES))] + [("ENDINGS", i) for i in range(len(MC.ENDINGS))] + [("ALL_K", i) for i in range(len(MC.ALL_K))]


@pytest.mark.parametrize("table,idx", ALL, ids=[getattr(MC, t)[i].id for t, i in ALL])
def test_the_oracle_solves_every_case_alike_on_both_closures(table, idx):
    case = getattr(MC, table)[idx]
    a = _quiet(cpu_ref.minimize_proximal_gradient, *case.ref().callbacks(), case.x0(), return_all=True, **case.opts)
    b = _quiet(cpu_ref.minimize_proximal_gradient, *case.ref(MC.KronRef).callbacks(), case.x0(), return_all=True, **case.opts)
    assert a.nit == b.nit and a.message == b.message and a.success == b.success
    assert list(a.alltrials) == list(b.alltrials) and list(a.alllrs) == list(b.alllrs), "both evaluations decide every trial alike"
    size = max(1.0, max(float(np.max(np.abs(v))) for v in a.allvecs))
    assert max(float(np.max(np.abs(x - y))) for x, y in zip(a.allvecs, b.allvecs)) <= MC.ITER_TOL * size * max(1, a.nit)
    assert np.all(np.isfinite(np.asarray(a.allfuns, float)))
    if case.tag == "tol":
        assert a.success and a.nit < case.opts["max_iter"]
    elif case.tag == "fail0":
        assert not a.success and "Backtracking failed" in a.message
    elif case.tag == "one":
        assert a.nit == 1
    elif case.tag == "allk":
        assert a.nit == 30
    else:
        assert a.nit == case.opts["max_iter"] and np.any(a.x != 0)
    if case.box:
        assert np.all(a.x >= case.box[0]) and np.all(a.x <= case.box[1])
    if case.factors == "zero":
        assert np.any(a.x.reshape(case.n, case.K)[0] != 0), "the unpenalised row moves"


@pytest.mark.parametrize("idx", range(len(MC.CASES)), ids=[c.id for c in MC.CASES])
def test_the_longdouble_restatement_brackets_the_fp64_closures(idx):
    case = MC.CASES[idx]
    A, Y, lam, w, Pf, l2 = case.data()
    ref = case.ref()
    rng = np.random.default_rng(idx)
    for x in (np.zeros(case.n * case.K), 0.3 * rng.standard_normal(case.n * case.K) * (rng.random(case.n * case.K) < 0.3)):
        Z = A @ x.reshape(case.n, case.K)
        ds = MC.GC._gamma(case.n) * (np.abs(A) @ np.abs(x.reshape(case.n, case.K)))
        f, fb, wpsi, pb = MC.loss_longdouble(Z, Y, MC.SCALE, w, ds)
        psi, phi = ref._rows(x)
        assert abs(float(np.longdouble(ref.f(x)) - f)) <= fb
        assert np.all(np.abs((psi.astype(np.longdouble) - wpsi).astype(np.float64)) <= pb)
        if case.factors == "zero" or case.box:
            continue   # (no certificate: an unpenalised column / a box)
        vals, bounds, extra = MC.gap_longdouble(A, Y, x, lam, MC.SCALE, l2, w, Pf)
        assert float(vals["rows_gap"]) >= 0 and float(vals["gap"]) >= 0 and np.all(extra["terms"] >= 0)
        assert float(vals["dual"]) <= float(vals["primal"]), "D <= P"
        # the two forms of the gap are one number: P - D = rows (+ ridge) + columns
        assert abs(float(extra["gap_pd"] - vals["gap"])) <= 1e-15 * max(1.0, abs(float(vals["primal"])))
        if Pf is None:
            got = MC.gap_numpy(ref, x)
            ratios = MC.worst_ratio(got, vals, bounds)
            assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("K", [2, 5, 16])
def test_the_rows_gap_is_zero_at_alpha_one_and_positive_below(K):
    A, Y, lam = MC.make(50, 20, K, 40 + K)
    lam_max = float(np.max(np.abs(A.T @ (1.0 / K - Y))))
    x = np.zeros(20 * K)
    vals, bounds, extra = MC.gap_longdouble(A, Y, x, 1.5 * lam_max)
    assert vals["alpha"] == 1 and vals["rows_gap"] == 0 and bounds["rows_gap"] == 0 and vals["gap"] == 0
    got = MC.gap_numpy(MC.MultinomialRef(A, Y, 1.5 * lam_max), x)
    assert got["rows_gap"] == 0.0 and got["alpha"] == 1.0
    vals, _, extra = MC.gap_longdouble(A, Y, x, 0.5 * lam_max)
    assert 0 < vals["alpha"] < 1 and vals["rows_gap"] > 0 and np.all(extra["terms"] >= 0)
    # p underflowed to 0 where y > 0: the row term stays finite
    big = np.zeros((20, K))
    big[0, 0] = 800.0
    A2 = np.zeros((50, 20))
    A2[:, 0] = 1.0
    Y2 = MC.one_hot(np.ones(50, int), K)
    vals, bounds, _ = MC.gap_longdouble(A2, Y2, big, 1.0)
    assert np.isfinite(float(vals["rows_gap"])) and np.isfinite(float(vals["dual"])) and np.isfinite(bounds["rows_gap"])
    got = MC.gap_numpy(MC.MultinomialRef(A2, Y2, 1.0), big.reshape(-1))
    assert np.isfinite(got["rows_gap"]) and np.isfinite(got["dual"]) and got["rows_gap"] > 0


@pytest.mark.parametrize("K", [2, 3, 8, 16])
def test_the_gradient_passes_a_finite_difference_check(K):
    m, n = 30, 12
    A, Y, lam = MC.make(m, n, K, 70 + K, labels="soft")
    w = MC.make_weights(m, 70 + K, "real")
    ref = MC.MultinomialRef(A, Y, lam, w=w)
    rng = np.random.default_rng(K)
    x = 0.2 * rng.standard_normal(n * K)
    g = ref.jac_f(x)
    for _ in range(5):
        v = rng.standard_normal(n * K)
        h = 1e-6
        fd = (ref.f(x + h * v) - ref.f(x - h * v)) / (2 * h)
        assert abs(fd - g @ v) <= 1e-7 * max(1.0, abs(g @ v))
    # the columns of the gradient sum to 0 across the classes (softmax and y both sum to 1 per row)
    assert np.max(np.abs(g.reshape(n, K).sum(axis=1))) <= 1e-12
    assert np.allclose(MC.KronRef(A, Y, lam, w=w).jac_f(x), g, rtol=0, atol=1e-13)


@pytest.mark.parametrize("ci", range(len(MC.GOLDEN_CASES)), ids=[c.id for c in MC.GOLDEN_CASES])
def test_the_oracle_reproduces_the_reference_fixture(ci, golden):
    """g20_multinomial.npz holds what the reference's solver returned on these closures (tests/golden/make_golden_multinomial.py)."""
    G, pre, case = golden("g20_multinomial.npz"), MC.golden_prefix(ci), MC.GOLDEN_CASES[ci]
    A, Y, lam, _, _, _ = case.data()
    assert float(G(f"{pre}.lam")) == lam and abs(float(G(f"{pre}.ysum")) - Y.sum()) <= 1e-12 * case.m
    r = _quiet(cpu_ref.minimize_proximal_gradient, *case.ref().callbacks(), case.x0(), return_all=True, **case.opts)
    assert r.nit == int(G(f"{pre}.nit")) == 60 and list(G(f"{pre}.kept")) == MC.GOLDEN_KEPT
    np.testing.assert_allclose(np.stack([r.allvecs[k][::MC.GOLDEN_STRIDE] for k in MC.GOLDEN_KEPT]), G(f"{pre}.vecs"), rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.x, G(f"{pre}.x"), rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.allfuns, G(f"{pre}.allfuns"), rtol=1e-12)
    assert np.array_equal(np.asarray(r.alllrs), G(f"{pre}.alllrs")) and np.array_equal(np.asarray(r.alltrials), G(f"{pre}.alltrials"))
    assert int(G(f"{pre}.alltrials").sum()) > 60, "the fixture backtracks"


def test_the_fixture_holds_numbers_only():
    import os

    from conftest import GOLDEN

    path = os.path.join(GOLDEN, "g20_multinomial.npz")
    assert os.path.getsize(path) < (1 << 20)
    with np.load(path, allow_pickle=False) as z:
        assert all(z[k].dtype.kind in "fiu" for k in z.files)
