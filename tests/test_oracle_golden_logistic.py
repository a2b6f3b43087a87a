"""CPU: the oracle on the logistic closures (tests/logistic_cases.py) against the committed fixture G15 (outputs of the
REFERENCE solver, tests/golden/make_golden_logistic.py); the two evaluation forms - the stable expressions the device
kernels use, and np.logaddexp / scipy.special.expit summed in reverse order - against each other: the inputs must not sit
on a knife edge of the line search; and the stable form at margins where the naive one overflows."""
import warnings

import numpy as np
import pytest

import logistic_cases as L
from oracle import cpu_ref


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


@pytest.mark.parametrize("tag", list(L.GOLDEN_VARIANTS))
@pytest.mark.parametrize("storage", L.GOLDEN_FORMS)
@pytest.mark.parametrize("ci", L.GOLDEN_CASES)
def test_g15_logistic_l1(golden, ci, storage, tag):
    G = golden("g15_logistic_l1.npz")
    m, n, density, seed = L.SMALL[ci]
    A, b, lam = L.make_logistic(m, n, density, seed)
    assert lam == float(G(f"c{ci}.lam")) and A.nnz == int(G(f"c{ci}.nnz")) and np.count_nonzero(b == 1) == int(G(f"c{ci}.positives"))
    assert set(np.unique(b)) == {-1.0, 1.0}
    r = _quiet(cpu_ref.minimize_proximal_gradient, *L.LogisticL1Ref(L.golden_matrix(A, storage), b, lam).callbacks(), np.zeros(n),
               **L.GOLDEN_KW, **L.GOLDEN_VARIANTS[tag])
    pre = f"c{ci}.{storage}.{tag}"
    assert r.nit == int(G(f"{pre}.nit")) == 80
    # same expressions -> equal; the tolerance only guards another BLAS / libm behind the matrix products and exp / log1p
    np.testing.assert_allclose(np.stack([r.allvecs[k][::L.GOLDEN_STRIDE] for k in G(f"{pre}.kept")]), G(f"{pre}.vecs"),
                               rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.x, G(f"{pre}.x"), rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.allfuns, G(f"{pre}.allfuns"), rtol=1e-12)
    assert np.array_equal(np.asarray(r.alllrs), G(f"{pre}.alllrs"))
    assert np.array_equal(np.asarray(r.alltrials), G(f"{pre}.alltrials"))
    assert 5 <= int(np.sum(G(f"{pre}.alltrials"))) - 80 <= 9, "the line search should backtrack 5 - 9 times from lr = 1"


@pytest.mark.parametrize("nest", [False, True], ids=["ista", "fista"])
@pytest.mark.parametrize("case", L.SMALL, ids=lambda c: f"{c[0]}x{c[1]}")
def test_two_evaluation_forms_take_the_same_decisions(case, nest):
    """Stable form on CSR, stable form on the dense matrix, library form (reverse-order sum) on both: identical trial and lr
    sequences, iterates within 3e-15 (norm-relative) of each other."""
    A, b, lam = L.make_logistic(*case)
    n = A.shape[1]
    kw = dict(lr=1, tol=0.0, max_iter=80, nesterov=nest, return_all=True)
    runs = [_quiet(cpu_ref.minimize_proximal_gradient, *L.LogisticL1Ref(L.golden_matrix(A, st), b, lam, form=form).callbacks(),
                   np.zeros(n), **kw) for st in L.GOLDEN_FORMS for form in ("stable", "library")]
    base = runs[0]
    assert base.nit == 80 and 5 <= sum(base.alltrials) - 80 <= 9
    for r in runs[1:]:
        assert np.array_equal(r.alltrials, base.alltrials) and np.array_equal(r.alllrs, base.alllrs)
        for a, e in zip(r.allvecs, base.allvecs):
            assert np.linalg.norm(a - e) <= 3e-15 * max(np.linalg.norm(e), 1.0)


def test_scale_one_over_m_does_not_backtrack():
    """Why the fixture uses scale = 1: with scale = 1 / m the step lr = 1 is accepted at once and the line search is idle."""
    m, n, density, seed = L.SMALL[0]
    A, b, lam = L.make_logistic(m, n, density, seed, scale=1.0 / m)
    r = _quiet(cpu_ref.minimize_proximal_gradient, *L.LogisticL1Ref(A, b, lam, scale=1.0 / m).callbacks(), np.zeros(n),
               lr=1, tol=0.0, max_iter=80, nesterov=True, return_all=True)
    assert sum(r.alltrials) == r.nit == 80


def test_stable_form_is_finite_where_the_naive_form_overflows():
    """Margins of +-750: exp(750) = inf in fp64.  The stable closures give softplus = max(t, 0) exactly, sigma in {0, 1},
    rho in {0, -+1}; log(1 + exp(t)) gives inf."""
    A = np.diag([750.0, 750.0, -750.0, -750.0, 0.0])
    b = np.array([1.0, -1.0, 1.0, -1.0, 1.0])
    x = np.ones(5)
    ref = L.LogisticL1Ref(A, b, 0.1)
    t = -b * (A @ x)
    assert np.array_equal(t, [-750.0, 750.0, 750.0, -750.0, 0.0])
    soft, sig = L.stable_terms(t)
    assert np.array_equal(soft, [0.0, 750.0, 750.0, 0.0, np.log(2.0)]) and np.array_equal(sig, [0.0, 1.0, 1.0, 0.0, 0.5])
    assert ref.f(x) == 1500.0 + np.log(2.0) and np.isfinite(ref.jac_f(x)).all()
    rho = -b * sig
    assert np.array_equal(rho, [-0.0, 1.0, -1.0, 0.0, -0.5])
    assert np.array_equal(ref.jac_f(x), A.T @ rho)
    with np.errstate(over="ignore"):
        assert np.isinf(np.sum(np.log(1.0 + np.exp(t))))
    # and the library form agrees with the stable one there
    lib = L.LogisticL1Ref(A, b, 0.1, form="library")
    assert lib.f(x) == ref.f(x) and np.array_equal(lib.jac_f(x), ref.jac_f(x))
