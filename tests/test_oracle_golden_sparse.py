"""CPU: the oracle on SciPy-sparse closures against the committed sparse-LASSO fixture (outputs of the REFERENCE solver,
tests/golden/make_golden_sparse.py), and the two summation orders - sparse closures, dense oracle class - against each
other: the inputs must not sit on a knife edge of the line search."""
import warnings

import numpy as np
import pytest

import sparse_cases as S
from oracle import cpu_ref, problems_ref as P


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


@pytest.mark.parametrize("tag", list(S.GOLDEN_VARIANTS))
@pytest.mark.parametrize("ci", S.GOLDEN_CASES)
def test_g14_sparse_lasso(golden, ci, tag):
    G = golden("g14_sparse_lasso.npz")
    m, n, density, seed = S.SMALL[ci]
    A, b, lam = S.make_sparse(m, n, density, seed)
    assert lam == float(G(f"c{ci}.lam")) and A.nnz == int(G(f"c{ci}.nnz"))
    r = _quiet(cpu_ref.minimize_proximal_gradient, *S.SparseLeastSquaresL1Ref(A, b, lam).callbacks(), np.zeros(n),
               **S.GOLDEN_KW, **S.GOLDEN_VARIANTS[tag])
    pre = f"c{ci}.{tag}"
    assert r.nit == int(G(f"{pre}.nit")) == 80
    # same expressions -> equal; the tolerance only guards another BLAS behind np.linalg.norm
    np.testing.assert_allclose(np.stack([r.allvecs[k][::S.GOLDEN_STRIDE] for k in G(f"{pre}.kept")]), G(f"{pre}.vecs"),
                               rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.x, G(f"{pre}.x"), rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.allfuns, G(f"{pre}.allfuns"), rtol=1e-12)
    assert np.array_equal(np.asarray(r.alllrs), G(f"{pre}.alllrs"))
    assert np.array_equal(np.asarray(r.alltrials), G(f"{pre}.alltrials"))
    assert 7 <= int(np.sum(G(f"{pre}.alltrials"))) - 80 <= 12, "the line search should backtrack from lr = 1"


@pytest.mark.parametrize("tag,nest,nit", [("ista", False, 4), ("fista", True, 5)])
def test_g14_matrix_without_stored_elements(golden, tag, nest, nit):
    G = golden("g14_sparse_lasso.npz")
    A, b, lam, scale, x0 = S.azero_problem()
    r = _quiet(cpu_ref.minimize_proximal_gradient, *S.SparseLeastSquaresL1Ref(A, b, lam, scale=scale).callbacks(), x0,
               return_all=True, nesterov=nest)
    assert r.nit == int(G(f"azero.{tag}.nit")) == nit and int(G(f"azero.{tag}.status")) == 1
    assert np.array_equal(r.x, [0.0]) and np.array_equal(G(f"azero.{tag}.x"), [0.0])
    np.testing.assert_allclose(r.allfuns, G(f"azero.{tag}.allfuns"), rtol=1e-12)
    np.testing.assert_allclose(r.allerrs, G(f"azero.{tag}.allerrs"), rtol=1e-12, atol=1e-16)


@pytest.mark.parametrize("case", S.SMALL + [S.TALL], ids=lambda c: f"{c[0]}x{c[1]}")
def test_sparse_and_dense_summation_orders_take_the_same_decisions(case):
    m, n, density, seed = case
    A, b, lam = S.make_sparse(m, n, density, seed)
    kw = dict(lr=1, tol=0.0, max_iter=80, nesterov=True, return_all=True)
    rs = _quiet(cpu_ref.minimize_proximal_gradient, *S.SparseLeastSquaresL1Ref(A, b, lam).callbacks(), np.zeros(n), **kw)
    rd = _quiet(cpu_ref.minimize_proximal_gradient, *P.LeastSquaresL1Ref(A.toarray(), b, lam).callbacks(), np.zeros(n), **kw)
    assert np.array_equal(rs.alltrials, rd.alltrials) and np.array_equal(rs.alllrs, rd.alllrs)
    for a, e in zip(rs.allvecs, rd.allvecs):
        assert np.linalg.norm(a - e) <= 1e-13 * max(np.linalg.norm(e), 1.0)
