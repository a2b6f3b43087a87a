"""CPU: the oracle on the Poisson closures (tests/poisson_cases.py) replays the committed fixture G18 (outputs of the REFERENCE
solver, tests/golden/make_golden_poisson.py)."""
import os
import warnings

import numpy as np
import pytest

import poisson_cases as PC
from conftest import GOLDEN
from oracle import cpu_ref

SOLVES = [(ci, fi, st, tag) for ci in range(len(PC.SMALL)) for fi, st, tag in PC.GOLDEN_SOLVES]


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


@pytest.mark.parametrize("ci,fi,storage,tag", SOLVES)
def test_g18_poisson(golden, ci, fi, storage, tag):
    G = golden("g18_poisson.npz")
    A, b, lam = PC.make_poisson(*PC.SMALL[ci])
    assert lam == float(G(f"poisson.c{ci}.lam")) and A.nnz == int(G(f"poisson.c{ci}.nnz")) and b.sum() == float(G(f"poisson.c{ci}.bsum"))
    ref = PC.PoissonRef(PC.matrix(A, storage), b, lam, l2=fi * lam)
    r = _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), np.zeros(A.shape[1]), **PC.GOLDEN_KW, **PC.GOLDEN_VARIANTS[tag])
    pre = PC.golden_prefix(ci, fi, storage, tag)
    assert r.nit == int(G(f"{pre}.nit")) == 80
    np.testing.assert_allclose(np.stack([r.allvecs[k][::PC.GOLDEN_STRIDE] for k in G(f"{pre}.kept")]), G(f"{pre}.vecs"), rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.x, G(f"{pre}.x"), rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.allfuns, G(f"{pre}.allfuns"), rtol=1e-12)
    assert np.array_equal(np.asarray(r.alllrs), G(f"{pre}.alllrs"))
    assert np.array_equal(np.asarray(r.alltrials), G(f"{pre}.alltrials"))
    assert int(G(f"{pre}.alltrials")[0]) >= 9, "the line search backtracks from lr = 1 (2000 x 5000: out of an overflowing trial)"
    if fi == 0:   # the other storage form took the same trial sequence (no knife edge of the line search)
        other = PC.golden_prefix(ci, fi, "dense" if storage == "csr" else "csr", tag)
        assert np.array_equal(G(f"{pre}.alltrials"), G(f"{other}.alltrials")) and np.array_equal(G(f"{pre}.alllrs"), G(f"{other}.alllrs"))


def test_the_fixture_is_below_the_size_limit_and_holds_numbers_only():
    path = os.path.join(GOLDEN, "g18_poisson.npz")
    assert os.path.getsize(path) < (1 << 20)
    with np.load(path, allow_pickle=False) as z:
        assert all(z[k].dtype.kind in "fiu" for k in z.files)
