"""CPU: the oracle on the Huber closures (tests/huber_cases.py) replays the committed fixture G17 (outputs of the REFERENCE
solver, tests/golden/make_golden_huber.py), and the fixture's inputs exercise both branches of the loss."""
import os
import warnings

import numpy as np
import pytest

import huber_cases as H
from conftest import GOLDEN
from oracle import cpu_ref

SOLVES = [(ci, fi, st, tag) for ci in range(len(H.SMALL)) for fi, st, tag in H.GOLDEN_SOLVES]


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


@pytest.mark.parametrize("ci,fi,storage,tag", SOLVES)
def test_g17_huber(golden, ci, fi, storage, tag):
    G = golden("g17_huber.npz")
    A, b, lam, delta = H.make_huber(H.SMALL[ci])
    assert lam == float(G(f"huber.c{ci}.lam")) and delta == float(G(f"huber.c{ci}.delta")) and A.nnz == int(G(f"huber.c{ci}.nnz"))
    ref = H.HuberRef(H.matrix(A, storage), b, lam, delta, l2=fi * lam)
    r = _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), np.zeros(A.shape[1]), **H.GOLDEN_KW, **H.GOLDEN_VARIANTS[tag])
    pre = H.golden_prefix(ci, fi, storage, tag)
    assert r.nit == int(G(f"{pre}.nit")) == 80
    np.testing.assert_allclose(np.stack([r.allvecs[k][::H.GOLDEN_STRIDE] for k in G(f"{pre}.kept")]), G(f"{pre}.vecs"), rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.x, G(f"{pre}.x"), rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.allfuns, G(f"{pre}.allfuns"), rtol=1e-12)
    assert np.array_equal(np.asarray(r.alllrs), G(f"{pre}.alllrs"))
    assert np.array_equal(np.asarray(r.alltrials), G(f"{pre}.alltrials"))
    assert int(np.sum(G(f"{pre}.alltrials"))) > 80, "the line search should backtrack from lr = 1"
    # both branches of the loss run at both ends of the solve: the clipped share of the reference's iterates
    share = [H.clipped_share(A, b, r.allvecs[0], delta), H.clipped_share(A, b, r.allvecs[-1], delta)]
    assert share == G(f"{pre}.share").tolist()
    assert all(H.SHARE[0] <= s <= H.SHARE[1] for s in share), share
    if fi == 0:   # the other storage form took the same trial sequence (no knife edge of the line search)
        other = H.golden_prefix(ci, fi, "dense" if storage == "csr" else "csr", tag)
        assert np.array_equal(G(f"{pre}.alltrials"), G(f"{other}.alltrials")) and np.array_equal(G(f"{pre}.alllrs"), G(f"{other}.alllrs"))


def test_the_fixture_is_smaller_than_the_elastic_net_fixture():
    size = os.path.getsize(os.path.join(GOLDEN, "g17_huber.npz"))
    assert size < os.path.getsize(os.path.join(GOLDEN, "g16_enet.npz")) and size < (1 << 20)
