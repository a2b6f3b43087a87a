"""CPU: the oracle on the elastic-net closures (tests/enet_cases.py) against the committed fixture G16 (outputs of the
REFERENCE solver, tests/golden/make_golden_enet.py); the two storage forms against each other; and the long-double
restatement of the elastic-net certificate - gap = P - D, its reduction to the l1 restatement at l2 = 0, weak duality."""
import warnings

import numpy as np
import pytest

import enet_cases as E
import gap_cases as GC
from oracle import cpu_ref


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


@pytest.mark.parametrize("tag", list(E.GOLDEN_VARIANTS))
@pytest.mark.parametrize("storage", E.FORMS)
@pytest.mark.parametrize("fi", range(len(E.L2_FACTORS)))
@pytest.mark.parametrize("ci", range(len(E.SMALL)))
@pytest.mark.parametrize("loss", E.LOSSES)
def test_g16_enet(golden, loss, ci, fi, storage, tag):
    G = golden("g16_enet.npz")
    A, b, lam, scale = E.make_case(loss, E.SMALL[ci])
    assert lam == float(G(f"{loss}.c{ci}.lam")) and A.nnz == int(G(f"{loss}.c{ci}.nnz"))
    ref = E.EnetRef(loss, E.matrix(A, storage), b, lam, E.L2_FACTORS[fi] * lam, scale)
    r = _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), np.zeros(A.shape[1]), **E.GOLDEN_KW, **E.GOLDEN_VARIANTS[tag])
    pre = E.golden_prefix(loss, ci, fi, storage, tag)
    assert r.nit == int(G(f"{pre}.nit")) == 80
    np.testing.assert_allclose(np.stack([r.allvecs[k][::E.GOLDEN_STRIDE] for k in G(f"{pre}.kept")]), G(f"{pre}.vecs"), rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.x, G(f"{pre}.x"), rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.allfuns, G(f"{pre}.allfuns"), rtol=1e-12)
    assert np.array_equal(np.asarray(r.alllrs), G(f"{pre}.alllrs"))
    assert np.array_equal(np.asarray(r.alltrials), G(f"{pre}.alltrials"))
    assert int(np.sum(G(f"{pre}.alltrials"))) > 80, "the line search should backtrack from lr = 1"
    # the other storage form took the same trial sequence (the inputs do not sit on a knife edge of the line search)
    other = E.golden_prefix(loss, ci, fi, "dense" if storage == "csr" else "csr", tag)
    assert np.array_equal(G(f"{pre}.alltrials"), G(f"{other}.alltrials")) and np.array_equal(G(f"{pre}.alllrs"), G(f"{other}.alllrs"))


def test_the_closures_are_the_stated_expressions():
    A, b, lam, scale = E.make_case("ls", E.SMALL[0])
    ref = E.EnetRef("ls", A, b, lam, 0.3)
    rng = np.random.default_rng(0)
    v = rng.standard_normal(A.shape[1])
    w = 0.37
    from oracle import problems_ref as P

    assert np.array_equal(ref.prox_wsum_g(w, v), P.soft_threshold(v, lam * w) * (1.0 / (1.0 + 0.3 * w)))
    boxed = E.EnetRef("ls", A, b, lam, 0.3, bounds=(-0.1, 0.2))
    assert np.array_equal(boxed.prox_wsum_g(w, v), P.clip_box(P.soft_threshold(v, lam * w) * (1.0 / (1.0 + 0.3 * w)), -0.1, 0.2))
    assert boxed.g(np.full(A.shape[1], 0.3)) == np.inf
    assert abs(ref.g(v) - float(E.g_longdouble(v, lam, 0.3))) <= 1e-13 * ref.g(v)
    # the prox is the minimiser: a perturbation of any sign never lowers w g(p) + |p - v|^2 / 2, inside the box too
    for r in (ref, boxed):
        p = r.prox_wsum_g(w, v)
        obj = lambda q: w * r.g(q) + 0.5 * np.sum((q - v) ** 2)
        for _ in range(20):
            q = p + 1e-3 * rng.standard_normal(p.size)
            if r.bounds is not None:
                q = np.clip(q, *r.bounds)
            assert obj(q) >= obj(p) - 1e-12


_SOLVES = {}


def _iterates(loss, fi):
    """x_0, x_20, x_400, x_3000 of FISTA (0, 1/4) on the 300 x 1000 case (one oracle run per loss and l2, shared)."""
    key = (loss, fi)
    if key not in _SOLVES:
        A, b, lam, scale = E.make_case(loss, E.SMALL[0])
        ref = E.EnetRef(loss, A, b, lam, E.L2_FACTORS[fi] * lam, scale)
        r = _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), np.zeros(A.shape[1]), lr=1, tol=0.0, max_iter=3000, nesterov=True,
                   return_all=True)
        assert r.nit == 3000
        _SOLVES[key] = (A, b, lam, scale, [r.allvecs[k] for k in (0, 20, 400, 3000)])
    return _SOLVES[key]


@pytest.mark.parametrize("fi", range(len(E.L2_FACTORS)))
@pytest.mark.parametrize("loss", E.LOSSES)
def test_restatement_gap_is_p_minus_d_and_weak_duality_holds(loss, fi):
    A, b, lam, scale, xs = _iterates(loss, fi)
    l2 = E.L2_FACTORS[fi] * lam
    logistic = loss == "logit"
    out = [E.gap_longdouble(A, b, x, lam, l2, scale, logistic) for x in xs]
    P_end = out[3][0]["primal"]
    for x, (vals, bounds, extra) in zip(xs, out):
        assert abs(float(vals["gap"] - extra["gap_pd"])) <= 1e-15 * max(abs(float(vals["primal"])), 1.0), "gap = P - D"
        assert vals["gap"] >= 0 and vals["rows_gap"] >= 0 and vals["ridge_gap"] >= 0 and extra["cols"] >= -1e-18
        assert vals["dual"] <= P_end + 1e-15 * abs(float(P_end)), "weak duality: D(x) <= P(x_3000)"
        assert abs(float(vals["primal"] - E.primal_longdouble(A, b, x, lam, l2, scale, logistic))) <= 1e-16 * abs(float(vals["primal"]))
        assert all(np.isfinite(v) and v >= 0 for v in bounds.values())
    gaps = [float(o[0]["gap"]) for o in out]
    assert gaps[0] > gaps[1] > gaps[2] > gaps[3], gaps
    if fi == 0:   # l2 = lam: strongly convex enough for 3000 iterations to certify the optimum closely
        assert gaps[3] <= (1e-7 if logistic else 1e-11), gaps
    assert float(out[0][0]["g_l2"]) == 0.0 and float(out[3][0]["g_l2"]) > 0.0


@pytest.mark.parametrize("loss", E.LOSSES)
def test_restatement_reduces_to_the_l1_restatement_at_l2_zero(loss):
    A, b, lam, scale, xs = _iterates(loss, 0)
    for x in xs[:3]:
        v0, b0, e0 = GC.gap_longdouble(A, b, x, lam, scale, loss == "logit")
        v1, b1, e1 = E.gap_longdouble(A, b, x, lam, 0.0, scale, loss == "logit")
        for k in GC.KEYS:
            assert v0[k] == v1[k], k
            # (the roundings of gt and of the added sums widen a bound a little, never tighten it)
            assert b0[k] <= b1[k] <= 2 * b0[k] + 16 * E.U * abs(float(v0[k])), k
        assert v1["g_l2"] == 0 and v1["ridge_gap"] == 0 and e0["gap_pd"] == e1["gap_pd"]
