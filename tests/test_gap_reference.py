"""CPU: the extended-precision restatement of the duality gap (tests/gap_cases.py) proved on its own - the two forms of the
gap agree, gap >= 0, gap = 0 at x = 0 for lam >= lam_max, and the dual value never exceeds the primal value of a tightly
converged oracle solution (weak duality)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import gap_cases as G
import logistic_cases as L
import sparse_cases as S
from oracle import cpu_ref


def _problem(logistic, case=0):
    if logistic:
        A, b, lam = L.make_logistic(*L.SMALL[case])
        return A, b, lam, 1.0
    A, b, lam = S.make_sparse(*S.SMALL[case])
    return A, b, lam, 0.5


def _points(n, seed):
    rng = np.random.default_rng(seed)
    dense = rng.standard_normal(n)
    sparse = dense * (rng.random(n) < 0.05)
    return [np.zeros(n), sparse, dense, 1e-3 * sparse]


@pytest.mark.parametrize("logistic", [False, True])
@pytest.mark.parametrize("case", [0, 2])
def test_the_two_forms_agree_and_the_gap_is_non_negative(logistic, case):
    A, b, lam0, scale = _problem(logistic, case)
    for x in _points(A.shape[1], case):
        G0 = float(G.gap_longdouble(A, b, x, 1.0, scale, logistic)[0]["grad_inf"])
        for lam in (0.1 * G0, 0.5 * G0, G0, 2.0 * G0, lam0):
            v, bd, ex = G.gap_longdouble(A, b, x, lam, scale, logistic)
            # P - D in longdouble loses eps_ld |P|; the Fenchel-Young sum does not
            assert abs(float(v["gap"] - ex["gap_pd"])) <= 1e-15 * (abs(float(v["primal"])) + abs(float(v["dual"]))) + 1e-300
            # (the reference's own rounding: 2^-64 of the terms of a sum, each formed from parts of the size of P at most)
            slack = 1e-17 * (1 + abs(float(v["primal"])))
            assert v["gap"] >= -slack and v["rows_gap"] >= -slack and ex["cols"] >= -slack
            assert 0 <= v["alpha"] <= 1
            assert np.all(np.abs(float(v["alpha"]) * ex["grad"].astype(float)) <= lam * (1 + 1e-15)), "the dual point must be feasible"
            assert all(np.isfinite(list(bd.values())))


@pytest.mark.parametrize("logistic", [False, True])
def test_gap_is_zero_at_the_origin_from_lam_max_on(logistic):
    A, b, _, scale = _problem(logistic)
    n = A.shape[1]
    lam_max = float(G.gap_longdouble(A, b, np.zeros(n), 1.0, scale, logistic)[0]["grad_inf"])
    if logistic:
        assert lam_max == pytest.approx(scale * np.max(np.abs(A.T @ (b / 2))), rel=1e-13)
    else:
        assert lam_max == pytest.approx(2 * scale * np.max(np.abs(A.T @ b)), rel=1e-13)
    for lam in (np.nextafter(lam_max, np.inf), 1.5 * lam_max):   # (lam_max itself was rounded to fp64: up, to stay >= the longdouble norm)
        v = G.gap_longdouble(A, b, np.zeros(n), lam, scale, logistic)[0]
        assert v["gap"] == 0 and v["alpha"] == 1 and v["rows_gap"] == 0 and v["primal"] == v["f"]
    v = G.gap_longdouble(A, b, np.zeros(n), 0.5 * lam_max, scale, logistic)[0]
    assert v["gap"] > 0 and v["alpha"] == pytest.approx(0.5, rel=1e-15)


@pytest.mark.parametrize("logistic", [False, True])
def test_weak_duality_against_a_converged_oracle_solution(logistic):
    """D(nu(x)) <= P(x*) for every x, and the gap at x* is small: x* from the CPU oracle (FISTA, tol 1e-12)."""
    rng = np.random.default_rng(5)
    m, n = 300, 120
    A = sp.csr_matrix(rng.standard_normal((m, n)))
    x_true = np.zeros(n)
    x_true[:10] = rng.standard_normal(10)
    if logistic:
        b = np.sign(A @ x_true + 0.1 * rng.standard_normal(m))
        b[b == 0] = 1.0
        scale = 1.0
        lam = 0.1 * scale * np.max(np.abs(A.T @ (b / 2)))
        ref = L.LogisticL1Ref(A, b, lam, scale)
    else:
        b = A @ x_true + 0.01 * rng.standard_normal(m)
        scale = 0.5
        lam = 0.1 * np.max(np.abs(A.T @ b))
        ref = S.SparseLeastSquaresL1Ref(A, b, lam, scale)
    gaps = {}
    for it in (5, 20, 80, 4000):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = cpu_ref.minimize_proximal_gradient(*ref.callbacks(), np.zeros(n), lr=1.0, nesterov=True, tol=1e-13, max_iter=it)
        gaps[it] = (res.x, G.gap_longdouble(A, b, res.x, lam, scale, logistic)[0])
    x_star, v_star = gaps[4000]
    P_star = v_star["primal"]
    assert 0 <= v_star["gap"] <= 1e-9 * float(P_star)
    seq = [float(gaps[it][1]["gap"]) for it in (5, 20, 80)]
    assert seq[0] > seq[1] > seq[2] >= 0
    for x in [gaps[it][0] for it in (5, 20, 80)] + _points(n, 3):
        for lam_other in (lam,):
            v = G.gap_longdouble(A, b, x, lam_other, scale, logistic)[0]
            assert v["dual"] <= P_star + 1e-16 * abs(float(P_star)), "weak duality"
            assert v["primal"] >= P_star - float(v_star["gap"]) - 1e-16 * abs(float(P_star))
            assert v["gap"] >= v["primal"] - P_star - 1e-16 * abs(float(P_star))
