"""CPU: the oracle on the penalty-factor closures (tests/penalty_cases.py) replays the committed fixture G19 (outputs of the
REFERENCE solver, tests/golden/make_golden_penalty.py); the closures are the stated expressions - p = 1 is the unfactored closure
bit for bit, p = 0 leaves a coordinate unthresholded (NaN and +-inf kept), an intercept column keeps its coordinate; the factored
problem is the unfactored one on A diag(1 / p) in p o x; the long-double certificate is P - D and obeys weak duality.

zf_host_prox_pf_box and zf_host_pf_g take host pointers but compute on the device (as zf_host_prox_l1_box does): their bits
against NumPy on +-0, NaN, +-inf and p = 0 are checked in tests/test_gpu_penalty.py; their argument checks, which need no device,
in tests/test_penalty_host.py."""
import os
import warnings

import numpy as np
import pytest

import penalty_cases as PF
import sparse_cases as S
import weight_cases as W
from conftest import GOLDEN
from oracle import cpu_ref, problems_ref as P


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.mark.parametrize("loss,ci,storage,tag", PF.GOLDEN_SOLVES)
def test_g19_penalty(golden, loss, ci, storage, tag):
    G = golden("g19_penalty.npz")
    ref, A, b, lam = PF.golden_ref(loss, ci, storage)
    assert lam == float(G(f"penalty.{loss}.c{ci}.lam")) and A.nnz == int(G(f"penalty.{loss}.c{ci}.nnz"))
    assert ref.p.sum() == float(G(f"penalty.{loss}.c{ci}.psum")) and np.count_nonzero(ref.p == 0) == int(G(f"penalty.{loss}.c{ci}.pzeros")) > 0
    r = _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), np.zeros(A.shape[1]), **PF.GOLDEN_KW, **PF.GOLDEN_VARIANTS[tag])
    pre = PF.golden_prefix(loss, ci, storage, tag)
    assert r.nit == int(G(f"{pre}.nit")) == 80
    assert np.array_equal(np.stack([r.allvecs[k][::PF.GOLDEN_STRIDE] for k in G(f"{pre}.kept")]), G(f"{pre}.vecs"))
    assert np.array_equal(r.x, G(f"{pre}.x"))
    assert np.array_equal(np.asarray(r.allfuns, float), G(f"{pre}.allfuns")) and np.array_equal(np.asarray(r.allerrs, float), G(f"{pre}.allerrs"))
    assert np.array_equal(np.asarray(r.alllrs), G(f"{pre}.alllrs"))
    assert np.array_equal(np.asarray(r.alltrials), G(f"{pre}.alltrials"))
    # the unpenalised columns move, and the other storage form took the same trial sequence (no knife edge of the line search)
    assert np.count_nonzero(r.x[ref.p == 0]) > 0
    other = PF.golden_prefix(loss, ci, "dense" if storage == "csr" else "csr", tag)
    assert np.array_equal(G(f"{pre}.alltrials"), G(f"{other}.alltrials")) and np.array_equal(G(f"{pre}.alllrs"), G(f"{other}.alllrs"))


def test_the_fixture_is_below_the_size_limit_and_holds_numbers_only():
    path = os.path.join(GOLDEN, "g19_penalty.npz")
    assert os.path.getsize(path) < (1 << 20)
    with np.load(path, allow_pickle=False) as z:
        assert all(z[k].dtype.kind in "fiu" for k in z.files)


def test_factor_generators():
    for n, seed in ((1000, 1), (257, 3), (4099, 4)):
        real, pos = PF.make_factors(n, seed, "real"), PF.make_factors(n, seed, "positive")
        assert 0.05 <= np.mean(real == 0) <= 0.15 and np.all((real == 0) | ((real > 0.25) & (real < 4)))
        assert np.all((pos > 0.25) & (pos < 4)) and np.array_equal(pos[real != 0], real[real != 0])
        assert PF.make_factors(n, seed, "intercept").tolist() == [0.0] + [1.0] * (n - 1) and np.all(PF.make_factors(n, seed, "ones") == 1)


def test_the_closures_are_the_stated_expressions():
    rng = np.random.default_rng(0)
    n = 257
    v = 0.05 * rng.standard_normal(n)
    v[:9] = [0.0, -0.0, np.nan, np.inf, -np.inf, 1e-320, -1e-320, 1e300, -1e300]
    p = PF.make_factors(n, 3, "real")
    p[:9] = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0, 0.0, 1.0]
    for t in (0.37, 2.0 ** -20, 0.0):
        with np.errstate(invalid="ignore"):
            got = PF.prox_pf(v, t, p)
            # p = 1: the unfactored closure, bit for bit (t * 1 == t)
            one = PF.prox_pf(v, t, np.ones(n))
            want = P.soft_threshold(v, t)
        assert np.array_equal(_bits(one)[~np.isnan(want)], _bits(want)[~np.isnan(want)]) and np.array_equal(np.isnan(one), np.isnan(want))
        # p = 0: the coordinate is carried through - finite values exactly, +-inf kept, NaN kept
        z = p == 0
        fin = z & np.isfinite(v)
        assert np.array_equal(got[fin], v[fin]) and np.isnan(got[2]) and got[3] == np.inf and got[4] == -np.inf
        assert got[5] == 1e-320 and got[7] == 1e300
        # p > 0: the soft threshold at t p_j
        for j in np.flatnonzero(~z & np.isfinite(v)):
            assert got[j] == np.sign(v[j]) * max(abs(v[j]) - t * p[j], 0.0)
    box = (-0.02, 0.03)
    assert np.array_equal(PF.prox_pf(v[9:], 0.01, p[9:], box), np.clip(PF.prox_pf(v[9:], 0.01, p[9:]), *box))


@pytest.mark.parametrize("loss", PF.LOSSES)
def test_ones_is_the_unfactored_closure_and_the_intercept_is_not_thresholded(loss):
    case = S.SMALL[2]
    A, b, lam, delta = PF.make_problem(case, loss)
    n = A.shape[1]
    rng = np.random.default_rng(1)
    x = 0.05 * rng.standard_normal(n)
    ones = PF.PenaltyRef(A, b, lam, np.ones(n), loss, delta)
    if loss == "poisson":
        import poisson_cases as PC

        plain = PC.PoissonRef(A, b, lam)
    else:
        plain = W.WeightedRef(A, b, lam, np.ones(A.shape[0]), loss, delta)
    assert ones.f(x) == plain.f(x) and np.array_equal(ones.jac_f(x), plain.jac_f(x))
    assert np.array_equal(_bits(ones.prox_wsum_g(0.3, x)), _bits(plain.prox_wsum_g(0.3, x)))
    assert abs(ones.g(x) - plain.g(x)) <= 4 * n * PF.U * plain.g(x)
    # an intercept: a column of ones with p = 0 - whatever the weight, the coordinate is v_0 itself
    import scipy.sparse as sp

    A1 = sp.hstack([sp.csr_matrix(np.ones((A.shape[0], 1))), A], format="csr")
    icpt = PF.PenaltyRef(A1, b, lam, PF.make_factors(n + 1, 0, "intercept"), loss, delta)
    v = np.concatenate([[1e-9], x])
    for wgt in (1.0, 1e6):
        out = icpt.prox_wsum_g(wgt, v)
        assert out[0] == 1e-9 and np.array_equal(out[1:], P.soft_threshold(x, lam * wgt))
    assert icpt.g(v) == icpt.g(np.concatenate([[1e9], x])), "the intercept costs nothing"
    assert abs(icpt.g(v) - lam * np.sum(np.abs(x))) <= 4 * n * PF.U * icpt.g(v)


@pytest.mark.parametrize("loss", PF.LOSSES)
def test_the_factored_problem_is_the_unfactored_one_on_the_scaled_matrix(loss):
    """F(x; A, p) = F'(p o x; A diag(1 / p)) up to the roundings of the scaling, and the long-double certificate of the scaled
    problem is P - D >= 0 with P the factored primal."""
    case = S.SMALL[2]
    A, b, lam, delta = PF.make_problem(case, loss)
    m, n = A.shape
    p = PF.make_factors(n, case[3], "positive")
    rng = np.random.default_rng(2)
    x = 0.02 * rng.standard_normal(n) * (rng.random(n) < 0.3)
    ref = PF.PenaltyRef(A, b, lam, p, loss, delta)
    A1, x1 = PF.scaled(A, p, x)
    un = PF.PenaltyRef(A1, b, lam, np.ones(n), loss, delta)
    F, F1 = ref.f(x) + ref.g(x), un.f(x1) + un.g(x1)
    assert abs(F - F1) <= 1e-12 * abs(F)
    np.testing.assert_allclose(ref.jac_f(x) / p, un.jac_f(x1), rtol=1e-11, atol=1e-13)
    vals, bounds, extra = PF.gap_longdouble(A, b, p, x, lam, loss, delta)
    assert set(vals) == set(PF.KEYS8) == set(bounds)
    assert abs(float(vals["gap"] - extra["gap_pd"])) <= 1e-15 * max(1.0, abs(float(vals["primal"]))) and vals["gap"] >= 0
    Pl = PF.primal_longdouble(A, b, p, x, lam, loss, delta)
    assert abs(float(vals["primal"] - Pl)) <= 1e-13 * abs(float(Pl))
    assert float(vals["g_l1"]) == pytest.approx(float(ref.g(x)), rel=1e-13)
    # every bound is far smaller than what it guards, and widened by the stated factor
    assert bounds["gap"] <= 1e-9 * max(1.0, abs(float(vals["primal"]))) and PF.widen(m, n) > 1
