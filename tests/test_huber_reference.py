"""CPU: the restatements of tests/huber_cases.py - the closures are the stated expressions; the long-double certificate is
P - D, obeys weak duality, has a rows part of exactly 0 at alpha = 1 and reproduces the least-squares certificate when nothing
is clipped; the clipped share of every case; the exact screening rule never discards a column that is non-zero at a
high-accuracy optimum; the guard's candidate line holds for a row whose perturbation crosses delta."""
import numpy as np
import pytest

import gap_cases as GC
import huber_cases as H
import screen_cases as SC

ALL = H.SMALL + [H.TALL]
_id = lambda c: f"{c[0]}x{c[1]}"
_CASES = {}


def _case(case):
    """(A, b, lam, delta, {k: x_k of fixed-step FISTA}) - one run per case, shared and left unchanged."""
    if case not in _CASES:
        A, b, lam, delta = H.make_huber(case)
        x, kept = H.fista(A, b, lam, delta, np.zeros(A.shape[1]), 400, record=(20, 80, 400))
        kept[0] = np.zeros(A.shape[1])
        _CASES[case] = (A, b, lam, delta, kept)
    return _CASES[case]


def test_the_closures_are_the_stated_expressions():
    A, b, lam, delta = H.make_huber(H.SMALL[2])
    rng = np.random.default_rng(0)
    x = 0.1 * rng.standard_normal(A.shape[1])
    r = A @ x - b
    textbook = np.where(np.abs(r) <= delta, 0.5 * r * r, delta * (np.abs(r) - 0.5 * delta))
    for storage in H.FORMS:
        ref = H.HuberRef(H.matrix(A, storage), b, lam, delta)
        assert abs(ref.f(x) - textbook.sum()) <= 1e-13 * textbook.sum(), "scale 1/2 is the textbook Huber function"
        np.testing.assert_allclose(ref.jac_f(x), A.T @ np.clip(r, -delta, delta), rtol=1e-12, atol=1e-13)
        # the gradient is the derivative (central differences on a few coordinates)
        g = ref.jac_f(x)
        for j in rng.choice(A.shape[1], 5, replace=False):
            e = np.zeros_like(x)
            e[j] = 1e-6
            assert abs((ref.f(x + e) - ref.f(x - e)) / 2e-6 - g[j]) <= 1e-5 * max(1.0, abs(g[j]))
    c, Hv = H.huber_terms(r, delta)
    assert np.array_equal(c, np.clip(r, -delta, delta)) and (Hv >= 0).all()
    inside = np.abs(r) <= delta
    assert inside.any() and (~inside).any() and np.array_equal(Hv[inside], r[inside] * r[inside]), "an unclipped row gives r r"
    # |r| = delta exactly, signed zeros, a NaN
    edge = np.array([delta, -delta, 0.0, -0.0, np.nan, np.inf, -np.inf])
    with np.errstate(invalid="ignore"):
        ce, He = H.huber_terms(edge, delta)
    assert np.array_equal(ce[:2], [delta, -delta]) and np.array_equal(He[:2], [delta * delta] * 2)
    assert np.array_equal(np.signbit(ce[2:4]), [False, True]) and np.array_equal(He[2:4], [0.0, 0.0])
    assert np.isnan(He[4]) and He[5] == np.inf and He[6] == np.inf and np.array_equal(ce[5:], [delta, -delta])


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_both_branches_of_the_loss_run_in_every_case(case):
    """The share of clipped rows lies in [0.05, 0.95] at x0 = 0 and at iteration 80 of fixed-step FISTA."""
    A, b, lam, delta, xs = _case(case)
    shares = [H.clipped_share(A, b, xs[k], delta) for k in (0, 80)]
    print(_id(case), "clipped share at x0 and x_80:", shares)
    assert all(H.SHARE[0] <= s <= H.SHARE[1] for s in shares), shares
    assert H.SHARE == (0.05, 0.95)


@pytest.mark.parametrize("fac", [0.0, 1.0])
@pytest.mark.parametrize("case", ALL, ids=_id)
def test_restatement_gap_is_p_minus_d_and_weak_duality_holds(case, fac):
    A, b, lam, delta, xs = _case(case)
    l2 = fac * lam
    ks = sorted(xs)
    out = {k: H.gap_longdouble(A, b, xs[k], lam, delta, l2=l2) for k in ks}
    # (the iterates are those of the l1 problem: P of the last one still bounds min P from above for either penalty)
    P_end = min(float(o[0]["primal"]) for o in out.values())
    for k in ks:
        vals, bounds, extra = out[k]
        assert abs(float(vals["gap"] - extra["gap_pd"])) <= 4e-15 * max(abs(float(vals["primal"])), 1.0), "gap = P - D"
        assert vals["gap"] >= 0 and vals["rows_gap"] >= 0 and extra["cols"] >= -1e-18 and (extra["terms"] >= 0).all()
        assert vals["dual"] <= P_end * (1 + 1e-15), "weak duality: D(x) <= P at any point"
        assert all(np.isfinite(v) and v >= 0 for v in bounds.values())
        assert set(vals) == set(H.KEYS10 if l2 > 0 else H.KEYS8)
        if k <= 80:   # (the condition on the inputs: later iterates of the wide 64 x 4099 case fit every row inside delta)
            assert 0.0 < extra["share"] < 1.0 and extra["T"] > 0
    if fac == 0.0:
        gaps = [float(out[k][0]["gap"]) for k in ks]
        assert gaps[0] > gaps[-1] > 0, gaps


def test_rows_part_is_exactly_zero_at_alpha_one():
    A, b, lam, delta, xs = _case(H.SMALL[0])
    big = 2.0 * H.lam_max(A, b, delta)
    vals, bounds, extra = H.gap_longdouble(A, b, np.zeros(A.shape[1]), big, delta)
    assert vals["alpha"] == 1 and vals["rows_gap"] == 0 and bounds["rows_gap"] == 0.0 and bounds["alpha"] == 0.0
    assert extra["T"] > 0, "clipped rows are there: the factor 1 - alpha = 0 removes them"
    assert vals["gap"] == 0 and vals["primal"] == vals["f"], "x = 0 is optimal at lam >= lam_max"
    assert abs(float(vals["primal"] - vals["dual"])) <= 1e-15 * float(vals["primal"])


@pytest.mark.parametrize("case", [H.SMALL[0], H.SMALL[2]], ids=_id)
def test_a_delta_beyond_every_residual_reproduces_the_least_squares_certificate(case):
    A, b, lam, delta, xs = _case(case)
    for k in (0, 20, 400):
        x = xs[k]
        wide = 2.0 * float(np.max(np.abs(A @ x - b)))
        v0, b0, e0 = GC.gap_longdouble(A, b, x, lam, H.SCALE, False)
        v1, b1, e1 = H.gap_longdouble(A, b, x, lam, wide)
        assert e1["T"] == 0 and e1["share"] == 0.0
        for key in GC.KEYS:
            assert abs(float(v0[key] - v1[key])) <= 8 * 2.0 ** -63 * abs(float(v0[key])), key
            assert 0.5 * b0[key] <= b1[key] <= 2 * b0[key] + 16 * H.U * abs(float(v0[key])), key


def test_the_screening_rule_never_discards_a_column_of_the_optimum():
    """Three restarts of 500 FISTA iterations on the 1000 x 257 case certify themselves to a gap below 1e-12 P: the support
    is the optimum's to that accuracy, and the exact rule at x_0, x_20, x_400 and at that point keeps every column of it.
    (The 300 x 1000 case is too ill-conditioned for a fixed step: its gap is still 0.3 P after 3000 iterations.)"""
    A, b, lam, delta, xs = _case(H.SMALL[2])
    x = np.zeros(A.shape[1])
    for _ in range(3):
        x, _kept = H.fista(A, b, lam, delta, x, 500)
    best = H.screen_longdouble(A, b, x, lam, delta)
    assert float(best["vals"]["gap"]) <= 1e-12 * float(best["vals"]["primal"])
    support = np.flatnonzero(x)
    assert 0 < support.size < A.shape[1] // 4
    dropped = []
    for point in (xs[0], xs[20], xs[400], x):
        sc = H.screen_longdouble(A, b, point, lam, delta)
        assert not sc["discard"][support].any()
        assert np.isfinite(sc["E"]) and 0 < sc["E"] <= 2.0 ** -19 * float(sc["radius"]) + 1e-7, "2^-20 r and a rounding-size rest"
        dropped.append(int(sc["discard"].sum()))
    print("columns discarded at x_0, x_20, x_400 and the optimum:", dropped)
    assert dropped[-1] > dropped[0] and dropped[-1] >= A.shape[1] // 2
    assert dropped[-1] + support.size <= A.shape[1]
    # the radius is the least-squares one: L = 2 scale
    assert SC.lipschitz(H.SCALE, False) == 2 * H.SCALE


def test_the_guards_candidate_line_holds_across_delta():
    """dc_i <= dz_i + u |c_i| for rows whose rounding or margin error crosses delta: r within a few ulps of +-delta."""
    delta = 0.7368421052631579
    rng = np.random.default_rng(5)
    ld = np.longdouble
    b = rng.standard_normal(4000)
    # exact margins z (longdouble) with r = z - b within 4 ulps of +-delta, and a device margin z^ within dz of z
    sign = rng.choice([-1.0, 1.0], b.size)
    r_exact = sign * ld(delta) * (1 + ld(2.0 ** -53) * rng.integers(-4, 5, b.size))
    z = r_exact + b.astype(ld)
    dz = np.abs(z).astype(np.float64) * 2.0 ** -52 * rng.random(b.size)
    z_dev = (z + dz * rng.choice([-1.0, 1.0], b.size)).astype(np.float64)
    r_dev = z_dev - b                                   # the device's subtraction, rounded
    c_dev, _ = H.huber_terms(r_dev, delta)
    c_exact, _ = H.huber_terms(r_exact, ld(delta))
    crossed = (np.abs(r_dev) > delta) != (np.abs(r_exact) > ld(delta))
    assert crossed.sum() > 100, "the rows must cross delta"
    dz_true = np.abs(z_dev.astype(ld) - z).astype(np.float64)
    err = np.abs(c_dev.astype(ld) - c_exact).astype(np.float64)
    assert (err <= dz_true + H.U * np.abs(c_dev) * (1 + 2.0 ** -50)).all()
    # and in norm, the line of the guard
    assert np.linalg.norm(err) <= np.linalg.norm(dz_true) + H.U * np.linalg.norm(c_dev) * (1 + 2.0 ** -50)
