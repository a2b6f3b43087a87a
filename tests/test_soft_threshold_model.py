"""CPU: NumPy models of the device soft-threshold forms (csrc/zf_common.h), compared as uint64 views.

    general   copysign(|u| - tau < 0 ? 0 : |u| - tau, u)                     zf_soft_threshold
    four      copysign(u - min(max(u, -tau), tau), u)                        zf_soft_threshold_nn, rounds 2 to 5
    three     copysign(|u| - min(|u|, tau), u)                               zf_soft_threshold_nn, now
    max_form  copysign(max(|u| - tau, 0), u)                                 the three-instruction form that loses a NaN

The device's v_min_f64 / v_max_f64 return the other operand when one is NaN: np.fmin / np.fmax.  All forms must give
the same 64 bits for every u and every tau >= 0 (NaN results: NaN in all of them, except max_form - which is why it
is not the one in the library), and be value-equal to the reference expression sign(u) * maximum(|u| - tau, 0)."""
import numpy as np
import pytest


def general(u, tau):
    a = np.abs(u) - tau
    return np.copysign(np.where(a < 0, 0.0, a), u)


def four(u, tau):
    return np.copysign(u - np.fmin(np.fmax(u, -tau), tau), u)


def three(u, tau):
    return np.copysign(np.abs(u) - np.fmin(np.abs(u), tau), u)


def max_form(u, tau):
    return np.copysign(np.fmax(np.abs(u) - tau, 0.0), u)


def reference(u, tau):   # oracle/problems_ref.py: soft_threshold
    return np.sign(u) * np.maximum(np.abs(u) - tau, 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ulps(x, ks):
    """x moved by k ulp for every k in ks (towards +inf for k > 0)."""
    out = []
    for k in ks:
        y = np.float64(x)
        for _ in range(abs(k)):
            y = np.nextafter(y, np.inf if k > 0 else -np.inf)
        out.append(y)
    return out


TAUS = [0.0, 5e-324, 2.2250738585072014e-308, 1e-300, 0.045, 0.1, 1.0, 3.0, 1e300, np.inf]


def edge_u(tau):
    tiny, big = 5e-324, np.finfo(float).max
    mags = [0.0, tiny, 3 * tiny, 2.2250738585072009e-308, 2.2250738585072014e-308, 1e-300, 1e300, big, np.inf]
    if np.isfinite(tau):
        mags += [m for m in ulps(tau, range(-3, 4)) if m >= 0]
        mags += [2 * tau, tau / 2]
    u = np.array(mags, dtype=np.float64)
    return np.concatenate([u, -u])


def check_all_forms(u, tau):
    with np.errstate(invalid="ignore", over="ignore"):
        g, f4, f3, fm, ref = general(u, tau), four(u, tau), three(u, tau), max_form(u, tau), reference(u, tau)
    nan = np.isnan(g)
    # NaN results (u = NaN; u = +-inf with tau = inf): NaN in the general form, the old form and the new one alike
    assert np.array_equal(np.isnan(f4), nan) and np.array_equal(np.isnan(f3), nan)
    ok = ~nan
    assert np.array_equal(bits(f3[ok]), bits(g[ok])), "three-instruction form vs general form"
    assert np.array_equal(bits(f3[ok]), bits(f4[ok])), "three-instruction form vs four-instruction form"
    assert np.array_equal(bits(fm[ok]), bits(g[ok])), "max form vs general form (non-NaN)"
    assert np.array_equal(f3[ok], ref[ok]), "value-equal to the reference expression (signed zeros compare equal)"
    # the sign of u is on every result, zeros included
    assert np.array_equal(np.signbit(f3[ok]), np.signbit(u[ok]))


@pytest.mark.parametrize("tau", TAUS)
def test_edge_list(tau):
    check_all_forms(edge_u(tau), np.float64(tau))


def test_nan_is_kept_by_the_library_form_and_lost_by_the_max_form():
    u = np.array([np.nan, -np.nan, np.inf, -np.inf])
    with np.errstate(invalid="ignore"):
        assert np.isnan(three(u[:2], 0.5)).all() and np.isnan(four(u[:2], 0.5)).all() and np.isnan(general(u[:2], 0.5)).all()
        assert np.isnan(three(u[2:], np.inf)).all() and np.isnan(four(u[2:], np.inf)).all() and np.isnan(general(u[2:], np.inf)).all()
        assert not np.isnan(max_form(u, np.inf)).any() and not np.isnan(max_form(u[:2], 0.5)).any()


@pytest.mark.parametrize("seed", range(4))
def test_seeded_random_sweep(seed):
    rng = np.random.default_rng(600 + seed)
    n = 500_000
    # magnitudes over the whole exponent range, both signs; tau likewise (and the two of the benchmark / the tests)
    for tau in (0.045, 1.0, float(10 ** rng.uniform(-300, 300)), float(10 ** rng.uniform(-3, 3)), 0.0):
        u = 10.0 ** rng.uniform(-300, 300, n) * rng.choice([-1.0, 1.0], n)
        check_all_forms(u, np.float64(tau))
        # |u| within +-3 ulp of tau, and the same exponent as tau
        if tau > 0:
            k = rng.integers(-3, 4, n)
            near = (bits(np.full(n, tau)).astype(np.int64) + k).astype(np.uint64).view(np.float64) * rng.choice([-1.0, 1.0], n)
            check_all_forms(near, np.float64(tau))
            check_all_forms(tau * rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n), np.float64(tau))
    # raw bit patterns: every class of double, subnormals and NaNs included, against a random non-negative tau each
    raw = rng.integers(0, 2**64, n, dtype=np.uint64).view(np.float64)
    tau = np.abs(rng.integers(0, 2**63, n, dtype=np.uint64).view(np.float64))
    keep = ~np.isnan(tau)
    check_all_forms(raw[keep], tau[keep])
