"""GPU: the soft-threshold of the device code, element by element and bit by bit, on data crafted so that its
argument u hits the edges of the function: +-tau, tau +- 1..3 ulp, +-0, subnormals, 1e+-300, +-inf.

The expected value is the reference expression sign(u) * maximum(|u| - tau, 0) (oracle.problems_ref.soft_threshold)
with the sign of u on a zero result - copysign(maximum(|u| - tau, 0), u), what jaxopt's prox_lasso and the library's
general form compute - compared as uint64 views, so that signed zeros count.  Three ways into the device code:

* the device prox (problem.prox_wsum_g: the general form, zf_soft_threshold);
* ONE accepted DiagQuadL1 iteration through the fused trial kernels (zf_soft_threshold_nn, three instructions), with
  solvers of chain length 1 and 16: x0 = c = u and d = 1 give r = y - c = 0, grad = 0 and v = y - lr * 0 = y exactly, so
  the iterate the solve returns is prox(y) and nothing else; y = u without momentum and y = u + beta * (u - u) with it
  (:534) - u again, but for u = -0, which the addition of beta * (+0) turns into +0 in the reference as on the device;
* whole chains of 16, 10 and 10 + 10 accepted iterations (the full-chain and the mid-chain kernels) with d = 1, lr = 1:
  v = y - (y - c) lands on c or an ulp or two beside it in every trial, and c is drawn from the edge list around tau -
  against the CPU oracle's iterate.

No case is skipped.  +-inf cannot reach the threshold of an iteration as a number (y = +-inf makes r, grad or v a NaN in
the reference as well), so the iteration's +-inf case is an x0 that holds them, accepted with decay_rate = 1 (:298):
the NaN must come out in those elements exactly as the oracle's, the finite elements bit for bit."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def expected(u, tau):
    from oracle.problems_ref import soft_threshold

    with np.errstate(invalid="ignore", over="ignore"):
        ref = soft_threshold(u, tau)
        out = np.copysign(np.maximum(np.abs(u) - tau, 0), u)
    ok = ~np.isnan(ref)
    assert np.array_equal(out[ok], ref[ok]) and np.array_equal(np.isnan(out), np.isnan(ref))   # value-equal to the oracle's
    return out


def first_y(u, nesterov):
    """y of the first iteration from x0 = x_prev = u (proximal_gradient.py:534): u, or u + beta * (u - u)."""
    if not nesterov:
        return u
    with np.errstate(invalid="ignore"):
        return u + 0.25 * (u - u)   # (any finite beta >= 0 gives the same bits: beta * (+0) = +0)


def ulps(x, k):
    y = np.float64(x)
    for _ in range(abs(k)):
        y = np.nextafter(y, np.inf if k > 0 else -np.inf)
    return y


def edge_list(tau, huge=True, inf=False):
    tiny = 5e-324
    mags = [0.0, tiny, 7 * tiny, 2.2250738585072009e-308, 2.2250738585072014e-308, 1e-300, tau / 2, 2 * tau, 1.0, 3.5]
    mags += [ulps(tau, k) for k in range(-3, 4)]
    if huge:
        mags += [1e300]
    if inf:
        mags += [np.inf]
    u = np.array(mags, dtype=np.float64)
    return np.concatenate([u, -u])


def spread(edges, n, seed):
    """n elements: the edge list first, then seeded draws from it mixed with ordinary numbers around tau."""
    rng = np.random.default_rng(seed)
    rest = n - edges.size
    pick = rng.choice(edges, rest)
    plain = rng.standard_normal(rest)
    return np.concatenate([edges, np.where(rng.random(rest) < 0.7, pick, plain)])


TAUS = [0.045, 1.0, 0.1 * 0.45]   # (0.1 * 0.45: lam * lr of the benchmark, as the device multiplies it)


@pytest.mark.parametrize("tau", TAUS)
def test_device_prox_bits(tau):
    from zfista_amd.problems import DiagQuadL1

    n = 5001
    u = spread(edge_list(tau, inf=True), n, seed=11)
    prob = DiagQuadL1(np.ones(n), np.zeros(n), 1.0)
    out = prob.prox_wsum_g(tau, u)
    exp = expected(u, np.float64(tau))
    bad = np.flatnonzero(bits(out) != bits(exp))
    assert bad.size == 0, [(u[i].hex(), out[i].hex(), exp[i].hex()) for i in bad[:5]]


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("sub_iters", [1, 16])
@pytest.mark.parametrize("tau", TAUS)
def test_one_accepted_iteration_bits(tau, sub_iters, nesterov):
    """decay_rate = 0.5: the trial goes through the real acceptance test (f(x+) = |dx|^2 / 2 against the model's
    |dx|^2 / (2 lr) = |dx|^2 at lr = 1/2: accepted with room to spare, no rounding knife-edge)."""
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.problems import DiagQuadL1

    n = 5001
    u = spread(edge_list(tau, huge=False), n, seed=12)
    lr, lam = 0.5, 2.0 * tau   # lam * lr == tau exactly
    assert lam * lr == tau
    prob = DiagQuadL1(np.ones(n), u.copy(), lam)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = minimize_proximal_gradient(*prob.callbacks(), u.copy(), lr=lr, tol=0.0, max_iter=1, decay_rate=0.5,
                                         nesterov=nesterov, sub_iters=sub_iters)
    assert res.nit == 1
    exp = expected(first_y(u, nesterov), np.float64(tau))
    bad = np.flatnonzero(bits(res.x) != bits(exp))
    assert bad.size == 0, [(u[i].hex(), res.x[i].hex(), exp[i].hex()) for i in bad[:5]]


@pytest.mark.parametrize("sub_iters", [1, 16])
@pytest.mark.parametrize("special", ["1e300", "inf"])
def test_one_accepted_iteration_huge_and_inf(special, sub_iters):
    """1e300 among the data makes F of the size 1e299, where the acceptance test resolves nothing; +-inf makes it NaN.
    decay_rate = 1 accepts the trial whatever its sums (:298), in the reference as on the device: x+ is committed and
    compared - the finite elements as uint64 against the expression, all of them against the oracle's solve."""
    from oracle import cpu_ref, problems_ref as P
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.problems import DiagQuadL1

    tau, n = 0.045, 5001
    u = spread(edge_list(tau, huge=True, inf=(special == "inf")), n, seed=13)
    lr, lam = 0.5, 2.0 * tau
    c = np.where(np.isinf(u), 0.0, u)   # (c = +-inf would be a NaN in the data; x0 = +-inf is the case)
    kw = dict(lr=lr, tol=0.0, max_iter=1, decay_rate=1.0, nesterov=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with np.errstate(invalid="ignore", over="ignore"):
            ref = cpu_ref.minimize_proximal_gradient(*P.DiagQuadL1Ref(np.ones(n), c, lam).callbacks(), u.copy(), **kw)
        res = minimize_proximal_gradient(*DiagQuadL1(np.ones(n), c, lam).callbacks(), u.copy(), sub_iters=sub_iters, **kw)
    assert res.nit == ref.nit == 1
    fin = np.isfinite(u)
    exp = expected(first_y(u[fin], True), np.float64(tau))
    bad = np.flatnonzero(bits(res.x[fin]) != bits(exp))
    assert bad.size == 0, [(u[fin][i].hex(), res.x[fin][i].hex(), exp[i].hex()) for i in bad[:5]]
    # the elements that started at +-inf: inf - inf = NaN in r, hence in v and in x+ - kept, as the oracle keeps it
    assert np.array_equal(np.isnan(res.x), np.isnan(ref.x))
    assert np.isnan(res.x[~fin]).all() or special != "inf"
    assert np.array_equal(res.x[fin], ref.x[fin])


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("iters", [16, 10, 20, 1, 37])
def test_chains_on_the_threshold_against_the_oracle(iters, nesterov):
    """d = 1, lr = 1: v = y - (y - c) is c or an ulp or two beside it in EVERY trial of the chain, c drawn from the
    edge list around tau: the full chain (16), a mid chain (10), two of them (20), the short bodies (1) and a run of
    passes (37) threshold on the edges trial after trial.  decay_rate = 1: every trial is accepted, as in the oracle."""
    from oracle import cpu_ref, problems_ref as P
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.problems import DiagQuadL1

    tau, n = 0.045, 6145
    c = spread(edge_list(tau, huge=False), n, seed=14 + iters)
    rng = np.random.default_rng(99)
    x0 = np.where(rng.random(n) < 0.5, c, rng.standard_normal(n))
    kw = dict(lr=1.0, tol=0.0, max_iter=iters, decay_rate=1.0, nesterov=nesterov)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = cpu_ref.minimize_proximal_gradient(*P.DiagQuadL1Ref(np.ones(n), c, tau).callbacks(), x0.copy(), **kw)
        res = minimize_proximal_gradient(*DiagQuadL1(np.ones(n), c, tau).callbacks(), x0.copy(), sub_iters=16, **kw)
        res1 = minimize_proximal_gradient(*DiagQuadL1(np.ones(n), c, tau).callbacks(), x0.copy(), sub_iters=1, **kw)
    assert res.nit == res1.nit == ref.nit == iters
    assert np.array_equal(bits(res.x), bits(res1.x)), "chains of 16 and single trials: the same bits"
    assert np.array_equal(res.x, ref.x)
    # signed zeros: the oracle's sign(u) * 0 is +0 for u = +-0 and carries the sign of u otherwise; the device carries the
    # sign of u always - they may differ only where the result is a zero AND u was a zero; every nonzero bit pattern agrees
    nz = ref.x != 0
    assert np.array_equal(bits(res.x[nz]), bits(ref.x[nz]))
    assert (np.flatnonzero(ref.x == 0).size > 0) and (np.flatnonzero(nz).size > 0)
