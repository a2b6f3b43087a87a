"""CPU: the case tables of the multi-response tests are honest (tests/multiresponse_cases.py).

Every case is solved by the reference solver twice - on the closures of the existing case modules over np.kron(A, I_K), and on the
per-response closures (A @ X, A.T @ R) - and both must decide every trial alike (the same nit, message, step and trial sequences)
and keep every iterate within 3e-15 of each other: the table then says nothing about summation orders, and a device that departs
from the oracle on it departs for a reason of its own.  The endings table holds every way a run ends three times per loss; ALL_K
holds one solve per loss and per K = 2 .. 16 (every K is a kernel instantiation of its own), each under both load widths."""
import contextlib
import io
import warnings

import numpy as np
import pytest

import multiresponse_cases as M
from oracle import cpu_ref


def _solve(ref, case):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with contextlib.redirect_stdout(io.StringIO()):
            return cpu_ref.minimize_proximal_gradient(*ref.callbacks(), case.x0(), return_all=True, **case.opts)


def _dev(a, b):
    return max((np.max(np.abs(np.asarray(u) - np.asarray(v))) / (np.max(np.abs(u)) or 1.0) for u, v in zip(a.allvecs, b.allvecs)),
               default=0.0)


_RES = {}


def _both(case):
    if case.id not in _RES:
        _RES[case.id] = (_solve(M.kron_ref(case), case), _solve(M.MRRef(case), case))
    return _RES[case.id]


@pytest.mark.parametrize("case", M.CASES + M.ENDINGS + M.TALL + M.ALL_K, ids=lambda c: c.id)
def test_the_two_evaluations_decide_alike_and_stay_together(case):
    a, b = _both(case)
    assert a.nit == b.nit and a.message == b.message and a.success == b.success
    assert list(a.alllrs) == list(b.alllrs) and list(a.alltrials) == list(b.alltrials), "the step and trial sequences, exactly"
    assert len(a.allvecs) == len(b.allvecs) and len(a.allfuns) == len(b.allfuns)
    dev = _dev(a, b)
    print(f"{case.id}: nit {a.nit}, deviation {dev:.2e}")
    assert dev <= M.ITER_TOL
    fa, fb = np.asarray(a.allfuns, float).reshape(-1), np.asarray(b.allfuns, float).reshape(-1)
    fin = np.isfinite(fa)
    assert np.array_equal(fin, np.isfinite(fb)) and np.allclose(fa[fin], fb[fin], rtol=1e-12, atol=0)


def test_ids_are_unique_and_the_kronecker_matrices_stay_small():
    ids = [c.id for c in M.CASES + M.ENDINGS + M.ALL_K]
    assert len(set(ids)) == len(ids)
    assert all(c.m * c.K > 32768 and c.m * c.K * c.n * c.K * 8 <= 64 << 20 and c.weights is None and c.loss == "square" for c in M.TALL)
    for c in M.CASES + M.ENDINGS + M.ALL_K:
        assert c.m * c.K <= 1200 and c.n * c.K <= 2100 and 2 <= c.K <= 16, c.id
    assert {c.K for c in M.CASES} == {2, 5, 9, 12, 16} and {c.loss for c in M.CASES} == {"square", "logistic"}
    assert all(0 <= i < len(M.CASES) for i in M.SNAPSHOT_CASES) and len(M.SNAPSHOT_CASES) == 4
    assert M.REPLACED >= 0


def test_all_k_holds_every_k_under_both_losses_and_both_load_widths():
    """ALL_K as the issue of this table fixes it: 30 cases, K = 2 .. 16 under both losses; one row into the second workgroup of the row
    sweep; each K with an odd n (V = 1) under one loss and an even n (V = 2) under the other; none / weights / factors by K % 3; every
    case rejects trials (the acceptance test is exercised); at most one seed in four replaced (by seed + 100, counted in REPLACED)."""
    assert len(M.ALL_K) == 30 and M.KS == tuple(range(2, 17))
    for loss, s0 in (("square", 600), ("logistic", 700)):
        mine = [c for c in M.ALL_K if c.loss == loss]
        assert [c.K for c in mine] == list(range(2, 17))
        assert {c.seed - s0 - c.K for c in mine} <= {0, 100} and sum(c.seed != s0 + c.K for c in mine) <= len(mine) // 4
        assert {c.n % 2 for c in mine} == {0, 1}
    for K in range(2, 17):
        sq, lg = (next(c for c in M.ALL_K if c.K == K and c.loss == loss) for loss in ("square", "logistic"))
        assert sq.m == lg.m == M.rows_per_wg(K) + 1 and sq.n == (67, 130)[(K // 2) % 2] and {sq.n, lg.n} == {67, 130}, "both column parities"
        for c in (sq, lg):
            assert (c.weights, c.factors) == ((None, None), ("real", None), (None, "pos"))[K % 3] and c.opts["max_iter"] == 30
            assert c.box is None and not c.l2fac, "a certificate exists for every case"
            a, _ = _both(c)
            assert a.nit == 30 and int(np.sum(a.alltrials)) > a.nit, (c.id, "the case must reject trials")


@pytest.mark.parametrize("loss", ["square", "logistic"])
def test_every_ending_occurs_three_times(loss):
    seen = dict(tol=0, fail0=0, failk=0, one=0, inf=0)
    for c in M.ENDINGS:
        if c.loss != loss:
            continue
        a, _ = _both(c)
        F0 = float(np.asarray(a.allfuns[0]).reshape(-1)[0])
        if c.tag == "tol":
            seen["tol"] += bool(a.success and a.nit < c.opts["max_iter"])
        elif c.tag == "fail0":
            seen["fail0"] += bool("Backtracking failed" in a.message and a.nit == 0)
        elif c.tag == "failk":
            seen["failk"] += bool("Backtracking failed" in a.message and 0 < a.nit < c.opts["max_iter"])
        elif c.tag == "one":
            seen["one"] += bool(a.nit == 1)
        elif c.tag == "inf":
            seen["inf"] += bool(np.isinf(F0) and a.nit > 0 and np.isfinite(float(np.asarray(a.allfuns[-1]).reshape(-1)[0])))
    assert all(v >= 3 for v in seen.values()), seen


def test_the_restated_launch_rules():
    assert [M.rows_per_wg(K) for K in (2, 8, 9, 12, 13, 16)] == [16, 16, 24, 24, 32, 32] and M.KS == tuple(range(2, 17))
    assert [M.rows_per_wg(K) for K in M.KS] == [16] * 7 + [24] * 4 + [32] * 4
    assert M.slices_of(100, 518) == (13, 8) and M.slices_of(17, 64) == (3, 6) and M.slices_of(1, 7) == (1, 1)
    for K in M.KS:
        shapes = M.sweep_shapes(K)
        assert {n % 4 for _, n in shapes} >= {0, 2} and any(n % 2 for _, n in shapes) and shapes[0][0] == 1
        assert shapes[-1][0] > 2048 * M.rows_per_wg(K)
