"""CPU: the tables of tests/sparse_multiresponse_cases.py are what they claim.  The plan and the row contents of
sp.kron(A, I_K) are those of A per response, for A and for A^T, on every matrix the GPU file uses (the claim the exact comparisons
rest on); the shapes reach all five lane widths in both sweeps and split rows in both; every case decides every trial alike under
two CPU evaluations; the endings end as their tags say; ALL_K holds one solve per loss and per K = 2 .. 16."""
import contextlib
import io
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import sparse_cases as S
import sparse_multiresponse_cases as SM
from oracle import cpu_ref


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with contextlib.redirect_stdout(io.StringIO()):
            return fn(*a, **k)


def test_the_constants_restate_the_library():
    from zfista_amd import problems, sparse

    assert SM.THRESHOLD == sparse.SPLIT_THRESHOLD and SM.LANES == (4, 8, 16, 32, 64)
    assert (sparse.MIN_LANES, sparse.MAX_LANES) == (4, 64) and max(SM.KS + SM.SOLVE_KS) == problems.MAX_RESPONSES == 16
    rng = np.random.default_rng(0)
    for _ in range(50):
        lengths = rng.integers(0, int(rng.integers(2, 300)), int(rng.integers(1, 40)))
        A = SM.rows_matrix(lengths, 300, int(rng.integers(1 << 30)))
        assert SM.lanes_of(A) == sparse.lanes_for(lengths)


@pytest.mark.parametrize("K", SM.KS)
def test_the_kronecker_matrix_has_the_plan_and_the_rows_of_a_per_response(K):
    """Every K = 2 .. 16 on every matrix the GPU file uses - SMALL, TALL, the hand-built sweep matrices and SHAPES (the whole
    parametrisation takes ten seconds); `many-split` (1.2e6 elements) at the K the GPU file sweeps it with."""
    seen, split_A, split_At = set(), 0, 0
    mats = [(f"small{i}", S.make_sparse(*c)[0]) for i, c in enumerate(S.SMALL)]
    mats.append(("tall", S.make_sparse(*S.TALL)[0]))
    mats += [(n, A) for n, A in SM.sweep_matrices() if n != "many-split" or K in SM.MANY_SPLIT_KS]
    mats += [(s, SM.make("square", s, K, 1)[0]) for s in SM.SHAPES]
    for name, A in mats:
        (la, sa), (lt, st) = SM.plan_claim(A, K)
        seen |= {("A", la), ("At", lt)}
        split_A, split_At = split_A + (sa if name != "many-split" else 0), split_At + st
        if name in SM.SHAPES:
            assert (la, lt) == SM.SHAPE_LANES[name], (name, la, lt)
        if name.startswith("edges-L") and not name.endswith("-T"):
            assert la == int(name[7:]), (name, la)
        if name == "threshold":
            assert sa == 1, "the row of exactly `threshold` elements is not split"
        if name == "many-split":
            assert sa == 300
        if name == "tall":
            assert st >= 1 and np.diff(sp.csr_matrix(A.T).indptr).max() == 39999
    assert seen == {(d, L) for d in ("A", "At") for L in SM.LANES}, "all five lane widths occur in both sweeps"
    assert split_A >= 3 and split_At >= 1
    lens = [np.diff(S.make_sparse(*c)[0].indptr).max() for c in (S.SMALL[1], S.SMALL[3])]
    assert all(l > SM.THRESHOLD for l in lens), "a split row in A for the 2000 x 5000 and 64 x 4099 cases"


def test_the_edge_rows_hit_every_remainder_of_a_lane():
    for L in SM.LANES:
        lengths = SM.edge_lengths(L)
        assert {0, 1, L - 1, L, L + 1, 2 * L, 2 * L + 1, 4 * L, 4 * L + 1, 4 * L + 3} <= set(lengths)
        assert L <= sum(lengths) / len(lengths) < 2 * L


def test_the_tables_cover_what_they_name():
    ks = {c.K for c in SM.CASES}
    assert ks == set(SM.SOLVE_KS) and SM.KS == tuple(range(2, 17)) and set(SM.MANY_SPLIT_KS) == {2, 4, 7, 16}
    # ALL_K: 30 cases, K = 2 .. 16 under both losses, the shape by K % 4 and the extras by K % 3, seeds 600 + K / 700 + K (a replaced one:
    # + 100, at most one in four, counted in REPLACED)
    assert len(SM.ALL_K) == 30
    for loss, s0 in (("square", 600), ("logistic", 700)):
        mine = [c for c in SM.ALL_K if c.loss == loss]
        assert [c.K for c in mine] == list(range(2, 17))
        assert {c.seed - s0 - c.K for c in mine} <= {0, 100} and sum(c.seed != s0 + c.K for c in mine) <= len(mine) // 4
        for c in mine:
            assert c.shape == "abcd"[c.K % 4] and c.opts["max_iter"] == 30 and c.box is None and not c.l2fac
            assert (c.weights, c.factors) == ((None, None), ("real", None), (None, "pos"))[c.K % 3]
    assert sum(c.seed not in (600 + c.K, 700 + c.K) for c in SM.ALL_K) <= SM.REPLACED
    for loss in ("square", "logistic"):
        mine = [c for c in SM.CASES if c.loss == loss]
        assert {c.weights for c in mine} == {None, "real", "mask"} and {c.factors for c in mine} == {None, "pos", "zero"}
        assert any(c.l2fac for c in mine) and any(c.box for c in mine)
        assert {c.shape for c in mine} == set(SM.SHAPES)
        tags = [c.tag for c in SM.ENDINGS if c.loss == loss]
        assert sorted(tags) == sorted(["tol", "fail0", "one", "failk"] * 2)
    assert len({c.id for c in SM.CASES + SM.ENDINGS + SM.ALL_K}) == len(SM.CASES) + len(SM.ENDINGS) + len(SM.ALL_K)
    assert all(SM.CASES[i].K in (2, 9, 16) for i in SM.SNAPSHOT_CASES)
    A, B, lam = SM.make_tall()
    assert A.shape[0] * SM.TALL_K > 32768 and B.shape == (A.shape[0], SM.TALL_K) and lam > 0


@pytest.mark.parametrize("table", ["CASES", "ENDINGS", "ALL_K"])
def test_two_cpu_evaluations_decide_every_trial_alike(table):
    worst = 0.0
    for case in getattr(SM, table):
        a = _quiet(cpu_ref.minimize_proximal_gradient, *SM.kron_ref(case).callbacks(), case.x0(), return_all=True, **case.opts)
        b = _quiet(cpu_ref.minimize_proximal_gradient, *SM.second_ref(case).callbacks(), case.x0(), return_all=True, **case.opts)
        assert a.nit == b.nit and a.message == b.message, case.id
        assert list(a.alltrials) == list(b.alltrials) and list(a.alllrs) == list(b.alllrs), case.id
        size = max(1.0, max(float(np.max(np.abs(v))) for v in a.allvecs))
        dev = max(float(np.max(np.abs(np.asarray(u) - np.asarray(v)))) for u, v in zip(a.allvecs, b.allvecs)) / size
        worst = max(worst, dev)
        if table == "ALL_K":
            print(f"{case.id}: nit {a.nit}, trials {int(np.sum(a.alltrials))}, deviation {dev:.2e}")
        if case.tag == "tol":
            assert a.success and 1 < a.nit < case.opts["max_iter"]
        elif case.tag == "fail0":
            assert "Backtracking failed" in a.message and a.nit == 0
        elif case.tag == "failk":
            assert "Backtracking failed" in a.message and a.nit >= 2 and int(np.sum(a.alltrials)) == a.nit
        elif case.tag == "one":
            assert a.nit == 1
        elif case.tag == "allk":
            assert a.nit == 30 and int(np.sum(a.alltrials)) > a.nit, (case.id, "the case must reject trials")
        else:
            assert a.nit == 60 and int(np.sum(a.alltrials)) > a.nit, "the case must reject trials"
    print(f"{table}: the two evaluations part by at most {worst:.2e} of the iterates' size")
    assert worst <= 1e-10   # (the tolerance of the GPU comparison against this oracle)
