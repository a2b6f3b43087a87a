"""CPU: the case tables of the lifecycle tests are honest (tests/lifecycle_cases.py).

Every case is solved by the reference solver twice - on the project's reference closures and on their second evaluation (matrix
products in np.longdouble; the operator's correlation on the transposed image) - and both must decide every trial alike: the same
nit, message, step and trial sequences.  Every run backtracks and accepts and ends the way its table says; the snapshot points of
the resume tables land on the accepted counts they name; the shapes of the small-matrix table walk the loop structure of the rows
kernel's row dot as the table claims."""
import numpy as np
import pytest

import lifecycle_cases as LC

_SECOND = {}


def _both(case, **over):
    key = (case.id, tuple(sorted(over.items())))
    if key not in _SECOND:
        first = case.solve(case.ref(), **over) if over else case.oracle()
        _SECOND[key] = (first, case.solve(case.second(), **over))
    return _SECOND[key]


def _over(case):
    return dict(max_iter=LC.MAXITER_THEN) if case in LC.MAXITER else {}


@pytest.mark.parametrize("case", LC.ALL, ids=lambda c: c.id)
def test_the_two_evaluations_decide_alike(case):
    a, b = _both(case, **_over(case))
    print(f"{case.id}: nit {a.nit}, trials {sum(a.alltrials)}, first {list(a.alltrials[:3])}")
    assert a.nit == b.nit and a.message == b.message and a.success == b.success
    assert list(a.alllrs) == list(b.alllrs) and list(a.alltrials) == list(b.alltrials), "the step and trial sequences, exactly"
    for k, (u, v) in enumerate(zip(a.allvecs, b.allvecs)):
        assert np.max(np.abs(np.asarray(u) - np.asarray(v))) <= 1e-10 * max(np.max(np.abs(u)), 1e-300), k


def test_ids_are_unique_and_few_seeds_were_replaced():
    ids = [c.id for c in LC.ALL]
    assert len(set(ids)) == len(ids)
    assert 0 <= LC.REPLACED <= len(LC.ALL) // 10


@pytest.mark.parametrize("case", LC.RESUME_SMALL + LC.RESUME_OP, ids=lambda c: c.id)
def test_resume_cases_backtrack_accept_and_end_by_max_iter(case):
    exp = case.oracle()
    assert exp.nit == case.opts["max_iter"] and not exp.success, "tol = 0: the run ends by max_iter"
    assert exp.alltrials[0] >= 2 and sum(exp.alltrials) > exp.nit, "the first passes reject"
    assert sum(exp.alltrials) <= 300, "a few hundred passes at the most"
    if case.family == "small" and not case.tag:
        assert case.opts["lr"] == LC.LR_REJECT and exp.alltrials[0] >= 10
    # the snapshot points: inside the run, in order, and on the accepted count they name
    passes = [case.passes_at(p) for p in case.snap]
    assert passes == sorted(set(passes)) and 0 < passes[0] and passes[-1] < sum(exp.alltrials)
    for point, p in zip(case.snap, passes):
        nit, retry = case.nit_after(p)
        if point == "nit0":
            assert nit == 0 and retry, "between a rejected trial and its retry"
        elif point in ("nit1", "nit2"):
            assert nit == int(point[3]) and not retry
        else:
            assert 2 < nit < exp.nit


def test_the_resume_tables_cover_what_they_claim():
    S = [c for c in LC.RESUME_SMALL if not c.tag and len(c.snap) == 1]
    assert {c.shape for c in S} == {s for s, _, _ in LC.SMALL_SHAPES} and all(LC.small_path(*c.shape) for c in LC.RESUME_SMALL)
    assert len(S) == 8 * len(LC.SMALL_SHAPES)
    for shape, _, _ in LC.SMALL_SHAPES:
        mine = [c for c in S if c.shape == shape]
        combos = {(bool(c.opts["nesterov"]), c.box is not None, c.opts["acceptance"]) for c in mine}
        assert len(combos) == 8, "the full cross on every shape: FISTA / ISTA x box x acceptance"
        for nest in (True, False):   # FISTA reads A x_{k-1}: it - and ISTA - meets nit0, nit1, nit2 and mid on every shape
            assert {c.snap[0] for c in mine if c.opts["nesterov"] == nest} == {"nit0", "nit1", "nit2", "mid"}, (shape, nest)
    for point in ("nit0", "nit1", "nit2", "mid"):   # ... and every point meets every box x acceptance combination
        assert len({(c.box is not None, c.opts["acceptance"]) for c in S if c.snap == (point,)}) == 4
    # a small-eligible shape off the fused path: the host-driven sequence and a one-rank communicator, FISTA past nit = 2
    for tag in ("split", "comm"):
        mine = [c for c in LC.RESUME_SMALL if c.tag == tag]
        assert len(mine) == 3 and all(LC.small_path(*c.shape) for c in mine)
        assert any(c.opts["nesterov"] and c.nit_after(c.passes_at(c.snap[0]))[0] >= 2 for c in mine)
        assert all((c.env == {"ZF_FORCE_SPLIT": "1"}) == (tag == "split") for c in mine)
    for table in (LC.RESUME_SMALL, LC.RESUME_OP):
        assert {p for c in table for p in c.snap} >= {"nit0", "nit1", "nit2", "mid"}
    assert sum(len(c.snap) == 2 for c in LC.RESUME_SMALL) == 2, "a resume of a resumed solve, in both modes"
    stalled = [c for c in LC.RESUME_SMALL if c.tag == "stalled"]
    assert len(stalled) == 1 and stalled[0].opts["acceptance"] == "remainder" and stalled[0].snap == (144,)
    # the operator table: every image under FISTA and ISTA, each with the prox step fused and apart; one box
    for shape, _, _, _ in LC.OP_IMAGES:
        mine = [c for c in LC.RESUME_OP if c.shape == shape]
        assert {(c.opts["nesterov"], c.env["ZF_OP_FUSE_PROX"]) for c in mine} == {(n, f) for n in (True, False) for f in "01"}
        assert len({c.snap for c in mine}) >= 2
    assert any(c.box for c in LC.RESUME_OP)
    assert {c.tile_height for c in LC.RESUME_OP} == {8, 32}
    assert {c.shape[3] for c in LC.RESUME_OP} == {"separable", "general"}


def test_the_resume_tables_cover_every_saved_count():
    """Over each table the snapshots are taken at nit = 0, 1, 2 and in the middle of a run, one of them between a rejected trial
    and its retry (the trial sequences are the oracle's, which every device id is held to)."""
    for table in (LC.RESUME_SMALL, LC.RESUME_OP):
        saved = {c.nit_after(c.passes_at(p))[0] for c in table for p in c.snap}
        assert {0, 1, 2} <= saved and max(saved) >= 3, saved
        assert any(c.nit_after(c.passes_at(p))[1] for c in table for p in c.snap), "one snapshot between a rejected trial and its retry"


def test_the_stalled_case_is_past_where_the_reference_test_decides():
    """Problem "D" of tests/test_gpu_accept_remainder.py: under the reference's evaluation of the sufficient-decrease test the
    same solve departs from the cancellation-free one before the snapshot point - the snapshot lies in the regime the
    remainder mode exists for."""
    case = next(c for c in LC.RESUME_SMALL if c.tag == "stalled")
    rem = case.oracle()
    ref = case.solve(case.ref(), acceptance="reference")
    k = next((i for i, (a, b) in enumerate(zip(rem.alltrials, ref.alltrials)) if a != b), min(len(rem.alltrials), len(ref.alltrials)))
    assert (list(ref.alltrials) != list(rem.alltrials) or ref.nit != rem.nit) and sum(rem.alltrials[:k]) < case.passes_at(144)
    assert 100 < case.nit_after(144)[0] < rem.nit


def test_small_shapes_walk_the_row_dot_as_claimed():
    walk = {shape: LC.row_dot_walk(shape[1]) for shape, _, _ in LC.SMALL_SHAPES}
    w = walk[(1, 32)]
    assert all(w[l] == (0, 1) for l in range(16)) and all(w[l] == (0, 0) for l in range(16, 64))
    assert set(walk[(65, 128)].values()) == {(0, 1)} and 65 % 8 == 1
    w = walk[(200, 960)]
    assert all(w[l] == (1, 0) for l in range(32)) and all(w[l] == (0, 7) for l in range(32, 64))
    assert set(walk[(512, 1024)].values()) == {(1, 0)} == set(walk[(4096, 1024)].values())
    w = walk[(96, 1056)]
    assert all(w[l] == (1, 1) for l in range(16)) and all(w[l] == (1, 0) for l in range(16, 64))
    assert 4096 * 1024 == 1 << 22 and not LC.small_path(4097, 1024) and not LC.small_path(4096, 1056)
    # every pair of a row is taken exactly once
    for (m, n), lanes in walk.items():
        assert sum(8 * un + tail for un, tail in lanes.values()) == n // 2


@pytest.mark.parametrize("case", LC.RING, ids=lambda c: c.id)
def test_ring_cases_reject_and_end_by_tolerance_well_past_the_ring(case):
    exp = case.oracle()
    assert exp.success and exp.nit < case.opts["max_iter"], "ends by tol"
    assert sum(exp.alltrials) > exp.nit, "trials are rejected: a rejected iterate is overwritten by its retry"
    assert exp.nit >= 2 * 5, "the 5-slot ring wraps at least twice (the 4-slot one more often)"
    assert sum(exp.alltrials) <= 300


def test_the_ring_table_holds_every_family():
    fams = [f[0] for f in LC.RING_FAMILIES]
    assert fams == ["dense", "csr", "mr", "small", "enet", "pf", "diag", "op"]
    for fam in fams:
        mine = [c for c in LC.RING if c.family == fam]
        assert {c.opts["nesterov"] for c in mine} == {True, False}
        assert {c.box is not None for c in mine} == {False, True} and len(mine) == 4, "one row per family x nesterov x box"
    small = next(c for c in LC.RING if c.family == "small")
    dense = next(c for c in LC.RING if c.family == "dense")
    mr = next(c for c in LC.RING if c.family == "mr")
    assert LC.small_path(*small.shape) and not LC.small_path(*dense.shape) and dense.shape[1] % 2 == 0
    assert mr.n_features == 201 and mr.n_features % 64 and LC.RING_SLOTS == (None, 5, 1)
    assert next(c for c in LC.RING if c.family == "pf").data()["p"].min() == 0.0
    assert next(c for c in LC.RING if c.family == "enet").data()["l2"] > 0
    diag = next(c for c in LC.RING if c.family == "diag")
    assert diag.opts["acceptance"] == "resolved" and diag.opts["sub_iters"] == 1 and diag.shape == (10007,)


@pytest.mark.parametrize("case", LC.MAXITER, ids=lambda c: c.id)
def test_max_iter_cases_run_past_both_limits(case):
    a, _ = _both(case, max_iter=LC.MAXITER_THEN)
    assert a.nit == LC.MAXITER_THEN and not a.success
    head = case.solve(case.ref(), max_iter=LC.MAXITER_FIRST)
    assert head.nit == LC.MAXITER_FIRST and list(head.alllrs) == list(a.alllrs[:LC.MAXITER_FIRST])


@pytest.mark.parametrize("case", LC.CONVERGED, ids=lambda c: c.id)
def test_converged_cases_converge(case):
    exp = case.oracle()
    assert exp.success and 5 < exp.nit < case.opts["max_iter"]
