"""CPU: the tables of tests/sharded_ls_cases.py are sound.  The shape cases claim the plans the restated dispatch rule gives and
reach the forms, mixes and edges they were chosen for; every solve the GPU tests compare with the oracle - the 30 FISTA iterations
of each shape case, the 2 x 24 sweep cases, the thread-rank cases - is decided alike by two CPU evaluations that add in different
orders (LeastSquaresL1Ref, and ShardedLSRef with the rank-ordered sums of the case's own split), none has lost its run to the
stagnation cut, and the sweep holds every pair of levels and every situation it was laid out for.
tests/test_gpu_sharded_ls.py runs the same tables on the device and may therefore treat every mismatch as a finding about the
product."""
import collections
import itertools

import numpy as np
import pytest

import sharded_ls_cases as C
from oracle import cpu_ref, problems_ref as P

SWEEP_IDS = [C.spec_id(sp) for sp in C.SWEEP]


# -- the shape table ---------------------------------------------------------------------------------------------------------
def test_the_restated_rule_is_the_dense_suite_s_rule_for_one_rank():
    import test_gpu_dense_ls_paths as D

    for (m, n), _, env, plan, _ in D.CASES:
        if not env:
            assert C.dispatch(m, n, 1) == D.dispatch(m, n, {}) == plan, (m, n)
        if plan[0] == C.SMALL:   # the small form is never chosen when world > 1: the MFMA form takes its shapes (n % 32 == 0)
            assert C.dispatch(m, n, 2)[:2] == (C.MFMA, C.ROWS_V2) and C.dispatch(m, n, 2)[2:] == D.dispatch(m, n, {})[2:]


@pytest.mark.parametrize("case", C.SHAPE_CASES, ids=[c.name for c in C.SHAPE_CASES])
def test_shape_case_claims_the_plan_the_rule_gives(case):
    m, n = case.shape
    world = len(case.parts)
    assert world >= 2 and min(case.parts) >= 1 and sum(case.parts) == (n if case.layout == "columns" else m)
    blocks = C.block_shapes(case.shape, case.parts, case.layout)
    assert tuple(C.dispatch(mp, np_, world) for mp, np_ in blocks) == case.plans
    assert all(p[0] != C.SMALL and p[1] != C.ROWS_SMALL for p in case.plans)
    assert case.scale in (0.5, 1 / 6)


def test_shape_table_reaches_what_it_was_chosen_for():
    by = {c.name: c for c in C.SHAPE_CASES}
    for layout in ("columns", "rows"):
        cases = [c for c in C.SHAPE_CASES if c.layout == layout]
        assert len(cases) == 5
        assert {p[0] for c in cases for p in c.plans} == {C.MFMA, C.VALU2, C.VALU1}, layout     # every form that world > 1 has
        assert {p[1] for c in cases for p in c.plans} == {C.ROWS_V2, C.ROWS_V1}, layout
        assert any(1 in c.parts for c in cases), "a one-element rank"
        assert any(mp > C.ROW_SWEEP_LOOPS for c in cases for mp, _ in C.block_shapes(c.shape, c.parts, c.layout)), "a looping row sweep"
        assert {c.scale for c in cases} == {0.5, 1 / 6}
    assert len({p[0] for p in by["C1"].plans}) == 3, "three forms in one solve"
    assert len({p[0] for p in by["C2"].plans}) == 2 and by["C2"].shape[0] > C.ROW_SWEEP_LOOPS
    # C3: a rank's block alone would take the small form
    assert all(C.dispatch(mp, np_, 1)[0] == C.SMALL for mp, np_ in C.block_shapes(by["C3"].shape, by["C3"].parts, "columns"))
    assert all(p[0] == C.MFMA for p in by["C3"].plans)
    assert by["R3"].plans[0][2:] == (63, 24) and by["R3"].plans[1][2] == 2
    assert by["R2"].plans[0][2:] == (1, 1)
    # ranks of one row-sharded solve run different slice counts
    assert all(len({p[2] for p in c.plans}) > 1 for c in C.SHAPE_CASES if c.name in ("R2", "R3", "R4"))


@pytest.mark.parametrize("case", C.SHAPE_CASES, ids=[c.name for c in C.SHAPE_CASES])
def test_shape_case_solve_is_decision_stable(case):
    """The 30 FISTA iterations from lr = 1 that the GPU test compares with the oracle: the line search backtracks, and the two
    summation orders take the same decisions."""
    A, b, lam, _ = C.shape_data(case.shape)
    x0 = C.solve_x0(case)
    exp = C.shape_oracle(case.name)
    other = C.run_ref(C.ShardedLSRef(A, b, lam, C.bounds_of(case.parts), case.layout, scale=case.scale), x0, C.SOLVE_OPTIONS)
    assert exp.nit == 30 and exp.alltrials[0] > 1, "lr = 1 should be rejected at first"
    for k in ("nit", "success", "message", "status"):
        assert exp[k] == other[k], k
    assert list(exp.alllrs) == list(other.alllrs) and list(exp.alltrials) == list(other.alltrials)
    # (sums over up to 70001 rows: the two orders differ by more than the 3e-15 asked of the sweep's small shapes; 1e-12 is
    #  a hundredth of what the device has to meet)
    for u, v in zip(exp.allvecs, other.allvecs):
        assert np.linalg.norm(u - v) <= 1e-12 * max(np.linalg.norm(v), 1.0)
    # where F stagnates within the 30 iterations, the residues the acceptance test then compares (64 eps |F|) stay below a
    # quarter of tol_internal = 1e-12: the decisions do not depend on the summation order
    cut = C.stagnation_cut(exp)
    if cut is not None:
        assert max(abs(float(v)) for v in exp.allfuns[cut:]) <= 16, (cut, exp.allfuns[cut:])
    assert exp.alllrs[-1] >= C.accepted_lr(case.shape, case.scale) / 2, "lr has not collapsed: no rejection on rounding noise"


# -- the closures --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["columns", "rows"])
def test_sharded_closures_are_the_reference_closures_in_another_order(layout):
    A, b, lam = P.make_plasso(23, 37, seed=3, n_informative=5)
    splits = [0, 1, 20, 37] if layout == "columns" else [0, 9, 10, 23]
    rng = np.random.default_rng(0)
    for bounds in C.BOXES:
        ref = P.LeastSquaresL1Ref(A, b, lam, scale=1 / 6, bounds=bounds)
        sh = C.ShardedLSRef(A, b, lam, splits, layout, scale=1 / 6, bounds=bounds)
        x = rng.uniform(0.02, 0.07, 37) if bounds else rng.standard_normal(37)
        np.testing.assert_allclose(sh.f(x), ref.f(x), rtol=1e-13)
        np.testing.assert_allclose(sh.g(x), ref.g(x), rtol=1e-13)
        np.testing.assert_allclose(sh.jac_f(x), ref.jac_f(x), rtol=1e-12, atol=1e-12)
        assert np.array_equal(sh.prox_wsum_g(0.3, x), ref.prox_wsum_g(0.3, x))
        if bounds:
            x[0] = 0.9   # outside on the first shard only: inf + finite values = inf
            assert sh.g(x) == ref.g(x) == np.inf


# -- the sweep -----------------------------------------------------------------------------------------------------------------
def test_the_sweep_is_a_fixed_table_of_2_x_24_distinct_seeds():
    assert len(C.SWEEP) == 48
    for layout in ("columns", "rows"):
        seeds = C.SEEDS[layout]
        assert len(seeds) == len(set(seeds)) == 24
        assert all(s % 24 == i for i, s in enumerate(seeds)), "a replaced seed stays in its slot: i + 24 k"
        specs = [sp for sp in C.SWEEP if sp.layout == layout]
        assert [sp.shape for sp in specs] == [C.SWEEP_SHAPES[layout][i % 6] for i in range(24)]
        for sp in specs:
            total = sp.shape[1] if layout == "columns" else sp.shape[0]
            assert 2 <= sp.world <= min(5, total) and len(sp.parts) == sp.world and sum(sp.parts) == total and min(sp.parts) >= 1
            assert sp.options["max_backtrack_iter"] in (1, 2, 5, 100) and sp.options["decay_rate"] in (0.3, 0.5, 0.9, 1.0)
            assert 1e-4 <= sp.options["lr"] <= 1.0
    assert C.SWEEP_SHAPES["rows"][0] == (3, 1) and C.SWEEP_SHAPES["columns"][0] == (3, 4)
    assert C.SWEEP_SHAPES["rows"][1:] == C.SWEEP_SHAPES["columns"][1:]


def test_split_kinds_give_what_they_are_named_for():
    rng = np.random.default_rng(0)
    assert C.split_parts("even", 33, 4, rng) == (8, 8, 8, 9)
    assert C.split_parts("pm1", 33, 4, rng) == (9, 8, 8, 8)
    assert C.split_parts("one-first", 33, 4, rng) == (1, 11, 11, 10)
    assert C.split_parts("one-last", 33, 4, rng) == (11, 11, 10, 1)
    assert C.split_parts("one-first", 2, 2, rng) == (1, 1) and C.split_parts("random", 4, 4, rng) == (1, 1, 1, 1)
    for layout in ("columns", "rows"):
        specs = [sp for sp in C.SWEEP if sp.layout == layout]
        # a split more uneven than +-1, in the sweep as in the shape table
        assert sum(max(sp.parts) - min(sp.parts) > 1 for sp in specs) >= 8, layout
        assert any(sp.split_kind == "random" and max(sp.parts) > 3 * min(sp.parts) for sp in specs), layout


@pytest.mark.parametrize("layout", ["columns", "rows"])
def test_every_pair_of_levels_occurs(layout):
    """Every pair of levels of two different factors, per layout - but shape x split kind (30 pairs: 24 distinct ones), and a
    world beyond the dimension that is split."""
    specs = [sp for sp in C.SWEEP if sp.layout == layout]
    shapes = C.SWEEP_SHAPES[layout]
    factor = {
        "shape": ([sp.shape for sp in specs], shapes),
        "world": ([sp.world for sp in specs], list(C.WORLDS)),
        "split": ([sp.split_kind for sp in specs], list(C.SPLIT_KINDS)),
        "box": ([sp.bounds for sp in specs], list(C.BOXES)),
        "start": ([sp.start for sp in specs], list(C.STARTS)),
    }
    for (na, (va, la)), (nb, (vb, lb)) in itertools.combinations(factor.items(), 2):
        got = set(zip(va, vb))
        if (na, nb) == ("shape", "split"):
            assert len(got) == 24
            continue
        for u, v in itertools.product(la, lb):
            if (na, nb) == ("shape", "world") and v > (u[1] if layout == "columns" else u[0]):
                continue   # (3, 1) by rows with 4 or 5 ranks, (3, 4) by columns with 5
            assert (u, v) in got, (layout, na, u, nb, v)


@pytest.mark.parametrize("spec", C.SWEEP, ids=SWEEP_IDS)
def test_sweep_case_is_decision_stable_and_keeps_its_run(spec):
    A, b, lam, x0, o, exp = C.oracle(spec)
    assert exp is not None, "x0 is already at the resolution limit of the acceptance test: nothing left to run"
    assert C.sound(spec) is None
    if C.ending(exp) == "error":
        assert exp.message == "Error: " + cpu_ref.MSG_BACKTRACK and not exp.success and "status" not in exp
        if exp.nit == 0:
            assert np.array_equal(exp.x, x0)
    else:
        assert exp.nit >= 1
        assert o["max_iter"] == spec.options["max_iter"] or C.ending(exp) == "max_iter"   # (a cut run ends at the cut)
    assert len(exp.alllrs) == len(exp.alltrials) == exp.nit
    outside = C.ranks_outside(spec, x0)
    assert np.isfinite(exp.allfuns[0]) == (not outside), "F(x0) = inf exactly where x0 lies outside the box"
    if spec.start == "outside" and spec.bounds is not None:
        assert len(outside) == (1 if spec.layout == "columns" else spec.world), "columns: outside on exactly one rank's shard"
    if spec.start == "random" and spec.bounds is not None:
        assert not outside
    # the driver's bound on the number of steps holds for the oracle's own run
    assert sum(exp.alltrials) <= o["max_iter"] * o["max_backtrack_iter"]


def test_sweep_reaches_every_situation_three_times_per_layout():
    for layout in ("columns", "rows"):
        counts = collections.Counter()
        for sp in C.SWEEP:
            if sp.layout == layout:
                counts.update(C.situations(sp))
        print(layout, {k: counts[k] for k in C.SITUATIONS})
        for k in C.SITUATIONS:
            assert counts[k] >= 3, (layout, k, counts[k])
        specs = [sp for sp in C.SWEEP if sp.layout == layout]
        assert {sp.options["nesterov"] for sp in specs} == {False, True}
        assert {sp.options["decay_rate"] for sp in specs} == {0.3, 0.5, 0.9, 1.0}
        assert any(sp.options["deprecated"] for sp in specs)
        assert any(max(C.oracle(sp)[5].alltrials, default=0) > 1 for sp in specs), "a rejected trial"


# -- the thread-rank cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.THREAD_CASES, ids=[f"{c.layout}-{c.name}" for c in C.THREAD_CASES])
def test_thread_case_is_decision_stable(case):
    A, b, lam, x0 = C.thread_inputs(case)
    m, n = case.shape
    assert sum(case.parts) == (n if case.layout == "columns" else m) and max(m, n) <= 4096   # (the local group's capacity)
    exp = C.run_ref(P.LeastSquaresL1Ref(A, b, lam, scale=case.scale, bounds=case.bounds), x0, case.options)
    assert C.stagnation_cut(exp) is None
    other = C.run_ref(C.ShardedLSRef(A, b, lam, C.bounds_of(case.parts), case.layout, scale=case.scale, bounds=case.bounds), x0, case.options)
    assert C.disagreement(exp, other) is None and C.disagreement(other, exp) is None
    assert max(exp.alltrials) > 1, "lr = 1 backtracks"
    if case.name == "split":
        twin = C.SHAPE_BY_NAME["C1" if case.layout == "columns" else "R4"]
        assert (case.shape, case.parts) == (twin.shape, twin.parts)
    if case.name == "box-ista":
        X = np.stack(exp.allvecs[1:])
        assert not case.options["nesterov"] and np.count_nonzero((X == case.bounds[0]) | (X == case.bounds[1])) >= 30
        assert 1 in case.parts
    if case.name == "x0-tol":
        assert np.any(x0 != 0) and C.ending(exp) == "tol" and 1 < exp.nit < case.options["max_iter"]
    else:
        assert C.ending(exp) == "max_iter"


# -- what a sharded LeastSquaresL1 refuses before anything touches the device --------------------------------------------------
class _Group:
    """Stands in for a process group: the refusals below must come before the group, or the device, is looked at."""
    rank, world = 0, 2

    def all_gather_host(self, arr):   # pragma: no cover - never reached
        raise AssertionError("a refused problem must not exchange anything")


@pytest.mark.parametrize("shard", ["columns", "rows"])
def test_a_sharded_least_squares_problem_still_refuses_l2_weights_and_penalty_factors(shard):
    from zfista_amd.problems import LeastSquaresL1

    A, b, lam = P.make_plasso(6, 4, seed=0, n_informative=2)
    with pytest.raises(ValueError, match="l2 > 0 is not available with group="):
        LeastSquaresL1(A, b, lam, group=_Group(), shard=shard, l2=0.1)
    with pytest.raises(ValueError, match="sample_weight is not available with group="):
        LeastSquaresL1(A, b, lam, group=_Group(), shard=shard, sample_weight=np.ones(6))
    with pytest.raises(ValueError, match="penalty_factor is not available with group="):
        LeastSquaresL1(A, b, lam, group=_Group(), shard=shard, penalty_factor=np.ones(4))
    with pytest.raises(ValueError, match="shard must be"):
        LeastSquaresL1(A, b, lam, group=_Group(), shard="both")
