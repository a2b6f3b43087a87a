"""CPU: the case table of tests/f32_fuzz_cases.py is sound - every case meets the criteria of margins_fuzz_ext_cases.accepted,
unchanged, on A64 = float64(float32(A)) (decided alike by the closures over the CSR form of A64 and over the dense A64 with the
rows of (A64, b, w) reversed; a run left after the stagnation cut; every accepted F finite), the seeds are the first 48 per loss
that do, inside the replacement cap, and the table holds every load width of the fp32 sweeps with every loss, weights kind and
factor kind.  The restated ls_plan of the six shapes is proved against f32_cases.dispatch_f32.  tests/test_gpu_fuzz_f32.py runs the
same table on the fp32 device classes and may therefore treat every mismatch as a finding about the product."""
import collections
import itertools

import numpy as np
import pytest

import f32_cases as F
import f32_fuzz_cases as XF
import margins_fuzz_ext_cases as X
from oracle import cpu_ref

SPECS = [XF.draw(loss, seed) for loss, seed in XF.TABLE]
IDS = [f"{sp.loss}-s{sp.seed:02d}" for sp in SPECS]
KIND_NAMES = ("few_trials", "box", "to_tol", "short")
WIDTHS = (4, 2, 1)


def test_the_table_is_the_first_48_accepted_seeds_per_loss_inside_the_replacement_cap():
    assert XF.BLOCK == 48 and len(XF.TABLE) == 48 * len(XF.LOSSES) == len(set(XF.TABLE))
    for loss in XF.LOSSES:
        seeds, examined, replaced = XF.SEEDS[loss], XF.EXAMINED[loss], XF.REPLACED[loss]
        assert len(seeds) == len(set(seeds)) == XF.BLOCK and seeds == sorted(seeds), loss
        # the first BLOCK accepted seeds counted from 0: what was examined is 0 .. max, and what is missing was replaced
        assert examined == max(seeds) + 1 == len(seeds) + len(replaced) and sorted(set(range(examined)) - set(seeds)) == sorted(replaced)
        assert all(isinstance(why, str) and why for why in replaced.values()), "every replaced seed carries its reason"
        print(loss, "examined", examined, "replaced", len(replaced), replaced)
        assert 4 * len(replaced) <= examined, "at most one examined seed in four is replaced"


@pytest.mark.parametrize("loss", XF.LOSSES)
def test_a_replaced_seed_fails_on_the_cpu(loss):
    """A seed is replaced for failing the CPU criteria, and for nothing else; the recorded reason is of the kind found."""
    for seed, why in XF.REPLACED[loss].items():
        got = XF.accepted(XF.draw(loss, seed))
        assert got is not None, seed
        assert got.split(":")[0].split()[0] == why.split(":")[0].split()[0], (seed, got, why)


def test_the_shapes_are_the_ext_tables_with_two_swaps_and_hold_every_width():
    assert len(XF.SHAPES) == len(X.SHAPES) == 6
    differ = [i for i in range(6) if XF.SHAPES[i] != X.SHAPES[i]]
    assert differ == [2, 4]
    for i in differ:   # the same rows or columns but for the width, the same density and seed
        (m, n, d, s), (m0, n0, d0, s0) = XF.SHAPES[i], X.SHAPES[i]
        assert (d, s) == (d0, s0) and m == m0 and abs(n - n0) <= 2
    widths = collections.Counter(F.width(sh[1]) for sh in XF.SHAPES)
    assert widths == {4: 3, 2: 2, 1: 1}
    assert max(sh[0] for sh in XF.SHAPES) > 32768, "the many-workgroup shape of the loss kernels"
    # where the fp64 class would take the fused small-matrix form
    m, n = XF.SHAPES[3][:2]
    assert n % 32 == 0 and m <= 4096 and m * n <= 1 << 22


def test_the_restated_plans_are_dispatch_f32s():
    assert set(XF.PLANS) == {sh[:2] for sh in XF.SHAPES}
    for (m, n), plan in XF.PLANS.items():
        assert plan == F.dispatch_f32(m, n), (m, n)
        V = F.width(n)
        assert plan[:2] == {4: (F.COLS_V4, F.ROWS_V4), 2: (F.COLS_V2, F.ROWS_V2), 1: (F.COLS_V1, F.ROWS_V1)}[V]
        assert (plan[2] - 1) * plan[3] < m <= plan[2] * plan[3] and plan[2] <= 64
    assert XF.PLANS[40000, 500][2] == 64
    for sp in SPECS:
        assert XF.plan(sp) == F.dispatch_f32(*sp.shape[:2]) and XF.dense_form(sp) == XF.plan(sp)[0]


def test_a_case_is_the_ext_tables_but_for_the_matrix():
    """The same seed gives X's layout, scale, start and options; the matrix is A64, in both evaluations."""
    for loss, seed in XF.TABLE[::7]:
        mine, theirs = XF.draw(loss, seed), X.draw(loss, seed)
        assert mine._replace(shape=theirs.shape) == theirs
        assert XF.SHAPES.index(mine.shape) == X.SHAPES.index(theirs.shape)
        assert {k: v for k, v in XF.layout(seed).items() if k != "shape"} == {k: v for k, v in X.layout(seed).items() if k != "shape"}
    for loss in XF.LOSSES:
        for shape in XF.SHAPES[:5]:
            gen = XF.generated(loss, shape)
            A64 = gen.astype(np.float32).astype(np.float64)
            assert np.array_equal(XF.dense(loss, shape), A64) and np.array_equal(XF.data(loss, shape)[0].toarray(), A64)
            assert np.array_equal(XF.dense_reversed(loss, shape), A64[::-1])
            assert np.count_nonzero(A64 != gen) > 0.9 * np.count_nonzero(gen), "the rounding changes the matrix"
            assert XF.data(loss, shape)[1] is X.data(loss, shape)[1]   # (b, lam, delta: the unrounded problem's)
    case = XF.build(SPECS[0])
    ref, second = X.make_ref(case, cases=XF), X.make_ref(case, second=True, cases=XF)
    A64 = XF.dense(case.spec.loss, case.spec.shape)
    assert np.array_equal(ref.rows.A.toarray(), A64) and np.array_equal(second.rows.A, A64[::-1])


@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_case_is_decision_stable_and_keeps_its_run(spec):
    case, o, exp, nonfinite = XF.oracle(spec)
    assert exp is not None, "x0 is already at the resolution limit of the acceptance test: nothing left to run"
    if XF.ending(exp) == "error":
        assert exp.message == "Error: " + cpu_ref.MSG_BACKTRACK and not exp.success and "status" not in exp
        if exp.nit == 0:
            assert np.array_equal(exp.x, case.x0)
    else:
        assert exp.nit >= 1, "the stagnation cut left no iteration"
        assert o["max_iter"] == spec.options["max_iter"] or XF.ending(exp) == "max_iter"   # (a cut run ends at the cut)
    assert len(exp.alllrs) == len(exp.alltrials) == exp.nit
    assert np.all(np.isfinite(np.asarray(exp.allfuns[1:], float))) and np.all(np.isfinite(exp.x)), "every accepted F is finite"
    assert np.isfinite(exp.allfuns[0]) or XF.outside_box(case), "F(x0) = inf only where x0 lies outside the box"
    other = XF.other_form(spec)
    assert XF.disagreement(exp, other) is None and XF.disagreement(other, exp) is None
    assert XF.accepted(spec) is None
    assert (case.w is None) == (spec.weights is None) and (case.p is None) == (spec.factors is None)
    assert case.l2 == 0 or case.p is None, "factors with l2 > 0 are refused"
    assert np.array_equal(case.A.data, case.A.data.astype(np.float32).astype(np.float64)), "the oracle runs on A64"


def test_every_width_meets_every_loss_weights_kind_and_factor_kind():
    by = collections.Counter()
    for sp in SPECS:
        V = XF.width(sp)
        kind = XF.layout(sp.seed)["kind"]
        by.update([("loss-width", sp.loss, V), ("width-weights", V, sp.weights), ("width-factors", V, sp.factors),
                   ("loss-weights", sp.loss, sp.weights), ("loss-factors", sp.loss, sp.factors), ("loss-kind", sp.loss, kind),
                   ("loss-shape", sp.loss, sp.shape)])
    for loss, V in itertools.product(XF.LOSSES, WIDTHS):
        assert by["loss-width", loss, V] >= 1, (loss, V)
    for V, w in itertools.product(WIDTHS, XF.WEIGHTS):
        assert by["width-weights", V, w] >= 1, (V, w)
    for V, p in itertools.product(WIDTHS, XF.FACTORS):
        assert by["width-factors", V, p] >= 1, (V, p)
    for loss in XF.LOSSES:
        for w in XF.WEIGHTS:
            assert by["loss-weights", loss, w] >= 3, (loss, w, by["loss-weights", loss, w])
        for p in XF.FACTORS:
            assert by["loss-factors", loss, p] >= 3, (loss, p, by["loss-factors", loss, p])
        for kind in KIND_NAMES:
            assert by["loss-kind", loss, kind] >= 1, (loss, kind)
        for shape in XF.SHAPES:
            assert by["loss-shape", loss, shape] >= 1, (loss, shape)
    print({k: v for k, v in sorted(by.items(), key=str) if k[0] in ("loss-width", "width-weights", "width-factors")})


def test_what_the_runs_reach_per_loss():
    """Runs ended by tol, by max_iter and by "Backtracking failed", starts outside the box, l2 > 0 with weights, every decay
    rate, deprecated, NaN-able rows (w == 0) and p_j == 0 columns: each at least once per loss on the table as it stands."""
    for loss in XF.LOSSES:
        got = collections.Counter()
        for sp in (s for s in SPECS if s.loss == loss):
            case, o, exp, _ = XF.oracle(sp)
            got.update([XF.ending(exp), ("rate", o["decay_rate"])])
            got.update(["outside"] * (sp.bounds is not None and XF.outside_box(case)) + ["deprecated"] * bool(o["deprecated"])
                       + ["w-l2"] * bool(case.w is not None and case.l2 > 0) + ["w-zero"] * (case.w is not None and bool((case.w == 0).any()))
                       + ["p-zero"] * (case.p is not None and bool((case.p == 0).any())) + ["w-p"] * (case.w is not None and case.p is not None)
                       + ["rejected"] * any(t > 1 for t in exp.alltrials))
        print(loss, dict(got))
        for key in ("tol", "max_iter", "error", "outside", "deprecated", "w-l2", "w-zero", "p-zero", "w-p", "rejected"):
            assert got[key] >= 1, (loss, key)
        assert all(got["rate", r] >= 3 for r in X.DECAY_RATES), (loss, got)
    picks = XF.resume_cases()
    assert {(sp.loss, kind) for sp, kind in picks} == {(loss, kind) for loss in XF.LOSSES for kind in ("tol", "error")}
