"""CPU: the case table of tests/mr_fuzz_cases.py is sound - every case is decided alike by two evaluations of its closures (per
response over the CSR matrix against the dense array with the rows of (A, Y, w) reversed and the library forms of the logistic and
multinomial rows), none has lost its run to the stagnation cut, the per-response closures are the Kronecker closures the project
already has, the layout over the seed holds what it promises - on any block of 30 seeds and on the table after its replacements -
and the replaced seeds are inside the cap.  tests/test_gpu_fuzz_mr.py runs the same table on the device classes and may therefore
treat every mismatch as a finding about the product."""
import collections
import itertools

import numpy as np
import pytest

import mr_fuzz_cases as F
import multiresponse_cases as MR
from oracle import cpu_ref

SPECS = [F.draw(loss, seed) for loss, seed in F.TABLE]
IDS = [f"{sp.loss}-s{sp.seed:02d}" for sp in SPECS]
KIND_NAMES = ("few_trials", "box", "to_tol", "short")
SMALL3 = F.SHAPES[:3]


def test_the_table_is_one_seed_per_cell_inside_the_replacement_cap():
    for loss in F.LOSSES:
        seeds, replaced = F.SEEDS[loss], F.REPLACED[loss]
        assert len(seeds) == len(set(seeds)) == F.BLOCK == 30 and sorted(s % F.STRIDE for s in seeds) == list(range(30)), loss
        # what was examined: per cell c, c + 90, ... up to the seed the table holds; what is not in the table was replaced
        examined = sorted(s for seed in seeds for s in range(seed % F.STRIDE, seed + 1, F.STRIDE))
        assert len(examined) == F.EXAMINED[loss] and sorted(set(examined) - set(seeds)) == sorted(replaced)
        print(loss, "examined", len(examined), "replaced", len(replaced), replaced)
        assert 4 * len(replaced) <= len(examined), "at most one examined seed in four is replaced"


@pytest.mark.parametrize("loss", F.LOSSES)
def test_a_replaced_seed_fails_on_the_cpu(loss):
    """A seed is replaced for failing the CPU criteria of this file, and for nothing else."""
    for seed in F.REPLACED[loss]:
        assert F.accepted(F.draw(loss, seed)) is not None, seed


@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_case_is_accepted(spec):
    case, o, exp, nonfinite = F.oracle(spec)
    assert exp is not None, "x0 is already at the resolution limit of the acceptance test: nothing left to run"
    if F.ending(exp) == "error":
        assert exp.message == "Error: " + cpu_ref.MSG_BACKTRACK and not exp.success and "status" not in exp
        if exp.nit == 0:
            assert np.array_equal(exp.x, case.x0)
    else:
        assert exp.nit >= 1, "the stagnation cut left no iteration"
        assert o["max_iter"] == spec.options["max_iter"] or F.ending(exp) == "max_iter"   # (a cut run ends at the cut)
    assert len(exp.alllrs) == len(exp.alltrials) == exp.nit and exp.x.shape == (spec.shape[1] * spec.K,)
    assert exp.nit <= 60 and max(exp.alltrials, default=0) <= 100
    assert np.all(np.isfinite(np.asarray(exp.allfuns[1:], float))) and np.all(np.isfinite(exp.x)), "every accepted F is finite"
    assert np.isfinite(exp.allfuns[0]) or F.outside_box(case), "F(x0) = inf only where x0 lies outside the box"
    assert nonfinite == 0 or not np.isfinite(exp.allfuns[0]), "no loss of this table overflows"
    other = F.other_form(spec)
    assert F.disagreement(exp, other) is None and F.disagreement(other, exp) is None
    assert F.accepted(spec) is None
    # the case is what its spec says
    m, n = spec.shape[:2]
    assert case.B.shape == (m, spec.K) and case.x0.shape == (n * spec.K,)
    assert (case.w is None) == (spec.weights is None) and (case.p is None) == (spec.factors is None)
    assert case.l2 == 0 or case.p is None, "factors with l2 > 0 are refused"
    if case.w is not None:
        assert case.w.shape == ((m, spec.K) if spec.wide else (m,)) and (case.w == 0).any() and (case.w > 0).any()
    if case.p is not None:
        assert case.p.shape == ((n, spec.K) if spec.factors == "positive" else (n,)) and bool(np.all(case.p[0] == 0)) == (spec.factors == "zero")
    if spec.loss == "multinomial":
        there = np.ones(m, bool) if case.w is None else case.w != 0
        assert not spec.wide and np.all(np.abs(case.B[there].sum(axis=1) - 1.0) <= 1e-12) and np.all(case.B[there] >= 0)
        assert bool((~there).any() and np.isnan(case.B[~there]).all()) == spec.nan and not np.isnan(case.B[there]).any()
        assert ((case.B[there] == 1.0).any(axis=1).all()) == (spec.labels == "hot")
        if spec.absent:
            assert spec.K > 2 and np.all(case.B[there][:, spec.K - 1] == 0)
    else:
        assert np.isfinite(case.B).all() and not spec.nan and not spec.absent


def _conditions(lays):
    """The combinations the layout promises, on a list of layout dicts (each with its loss-independent fields)."""
    assert {(l["shape"], l["K"]) for l in lays} == set(itertools.product(F.SHAPES, F.KS)), "every (shape, K) pair"
    assert {(l["K"], l["weights"]) for l in lays} == set(itertools.product(F.KS, F.WEIGHTS)), "every K meets every weights kind"
    assert {(l["K"], l["factors"]) for l in lays} == set(itertools.product(F.KS, F.FACTORS)), "every K meets every factor kind"
    assert {(l["weights"], l["factors"]) for l in lays} == set(itertools.product(F.WEIGHTS, F.FACTORS))
    assert all(l["l2fac"] == 0.0 for l in lays if l["factors"] is not None)
    assert sum(l["weights"] is not None and l["l2fac"] > 0 for l in lays) >= 2, "weights with l2 > 0"
    assert sum(l["factors"] is not None and l["bounds"] is not None for l in lays) >= 2, "factors with the box"
    assert {l["wide"] for l in lays if l["weights"] is not None} == {False, True}, "(m,) and (m, K) weights"
    assert sum(l["nan"] for l in lays) >= 2 and sum(l["absent"] for l in lays) == 3
    assert 9 <= sum(l["x0_2d"] for l in lays) <= 11 and sum(l["sibling"] for l in lays) == 15


def test_the_layout_holds_every_combination_in_30_consecutive_seeds():
    """By construction, before any draw: on 30 seeds from any multiple of 30 (and so on every ZF_FUZZ_SCALE block)."""
    for start in range(0, 300, 30):
        lays = [F.layout(s) for s in range(start, start + 30)]
        _conditions(lays)
        assert {l["kind"] for l in lays} == set(KIND_NAMES) and {l["decay_rate"] for l in lays} == set(F.DECAY_RATES)
    # a replaced seed's successor keeps its cell
    same = ("shape", "K", "weights", "factors", "l2fac", "nan", "x0_2d", "labels", "absent", "sibling")
    for s in range(90):
        a, b = F.layout(s), F.layout(s + F.STRIDE)
        assert all(a[k] == b[k] for k in same) and a["kind"] != b["kind"]
    # m K on either side of the many-workgroup threshold of the rows kernels at m = 4097
    assert 4097 * 7 < F.MC.WIDE < 4097 * 8 and {MR.rows_per_wg(K) for K in F.KS} == {16, 24, 32}


@pytest.mark.parametrize("loss", F.LOSSES)
def test_the_combinations_hold_on_the_table_after_replacement(loss):
    mine = [sp for sp in SPECS if sp.loss == loss]
    lays = []
    for sp in mine:
        lay = F.layout(sp.seed)
        # the spec carries the layout (the multinomial-only fields are off for the other two losses)
        assert (sp.shape, sp.K, sp.weights, sp.factors, sp.l2fac, sp.bounds) == tuple(lay[k] for k in ("shape", "K", "weights", "factors", "l2fac", "bounds"))
        assert sp.x0_2d == lay["x0_2d"] and sp.sibling == lay["sibling"] and sp.options["decay_rate"] == lay["decay_rate"]
        if loss == "multinomial":
            assert (sp.wide, sp.nan, sp.absent, sp.labels) == (False, lay["nan"], lay["absent"], lay["labels"])
        else:
            assert (sp.wide, sp.nan, sp.absent, sp.labels) == (lay["wide"], False, False, None)
        lays.append(lay)
    _conditions(lays)
    outside = sum(sp.bounds is not None and F.outside_box(F.build(sp)) for sp in mine)
    ends = collections.Counter((F.ending(F.oracle(sp).exp), F.oracle(sp).exp.nit >= 1) for sp in mine)
    rejected_later = sum(any(t > 1 for t in list(F.oracle(sp).exp.alltrials)[1:]) for sp in mine)
    print(loss, "x0 outside the box:", outside, "endings:", dict(ends), "a rejection after the first iteration:", rejected_later)
    assert outside >= 2, "a start outside the box"
    assert sum(sp.weights is not None and sp.l2fac > 0 for sp in mine) >= 2 and sum(sp.factors is not None and sp.bounds is not None for sp in mine) >= 2
    assert ends["tol", True] >= 3 and ends["max_iter", True] >= 3 and ends["error", False] >= 3 and rejected_later >= 1
    assert {sp.options["decay_rate"] for sp in mine} == set(F.DECAY_RATES) and {F.layout(sp.seed)["kind"] for sp in mine} == set(KIND_NAMES)
    assert {sp.options["max_backtrack_iter"] for sp in mine} >= {1, 2, 5}
    assert {F.dense_form(sp) for sp in mine} == {F.MR_VALU2, F.MR_VALU1}
    if loss == "multinomial":
        wide = {(sp.K, sp.shape[0] * sp.K > F.MC.WIDE) for sp in mine if sp.shape[0] == 4097}
        assert wide == {(K, K >= 8) for K in F.KS}, "both shapes of the rows kernels, K = 7 and 8 on either side"


def test_resume_cases_hold_a_tol_and_an_error_ending_per_loss():
    picks = F.resume_cases()
    assert [(sp.loss, kind) for sp, kind in picks] == [(loss, kind) for loss in F.LOSSES for kind in ("tol", "error")]
    for sp, kind in picks:
        assert F.ending(F.oracle(sp).exp) == kind and (sp.loss, sp.seed) in F.TABLE
    late = [sp.loss for sp, kind in picks if kind == "error" and F.oracle(sp).exp.nit >= 1]
    print("error endings after accepted iterations:", late)
    assert late, "Backtracking failed after accepted iterations, for at least one loss"
    sib = F.sibling_cases()
    assert [(sp.loss, F.layout(sp.seed)["kind"]) for sp in sib] == list(itertools.product(F.LOSSES, KIND_NAMES))


def _kron_spec(loss, shape, K, variant):
    """A table draw moved to ``shape`` and ``K`` at the scale of multiresponse_cases.SCALE: 0 weights and l2, 1 factors and the box."""
    spec = F.draw(loss, 4)._replace(shape=shape, K=K, scale=1.0 if loss == "multinomial" else MR.SCALE[loss], start="near", absent=False,
                                    labels="soft" if loss == "multinomial" else None, nan=False)
    if variant == 0:
        return spec._replace(weights="real", wide=loss != "multinomial", factors=None, l2fac=0.01, bounds=None)
    return spec._replace(weights=None, wide=False, factors="positive" if K == 2 else "zero", l2fac=0.0, bounds=F.BOX)


@pytest.mark.parametrize("variant", [0, 1], ids=["weights-l2", "factors-box"])
@pytest.mark.parametrize("K", [2, 16])
@pytest.mark.parametrize("shape", SMALL3, ids=[f"{s[0]}x{s[1]}" for s in SMALL3])
@pytest.mark.parametrize("loss", F.LOSSES)
def test_the_per_response_closures_are_the_kronecker_closures(loss, shape, K, variant):
    """f, g, jac_f and prox of the oracle's closures against sparse_multiresponse_cases.kron_ref / multinomial_cases.KronRef on
    sp.kron(A, I_K): another order of the same sums.  Bounds: 1e-13 of the largest entry for the gradient (what
    tests/test_multinomial_cases.py asks of the same pair), 1e-13 relative for f; g and the prox are the same element-wise
    expressions - 4 ulp for the sums of g (pairwise against sequential over n K terms of one sign), the prox bit for bit."""
    case = F.build(_kron_spec(loss, shape, K, variant))
    ref, kron = F.make_ref(case), F.kron_ref(case)
    rng = np.random.default_rng(shape[3] + K)
    x = 0.1 * rng.standard_normal(shape[1] * K)
    inside = np.clip(x, *F.BOX)
    assert abs(ref.f(x) - kron.f(x)) <= 1e-13 * abs(kron.f(x))
    ga, gb = ref.jac_f(x), kron.jac_f(x)
    assert ga.shape == gb.shape == x.shape and np.max(np.abs(ga - gb)) <= 1e-13 * max(1.0, float(np.max(np.abs(gb))))
    for v in (x, inside):
        a, b = ref.g(v), kron.g(v)
        assert (np.isinf(a) and np.isinf(b)) if case.spec.bounds is not None and v is x else abs(a - b) <= 4 * np.finfo(float).eps * abs(b)
    for wt in (0.37, 2.0 ** -9):
        assert np.array_equal(ref.prox_wsum_g(wt, x), kron.prox_wsum_g(wt, x))
    # the second evaluation is the same function of x (rows reversed, library forms)
    second = F.make_ref(case, second=True)
    assert abs(second.f(x) - ref.f(x)) <= 1e-13 * abs(ref.f(x)) and np.max(np.abs(second.jac_f(x) - ga)) <= 1e-13 * max(1.0, float(np.max(np.abs(ga))))


def test_dense_plan_and_ids():
    ids = [F.case_id(sp) for sp in SPECS]
    assert len(set(ids)) == len(ids) == 90
    for sp in SPECS:
        plan = F.dense_plan(sp)
        assert plan[0] == (9 if sp.shape[1] % 2 == 0 else 10) and plan[4] == sp.K and plan[5] == MR.rows_per_wg(sp.K)
