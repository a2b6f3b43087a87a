"""CPU: the case table of tests/margins_fuzz_ext_cases.py is sound - its closures are the existing references' bit for bit
wherever those exist, every case is decided alike by two evaluations of them (CSR against the dense array with the rows of
(A, b, w) reversed; logistic: np.logaddexp / expit there), none has lost its run to the stagnation cut, the layout over the seed
holds what it promises, and the table reaches every situation it was drawn for at least three times per loss.
tests/test_gpu_fuzz_margins_ext.py runs the same table on the device classes and may therefore treat every mismatch as a finding
about the product."""
import collections
import itertools

import numpy as np
import pytest

import margins_fuzz_cases as M
import margins_fuzz_ext_cases as X
import poisson_cases as PC
import weight_cases as W
from oracle import cpu_ref
from test_margins_fuzz_cases import COVERAGE as OLD_COVERAGE

SPECS = [X.draw(loss, seed) for loss, seed in X.TABLE]
IDS = [f"{sp.loss}-s{sp.seed:02d}" for sp in SPECS]

COVERAGE = OLD_COVERAGE + ("weights with zero rows", "fold mask", "factor with zeros", "intercept", "factors and weights together",
                           "factors with the box and x0 outside", "weights with l2 > 0")
POISSON_COVERAGE = ("a rejected trial with f = +inf",)
KIND_NAMES = ("few_trials", "box", "to_tol", "short")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def features(spec):
    """What a case reaches, after the stagnation cut."""
    case, o, exp, nonfinite = X.oracle(spec)
    trials = list(exp.alltrials)
    end = X.ending(exp)
    outside = spec.bounds is not None and X.outside_box(case)
    got = {
        "backtracking failed": end == "error" and exp.nit == 0,
        "backtracking failed after accepted iterations": end == "error" and exp.nit > 0,
        "success by tol": end == "tol",
        "max_iter reached": end == "max_iter",
        "rejection in the first iteration": bool(trials) and trials[0] > 1,
        "rejection in a later iteration": any(t > 1 for t in trials[1:]),
        "box": spec.bounds is not None,
        "box with x0 outside": outside,
        "l2 > 0": case.l2 > 0,
        "x0 != 0": bool(np.any(case.x0 != 0)),
        "deprecated": o["deprecated"],
        "decay_rate 0.9": o["decay_rate"] == 0.9,
        "decay_rate 1.0": o["decay_rate"] == 1.0,
        "max_iter <= 2": o["max_iter"] <= 2,
        "weights with zero rows": case.w is not None and bool((case.w == 0).any()),
        "fold mask": spec.weights == "fold",
        "factor with zeros": spec.factors == "real" and bool((case.p == 0).any()),
        "intercept": spec.factors == "intercept",
        "factors and weights together": case.p is not None and case.w is not None,
        "factors with the box and x0 outside": case.p is not None and outside,
        "weights with l2 > 0": case.w is not None and case.l2 > 0,
        "a rejected trial with f = +inf": spec.loss == "poisson" and nonfinite > 0 and np.isfinite(exp.allfuns[0]),
    }
    return {k for k, v in got.items() if v}


def test_the_table_is_a_fixed_list_of_distinct_seeds_inside_the_replacement_cap():
    for loss in X.LOSSES:
        seeds = X.SEEDS[loss]
        assert len(seeds) == len(set(seeds)) == X.BLOCK and 24 <= X.BLOCK <= 48 and seeds == sorted(seeds), loss
        examined, replaced = X.EXAMINED[loss], X.REPLACED[loss]
        # the first BLOCK accepted seeds counted from 0: what was examined is 0 .. max, and what is missing was replaced
        assert examined == max(seeds) + 1 == len(seeds) + len(replaced) and sorted(set(range(examined)) - set(seeds)) == sorted(replaced)
        print(loss, "examined", examined, "replaced", len(replaced), replaced)
        assert 4 * len(replaced) <= examined, "at most one examined seed in four is replaced"


@pytest.mark.parametrize("loss", X.LOSSES)
def test_a_replaced_seed_fails_on_the_cpu(loss):
    """A seed is replaced for failing the CPU criteria of this file, and for nothing else."""
    for seed in X.REPLACED[loss]:
        assert X.accepted(X.draw(loss, seed)) is not None, seed


def _points(case, k=3):
    rng = np.random.default_rng(case.spec.seed + 77)
    n = case.spec.shape[1]
    return [np.zeros(n), 0.1 * rng.standard_normal(n), case.x0 if case.x0.any() else 0.5 + 0.1 * rng.standard_normal(n)][:k]


def _same_closures(ref, old, case):
    for x in _points(case):
        assert _bits(ref.f(x)) == _bits(old.f(x)) and _bits(ref.g(x)) == _bits(old.g(x))
        assert np.array_equal(_bits(ref.jac_f(x)), _bits(old.jac_f(x)))
        for wt in (0.37, 2.0 ** -9):
            assert np.array_equal(_bits(ref.prox_wsum_g(wt, x)), _bits(old.prox_wsum_g(wt, x)))


def _variant(loss, shape, l2fac, weights=None, bounds=None, seed=1):
    spec = X.draw(loss, seed)._replace(shape=shape, l2fac=l2fac, weights=weights, factors=None, bounds=bounds, start="shifted")
    return X.build(spec)


@pytest.mark.parametrize("l2fac", X.L2_FACTORS)
@pytest.mark.parametrize("loss", X.LOSSES[:3])
def test_without_weights_and_factors_the_closures_are_the_old_sweeps(loss, l2fac):
    """Bit-identical f, g, jac_f and prox to margins_fuzz_cases.make_ref, on both storage forms, with and without the box."""
    for bounds in (None, X.BOX):
        case = _variant(loss, X.SHAPES[0], l2fac, bounds=bounds)
        sp_ = case.spec
        old_spec = M.Spec(X.CLS[loss], sp_.seed, sp_.shape, sp_.scale, bounds, l2fac, sp_.start, sp_.x0_seed, sp_.options)
        old_case = M.build(old_spec)
        assert old_case.lam == case.lam and old_case.delta == (case.delta or None) and np.array_equal(old_case.b, case.b)
        for storage in X.FORMS:
            _same_closures(X.make_ref(case, storage), M.make_ref(old_case, storage), case)


@pytest.mark.parametrize("l2fac", X.L2_FACTORS)
@pytest.mark.parametrize("kind", X.WEIGHTS[1:])
@pytest.mark.parametrize("loss", X.LOSSES[:3])
def test_with_weights_only_the_closures_are_weighted_ref(loss, kind, l2fac):
    case = _variant(loss, X.SHAPES[1], l2fac, weights=kind, bounds=X.BOX if l2fac == 0.01 else None)
    sp_ = case.spec
    for storage in X.FORMS:
        old = W.WeightedRef(W.matrix(case.A, storage), case.b, case.lam, case.w, loss, case.delta, sp_.scale, sp_.bounds, case.l2)
        _same_closures(X.make_ref(case, storage), old, case)


@pytest.mark.parametrize("l2fac", X.L2_FACTORS)
@pytest.mark.parametrize("kind", X.WEIGHTS)
def test_with_poisson_the_closures_are_poisson_ref(kind, l2fac):
    case = _variant("poisson", X.SHAPES[2], l2fac, weights=kind, bounds=X.BOX if l2fac == 0.01 else None)
    sp_ = case.spec
    for storage in X.FORMS:
        old = PC.PoissonRef(PC.matrix(case.A, storage), case.b, case.lam, sp_.scale, sp_.bounds, case.l2, case.w)
        _same_closures(X.make_ref(case, storage), old, case)


@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_case_is_decision_stable_and_keeps_its_run(spec):
    case, o, exp, nonfinite = X.oracle(spec)
    assert exp is not None, "x0 is already at the resolution limit of the acceptance test: nothing left to run"
    if X.ending(exp) == "error":
        assert exp.message == "Error: " + cpu_ref.MSG_BACKTRACK and not exp.success and "status" not in exp
        if exp.nit == 0:
            assert np.array_equal(exp.x, case.x0)
    else:
        assert exp.nit >= 1, "the stagnation cut left no iteration"
        assert o["max_iter"] == spec.options["max_iter"] or X.ending(exp) == "max_iter"   # (a cut run ends at the cut)
    assert len(exp.alllrs) == len(exp.alltrials) == exp.nit
    assert np.all(np.isfinite(np.asarray(exp.allfuns[1:], float))) and np.all(np.isfinite(exp.x)), "every accepted F is finite"
    assert np.isfinite(exp.allfuns[0]) or X.outside_box(case), "F(x0) = inf only where x0 lies outside the box"
    assert nonfinite == 0 or spec.loss == "poisson" or not np.isfinite(exp.allfuns[0]), "only exp overflows"
    other = X.other_form(spec)
    assert X.disagreement(exp, other) is None and X.disagreement(other, exp) is None
    assert X.accepted(spec) is None
    assert (case.w is None) == (spec.weights is None) and (case.p is None) == (spec.factors is None)
    assert case.l2 == 0 or case.p is None, "factors with l2 > 0 are refused"


def test_the_layout_holds_every_combination_in_24_consecutive_seeds():
    """By construction, before any draw: the conditions of the table on 24 seeds from any multiple of 6 (and so on every block)."""
    for start in range(0, 96, 6):
        lay = [X.layout(s) for s in range(start, start + 24)]
        pairs = collections.Counter((l["weights"], l["factors"]) for l in lay)
        assert len(pairs) == 12 and min(pairs.values()) >= 2
        assert {(l["shape"], l["factors"]) for l in lay} == set(itertools.product(X.SHAPES, X.FACTORS))
        assert {(l["shape"], l["weights"]) for l in lay} == set(itertools.product(X.SHAPES, X.WEIGHTS))
        assert {(l["kind"], l["factors"]) for l in lay} == set(itertools.product(KIND_NAMES, X.FACTORS))
        assert {(l["kind"], l["weights"]) for l in lay} == set(itertools.product(KIND_NAMES, X.WEIGHTS))
        for key in ("factors", "weights"):
            rates = collections.Counter(l["decay_rate"] for l in lay if l[key] is not None)
            assert set(rates) == set(X.DECAY_RATES) and min(rates.values()) >= 2
        assert all(l["l2fac"] == 0.0 for l in lay if l["factors"] is not None)


def _layout_counts(specs):
    c = collections.Counter()
    for sp in specs:
        kind = X.layout(sp.seed)["kind"]
        rate = sp.options["decay_rate"]
        c.update([("pair", sp.weights, sp.factors), ("kind-factors", kind, sp.factors), ("kind-weights", kind, sp.weights),
                  ("shape-factors", sp.shape, sp.factors), ("shape-weights", sp.shape, sp.weights)])
        c.update([("rate-factors", rate)] * (sp.factors is not None) + [("rate-weights", rate)] * (sp.weights is not None))
    return c


def test_coverage_three_times_per_loss_and_the_layout_conditions_on_the_table():
    counts = {loss: collections.Counter() for loss in X.LOSSES}
    for spec in SPECS:
        counts[spec.loss].update(features(spec))
    for loss in X.LOSSES:
        names = COVERAGE + (POISSON_COVERAGE if loss == "poisson" else ())
        print(loss, {k: counts[loss][k] for k in names}, "late failures:", counts[loss]["backtracking failed after accepted iterations"])
        for k in names:
            assert counts[loss][k] >= 3, (loss, k, counts[loss][k])
        c = _layout_counts([sp for sp in SPECS if sp.loss == loss])
        low = {
            "pair": min(c["pair", w, p] for w in X.WEIGHTS for p in X.FACTORS),
            "kind-factors": min(c["kind-factors", k, p] for k in KIND_NAMES for p in X.FACTORS),
            "kind-weights": min(c["kind-weights", k, w] for k in KIND_NAMES for w in X.WEIGHTS),
            "shape-factors": min(c["shape-factors", s, p] for s in X.SHAPES for p in X.FACTORS),
            "shape-weights": min(c["shape-weights", s, w] for s in X.SHAPES for w in X.WEIGHTS),
            "rate-factors": min(c["rate-factors", r] for r in X.DECAY_RATES),
            "rate-weights": min(c["rate-weights", r] for r in X.DECAY_RATES),
        }
        print(loss, "layout minima", low)
        assert low["pair"] >= 2 and low["rate-factors"] >= 2 and low["rate-weights"] >= 2, (loss, low)
        assert min(low["kind-factors"], low["kind-weights"], low["shape-factors"], low["shape-weights"]) >= 1, (loss, low)


def test_a_rejected_poisson_trial_with_f_inf_leaves_f_finite():
    hit = [sp for sp in SPECS if "a rejected trial with f = +inf" in features(sp)]
    assert len(hit) >= 3
    for sp in hit:
        exp = X.oracle(sp).exp
        assert np.isfinite(np.asarray(exp.allfuns, float)).all() and sum(exp.alltrials) > exp.nit - (X.ending(exp) == "error")


def test_every_dense_form_tall_and_a_resume_case_of_each_kind_is_in_the_table():
    forms = collections.defaultdict(set)
    for spec in SPECS:
        forms[spec.loss].add(X.dense_form(spec))
    for loss in X.LOSSES:
        assert forms[loss] == X.dense_forms_possible(loss), (loss, forms[loss])
        mine = [sp for sp in SPECS if sp.loss == loss]
        # a weighted, a factored and an l2 sibling of the 48 x 96 problem leave the fused small-matrix form
        for sp in mine:
            if sp.shape[:2] == (48, 96):
                plain = loss == "square" and sp.weights is None and sp.factors is None and sp.l2fac == 0
                assert X.dense_form(sp) == (X.SMALL_FORM if plain else X.MFMA)
        assert any(sp.shape[:2] == (48, 96) and (sp.weights or sp.factors) for sp in mine)
        assert any(sp.shape == X.S.TALL and sp.weights is None for sp in mine) and any(sp.shape == X.S.TALL and sp.weights for sp in mine)
        assert {sp.shape for sp in mine} == set(X.SHAPES)
    picks = X.resume_cases()
    assert {(sp.loss, kind) for sp, kind in picks} == {(loss, kind) for loss in X.LOSSES for kind in ("tol", "error")}
    ones = X.ones_cases()
    assert {(sp.loss, X.layout(sp.seed)["kind"]) for sp in ones} == set(itertools.product(X.LOSSES, KIND_NAMES))
