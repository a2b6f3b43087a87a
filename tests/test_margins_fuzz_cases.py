"""CPU: the case table of tests/margins_fuzz_cases.py is sound - every case is decided alike by two evaluations of the reference
closures (CSR against .toarray(); logistic: the stable form against np.logaddexp / expit with the loss summed in reverse), none
has lost its run to the stagnation cut, and the table reaches every situation it was drawn for at least three times per class.
tests/test_gpu_fuzz_margins.py runs the same table on the device classes and may therefore treat every mismatch as a finding
about the product."""
import collections

import numpy as np
import pytest

import margins_fuzz_cases as M
from oracle import cpu_ref

SPECS = [M.draw(cls, seed) for cls, seed in M.TABLE]
IDS = [f"{sp.cls}-s{sp.seed:02d}" for sp in SPECS]

COVERAGE = ("backtracking failed", "success by tol", "max_iter reached", "rejection in the first iteration",
            "rejection in a later iteration", "box", "box with x0 outside", "l2 > 0", "x0 != 0", "deprecated", "decay_rate 0.9",
            "decay_rate 1.0", "max_iter <= 2")


def features(spec):
    """What a case reaches, after the stagnation cut."""
    case, o, exp = M.oracle(spec)
    trials = list(exp.alltrials)
    end = M.ending(exp)
    got = {
        "backtracking failed": end == "error" and exp.nit == 0,
        "backtracking failed after accepted iterations": end == "error" and exp.nit > 0,
        "success by tol": end == "tol",
        "max_iter reached": end == "max_iter",
        "rejection in the first iteration": bool(trials) and trials[0] > 1,
        "rejection in a later iteration": any(t > 1 for t in trials[1:]),
        "box": spec.bounds is not None,
        "box with x0 outside": spec.bounds is not None and M.outside_box(case),
        "l2 > 0": case.l2 > 0,
        "x0 != 0": bool(np.any(case.x0 != 0)),
        "deprecated": o["deprecated"],
        "decay_rate 0.9": o["decay_rate"] == 0.9,
        "decay_rate 1.0": o["decay_rate"] == 1.0,
        "max_iter <= 2": o["max_iter"] <= 2,
    }
    return {k for k, v in got.items() if v}


def test_the_table_is_a_fixed_list_of_distinct_seeds():
    for cls in M.CLASSES:
        seeds = [s for c, s in M.TABLE if c == cls]
        assert len(seeds) == len(set(seeds)) >= 16, cls
    assert {sp.shape for sp in SPECS} == set(M.SHAPES)


@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_case_is_decision_stable_and_keeps_its_run(spec):
    case, o, exp = M.oracle(spec)
    assert exp is not None, "x0 is already at the resolution limit of the acceptance test: nothing left to run"
    if M.ending(exp) == "error":
        assert exp.message == "Error: " + cpu_ref.MSG_BACKTRACK and not exp.success and "status" not in exp
        if exp.nit == 0:
            assert np.array_equal(exp.x, case.x0)
    else:
        assert exp.nit >= 1, "the stagnation cut left no iteration"
        assert o["max_iter"] == spec.options["max_iter"] or M.ending(exp) == "max_iter"   # (a cut run ends at the cut)
    assert len(exp.alllrs) == len(exp.alltrials) == exp.nit
    assert np.all(np.isfinite(np.asarray(exp.allfuns[1:], float))) and np.all(np.isfinite(exp.x))
    assert np.isfinite(exp.allfuns[0]) or M.outside_box(case), "F(x0) = inf only where x0 lies outside the box"
    other = M.other_form(spec)
    assert M.disagreement(exp, other) is None and M.disagreement(other, exp) is None


def test_coverage_three_times_per_class():
    counts = {cls: collections.Counter() for cls in M.CLASSES}
    for spec in SPECS:
        counts[spec.cls].update(features(spec))
    for cls in M.CLASSES:
        print(cls, {k: counts[cls][k] for k in COVERAGE}, "late failures:", counts[cls]["backtracking failed after accepted iterations"])
        for k in COVERAGE:
            assert counts[cls][k] >= 3, (cls, k, counts[cls][k])


def test_every_dense_form_and_a_resume_case_of_each_kind_is_in_the_table():
    forms = collections.defaultdict(set)
    for spec in SPECS:
        forms[spec.cls].add(M.dense_form(spec))
    assert forms["ls"] == {M.SMALL_FORM, M.MFMA, M.VALU2, M.VALU1}
    assert forms["logit"] == forms["huber"] == {M.MFMA, M.VALU2, M.VALU1}   # (the fused small-matrix kernels: squared loss only)
    # 4097 x 64: one row more than the small form takes
    assert any(sp.cls == "ls" and sp.l2fac == 0 and sp.shape[:2] == (4097, 64) for sp in SPECS)
    picks = M.resume_cases()
    assert {(sp.cls, kind) for sp, kind in picks} == {(cls, kind) for cls in M.CLASSES for kind in ("tol", "error")}
