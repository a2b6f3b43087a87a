"""GPU: the option sweep of tests/margins_fuzz_ext_cases.py on the eight margins classes with per-row sample weights (real and
0 / 1 fold masks, with zero rows), per-column penalty factors (with zeros, positive, an intercept) and the Poisson loss - under
the box, the elastic-net l2, a start away from 0 (also outside the box), decay rates that are no power of two or 1, one to a
hundred trials per line search, runs of 1 or 2 iterations, runs ended by tol and by "Backtracking failed", and on 40000 rows -
against the CPU oracle on the reference closures.

tests/test_margins_fuzz_ext_cases.py has shown on the CPU that the oracle's decisions on every case of the fixed table do not
depend on the summation order, so a mismatch here is a finding about the product.  One test id is one case; it runs the sparse and
the dense class of the case against one oracle run.  The checks are those of tests/test_gpu_fuzz_margins.py (``_check_storage``,
TOL = 1e-10), and per storage form:

  * one more solve at a sub_iters of (1, 4, 16) gives the x and the trace of the default, bit for bit;
  * with factors, the accepted iterates restricted to the columns with p_j = 0 match the oracle's to the same tolerance (without a
    box such a column takes the plain gradient step: no threshold);
  * with zero-weight rows, b on those rows is overwritten with NaN in device memory and the solve is unchanged bit for bit.

ZF_FUZZ_SCALE=k appends k - 1 further blocks of seeds (a one-off soak), each case filtered by the CPU criteria while the ids are
collected."""
import os

import numpy as np
import pytest

import margins_fuzz_ext_cases as X
from conftest import rel_err
from test_gpu_fuzz_margins import TOL, _bits, _check_resume, _check_storage, default_switches, solve   # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SCALE = int(os.environ.get("ZF_FUZZ_SCALE", "1"))
TABLE = X.TABLE + [c for k in range(1, SCALE) for c in X.extra_block(k)]
SPECS = [X.draw(loss, seed) for loss, seed in TABLE]
SUB_ITERS = (1, 4, 16)


def _extra_checks(case, storage, o, exp, solve, kept):
    import torch

    spec, x0 = case.spec, case.x0
    prob, res, res1, rows1 = kept["prob"], kept["res"], kept["res1"], kept["rows1"]
    sub = SUB_ITERS[spec.seed % 3]
    again, rows_sub, _ = solve(prob, x0, return_all=False, sub_iters=sub, **o)
    assert np.array_equal(_bits(again.x), _bits(res1.x)) and np.array_equal(rows_sub, rows1), ("sub_iters", sub)
    if case.p is not None and (case.p == 0).any():
        free = case.p == 0
        assert max(rel_err(a[free], e[free]) for a, e in zip(res.allvecs, exp.allvecs)) <= TOL, "the columns with p_j = 0"
    if case.w is not None and (case.w == 0).any():
        off = torch.from_numpy(np.flatnonzero(case.w == 0)).to(prob.b.device)
        prob.b[off] = float("nan")   # (what a row with w = 0 holds must not matter; the constructor refuses such a b)
        spoiled, rows_sp, _ = solve(prob, x0, return_all=True, **o)
        assert np.array_equal(_bits(spoiled.x), _bits(res.x)) and np.array_equal(rows_sp, kept["rows"]), "NaN on rows with w = 0"
        assert np.array_equal(_bits(np.asarray(spoiled.allfuns)), _bits(np.asarray(res.allfuns)))
        assert all(np.array_equal(_bits(a), _bits(e)) for a, e in zip(spoiled.allvecs, res.allvecs))


@pytest.mark.parametrize("spec", SPECS, ids=[X.case_id(sp) for sp in SPECS])
def test_fuzz_margins_ext(spec, solve):
    case, o, exp, _ = X.oracle(spec)
    assert exp is not None
    cols = {}
    for storage in X.FORMS:
        kept = {}
        cols[storage] = _check_storage(case, storage, o, exp, solve, cases=X, keep=kept)
        _extra_checks(case, storage, o, exp, solve, kept)
    assert np.array_equal(cols["csr"], cols["dense"]), "the sparse and the dense class of a case take the same lr and trial sequences"


ONES = X.ones_cases()


@pytest.mark.parametrize("spec", ONES, ids=[f"{sp.loss}-{X.layout(sp.seed)['kind']}-s{sp.seed:02d}" for sp in ONES])
def test_unit_factors_are_the_plain_class_bit_for_bit(spec, solve, monkeypatch):
    """penalty_factor = ones against the plain class under the case's weights, box, start and options (l2 = 0 and no factors of
    the case's own): the same x, trace rows, allvecs and allfuns.  Where the plain class would take the fused small-matrix form -
    which a factored sibling leaves - both run on the general path."""
    case = X.build(spec)._replace(l2=0.0, p=None)
    plain_spec = spec._replace(l2fac=0.0, factors=None)
    if X.dense_form(plain_spec) == X.SMALL_FORM:
        monkeypatch.setenv("ZF_LS_SMALL", "0")
    o = dict(spec.options)
    for storage in X.FORMS:
        out = []
        for p in (None, np.ones(spec.shape[1])):
            res, rows, plan = solve(X.make_problem(case, storage, factors=p), case.x0, return_all=True, **o)
            out.append((res, rows, plan))
        (r0, rows0, plan0), (r1, rows1, plan1) = out
        assert plan0[0] == plan1[0] == (X.CSR if storage == "csr" else max(X.dense_form(plain_spec), X.MFMA))
        assert r0.nit == r1.nit and r0.message == r1.message and r0.success == r1.success
        assert np.array_equal(rows0, rows1) and np.array_equal(_bits(r0.x), _bits(r1.x))
        assert len(r0.allvecs) == len(r1.allvecs) and all(np.array_equal(_bits(a), _bits(e)) for a, e in zip(r0.allvecs, r1.allvecs))
        assert np.array_equal(_bits(np.asarray(r0.allfuns)), _bits(np.asarray(r1.allfuns)))


RESUME = X.resume_cases()


@pytest.mark.parametrize("spec,kind", RESUME, ids=[f"{sp.loss}-{kind}-s{sp.seed:02d}" for sp, kind in RESUME])
def test_snapshot_resume_across_the_last_chunk(spec, kind, tmp_path):
    """The table's longest run of the loss that ends by tol, and its longest that ends in the error path: a snapshot taken one
    chunk before the end, and the run resumed from it, end with the status, x and trace of the uninterrupted run."""
    case, o, exp, _ = X.oracle(spec)
    _check_resume(case, o, exp, kind, tmp_path, cases=X)
