"""GPU: the option sweep of tests/mr_fuzz_cases.py on the six K-response classes - MultiResponseLeastSquaresL1 /
SparseMultiResponseLeastSquaresL1, MultiResponseLogisticL1 / SparseMultiResponseLogisticL1, MultinomialL1 / SparseMultinomialL1 - at
K in (2, 3, 7, 8, 12, 16) with (m,) and (m, K) weights (zero rows, fold masks, NaN targets on rows that are not there), (n, K) and (n,)
penalty factors, the box, the elastic-net l2, a start away from 0 (also outside the box, also handed over as the (n, K) array), decay
rates that are no power of two or 1, one to a hundred trials per line search, runs of 1 or 2 iterations, runs ended by tol and by
"Backtracking failed", problems built through the constructors and as siblings - against the CPU oracle on the per-response closures.

tests/test_mr_fuzz_cases.py has shown on the CPU that the oracle's decisions on every case of the fixed table do not depend on the
summation order, so a mismatch here is a finding about the product.  One test id is one case; it runs the sparse and the dense class
of the case against one oracle run.  The checks are those of tests/test_gpu_fuzz_margins.py (``_check_storage``, TOL = 1e-10), and
per storage form:

  * zf_solver_ls_plan is what mr_fuzz_cases.dense_plan says (the K-response sweep form, K, the rows of a workgroup), or CSR with K;
  * x0 in its other shape - (n, K) where the case passes it flat, flat where it passes (n, K) - gives the same result bit for bit;
  * coef(x) is (n, K); for the multinomial loss the rows of predict_proba(x) sum to 1 within 4 ulp;
  * with an exact-zero factor, the accepted iterates restricted to that row of X match the oracle's to the same tolerance;
  * with zero-weight rows whose targets are finite, those targets are overwritten with NaN in device memory and the solve is
    unchanged bit for bit (the multinomial cases whose Y holds NaN from the start run the whole test that way).

ZF_FUZZ_SCALE=k appends k - 1 further blocks of seeds (a one-off soak), each case filtered by the CPU criteria while the ids are
collected."""
import os

import numpy as np
import pytest

import mr_fuzz_cases as F
from conftest import rel_err
from test_gpu_fuzz_margins import TOL, _bits, _check_resume, _check_storage, default_switches, solve   # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SCALE = int(os.environ.get("ZF_FUZZ_SCALE", "1"))
TABLE = F.TABLE + [c for k in range(1, SCALE) for c in F.extra_block(k)]
SPECS = [F.draw(loss, seed) for loss, seed in TABLE]
ULP = float(np.finfo(np.float64).eps)


@pytest.fixture
def solve_k(solve, monkeypatch):
    """``solve`` of tests/test_gpu_fuzz_margins.py with the plan extended by zf_solver_ls_plan's slots 4 and 5 (K, the rows a
    workgroup of the row sweep owns), and x0 handed over as the (n, K) array while ``two_d`` is set."""
    from zfista_amd import proximal_gradient as pg

    class _WithResponses(pg.NativeRun):   # (the recording class ``solve`` has put there)
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.plan = tuple(self.plan) + tuple(self.solver.responses_plan())

    monkeypatch.setattr(pg, "NativeRun", _WithResponses)

    def run(prob, x0, **kw):
        if run.two_d:
            x0 = np.asarray(x0).reshape(prob._n, prob.n_responses)
            assert x0.ndim == 2
        return solve(prob, x0, **kw)

    run.two_d = False
    return run


def _same(a, b, rows_a, rows_b, what):
    assert a.nit == b.nit and a.message == b.message and a.success == b.success, what
    assert np.array_equal(rows_a, rows_b) and np.array_equal(_bits(a.x), _bits(b.x)), what
    assert len(a.allvecs) == len(b.allvecs) and all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a.allvecs, b.allvecs)), what
    assert np.array_equal(_bits(np.asarray(a.allfuns)), _bits(np.asarray(b.allfuns))), what
    assert np.array_equal(_bits(np.asarray(a.allerrs)), _bits(np.asarray(b.allerrs))), what


def _extra_checks(case, storage, o, exp, solve_k, kept):
    import torch

    spec, x0 = case.spec, case.x0
    n, K = spec.shape[1], spec.K
    prob, res, rows, plan = kept["prob"], kept["res"], kept["rows"], kept["plan"]
    want = F.sparse_plan(spec) if storage == "csr" else F.dense_plan(spec)
    assert len(plan) == 6 and all(plan[slot] == v for slot, v in want.items()), (plan, want)
    assert prob.n_responses == K and prob.n_features == n * K
    # x0 in its other shape
    solve_k.two_d = not spec.x0_2d
    other, rows_o, plan_o = solve_k(prob, x0, return_all=True, **o)
    solve_k.two_d = spec.x0_2d
    assert plan_o == plan
    _same(other, res, rows_o, rows, "x0 as (n, K) and flat")
    assert res.x.shape == (n * K,) and all(v.shape == (n * K,) for v in res.allvecs)
    coef = prob.coef(res.x)
    assert coef.shape == (n, K) and np.array_equal(_bits(coef.reshape(-1)), _bits(res.x))
    if spec.loss == "multinomial":
        proba = prob.predict_proba(res.x)
        assert proba.shape == (spec.shape[0], K) and np.all(proba >= 0)
        assert np.max(np.abs(proba.sum(axis=1) - 1.0)) <= 4 * ULP
        assert np.array_equal(_bits(prob.predict_proba(coef)), _bits(proba))
    if spec.factors == "zero":
        free = np.arange(K)   # (row 0 of X: p_0 = 0 for every response)
        assert max(rel_err(a[free], e[free]) for a, e in zip(res.allvecs, exp.allvecs)) <= TOL, "the row of X with p = 0"
    if case.w is not None and not spec.nan:
        w = case.w if case.w.ndim == 2 else np.repeat(case.w.reshape(-1, 1), K, axis=1)
        off = torch.from_numpy(np.flatnonzero(w.reshape(-1) == 0)).to(prob.b.device)
        assert off.numel() > 0
        prob.b[off] = float("nan")   # (what a row with w = 0 holds must not matter)
        spoiled, rows_sp, _ = solve_k(prob, x0, return_all=True, **o)
        _same(spoiled, res, rows_sp, rows, "NaN on rows with w = 0")


@pytest.mark.parametrize("spec", SPECS, ids=[F.case_id(sp) for sp in SPECS])
def test_fuzz_mr(spec, solve_k):
    case, o, exp, _ = F.oracle(spec)
    assert exp is not None
    solve_k.two_d = spec.x0_2d
    cols = {}
    for storage in F.FORMS:
        kept = {}
        cols[storage] = _check_storage(case, storage, o, exp, solve_k, cases=F, keep=kept)
        _extra_checks(case, storage, o, exp, solve_k, kept)
    assert np.array_equal(cols["csr"], cols["dense"]), "the sparse and the dense class of a case take the same lr and trial sequences"


RESUME = F.resume_cases()


@pytest.mark.parametrize("spec,kind", RESUME, ids=[f"{sp.loss}-{kind}-s{sp.seed:02d}-K{sp.K}" for sp, kind in RESUME])
def test_snapshot_resume_across_the_last_chunk(spec, kind, tmp_path):
    """The table's longest run of the loss that ends by tol, and its longest that ends in the error path: a snapshot taken one
    chunk before the end, and the run resumed from it, end with the status, x and trace of the uninterrupted run."""
    case, o, exp, _ = F.oracle(spec)
    _check_resume(case, o, exp, kind, tmp_path, cases=F)


SIBLINGS = F.sibling_cases()


@pytest.mark.parametrize("spec", SIBLINGS, ids=[f"{sp.loss}-{F.layout(sp.seed)['kind']}-s{sp.seed:02d}-K{sp.K}" for sp in SIBLINGS])
def test_sibling_and_constructor_build_the_same_problem(spec, solve_k):
    """plain.with_responses / with_classes, then with_penalty, then with_penalty_factor, against the constructor's keywords: the same
    x, trace rows, allvecs, allfuns and allerrs, bit for bit, on both storage forms."""
    case = F.build(spec)
    o = dict(spec.options)
    for storage in F.FORMS:
        sib, rows_s, plan_s = solve_k(F.make_problem(case, storage, sibling=True), case.x0, return_all=True, **o)
        new, rows_n, plan_n = solve_k(F.make_problem(case, storage, sibling=False), case.x0, return_all=True, **o)
        assert plan_s == plan_n
        _same(sib, new, rows_s, rows_n, storage)
