"""GPU: the option sweep of tests/margins_fuzz_cases.py on the six margins classes - SparseLeastSquaresL1 / LeastSquaresL1,
SparseLogisticL1 / LogisticL1, SparseHuberL1 / HuberL1, with the box, the elastic-net l2, a start away from 0 (also outside the
box), decay rates that are no power of two or 1, one to a hundred trials per line search, runs of 1 or 2 iterations, runs ended
by tol and runs ended by "Backtracking failed" - against the CPU oracle on the reference closures.

tests/test_margins_fuzz_cases.py has shown on the CPU that the oracle's decisions on every case of the fixed table do not
depend on the summation order, so a mismatch here is a finding about the product.  One test id is one case; it runs the sparse and
the dense class of the case against one oracle run.  The tolerances are those of the classes' own test_solve_vs_oracle (1e-10,
norm-relative for iterates, element by element for allfuns and allerrs).

ZF_FUZZ_SCALE=k appends k - 1 further blocks of seeds (a one-off soak).  Those lie outside the CPU-checked table: a case of theirs
whose two CPU evaluations disagree is dropped while the ids are collected."""
import os
import warnings

import numpy as np
import pytest

import margins_fuzz_cases as M
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-10
SCALE = int(os.environ.get("ZF_FUZZ_SCALE", "1"))
TABLE = M.TABLE + [c for k in range(1, SCALE) for c in M.extra_block(k)]
SPECS = [M.draw(cls, seed) for cls, seed in TABLE]
SWITCHES = ("ZF_LS_SMALL", "ZF_GEMV_MFMA", "ZF_ACCEPT")   # would select other kernels / another acceptance test than the table says
FULL = dict(max_iter_internal=100000, warm_start=False, verbose=False, return_all=False)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture
def solve(monkeypatch):
    """minimize_proximal_gradient on the native path; returns (result, trace rows of every accepted iteration, ls_plan)."""
    from zfista_amd import minimize_proximal_gradient, proximal_gradient as pg

    seen = []

    class _Recorded(pg.NativeRun):
        def __init__(self, *a, **k):
            self.rows = []
            super().__init__(*a, **k)
            self.plan = self.solver.ls_plan()
            seen.append(self)

        def collect(self):
            rows = super().collect()
            self.rows.append(rows)
            return rows

    monkeypatch.setattr(pg, "NativeRun", _Recorded)

    def run(prob, x0, **kw):
        del seen[:]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = minimize_proximal_gradient(*prob.callbacks(), x0, **kw)
        assert len(seen) == 1, "the solve did not run on the native path"
        return res, np.concatenate(seen[0].rows), seen[0].plan

    return run


def _drain(run, chunk=3):
    """Advance a NativeRun to its end in chunks of ``chunk`` passes: (trace rows, number of chunks)."""
    from zfista_amd import _lib

    rows, chunks = [np.zeros((0, _lib.ZF_TRACE_COLS))], 0
    while run.status == _lib.ZF_RUNNING:
        rows.append(run.advance(chunk))
        chunks += 1
    return np.concatenate(rows), chunks


def _check_trace(rows, exp):
    from zfista_amd import _lib

    assert len(rows) == exp.nit == len(exp.alllrs)
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float))
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), np.asarray(exp.alltrials, np.int64))


def _check_storage(case, storage, o, exp, solve, cases=M, keep=None):
    """Both solves and the chunked run of one storage form against the oracle's result; returns the lr / trial columns.
    ``cases``: the table module the case comes from (its make_problem and dense_form); ``keep``: a dict that receives the
    problem, what the two solves returned and the solver's ls_plan, for a caller with further checks on them."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    spec, x0 = case.spec, case.x0
    prob = cases.make_problem(case, storage)
    res, rows, plan = solve(prob, x0, return_all=True, **o)
    res1, rows1, plan1 = solve(prob, x0, return_all=False, **o)
    if keep is not None:
        keep.update(prob=prob, res=res, rows=rows, res1=res1, rows1=rows1, plan=plan)
    assert plan == plan1 and plan[0] == (M.CSR if storage == "csr" else cases.dense_form(spec)), (plan, plan1)
    ref_keys = set(exp.keys()) - {"alllrs", "alltrials"}       # (the oracle's two extra fields)
    for r, tr in ((res, rows), (res1, rows1)):
        assert r.success == exp.success and r.message == exp.message, (r.message, exp.message)
        assert r.nit == exp.nit
        assert ("status" in r) == ("status" in exp) and r.get("status") == exp.get("status")
        assert set(r.keys()) - {"overrides", "runahead"} == ref_keys
        assert rel_err(r.x, exp.x) <= TOL
        np.testing.assert_allclose(r.fun, exp.fun, rtol=TOL, atol=0)
        _check_trace(tr, exp)
        if M.ending(exp) == "error":
            # the error-shaped result (proximal_gradient.py:493-509): x is x_{k-1} - x0 itself, bit for bit, when the first line
            # search fails
            assert not r.success and r.message.startswith("Error: Backtracking failed") and "status" not in r
            if exp.nit == 0:
                assert np.array_equal(_bits(r.x), _bits(x0)) and np.array_equal(_bits(exp.x), _bits(x0))
    assert np.array_equal(_bits(res1.x), _bits(res.x)), "return_all must not change the iterate"
    assert res1.allvecs is None and res1.allfuns is None and res1.allerrs is None
    # every iterate, F and err of the return_all solve
    assert len(res.allvecs) == len(exp.allvecs) == exp.nit + 1 and len(res.allfuns) == exp.nit + 1 and len(res.allerrs) == exp.nit
    assert np.array_equal(_bits(res.allvecs[0]), _bits(x0)) and np.array_equal(_bits(res.allvecs[exp.nit]), _bits(res.x))
    assert max(rel_err(a, e) for a, e in zip(res.allvecs, exp.allvecs)) <= TOL
    # F(x0) = inf where x0 lies outside the box, in the reference (its g returns inf) and here (zf_solver.hip: a violated bound makes
    # g INFINITY; DESIGN.md 4.4 names the consequence - the first trial is accepted whatever it is); inf == inf below
    assert np.isinf(exp.allfuns[0]) == M.outside_box(case)
    np.testing.assert_allclose(res.allfuns, exp.allfuns, rtol=TOL, atol=0)
    if exp.nit:
        assert rel_err(res.allerrs, exp.allerrs) <= TOL
        xnorm = max(float(np.linalg.norm(v)) for v in exp.allvecs)
        np.testing.assert_allclose(res.allerrs, exp.allerrs, rtol=TOL, atol=2 * TOL * xnorm)
    # the trace ring of a run advanced in chunks of 3 passes
    run = NativeRun(prob, x0, FULL | o)
    chunked, _ = _drain(run)
    x_chunked = run.solver.get_x()
    run.solver.close()
    _check_trace(chunked, exp)
    assert np.array_equal(chunked, rows1) and np.array_equal(_bits(x_chunked), _bits(res.x))
    return rows[:, [_lib.TR_LR, _lib.TR_TRIALS]]


@pytest.mark.parametrize("spec", SPECS, ids=[M.case_id(sp) for sp in SPECS])
def test_fuzz_margins(spec, solve):
    case, o, exp = M.oracle(spec)
    assert exp is not None
    csr = _check_storage(case, "csr", o, exp, solve)
    dense = _check_storage(case, "dense", o, exp, solve)
    assert np.array_equal(csr, dense), "the sparse and the dense class of a case take the same lr and trial sequences"


@pytest.mark.parametrize("kind", ["tol", "error"])
@pytest.mark.parametrize("cls", M.CLASSES)
def test_snapshot_resume_across_the_last_chunk(cls, kind, tmp_path):
    """The table's longest run of the class that ends by tol, and its longest that ends in the error path: a snapshot taken one
    chunk before the end, and the run resumed from it, end with the status, x and trace of the uninterrupted run."""
    spec = {(sp.cls, k): sp for sp, k in M.resume_cases()}[(cls, kind)]
    case, o, exp = M.oracle(spec)
    _check_resume(case, o, exp, kind, tmp_path)


def _check_resume(case, o, exp, kind, tmp_path, cases=M):
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    assert M.ending(exp) == kind
    want = {"tol": _lib.ZF_CONVERGED, "error": _lib.ZF_BACKTRACK_FAILED}[kind]
    for storage in cases.FORMS:   # (every table module has M.FORMS but the fp32 one, which has no CSR form)
        prob = cases.make_problem(case, storage)
        whole = NativeRun(prob, case.x0, FULL | o)
        ref_rows, chunks = _drain(whole)
        ref_x, ref_status = whole.solver.get_x(), whole.status
        whole.solver.close()
        assert ref_status == want and chunks >= 1
        _check_trace(ref_rows, exp)
        first = NativeRun(prob, case.x0, FULL | o)
        head = [first.advance(3) for _ in range(chunks - 1)]
        assert first.status == _lib.ZF_RUNNING
        state = first.snapshot()
        first.solver.close()
        np.savez(tmp_path / "ckpt.npz", **state)
        run = NativeRun.from_snapshot(prob, dict(np.load(tmp_path / "ckpt.npz")), FULL | o)
        tail, tail_chunks = _drain(run)
        assert tail_chunks == 1 and run.status == ref_status
        assert np.array_equal(np.concatenate(head + [tail]), ref_rows)
        assert np.array_equal(_bits(run.solver.get_x()), _bits(ref_x))
        run.solver.close()
