"""GPU: the elastic-net penalty g(x) = lam |x|_1 + (l2 / 2) |x|^2 (+ box) of the four margins classes.

(1) Element bits of the fused step (zf_trial_enet_kernel): one accepted iteration against the l1 sibling's, bit for bit.
(2) prox_wsum_g / g as callables.  (3) Solves against the reference's fixture G16 and against the CPU oracle on the closures
of tests/enet_cases.py; the shared machinery (return_all, sub_iters, snapshots, acceptance="remainder", lam = 0).
(4) The certificate: all ten outputs inside the bounds derived in tests/enet_cases.py; the live solver's gap.  (5) gap_tol and
the path.  (6) An l1 problem runs what it ran.

The least-squares classes take ``l2=`` in the constructor; the logistic classes (whose constructor parameters are fixed) through
``with_penalty``.  ZF_ENET_BOUNDS_RECORD=1 appends the worst error-to-bound ratio of every certificate case to
profiles/enet_gap_bounds.jsonl (any other value: to that path) - records, not thresholds."""
import json
import os
import warnings

import numpy as np
import pytest

import enet_cases as E
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-10
U = E.U
ALL = E.SMALL + [E.TALL]
_id = lambda c: f"{c[0]}x{c[1]}"


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _make(loss, storage, A, b, lam, l2, scale=None, bounds=None):
    """The device problem of one loss and storage form with the ridge weight l2."""
    from zfista_amd import problems as Z

    M = E.matrix(A, storage)
    scale = (E.LS_SCALE if loss == "ls" else E.LOGIT_SCALE) if scale is None else scale
    if loss == "ls":
        cls = Z.SparseLeastSquaresL1 if storage == "csr" else Z.LeastSquaresL1
        return cls(M, b, lam, scale=scale, bounds=bounds, l2=l2)
    cls = Z.SparseLogisticL1 if storage == "csr" else Z.LogisticL1
    prob = cls(M, b, lam, scale=scale, bounds=bounds)
    return prob.with_penalty(lam, l2) if l2 else prob


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.fixture
def solve(monkeypatch):
    """minimize_proximal_gradient on the native path; returns (result, trace rows of every accepted iteration, ls_plan, counts)."""
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
            self.counts = self.solver.launch_counts()   # (the solver is closed when the solve returns)
            return rows

    monkeypatch.setattr(pg, "NativeRun", _Recorded)

    def run(prob, x0, **kw):
        del seen[:]
        res = _quiet(minimize_proximal_gradient, *prob.callbacks(), x0, **kw)
        assert len(seen) == 1, "the solve did not run on the native path"
        return res, np.concatenate(seen[0].rows), seen[0].plan, seen[0].counts

    return run


# ---- (1) element bits of the fused step --------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", E.FORMS)
@pytest.mark.parametrize("loss", E.LOSSES)
@pytest.mark.parametrize("case", E.SMALL, ids=_id)
def test_one_iteration_is_the_l1_step_times_shrink_bit_for_bit(case, loss, storage, solve, monkeypatch):
    """max_iter = 1 from a random x0 of size 1e-3 (a fifth of it exact zeros: those elements end below the threshold, as zeros
    of both signs), lr = 2^-20, small enough that the first trial is accepted: with S = x_1 of the l1 sibling without a box,
    x_1 of the elastic-net solve is clip(S * shrink, lo, hi), shrink = 1.0 / (1.0 + l2 * lr), in every bit - for l2 = lam and
    for an l2 that makes shrink 1 / 1.3, without and with an active box, with 1 and with 3 tiles per workgroup."""
    from zfista_amd import _lib

    A, b, lam, scale = E.make_case(loss, case)
    n = A.shape[1]
    rng = np.random.default_rng(case[3] + 50)
    x0 = 1e-3 * rng.standard_normal(n)
    x0[rng.random(n) < 0.2] = 0.0
    lr = 2.0 ** -20
    kw = dict(lr=lr, tol=0.0, max_iter=1, nesterov=True, return_all=False)
    box = (-5e-4, 7e-4)
    l1 = _make(loss, storage, A, b, lam, 0.0)
    for tiles in ("1", "3"):
        monkeypatch.setenv("ZF_TILES_PER_WG", tiles)
        base, rows, _, _ = solve(l1, x0, **kw)
        assert rows[:, _lib.TR_TRIALS].tolist() == [1.0]
        S = base.x
        assert np.count_nonzero(S == 0.0) >= 5 and np.signbit(S[S == 0.0]).any() and not np.signbit(S[S == 0.0]).all()
        for l2 in (lam, 0.3 / lr):
            shrink = 1.0 / (1.0 + l2 * lr)
            for bounds in (None, box):
                res, rows, plan, _ = solve(_make(loss, storage, A, b, lam, l2, bounds=bounds), x0, **kw)
                assert rows[:, _lib.TR_TRIALS].tolist() == [1.0] and res.nit == 1
                want = S * shrink
                if bounds is not None:
                    want = np.clip(want, *bounds)
                    assert np.count_nonzero(want == box[0]) >= 5 and np.count_nonzero(want == box[1]) >= 5, "the box must be active"
                bad = np.flatnonzero(_bits(res.x) != _bits(want))
                assert bad.size == 0, (tiles, l2, bounds, bad[:8], res.x[bad[:8]], want[bad[:8]])
                assert plan[0] != 1, "an elastic-net solve never takes the fused small-matrix path"
                if (tiles, bounds) == ("1", None):   # the reported F is f(x_1) + g(x_1) with the ridge term
                    F1 = float(l1.f(res.x)) + float(E.g_longdouble(res.x, lam, l2))
                    assert abs(float(res.fun) - F1) <= 1e-12 * abs(F1)


# ---- (2) the callables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,storage", [("ls", "dense"), ("logit", "csr")])
def test_prox_matches_the_numpy_closure_bit_for_bit_and_g_its_bound(loss, storage):
    from oracle import problems_ref as P

    A, b, lam, scale = E.make_case(loss, E.SMALL[2])   # n = 257: an odd tail
    n = A.shape[1]
    rng = np.random.default_rng(3)
    v = 0.05 * rng.standard_normal(n)
    v[:9] = [0.0, -0.0, np.nan, np.inf, -np.inf, 1e-320, -1e-320, 1e300, -1e300]
    for lam_k, l2 in ((lam, lam), (lam, 37.5), (0.0, 0.25), (lam, 0.01 * lam)):
        for bounds in (None, (-0.02, 0.03)):
            prob = _make(loss, storage, A, b, lam_k, l2, bounds=bounds)
            for w in (1.0, 0.37, 2.0 ** -20):
                with np.errstate(invalid="ignore"):
                    want = P.soft_threshold(v, lam_k * w) * (1.0 / (1.0 + l2 * w))
                    if bounds is not None:
                        want = P.clip_box(want, *bounds)
                got = prob.prox_wsum_g(w, v)
                bad = np.flatnonzero((_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want)))
                assert bad.size == 0 and np.array_equal(np.isnan(got), np.isnan(want)), (lam_k, l2, bounds, w, bad[:8], got[bad[:8]], want[bad[:8]])
            # g: n terms of two fused multiply-adds each, summed in some order: (n + 4) u relative to g (every term >= 0)
            for x in (0.05 * rng.standard_normal(n), np.zeros(n), np.full(n, 0.01)):
                if bounds is not None:
                    x = np.clip(x, *bounds)
                exact = E.g_longdouble(x, lam_k, l2)
                assert abs(float(np.longdouble(prob.g(x)) - exact)) <= (n + 4) * U * float(exact)
            if bounds is not None:
                x = np.zeros(n)
                x[n - 1] = 0.031
                assert prob.g(x) == np.inf and prob.g(-x) == np.inf and np.isfinite(prob.g(0.9 * x))


# ---- (3) solves --------------------------------------------------------------------------------------------------------------
def _check_solve(res, rows, exp):
    """tests/test_gpu_logistic.py's criteria: equal nit, status and trial / lr sequences; iterates, allfuns, allerrs to 1e-10."""
    from zfista_amd import _lib

    assert res.nit == exp.nit and bool(res.success) == bool(exp.success)
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), np.asarray(exp.alltrials, np.int64))
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float))
    assert rel_err(res.x, exp.x) <= TOL
    assert len(res.allvecs) == len(exp.allvecs) == exp.nit + 1
    worst = max(rel_err(a, e) for a, e in zip(res.allvecs, exp.allvecs))
    print(f"nit {res.nit}, trials {int(rows[:, _lib.TR_TRIALS].sum())}: iterates within {worst:.3g}, "
          f"allfuns within {np.max(np.abs(np.asarray(res.allfuns) - exp.allfuns) / np.abs(exp.allfuns)):.3g}, "
          f"allerrs within {rel_err(res.allerrs, exp.allerrs):.3g}")
    assert worst <= TOL
    np.testing.assert_allclose(res.allfuns, exp.allfuns, rtol=TOL, atol=0)
    assert rel_err(res.allerrs, exp.allerrs) <= TOL
    xnorm = max(float(np.linalg.norm(v)) for v in exp.allvecs)
    np.testing.assert_allclose(res.allerrs, exp.allerrs, rtol=TOL, atol=2 * TOL * xnorm)


@pytest.mark.parametrize("tag", list(E.GOLDEN_VARIANTS))
@pytest.mark.parametrize("storage", E.FORMS)
@pytest.mark.parametrize("fi", range(len(E.L2_FACTORS)))
@pytest.mark.parametrize("ci", range(len(E.SMALL)))
@pytest.mark.parametrize("loss", E.LOSSES)
def test_solve_vs_reference_fixture(golden, loss, ci, fi, storage, tag, solve):
    """80 iterations from lr = 1 against what the REFERENCE solver produced on the closures (tests/golden/make_golden_enet.py)."""
    from zfista_amd import _lib

    G = golden("g16_enet.npz")
    A, b, lam, scale = E.make_case(loss, E.SMALL[ci])
    assert lam == float(G(f"{loss}.c{ci}.lam"))
    res, rows, plan, _ = solve(_make(loss, storage, A, b, lam, E.L2_FACTORS[fi] * lam), np.zeros(A.shape[1]), **E.GOLDEN_KW, **E.GOLDEN_VARIANTS[tag])
    pre = E.golden_prefix(loss, ci, fi, storage, tag)
    assert plan[0] == 5 if storage == "csr" else plan[0] in (2, 3, 4)
    assert res.nit == int(G(f"{pre}.nit")) == 80
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), G(f"{pre}.alltrials")) and rows[:, _lib.TR_TRIALS].sum() > 80
    assert np.array_equal(rows[:, _lib.TR_LR], G(f"{pre}.alllrs"))
    assert rel_err(res.x, G(f"{pre}.x")) <= TOL
    assert abs(np.linalg.norm(res.x) - float(G(f"{pre}.xnorm"))) <= TOL * float(G(f"{pre}.xnorm"))
    for k, v in zip(G(f"{pre}.kept"), G(f"{pre}.vecs")):
        assert rel_err(res.allvecs[k][::E.GOLDEN_STRIDE], v) <= TOL, k
    np.testing.assert_allclose(res.allfuns, G(f"{pre}.allfuns"), rtol=TOL, atol=0)
    assert rel_err(res.allerrs, G(f"{pre}.allerrs")) <= TOL
    np.testing.assert_allclose(res.allerrs, G(f"{pre}.allerrs"), rtol=TOL, atol=2 * TOL * float(G(f"{pre}.xnorm")))


_ORACLE = {}
VARIANTS = {
    "fista-l2-lam": dict(nesterov=True, fac=1.0),
    "ista-l2-lam-100th": dict(nesterov=False, fac=0.01),
    "momentum-half-16th-box": dict(nesterov=True, nesterov_ratio=(0.5, 1 / 16), fac=1.0, bounds=(-0.05, 0.3)),
    "ridge-only": dict(nesterov=True, fac=1.0, lam0=True),   # lam = 0: g = (l2 / 2) |x|^2, l2 = the case's lam
}


def _oracle(loss, case, variant):
    """The CPU oracle on the closures over the CSR matrix (one run per loss, case and variant, shared by both storage forms)."""
    from oracle import cpu_ref

    key = (loss, case, variant)
    if key not in _ORACLE:
        A, b, lam, scale = E.make_case(loss, case)
        v = dict(VARIANTS[variant])
        l2 = v.pop("fac") * lam
        ref = E.EnetRef(loss, A, b, 0.0 if v.pop("lam0", False) else lam, l2, scale, bounds=v.pop("bounds", None))
        _ORACLE[key] = _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), np.zeros(A.shape[1]), lr=1, tol=0.0, max_iter=80,
                              return_all=True, **v)
    return _ORACLE[key]


@pytest.mark.parametrize("storage", E.FORMS)
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("loss", E.LOSSES)
@pytest.mark.parametrize("case", [E.SMALL[0], E.SMALL[3], E.TALL], ids=_id)
def test_solve_vs_oracle(case, loss, variant, storage, solve):
    """The variants the fixture does not hold - another momentum ratio inside an active box, lam = 0 (pure ridge) - and the
    tall case (the many-workgroup residual / loss kernels), every iterate against the oracle."""
    A, b, lam, scale = E.make_case(loss, case)
    v = dict(VARIANTS[variant])
    l2, lam_k, bounds = v.pop("fac") * lam, (0.0 if v.pop("lam0", False) else lam), v.pop("bounds", None)
    exp = _oracle(loss, case, variant)
    res, rows, plan, _ = solve(_make(loss, storage, A, b, lam_k, l2, bounds=bounds), np.zeros(A.shape[1]), lr=1, tol=0.0, max_iter=80,
                               return_all=True, **v)
    assert exp.nit == 80 and sum(exp.alltrials) > 80
    _check_solve(res, rows, exp)
    if bounds is not None:
        assert res.x.min() >= bounds[0] and res.x.max() <= bounds[1] and np.count_nonzero((res.x == bounds[0]) | (res.x == bounds[1])) >= 3
    if lam_k == 0.0:
        assert np.count_nonzero(res.x) > 0.9 * np.count_nonzero(np.diff(A.T.tocsr().indptr)), "a ridge solution is dense"


@pytest.mark.parametrize("loss", E.LOSSES)
@pytest.mark.parametrize("case", ALL, ids=_id)
def test_dense_and_sparse_classes_take_the_same_trials(case, loss, solve):
    from zfista_amd import _lib

    A, b, lam, scale = E.make_case(loss, case)
    kw = dict(lr=1, tol=0.0, max_iter=80, nesterov=True, return_all=True)
    rs, rows_s, plan_s, _ = solve(_make(loss, "csr", A, b, lam, lam), np.zeros(A.shape[1]), **kw)
    rd, rows_d, plan_d, _ = solve(_make(loss, "dense", A, b, lam, lam), np.zeros(A.shape[1]), **kw)
    assert plan_s[0] == 5 and plan_d[0] in (2, 3, 4)
    assert rs.nit == rd.nit == 80 and rows_s[:, _lib.TR_TRIALS].sum() > 80
    assert np.array_equal(rows_s[:, _lib.TR_TRIALS], rows_d[:, _lib.TR_TRIALS]) and np.array_equal(rows_s[:, _lib.TR_LR], rows_d[:, _lib.TR_LR])
    assert max(rel_err(a, e) for a, e in zip(rs.allvecs, rd.allvecs)) <= TOL
    np.testing.assert_allclose(rs.allfuns, rd.allfuns, rtol=TOL, atol=0)


@pytest.mark.parametrize("storage", E.FORMS)
@pytest.mark.parametrize("loss", E.LOSSES)
def test_bit_reproducible_and_sub_iters_and_return_all(loss, storage, solve):
    """Two solves give the same bits; sub_iters changes nothing; a solve without return_all (the kernel without the history
    ring) ends at the same bits as the recording one."""
    A, b, lam, scale = E.make_case(loss, E.SMALL[1])
    n = A.shape[1]
    kw = dict(lr=1, tol=0.0, max_iter=60, nesterov=True, return_all=True)
    r1, rows1, p1, c1 = solve(_make(loss, storage, A, b, lam, lam), np.zeros(n), **kw)
    assert len(r1.allvecs) == 61 and np.array_equal(r1.allvecs[-1], r1.x) and np.array_equal(r1.allvecs[0], np.zeros(n))
    for extra in ({}, dict(sub_iters=1), dict(sub_iters=4), dict(sub_iters=16), dict(return_all=False)):
        r2, rows2, p2, _ = solve(_make(loss, storage, A, b, lam, lam), np.zeros(n), **dict(kw, **extra))
        assert p1 == p2 and np.array_equal(r1.x, r2.x) and np.array_equal(rows1, rows2) and r1.fun == r2.fun, extra
        if dict(kw, **extra)["return_all"]:
            assert np.array_equal(np.asarray(r1.allvecs), np.asarray(r2.allvecs)) and np.array_equal(r1.allfuns, r2.allfuns)


_OPTS = dict(lr=1, tol=0.0, tol_internal=1e-12, max_iter=70, max_iter_internal=100000, max_backtrack_iter=100, warm_start=False,
             decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False, deprecated=False)


def _drain(run, step=5):
    from zfista_amd import _lib

    rows = [np.zeros((0, _lib.ZF_TRACE_COLS))]
    while run.status == _lib.ZF_RUNNING:
        rows.append(run.advance(step))
    return np.concatenate(rows)


@pytest.mark.parametrize("storage", E.FORMS)
@pytest.mark.parametrize("loss", E.LOSSES)
def test_snapshot_resume_is_bit_identical(loss, storage, tmp_path):
    """from_snapshot recreates the solver from the problem - which sets l2 again - and continues bit for bit."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    A, b, lam, scale = E.make_case(loss, E.SMALL[0])
    prob = _make(loss, storage, A, b, lam, lam)
    whole = NativeRun(prob, np.zeros(prob.n_features), _OPTS)
    ref_rows, ref_x = _drain(whole), whole.solver.get_x()
    whole.solver.close()
    assert len(ref_rows) == 70 and ref_rows[:, _lib.TR_TRIALS].sum() > 70
    for stop_after in (3, 20):   # inside the backtracking phase, and behind it
        first = NativeRun(prob, np.zeros(prob.n_features), _OPTS)
        head = [first.advance(1) for _ in range(stop_after)]
        state = first.snapshot()
        first.solver.close()
        np.savez(tmp_path / "ckpt.npz", **state)
        run = NativeRun.from_snapshot(prob, dict(np.load(tmp_path / "ckpt.npz")), _OPTS)
        rows = np.concatenate(head + [_drain(run)])
        assert np.array_equal(rows, ref_rows) and np.array_equal(run.solver.get_x(), ref_x), stop_after
        run.solver.close()


@pytest.mark.parametrize("storage", E.FORMS)
def test_acceptance_remainder(storage, solve):
    """R = scale |A (x+ - y)|^2 does not involve g: the remainder test decides as the reference's test does on a well-resolved
    solve - the same trial sequence, the same iterates bit for bit."""
    from zfista_amd import _lib

    A, b, lam, scale = E.make_case("ls", E.SMALL[0])
    kw = dict(lr=1, tol=0.0, max_iter=80, nesterov=True, return_all=True)
    ref, rows_ref, _, _ = solve(_make("ls", storage, A, b, lam, lam), np.zeros(A.shape[1]), **kw)
    rem, rows_rem, plan, _ = solve(_make("ls", storage, A, b, lam, lam), np.zeros(A.shape[1]), acceptance="remainder", **kw)
    assert rem.acceptance == "remainder" and rem.nit == 80 and plan[0] != 1
    assert np.array_equal(rows_ref[:, _lib.TR_TRIALS], rows_rem[:, _lib.TR_TRIALS]) and rows_rem[:, _lib.TR_TRIALS].sum() > 80
    assert np.array_equal(rem.x, ref.x) and np.array_equal(np.asarray(rem.allvecs), np.asarray(ref.allvecs))


# ---- (4) the certificate -----------------------------------------------------------------------------------------------------
def _record(**rec):
    where = os.environ.get("ZF_ENET_BOUNDS_RECORD", "")
    if where in ("", "0"):
        return
    path = os.path.join(ROOT, "profiles", "enet_gap_bounds.jsonl") if where == "1" else where
    with open(path, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


def _gap_bits(gp):
    return np.array([getattr(gp, k) for k in E.KEYS]).view(np.uint64)


@pytest.mark.parametrize("storage", E.FORMS)
@pytest.mark.parametrize("fi", range(len(E.L2_FACTORS)))
@pytest.mark.parametrize("loss", E.LOSSES)
@pytest.mark.parametrize("case", E.SMALL, ids=_id)
def test_every_output_within_its_rounding_bound(case, loss, fi, storage, solve):
    """problem.duality_gap(x) (zf_gap_eval_enet / zf_spmat_gap_eval_enet) at x = 0 and at the iterates 20 and 400 of a FISTA
    solve: all ten outputs inside the bounds of tests/enet_cases.py."""
    A, b, lam, scale = E.make_case(loss, case)
    l2 = E.L2_FACTORS[fi] * lam
    prob = _make(loss, storage, A, b, lam, l2)
    n = A.shape[1]
    res, _, _, _ = solve(prob, np.zeros(n), lr=1, tol=0.0, max_iter=400, nesterov=True, return_all=True)
    assert res.nit == 400
    gaps = []
    for k in (0, 20, 400):
        x = np.asarray(res.allvecs[k])
        vals, bounds, _ = E.gap_longdouble(A, b, x, lam, l2, scale, loss == "logit")
        got = prob.duality_gap(x)
        ratios = E.worst_ratio(got, vals, bounds)
        worst = max(ratios, key=ratios.get)
        print(f"{_id(case)} {loss} {storage} l2 = {E.L2_FACTORS[fi]} lam, x_{k}: worst error / bound {ratios[worst]:.3g} ({worst}); "
              f"gap {float(got.gap):.6g} alpha {float(got.alpha):.6g} ridge {float(got.ridge_gap):.3g}")
        _record(case=_id(case), loss=loss, storage=storage, l2_over_lam=E.L2_FACTORS[fi], iterate=k, worst=worst, ratio=ratios[worst],
                ratios=ratios, gap=float(got.gap))
        assert all(np.isfinite(getattr(got, key)) for key in E.KEYS), got
        assert ratios[worst] <= 1.0, (k, worst, ratios, got)
        assert got.gap >= 0 and got.rows_gap >= 0 and got.ridge_gap >= 0 and got.gap >= got.rows_gap + got.ridge_gap * (1 - 4 * U)
        gaps.append(float(got.gap))
    assert gaps[2] < gaps[1] < gaps[0]
    x = np.asarray(res.allvecs[400])
    assert np.array_equal(_gap_bits(prob.duality_gap(x)), _gap_bits(prob.duality_gap(x))), "two evaluations: the same bits"


_BASE = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=100000, max_backtrack_iter=100, nesterov=True,
             nesterov_ratio=(0, 0.25), deprecated=False, return_all=False, verbose=False)


def _walk(prob, passes, gap_after=()):
    """`passes` chunks of ONE pass each; a gap call after the chunks listed in gap_after."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    run = NativeRun(prob, np.zeros(prob.n_features), dict(_BASE))
    rows, gaps, after_reject = [np.zeros((0, _lib.ZF_TRACE_COLS))], {}, 0
    for k in range(passes):
        rows.append(run.advance(1))
        if k in gap_after:
            ctl = run.solver.ctl
            after_reject += int(ctl.trial > 0 and ctl.need_grad == 0)   # between a rejected trial and its retry
            gaps[k] = run.duality_gap()
    ctl, _ = run.solver.poll()
    out = dict(rows=np.concatenate(rows), x=run.solver.get_x(), nit=int(ctl.nit), lr=ctl.lr, F=ctl.F_old, trials=int(ctl.total_trials),
               gaps=gaps, after_reject=after_reject, counts=run.solver.launch_counts())
    run.solver.close()
    return out


@pytest.mark.parametrize("storage", E.FORMS)
@pytest.mark.parametrize("loss", E.LOSSES)
def test_the_gap_of_a_live_solve(loss, storage):
    """NativeRun.duality_gap() equals the standalone evaluation at get_x() bit for bit (the margins come from the same
    kernels: an elastic-net solve is always on the general path), and a solve probed after every pass - also between a
    rejected trial and its retry - is the solve that was never asked, bit for bit."""
    A, b, lam, scale = E.make_case(loss, E.SMALL[1])   # n = 5000: more than one gap chunk
    prob = _make(loss, storage, A, b, lam, lam)
    passes = 24
    plain = _walk(prob, passes)
    assert plain["trials"] > plain["nit"] > 0, "the case must backtrack and accept"
    probed = _walk(prob, passes, gap_after=range(passes))
    assert (plain["nit"], plain["lr"], plain["F"], plain["trials"]) == (probed["nit"], probed["lr"], probed["F"], probed["trials"])
    assert np.array_equal(plain["rows"], probed["rows"]) and np.array_equal(plain["x"], probed["x"])
    assert probed["after_reject"] >= 1, "no gap call fell between a rejected trial and its retry"
    assert plain["counts"] == probed["counts"]
    live, alone = probed["gaps"][passes - 1], prob.duality_gap(probed["x"])
    assert np.array_equal(_gap_bits(live), _gap_bits(alone)), (live, alone)
    vals, bounds, _ = E.gap_longdouble(A, b, probed["x"], lam, lam, scale, loss == "logit")
    ratios = E.worst_ratio(live, vals, bounds)
    assert max(ratios.values()) <= 1.0, ratios
    assert live.g_l2 > 0 and live.gap < probed["gaps"][0].gap


# ---- (5) stopping and the path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", E.FORMS)
@pytest.mark.parametrize("loss", E.LOSSES)
def test_gap_tol_stops_the_solve_with_a_valid_certificate(loss, storage):
    from zfista_amd import minimize_proximal_gradient as solve

    A, b, lam, scale = E.make_case(loss, E.SMALL[0])
    prob = _make(loss, storage, A, b, lam, lam)
    n = A.shape[1]
    logistic = loss == "logit"
    P0 = float(E.primal_longdouble(A, b, np.zeros(n), lam, lam, scale, logistic))
    gap_tol = 1e-6 * P0
    kw = dict(lr=1.0, nesterov=True, tol=0.0)
    res = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=4000, gap_tol=gap_tol, **kw)
    assert res.success and res.status == 1 and res.message == "Duality gap reached gap_tol" and res.nit < 4000
    assert 0 <= res.dual_gap <= gap_tol and res.dual_gap == prob.duality_gap(res.x).gap
    plain = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=res.nit, **kw)
    assert plain.nit == res.nit and np.array_equal(plain.x, res.x) and plain.fun == res.fun, "the keyword does not alter the iterates"
    # the certificate: P(x) - min P <= gap, with P(x_3000) >= min P standing in for the minimum
    far = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=3000, **kw)
    assert far.nit == 3000
    excess = E.primal_longdouble(A, b, res.x, lam, lam, scale, logistic) - E.primal_longdouble(A, b, far.x, lam, lam, scale, logistic)
    print(f"{loss} {storage}: stopped at nit {res.nit}, gap {float(res.dual_gap):.3g} <= {gap_tol:.3g}; P(x) - P(x_3000) = {float(excess):.3g}")
    assert np.longdouble(res.dual_gap) >= excess


@pytest.mark.parametrize("loss,storage", [("ls", "csr"), ("logit", "dense")])
def test_l1_path_with_l2(loss, storage):
    from zfista_amd import minimize_proximal_gradient as solve
    from zfista_amd.path import l1_path

    A, b, lam, scale = E.make_case(loss, E.SMALL[0])
    prob = _make(loss, storage, A, b, lam, 0.0)
    n = prob.n_features
    lam_max = float(prob.lam_max())
    assert lam_max == float(prob.with_penalty(lam, lam).lam_max()), "the ridge term vanishes at 0"
    lams = [lam_max * f for f in (1.0000001, 0.7, 0.5, 0.35, 0.25)]
    l2s = [0.5 * v for v in lams]
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=3000)
    gap_tol = 1e-5 * float(prob.with_penalty(lams[-1], l2s[-1]).duality_gap(np.zeros(n)).primal)
    for l2 in (l2s, l2s[2]):
        path = _quiet(l1_path, prob, lams, gap_tol=gap_tol, l2=l2, **kw)
        each = l2 if isinstance(l2, list) else [l2] * 5
        assert [r.lam for r in path] == lams and [r.l2 for r in path] == each
        x = np.zeros(n)
        for lam_k, l2_k, r in zip(lams, each, path):
            sib = prob.with_penalty(lam_k, l2_k)
            assert sib.b.data_ptr() == prob.b.data_ptr() and (sib._spmat is prob._spmat if storage == "csr" else sib.A.data_ptr() == prob.A.data_ptr())
            alone = _quiet(solve, *sib.callbacks(), x, gap_tol=gap_tol, **kw)
            assert alone.nit == r.nit and np.array_equal(alone.x, r.x) and alone.dual_gap == r.dual_gap and r.success and r.dual_gap <= gap_tol
            x = r.x
        assert not path[0].x.any() and np.count_nonzero(path[-1].x) > np.count_nonzero(path[1].x) >= 1
    assert prob.l2 == 0.0 and prob.lam == lam
    # l2 = None keeps the problem's own ridge weight
    own = _quiet(l1_path, prob.with_penalty(lam, l2s[2]), lams[:3], gap_tol=gap_tol, **kw)
    assert all(np.array_equal(a.x, c.x) for a, c in zip(own, path[:3]))
    # restrict carries l2
    keep = np.arange(0, n, 2)
    sub = prob.with_penalty(lam, 0.25).restrict(keep)
    assert sub.l2 == 0.25 and sub.n_features == keep.size
    xs = 0.01 * np.random.default_rng(0).standard_normal(keep.size)
    assert abs(float(np.longdouble(sub.g(xs)) - E.g_longdouble(xs, lam, 0.25))) <= (keep.size + 4) * U * float(E.g_longdouble(xs, lam, 0.25))


# ---- (6) nothing moved -------------------------------------------------------------------------------------------------------
def test_an_l1_problem_runs_what_it_ran(solve):
    """l2 = 0 - by default, by the keyword, by with_penalty, by zf_solver_set_l2(0) - takes the l1 paths: the plan, the launch
    counts and the bits of the problem that was never asked; the same matrix with l2 > 0 leaves the fused small-matrix path."""
    from oracle import problems_ref as P
    from zfista_amd.engine import DeviceSolver
    from zfista_amd.problems import DiagQuadL1, LeastSquaresL1

    A, b, lam = P.make_plasso(512, 1024, seed=0)
    kw = dict(lr=1, tol=0.0, max_iter=40, nesterov=True)
    plain, rows0, plan0, counts0 = solve(LeastSquaresL1(A, b, lam), np.zeros(1024), **kw)
    assert plan0[:2] == (1, 1), "the fused small-matrix path"
    for prob in (LeastSquaresL1(A, b, lam, l2=0.0), LeastSquaresL1(A, b, lam).with_penalty(lam, 0.0), LeastSquaresL1(A, b, lam, l2=0.3).with_penalty(lam, 0)):
        r, rows, plan, counts = solve(prob, np.zeros(1024), **kw)
        assert plan == plan0 and counts == counts0 and np.array_equal(rows, rows0) and np.array_equal(r.x, plain.x)
        assert np.array_equal(_bits(prob.prox_wsum_g(0.5, plain.x)), _bits(LeastSquaresL1(A, b, lam).prox_wsum_g(0.5, plain.x)))
        assert prob.g(plain.x) == LeastSquaresL1(A, b, lam).g(plain.x)
        assert len(prob.duality_gap(plain.x).__slots__) == 10 and prob.duality_gap(plain.x).g_l2 == 0.0
    enet, _, plan1, counts1 = solve(LeastSquaresL1(A, b, lam, l2=lam), np.zeros(1024), **kw)
    assert plan1[:2] == (2, 2), "the general path (n % 32 == 0: the MFMA column sweep)"
    assert counts1 == counts0, "the counts are those of the separable kind's shape kernels: none here, before and after"
    assert enet.nit == 40 and not np.array_equal(enet.x, plain.x)
    # the library: l2 = 0 keeps the plan; refusals
    options = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=3, max_backtrack_iter=10)
    fields, keep = LeastSquaresL1(A, b, lam)._descriptor()
    s = DeviceSolver(fields, options, keepalive=keep)
    lib = s.lib
    assert lib.zf_solver_set_l2(s.handle, 0.0) == 0 and s.ls_plan()[0] == 1
    for bad in (-1.0, float("inf"), float("nan")):
        assert lib.zf_solver_set_l2(s.handle, bad) == -2 and b"finite" in lib.zf_last_error()   # ZF_ERR_ARG
    assert lib.zf_solver_set_l2(s.handle, 0.5) == 0 and s.ls_plan()[0] == 2
    import torch

    x0 = torch.zeros(1024, dtype=torch.float64, device="cuda")
    s.init(x0.data_ptr())
    assert lib.zf_solver_set_l2(s.handle, 0.25) == -3 and b"before" in lib.zf_last_error()   # ZF_ERR_STATE
    s.close()
    d, c, lam_d = P.make_pdiag(1000, seed=1)
    fields, keep = DiagQuadL1(d, c, lam_d)._descriptor()
    s = DeviceSolver(fields, options, keepalive=keep)
    assert lib.zf_solver_set_l2(s.handle, 0.5) == -2 and b"only for" in lib.zf_last_error()
    s.close()
