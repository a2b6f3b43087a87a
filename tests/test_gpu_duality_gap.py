"""GPU: duality-gap certificates (csrc/zf_kernels_gap.h), gap-based stopping and the l1 path.

(1) Element-wise accuracy.  ``problem.duality_gap(x)`` (zf_gap_eval / zf_spmat_gap_eval) against the np.longdouble
restatement of tests/gap_cases.py on the four SMALL matrices of tests/sparse_cases.py (a dense row, a dense column, an
empty row, an empty column), as CSR and as .toarray(), for both losses, at alpha = 1 (lam = 2 |g|_inf), alpha = 1/2
and x = 0.  Every one of the eight outputs is held to the rounding bound derived in the docstring of tests/gap_cases.py from
the operation counts (u = 2^-53; margins gamma_n |A| |x|, the loss kernels' documented ulps, sums of m or n terms in any
order, first order with a safety factor 2).  The bound on ``gap`` is d(rows) + d(cols) + u gap: it is written in the
gap's own terms - (1 - alpha)^2 |r|^2, the two parts q alpha log alpha and (1 - alpha q) L of every KL term, lam |x_j| and
alpha g_j x_j of every column term - and holds no term of the size of P.  The worst error-to-bound ratio of every case is
asserted <= 1; ZF_GAP_BOUNDS_RECORD=1 appends it to profiles/duality_gap_bounds.jsonl (any other value: to that path).
(2) Shape thresholds: m around ZF_SPMV_WIDE_RESID_MIN_ROWS, n around ZF_GAP_ONE_WG_MAX_N, n = 1, n beyond 2048 * 1024 (chunks
longer than 2048).  (3) Special values.  (4) The gap of a live solver.  (5) gap_tol.  (6) l1_path.  (7) Refusals."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import gap_cases as G
import logistic_cases as L
import sparse_cases as S
from conftest import ROOT

pytestmark = pytest.mark.gpu
WIDE = 1 << 15      # ZF_SPMV_WIDE_RESID_MIN_ROWS, restated
ONE_WG = 4096       # ZF_GAP_ONE_WG_MAX_N, restated
BASE = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=100000, max_backtrack_iter=100, nesterov=True,
            nesterov_ratio=(0, 0.25), deprecated=False, return_all=False, verbose=False)


def _cls(logistic, storage):
    from zfista_amd import problems as Z

    return {(False, "dense"): Z.LeastSquaresL1, (False, "csr"): Z.SparseLeastSquaresL1,
            (True, "dense"): Z.LogisticL1, (True, "csr"): Z.SparseLogisticL1}[(bool(logistic), storage)]


def _make(A, b, lam, logistic, storage, scale=None):
    scale = (1.0 if logistic else 0.5) if scale is None else scale
    return _cls(logistic, storage)(A if storage == "csr" else A.toarray(), b, lam, scale=scale)


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _record(**rec):
    where = os.environ.get("ZF_GAP_BOUNDS_RECORD", "")
    if where in ("", "0"):
        return
    path = os.path.join(ROOT, "profiles", "duality_gap_bounds.jsonl") if where == "1" else where
    with open(path, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


def _bits(gp):
    return np.array([getattr(gp, k) for k in G.KEYS]).view(np.uint64)


def _labels(m, seed):
    return np.where(np.random.default_rng(seed).random(m) < 0.5, -1.0, 1.0)


def _rand(m, n, nnz, seed):
    rng = np.random.default_rng(seed)
    flat = rng.choice(m * n, size=nnz, replace=False)
    A = sp.csr_matrix((rng.standard_normal(nnz), (flat // n, flat % n)), shape=(m, n))
    A.sort_indices()
    return A


def _held(case, prob, A, b, x, lam, scale, logistic, **tags):
    """prob.with_lam(lam).duality_gap(x) inside every bound; returns it."""
    vals, bounds, _ = G.gap_longdouble(A, b, x, lam, scale, logistic)
    got = prob.with_lam(lam).duality_gap(x)
    ratios = G.worst_ratio(got, vals, bounds)
    worst = max(ratios, key=ratios.get)
    print(f"{case} {tags}: worst error / bound {ratios[worst]:.3g} ({worst}); gap {float(got.gap):.6g} alpha {float(got.alpha):.6g}")
    _record(case=case, lam=float(lam), scale=scale, logistic=bool(logistic), worst=worst, ratio=ratios[worst], ratios=ratios, **tags)
    assert all(np.isfinite(getattr(got, k)) for k in G.KEYS), got
    assert ratios[worst] <= 1.0, (worst, ratios, got)
    assert got.gap >= 0 and got.rows_gap >= 0
    return got


# ---- (1) element-wise accuracy -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["csr", "dense"])
@pytest.mark.parametrize("logistic", [False, True], ids=["ls", "logistic"])
@pytest.mark.parametrize("case", range(4))
def test_every_output_within_its_rounding_bound(case, logistic, storage):
    if logistic:
        A, b, lam0 = L.make_logistic(*L.SMALL[case])
    else:
        A, b, lam0 = S.make_sparse(*S.SMALL[case])
    m, n = A.shape
    for scale in ((1.0, 1 / 3) if logistic else (0.5, 1 / 6)):
        prob = _make(A, b, lam0, logistic, storage, scale)
        rng = np.random.default_rng(100 + case)
        x = rng.standard_normal(n) * (rng.random(n) < 0.05)
        name = f"small-{m}x{n}"
        tags = dict(storage=storage, shape=[m, n])
        for xv, xname in ((x, "x"), (np.zeros(n), "zero")):
            G0 = float(G.gap_longdouble(A, b, xv, 1.0, scale, logistic)[0]["grad_inf"])
            got = _held(name, prob, A, b, xv, 2.0 * G0, scale, logistic, point=xname, alpha="1", **tags)
            assert got.alpha == 1.0 and got.rows_gap == 0.0, "alpha = 1: every row term is exactly 0"
            if xname == "zero":
                assert got.gap == 0.0 and got.g_l1 == 0.0 and got.primal == got.f
            got = _held(name, prob, A, b, xv, 0.5 * G0, scale, logistic, point=xname, alpha="1/2", **tags)
            assert abs(got.alpha - 0.5) < 1e-12 and got.rows_gap > 0
            _held(name, prob, A, b, xv, lam0 * scale / (1.0 if logistic else 0.5), scale, logistic, point=xname, alpha="lam0", **tags)
        # lam_max: |grad f(0)|_inf, the smallest lam for which x = 0 is optimal
        at0 = G.gap_longdouble(A, b, np.zeros(n), 1.0, scale, logistic)
        assert abs(float(np.longdouble(prob.lam_max()) - at0[0]["grad_inf"])) <= at0[1]["grad_inf"]
        assert prob.with_lam(np.nextafter(prob.lam_max(), np.inf)).duality_gap(np.zeros(n)).gap == 0.0
        # the bound holds no term of the size of P: close to the origin under alpha = 1 the gap is its column part, of the size
        # of lam |x|_1, and the bound stays below ONE rounding of P - what forming P - D would lose at the least
        xs = 1e-8 * x
        lam_s = 2.0 * float(G.gap_longdouble(A, b, xs, 1.0, scale, logistic)[0]["grad_inf"])
        vals, bounds, _ = G.gap_longdouble(A, b, xs, lam_s, scale, logistic)
        assert 0 < bounds["gap"] < 2.0 ** -53 * float(vals["primal"]) and float(vals["gap"]) < 1e-5 * float(vals["primal"])
        _held(name, prob, A, b, xs, lam_s, scale, logistic, point="1e-8 x", alpha="1", **tags)


# ---- (2) shape thresholds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logistic", [False, True], ids=["ls", "logistic"])
@pytest.mark.parametrize("m", [WIDE - 1, WIDE, WIDE + 1])
def test_row_count_thresholds_and_equal_row_sums_of_both_storage_forms(m, logistic):
    """One below, at and one above ZF_SPMV_WIDE_RESID_MIN_ROWS (n = 64, three stored elements per row), inside the bounds.
    Then a matrix and a point with DYADIC entries - every margin is exact in fp64 whatever the sweep - at alpha = 1: f and
    the dual value are pure row sums then (least squares: sum r^2 and sum b r; logistic: the loss and the entropies), and
    their order is a function of m alone: the dense and the CSR class give the same bits."""
    n = 64
    A = _rand(m, n, 3 * m, m)
    rng = np.random.default_rng(m + 2)
    x = rng.standard_normal(n)
    b = _labels(m, m + 1) if logistic else rng.standard_normal(m)
    scale = 1.0 if logistic else 0.5
    for storage in ("csr", "dense"):
        prob = _make(A, b, 1.0, logistic, storage)
        G0 = float(G.gap_longdouble(A, b, x, 1.0, scale, logistic)[0]["grad_inf"])
        for frac in (2.0, 0.5):
            _held(f"rows-{m}", prob, A, b, x, frac * G0, scale, logistic, storage=storage, shape=[m, n], alpha=str(frac))
    Ad = A.copy()
    Ad.data = np.round(Ad.data * 8) / 8
    xd = np.round(x * 8) / 8
    bd = b if logistic else np.round(b * 8) / 8
    outs = {}
    for storage in ("csr", "dense"):
        outs[storage] = _make(Ad, bd, 1e9, logistic, storage).duality_gap(xd)
        assert outs[storage].alpha == 1.0 and outs[storage].rows_gap == 0.0
    assert outs["csr"].f == outs["dense"].f and outs["csr"].dual == outs["dense"].dual, (outs["csr"], outs["dense"])
    assert outs["csr"].g_l1 == outs["dense"].g_l1 and outs["csr"].primal == outs["dense"].primal


@pytest.mark.parametrize("logistic", [False, True], ids=["ls", "logistic"])
@pytest.mark.parametrize("n", [1, 777, ONE_WG - 1, ONE_WG, ONE_WG + 1, 3 * 2048 + 5])
def test_column_count_thresholds(n, logistic):
    """n one below, at and one above the size that switches |g|_inf and the column pass from one workgroup to several; n no
    multiple of the block; n = 1."""
    m = 50
    A = _rand(m, n, min(m * n, 4 * max(n, m)), n)
    rng = np.random.default_rng(n + 7)
    x = rng.standard_normal(n)
    b = _labels(m, n) if logistic else rng.standard_normal(m)
    scale = 1.0 if logistic else 0.5
    G0 = float(G.gap_longdouble(A, b, x, 1.0, scale, logistic)[0]["grad_inf"])
    for storage in ("csr", "dense"):
        prob = _make(A, b, 1.0, logistic, storage)
        for frac in (2.0, 0.5):
            a = _held(f"cols-{n}", prob, A, b, x, frac * G0, scale, logistic, storage=storage, shape=[m, n], alpha=str(frac))
            again = prob.with_lam(frac * G0).duality_gap(x)
            assert np.array_equal(_bits(a), _bits(again)), "two evaluations give the same bits"


def test_more_columns_than_1024_chunks_of_2048():
    """n = 2 200 001 > 2048 * 1024: the chunks grow beyond 2048 elements (1024 workgroups); CSR, both losses."""
    m, n = 64, 2_200_001
    rng = np.random.default_rng(3)
    nnz = 300_000
    A = sp.csr_matrix((rng.standard_normal(nnz), (rng.integers(0, m, nnz), rng.integers(0, n, nnz))), shape=(m, n))
    A.sum_duplicates()
    A.sort_indices()
    x = rng.standard_normal(n) * (rng.random(n) < 0.01)
    for logistic in (False, True):
        b = _labels(m, 4) if logistic else rng.standard_normal(m)
        scale = 1.0 if logistic else 0.5
        prob = _make(A, b, 1.0, logistic, "csr")
        G0 = float(G.gap_longdouble(A, b, x, 1.0, scale, logistic)[0]["grad_inf"])
        _held(f"cols-{n}", prob, A, b, x, 0.5 * G0, scale, logistic, storage="csr", shape=[m, n], alpha="0.5")


# ---- (3) special values ------------------------------------------------------------------------------------------------------
def _margins_750():
    """Rows 0 .. 3 hold the single element +-750 against x_0 = 1 under both labels (t = +-750 in all four combinations), row 4
    is empty (t = 0); the other rows are ordinary.  n odd."""
    A = _rand(40, 33, 300, 17).tolil()
    for i, v in enumerate((750.0, 750.0, -750.0, -750.0)):
        A[i, :] = 0
        A[i, 0] = v
    A[4, :] = 0
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    b = _labels(40, 18)
    b[:4] = (1.0, -1.0, 1.0, -1.0)
    x = np.random.default_rng(19).standard_normal(33)
    x[0] = 1.0
    return A, b, x


@pytest.mark.parametrize("storage", ["csr", "dense"])
def test_saturated_and_zero_margins_stay_finite(storage):
    A, b, x = _margins_750()
    t = -b * (A @ x)
    assert sorted(t[:4]) == [-750.0, -750.0, 750.0, 750.0] and t[4] == 0.0
    prob = _make(A, b, 1.0, True, storage)
    G0 = float(G.gap_longdouble(A, b, x, 1.0, 1.0, True)[0]["grad_inf"])
    for frac in (2.0, 0.5, 1e-3):
        got = _held("margins-750", prob, A, b, x, frac * G0, 1.0, True, storage=storage, alpha=str(frac))
        assert got.f > 1500.0 and np.isfinite(got.dual) and np.isfinite(got.gap)
        if frac == 2.0:
            assert got.rows_gap == 0.0 and got.alpha == 1.0
        else:
            assert got.rows_gap > 750.0 * (1 - frac), "the two rows at t = +750 carry (1 - alpha) (750 + log(1 - alpha)) + alpha log alpha each"


@pytest.mark.parametrize("logistic", [False, True], ids=["ls", "logistic"])
@pytest.mark.parametrize("storage", ["csr", "dense"])
def test_a_nan_or_inf_in_x_gives_a_nan_gap(storage, logistic):
    """The bad element in the range of the first and of the last workgroup of the n-passes (n = 3 * 2048 + 5: four chunks), in a
    column WITH stored elements (the NaN reaches g through the margins: v_max_f64 would drop it from |g|_inf) and in an
    EMPTY column (CSR: nothing but the column pass ever reads x_j)."""
    m, n = 50, 3 * 2048 + 5
    A = _rand(m, n, 4 * n, 5).tolil()
    A[:, 0] = 0
    A[:, n - 1] = 0
    A[3, 1] = 1.5
    A[7, n - 2] = -0.5
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    rng = np.random.default_rng(6)
    b = _labels(m, 7) if logistic else rng.standard_normal(m)
    prob = _make(A, b, 0.3, logistic, storage)
    x = rng.standard_normal(n)
    assert np.isfinite(prob.duality_gap(x).gap)
    for bad in (np.nan, np.inf, -np.inf):
        for j in (0, 1, n - 2, n - 1):
            xb = x.copy()
            xb[j] = bad
            got = prob.duality_gap(xb)
            assert np.isnan(got.gap), (bad, j, got)
            if j in (1, n - 2) and (np.isnan(bad) or not logistic):
                # (an infinite margin saturates the logistic loss: rho is 0 or -+1 and g stays finite - the column pass catches x_j)
                assert np.isnan(got.grad_inf) and np.isnan(got.alpha), (bad, j, got)


@pytest.mark.parametrize("logistic", [False, True], ids=["ls", "logistic"])
def test_negative_zeros_in_x_behave_as_zeros(logistic):
    if logistic:
        A, b, lam = L.make_logistic(*L.SMALL[2])
    else:
        A, b, lam = S.make_sparse(*S.SMALL[2])
    n = A.shape[1]
    rng = np.random.default_rng(8)
    x = rng.standard_normal(n) * (rng.random(n) < 0.3)
    xm = np.where(x == 0.0, -0.0, x)
    assert np.signbit(xm).sum() > np.signbit(x).sum()
    for storage in ("csr", "dense"):
        prob = _make(A, b, lam, logistic, storage)
        assert np.array_equal(_bits(prob.duality_gap(x)), _bits(prob.duality_gap(xm)))
        assert prob.duality_gap(-np.zeros(n)).gap == prob.duality_gap(np.zeros(n)).gap


def test_a_cuda_tensor_is_accepted_and_a_wrong_length_is_not():
    import torch

    A, b, lam = S.make_sparse(*S.SMALL[2])
    prob = _make(A, b, lam, False, "csr")
    x = np.random.default_rng(1).standard_normal(A.shape[1])
    assert np.array_equal(_bits(prob.duality_gap(x)), _bits(prob.duality_gap(torch.from_numpy(x).cuda())))
    with pytest.raises(ValueError):
        prob.duality_gap(x[:-1])


# ---- (4) the live solver -----------------------------------------------------------------------------------------------------
def _live_case(name):
    from oracle import problems_ref as P

    if name in ("small", "dense-mfma", "dense-valu"):
        A, b, lam = P.make_plasso(512, 1024, seed=0)
        return sp.csr_matrix(A), b, lam, False, "dense"
    if name == "dense-logistic":
        A, b, lam = L.make_logistic(*L.SMALL[0])
        return A, b, lam, True, "dense"
    if name == "sparse-narrow":
        A, b, lam = S.make_sparse(*S.SMALL[1])
        return A, b, lam, False, "csr"
    if name == "sparse-wide":
        A, b, lam = S.make_sparse(*S.TALL)
        return A, b, lam, False, "csr"
    if name == "sparse-logistic":
        A, b, lam = L.make_logistic(*L.SMALL[1])
        return A, b, lam, True, "csr"
    A, b, lam = L.make_logistic(*L.TALL)
    return A, b, lam, True, "csr"


_LIVE = ["small", "dense-mfma", "dense-valu", "dense-logistic", "sparse-narrow", "sparse-wide", "sparse-logistic", "sparse-logistic-wide"]
_ENV = {"dense-mfma": {"ZF_LS_SMALL": "0"}, "dense-valu": {"ZF_LS_SMALL": "0", "ZF_GEMV_MFMA": "0"}}
_PLAN0 = {"small": 1, "dense-mfma": 2, "dense-valu": 3, "dense-logistic": 3, "sparse-narrow": 5, "sparse-wide": 5, "sparse-logistic": 5,
          "sparse-logistic-wide": 5}


def _walk(prob, passes, gap_after=(), opts=None, resume=None, snapshot_at=None):
    """`passes` chunks of ONE pass each; a gap call after the chunks listed in gap_after.  Returns what a solve is compared by."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    o = dict(BASE, **(opts or {}))
    run = NativeRun(prob, np.zeros(prob.n_features), o) if resume is None else NativeRun.from_snapshot(prob, resume, o)
    rows, gaps, state, after_reject = [np.zeros((0, _lib.ZF_TRACE_COLS))], {}, None, 0
    for k in range(passes):
        rows.append(run.advance(1))
        if k in gap_after:
            ctl = run.solver.ctl
            after_reject += int(ctl.trial > 0 and ctl.need_grad == 0)   # between a rejected trial and its retry
            gaps[k] = run.duality_gap()
        if snapshot_at == k:
            state = run.snapshot()
    ctl, _ = run.solver.poll()
    out = dict(rows=np.concatenate(rows), x=run.solver.get_x(), nit=int(ctl.nit), lr=ctl.lr, F=ctl.F_old, trials=int(ctl.total_trials),
               gaps=gaps, after_reject=after_reject, state=state, plan=run.solver.ls_plan(), run=run)
    return out


def _same(a, b):
    assert (a["nit"], a["lr"], a["F"], a["trials"]) == (b["nit"], b["lr"], b["F"], b["trials"])
    assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["x"], b["x"])


@pytest.mark.parametrize("name", _LIVE)
def test_the_gap_of_a_live_solve(name, monkeypatch):
    """NativeRun.duality_gap() after k passes against the standalone evaluation at get_x(): inside the derived bounds of the
    longdouble value everywhere, and bit for bit where the margins come from the same kernels (every path but the fused
    small-matrix one, whose rows kernel sums A x in another order than the row sweep of the evaluation).  A solve
    interrupted by a gap call after every pass - the lr = 1 starts backtrack, so calls fall between a rejected trial and its
    retry - is bit-identical to the uninterrupted one, and a snapshot taken after a gap call is the snapshot of the solve that
    was never asked, and resumes bit-identically."""
    for k, v in _ENV.get(name, {}).items():
        monkeypatch.setenv(k, v)
    A, b, lam, logistic, storage = _live_case(name)
    scale = 1.0 if logistic else 0.5
    prob = _make(A, b, lam, logistic, storage)
    passes = 24
    plain = _walk(prob, passes, snapshot_at=11)
    assert plain["plan"][0] == _PLAN0[name], plain["plan"]
    assert plain["trials"] > plain["nit"] > 0, "the case must backtrack and accept"
    probed = _walk(prob, passes, gap_after=range(passes), snapshot_at=11)
    _same(plain, probed)
    assert probed["after_reject"] >= 1, "no gap call fell between a rejected trial and its retry"
    # the last gap of the live solve against the standalone evaluation at the same x, and both against the reference
    live, alone = probed["gaps"][passes - 1], prob.duality_gap(probed["x"])
    vals, bounds, _ = G.gap_longdouble(A, b, probed["x"], lam, scale, logistic)
    for got, what in ((live, "live"), (alone, "standalone")):
        ratios = G.worst_ratio(got, vals, bounds)
        print(f"{name} {what}: worst error / bound {max(ratios.values()):.3g}; gap {float(got.gap):.6g}")
        _record(case="live-" + name, what=what, ratio=max(ratios.values()), ratios=ratios)
        assert max(ratios.values()) <= 1.0, (what, ratios)
    if name != "small":
        assert np.array_equal(_bits(live), _bits(alone)), (live, alone)
    # the gap falls along the solve (not monotonically, but by a lot over 24 passes)
    assert probed["gaps"][passes - 1].gap < probed["gaps"][0].gap
    # the snapshot taken after the gap call of pass 11 is the snapshot of the solve that was never asked, byte for byte, and
    # resumes as that one does: as the uninterrupted solve, on every path (the fused small-matrix one included: its restore
    # rebuilds the margins in the order its rows kernel left them)
    for key in ("x", "x_prev", "control"):
        assert np.array_equal(probed["state"][key], plain["state"][key]), key
    resumed = _walk(prob, passes - 12, resume=probed["state"])
    _same(resumed, _walk(prob, passes - 12, resume=plain["state"]))
    assert np.array_equal(resumed["x"], plain["x"]) and (resumed["nit"], resumed["lr"], resumed["F"]) == (plain["nit"], plain["lr"], plain["F"])
    assert np.array_equal(resumed["rows"], plain["rows"][len(plain["rows"]) - len(resumed["rows"]):])
    # a solver that is never asked allocates nothing for the gap and launches what it launched: same launch counts
    assert plain["run"].solver.launch_counts() == probed["run"].solver.launch_counts()


# ---- (5) stopping ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def recorded(monkeypatch):
    """Every gap check of a solve: (nit, gap)."""
    from zfista_amd import proximal_gradient as pg

    seen = []
    orig = pg.NativeRun.duality_gap

    def spy(self):
        gp = orig(self)
        seen.append((int(self.nit_seen), float(gp.gap)))
        return gp

    monkeypatch.setattr(pg.NativeRun, "duality_gap", spy)
    return seen


@pytest.mark.parametrize("name", ["small", "sparse-narrow", "dense-logistic", "sparse-logistic"])
def test_gap_tol_stops_at_the_first_check_at_or_below_it(name, recorded):
    from zfista_amd import minimize_proximal_gradient as solve

    A, b, lam, logistic, storage = _live_case(name)
    prob = _make(A, b, lam, logistic, storage)
    x0 = np.zeros(prob.n_features)
    kw = dict(lr=1.0, nesterov=True, tol=0.0)
    # the gap after EVERY pass of a long run (gap_tol = 0 never stops this early): what every stop below is re-derived from
    _quiet(solve, *prob.callbacks(), x0, max_iter=200, gap_tol=0.0, gap_every=1, **kw)
    every = list(recorded)[:-1]          # (the last entry is the gap at the final x of a solve that max_iter ended)
    gaps = np.array([gp for _, gp in every])
    assert len(every) >= 200 and gaps[-1] < 0.1 * gaps[0]
    # The gap of an accelerated method is not monotone.  The tolerance is taken where it has stopped crossing: the largest
    # gap from the middle of the record on, raised until no later pass of the record exceeds it after the first pass at or
    # below it - so "the first check at or below gap_tol" is within one chunk of passes for every gap_every.
    later_max = np.maximum.accumulate(gaps[::-1])[::-1]
    gap_tol = later_max[len(gaps) // 2]
    while True:
        p1 = int(np.argmax(gaps <= gap_tol))
        if later_max[p1] <= gap_tol:
            break
        gap_tol = later_max[p1]
    assert 16 < p1 < len(gaps) - 32

    def expected(k):
        """index into `every` of the first check a solve with gap_every = k stops at"""
        return next(i for i in range(k - 1, len(every), k) if gaps[i] <= gap_tol)

    stops = {}
    for k in (4, 1, 16):
        del recorded[:]
        res = _quiet(solve, *prob.callbacks(), x0, max_iter=200, gap_tol=gap_tol, gap_every=k, **kw)
        i = expected(k)
        assert recorded == every[k - 1:i + 1:k], "the same checks, and none after the first at or below gap_tol"
        assert res.success and res.status == 1 and res.message == "Duality gap reached gap_tol"
        assert res.dual_gap == gaps[i] <= gap_tol and res.dual_gap_checks == (i + 1) // k and res.nit == every[i][0]
        plain = _quiet(solve, *prob.callbacks(), x0, max_iter=res.nit, **kw)
        assert plain.nit == res.nit and np.array_equal(plain.x, res.x) and plain.fun == res.fun
        assert name == "small" or res.dual_gap == prob.duality_gap(res.x).gap
        stops[k] = (i, res.nit)
    assert "dual_gap" not in plain and "dual_gap_checks" not in plain
    assert set(plain.keys()) == {"x0", "tol", "tol_internal", "nesterov", "nesterov_ratio", "status", "message", "success", "x", "fun",
                                 "nit", "allvecs", "allfuns", "allerrs", "time"}, "result keys without the keyword are today's"
    # gap_every = 1 and gap_every = 16 stop within one chunk of each other
    assert stops[1][0] <= stops[4][0] <= stops[16][0] < stops[1][0] + 16 and stops[1][1] <= stops[16][1] <= stops[1][1] + 16


def test_a_solve_ended_by_tol_or_max_iter_still_carries_the_gap(recorded):
    from zfista_amd import minimize_proximal_gradient as solve

    A, b, lam, logistic, storage = _live_case("sparse-narrow")
    prob = _make(A, b, lam, logistic, storage)
    x0 = np.zeros(prob.n_features)
    res = _quiet(solve, *prob.callbacks(), x0, lr=1.0, nesterov=True, tol=0.0, max_iter=37, gap_tol=0.0, gap_every=16)
    assert not res.success and res.nit == 37 and res.message == "Maximum number of iterations reached"
    assert res.dual_gap == prob.duality_gap(res.x).gap > 0 and res.dual_gap_checks == len(recorded) - 1
    del recorded[:]
    res = _quiet(solve, *prob.callbacks(), x0, lr=1.0, nesterov=True, tol=1e-3, gap_tol=0.0, gap_every=8)
    assert res.success and res.message == "Optimization terminated successfully"
    assert res.dual_gap == prob.duality_gap(res.x).gap and res.dual_gap == recorded[-1][1]
    plain = _quiet(solve, *prob.callbacks(), x0, lr=1.0, nesterov=True, tol=1e-3)
    assert plain.nit == res.nit and np.array_equal(plain.x, res.x)


# ---- (6) the path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse-narrow", "dense-logistic"])
def test_l1_path(name):
    from zfista_amd import minimize_proximal_gradient as solve
    from zfista_amd.path import l1_path
    from zfista_amd.replicas import solve_on_streams

    A, b, lam, logistic, storage = _live_case(name)
    prob = _make(A, b, lam, logistic, storage)
    n = prob.n_features
    lam_max = float(prob.lam_max())
    lams = [np.nextafter(lam_max, np.inf)] + [lam_max * f for f in (0.7, 0.5, 0.35, 0.25)]
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=600)
    gap_tol = 1e-4 * float(prob.with_lam(lams[-1]).duality_gap(np.zeros(n)).primal)
    path = _quiet(l1_path, prob, lams, gap_tol=gap_tol, **kw)
    assert [r.lam for r in path] == [float(v) for v in lams]
    assert not path[0].x.any() and path[0].dual_gap == 0.0 and path[0].success, "from lam_max on x = 0 is optimal"
    x = np.zeros(n)
    nnz = []
    for lam_k, r in zip(lams, path):
        sib = prob.with_lam(lam_k)
        if storage == "csr":
            assert sib._spmat is prob._spmat and sib._spmat.value.value == prob._spmat.value.value
        else:
            assert sib.A.data_ptr() == prob.A.data_ptr()
        assert sib.b.data_ptr() == prob.b.data_ptr() and sib.lam == float(lam_k) and prob.lam == lam
        alone = _quiet(solve, *sib.callbacks(), x, gap_tol=gap_tol, **kw)
        assert alone.nit == r.nit and np.array_equal(alone.x, r.x) and alone.dual_gap == r.dual_gap
        assert r.success and r.dual_gap <= gap_tol
        x = r.x
        nnz.append(int(np.count_nonzero(r.x)))
    assert nnz[0] == 0 and nnz[-1] > nnz[1] >= 1, nnz
    # two paths at once, each on a stream of its own, over the SAME device matrix: the same bits
    jobs = [(prob.with_lam(lams[1]), np.zeros(n), dict(kw, gap_tol=gap_tol)), (prob.with_lam(lams[2]), path[1].x, dict(kw, gap_tol=gap_tol)),
            (prob.with_lam(lams[1]), np.zeros(n), dict(kw, gap_tol=gap_tol))]
    both = solve_on_streams(jobs, streams=3)
    assert np.array_equal(both[0].x, path[1].x) and np.array_equal(both[1].x, path[2].x) and np.array_equal(both[2].x, path[1].x)
    assert (both[0].nit, both[1].nit, both[0].dual_gap, both[1].dual_gap) == (path[1].nit, path[2].nit, path[1].dual_gap, path[2].dual_gap)


# ---- (7) refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_at_the_c_level_and_in_python():
    from zfista_amd import _lib, minimize_proximal_gradient as solve
    from zfista_amd.engine import DeviceSolver
    from zfista_amd.path import l1_path
    from zfista_amd.problems import BlurHaarL1, DiagQuadL1, LeastSquaresL1
    from zfista_amd.proximal_gradient import NativeRun

    A, b, lam = S.make_sparse(*S.SMALL[2])
    n = A.shape[1]
    boxed = _cls(False, "csr")(A, b, lam, bounds=(-1.0, 1.0))
    run = NativeRun(boxed, np.zeros(n), dict(BASE))
    run.advance(2)
    with pytest.raises(_lib.ZfError, match="box"):
        run.duality_gap()
    out = np.full(8, -7.0)
    assert run.solver.lib.zf_solver_duality_gap(run.solver.handle, C.c_void_p(_lib.ptr(out)), 7) == -2 and (out == -7.0).all()
    run.solver.close()
    diag = DiagQuadL1(np.ones(100), np.ones(100), 0.1)
    run = NativeRun(diag, np.zeros(100), dict(BASE))
    with pytest.raises(_lib.ZfError, match="only for"):
        run.duality_gap()
    run.solver.close()
    dense = LeastSquaresL1(A.toarray(), b, lam)
    fields, keep = dense._descriptor()
    options = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=10, max_backtrack_iter=10, nesterov=1, deprecated=0)
    sharded = DeviceSolver(dict(fields, world=2, rank=0), options, keepalive=keep)
    with pytest.raises(_lib.ZfError, match="world > 1"):
        sharded.duality_gap()
    sharded.close()
    for prob, x0 in ((boxed, np.zeros(n)), (diag, np.zeros(100)), (LeastSquaresL1(A.toarray(), b, lam, group=object()), np.zeros(n))):
        with pytest.raises(ValueError, match="gap_tol is not available"):
            solve(*prob.callbacks(), x0, gap_tol=1e-6)
        if hasattr(prob, "duality_gap"):
            with pytest.raises(ValueError, match="duality_gap is not available"):
                prob.duality_gap(x0)
    with pytest.raises(ValueError):
        l1_path(diag, [0.1])
    op = BlurHaarL1(np.full((3, 3), 1 / 9), np.ones((8, 8)), 0.01)
    with pytest.raises(ValueError, match="gap_tol is not available"):
        solve(*op.callbacks(), np.zeros(64), gap_tol=1e-6)
