"""GPU: the Poisson loss on the trials of the least-squares classes (PoissonL1, SparsePoissonL1; csrc/zf_kernels_poisson.h).

(1) The row kernels at every row count around the unroll tail, the block stride and the change of shape, for both classes and
    two scales: with A the sparse identity (and the same matrix densified where that fits) the margins are x exactly and the
    gradient is scale * psi - f and every gradient element inside the bounds derived in tests/poisson_cases.py against
    np.longdouble, psi within the exp allowance of NumPy's value, equal bits of f from both storage forms; a margin beyond the
    range of exp gives f = +inf (not NaN), a NaN margin NaN; the weighted kernels give +0 on rows with w = 0.
(2) Solves against the CPU oracle on tests/poisson_cases.PoissonRef and against the reference's fixture G18: ISTA, FISTA, a box,
    l2 = lam and weights on every SMALL case and both storage forms; the overflowing first trial; MFMA against VALU sweeps;
    reproducibility, snapshots, streams.
(3) The certificate: all eight / ten outputs inside their bounds; the live solver's gap; gap_tol, l1_path, l1_cv.
(4) Solvers that never asked launch what the parent commit's library launched (values recorded from it: DESIGN 4.5j), and the
    refusals.

ZF_POISSON_BOUNDS_RECORD=1 appends the worst error-to-bound ratios to profiles/poisson_kernel_bounds.jsonl and
profiles/poisson_gap_bounds.jsonl (any other value: to files of those names in that directory) - records, not thresholds."""
import functools
import hashlib
import json
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import poisson_cases as PC
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-10
U = PC.U
_id = lambda c: f"{c[0]}x{c[1]}"


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _cls(storage):
    from zfista_amd import problems as Z

    return Z.SparsePoissonL1 if storage == "csr" else Z.PoissonL1


def _make(storage, A, b, lam, l2=0.0, bounds=None, scale=PC.SCALE, w=None):
    return _cls(storage)(PC.matrix(A, storage) if sp.issparse(A) else A, b, lam, scale=scale, bounds=bounds, l2=l2, sample_weight=w)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _record(name, **rec):
    where = os.environ.get("ZF_POISSON_BOUNDS_RECORD", "")
    if where in ("", "0"):
        return
    path = os.path.join(os.path.join(ROOT, "profiles") if where == "1" else where, name)
    with open(path, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


@functools.lru_cache(maxsize=None)
def _data(case):
    """(A, b, lam) of poisson_cases.make_poisson - read-only, shared."""
    return PC.make_poisson(*case)


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
            self.counts = self.solver.launch_counts()
            return rows

    monkeypatch.setattr(pg, "NativeRun", _Recorded)

    def run(prob, x0, **kw):
        del seen[:]
        res = _quiet(minimize_proximal_gradient, *prob.callbacks(), x0, **kw)
        assert len(seen) == 1, "the solve did not run on the native path"
        return res, np.concatenate(seen[0].rows), seen[0].plan, seen[0].counts

    return run


# ---- (1) the row kernels -----------------------------------------------------------------------------------------------------------
ROWS = [1, 63, 64, 65, 1023, 1024, 1025, 2049, 32768, 32769, 40000]
SCALES = [1.0, 0.5]   # (powers of two: scale * psi is exact, so the gradient shows psi itself)
DENSE_IDENTITY_MAX = 2049   # (an identity of 32768 rows is 8.6 GB in dense storage: beyond this, the dense class gets the m x 2
#                              matrix [z, 0] at x = (1, 0), whose margins are z exactly as well)


def _margins(m, seed):
    """(z, b): margins with zeros of both signs, |z| up to 30, one row at 700 and one at -700 (m >= 63); counts with b = 0 rows.
    (A margin of -0 reaches the row kernel as +0 - the row sums of every sweep start from +0 - and exp(+-0) = 1 either way.)"""
    rng = np.random.default_rng(seed)
    b = rng.poisson(1.5, m).astype(np.float64)
    z = rng.uniform(-3.0, 3.0, m)
    z[::5] = rng.uniform(-30.0, 30.0, z[::5].size)
    z[3::11] = 0.0
    z[4::11] = -0.0
    b[2::7] = 0.0
    b[5::13] += 0.25   # (counts need not be integers)
    if m >= 63:
        z[m // 2], z[m // 3] = 700.0, -700.0
        b[m // 2], b[m // 3] = 2.0, 3.0
    return z, b


def _eval_both(m, z, b, scale, w=None, poison=None):
    """f and the gradient of both classes at margins z: {storage: (f, grad or None)}; the dense gradient only for the identity.
    poison: rows whose count is overwritten with NaN in device memory once the problem stands (the constructor refuses such a
    b on the host; what a row with w = 0 holds there must not matter to the kernels)."""
    import torch

    def spoil(prob):
        if poison is not None:
            prob.b[torch.from_numpy(np.flatnonzero(poison)).to(prob.b.device)] = float("nan")
        return prob

    I = sp.identity(m, format="csr", dtype=np.float64)
    out = {}
    ps = spoil(_make("csr", I, b, 0.1, scale=scale, w=w))
    out["csr"] = (ps.f(z), ps.jac_f(z))
    if m <= DENSE_IDENTITY_MAX:
        pd = spoil(_make("dense", np.eye(m), b, 0.1, scale=scale, w=w))
        out["dense"] = (pd.f(z), pd.jac_f(z))
    else:
        pd = spoil(_make("dense", np.stack([z, np.zeros(m)], axis=1), b, 0.1, scale=scale, w=w))
        out["dense"] = (pd.f(np.array([1.0, 0.0])), None)
    return out


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("m", ROWS)
def test_row_kernels_within_their_bounds(m, scale):
    z, b = _margins(m, seed=m)
    f_exact, f_bound, psi, psi_bound = PC.loss_longdouble(z, b, scale)
    psi_np = np.exp(z) - b
    allow = PC.psi_allowance(z, b)
    got = _eval_both(m, z, b, scale)
    worst_f = worst_g = 0.0
    for storage, (f, grad) in got.items():
        err = abs(float(np.longdouble(f) - f_exact))
        ratio = 0.0 if err == 0.0 else err / f_bound
        worst_f = max(worst_f, ratio)
        print(f"m={m} scale={scale} {storage}: f {float(f):.17g}, error / bound {ratio:.3g}")
        assert np.isfinite(f) and ratio <= 1.0, (storage, f, float(f_exact), f_bound)
        if grad is not None:   # the gradient is scale * psi, exactly
            gerr = np.abs((grad.astype(np.longdouble) - np.longdouble(scale) * psi).astype(np.float64))
            gr = np.max(np.where(gerr == 0.0, 0.0, gerr / (scale * psi_bound)))
            worst_g = max(worst_g, float(gr))
            assert gr <= 1.0, (storage, int(np.argmax(gerr / (scale * psi_bound))), gr)
            assert (np.abs(grad / scale - psi_np) <= allow).all(), "psi within the exp allowance of NumPy's value"
    assert _bits(got["csr"][0]) == _bits(got["dense"][0]), "both classes sum a loss of the same m in the same order"
    if m >= 63:
        assert z.max() == 700.0 and z.min() == -700.0 and (b == 0).any() and np.signbit(z[4])
    _record("poisson_kernel_bounds.jsonl", test="rows", m=m, scale=scale, f_ratio=worst_f, grad_ratio=worst_g)


@pytest.mark.parametrize("m", [65, 2049, 32769, 40000])
def test_an_overflowing_margin_gives_inf_and_a_nan_margin_nan(m):
    """One margin of 800 among m: f = +inf in both shapes of the kernels - not NaN.  One NaN margin: NaN.  The sparse class on the
    identity at x = z, the dense class on the m x 2 matrix [z, 0] at x = (1, 0) - in both only that row's margin is not finite."""
    z, b = _margins(m, seed=m + 1)
    sparse = _make("csr", sp.identity(m, format="csr", dtype=np.float64), b, 0.1)
    e1 = np.array([1.0, 0.0])
    f_of = {"csr": lambda v: sparse.f(v), "dense": lambda v: _make("dense", np.stack([v, np.zeros(m)], axis=1), b, 0.1).f(e1)}
    for storage, f in f_of.items():
        assert np.isfinite(f(z)), storage
        for k in (0, m // 2, m - 1):
            big = z.copy()
            big[k] = 800.0
            assert f(big) == np.inf, (storage, k, "exp overflows: inf - b z is inf, not NaN")
            bad = z.copy()
            bad[k] = np.nan
            assert np.isnan(f(bad)), (storage, k)
    big = z.copy()
    big[m // 2] = 800.0
    g = sparse.jac_f(big)
    assert g[m // 2] == np.inf and np.isfinite(np.delete(g, m // 2)).all()


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("m", [1, 65, 1025, 2049, 32769])
def test_weighted_row_kernels_give_plus_zero_on_rows_that_are_not_there(m, scale):
    z, b = _margins(m, seed=m + 2)
    rng = np.random.default_rng(m)
    w = 0.5 + 1.5 * rng.random(m)
    off = rng.random(m) < 0.3
    if m > 1:
        off[0], off[-1] = True, False
    else:
        off[:] = False
    w[off] = 0.0
    f_exact, f_bound, wpsi, wpsi_bound = PC.loss_longdouble(z, b, scale, w=w)
    got = _eval_both(m, z, b, scale, w=w, poison=off)   # NaN counts on the rows with w = 0: whatever such a row holds
    for storage, (f, grad) in got.items():
        err = abs(float(np.longdouble(f) - f_exact))
        assert np.isfinite(f) and err <= f_bound, (storage, f, float(f_exact), f_bound)
        if grad is not None:
            assert (_bits(grad[off]) == 0).all(), "+0 on a row with w = 0"
            gerr = np.abs((grad.astype(np.longdouble) - np.longdouble(scale) * wpsi).astype(np.float64))
            assert (gerr <= scale * wpsi_bound).all(), storage
    assert _bits(got["csr"][0]) == _bits(got["dense"][0])
    if m > 1:   # all weights but zeros equal to one: the unweighted kernels' f on the rows that are there, to the bound
        ones = np.where(off, 0.0, 1.0)
        sub = _make("csr", sp.identity(int((~off).sum()), format="csr", dtype=np.float64), b[~off], 0.1, scale=scale).f(z[~off])
        full = _make("csr", sp.identity(m, format="csr", dtype=np.float64), b, 0.1, scale=scale, w=ones).f(z)
        assert abs(float(full) - float(sub)) <= 2 * PC.loss_longdouble(z[~off], b[~off], scale)[1]


# ---- (2) solves --------------------------------------------------------------------------------------------------------------------
BOX = (-0.05, 0.25)
VARIANTS = {
    "ista": dict(kw=dict(nesterov=False)),
    "fista": dict(kw=dict(nesterov=True, nesterov_ratio=(0, 0.25))),
    "box": dict(kw=dict(nesterov=True, nesterov_ratio=(0, 0.25)), bounds=BOX),
    "l2": dict(kw=dict(nesterov=True, nesterov_ratio=(0, 0.25)), l2fac=1.0),
    "weights": dict(kw=dict(nesterov=True, nesterov_ratio=(0, 0.25)), weighted=True),
}
_ORACLE = {}


def _variant_problem(case, tag):
    A, b, lam = _data(case)
    v = VARIANTS[tag]
    return A, b, lam, dict(l2=v.get("l2fac", 0.0) * lam, bounds=v.get("bounds"), w=PC.case_weights(case) if v.get("weighted") else None)


def _oracle(case, tag):
    """The CPU oracle on the closures over the CSR matrix: one run per (case, variant), shared by both storage forms."""
    from oracle import cpu_ref

    if (case, tag) not in _ORACLE:
        A, b, lam, opt = _variant_problem(case, tag)
        ref = PC.PoissonRef(A, b, lam, l2=opt["l2"], bounds=opt["bounds"], sample_weight=opt["w"])
        _ORACLE[case, tag] = _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), np.zeros(A.shape[1]), **PC.GOLDEN_KW,
                                    **VARIANTS[tag]["kw"])
    return _ORACLE[case, tag]


def _check_solve(res, rows, exp):
    from zfista_amd import _lib

    assert res.nit == exp.nit == 80 and bool(res.success) == bool(exp.success) and res.get("status") == exp.get("status")
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), np.asarray(exp.alltrials, np.int64))
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float))
    assert rel_err(res.x, exp.x) <= TOL
    assert max(rel_err(a, e) for a, e in zip(res.allvecs[1:], exp.allvecs[1:])) <= TOL
    np.testing.assert_allclose(res.allfuns, exp.allfuns, rtol=TOL, atol=0)
    xnorm = max(float(np.linalg.norm(v)) for v in exp.allvecs)
    np.testing.assert_allclose(res.allerrs, exp.allerrs, rtol=TOL, atol=2 * TOL * xnorm)


@pytest.mark.parametrize("storage", PC.FORMS)
@pytest.mark.parametrize("tag", sorted(VARIANTS))
@pytest.mark.parametrize("case", PC.SMALL, ids=_id)
def test_solve_vs_oracle(case, tag, storage, solve):
    """80 iterations from lr = 1: nit, status, the lr and trial sequences equal to the CPU oracle's on PoissonRef; iterates, F and
    err to 1e-10."""
    from zfista_amd import _lib

    A, b, lam, opt = _variant_problem(case, tag)
    exp = _oracle(case, tag)
    res, rows, plan, _ = solve(_make(storage, A, b, lam, **opt), np.zeros(A.shape[1]), **PC.GOLDEN_KW, **VARIANTS[tag]["kw"])
    assert plan[0] == 5 if storage == "csr" else plan[0] in (2, 3, 4), "never the fused small-matrix path"
    assert sum(exp.alltrials) > 80 and exp.alltrials[0] >= 5, "the line search backtracks from lr = 1 (8 - 11 rejections at the start)"
    _check_solve(res, rows, exp)
    if tag == "box":
        assert np.count_nonzero(res.x == BOX[0]) + np.count_nonzero(res.x == BOX[1]) >= 1, "the box must be active"
    if case == PC.OVERFLOW_CASE:   # the first trial's largest margin is beyond the range of exp: rejected, and the solve goes on
        assert rows[0, _lib.TR_TRIALS] >= 2 and res.nit == 80 and np.isfinite(res.allfuns).all()


SOLVES = [(ci, fi, st, tag) for ci in range(len(PC.SMALL)) for fi, st, tag in PC.GOLDEN_SOLVES]


@pytest.mark.parametrize("ci,fi,storage,tag", SOLVES)
def test_solve_vs_reference_fixture(golden, ci, fi, storage, tag, solve):
    """80 iterations from lr = 1 against what the REFERENCE solver produced on the closures (tests/golden/make_golden_poisson.py)."""
    from zfista_amd import _lib

    G = golden("g18_poisson.npz")
    A, b, lam = _data(PC.SMALL[ci])
    assert lam == float(G(f"poisson.c{ci}.lam"))
    res, rows, plan, _ = solve(_make(storage, A, b, lam, l2=fi * lam), np.zeros(A.shape[1]), **PC.GOLDEN_KW, **PC.GOLDEN_VARIANTS[tag])
    pre = PC.golden_prefix(ci, fi, storage, tag)
    assert res.nit == int(G(f"{pre}.nit")) == 80 and res.status == int(G(f"{pre}.status"))
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), G(f"{pre}.alltrials")) and rows[:, _lib.TR_TRIALS].sum() > 80
    assert np.array_equal(rows[:, _lib.TR_LR], G(f"{pre}.alllrs"))
    assert rel_err(res.x, G(f"{pre}.x")) <= TOL
    assert abs(np.linalg.norm(res.x) - float(G(f"{pre}.xnorm"))) <= TOL * float(G(f"{pre}.xnorm"))
    for k, v in zip(G(f"{pre}.kept"), G(f"{pre}.vecs")):
        if k > 0:
            assert rel_err(res.allvecs[k][::PC.GOLDEN_STRIDE], v) <= TOL, k
    np.testing.assert_allclose(res.allfuns, G(f"{pre}.allfuns"), rtol=TOL, atol=0)
    np.testing.assert_allclose(res.allerrs, G(f"{pre}.allerrs"), rtol=TOL, atol=2 * TOL * float(G(f"{pre}.xnorm")))


@pytest.mark.parametrize("storage", PC.FORMS)
def test_tall_solve_vs_oracle(storage, solve):
    """40 000 rows: the many-workgroup shape of the loss kernels inside a live solve with momentum."""
    A, b, lam = _data(PC.TALL)
    exp = _oracle(PC.TALL, "fista")
    res, rows, plan, _ = solve(_make(storage, A, b, lam), np.zeros(A.shape[1]), **PC.GOLDEN_KW, **VARIANTS["fista"]["kw"])
    _check_solve(res, rows, exp)


@pytest.mark.parametrize("case", PC.SMALL, ids=_id)
def test_dense_and_sparse_classes_take_the_same_trials(case, solve):
    from zfista_amd import _lib

    A, b, lam = _data(case)
    kw = dict(PC.GOLDEN_KW, **VARIANTS["fista"]["kw"])
    out = {st: solve(_make(st, A, b, lam), np.zeros(A.shape[1]), **kw) for st in PC.FORMS}
    (rs, rows_s, _, _), (rd, rows_d, _, _) = out["csr"], out["dense"]
    assert np.array_equal(rows_s[:, _lib.TR_TRIALS], rows_d[:, _lib.TR_TRIALS]) and np.array_equal(rows_s[:, _lib.TR_LR], rows_d[:, _lib.TR_LR])
    assert rel_err(rd.x, rs.x) <= TOL


def test_mfma_and_valu_column_sweeps_decide_alike(solve, monkeypatch):
    """n % 32 == 0: the dense class sweeps A^T on v_mfma_f64_16x16x4 unless ZF_GEMV_MFMA=0; the two orders of summation take
    the same trials."""
    from zfista_amd import _lib

    case = (300, 1024, 0.02, 11)
    A, b, lam = _data(case)
    kw = dict(PC.GOLDEN_KW, **VARIANTS["fista"]["kw"])
    mf, rows_m, plan_m, _ = solve(_make("dense", A, b, lam), np.zeros(1024), **kw)
    monkeypatch.setenv("ZF_GEMV_MFMA", "0")
    va, rows_v, plan_v, _ = solve(_make("dense", A, b, lam), np.zeros(1024), **kw)
    assert plan_m[0] == 2 and plan_v[0] == 3
    assert mf.nit == va.nit == 80 and rows_m[:, _lib.TR_TRIALS].sum() > 80
    assert np.array_equal(rows_m[:, _lib.TR_TRIALS], rows_v[:, _lib.TR_TRIALS]) and np.array_equal(rows_m[:, _lib.TR_LR], rows_v[:, _lib.TR_LR])
    assert rel_err(mf.x, va.x) <= TOL


@pytest.mark.parametrize("storage", PC.FORMS)
def test_results_are_bit_reproducible(storage, solve):
    """Twice the same solve, with and without return_all, at sub_iters 1 and at the default: the same bits."""
    A, b, lam = _data(PC.SMALL[0])
    prob = _make(storage, A, b, lam)
    kw = dict(lr=1, tol=0.0, max_iter=80, nesterov=True)
    base, rows0, _, _ = solve(prob, np.zeros(A.shape[1]), **kw)
    for extra in (dict(), dict(return_all=True), dict(sub_iters=1), dict(sub_iters=1, return_all=True)):
        res, rows, _, _ = solve(prob, np.zeros(A.shape[1]), **kw, **extra)
        assert res.nit == 80 and np.array_equal(_bits(res.x), _bits(base.x)) and res.fun == base.fun, extra
        assert np.array_equal(rows, rows0), extra


_OPTS = dict(lr=1, tol=0.0, tol_internal=1e-12, max_iter=70, max_iter_internal=100000, max_backtrack_iter=100, warm_start=False,
             decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False, deprecated=False)


def _drain(run, step=5):
    from zfista_amd import _lib

    rows = [np.zeros((0, _lib.ZF_TRACE_COLS))]
    while run.status == _lib.ZF_RUNNING:
        rows.append(run.advance(step))
    return np.concatenate(rows)


@pytest.mark.parametrize("variant", ["l1", "l2=lam", "weights"])
@pytest.mark.parametrize("storage", PC.FORMS)
def test_snapshot_resume_is_bit_identical(storage, variant, tmp_path):
    """from_snapshot recreates the solver from the problem - which sets the loss (and l2, the weights) again - and continues
    bit for bit."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    A, b, lam = _data(PC.SMALL[0])
    prob = _make(storage, A, b, lam, l2=lam if variant == "l2=lam" else 0.0, w=PC.case_weights(PC.SMALL[0]) if variant == "weights" else None)
    whole = NativeRun(prob, np.zeros(prob.n_features), _OPTS)
    ref_rows, ref_x = _drain(whole), whole.solver.get_x()
    whole.solver.close()
    assert len(ref_rows) == 70 and ref_rows[:, _lib.TR_TRIALS].sum() > 70
    for stop_after in (3, 20):
        first = NativeRun(prob, np.zeros(prob.n_features), _OPTS)
        head = [first.advance(1) for _ in range(stop_after)]
        state = first.snapshot()
        first.solver.close()
        np.savez(tmp_path / "ckpt.npz", **state)
        run = NativeRun.from_snapshot(prob, dict(np.load(tmp_path / "ckpt.npz")), _OPTS)
        rows = np.concatenate(head + [_drain(run)])
        assert np.array_equal(rows, ref_rows) and np.array_equal(run.solver.get_x(), ref_x), stop_after
        run.solver.close()


@pytest.mark.parametrize("which", ["small", "tall"])
def test_concurrent_solves_of_one_problem_equal_the_solves_alone(which):
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.replicas import solve_on_streams

    A, b, lam = _data(PC.SMALL[1] if which == "small" else PC.TALL)
    n = A.shape[1]
    prob = _make("csr", A, b, lam)
    ratios = [(0, 0.25), (0.5, 1 / 16)]
    kws = [dict(lr=1, tol=0.0, max_iter=60, nesterov=True, nesterov_ratio=r, return_all=(k % 2 == 0)) for k, r in enumerate(ratios)]
    alone = [_quiet(minimize_proximal_gradient, *prob.callbacks(), np.zeros(n), **kw) for kw in kws]
    two = solve_on_streams([(prob, np.zeros(n), kw) for kw in kws], streams=2)
    for a, c in zip(alone, two):
        assert a.nit == c.nit == 60 and np.array_equal(a.x, c.x) and a.fun == c.fun
        if a.allfuns is not None:
            assert np.array_equal(np.asarray(a.allfuns), np.asarray(c.allfuns)) and np.array_equal(np.asarray(a.allvecs), np.asarray(c.allvecs))


def test_callables_against_the_closures():
    """f, jac_f, g, prox_wsum_g and lam_max of both classes against PoissonRef on the 2000 x 5000 case, with and without weights."""
    A, b, lam = _data(PC.SMALL[1])
    n = A.shape[1]
    rng = np.random.default_rng(4)
    x = np.zeros(n)
    x[rng.choice(n, 40, replace=False)] = 0.1 * rng.standard_normal(40)
    for w in (None, PC.case_weights(PC.SMALL[1])):
        ref = PC.PoissonRef(A, b, lam, l2=0.5 * lam, sample_weight=w)
        for storage in PC.FORMS:
            prob = _make(storage, A, b, lam, l2=0.5 * lam, w=w)
            assert abs(float(prob.f(x)) - ref.f(x)) <= 1e-12 * ref.f(x)
            np.testing.assert_allclose(prob.jac_f(x), ref.jac_f(x), rtol=1e-11, atol=1e-12)
            assert abs(float(prob.g(x)) - ref.g(x)) <= 1e-12 * ref.g(x)
            v = 0.01 * rng.standard_normal(n)
            assert np.array_equal(prob.prox_wsum_g(0.37, v), ref.prox_wsum_g(0.37, v))
            lmax = PC.lam_max(A, b, w=w)
            assert abs(float(prob.lam_max()) - lmax) <= 1e-12 * lmax
            assert abs(lmax - float(np.max(np.abs(A.T @ ((1.0 if w is None else w) * (1.0 - b)))))) <= 1e-12 * lmax, "scale |A^T (w o (1 - b))|_inf"


# ---- (3) the certificate -----------------------------------------------------------------------------------------------------------
def _gap_bits(gp, keys):
    return np.array([getattr(gp, k) for k in keys]).view(np.uint64)


_ITERATES = {}


def _iterates(case, fac, weighted):
    """x_0, x_20 and x_400 of a FISTA solve of the sparse class - one solve per (case, l2, weights), shared by both storage forms."""
    from zfista_amd import minimize_proximal_gradient

    key = (case, fac, weighted)
    if key not in _ITERATES:
        A, b, lam = _data(case)
        prob = _make("csr", A, b, lam, l2=fac * lam, w=PC.case_weights(case) if weighted else None)
        res = _quiet(minimize_proximal_gradient, *prob.callbacks(), np.zeros(A.shape[1]), lr=1, tol=0.0, max_iter=400, nesterov=True,
                     return_all=True)
        assert res.nit == 400
        _ITERATES[key] = {k: np.array(res.allvecs[k]) for k in (0, 20, 400)}
    return _ITERATES[key]


@pytest.mark.parametrize("storage", PC.FORMS)
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("fac", [0.0, 1.0], ids=["l1", "l2=lam"])
@pytest.mark.parametrize("case", PC.SMALL + [PC.TALL], ids=_id)
def test_every_output_within_its_rounding_bound(case, fac, weighted, storage):
    """problem.duality_gap(x) at x = 0 and at the iterates 20 and 400 of a FISTA solve: all eight (l2 = 0) / ten (l2 = lam)
    outputs inside the bounds of tests/poisson_cases.py; gap >= 0."""
    A, b, lam = _data(case)
    l2 = fac * lam
    w = PC.case_weights(case) if weighted else None
    keys = PC.KEYS10 if l2 > 0 else PC.KEYS8
    prob = _make(storage, A, b, lam, l2=l2, w=w)
    xs = _iterates(case, fac, weighted)
    gaps = []
    for k in (0, 20, 400):
        x = xs[k]
        vals, bounds, extra = PC.gap_longdouble(A, b, x, lam, l2=l2, w=w)
        got = prob.duality_gap(x)
        ratios = PC.worst_ratio(got, vals, bounds)
        worst = max(ratios, key=ratios.get)
        print(f"{_id(case)} {storage} l2 = {fac} lam weighted {weighted}, x_{k}: worst error / bound {ratios[worst]:.3g} ({worst}); "
              f"gap {float(got.gap):.6g} alpha {float(got.alpha):.6g} rows {float(got.rows_gap):.3g}")
        _record("poisson_gap_bounds.jsonl", case=_id(case), storage=storage, l2_over_lam=fac, weighted=weighted, iterate=k, worst=worst,
                ratio=ratios[worst], ratios=ratios, gap=float(got.gap), alpha=float(got.alpha))
        assert all(np.isfinite(getattr(got, key)) for key in keys), got
        assert ratios[worst] <= 1.0, (k, worst, ratios, got)
        assert got.gap >= 0 and got.rows_gap >= 0 and got.ridge_gap >= 0 and got.gap >= (got.rows_gap + got.ridge_gap) * (1 - 4 * U)
        if l2 == 0:
            assert got.g_l2 == 0.0 and got.ridge_gap == 0.0
        gaps.append(float(got.gap))
    assert gaps[2] < gaps[0]
    x = xs[400]
    assert np.array_equal(_gap_bits(prob.duality_gap(x), keys), _gap_bits(prob.duality_gap(x), keys)), "two evaluations: the same bits"


@pytest.mark.parametrize("storage", PC.FORMS)
@pytest.mark.parametrize("case", [PC.SMALL[0], PC.TALL], ids=_id)
def test_the_rows_gap_is_exactly_zero_at_alpha_one(case, storage):
    """lam >= lam_max at x = 0: alpha = 1, 1 - alpha = 0 exactly, every row term exactly 0 (the pass skips them), gap = 0 and
    D = P = f(0) = scale m to rounding - in both shapes of the rows pass, with and without weights."""
    A, b, lam = _data(case)
    for w in (None, PC.case_weights(case)):
        big = 2.0 * PC.lam_max(A, b, w=w)
        got = _make(storage, A, b, big, w=w).duality_gap(np.zeros(A.shape[1]))
        assert got.alpha == 1.0 and _bits(got.rows_gap) == 0 and got.gap == 0.0
        mass = float(A.shape[0] if w is None else w.sum())
        assert abs(float(got.primal) - mass) <= 1e-12 * mass and abs(float(got.dual) - mass) <= 1e-12 * mass


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


@pytest.mark.parametrize("variant", ["l1", "l2=lam", "weights"])
@pytest.mark.parametrize("storage", PC.FORMS)
def test_the_gap_of_a_live_solve(storage, variant):
    """NativeRun.duality_gap() equals the standalone evaluation at get_x() bit for bit (a Poisson solve is always on the general
    path: the margins come from the same kernels), and a solve probed after every pass - also between a rejected trial and
    its retry - is the solve that was never asked, bit for bit."""
    A, b, lam = _data(PC.SMALL[1])   # n = 5000: more than one gap chunk
    l2 = lam if variant == "l2=lam" else 0.0
    w = PC.case_weights(PC.SMALL[1]) if variant == "weights" else None
    keys = PC.KEYS10 if l2 > 0 else PC.KEYS8
    prob = _make(storage, A, b, lam, l2=l2, w=w)
    passes = 30
    plain = _walk(prob, passes)
    assert plain["trials"] > plain["nit"] > 0, "the case must backtrack and accept"
    probed = _walk(prob, passes, gap_after=range(passes))
    assert (plain["nit"], plain["lr"], plain["F"], plain["trials"]) == (probed["nit"], probed["lr"], probed["F"], probed["trials"])
    assert np.array_equal(plain["rows"], probed["rows"]) and np.array_equal(plain["x"], probed["x"])
    assert probed["after_reject"] >= 1, "no gap call fell between a rejected trial and its retry"
    assert plain["counts"] == probed["counts"]
    live, alone = probed["gaps"][passes - 1], prob.duality_gap(probed["x"])
    assert np.array_equal(_gap_bits(live, keys), _gap_bits(alone, keys)), (live, alone)
    vals, bounds, _ = PC.gap_longdouble(A, b, probed["x"], lam, l2=l2, w=w)
    ratios = PC.worst_ratio(live, vals, bounds)
    assert max(ratios.values()) <= 1.0, ratios
    assert (live.g_l2 > 0) == (l2 > 0) and live.gap >= 0


@pytest.mark.parametrize("storage", PC.FORMS)
def test_gap_tol_stops_the_solve_with_a_valid_certificate(storage):
    """The 1000 x 257 case at lam_max / 2: the solve stops with dual_gap <= gap_tol, on the iterates of the solve without the
    keyword."""
    from zfista_amd import minimize_proximal_gradient as solve

    A, b, _ = _data(PC.GAP_CASE)
    n = A.shape[1]
    lam = 0.5 * PC.lam_max(A, b)
    prob = _make(storage, A, b, lam)
    P0 = float(PC.primal_longdouble(A, b, np.zeros(n), lam))
    gap_tol = 1e-7 * P0   # (the CPU oracle reaches gap / P of 5e-10 after 400 FISTA iterations here)
    kw = dict(lr=1.0, nesterov=True, tol=0.0)
    res = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=2000, gap_tol=gap_tol, **kw)
    assert res.success and res.status == 1 and res.message == "Duality gap reached gap_tol" and res.nit < 2000
    assert 0 <= res.dual_gap <= gap_tol and res.dual_gap == prob.duality_gap(res.x).gap
    plain = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=res.nit, **kw)
    assert plain.nit == res.nit and np.array_equal(plain.x, res.x) and plain.fun == res.fun, "the keyword does not alter the iterates"
    vals, _, _ = PC.gap_longdouble(A, b, res.x, lam)
    print(f"{storage}: stopped at nit {res.nit}, gap {float(res.dual_gap):.3g} <= {gap_tol:.3g}; long double {float(vals['gap']):.3g}")
    assert float(vals["gap"]) <= gap_tol * (1 + 1e-6)
    for bad in ("remainder", "resolved"):
        with pytest.raises(ValueError, match="acceptance="):
            solve(*prob.callbacks(), np.zeros(n), acceptance=bad, max_iter=3)


def test_zf_accept_remainder_in_the_environment_falls_back_to_the_reference_test(monkeypatch):
    from zfista_amd import minimize_proximal_gradient as solve

    A, b, lam = _data(PC.GAP_CASE)
    prob = _make("csr", A, b, lam)
    n = A.shape[1]
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=40)
    plain = _quiet(solve, *prob.callbacks(), np.zeros(n), **kw)
    monkeypatch.setenv("ZF_ACCEPT", "remainder")
    env = _quiet(solve, *prob.callbacks(), np.zeros(n), **kw)
    assert np.array_equal(env.x, plain.x) and env.nit == plain.nit == 40 and "acceptance" not in env


@pytest.mark.parametrize("storage", PC.FORMS)
def test_l1_path_and_l1_cv_match_the_same_calls_made_problem_by_problem(storage):
    """l1_path over five weights and l1_cv(folds=3) with an exposure vector on the 1000 x 257 case: each point is the solve of the
    sibling problem from the point before, bit for bit; a fold is the sample_weight sibling."""
    from zfista_amd import minimize_proximal_gradient as solve
    from zfista_amd.path import cv_fold_ids, l1_cv, l1_path

    A, b, _ = _data(PC.GAP_CASE)
    m, n = A.shape
    exposure = 0.5 + 1.5 * np.random.default_rng(8).random(m)
    rate = b / exposure
    prob = _make(storage, A, rate, 1.0, w=exposure)
    lmax = float(prob.lam_max())
    assert abs(lmax - PC.lam_max(A, rate, w=exposure)) <= 1e-12 * lmax
    lams = [lmax * f for f in (1.0000001, 0.5, 0.25, 0.15, 0.1)]
    gap_tol = 1e-6 * float(PC.primal_longdouble(A, rate, np.zeros(n), lams[-1], w=exposure))
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=4000)
    pth = _quiet(l1_path, prob, lams, gap_tol=gap_tol, **kw)
    assert not pth[0].x.any() and len(pth) == 5
    x = np.zeros(n)
    for lam_k, r in zip(lams, pth):
        sib = prob.with_lam(lam_k)
        assert sib.b.data_ptr() == prob.b.data_ptr()
        one = _quiet(solve, *sib.callbacks(), x, gap_tol=gap_tol, **kw)
        assert r.success and r.dual_gap <= gap_tol and r["lam"] == lam_k
        assert one.nit == r.nit and np.array_equal(one.x, r.x) and one.dual_gap == r.dual_gap
        vals, _, _ = PC.gap_longdouble(A, rate, r.x, lam_k, w=exposure)
        assert float(vals["gap"]) <= gap_tol * (1 + 1e-6)
        x = r.x
    assert np.count_nonzero(pth[-1].x) > np.count_nonzero(pth[1].x) > 0
    cv = _quiet(l1_cv, prob, lams[1:4], folds=3, seed=5, gap_tol=gap_tol, return_paths=True, **kw)
    ids = cv_fold_ids(m, 3, 5)
    assert np.array_equal(cv.fold_ids, ids) and cv.scores.shape == (3, 3) and np.isfinite(cv.scores).all()
    for r_, k in enumerate(cv.folds):
        train, test = prob.with_sample_weight(exposure * (ids != k)), prob.with_sample_weight(exposure * (ids == k))
        x = np.zeros(n)
        for l, lam_l in enumerate(lams[1:4]):
            one = _quiet(solve, *train.with_lam(lam_l).callbacks(), x, gap_tol=gap_tol, **kw)
            assert np.array_equal(one.x, cv.paths[r_][l].x) and one.nit == cv.paths[r_][l].nit
            held = float(test.f(one.x)) / float((exposure * (ids == k)).sum())
            assert cv.scores[r_, l] == held
            ref = PC.PoissonRef(A, rate, lam_l, sample_weight=exposure * (ids == k)).f(one.x) / float((exposure * (ids == k)).sum())
            assert abs(held - ref) <= 1e-12 * abs(ref)
            x = one.x
    assert cv.lam_best in lams[1:4] and cv.lam_1se >= cv.lam_best and len(cv.path) == 3


# ---- (4) unchanged defaults and refusals ---------------------------------------------------------------------------------------------
# What solvers that never call zf_solver_set_poisson launched, planned and computed with the PARENT commit's library (recorded
# from that library on an MI355X in the session that added the Poisson loss): (launch counts, ls_plan, sha256 of
# the bytes of x_40).  40 iterations from lr = 1 with momentum.
PARENT = {
    "ls_small": [[0, 0], [1, 1, 64, 8], "140644d478064c34d9df6bf34441bbf3ed3161eee13154280815f0feb95de89c"],
    "ls_general": [[0, 0], [3, 2, 60, 10], "cdcc96d756b64be74285e8a105cc62bbf0ee1545c5a76059df1a6a25c1ba22ad"],
    "logistic": [[0, 0], [2, 2, 64, 8], "36ad5e3411402a8cdb0d1ac8c00ecf505878ea31b151144902baaf8e67c690f5"],
    "sparse": [[0, 0], [5, 16, 4, 0], "be38efb83e1d4dedd6671d89c8eeab69984bb8d45afbb4e87989a9ee7145f779"],
}


def _default_solves():
    from oracle import problems_ref as P
    from zfista_amd.problems import LeastSquaresL1, LogisticL1, SparseLeastSquaresL1

    A, b, lam = P.make_plasso(512, 1024, seed=0)
    A2, b2, lam2 = P.make_plasso(600, 3000, seed=1)
    S, bs, lams = PC.S.make_sparse(*PC.SMALL[0])
    return {
        "ls_small": lambda: LeastSquaresL1(A, b, lam),
        "ls_general": lambda: LeastSquaresL1(A2, b2, lam2),
        "logistic": lambda: LogisticL1(A, np.where(b > 0, 1.0, -1.0), lam),
        "sparse": lambda: SparseLeastSquaresL1(S, bs, lams),
    }


def _fingerprint(solve, make):
    prob = make()
    res, _, plan, counts = solve(prob, np.zeros(prob.n_features), lr=1, tol=0.0, max_iter=40, nesterov=True)
    assert res.nit == 40
    return [list(map(int, counts)), list(map(int, plan)), hashlib.sha256(np.ascontiguousarray(res.x).tobytes()).hexdigest()]


@pytest.mark.parametrize("name", sorted(PARENT))
def test_solvers_that_never_asked_launch_what_the_parent_library_launched(name, solve):
    """zf_solver_launch_counts, zf_solver_ls_plan and the bits of x_40 of a least-squares solve (fused small-matrix path and
    general path), a logistic solve and a sparse solve, made without the new call - also after a Poisson solve in between."""
    make = _default_solves()[name]
    got = _fingerprint(solve, make)
    print(name, json.dumps(got))
    A, b, lam = _data(PC.SMALL[0])
    solve(_make("dense", A, b, lam), np.zeros(A.shape[1]), lr=1, tol=0.0, max_iter=10, nesterov=True)
    assert _fingerprint(solve, make) == got, "a Poisson solve in between does not disturb the other classes"
    assert (got[1][0] == 1) == (name == "ls_small"), "the fused small-matrix path is taken where it was"
    assert got == PARENT[name]


def test_refusals_at_the_c_level_and_composition():
    import torch

    from oracle import problems_ref as P
    from zfista_amd import _lib
    from zfista_amd.engine import DeviceSolver
    from zfista_amd.problems import DiagQuadL1, LeastSquaresL1, LogisticL1

    A, b, lam = P.make_plasso(512, 1024, seed=0)
    counts = np.abs(np.round(b))
    options = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=3, max_backtrack_iter=10)
    fields, keep = LeastSquaresL1(A, counts, lam)._descriptor()
    w = torch.ones(512, dtype=torch.float64, device="cuda")
    s = DeviceSolver(fields, options, keepalive=keep)
    lib = s.lib
    assert s.ls_plan()[0] == 1, "the fused small-matrix path"
    assert lib.zf_solver_set_poisson(s.handle) == 0 and s.ls_plan()[0] == 2, "the call switches the small-matrix path off"
    assert lib.zf_solver_set_huber(s.handle, 0.5) == -2 and b"Poisson" in lib.zf_last_error(), "one loss per solver"   # ZF_ERR_ARG
    assert lib.zf_solver_set_poisson(s.handle) == 0, "asking twice is asking once"
    # any order with zf_solver_set_l2 and zf_solver_set_row_weights
    assert lib.zf_solver_set_l2(s.handle, 0.25) == 0 and lib.zf_solver_set_row_weights(s.handle, w.data_ptr()) == 0
    x0 = torch.zeros(1024, dtype=torch.float64, device="cuda")
    s.init(x0.data_ptr())
    assert lib.zf_solver_set_poisson(s.handle) == -3 and b"before" in lib.zf_last_error()   # ZF_ERR_STATE
    s.close()
    s = DeviceSolver(fields, options, keepalive=keep)
    assert lib.zf_solver_set_row_weights(s.handle, w.data_ptr()) == 0 and lib.zf_solver_set_l2(s.handle, 0.25) == 0
    assert lib.zf_solver_set_poisson(s.handle) == 0 and s.ls_plan()[0] == 2
    s.close()
    s = DeviceSolver(fields, options, keepalive=keep)
    assert lib.zf_solver_set_huber(s.handle, 0.5) == 0
    assert lib.zf_solver_set_poisson(s.handle) == -2 and b"Huber" in lib.zf_last_error()
    s.close()
    # other kinds
    d, c, lam_d = P.make_pdiag(1000, seed=1)
    for prob in (DiagQuadL1(d, c, lam_d), LogisticL1(A, np.where(b > 0, 1.0, -1.0), lam)):
        f2, k2 = prob._descriptor()
        s = DeviceSolver(f2, options, keepalive=k2)
        assert lib.zf_solver_set_poisson(s.handle) == -2 and b"only for" in lib.zf_last_error()
        s.close()
    # ZF_ACCEPT_REMAINDER
    s = DeviceSolver(fields, dict(options, accept_mode=_lib.ZF_ACCEPT_REMAINDER), keepalive=keep)
    assert lib.zf_solver_set_poisson(s.handle) == -2 and b"ZF_ACCEPT_REMAINDER" in lib.zf_last_error()
    s.close()


def test_refusals_of_the_python_classes():
    from zfista_amd import minimize_proximal_gradient as solve
    from zfista_amd.path import l1_path
    from zfista_amd.screening import solve_screened

    A, b, lam = _data(PC.GAP_CASE)
    n = A.shape[1]
    for storage in PC.FORMS:
        for bad in (-1.0, np.nan, np.inf):
            counts = b.copy()
            counts[3] = bad
            with pytest.raises(ValueError, match="counts b must be finite and >= 0"):
                _make(storage, A, counts, lam)
        with pytest.raises(ValueError, match="group="):
            _cls(storage)(PC.matrix(A, storage), b, lam, group=object())
        prob = _make(storage, A, b, lam)
        for call in (prob.column_norms, lambda: prob.screen(np.zeros(n)), lambda: prob.restrict(np.arange(5)),
                     lambda: solve_screened(prob, np.zeros(n), 1e-6), lambda: l1_path(prob, [lam], screen=True)):
            with pytest.raises(ValueError, match="globally Lipschitz"):
                call()
        for bad in ("remainder", "resolved"):
            with pytest.raises(ValueError, match="acceptance="):
                solve(*prob.callbacks(), np.zeros(n), acceptance=bad, max_iter=3)
        boxed = _make(storage, A, b, lam, bounds=(-1.0, 1.0))
        with pytest.raises(ValueError, match="bounds are set"):
            boxed.duality_gap(np.zeros(n))
        with pytest.raises(ValueError, match="bounds are set"):
            solve(*boxed.callbacks(), np.zeros(n), gap_tol=1e-6, max_iter=3)
