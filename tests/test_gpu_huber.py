"""GPU: Huber's loss on the trials of the least-squares classes (HuberL1, SparseHuberL1; csrc/zf_kernels_huber.h).

(1) Element bits of the row kernels: with A the sparse identity (and the same matrix densified where that fits) the margins
    are x exactly and, at scale 1/2, the gradient is c itself - bit for bit NumPy's copysign(min(|r|, delta), r); f inside
    its derived bound; the row counts around the unroll tail, the block stride and the change of shape; equal bits of f
    from both storage forms at every m; a NaN margin gives a NaN f.
(2) The first iterate against NumPy's expression, bit for bit; against the LeastSquaresL1 sibling's when nothing is clipped.
(3) Solves against the reference's fixture G17 (the comparisons and tolerances tests/test_gpu_enet.py applies to G16) and the
    tall shape against the CPU oracle on tests/huber_cases.HuberRef.
(4) The certificate: all eight / ten outputs inside the bounds derived in tests/huber_cases.py; the live solver's gap.
(5) Screening: the device mask against the exact long-double rule; solve_screened, l1_path(screen=True), restrict.
(6) gap_tol, snapshots, concurrent solves, the refusals at the C level, and that the other classes launch what they launched.

ZF_HUBER_BOUNDS_RECORD=1 appends the worst error-to-bound ratios to profiles/huber_kernel_bounds.jsonl and
profiles/huber_gap_bounds.jsonl (any other value: to files of those names in that directory) - records, not thresholds."""
import functools
import json
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import huber_cases as H
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-10
U = H.U
_id = lambda c: f"{c[0]}x{c[1]}"


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _cls(storage):
    from zfista_amd import problems as Z

    return Z.SparseHuberL1 if storage == "csr" else Z.HuberL1


def _make(storage, A, b, lam, delta, l2=0.0, bounds=None, scale=H.SCALE):
    return _cls(storage)(H.matrix(A, storage) if sp.issparse(A) else A, b, lam, delta, scale=scale, bounds=bounds, l2=l2)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _record(name, **rec):
    where = os.environ.get("ZF_HUBER_BOUNDS_RECORD", "")
    if where in ("", "0"):
        return
    path = os.path.join(os.path.join(ROOT, "profiles") if where == "1" else where, name)
    with open(path, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


@functools.lru_cache(maxsize=None)
def _data(case):
    """(A, b, lam, delta) of huber_cases.make_huber - read-only, shared."""
    return H.make_huber(case)


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


# ---- (1) element bits of the row kernels ------------------------------------------------------------------------------------------
DELTA = 0.75
ROWS = [1, 63, 64, 65, 1023, 1024, 1025, 2049, 32768, 32769, 40000]
DENSE_IDENTITY_MAX = 2049   # (an identity of 32768 rows is 8.6 GB in dense storage: beyond this, the dense class gets the m x 2
#                              matrix [z, 0] at x = (1, 0), whose margins are z exactly as well)


def _margins(m, kind, seed):
    """(z, b): margins and right-hand side on a grid of 2^-6, so that z - b is exact and |r| = delta happens exactly.
    Signed zeros: the row sums of every sweep start from +0 (`double acc = 0.0` in the SpMV and GEMV kernels), and
    +0 + (-0) = +0, so a margin of -0 reaches the row kernel as +0 and a c of -0 reaches the gradient as +0: the sign of a zero
    cannot be carried through either sweep, in or out.  What the rows with x = -0 pin is that c is 0 there and that f is, bit
    for bit, the f of the same rows with +0 (H = +-0 adds nothing to the sum)."""
    rng = np.random.default_rng(seed)
    b = rng.integers(-128, 129, m) / 64.0
    if kind == "none":       # every |r| < delta
        r = rng.integers(-47, 48, m) / 64.0
    elif kind == "all":      # every |r| > delta
        r = rng.choice([-1.0, 1.0], m) * rng.integers(49, 400, m) / 64.0
    else:                    # mixed, with |r| = delta exactly, r = 0 and values that are no grid points
        r = rng.integers(-120, 121, m) / 64.0
        r[::7] = rng.choice([-1.0, 1.0], r[::7].size) * DELTA
        r[3::11] = 0.0
        odd = slice(5, None, 13)
        r[odd] = r[odd] + 1e-3 * rng.standard_normal(r[odd].size)
        z = b + r
        z[9::17], b[9::17] = -0.0, 0.0    # a margin of -0 against b = +0: in NumPy r = -0, c = -0, H = -0
        z[10::17], b[10::17] = 0.0, -0.0  # and r = +0 from b = -0
        return z, b
    return b + r, b


def _eval_both(m, z, b):
    """f and the gradient of both classes at margins z: {storage: (f, grad or None)}; the dense gradient only for the identity."""
    I = sp.identity(m, format="csr", dtype=np.float64)
    out = {}
    ps = _make("csr", I, b, 0.1, DELTA)
    out["csr"] = (ps.f(z), ps.jac_f(z))
    if m <= DENSE_IDENTITY_MAX:
        pd = _make("dense", np.eye(m), b, 0.1, DELTA)
        out["dense"] = (pd.f(z), pd.jac_f(z))
    else:
        pd = _make("dense", np.stack([z, np.zeros(m)], axis=1), b, 0.1, DELTA)
        x = np.array([1.0, 0.0])
        out["dense"] = (pd.f(x), None)
        g = pd.jac_f(x)   # = (sum z_i c_i, 0): the kernel at y wrote the same c
        c, _ = H.huber_terms(z.astype(np.longdouble) - b.astype(np.longdouble), np.longdouble(DELTA))
        exact = float(np.sum(z.astype(np.longdouble) * c))
        assert abs(g[0] - exact) <= 2 * (m + 2) * U * float(np.sum(np.abs(z * c.astype(np.float64)))) and g[1] == 0.0
    return out


@pytest.mark.parametrize("kind", ["mixed", "all", "none"])
@pytest.mark.parametrize("m", ROWS)
def test_row_kernels_element_bits(m, kind):
    z, b = _margins(m, kind, seed=m)
    r = z - b
    c, Hv = H.huber_terms(r, DELTA)
    clipped = np.abs(r) > DELTA
    assert {"mixed": 0 < clipped.sum() < m or m == 1, "all": clipped.all(), "none": not clipped.any()}[kind]
    f_exact, f_bound, _, _ = H.loss_longdouble(z, b, DELTA, H.SCALE)
    got = _eval_both(m, z, b)
    worst = 0.0
    for storage, (f, grad) in got.items():
        err = abs(float(np.longdouble(f) - f_exact))
        ratio = 0.0 if err == 0.0 else err / f_bound
        worst = max(worst, ratio)
        print(f"m={m} {kind} {storage}: f {float(f):.17g}, error / bound {ratio:.3g}")
        assert np.isfinite(f) and f >= 0 and ratio <= 1.0, (storage, f, float(f_exact), f_bound)
        if grad is not None:   # scale 1/2: the gradient is c itself
            nz = c != 0.0
            bad = np.flatnonzero(_bits(grad)[nz] != _bits(c)[nz])
            assert bad.size == 0, (storage, bad[:8], grad[nz][bad[:8]], c[nz][bad[:8]])
            assert (grad[~nz] == 0.0).all()   # (either sign: see _margins)
    assert _bits(got["csr"][0]) == _bits(got["dense"][0]), "both classes sum a loss of the same m in the same order"
    if kind == "mixed" and m > 10:
        assert np.signbit(z[9]) and np.signbit(c[9]) and c[9] == 0.0 and not np.signbit(c[10]), "the inputs hold both zeros"
        plus = _make("csr", sp.identity(m, format="csr", dtype=np.float64), np.where(b == 0.0, 0.0, b), 0.1, DELTA).f(np.where(z == 0.0, 0.0, z))
        assert _bits(plus) == _bits(got["csr"][0]), "rows with r = -0 add nothing to f"
    if kind == "none":
        assert float(got["csr"][0]) == pytest.approx(0.5 * float(np.sum(r * r)), rel=1e-13)
    _record("huber_kernel_bounds.jsonl", test="rows", m=m, kind=kind, f_ratio=worst, clipped=int(clipped.sum()))


@pytest.mark.parametrize("m", [65, 2049, 32769])
def test_a_nan_margin_gives_a_nan_f_and_an_inf_margin_an_inf_f(m):
    """One bad margin among m: the sparse class on the identity at x = z, the dense class on the m x 2 matrix [z, 0] at
    x = (1, 0) - in both only that row's margin is not finite (a dense identity would spread 0 * NaN over every row)."""
    z, b = _margins(m, "mixed", seed=m + 1)
    sparse = _make("csr", sp.identity(m, format="csr", dtype=np.float64), b, 0.1, DELTA)
    e1 = np.array([1.0, 0.0])
    f_of = {"csr": lambda v: sparse.f(v), "dense": lambda v: _make("dense", np.stack([v, np.zeros(m)], axis=1), b, 0.1, DELTA).f(e1)}
    for storage, f in f_of.items():
        assert np.isfinite(f(z)), storage
        for k in (0, m // 2, m - 1):
            bad = z.copy()
            bad[k] = np.nan
            assert np.isnan(f(bad)), (storage, k, "v_min_f64 drops the NaN: 2 r - c must carry it")
        bad = z.copy()
        bad[m // 3] = np.inf
        assert f(bad) == np.inf, storage


# ---- (2) the first iterate -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,n", [("csr", 7001), ("dense", 1000)])
def test_first_iterate_is_numpys_expression_bit_for_bit(storage, n, solve, monkeypatch):
    """A = I, scale 1/2, lr = 1/2 (f is 1-smooth: the first trial is accepted): y = x0, g = c exactly, so
    x_1 = clip(copysign(max(|v| - lam lr, 0), v) * shrink), v = x0 - lr * c - with and without the box, with and without l2,
    at 1 and at 3 tiles per workgroup."""
    from zfista_amd import _lib

    rng = np.random.default_rng(n)
    x0, b = _margins(n, "mixed", seed=n + 7)
    x0, b = np.where(x0 == 0.0, 0.0, x0), np.where(b == 0.0, 0.0, b)   # (zeros of one sign: see _margins; here x0 is the iterate too)
    r = x0 - b
    c, _ = H.huber_terms(r, DELTA)
    lr, lam = 0.5, 0.3
    A = sp.identity(n, format="csr", dtype=np.float64) if storage == "csr" else np.eye(n)
    box = (-1.25, 1.5)
    for tiles in ("1", "3"):
        monkeypatch.setenv("ZF_TILES_PER_WG", tiles)
        for l2 in (0.0, 0.6):
            for bounds in (None, box):
                res, rows, plan, _ = solve(_make(storage, A, b, lam, DELTA, l2=l2, bounds=bounds), x0, lr=lr, tol=0.0, max_iter=1,
                                           nesterov=True)
                assert rows[:, _lib.TR_TRIALS].tolist() == [1.0] and res.nit == 1 and plan[0] != 1
                v = x0 - lr * c
                want = np.copysign(np.maximum(np.abs(v) - lam * lr, 0.0), v)
                if l2 > 0:
                    want = want * (1.0 / (1.0 + l2 * lr))
                if bounds is not None:
                    want = np.clip(want, *bounds)
                    assert np.count_nonzero(want == box[0]) >= 3 and np.count_nonzero(want == box[1]) >= 3, "the box must be active"
                bad = np.flatnonzero(_bits(res.x) != _bits(want))
                assert bad.size == 0, (tiles, l2, bounds, bad[:8], res.x[bad[:8]], want[bad[:8]])
                assert np.count_nonzero(want == 0.0) >= 5 and np.count_nonzero(np.abs(r) > DELTA) >= 5


@pytest.mark.parametrize("storage", H.FORMS)
@pytest.mark.parametrize("case", [H.SMALL[2], H.SMALL[3]], ids=_id)
def test_first_iterate_equals_the_least_squares_siblings_when_nothing_is_clipped(case, storage, solve):
    from zfista_amd import _lib, problems as Z

    A, b, lam, _ = _data(case)
    n = A.shape[1]
    M = H.matrix(A, storage)
    kw = dict(lr=2.0 ** -12, tol=0.0, max_iter=1, nesterov=True)
    sib = (Z.SparseLeastSquaresL1 if storage == "csr" else Z.LeastSquaresL1)(M, b, lam, scale=H.SCALE)
    base, rows0, plan0, _ = solve(sib, np.zeros(n), **kw)
    assert plan0[0] != 1, "the sibling must take the general path for its sums to be these"
    for delta in (float(np.max(np.abs(b))), 2.0 * float(np.max(np.abs(b)))):
        res, rows, plan, _ = solve(_make(storage, A, b, lam, delta), np.zeros(n), **kw)
        assert rows[:, _lib.TR_TRIALS].tolist() == rows0[:, _lib.TR_TRIALS].tolist() == [1.0]
        assert np.array_equal(_bits(res.x), _bits(base.x)) and np.count_nonzero(res.x) > 0
        assert abs(float(res.fun) - float(base.fun)) <= 1e-11 * abs(float(base.fun)), "F(x_1): the same number from two summation forms"


# ---- (3) solves ------------------------------------------------------------------------------------------------------------------
SOLVES = [(ci, fi, st, tag) for ci in range(len(H.SMALL)) for fi, st, tag in H.GOLDEN_SOLVES]


@pytest.mark.parametrize("ci,fi,storage,tag", SOLVES)
def test_solve_vs_reference_fixture(golden, ci, fi, storage, tag, solve):
    """80 iterations from lr = 1 against what the REFERENCE solver produced on the closures (tests/golden/make_golden_huber.py)."""
    from zfista_amd import _lib

    G = golden("g17_huber.npz")
    A, b, lam, delta = _data(H.SMALL[ci])
    assert lam == float(G(f"huber.c{ci}.lam")) and delta == float(G(f"huber.c{ci}.delta"))
    res, rows, plan, _ = solve(_make(storage, A, b, lam, delta, l2=fi * lam), np.zeros(A.shape[1]), **H.GOLDEN_KW, **H.GOLDEN_VARIANTS[tag])
    pre = H.golden_prefix(ci, fi, storage, tag)
    assert plan[0] == 5 if storage == "csr" else plan[0] in (2, 3, 4)
    assert res.nit == int(G(f"{pre}.nit")) == 80
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), G(f"{pre}.alltrials")) and rows[:, _lib.TR_TRIALS].sum() > 80
    assert np.array_equal(rows[:, _lib.TR_LR], G(f"{pre}.alllrs"))
    assert rel_err(res.x, G(f"{pre}.x")) <= TOL
    assert abs(np.linalg.norm(res.x) - float(G(f"{pre}.xnorm"))) <= TOL * float(G(f"{pre}.xnorm"))
    for k, v in zip(G(f"{pre}.kept"), G(f"{pre}.vecs")):
        assert rel_err(res.allvecs[k][::H.GOLDEN_STRIDE], v) <= TOL, k
    np.testing.assert_allclose(res.allfuns, G(f"{pre}.allfuns"), rtol=TOL, atol=0)
    assert rel_err(res.allerrs, G(f"{pre}.allerrs")) <= TOL
    np.testing.assert_allclose(res.allerrs, G(f"{pre}.allerrs"), rtol=TOL, atol=2 * TOL * float(G(f"{pre}.xnorm")))
    share = H.clipped_share(A, b, res.x, delta)
    assert H.SHARE[0] <= share <= H.SHARE[1], share


_ORACLE = {}


def _oracle_tall():
    from oracle import cpu_ref

    if "tall" not in _ORACLE:
        A, b, lam, delta = _data(H.TALL)
        ref = H.HuberRef(A, b, lam, delta)
        _ORACLE["tall"] = _quiet(cpu_ref.minimize_proximal_gradient, *ref.callbacks(), np.zeros(A.shape[1]), lr=1, tol=0.0, max_iter=80,
                                 nesterov=True, return_all=True)
    return _ORACLE["tall"]


@pytest.mark.parametrize("storage", H.FORMS)
def test_tall_solve_vs_oracle(storage, solve):
    """40 000 rows: the many-workgroup shape of the loss kernels inside a live solve with momentum, every iterate against the
    CPU oracle on HuberRef."""
    from zfista_amd import _lib

    A, b, lam, delta = _data(H.TALL)
    exp = _oracle_tall()
    res, rows, plan, _ = solve(_make(storage, A, b, lam, delta), np.zeros(A.shape[1]), lr=1, tol=0.0, max_iter=80, nesterov=True, return_all=True)
    assert exp.nit == 80 and sum(exp.alltrials) > 80
    assert res.nit == exp.nit
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), np.asarray(exp.alltrials, np.int64))
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float))
    assert max(rel_err(a, e) for a, e in zip(res.allvecs, exp.allvecs)) <= TOL
    np.testing.assert_allclose(res.allfuns, exp.allfuns, rtol=TOL, atol=0)
    assert rel_err(res.allerrs, exp.allerrs) <= TOL
    shares = [H.clipped_share(A, b, res.allvecs[k], delta) for k in (0, 80)]
    assert all(H.SHARE[0] <= s <= H.SHARE[1] for s in shares), shares


# ---- (4) the certificate -----------------------------------------------------------------------------------------------------------
def _gap_bits(gp, keys):
    return np.array([getattr(gp, k) for k in keys]).view(np.uint64)


@pytest.mark.parametrize("storage", H.FORMS)
@pytest.mark.parametrize("fac", [0.0, 1.0], ids=["l1", "l2=lam"])
@pytest.mark.parametrize("case", H.SMALL, ids=_id)
def test_every_output_within_its_rounding_bound(case, fac, storage, solve):
    """problem.duality_gap(x) at x = 0 and at the iterates 20 and 400 of a FISTA solve: all eight (l2 = 0) / ten (l2 = lam)
    outputs inside the bounds of tests/huber_cases.py."""
    A, b, lam, delta = _data(case)
    l2 = fac * lam
    keys = H.KEYS10 if l2 > 0 else H.KEYS8
    prob = _make(storage, A, b, lam, delta, l2=l2)
    n = A.shape[1]
    res, _, _, _ = solve(prob, np.zeros(n), lr=1, tol=0.0, max_iter=400, nesterov=True, return_all=True)
    assert res.nit == 400
    gaps = []
    for k in (0, 20, 400):
        x = np.asarray(res.allvecs[k])
        vals, bounds, extra = H.gap_longdouble(A, b, x, lam, delta, l2=l2)
        got = prob.duality_gap(x)
        ratios = H.worst_ratio(got, vals, bounds)
        worst = max(ratios, key=ratios.get)
        print(f"{_id(case)} {storage} l2 = {fac} lam, x_{k}: worst error / bound {ratios[worst]:.3g} ({worst}); gap {float(got.gap):.6g} "
              f"alpha {float(got.alpha):.6g} rows {float(got.rows_gap):.3g} clipped {extra['share']:.3f}")
        _record("huber_gap_bounds.jsonl", case=_id(case), storage=storage, l2_over_lam=fac, iterate=k, worst=worst, ratio=ratios[worst],
                ratios=ratios, gap=float(got.gap), clipped=extra["share"])
        assert all(np.isfinite(getattr(got, key)) for key in keys), got
        assert ratios[worst] <= 1.0, (k, worst, ratios, got)
        assert got.gap >= 0 and got.rows_gap >= 0 and got.ridge_gap >= 0 and got.gap >= (got.rows_gap + got.ridge_gap) * (1 - 4 * U)
        if l2 == 0:
            assert got.g_l2 == 0.0 and got.ridge_gap == 0.0
        gaps.append(float(got.gap))
    assert gaps[2] < gaps[0]
    x = np.asarray(res.allvecs[400])
    assert np.array_equal(_gap_bits(prob.duality_gap(x), keys), _gap_bits(prob.duality_gap(x), keys)), "two evaluations: the same bits"


@pytest.mark.parametrize("storage", H.FORMS)
def test_the_certificate_on_the_tall_shape_and_the_least_squares_limit(storage):
    """40 000 rows: the chunked rows pass and its two finishes.  With delta beyond every residual the eight values are the
    least-squares sibling's to rounding (the sums are taken by other kernels: not bit for bit)."""
    from zfista_amd import problems as Z

    A, b, lam, delta = _data(H.TALL)
    n = A.shape[1]
    rng = np.random.default_rng(9)
    x = np.zeros(n)
    x[rng.choice(n, 30, replace=False)] = 0.05 * rng.standard_normal(30)
    for l2 in (0.0, lam):
        prob = _make(storage, A, b, lam, delta, l2=l2)
        vals, bounds, extra = H.gap_longdouble(A, b, x, lam, delta, l2=l2)
        got = prob.duality_gap(x)
        ratios = H.worst_ratio(got, vals, bounds)
        print(f"tall {storage} l2 {l2:.3g}: worst error / bound {max(ratios.values()):.3g}; clipped {extra['share']:.3f}")
        _record("huber_gap_bounds.jsonl", case=_id(H.TALL), storage=storage, l2_over_lam=float(l2 > 0), iterate="random", ratios=ratios,
                ratio=max(ratios.values()), gap=float(got.gap), clipped=extra["share"])
        assert 0.05 <= extra["share"] <= 0.95 and max(ratios.values()) <= 1.0, ratios
    wide = 2.0 * float(np.max(np.abs(A @ x - b)))
    hub = _make(storage, A, b, lam, wide).duality_gap(x)
    ls = (Z.SparseLeastSquaresL1 if storage == "csr" else Z.LeastSquaresL1)(H.matrix(A, storage), b, lam, scale=H.SCALE).duality_gap(x)
    for k in H.KEYS8:   # (absolute, in units of P: D and the gap are differences of sums of that size)
        assert abs(float(getattr(hub, k)) - float(getattr(ls, k))) <= 1e-11 * max(float(ls.primal), 1.0), k
    assert hub.alpha == ls.alpha and hub.grad_inf == ls.grad_inf, "the same candidate through the same sweep"


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


@pytest.mark.parametrize("fac", [0.0, 1.0], ids=["l1", "l2=lam"])
@pytest.mark.parametrize("storage", H.FORMS)
def test_the_gap_of_a_live_solve(storage, fac):
    """NativeRun.duality_gap() equals the standalone evaluation at get_x() bit for bit (a Huber solve is always on the general
    path: the margins come from the same kernels), and a solve probed after every pass - also between a rejected trial and
    its retry - is the solve that was never asked, bit for bit."""
    A, b, lam, delta = _data(H.SMALL[1])   # n = 5000: more than one gap chunk
    l2 = fac * lam
    keys = H.KEYS10 if l2 > 0 else H.KEYS8
    prob = _make(storage, A, b, lam, delta, l2=l2)
    passes = 24
    plain = _walk(prob, passes)
    assert plain["trials"] > plain["nit"] > 0, "the case must backtrack and accept"
    probed = _walk(prob, passes, gap_after=range(passes))
    assert (plain["nit"], plain["lr"], plain["F"], plain["trials"]) == (probed["nit"], probed["lr"], probed["F"], probed["trials"])
    assert np.array_equal(plain["rows"], probed["rows"]) and np.array_equal(plain["x"], probed["x"])
    assert probed["after_reject"] >= 1, "no gap call fell between a rejected trial and its retry"
    assert plain["counts"] == probed["counts"]
    live, alone = probed["gaps"][passes - 1], prob.duality_gap(probed["x"])
    assert np.array_equal(_gap_bits(live, keys), _gap_bits(alone, keys)), (live, alone)
    vals, bounds, _ = H.gap_longdouble(A, b, probed["x"], lam, delta, l2=l2)
    ratios = H.worst_ratio(live, vals, bounds)
    assert max(ratios.values()) <= 1.0, ratios
    assert live.gap < probed["gaps"][0].gap and (live.g_l2 > 0) == (l2 > 0)


# ---- (5) screening ---------------------------------------------------------------------------------------------------------------
# (shape, lam / lam_max): fractions at which, on the CPU oracle's iterates, the rule discards 1 / 1 / 239, 2 / 2 / 858 and
# 211 / 223 / 4061 columns at x_0 / x_20 / x_400 while the gap stays 2^20 times above its own rounding bound (a larger lam
# brings these solves to a gap of rounding size within 400 iterations, where the precondition of the guard no longer holds)
MASK_SHAPES = {257: ((100, 257, 0.1, 11), 0.4), 1000: (H.SMALL[0], 0.35), 4099: (H.SMALL[3], 0.8)}


@pytest.mark.parametrize("storage", H.FORMS)
@pytest.mark.parametrize("n", [257, 1000, 4099])
def test_the_mask_is_the_exact_rules(n, storage):
    """The device mask against the exact long-double rule at x = 0 and after 20 and 400 iterations: safe, tight within the
    guard, and - as for the least-squares classes on these shapes - equal to it."""
    from zfista_amd import minimize_proximal_gradient as solve

    shape, frac = MASK_SHAPES[n]
    A, b, _, delta = _data(shape)
    assert A.shape[1] == n
    lam = frac * H.lam_max(A, b, delta)
    prob = _make(storage, A, b, lam, delta)
    discarded = []
    for its in (0, 20, 400):
        x = np.zeros(n) if its == 0 else _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=its, lr=1.0, nesterov=True, tol=0.0).x
        ref = H.screen_longdouble(A, b, x, lam, delta, dense=storage == "dense")
        gap, d_gap = float(ref["vals"]["gap"]), ref["bounds"]["gap"]
        print(f"n={n} {storage} its={its}: gap {gap:.4g}, d_gap / gap = {d_gap / gap * 2.0 ** 20:.3g} x 2^-20")
        assert gap > 0 and d_gap / gap <= 2.0 ** -20, "the precondition of E (from the gap's own bound)"
        sc = prob.screen(x)
        gp, keep_dev, count = sc
        keep = keep_dev.cpu().numpy()
        out = ~keep
        wrong = out & ~ref["discard"]
        assert not wrong.any(), ("the device discards a column the exact rule keeps", np.flatnonzero(wrong))
        norms = ref["norms"]
        slack = np.longdouble(lam) - ref["left"]
        must = slack > np.longdouble(2.0 * ref["E"]) * norms + np.longdouble(lam * 2.0 ** -40)
        missed = must & keep
        assert not missed.any(), ("the device keeps a column the exact rule discards with slack", np.flatnonzero(missed))
        amb = keep & ref["discard"]
        print(f"   discarded {int(out.sum())} (exact rule: {int(ref['discard'].sum())}); kept inside the guard: {int(amb.sum())}")
        assert abs(float(sc.radius) - float(ref["radius"])) <= 2.0 ** -20 * float(ref["radius"])
        assert 0.5 * ref["E"] <= float(sc.guard) <= 2.0 * ref["E"]
        index = sc.index.cpu().numpy()
        assert np.array_equal(index, np.cumsum(keep) - keep) and count == int(keep.sum())
        alone = prob.duality_gap(x)
        assert np.array_equal(_gap_bits(gp, H.KEYS8), _gap_bits(alone, H.KEYS8))
        _record("huber_gap_bounds.jsonl", test="mask", n=n, storage=storage, its=its, gap=gap, precondition=d_gap / gap * 2.0 ** 20,
                discarded=int(out.sum()), exact_discarded=int(ref["discard"].sum()), E=float(sc.guard), E_ref=ref["E"])
        assert np.array_equal(out, ref["discard"]), "the device mask equals the exact rule's"
        discarded.append(int(out.sum()))
    assert discarded[-1] > discarded[0] and discarded[-1] > n // 2, ("the rule must bite along the trajectory", discarded)


@pytest.mark.parametrize("storage", H.FORMS)
def test_screened_solves_reach_gap_tol_with_the_full_problems_certificate(storage):
    """solve_screened and l1_path(screen=True) on the 1000 x 257 case (the one of the four that a first-order method brings to
    1e-6 P(0) within a few hundred iterations); restrict keeps delta."""
    from zfista_amd.path import l1_path
    from zfista_amd.screening import solve_screened

    A, b, lam, delta = _data(H.SMALL[2])
    n = A.shape[1]
    prob = _make(storage, A, b, lam, delta)
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=4000)
    lmax = float(prob.lam_max())
    assert abs(lmax - H.lam_max(A, b, delta)) <= 1e-12 * lmax
    # at lam_max / 2 and 1e-9 P(0) the rule has discarded most columns long before the target is met (on the CPU oracle: 239 of
    # 257 at a gap of 5e-5 P(0)), so restricted Huber problems are solved on the way
    half = prob.with_lam(0.5 * lmax)
    tight = 1e-9 * float(H.primal_longdouble(A, b, np.zeros(n), half.lam, delta))
    res = _quiet(solve_screened, half, np.zeros(n), tight, **kw)
    print(f"{storage}: rounds {[(r['nit'], r['kept'], r['restricted']) for r in res.screen]}, gap {float(res.dual_gap):.3g} <= {tight:.3g}")
    assert res.success and 0 <= res.dual_gap <= tight and res.dual_gap == half.duality_gap(res.x).gap
    assert any(r["restricted"] for r in res.screen), "a restricted problem must have been solved"
    vals, _, _ = H.gap_longdouble(A, b, res.x, half.lam, delta)
    assert float(vals["gap"]) <= tight * (1 + 1e-6)
    gap_tol = 1e-6 * float(H.primal_longdouble(A, b, np.zeros(n), lam, delta))
    lams = [lmax * f for f in (1.0000001, 0.5, 0.25, 0.1)]
    path = _quiet(l1_path, prob, lams, gap_tol=gap_tol, screen=True, **kw)
    plain = _quiet(l1_path, prob, lams, gap_tol=gap_tol, **kw)
    assert not path[0].x.any()
    for lam_k, r, p in zip(lams, path, plain):
        sib = prob.with_lam(lam_k)
        assert sib.delta == delta and sib.b.data_ptr() == prob.b.data_ptr()
        assert r.success and r.dual_gap <= gap_tol and r.dual_gap == sib.duality_gap(r.x).gap
        assert p.success and abs(float(r.fun) - float(p.fun)) <= 2 * gap_tol
    # restrict carries delta and l2
    keep = np.arange(0, n, 2)
    sub = prob.with_penalty(lam, 0.25).restrict(keep)
    assert type(sub) is type(prob) and sub.delta == delta and sub.l2 == 0.25 and sub.n_features == keep.size
    xs = 0.05 * np.random.default_rng(0).standard_normal(keep.size)
    xf = np.zeros(n)
    xf[keep] = xs
    assert abs(float(sub.f(xs)) - float(prob.f(xf))) <= 1e-12 * float(prob.f(xf))
    np.testing.assert_allclose(sub.jac_f(xs), prob.jac_f(xf)[keep], rtol=1e-11, atol=1e-13)
    with pytest.raises(ValueError, match="l2 > 0"):
        prob.with_penalty(lam, 0.25).screen(np.zeros(n))


# ---- (6) stopping, snapshots, streams, refusals, nothing moved ---------------------------------------------------------------------
@pytest.mark.parametrize("storage", H.FORMS)
def test_gap_tol_stops_the_solve_with_a_valid_certificate(storage):
    from zfista_amd import minimize_proximal_gradient as solve

    A, b, lam, delta = _data(H.SMALL[2])
    prob = _make(storage, A, b, lam, delta)
    n = A.shape[1]
    P0 = float(H.primal_longdouble(A, b, np.zeros(n), lam, delta))
    gap_tol = 1e-6 * P0
    kw = dict(lr=1.0, nesterov=True, tol=0.0)
    res = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=4000, gap_tol=gap_tol, **kw)
    assert res.success and res.status == 1 and res.message == "Duality gap reached gap_tol" and res.nit < 4000
    assert 0 <= res.dual_gap <= gap_tol and res.dual_gap == prob.duality_gap(res.x).gap
    plain = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=res.nit, **kw)
    assert plain.nit == res.nit and np.array_equal(plain.x, res.x) and plain.fun == res.fun, "the keyword does not alter the iterates"
    far = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=3000, **kw)
    excess = H.primal_longdouble(A, b, res.x, lam, delta) - H.primal_longdouble(A, b, far.x, lam, delta)
    print(f"{storage}: stopped at nit {res.nit}, gap {float(res.dual_gap):.3g} <= {gap_tol:.3g}; P(x) - P(x_3000) = {float(excess):.3g}")
    assert np.longdouble(res.dual_gap) >= excess
    for bad in ("remainder", "resolved"):
        with pytest.raises(ValueError, match="acceptance="):
            solve(*prob.callbacks(), np.zeros(n), acceptance=bad, max_iter=3)


def test_zf_accept_remainder_in_the_environment_falls_back_to_the_reference_test(monkeypatch):
    from zfista_amd import minimize_proximal_gradient as solve

    A, b, lam, delta = _data(H.SMALL[2])
    prob = _make("csr", A, b, lam, delta)
    n = A.shape[1]
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=40)
    plain = _quiet(solve, *prob.callbacks(), np.zeros(n), **kw)
    monkeypatch.setenv("ZF_ACCEPT", "remainder")
    env = _quiet(solve, *prob.callbacks(), np.zeros(n), **kw)
    assert np.array_equal(env.x, plain.x) and env.nit == plain.nit == 40 and "acceptance" not in env


_OPTS = dict(lr=1, tol=0.0, tol_internal=1e-12, max_iter=70, max_iter_internal=100000, max_backtrack_iter=100, warm_start=False,
             decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False, deprecated=False)


def _drain(run, step=5):
    from zfista_amd import _lib

    rows = [np.zeros((0, _lib.ZF_TRACE_COLS))]
    while run.status == _lib.ZF_RUNNING:
        rows.append(run.advance(step))
    return np.concatenate(rows)


@pytest.mark.parametrize("l2fac", [0.0, 1.0], ids=["l1", "l2=lam"])
@pytest.mark.parametrize("storage", H.FORMS)
def test_snapshot_resume_is_bit_identical(storage, l2fac, tmp_path):
    """from_snapshot recreates the solver from the problem - which sets delta (and l2) again - and continues bit for bit."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    A, b, lam, delta = _data(H.SMALL[0])
    prob = _make(storage, A, b, lam, delta, l2=l2fac * lam)
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

    A, b, lam, delta = _data(H.SMALL[1] if which == "small" else H.TALL)
    n = A.shape[1]
    prob = _make("csr", A, b, lam, delta)
    ratios = [(0, 0.25), (0.5, 1 / 16), (0.75, 0.25), (0.25, 1 / 64)]
    kws = [dict(lr=1, tol=0.0, max_iter=60, nesterov=True, nesterov_ratio=r, return_all=(k % 2 == 0)) for k, r in enumerate(ratios)]
    alone = [_quiet(minimize_proximal_gradient, *prob.callbacks(), np.zeros(n), **kw) for kw in kws]
    four = solve_on_streams([(prob, np.zeros(n), kw) for kw in kws], streams=4)
    for a, c in zip(alone, four):
        assert a.nit == c.nit == 60 and np.array_equal(a.x, c.x) and a.fun == c.fun
        if a.allfuns is not None:
            assert np.array_equal(np.asarray(a.allfuns), np.asarray(c.allfuns)) and np.array_equal(np.asarray(a.allvecs), np.asarray(c.allvecs))


def test_callables_against_the_closures():
    """f, jac_f, g, prox_wsum_g and lam_max of both classes against HuberRef on the 2000 x 5000 case."""
    A, b, lam, delta = _data(H.SMALL[1])
    n = A.shape[1]
    rng = np.random.default_rng(4)
    x = np.zeros(n)
    x[rng.choice(n, 40, replace=False)] = 0.1 * rng.standard_normal(40)
    ref = H.HuberRef(A, b, lam, delta, l2=0.5 * lam)
    for storage in H.FORMS:
        prob = _make(storage, A, b, lam, delta, l2=0.5 * lam)
        assert abs(float(prob.f(x)) - ref.f(x)) <= 1e-12 * ref.f(x)
        np.testing.assert_allclose(prob.jac_f(x), ref.jac_f(x), rtol=1e-11, atol=1e-12)
        assert abs(float(prob.g(x)) - ref.g(x)) <= 1e-12 * ref.g(x)
        v = 0.01 * rng.standard_normal(n)
        assert np.array_equal(prob.prox_wsum_g(0.37, v), ref.prox_wsum_g(0.37, v))
        assert abs(float(prob.lam_max()) - H.lam_max(A, b, delta)) <= 1e-12 * H.lam_max(A, b, delta)
        assert 0.05 <= H.clipped_share(A, b, x, delta) <= 0.95


def test_refusals_at_the_c_level_and_composition_with_l2():
    import torch

    from oracle import problems_ref as P
    from zfista_amd import _lib
    from zfista_amd.engine import DeviceSolver
    from zfista_amd.problems import DiagQuadL1, LeastSquaresL1, LogisticL1

    A, b, lam = P.make_plasso(512, 1024, seed=0)
    options = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=3, max_backtrack_iter=10)
    fields, keep = LeastSquaresL1(A, b, lam)._descriptor()
    s = DeviceSolver(fields, options, keepalive=keep)
    lib = s.lib
    assert s.ls_plan()[0] == 1, "the fused small-matrix path"
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.zf_solver_set_huber(s.handle, bad) == -2 and b"delta" in lib.zf_last_error()   # ZF_ERR_ARG
    assert s.ls_plan()[0] == 1, "a refused call leaves the solver as it was"
    # either order with zf_solver_set_l2
    assert lib.zf_solver_set_huber(s.handle, 0.5) == 0 and s.ls_plan()[0] == 2, "delta switches the small-matrix path off"
    assert lib.zf_solver_set_l2(s.handle, 0.25) == 0 and lib.zf_solver_set_huber(s.handle, 0.75) == 0
    x0 = torch.zeros(1024, dtype=torch.float64, device="cuda")
    s.init(x0.data_ptr())
    assert lib.zf_solver_set_huber(s.handle, 0.25) == -3 and b"before" in lib.zf_last_error()   # ZF_ERR_STATE
    s.close()
    s = DeviceSolver(fields, options, keepalive=keep)
    assert lib.zf_solver_set_l2(s.handle, 0.25) == 0 and lib.zf_solver_set_huber(s.handle, 0.75) == 0 and s.ls_plan()[0] == 2
    s.close()
    # other kinds
    d, c, lam_d = P.make_pdiag(1000, seed=1)
    for prob in (DiagQuadL1(d, c, lam_d), LogisticL1(A, np.where(b > 0, 1.0, -1.0), lam)):
        f2, k2 = prob._descriptor()
        s = DeviceSolver(f2, options, keepalive=k2)
        assert lib.zf_solver_set_huber(s.handle, 0.5) == -2 and b"only for" in lib.zf_last_error()
        s.close()
    # ZF_ACCEPT_REMAINDER
    s = DeviceSolver(fields, dict(options, accept_mode=_lib.ZF_ACCEPT_REMAINDER), keepalive=keep)
    assert lib.zf_solver_set_huber(s.handle, 0.5) == -2 and b"ZF_ACCEPT_REMAINDER" in lib.zf_last_error()
    s.close()


def test_a_huber_solve_in_between_does_not_disturb_the_other_classes(solve):
    """A least-squares solve before and after a Huber solve on the same matrix, and a logistic solve twice: the same plan,
    launch counts and bits; the small least-squares matrix still takes the fused path and the Huber problem on it does not.
    (The comparison of the launch counts with the parent commit's is a measurement: DESIGN 4.5g.)"""
    from oracle import problems_ref as P
    from zfista_amd.problems import HuberL1, LeastSquaresL1, LogisticL1

    A, b, lam = P.make_plasso(512, 1024, seed=0)
    kw = dict(lr=1, tol=0.0, max_iter=40, nesterov=True)
    ls1, rows1, plan1, counts1 = solve(LeastSquaresL1(A, b, lam), np.zeros(1024), **kw)
    hub, _, plan_h, _ = solve(HuberL1(A, b, lam, float(np.median(np.abs(b)))), np.zeros(1024), **kw)
    ls2, rows2, plan2, counts2 = solve(LeastSquaresL1(A, b, lam), np.zeros(1024), **kw)
    assert plan1[:2] == plan2[:2] == (1, 1) and counts1 == counts2 and np.array_equal(rows1, rows2) and np.array_equal(ls1.x, ls2.x)
    assert plan_h[:2] == (2, 2) and hub.nit == 40 and not np.array_equal(hub.x, ls1.x)
    labels = np.where(b > 0, 1.0, -1.0)
    lg1, rl1, pl1, cl1 = solve(LogisticL1(A, labels, lam), np.zeros(1024), **kw)
    lg2, rl2, pl2, cl2 = solve(LogisticL1(A, labels, lam), np.zeros(1024), **kw)
    assert pl1 == pl2 and cl1 == cl2 and np.array_equal(rl1, rl2) and np.array_equal(lg1.x, lg2.x)
