"""GPU: every output of the two fp32 entries - ``zf_f32_eval`` (f, jac_f) and ``zf_f32_gap_eval`` (the certificate) - of the four
dense margins classes with ``matrix_dtype="float32"``, weighted and factored, against long double on
A64 = float64(float32(A)) within the a-priori rounding bounds of tests/weight_cases.py, tests/penalty_cases.py and
tests/poisson_cases.py AS THEY ARE (the fp32 sweeps widen exactly and sum in fp64, in another order: the bounds hold for any
order); lam_max, gap_tol stopping, l1_cv and the refusals on such problems.  Every test asserts the fp32 ls_plan of its shape.

The per-element bound of the gradient is the line ``g`` of those modules' docstrings, composed from what they return:
dg_j = gfac ((|A|^T drho)_j + gamma_(m+2) (|A|^T |rho|)_j), drho from their loss_longdouble at the margins float64(z) with
ds_i = gamma_n (|A| |x|)_i + u |z_i| (the sweep's error and the one rounding of z to fp64), the safety factor 2 on both terms -
what their gap_longdouble maximises over j for ``grad_inf``.

The matrices of (a) - (e) are dense Gaussian ones (f32_cases.Dense) so that every column meets every row: leaving the last row
out of one column would exceed the gradient's bound by more than 1e3 in the median column, which each gradient test asserts.
(f) compares with the CPU oracle and takes the 300 x 1000 instance of the fuzz tables, on which that comparison is known to be
decision-stable.

ZF_F32_BOUNDS_RECORD=1 (or a directory) appends the worst error / bound per (test, loss, setting) to
profiles/f32_output_bounds.jsonl."""
import functools
import json
import math
import os
import warnings
from collections import namedtuple

import numpy as np
import pytest
import scipy.sparse as sp

import f32_cases as F
import f32_fuzz_cases as XF
import gap_cases as GC
import penalty_cases as PF
import poisson_cases as PC
import weight_cases as W
from conftest import rel_err
from test_gpu_fuzz_margins import default_switches, solve   # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, U = 1e-10, W.U
LOSSES = PF.LOSSES
V4, V2, V1, LOOP = (300, 1000), (64, 4098), (1000, 257), (70003, 33)
# zf_solver_ls_plan of an fp32 view (tests/test_f32_fuzz_cases.py and tests/test_f32_cases.py prove these against dispatch_f32)
PLANS = {V4: XF.PLANS[V4], V2: XF.PLANS[V2], V1: XF.PLANS[V1], LOOP: F.BY_SHAPE[LOOP][3]}
BASE = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=100000, max_backtrack_iter=100, nesterov=True,
            nesterov_ratio=(0, 0.25), deprecated=False, return_all=False, verbose=False)
_id = lambda s: f"{s[0]}x{s[1]}"

Data = namedtuple("Data", "A A64 csr b lam delta")


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _record(**rec):
    where = os.environ.get("ZF_F32_BOUNDS_RECORD", "")
    if where in ("", "0"):
        return
    path = os.path.join(os.path.join(ROOT, "profiles") if where == "1" else where, "f32_output_bounds.jsonl")
    with open(path, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


def _gfac(loss):
    return PF.SCALE[loss] * (2 if loss in ("square", "huber") else 1)


def _psi0(loss, b, delta):
    """psi at z = 0 (NumPy), for lam."""
    z = np.zeros(b.size)
    return PC.poisson_terms(z, b)[0] if loss == "poisson" else W.row_terms(z, b, loss, delta)[0]


@functools.lru_cache(maxsize=None)
def _data(loss, shape):
    """(A as generated, A64, A64 as CSR, b, lam = 0.1 |grad f(0)|_inf, delta) of one loss on one shape - read-only.  The Poisson
    matrix is the Gaussian one times 2^-k (exact in both formats) so that the margins stay in the range of exp, its counts are
    drawn from the model.  At LOOP the columns 0 and 1 are zero but for +2 and -2 in the last row: through them one margin alone
    can be made to overflow, or to be inf - inf."""
    m, n = shape
    D = F.Dense(m, n, seed=11)
    A = D.A.copy()
    if loss == "poisson":
        A *= 2.0 ** -math.ceil(math.log2(math.sqrt(n) / 4))
    if shape == LOOP:
        A[:, :2] = 0.0
        A[-1, 0], A[-1, 1] = 2.0, -2.0
    A64 = A.astype(np.float32).astype(np.float64)
    if loss == "poisson":
        rng = np.random.default_rng(n + 17)
        xt = np.where(rng.random(n) < 0.05, rng.standard_normal(n), 0.0)
        xt[:2] = 0.0
        b = rng.poisson(np.exp(A64 @ xt)).astype(np.float64)
    else:
        b = np.where(D.b >= 0, 1.0, -1.0) if loss == "logistic" else D.b.copy()
    delta = 0.5 * float(np.std(b)) if loss == "huber" else 0.0
    lam = 0.1 * float(np.max(np.abs(_gfac(loss) * (A64.T @ _psi0(loss, b, delta)))))
    for a in (A, A64, b):
        a.setflags(write=False)
    return Data(A, A64, sp.csr_matrix(A64), b, lam, delta)


@functools.lru_cache(maxsize=None)
def _weights(shape, kind):
    """``real``: weight_cases.make_weights (about 20 % zeros); ``fold``: the training mask of one of five folds.  The first row is
    off and the last row is on in both (the last row is the one the gradient guard leaves out)."""
    m, n = shape
    if kind == "real":
        w = W.make_weights(m, n, "real")
        w[0], w[-1] = 0.0, 1.25
    else:
        ids = W.fold_ids(m, 5)
        w = (ids != ids[0]).astype(np.float64)
        assert w[0] == 0.0
        w[-1] = 1.0
    assert (w == 0).any() and (w > 0).sum() > m // 2
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _factors(shape):
    p = PF.make_factors(shape[1], shape[0], "positive")
    p.setflags(write=False)
    return p


def _make(loss, d, lam=None, w=None, p=None, l2=0.0, first=False, dtype="float32"):
    """The fp32 problem, from the matrix AS GENERATED.  The logistic class through with_matrix_dtype, before (``first``) or
    after its other siblings; the other three through their keywords.  ``dtype="float64"``: the fp64 class, likewise."""
    from zfista_amd import problems as Z

    lam, scale = d.lam if lam is None else lam, PF.SCALE[loss]
    if loss == "logistic":
        prob = Z.LogisticL1(d.A, d.b, lam, scale=scale)
        if first:
            prob = prob.with_matrix_dtype(dtype)
        if l2 > 0:
            prob = prob.with_penalty(lam, l2)
        if w is not None:
            prob = prob.with_sample_weight(w)
        if p is not None:
            prob = prob.with_penalty_factor(p)
        return prob if first else prob.with_matrix_dtype(dtype)
    cls = {"square": Z.LeastSquaresL1, "huber": Z.HuberL1, "poisson": Z.PoissonL1}[loss]
    lead = (d.A, d.b, lam, d.delta) if loss == "huber" else (d.A, d.b, lam)
    return cls(*lead, scale=scale, l2=l2, sample_weight=w, penalty_factor=p, matrix_dtype=dtype)


def _is_f32(prob, shape):
    """The problem stores a float32 tensor and a solver made from it takes the fp32 plan of its shape."""
    import torch

    from zfista_amd.proximal_gradient import NativeRun

    assert prob.matrix_dtype == "float32" and prob.A.dtype == torch.float32 and tuple(prob.A.shape) == shape
    run = NativeRun(prob, np.zeros(shape[1]), dict(BASE))
    plan = tuple(run.solver.ls_plan())
    run.solver.close()
    assert plan == PLANS[shape], (plan, PLANS[shape])


# ---- the long-double side ----------------------------------------------------------------------------------------------------------
def _eval_reference(loss, d, x, w):
    """(f, bound of f, gradient, bound of every gradient element) in long double on A64 (module docstring)."""
    ld = np.longdouble
    A = d.csr
    m, n = A.shape
    rows = np.repeat(np.arange(m), np.diff(A.indptr))
    data = A.data.astype(ld)
    z = np.zeros(m, dtype=ld)
    np.add.at(z, rows, data * np.asarray(x, np.float64).astype(ld)[A.indices])
    z64 = z.astype(np.float64)
    absA = abs(A)
    ds = GC._gamma(n) * (absA @ np.abs(x)) + U * np.abs(z64)
    scale = PF.SCALE[loss]
    if loss == "poisson":
        f, f_bound, rho, rho_bound = PC.loss_longdouble(z64, d.b, scale, w=w, ds=ds)
    else:
        f, f_bound, rho, rho_bound = W.loss_longdouble(z64, d.b, np.ones(m) if w is None else w, loss, d.delta, scale, ds=ds)
    g = np.zeros(n, dtype=ld)
    np.add.at(g, A.indices, data * rho[rows])
    g *= ld(_gfac(loss))
    arho = np.asarray(np.abs(rho), dtype=np.float64)
    g_bound = _gfac(loss) * (absA.T @ np.asarray(rho_bound, np.float64) + 2 * GC._gamma(m + 2) * (absA.T @ arho))
    if loss in ("logistic", "poisson"):
        g_bound = g_bound + 2 * m * 2.0 ** -1022
    return f, f_bound, g, g_bound, rho


def _check_eval(test, loss, shape, kind, x):
    d = _data(loss, shape)
    w = None if kind is None else _weights(shape, kind)
    prob = _make(loss, d, w=w, first=kind == "fold")
    _is_f32(prob, shape)
    f, f_bound, g, g_bound, rho = _eval_reference(loss, d, x, w)
    # the bound means something: leaving the last row out of one column would exceed it by orders of magnitude in the median column
    drop = _gfac(loss) * np.abs(d.A64[-1] * float(rho[-1]))
    assert np.median(drop / g_bound) > 1e3, float(np.median(drop / g_bound))
    fv = prob.f(x)
    f_ratio = abs(float(np.longdouble(fv) - f)) / f_bound
    gv = prob.jac_f(x)
    err = np.abs(gv.astype(np.longdouble) - g).astype(np.float64)
    g_ratio = float(np.max(err / g_bound))
    print(f"{test} {loss} {_id(shape)} w={kind}: f error / bound {f_ratio:.3g}, gradient elements up to {g_ratio:.3g} of theirs")
    _record(test=test, loss=loss, setting=f"w={kind}", shape=_id(shape), f=f_ratio, gradient=g_ratio)
    assert np.isfinite(fv) and f_ratio <= 1.0, (float(fv), float(f), f_bound)
    bad = np.flatnonzero(~(err <= g_bound))
    assert bad.size == 0, f"{bad.size} of {shape[1]} gradient elements outside their bound, first {bad[:8]}: up to {g_ratio:.3g}"
    if w is not None:   # a row with w = 0 is a row that is not there, whatever its b holds
        import torch

        prob.b[torch.from_numpy(np.flatnonzero(w == 0)).to(prob.b.device)] = float("nan")
        assert prob.f(x) == fv and np.array_equal(prob.jac_f(x), gv), "NaN in b on rows with w = 0"
    return prob


def _point(loss, n):
    """A dense x at which the margins have a standard deviation of about 1 (the Poisson matrix is scaled by about 4 / sqrt(n)):
    no row's loss saturates, so the last row's part of the gradient is of the size of the others'."""
    return np.random.default_rng(n + 5).standard_normal(n) * (0.25 if loss == "poisson" else 1 / math.sqrt(n))


# ---- (a) f and jac_f ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [None, "real", "fold"], ids=["plain", "wreal", "wfold"])
@pytest.mark.parametrize("shape", [V4, V2, V1], ids=_id)
@pytest.mark.parametrize("loss", LOSSES)
def test_f_and_jac_f_within_their_bounds(loss, shape, kind):
    """zf_f32_eval with and without w_dev: f inside its bound, every gradient element inside its own."""
    _check_eval("eval", loss, shape, kind, _point(loss, shape[1]))


# ---- (b) the row sweep loops, the loss kernels in their many-workgroup shape ----------------------------------------------------------
@pytest.mark.parametrize("loss", ["logistic", "poisson"])
def test_weighted_f_and_jac_f_where_the_row_sweep_loops(loss):
    """70003 x 33, weighted: the fp32 row sweep loops and its last group holds 3 of 4 rows; the loss kernels run many workgroups
    with a short last chunk.  Poisson: a margin of the last row beyond the range of exp gives f = +inf (not NaN), a NaN margin
    there NaN."""
    m, n = LOOP
    assert m > F.ROW_LOOP_MIN_M and m % 4 == 3 and m > 2 * 32768
    x = _point(loss, n)
    x[:2] = 0.1
    prob = _check_eval("eval-loop", loss, LOOP, "real", x)
    if loss != "poisson":
        return
    d = _data(loss, LOOP)
    assert _weights(LOOP, "real")[-1] > 0 and np.count_nonzero(d.A64[:-1, :2]) == 0
    assert np.isfinite(prob.f(x))
    big = x.copy()
    big[0] = 400.0    # z_last = 800 + ...: exp overflows, inf - b z is inf
    assert prob.f(big) == np.inf
    bad = x.copy()
    bad[:2] = 1e308   # 2e308 - 2e308 = inf - inf in the last row alone; 0 * 1e308 = 0 in every other
    assert np.isnan(prob.f(bad))


# ---- (c) the certificate -------------------------------------------------------------------------------------------------------------
#            setting             shape  weights  l2 / lam  factors
SETTINGS = {"plain":            (V2,    None,    0.0,      False),
            "weighted":         (V1,    "real",  0.0,      False),
            "weighted-l2":      (V4,    "real",  1.0,      False),
            "factors":          (V1,    None,    0.0,      True),
            "factors-weighted": (V2,    "fold",  0.0,      True)}


def _setting(loss, name):
    shape, kind, fac, factored = SETTINGS[name]
    d = _data(loss, shape)
    w = None if kind is None else _weights(shape, kind)
    p = _factors(shape) if factored else None
    return shape, d, w, p, fac * d.lam


def _gap_reference(loss, d, w, p, l2, x, lam=None):
    """(values, bounds, P(x)) from the cases module of the setting, unchanged, on A64."""
    lam = d.lam if lam is None else lam
    scale = PF.SCALE[loss]
    if p is not None:
        vals, bounds, _ = PF.gap_longdouble(d.csr, d.b, p, x, lam, loss, d.delta, scale, w=w)
        return vals, bounds, PF.primal_longdouble(d.csr, d.b, p, x, lam, loss, d.delta, scale, w=w)
    if loss == "poisson":
        vals, bounds, _ = PC.gap_longdouble(d.csr, d.b, x, lam, scale=scale, l2=l2, w=w)
    else:
        vals, bounds, _ = W.gap_longdouble(d.csr, d.b, np.ones(d.b.size) if w is None else w, x, lam, loss, d.delta, scale, l2)
    return vals, bounds, vals["primal"]


def _gap_bits(gp):
    return np.array([getattr(gp, k) for k in gp.__slots__]).view(np.uint64)


@pytest.mark.parametrize("name", list(SETTINGS))
@pytest.mark.parametrize("loss", LOSSES)
def test_every_output_of_the_certificate_within_its_bound(loss, name, solve):
    """duality_gap(x) (zf_f32_gap_eval, with and without p_dev) at x = 0 and at the iterates 20 and 300 of a FISTA solve: every
    output inside the bounds of its cases module; gap >= 0 and gap >= P(x) - P(x^), x^ the solve carried on to tol = 1e-12."""
    shape, d, w, p, l2 = _setting(loss, name)
    n = shape[1]
    prob = _make(loss, d, w=w, p=p, l2=l2, first=name == "factors")
    res, _, plan = solve(prob, np.zeros(n), lr=1, tol=0.0, max_iter=300, nesterov=True, return_all=True)
    assert tuple(plan) == PLANS[shape] and prob.matrix_dtype == "float32"
    assert res.nit == 300
    hat, _, _ = solve(prob, np.asarray(res.allvecs[300]), lr=1, tol=1e-12, max_iter=3000, nesterov=True)
    P_hat = _gap_reference(loss, d, w, p, l2, np.asarray(hat.x))[2]
    keys = W.KEYS10 if l2 > 0 else W.KEYS8
    gaps = []
    for k in (0, 20, 300):
        x = np.asarray(res.allvecs[k])
        vals, bounds, Px = _gap_reference(loss, d, w, p, l2, x)
        assert set(vals) == set(keys)
        got = prob.duality_gap(x)
        ratios = W.worst_ratio(got, vals, bounds)
        worst = max(ratios, key=ratios.get)
        print(f"{loss} {name} {_id(shape)}, x_{k}: worst error / bound {ratios[worst]:.3g} ({worst}); gap {float(got.gap):.6g} "
              f"alpha {float(got.alpha):.6g}")
        _record(test="gap", loss=loss, setting=name, shape=_id(shape), iterate=k, worst=ratios[worst], output=worst)
        assert all(np.isfinite(getattr(got, key)) for key in keys), got
        assert ratios[worst] <= 1.0, (k, worst, ratios, got)
        assert got.gap >= 0 and got.rows_gap >= 0 and got.ridge_gap >= 0
        assert np.longdouble(got.gap) + bounds["gap"] + bounds["primal"] >= Px - P_hat, "P(x) - min P <= gap"
        if l2 == 0:
            assert got.g_l2 == 0.0 and got.ridge_gap == 0.0
        gaps.append(float(got.gap))
    assert gaps[2] < gaps[0]
    x = np.asarray(res.allvecs[300])
    assert np.array_equal(_gap_bits(prob.duality_gap(x)), _gap_bits(prob.duality_gap(x))), "two evaluations: the same bits"


def _walk(prob, passes, gap_after=(), **opts):
    """`passes` chunks of ONE pass each; a gap call after the chunks listed in gap_after."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    run = NativeRun(prob, np.zeros(prob.n_features), dict(BASE, **opts))
    rows, gaps = [np.zeros((0, _lib.ZF_TRACE_COLS))], {}
    for k in range(passes):
        rows.append(run.advance(1))
        if k in gap_after:
            gaps[k] = run.duality_gap()
    ctl, _ = run.solver.poll()
    out = dict(rows=np.concatenate(rows), x=run.solver.get_x(), nit=int(ctl.nit), lr=ctl.lr, F=ctl.F_old, trials=int(ctl.total_trials),
               gaps=gaps, plan=tuple(run.solver.ls_plan()))
    run.solver.close()
    return out


@pytest.mark.parametrize("name", ["weighted-l2", "factors", "factors-weighted"])
@pytest.mark.parametrize("loss", LOSSES)
def test_the_gap_of_a_live_solve(loss, name):
    """NativeRun.duality_gap() on an fp32 view, with weights and with factors, equals the standalone evaluation at get_x() bit for
    bit and lies inside the bounds; a solve probed after every pass is the solve that was never asked, bit for bit."""
    shape, d, w, p, l2 = _setting(loss, name)
    prob = _make(loss, d, w=w, p=p, l2=l2)
    passes = 24
    plain = _walk(prob, passes)
    assert plain["plan"] == PLANS[shape]
    assert plain["trials"] > plain["nit"] > 0, "the case must backtrack and accept"
    probed = _walk(prob, passes, gap_after=range(passes))
    assert (plain["nit"], plain["lr"], plain["F"], plain["trials"]) == (probed["nit"], probed["lr"], probed["F"], probed["trials"])
    assert np.array_equal(plain["rows"], probed["rows"]) and np.array_equal(plain["x"], probed["x"])
    live, alone = probed["gaps"][passes - 1], prob.duality_gap(probed["x"])
    assert np.array_equal(_gap_bits(live), _gap_bits(alone)), (live, alone)
    vals, bounds, _ = _gap_reference(loss, d, w, p, l2, probed["x"])
    ratios = W.worst_ratio(live, vals, bounds)
    assert max(ratios.values()) <= 1.0, ratios
    assert live.gap < probed["gaps"][0].gap and (live.g_l2 > 0) == (l2 > 0)


WIDE = (512, 16900)   # the one shape here at which the fp64 slice rule (57 slices of 9 rows) and the fp32 rule (64 of 8) differ


@pytest.mark.parametrize("loss,weighted,factored", [("square", False, False), ("huber", True, True)], ids=["square-plain", "huber-w-p"])
def test_the_standalone_certificate_slices_the_rows_as_the_solver_does(loss, weighted, factored, solve):
    """zf_f32_gap_eval sizes its own slab and slices (zf_sweep_ws_alloc); the live solver has those of zf_solver_set_matrix_f32.
    Both must follow the fp32 rule: then the column sums are added in the same order and the two certificates agree to the bit.
    On the other shapes of this file the caps (64 slices, 8 rows per slice) make the fp64 rule give the same split; here n is
    large enough for the two rules to part (V = 4 halves the column panels of the fp64 sweep's V = 2)."""
    from zfista_amd import problems as Z

    m, n = WIDE
    assert F.dispatch_f32(m, n) == (F.COLS_V4, F.ROWS_V4, 64, 8)
    panels64 = -(-(n // 2) // 256)   # zf_col_slices with V = 2, restated: the fp64 rule on this shape
    rps64 = -(-m // min(-(-2048 // panels64), -(-m // 8), 64))
    assert (-(-m // rps64), rps64) == (57, 9)
    D = F.Dense(m, n, seed=11)
    rng = np.random.default_rng(3)
    w = np.where(rng.random(m) < 0.2, 0.0, 0.25 + 2.0 * rng.random(m)) if weighted else None
    p = 0.25 + 3.75 * rng.random(n) if factored else None
    lam = 0.02 * D.lam   # 0.002 lam_max: nearly every x_j is non-zero after one step, so every column sum enters the certificate
    lead = (D.A, D.b, lam, 0.5 * float(np.std(D.b))) if loss == "huber" else (D.A, D.b, lam)
    cls = Z.HuberL1 if loss == "huber" else Z.LeastSquaresL1
    prob = cls(*lead, sample_weight=w, penalty_factor=p, matrix_dtype="float32")
    # lr below 1 / L for the largest weight (2.25): the first trial of every pass is accepted, so twelve passes are twelve
    # iterations however many trials a pass may hold (from lr = 1 the first line search alone takes about 15)
    out = _walk(prob, 12, gap_after=[11], lr=0.3 / D.L(0.5))
    assert out["plan"] == F.dispatch_f32(m, n) and out["nit"] > 0
    live, alone = out["gaps"][11], prob.duality_gap(out["x"])
    assert np.array_equal(_gap_bits(live), _gap_bits(alone)), (live, alone)
    assert live.gap > 0 and live.alpha < 1 and np.count_nonzero(out["x"]) > n // 2
    # The certificate shows only the largest column sum and sums of all of them, which absorb a last-bit change of a few.  Every
    # column: one ISTA step with lam = 0 and lr = 2^-k is x1 = fl(x0 - lr g) with the solver's g (lr g is exact), and jac_f is
    # the standalone entry's g - the same bits in every element only if both add the slices in the same order.
    from zfista_amd import _lib

    x0 = rng.standard_normal(n)
    lr = 2.0 ** -math.ceil(math.log2(2 * 2.25 * D.L(0.5)))
    plain = prob.with_lam(0.0)
    res, rows, plan = solve(plain, x0, lr=lr, tol=0.0, max_iter=1, nesterov=False, return_all=True)
    assert tuple(plan) == F.dispatch_f32(m, n) and res.nit == 1 and rows[0, _lib.TR_TRIALS] == 1 and rows[0, _lib.TR_LR] == lr
    x1 = np.asarray(res.allvecs[1])
    assert np.array_equal(x1, x0 - lr * plain.jac_f(x0)), int(np.count_nonzero(x1 != x0 - lr * plain.jac_f(x0)))


# ---- (d) lam_max -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["weighted", "factors-weighted", "factors"])
@pytest.mark.parametrize("loss", LOSSES)
def test_lam_max(loss, name, solve):
    """lam_max of a weighted / factored fp32 problem against long double on A64 (1e-12 relative, the bound of the fp64 tests); the
    solve stays at 0 at lam_max (1 + 1e-9) and leaves it slightly below."""
    shape, d, w, p, _ = _setting(loss, name)
    n = shape[1]
    prob = _make(loss, d, w=w, p=p)
    lmax = float(prob.lam_max())
    A1 = d.csr if p is None else PF.scaled(d.csr, p)[0]
    if loss == "poisson":
        exact = PC.lam_max(A1, d.b, PF.SCALE[loss], w=w)
    else:
        exact = W.lam_max(A1, d.b, np.ones(shape[0]) if w is None else w, loss, d.delta, PF.SCALE[loss])
    assert abs(lmax - exact) <= 1e-12 * exact, (lmax, exact)
    top = prob.with_lam(lmax * (1 + 1e-9))
    assert top.A is prob.A and top.matrix_dtype == "float32"
    res, _, plan = solve(top, np.zeros(n), lr=1, tol=0.0, max_iter=30, nesterov=True)
    assert tuple(plan) == PLANS[shape]
    assert not res.x.any(), "at lam_max the solution is 0"
    gp = top.duality_gap(np.zeros(n))
    assert gp.alpha == 1.0 and gp.gap == 0.0, "x = 0 is certified optimal at lam_max"
    low = prob.with_lam(0.99 * lmax)
    gl = low.duality_gap(np.zeros(n))
    assert gl.alpha < 1.0 and gl.gap > 0.0
    below, _, _ = solve(low, np.zeros(n), lr=1, tol=0.0, max_iter=200, nesterov=True)
    P_below = _gap_reference(loss, d, w, p, 0.0, np.asarray(below.x), lam=0.99 * lmax)[2]
    assert below.x.any() and P_below < _gap_reference(loss, d, w, p, 0.0, np.zeros(n), lam=0.99 * lmax)[2], "0 is not optimal below lam_max"


# ---- (e) gap_tol ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
def test_gap_tol_stops_where_the_hand_probed_solve_says(loss):
    """A weighted fp32 solve with gap_tol stops at the check, and the nit, at which the same solve without the keyword - advanced
    by hand, gap_every passes at a time, and probed with the standalone certificate - first finds gap <= gap_tol."""
    from zfista_amd import _lib, minimize_proximal_gradient
    from zfista_amd.proximal_gradient import NativeRun

    shape, d, w, p, _ = _setting(loss, "weighted")
    n, every = shape[1], 5
    prob = _make(loss, d, w=w)
    P0 = float(_gap_reference(loss, d, w, None, 0.0, np.zeros(n))[2])
    gap_tol = 1e-4 * P0
    kw = {k: v for k, v in BASE.items() if k not in ("return_all", "verbose")}
    kw["max_iter"] = 4000
    res = _quiet(minimize_proximal_gradient, *prob.callbacks(), np.zeros(n), gap_tol=gap_tol, gap_every=every, **kw)
    assert res.success and res.status == 1 and res.message == "Duality gap reached gap_tol" and res.nit < 4000
    assert 0 <= res.dual_gap <= gap_tol and res.dual_gap == prob.duality_gap(res.x).gap
    run = NativeRun(prob, np.zeros(n), dict(BASE, max_iter=4000))
    assert tuple(run.solver.ls_plan()) == PLANS[shape]
    checks = 0
    while run.status == _lib.ZF_RUNNING:
        run.advance(every)
        checks += 1
        gp = prob.duality_gap(run.solver.get_x())
        if gp.gap <= gap_tol:
            break
        assert checks < res.dual_gap_checks, "the keyword's solve went past a check at which the gap was already small enough"
    nit, x = int(run.solver.ctl.nit), run.solver.get_x()
    run.solver.close()
    print(f"{loss}: stopped at check {res.dual_gap_checks}, nit {res.nit}, gap {float(res.dual_gap):.3g} <= {gap_tol:.3g}")
    assert (checks, nit) == (res.dual_gap_checks, res.nit)
    assert np.array_equal(x, res.x) and gp.gap == res.dual_gap, "the keyword does not alter the iterates"


# ---- (f) l1_cv ---------------------------------------------------------------------------------------------------------------------------
CV_SHAPE = XF.SHAPES[0]   # 300 x 1000 of the fuzz tables


def _cv_ref(loss, A64, b, lam, w, delta):
    if loss == "poisson":
        return PC.PoissonRef(A64, b, lam, PF.SCALE[loss], sample_weight=w)
    return W.WeightedRef(A64, b, lam, w, loss, delta, PF.SCALE[loss])


@pytest.mark.parametrize("loss", LOSSES)
def test_l1_cv_against_the_oracles_warm_started_chains(loss):
    """l1_cv on an fp32 problem: every fold's path against the oracle's warm-started chain on A64 with the fold's 0 / 1 mask as
    weights; every fold's problem shares the one float32 tensor."""
    import torch

    from oracle import cpu_ref
    from zfista_amd.path import l1_cv

    csr, b, lam, delta = XF.data(loss, CV_SHAPE)
    A64 = XF.dense(loss, CV_SHAPE)
    m, n = A64.shape
    d = Data(XF.generated(loss, CV_SHAPE), A64, csr, b, lam, delta)
    ids = np.random.default_rng(17).integers(0, 3, m)
    w_base = XF.X.weights(CV_SHAPE, "real", 0) if loss == "huber" else None   # one loss carries weights of its own
    wb = np.ones(m) if w_base is None else w_base
    prob = _make(loss, d, w=w_base, first=loss == "logistic")
    _is_f32(prob, (m, n))
    lams = [2.0 * lam, lam, 0.5 * lam]
    kw = dict(lr=1, tol=0.0, max_iter=40, nesterov=True)
    cv = _quiet(l1_cv, prob, lams, folds=ids, gap_tol=None, return_paths=True, **kw)
    assert np.array_equal(cv.fold_ids, ids) and cv.folds == [0, 1, 2] and cv.scores.shape == cv.nnz.shape == (3, 3)
    assert len(cv.paths) == 3 and len(cv.path) == 3 and len(cv.problems) == 4
    worst = 0.0
    for k in range(3):
        w_train, w_test = wb * (ids != k), wb * (ids == k)
        x = np.zeros(n)
        for l, lam_l in enumerate(lams):   # the oracle's chain: each point from the one before
            exp = _quiet(cpu_ref.minimize_proximal_gradient, *_cv_ref(loss, A64, b, lam_l, w_train, delta).callbacks(), x, **kw)
            got = cv.paths[k][l]
            assert got.nit == exp.nit == 40 and got["lam"] == lam_l
            worst = max(worst, rel_err(got.x, exp.x))
            assert rel_err(got.x, exp.x) <= TOL, (k, l, rel_err(got.x, exp.x))
            x = exp.x
            held_ref = _cv_ref(loss, A64, b, lam_l, w_test, delta)
            held = held_ref.f(got.x) / w_test.sum()
            size = PF.SCALE[loss] * float(np.sum(np.abs(held_ref._rows(got.x)[1]) if loss == "poisson" else held * w_test.sum() / PF.SCALE[loss]))
            assert abs(cv.scores[k, l] - held) <= 1e-12 * size / w_test.sum(), (k, l)
            assert cv.nnz[k, l] == np.count_nonzero(got.x)
    print(f"{loss}: fold paths within {worst:.3g} of the oracle's chains")
    # one resident fp32 matrix: the K training siblings and the problem of the refit
    assert len({p.A.data_ptr() for p in cv.problems}) == 1 and cv.problems[0].A.data_ptr() == prob.A.data_ptr()
    assert all(p.A.dtype == torch.float32 and p.matrix_dtype == "float32" for p in cv.problems)
    assert len({p.b.data_ptr() for p in cv.problems}) == 1
    for k, p in enumerate(cv.problems[:3]):
        assert np.array_equal(p.sample_weight, wb * (ids != k))
    chain = np.zeros(n)
    for lam_l in lams:
        chain = _quiet(cpu_ref.minimize_proximal_gradient, *_cv_ref(loss, A64, b, lam_l, wb, delta).callbacks(), chain, **kw).x
    assert rel_err(cv.path[-1].x, chain) <= TOL


@pytest.mark.parametrize("loss", LOSSES)
def test_two_folds_on_streams_equal_the_solves_alone(loss):
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.replicas import solve_on_streams

    shape = V2
    d = _data(loss, shape)
    m, n = shape
    prob = _make(loss, d)
    ids = W.fold_ids(m, 2, 0)
    folds = [prob.with_sample_weight((ids != k).astype(float)) for k in range(2)]
    assert folds[0].A is prob.A and folds[1].A is prob.A and folds[0].matrix_dtype == "float32"
    _is_f32(folds[1], shape)
    kw = dict(lr=1, tol=0.0, max_iter=60, nesterov=True)
    alone = [_quiet(minimize_proximal_gradient, *p.callbacks(), np.zeros(n), **kw) for p in folds]
    both = solve_on_streams([(p, np.zeros(n), kw) for p in folds], streams=2)
    for a, c in zip(alone, both):
        assert a.nit == c.nit == 60 and np.array_equal(a.x, c.x) and a.fun == c.fun
    assert not np.array_equal(alone[0].x, alone[1].x)


# ---- (g) refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from zfista_amd import problems as Z

    d = _data("square", V1)
    n = V1[1]
    grouped = Z.LeastSquaresL1(d.A, d.b, d.lam, group=object())
    assert grouped.matrix_dtype == "float64"
    with pytest.raises(ValueError, match="group="):
        grouped.with_matrix_dtype("float32")
    p = _factors(V1)
    zero = p.copy()
    zero[3] = 0.0

    def said(call):
        with pytest.raises(ValueError) as info:
            call()
        return str(info.value)

    for loss in LOSSES:
        d = _data(loss, V1)
        for first in (False, True):
            calls = {
                "penalty_factor": lambda dt: _make(loss, d, p=p, l2=0.5 * d.lam, first=first, dtype=dt),
                "penalty_factor ": lambda dt: _make(loss, d, p=p, first=first, dtype=dt).with_penalty(d.lam, 0.1),
                "penalty_factor  ": lambda dt: _make(loss, d, l2=0.1, first=first, dtype=dt).with_penalty_factor(p),
                "duality_gap is not available": lambda dt: _make(loss, d, p=zero, first=first, dtype=dt).duality_gap(np.zeros(n)),
            }
            for what, call in calls.items():   # an fp32 problem refuses what its fp64 class refuses, in the same words
                msg32, msg64 = said(lambda: call("float32")), said(lambda: call("float64"))
                assert what.strip() in msg32 and msg32 == msg64, (loss, what, msg32, msg64)
