"""GPU: every instantiation of the two correlation kernels of the operator-form LASSO (csrc/zf_kernels_op.h:
zf_op_apply_kernel, zf_op_adjoint_kernel over K in {3 .. 15} x tile height {32, 8} x separable / general = 28
combinations) - element by element against the exact reference of tests/operator_exact.py at derived rounding bounds
(operator level: prob.f / prob.jac_f, the unfused kernels), and as the fused trial of a solve (residual in the adjoint
tile load, prox step in its epilogue, decide pass in the apply kernel) against the three-launch trial and the oracle.

Operator-level taps are random with no symmetry (general: K x K normal; separable: u v^T with independent u, v), so a
transposed, mirrored or convolved window is O(1) wrong.  A solve needs jac_f to be the gradient of f - B applied as its
own adjoint has to BE self-adjoint - so the solver level mirrors its random taps in each axis (make_self_adjoint_taps:
still u != v, still no symmetry under a transposition); with taps of no symmetry the line search backtracks to a step of
1e-15 in the oracle too.  Every case asserts through ls_plan() the tile height and the path it is
about.  The sharp check is the operator level's: |jac_f - exact| <= bound for every coefficient, the bound a few
hundred u of the local magnitude (tests/test_operator_exact.py shows fp64 SciPy at 0.0005 ... 0.04 of it, and one
tap off by 1e-11 outside it).  The solver level compares at the project's 1e-10: iterations amplify rounding, the
element-wise bound does not carry over.

ZF_OP_BOUNDS_RECORD=1 appends the worst error-to-bound ratio of every operator-level case to
profiles/op_kernel_bounds.jsonl (any other value: to that path) - records for the next change of these kernels to
compare with, not thresholds."""
import json
import os
import warnings

import numpy as np
import pytest

import operator_exact as E
from conftest import ROOT, rel_err
from test_gpu_operator_lasso import _solve_recording_plan

pytestmark = pytest.mark.gpu
TOL = 1e-10
LAM = 0.5      # solves: a threshold of lam lr = 0.25 on coefficients of unit variance - a fifth of them end at zero
KS = (3, 5, 7, 9, 11, 13, 15)
# 566 x 950: 15 x 18 = 270 tiles of 64 x 32 (>= 256: tall tiles), 54 columns / 22 rows in the last ones, 270 % 8 = 6
# (zf_op_tile's remainder bands); 100 x 200: 4 x 13 = 52 tiles of 64 x 8 (>= 16: the remap runs, 52 % 8 = 4)
SHAPES = {32: (566, 950), 8: (100, 200)}
MATRIX = [pytest.param(k, ty, kind, id=f"k{k}-ty{ty}-{kind}") for k in KS for ty in (32, 8) for kind in ("separable", "general")]


def _problem(taps, observed, lam=LAM, scale=1.0, bounds=None):
    from zfista_amd.problems import BlurHaarL1

    return BlurHaarL1(taps, observed, lam, scale=scale, bounds=bounds)


def _plan(monkeypatch, prob):
    """ls_plan() of a solver made for `prob` under the current environment: (tile height, separable, walk, fused prox)."""
    x0 = np.zeros(prob.n_features)
    return _solve_recording_plan(monkeypatch, prob, x0, dict(lr=0.5 / prob.scale, tol=0.0, max_iter=1))[1]


def _record(label, plan, k, shape, ratio, f_rel):
    where = os.environ.get("ZF_OP_BOUNDS_RECORD", "")
    if where in ("", "0"):
        return
    path = os.path.join(ROOT, "profiles", "op_kernel_bounds.jsonl") if where == "1" else where
    with open(path, "a") as fh:
        fh.write(json.dumps(dict(case=label, K=k, tile_height=int(plan[0]), separable=int(plan[1]), walk=int(plan[2]),
                                 shape=list(shape), jac_err_over_bound=ratio, f_rel_err=f_rel)) + "\n")


def _check_operator(prob, taps, observed, plan, rng, label, scale=1.0, xs=None):
    """prob.jac_f element-wise inside the derived bound and prob.f at F_RTOL, each at a FRESH random x (zf_op_eval
    allocates and frees its output per call: a buffer left over from the call before must not be able to pass).
    Returns (jac_f, f) as computed, for bit-for-bit comparisons."""
    shape = observed.shape
    ex = E.Exact(taps, observed, scale)
    x, x2 = xs if xs is not None else (rng.standard_normal(prob.n_features), rng.standard_normal(prob.n_features))
    got = prob.jac_f(x)
    assert got.shape == (1, x.size)
    g, bound = ex.grad_and_bound(x, separable=bool(plan[1]))
    ratio, at = E.worst(got, g, bound)
    f_got, f_ref = prob.f(x2), ex.f(x2)
    assert f_got.shape == (1,)
    f_rel = float(abs(f_got[0] - f_ref) / f_ref)
    print(f"{label}: plan {tuple(plan)}  worst |jac_f - exact| / bound = {ratio:.3g} at {E.locate(at, shape, int(plan[0]))}  f rel {f_rel:.2g}")
    _record(label, plan, ex.k, shape, ratio, f_rel)
    assert ratio <= 1.0, (f"{label}: jac_f off by {ratio:.3g} x the bound at {E.locate(at, shape, int(plan[0]))}: "
                          f"got {got.reshape(-1)[at]!r}, exact {float(g[at])!r}, bound {bound[at]:.3g}")
    assert f_rel <= E.F_RTOL, (label, f_got[0], float(f_ref))
    return got, f_got


# ---- operator level -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,ty,kind", MATRIX)
def test_every_instantiation_element_by_element(k, ty, kind, monkeypatch):
    rng = np.random.default_rng(1000 * k + ty + (kind == "general"))
    shape = SHAPES[ty]
    taps, observed = E.make_taps(rng, k, kind), rng.standard_normal(shape)
    prob = _problem(taps, observed)
    plan = _plan(monkeypatch, prob)
    assert plan[0] == ty and plan[1] == (kind == "separable"), plan      # the instantiation this case is about ran
    _check_operator(prob, taps, observed, plan, rng, f"matrix k{k} ty{ty} {kind}")


def _zero_pattern(rng):
    return np.array([[0.0, 0.3, 0.0], [-0.2, 0.0, 0.0], [0.0, 0.1, 0.4]])


EDGE_CASES = {   # name: (K, kind or a taps maker, shape, expected tile height, scale)
    "scale_0.37": (11, "general", (100, 200), 8, 0.37),
    "k1": (1, lambda rng: np.array([[0.7]]), (64, 192), 8, 1.0),
    "k3_zero_pattern": (3, _zero_pattern, (100, 200), 8, 1.0),
    "image_2x2": (3, "general", (2, 2), 8, 1.0),
    "image_8x8_k15": (15, "separable", (8, 8), 8, 1.0),            # halo = image - 1: every row and column mirrored
    "image_16x130": (5, "general", (16, 130), 8, 1.0),             # the third tile column is two pixels wide
    "image_130x16": (7, "separable", (130, 16), 8, 1.0),
    "wide_2x16400": (3, "separable", (2, 16400), 32, 1.0),         # 257 tiles: 32-row tiles on a 2-row image
    "tall_16400x2": (3, "general", (16400, 2), 32, 1.0),           # 513 tiles of 64 x 32, two pixels wide
    "narrow_1000x2": (3, "separable", (1000, 2), 8, 1.0),          # 125 tiles of 64 x 8 on 2000 coefficients
    # 15 x 17 = 255 tall tiles: the most an image of 64 x 8 tiles has - 1020 of them.  By the compiler's register count
    # (134 VGPRs: 3 waves per SIMD) the device holds 768 workgroups of the separable 9 x 9 apply kernel, the one
    # instantiation on 64 x 8 tiles below 1024: if the runtime reports the same, its workgroups walk here (nothing forces it)
    "ty8_1020_tiles": (9, "separable", (544, 960), 8, 1.0),
}


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_edge_shapes_and_taps(name, monkeypatch):
    k, kind, shape, ty, scale = EDGE_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    taps = kind(rng) if callable(kind) else E.make_taps(rng, k, kind)
    observed = rng.standard_normal(shape)
    prob = _problem(taps, observed, scale=scale)
    plan = _plan(monkeypatch, prob)
    sep = {"k1": 1, "k3_zero_pattern": 0}.get(name, int(kind == "separable"))   # (one tap IS rank 1)
    assert plan[0] == ty and plan[1] == sep, plan
    _check_operator(prob, taps, observed, plan, rng, name, scale)


@pytest.mark.parametrize("eps,separable", [(1e-13, 0), (1e-15, 1)])
def test_near_rank_one_taps(eps, separable, monkeypatch):
    """u v^T plus eps max|tap| on one entry off the pivot's row and column: 1e-13 is beyond what zf_op_factor_rank1
    accepts (1e-14) - the general kernels; 1e-15 is inside - the separable kernels, whose factors then differ from the taps
    by that much: inside the bound by its slack term."""
    rng = np.random.default_rng(77)
    k, shape = 7, (100, 200)
    taps = E.make_taps(rng, k, "separable")
    pi, pj = np.unravel_index(np.argmax(np.abs(taps)), taps.shape)
    i, j = (pi + 1) % k, (pj + 1) % k
    before = taps[i, j]
    taps[i, j] += eps * np.abs(taps).max()
    assert taps[i, j] != before
    observed = rng.standard_normal(shape)
    prob = _problem(taps, observed)
    plan = _plan(monkeypatch, prob)
    assert plan[0] == 8 and plan[1] == separable, plan
    _check_operator(prob, taps, observed, plan, rng, f"near_rank1 {eps:g}")


@pytest.mark.parametrize("k,kind", [(3, "separable"), (3, "general"), (5, "separable"), (5, "general"), (7, "separable"), (9, "general")])
def test_walking_workgroups_at_the_operator_level(k, kind, monkeypatch):
    """1410 tiles of 64 x 32 (1502 x 1898, sides no multiples of the tile) - more than the device holds workgroups: a
    workgroup walks several tiles with the next one's coefficients in flight - for the six walking combinations
    tests/test_gpu_operator_lasso.py does not run.  ZF_OP_PERSIST=0 (a workgroup per tile): bit-identical; both inside
    the bound."""
    shape = (1502, 1898)
    seed = 500 + 10 * k + (kind == "general")
    taps, observed = E.make_taps(np.random.default_rng(seed), k, kind), np.random.default_rng(seed + 1).standard_normal(shape)
    prob = _problem(taps, observed)
    rng = np.random.default_rng(seed + 2)
    xs = rng.standard_normal(prob.n_features), rng.standard_normal(prob.n_features)
    monkeypatch.setenv("ZF_OP_PERSIST", "1")
    plan = _plan(monkeypatch, prob)
    assert plan[0] == 32 and plan[1] == (kind == "separable") and plan[2] == 1, plan
    jac, f = _check_operator(prob, taps, observed, plan, rng, f"walk k{k} {kind}", xs=xs)
    monkeypatch.setenv("ZF_OP_PERSIST", "0")
    plan = _plan(monkeypatch, prob)
    assert plan[0] == 32 and plan[1] == (kind == "separable") and plan[2] == 0, plan
    assert np.array_equal(prob.jac_f(xs[0]), jac) and np.array_equal(prob.f(xs[1]), f)     # (so inside the bound as well)


# ---- solver level: the fused trial --------------------------------------------------------------------------------------
def _oracle(taps, observed, lam, scale=1.0, bounds=None):
    """The oracle's four callbacks, with scale and a box wrapped around them (oracle/problems_ref.py: g is inf outside
    the box, the prox clips the soft-thresholded point into it)."""
    from oracle import operator_ref as O

    ref = O.BlurHaarL1Ref(taps, observed, l1_ratio=lam)

    def g(x):
        if bounds is not None and ((x < bounds[0]).any() or (x > bounds[1]).any()):
            return np.array([np.inf])
        return ref.g(x)

    def prox(weight, x):
        p = ref.prox_wsum_g(weight, x)
        return p if bounds is None else np.clip(p, *bounds)

    return (lambda x: scale * ref.f(x)), g, (lambda x: scale * ref.jac_f(x)), prox


def _fused_against_unfused_and_oracle(monkeypatch, taps, observed, kw, expect, lam=LAM, scale=1.0, bounds=None, label=""):
    """One solve with the prox step in the adjoint kernel's epilogue, one with a launch of its own (ZF_OP_FUSE_PROX=0):
    same decisions, x to 1e-13, fun to 1e-12 (only the order of the step's four sums differs); the fused one against
    the oracle at TOL.  `expect`: (tile height, separable) the plans must show."""
    from oracle import cpu_ref, operator_ref as O

    prob = _problem(taps, observed, lam, scale, bounds)
    x0 = O.dwt(observed)
    if bounds is not None:
        x0 = np.clip(x0, *bounds)
    out, plan = {}, {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("ZF_OP_FUSE_PROX", fuse)
        out[fuse], plan[fuse] = _solve_recording_plan(monkeypatch, prob, x0, kw)
        assert tuple(plan[fuse][:2]) == expect and plan[fuse][3] == int(fuse), plan      # this trial, this instantiation
    a, b = out["1"], out["0"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = cpu_ref.minimize_proximal_gradient(*_oracle(taps, observed, lam, scale, bounds), x0, **kw)
    print(f"{label}: plans {tuple(plan['1'])} / {tuple(plan['0'])}  fused-unfused x {rel_err(a.x, b.x):.2g}  fused-oracle x {rel_err(a.x, exp.x):.2g}  nit {a.nit}")
    assert a.nit == b.nit == exp.nit and a.status == b.status == exp.status
    assert rel_err(a.x, b.x) <= 1e-13
    np.testing.assert_allclose(np.asarray(a.fun), np.asarray(b.fun), rtol=1e-12)
    assert rel_err(a.x, exp.x) <= TOL
    np.testing.assert_allclose(np.asarray(a.fun), np.asarray(exp.fun), rtol=TOL)
    return a, exp


@pytest.mark.parametrize("k,ty,kind", MATRIX)
def test_fused_trial_of_every_instantiation(k, ty, kind, monkeypatch):
    """Four FISTA iterations at lr = 1 / (2 (sum |taps|)^2) = 0.5 - a valid 1 / L, no rejection.  (The sharp element-wise
    check of these kernels is test_every_instantiation_element_by_element; here the fused forms run at all, and agree.)"""
    rng = np.random.default_rng(2000 * k + ty + (kind == "general"))
    taps, observed = E.make_self_adjoint_taps(rng, k, kind), rng.standard_normal(SHAPES[ty])
    kw = dict(lr=0.5, nesterov=True, tol=0.0, max_iter=4)
    res, exp = _fused_against_unfused_and_oracle(monkeypatch, taps, observed, kw, (ty, int(kind == "separable")), label=f"fused k{k} ty{ty} {kind}")
    assert res.nit == 4 and exp.alltrials == [1, 1, 1, 1]


VARIANTS = {   # name: (K, kind, shape, tile height, solver options, problem options) - spread over the matrix, K > 9 among them
    "ista": (11, "separable", (100, 200), 8, dict(lr=0.5, nesterov=False, tol=0.0, max_iter=4), {}),                  # the epilogue's ov = kv branch
    "box": (13, "general", (566, 950), 32, dict(lr=0.5, nesterov=True, tol=0.0, max_iter=4), dict(bounds=(-0.05, 0.4))),
    "rejections": (15, "separable", (100, 200), 8, dict(lr=20.0, decay_rate=0.5, nesterov=True, tol=0.0, max_iter=4), {}),   # 40 x the safe step: a retry re-runs the fused adjoint
    "scale_0.37": (5, "general", (566, 950), 32, dict(lr=0.5 / 0.37, nesterov=True, tol=0.0, max_iter=4), dict(scale=0.37)),
    "narrow_1000x2": (3, "general", (1000, 2), 8, dict(lr=0.5, nesterov=True, tol=0.0, max_iter=4), {}),               # 125 workgroups write the step's partials
    "tall_16400x2": (3, "separable", (16400, 2), 32, dict(lr=0.5, nesterov=True, tol=0.0, max_iter=4), {}),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_fused_trial_variants(name, monkeypatch):
    k, kind, shape, ty, kw, popt = VARIANTS[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    taps, observed = E.make_self_adjoint_taps(rng, k, kind), rng.standard_normal(shape)
    res, exp = _fused_against_unfused_and_oracle(monkeypatch, taps, observed, kw, (ty, int(kind == "separable")), label=name, **popt)
    if name == "rejections":
        assert sum(exp.alltrials) > len(exp.alltrials), exp.alltrials      # trials really were rejected


@pytest.mark.parametrize("width,fused", [(2560, 1), (2562, 0)])
def test_fusion_threshold(width, fused, monkeypatch):
    """2048 x 2560 is 5 Mi pixels exactly - the largest image whose prox step rides in the adjoint kernel; two columns
    more and it is a launch of its own.  Three iterations against the oracle."""
    from oracle import cpu_ref, operator_ref as O

    rng = np.random.default_rng(width)
    taps, observed = E.make_self_adjoint_taps(rng, 3, "general"), rng.standard_normal((2048, width))
    prob = _problem(taps, observed)
    x0 = O.dwt(observed)
    kw = dict(lr=0.5, nesterov=True, tol=0.0, max_iter=3)
    res, plan = _solve_recording_plan(monkeypatch, prob, x0, kw)
    assert plan[0] == 32 and plan[1] == 0 and plan[3] == fused, plan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = cpu_ref.minimize_proximal_gradient(*_oracle(taps, observed, LAM), x0, **kw)
    assert res.nit == exp.nit == 3
    assert rel_err(res.x, exp.x) <= TOL
    np.testing.assert_allclose(np.asarray(res.fun), np.asarray(exp.fun), rtol=TOL)
