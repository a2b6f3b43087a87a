"""GPU: the kernels of csrc/zf_multiobj.hip element by element and sum by sum, at every m = 2 .. 8 and at the sizes where their
index arithmetic changes (tests/mo_cases.py: the table, the references and the bounds; tests/test_mo_cases.py proves on the CPU
that the table reaches what it claims and that the bounds show every mutant).

(a) k_prox_only, k_recover: prox_host(lr w, y) and recover(lr, w) + get(X_NEW) bit for bit, err bit for bit max |x+ - y|; every
    m x g variant at the sizes up to 1000, m = 2, 5, 8 with l1 + per-coordinate bounds at 262143 .. 524289 (the second trip of
    the stride loop starts at element 262144).
(b) k_commit: y = x_k + beta (x_k - x_{k-1}) and y = x_k bit for bit at every size.
(c) k_dual_eval, k_post_terms, k_g_terms: the 2m + 2, m + 1 and m sums within their a-priori bounds at three weights (uniform,
    interior, one zero component), same cases as (a).
(d) k_dual_hessian, m = 2 .. 5: the m x m sums within their bound.
(e) the violation count of k_g_terms: one element outside the box at 0, n - 1 and 262144 gives inf, none gives a finite g.
(f) k_jos1_* / k_fds_*: prepare() at every size; the JOS1 rows bit for bit, f and the FDS rows within the exp-aware bounds.
(g) a NaN in y (grid-stride kernels only): every sum that reads y is NaN, |w @ J|^2 stays within its bound.
(h) k_dual_solve<2 .. 8>: with the w* it returns, x+ and err bit for bit, g(x+) and the dual value within their bounds, w* on the
    simplex and within 1e-9 of the host-driven search; one row per workgroup (resident by construction), two, three, and two
    sizes of more than capmax(m) rows (streamed by construction); with per-coordinate bounds for m = 2, 3, 5, 8.
(i) the fused prologue of k_dual_solve (JOS1, FDS): y, J bit for bit what the unfused launches leave, f(y) within its bound,
    for the first trial and for the one after commit() (the make_y branch).
No skip, no expected failure; no non-finite input and no forced timeout goes to the persistent kernel.  ZF_MO_BOUNDS_RECORD=1
appends the worst error / bound per kernel and m to profiles/mo_kernel_bounds.jsonl (any other value: that path)."""
import json
import os

import numpy as np
import pytest

import mo_cases as C
from conftest import ROOT

pytestmark = pytest.mark.gpu
X_K, Y, X_NEW, X_OLD = 0, 1, 2, 3
WORST = {}


def _note(kernel, m, err, bound):
    """The worst err / bound of one comparison, kept per kernel and m; an error where the bound is 0 is infinite."""
    err, bound = np.atleast_1d(np.asarray(err, dtype=float)), np.atleast_1d(np.asarray(bound, dtype=float))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(err == 0.0, 0.0, err / bound), initial=0.0))
    WORST[(kernel, m)] = max(WORST.get((kernel, m), 0.0), ratio)
    return ratio


@pytest.fixture(scope="module", autouse=True)
def _record_worst_ratios():
    yield
    where = os.environ.get("ZF_MO_BOUNDS_RECORD", "")
    if where in ("", "0"):
        return
    path = os.path.join(ROOT, "profiles", "mo_kernel_bounds.jsonl") if where == "1" else where
    with open(path, "a") as fh:
        for (kernel, m), ratio in sorted(WORST.items()):
            fh.write(json.dumps({"test": "mo-kernels", "kernel": kernel, "m": m, "ratio": ratio}) + "\n")


def _within(kernel, m, got, want, bound, what):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    ratio = _note(kernel, m, np.abs(got - want), bound)
    print(f"  {kernel} m = {m} {what}: worst error / bound {ratio:.3g}")
    assert ratio <= 1.0, (kernel, what, got, want, bound)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(C.bits(got).reshape(-1) != C.bits(want).reshape(-1))
    assert bad.size == 0, (what, bad.size, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


def _cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- (a), (c) ----------------------------------------------------------------------------------------------------------------------
def _prox_recover_and_sums(m, variant, n):
    c = C.case(m, variant, n)
    g, lr = c.g, c.lr
    eng = C.engine(c)
    try:
        for name, w in C.weights(m).items():
            what = f"{variant} n = {n} {name}"
            coef, tail = C.coefs(g, lr, w)
            _same(eng.prox_host(lr * w, c.y), C.prox(g, coef, tail, c.y), "prox_host " + what)
            wJ, v, p, err = C.trial_point(c, lr, w)
            got_err = eng.recover(lr, w)
            _same(eng.get(X_NEW), p, "recover " + what)
            _same(np.array([got_err]), np.array([err]), "err " + what)
            S, B = C.dual_sums(c, lr, w)
            gp, pv, wj, dots = eng.dual_eval(lr, w)
            _within("k_dual_eval", m, np.concatenate([gp, [pv, wj], dots]), S, B, what)
            PS, PB = C.post_sums(c, lr, w, c.xk)
            dots, dv = eng.post_terms(lr, w, c.xk)
            _within("k_post_terms", m, np.append(dots, dv), PS, PB, what)
            # g at the recovered point (inside the box, some elements exactly on a bound: no violation)
            eng.put(X_K, p)
            gv, gb = C.g_ref(g, p)
            got = eng.eval_F(X_K, builtin_f=False)[1]
            assert np.isfinite(got).all(), what
            if g.l1:
                _within("k_g_terms", m, got, gv, gb, what)
            else:
                assert not got.any(), what
    finally:
        eng.close()


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("m", C.MS)
def test_prox_recovery_and_sums_at_the_wave_and_workgroup_edges(m, variant):
    for n in C.N_SMALL:
        _prox_recover_and_sums(m, variant, n)


@pytest.mark.parametrize("n", C.N_LARGE)
@pytest.mark.parametrize("m", C.M_LARGE)
def test_prox_recovery_and_sums_around_the_second_stride_trip(m, n):
    assert C.grid_of(n) == C.MO_GRID_MAX and (n > 262144) == (n > C.MO_GRID_MAX * C.ZF_BLOCK)
    _prox_recover_and_sums(m, "l1_boxv", n)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.N_GRID)
def test_commit_bit_for_bit(n):
    c = C.case(2, "plain", n)
    for nesterov in (True, False):
        eng = C.engine(c)
        try:
            eng.set_x0(c.xo)
            eng.put(X_NEW, c.xk)
            eng.commit(0.4375 + 1.0 / 3.0, nesterov)
            _same(eng.get(X_K), c.xk, "x_k")
            _same(eng.get(X_OLD), c.xo, "x_{k-1}")
            _same(eng.get(Y), C.commit_ref(c.xk, c.xo, 0.4375 + 1.0 / 3.0, nesterov), f"y n = {n} nesterov {nesterov}")
        finally:
            eng.close()


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 257, 1000, 262145])
@pytest.mark.parametrize("m", [2, 3, 4, 5])
def test_dual_hessian_within_its_bound(m, n):
    for variant in (("l1_boxv",) if n > 1000 else ("l1_boxv", "l1", "box", "plain")):
        c = C.case(m, variant, n)
        eng = C.engine(c)
        try:
            for name in ("uniform", "interior") if n <= 1000 else ("interior",):
                w = C.weights(m)[name]
                H, HB = C.hessian_ref(c, c.lr, w)
                _within("k_dual_hessian", m, eng.dual_hessian(c.lr, w), H, HB, f"{variant} n = {n} {name}")
        finally:
            eng.close()


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["box", "boxv", "l1_boxv"])
def test_one_box_violation_anywhere_makes_g_infinite(variant):
    m, n = 3, 262145
    c = C.case(m, variant, n)
    g = c.g
    eng = C.engine(c)
    try:
        p = C.prox(g, *C.coefs(g, c.lr, C.weights(m)["interior"]), c.y)   # feasible, with elements exactly on their bounds
        eng.put(X_K, p)
        assert np.isfinite(eng.eval_F(X_K, builtin_f=False)[1]).all()
        lo, hi = np.broadcast_to(g.lo, (n,)), np.broadcast_to(g.hi, (n,))
        for j in (0, n - 1, 262144):
            for side in (0, 1):
                x = p.copy()
                x[j] = np.nextafter(lo[j], -np.inf) if side == 0 else np.nextafter(hi[j], np.inf)
                eng.put(X_K, x)
                got = eng.eval_F(X_K, builtin_f=False)[1]
                assert np.isposinf(got).all(), (variant, j, side, got)
        eng.put(X_K, p)
        assert np.isfinite(eng.eval_F(X_K, builtin_f=False)[1]).all()
    finally:
        eng.close()


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------
def _builtin(kind, n, y):
    from zfista_amd import _lib
    from zfista_amd.multiobjective import MoEngine

    m = 2 if kind == "jos1" else 3
    ratios, shifts = C.l1_params(m)
    eng = MoEngine(_lib.ZF_MO_JOS1 if kind == "jos1" else _lib.ZF_MO_FDS, m, n, ratios / n, shifts)
    eng.set_x0(y)
    return eng


def _fds_rows_agree(J, rows, extra, what):
    """Rows 0 .. 2 of the FDS Jacobian: row 0 has no exp (bit for bit); rows 1 and 2 within 2 ulp of their np.longdouble values
    (row 1: plus the allowance for the order of sum(y) behind exp(sum(y) / n))."""
    _same(J[0], rows[0], what + " row 0")
    d1 = C.ulp_distance(J[1], rows[1], allow=extra)
    d2 = C.ulp_distance(J[2], rows[2])
    print(f"  FDS {what}: worst distance row 1 {d1.max():.3g} ulp, row 2 {d2.max():.3g} ulp")
    assert d1.max() <= 2.0 and d2.max() <= 2.0, (what, "ulp distances", float(d1.max()), float(d2.max()))


@pytest.mark.parametrize("n", C.N_GRID)
@pytest.mark.parametrize("kind", ["jos1", "fds"])
def test_builtin_f_and_jacobian_at_every_size(kind, n):
    y = C.case(3, "l1", n).y
    eng = _builtin(kind, n, y)
    try:
        f_y = eng.prepare()
        J = eng.get_jac()
        if kind == "jos1":
            _same(J, C.jos1_jac(y), f"JOS1 rows n = {n}")
            f, fb = C.jos1_f_ref(y)
            _within("k_jos1_sums", 2, f_y, f, fb, f"n = {n}")
        else:
            f, fb, rows, extra = C.fds_ref(y)
            _fds_rows_agree(J, rows, extra, f"n = {n}")
            _within("k_fds_sums", 3, f_y, f, fb, f"n = {n}")
    finally:
        eng.close()


# ---- (g) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [513, 262145])
def test_a_nan_in_the_last_element_of_y_reaches_every_sum_that_reads_y(n):
    m = 3
    c = C.case(m, "l1", n)
    eng = C.engine(c)
    try:
        y = c.y.copy()
        y[n - 1] = np.nan
        eng.put(Y, y)
        w = C.weights(m)["uniform"]
        gp, pv, wj, dots = eng.dual_eval(c.lr, w)
        assert np.isnan(gp).all() and np.isnan(pv) and np.isnan(dots).all(), (gp, pv, dots)
        S, B = C.dual_sums(c, c.lr, w)
        _within("k_dual_eval", m, [wj], [S[m + 1]], [B[m + 1]], f"|wJ|^2 beside a NaN, n = {n}")
        eng.put(Y, c.y)
        gp, pv, wj, dots = eng.dual_eval(c.lr, w)
        assert np.isfinite(np.concatenate([gp, [pv, wj], dots])).all()
    finally:
        eng.close()


# ---- (h) ---------------------------------------------------------------------------------------------------------------------------
SOLVE_SIZES = ("1", "511", "512", "513", "G512-1", "G512", "G512+1", "2G512+1", "streamed+1", "streamed+G256+3")


def _solve_n(tag, G, m):
    return (C.n_solve(G, m) + C.n_streamed(G, m))[SOLVE_SIZES.index(tag)]


def _persistent_search(m, variant, tag):
    G = _cus()
    n = _solve_n(tag, G, m)
    rows = -(-n // (min(-(-n // 512), G) * 512))
    if tag.startswith("streamed"):
        assert rows > C.capmax(m), "this size must stream at least one row whatever the kernel's static LDS is"
    elif tag not in ("G512+1", "2G512+1"):
        assert rows == 1, "this size must be wholly resident"
    c = C.case(m, variant, n)
    lr, g = c.lr, c.g
    f_y, F_old = C.solve_inputs(c)
    eng = C.engine(c)
    try:
        out = eng.solve_dual_device(lr, f_y, F_old, False, None, 1e-12, 100000)
        assert out is not None, "the device search was not attempted"
        w, fun, nit, err, _, g_x, fy_used = out
        x = eng.get(X_NEW)
        what = f"{variant} {tag} (n = {n}, {G} CUs, {rows} rows per workgroup)"
        print(f"  {what}: w* = {w}, nit {nit}, {eng.solve_stats()['evals']} evaluations")
        assert abs(w.sum() - 1.0) <= 1e-12 and (w >= 0).all(), w
        _same(fy_used, f_y, "f(y)")
        _, _, p, e = C.trial_point(c, lr, w)
        _same(x, p, "x+ " + what)
        _same(np.array([err]), np.array([e]), "err " + what)
        gv, gb = C.g_ref(g, p)
        _within("k_dual_solve g(x+)", m, g_x, gv, gb, what)
        np.testing.assert_allclose(g_x, eng.eval_F(X_NEW, builtin_f=False)[1], rtol=1e-12)
        S, B = C.dual_sums(c, lr, w)
        fun_ref, fb, _, _ = C.dual_ref(c, lr, w, f_y, F_old, S, B)
        _within("k_dual_solve fun", m, [fun], [fun_ref], [fb], what)
        host = eng.solve_dual(lr, f_y, F_old, False, None, 1e-12, 100000)
        assert host is not None
        assert np.abs(w - host[0]).max() <= 1e-9, (what, w, host[0])
    finally:
        eng.close()


@pytest.mark.parametrize("tag", SOLVE_SIZES)
@pytest.mark.parametrize("m", C.MS)
def test_persistent_search_resident_and_streamed(m, tag):
    _persistent_search(m, "l1", tag)


@pytest.mark.parametrize("tag", ["G512+1", "streamed+1", "streamed+G256+3"])
@pytest.mark.parametrize("m", [2, 3, 5, 8])
def test_persistent_search_with_per_coordinate_bounds(m, tag):
    _persistent_search(m, "l1_boxv", tag)


# ---- (i) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["1", "511", "513", "G512+1", "streamed+1"])
@pytest.mark.parametrize("kind", ["jos1", "fds"])
def test_fused_prologue_leaves_what_the_unfused_launches_leave(kind, tag):
    m = 2 if kind == "jos1" else 3
    G = _cus()
    n = _solve_n(tag, G, m)
    if tag == "streamed+1":
        assert -(-n // (G * 512)) > C.capmax(m)
    x0 = C.case(3, "l1", n).y
    lr = 1.0 if kind == "jos1" else min(1e-2, 0.1 / (4.0 * n * n))   # FDS: |J_0| reaches 4 n^2; the step stays below 0.1
    beta = 0.28125 + 1.0 / 3.0
    fused, plain = _builtin(kind, n, x0), _builtin(kind, n, x0)
    try:
        fused.set_fused(True)

        def f_ref(y):
            return C.jos1_f_ref(y) if kind == "jos1" else C.fds_ref(y)[:2]

        def trial(eng, F_old):
            eng.prepare_async()
            out = eng.solve_dual_device(lr, None, F_old, False, None, 1e-12, 100000)
            assert out is not None, "the device search was not attempted"
            return out

        def compare(which, y_want):
            ya, yb = fused.get(Y), plain.get(Y)
            _same(ya, yb, f"{kind} {tag} y, {which}")
            _same(ya, y_want, f"{kind} {tag} y against the reference, {which}")
            _same(fused.get_jac(), plain.get_jac(), f"{kind} {tag} J, {which}")
            f, fb = f_ref(y_want)
            for eng, name in ((fused, "fused"), (plain, "unfused")):
                _within("k_dual_solve prologue f(y)" if eng is fused else "prepare_async f(y)", m, eng.get_f_y(), f, fb,
                        f"{kind} {tag} {which} {name}")

        f0, g0 = plain.eval_F(X_K)
        F_old = f0 + g0
        out = trial(fused, F_old)
        plain.prepare_async()
        compare("first trial", x0)
        # the accepted point of the fused engine goes to both: the commit is deferred into the next launch (make_y)
        x_new = fused.get(X_NEW)
        F_new = out[4] + out[5]
        assert np.isfinite(F_new).all()
        plain.put(X_NEW, x_new)
        fused.commit(beta, True)
        plain.commit(beta, True)
        trial(fused, F_new)
        plain.prepare_async()
        compare("after commit", C.commit_ref(x_new, x0, beta, True))
    finally:
        fused.close()
        plain.close()
