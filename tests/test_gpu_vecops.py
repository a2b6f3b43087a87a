"""GPU: the vector kernels of csrc/zf_vecops.hip - the solver's own arithmetic on the callback paths and the g / jac_f /
prox_wsum_g callables of the problem classes - element by element and sum by sum, called directly through the C ABI, _VecOps,
_DevOps and the problem classes, at the sizes where their index arithmetic changes (tests/vecops_cases.py: the table, the
references, the bounds and the model of the summation order; tests/test_vecops_cases.py proves them on the CPU).

(a) element-wise, bit for bit, NaN for NaN: zf_host_ / zf_dev_grad_step, zf_host_ / zf_dev_momentum (beta 0, 1/4, 1),
    zf_host_prox_l1_box, zf_host_prox_enet_box (tau = 0 and > 0, four boxes), zf_host_diag_grad at every size up to 65537;
    grad_step, momentum and prox_l1_box around the grid cap and in the third trip of the stride loop.
(b) sums at every size: zf_host_model_terms, zf_dev_model_terms, zf_dev_model_terms_async, zf_eval_diag_l1, zf_host_asum,
    zf_host_enet_g - within the a-priori bound of the np.longdouble value, equal in every bit to the model of the summation
    order, and (model terms) the three forms and a second call equal in every bit.
(c) an infinite or NaN difference at the first, the last and a second-trip position; a NaN in the data of a solve on either
    callback engine ends as the oracle's does.
(d) the staging workspace: calls of shrinking and growing sizes, host- and device-pointer forms interleaved, zf_shutdown() in
    between, two threads at once, a thread that ended.
(e) every zf_dev_* call on a fresh stream gives the bits of the default stream.
(f) n = 0 and the refusals.
(g) one solve past the grid cap on each callback engine against the oracle.
No skip, no expected failure.  ZF_VECOPS_BOUNDS_RECORD=1 appends the worst error / bound per entry point and size class to
profiles/vecops_bounds.jsonl (any other value: that path)."""
import ctypes as C
import json
import os
import threading
import warnings

import numpy as np
import pytest

import vecops_cases as V
from conftest import ROOT

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _record_worst_ratios():
    yield
    where = os.environ.get("ZF_VECOPS_BOUNDS_RECORD", "")
    if where in ("", "0"):
        return
    path = os.path.join(ROOT, "profiles", "vecops_bounds.jsonl") if where == "1" else where
    with open(path, "a") as fh:
        for (entry, cls), ratio in sorted(WORST.items()):
            fh.write(json.dumps({"test": "vecops", "entry": entry, "size_class": cls, "ratio": ratio}) + "\n")


# ---- the entry points ----------------------------------------------------------------------------------------------------------------
def _lib():
    from zfista_amd import _lib as L

    return L.require_gpu()


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _d(t):
    return C.c_void_p(t.data_ptr())


def _dev(*arrays):
    import torch

    out = tuple(torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda() for a in arrays)   # (a copy: the cases are read-only)
    return out if len(out) > 1 else out[0]


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    from zfista_amd import _lib as L

    L.check(rc, what)


def host_model_terms(jac, x, y):
    out = np.full(3, -7.0)
    _ok(_lib().zf_host_model_terms(_p(jac), _p(x), _p(y), x.size, _p(out)), "zf_host_model_terms")
    return out


def dev_model_terms(jt, xt, yt):
    out = np.full(3, -7.0)
    _ok(_lib().zf_dev_model_terms(_d(jt), _d(xt), _d(yt), xt.numel(), _p(out), _stream()), "zf_dev_model_terms")
    return out


def dev_model_terms_async(jt, xt, yt):
    import torch

    out = torch.full((3,), -7.0, dtype=torch.float64, device="cuda")
    _ok(_lib().zf_dev_model_terms_async(_d(jt), _d(xt), _d(yt), xt.numel(), _d(out), _stream()), "zf_dev_model_terms_async")
    return out.cpu().numpy()


def eval_diag(xt, dt, ct, lam):
    out = np.full(2, -7.0)
    _ok(_lib().zf_eval_diag_l1(_d(xt), _d(dt), _d(ct), lam, xt.numel(), _p(out), _stream()), "zf_eval_diag_l1")
    return out


def host_asum(x):
    s = C.c_double(-7.0)
    _ok(_lib().zf_host_asum(_p(x), x.size, C.byref(s)), "zf_host_asum")
    return s.value


def host_enet_g(x, lam, l2):
    s = C.c_double(-7.0)
    _ok(_lib().zf_host_enet_g(_p(x), x.size, lam, l2, C.byref(s)), "zf_host_enet_g")
    return s.value


def host_prox_l1_box(u, tau, lo, hi):
    out = np.full_like(u, -7.0)
    _ok(_lib().zf_host_prox_l1_box(_p(out), _p(u), tau, lo, hi, u.size), "zf_host_prox_l1_box")
    return out


def host_prox_enet_box(u, tau, shrink, lo, hi):
    out = np.full_like(u, -7.0)
    _ok(_lib().zf_host_prox_enet_box(_p(out), _p(u), tau, shrink, lo, hi, u.size), "zf_host_prox_enet_box")
    return out


def host_diag_grad(x, dt, ct):
    out = np.full_like(x, -7.0)
    _ok(_lib().zf_host_diag_grad(_p(out), _p(x), _d(dt), _d(ct), x.size), "zf_host_diag_grad")
    return out


def _same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    bad = V.differing(got, want)
    assert bad.size == 0, (what, bad.size, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


def _sum_agrees(entry, n, got, ref, bound, model):
    """(i) within the bound of the np.longdouble value, (ii) the bits of the model of the summation order."""
    got, ref, bound, model = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (got, ref, bound, model))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(err == 0.0, 0.0, err / bound)))
    key = (entry, V.size_class(n))
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"  {entry} n = {n}: worst error / bound {ratio:.3g}; differs from the model by {np.abs(got - model).max():.3g}")
    assert ratio <= 1.0, (entry, n, got, ref, bound)
    _same(got, model, f"{entry} n = {n} against the model of the summation order")


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------
def _grad_step_and_momentum(n):
    from zfista_amd.proximal_gradient import _DevOps, _VecOps

    host, dev = _VecOps(), _DevOps()
    a, b, _ = V.elementwise_inputs(n)
    at, bt = _dev(a, b)
    want = V.grad_step(a, b, V.LR)
    _same(host.grad_step(a, b, V.LR), want, f"zf_host_grad_step n = {n}")
    _same(dev.grad_step(at, bt, V.LR).cpu().numpy(), want, f"zf_dev_grad_step n = {n}")
    for beta in V.BETAS:
        want = V.momentum(a, b, beta)
        _same(host.momentum(a, b, beta), want, f"zf_host_momentum n = {n} beta = {beta}")
        _same(dev.momentum(at, bt, beta).cpu().numpy(), want, f"zf_dev_momentum n = {n} beta = {beta}")


@pytest.mark.parametrize("n", V.N_ALL)
def test_grad_step_and_momentum_bit_for_bit(n):
    _grad_step_and_momentum(n)


@pytest.mark.parametrize("n", V.N_SMALL)
def test_prox_forms_and_diag_grad_bit_for_bit(n):
    from zfista_amd.problems import DiagQuadL1

    shrink = 1.0 / (1.0 + V.L2 * V.LR)
    for tau in V.TAUS:
        u = V.prox_input(n, tau)
        for lo, hi in V.BOXES:
            _same(host_prox_l1_box(u, tau, lo, hi), V.prox_l1_box(u, tau, lo, hi), f"zf_host_prox_l1_box n = {n} tau = {tau} [{lo}, {hi}]")
            for s in (1.0, shrink):
                _same(host_prox_enet_box(u, tau, s, lo, hi), V.prox_enet_box(u, tau, s, lo, hi),
                      f"zf_host_prox_enet_box n = {n} tau = {tau} shrink = {s} [{lo}, {hi}]")
    a, b, c = V.elementwise_inputs(n)
    bt, ct = _dev(b, c)
    _same(host_diag_grad(a, bt, ct), V.diag_grad(a, b, c), f"zf_host_diag_grad n = {n}")
    # the same kernels as the callables of a problem class: prox_wsum_g(weight, .) thresholds at lam * weight
    prob = DiagQuadL1(b.copy(), c.copy(), 0.1, bounds=(-0.3, 0.4))
    _same(prob.jac_f(a), V.diag_grad(a, b, c), f"DiagQuadL1.jac_f n = {n}")
    u = V.prox_input(n, V.TAUS[1])
    _same(prob.prox_wsum_g(0.45, u), V.prox_l1_box(u, 0.1 * 0.45, -0.3, 0.4), f"DiagQuadL1.prox_wsum_g n = {n}")


@pytest.mark.parametrize("n", V.N_LARGE)
def test_prox_l1_box_around_the_grid_cap(n):
    tau = V.TAUS[1]
    u = V.prox_input(n, tau)
    for lo, hi in V.BOXES[:2]:
        _same(host_prox_l1_box(u, tau, lo, hi), V.prox_l1_box(u, tau, lo, hi), f"zf_host_prox_l1_box n = {n} [{lo}, {hi}]")


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", V.N_ALL)
def test_every_sum_within_its_bound_and_in_the_documented_order(n):
    c = V.reduction_case(n)
    jt, xt, yt, dt, ct = _dev(c.jac, c.x, c.y, c.d, c.c)
    ref, bound = V.model_terms_ref(c.jac, c.x, c.y)
    model = V.emulate_model_terms(c.jac, c.x, c.y)
    forms = {"zf_host_model_terms": lambda: host_model_terms(c.jac, c.x, c.y), "zf_dev_model_terms": lambda: dev_model_terms(jt, xt, yt),
             "zf_dev_model_terms_async": lambda: dev_model_terms_async(jt, xt, yt)}
    got = {}
    for entry, call in forms.items():
        got[entry] = call()
        _sum_agrees(entry, n, got[entry], ref, bound, model)
        _same(call(), got[entry], f"{entry} n = {n}, a second call")
    _same(got["zf_dev_model_terms"], got["zf_host_model_terms"], "device against host pointers")
    _same(got["zf_dev_model_terms_async"], got["zf_host_model_terms"], "async against host pointers")
    _sum_agrees("zf_eval_diag_l1", n, eval_diag(xt, dt, ct, V.LAM), *V.eval_diag_ref(c.x, c.d, c.c, V.LAM),
                V.emulate_eval_diag(c.x, c.d, c.c, V.LAM))
    _sum_agrees("zf_host_asum", n, host_asum(c.x), *V.asum_ref(c.x), V.emulate_asum(c.x))
    _sum_agrees("zf_host_enet_g", n, host_enet_g(c.x, V.LAM, V.L2), *V.enet_g_ref(c.x, V.LAM, V.L2), V.emulate_enet_g(c.x, V.LAM, V.L2))


def test_the_problem_classes_reach_the_same_sums():
    """DiagQuadL1.f / .g are zf_eval_diag_l1, the g of a margins class is zf_host_asum (l2 = 0) or zf_host_enet_g."""
    from zfista_amd.problems import DiagQuadL1, LeastSquaresL1

    n = 65537
    c = V.reduction_case(n)
    x = c.x.copy()   # (the classes hand their argument to torch, which wants it writable)
    prob = DiagQuadL1(c.d.copy(), c.c.copy(), V.LAM)
    want = V.emulate_eval_diag(c.x, c.d, c.c, V.LAM)
    _same([prob.f(x), prob.g(x)], want, "DiagQuadL1.f, .g")
    rng = np.random.default_rng(5)
    A, b = rng.standard_normal((3, n)), rng.standard_normal(3)
    _same([LeastSquaresL1(A, b, V.LAM).g(c.x)], [V.LAM * V.emulate_asum(c.x)], "LeastSquaresL1.g")
    _same([LeastSquaresL1(A, b, V.LAM, l2=V.L2).g(c.x)], [V.emulate_enet_g(c.x, V.LAM, V.L2)], "LeastSquaresL1(l2=).g")


# ---- (c) -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 524289])
def test_a_non_finite_difference_in_model_terms(n):
    c = V.reduction_case(n)
    jt, yt = _dev(c.jac, c.y)
    for j in sorted({0, n - 1, min(n - 1, V.CAP)}):
        rest = np.abs(np.delete(c.x - c.y, j)).max()
        for bad in (np.inf, -np.inf, np.nan):
            x = c.x.copy()
            x[j] = bad
            xt = _dev(x)
            model = V.emulate_model_terms(c.jac, x, c.y)
            for entry, got in (("host", host_model_terms(c.jac, x, c.y)), ("dev", dev_model_terms(jt, xt, yt)),
                               ("async", dev_model_terms_async(jt, xt, yt))):
                what = f"{entry} n = {n} x[{j}] = {bad}"
                if np.isnan(bad):   # the sums keep the NaN; fmax drops it: the maximum is that of the other elements
                    assert np.isnan(got[0]) and np.isnan(got[1]), what
                    _same(got[2], rest, what + ": the maximum without the NaN")
                else:
                    assert got[0] == np.sign(bad) * np.sign(c.jac[j]) * np.inf and got[1] == np.inf and got[2] == np.inf, (what, got)
                _same(got, model, what)


def _torch_diag(d, c, lam):
    import torch

    dt, ct = _dev(d, c)
    return (lambda x: 0.5 * torch.sum(dt * ((x - ct) * (x - ct))), lambda x: lam * torch.sum(torch.abs(x)),
            lambda x: dt * (x - ct), lambda w, v: torch.sign(v) * torch.clamp(torch.abs(v) - lam * w, min=0.0))


@pytest.mark.parametrize("engine", ["host", "tensor"])
@pytest.mark.parametrize("where", [0, 17])
def test_a_nan_in_the_data_ends_a_callback_solve_as_the_oracle_does(where, engine, capsys):
    """max(abs(xk - yk)) of the reference depends on the place of a NaN (proximal_gradient.py:510) where fmax drops it: there is
    no element-level parity to ask for.  The solve never gets there: no trial is accepted (NaN <= x is False), the line search
    fails and the error-shaped result is returned (:303-307, :493-509) - by both engines as by the oracle."""
    import torch

    from oracle import cpu_ref, problems_ref as P
    from zfista_amd import minimize_proximal_gradient

    n = 1000
    d, c, lam = P.make_pdiag(n, seed=4)
    c[where] = np.nan
    kw = dict(lr=0.45, nesterov=True, max_iter=10, max_backtrack_iter=6)
    ref = P.DiagQuadL1Ref(d, c, lam)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = cpu_ref.minimize_proximal_gradient(*ref.callbacks(), np.zeros(n), **kw)
        if engine == "host":
            res = minimize_proximal_gradient(*ref.callbacks(), np.zeros(n), **kw)
            x = res.x
        else:
            res = minimize_proximal_gradient(*_torch_diag(d, c, lam), torch.zeros(n, dtype=torch.float64, device="cuda"), **kw)
            x = res.x.cpu().numpy()
    capsys.readouterr()
    assert exp.success is False and res.success is False and res.message == exp.message
    assert res.nit == exp.nit == 0
    _same(x, exp.x, "x")


# ---- (d) -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def workspace_models():
    """The model's bits of every call of the workspace tests, computed once."""
    out = {}
    for n in (5000, 3, 600001, 1025, 1024, 70000, 65537):
        c = V.reduction_case(n)
        out[n] = dict(mt=V.emulate_model_terms(c.jac, c.x, c.y), asum=V.emulate_asum(c.x),
                      diag=V.emulate_eval_diag(c.x, c.d, c.c, V.LAM))
    return out


def _workspace_sequence(models):
    mid = V.reduction_case(70000)
    jt, xt, yt, dt, ct = _dev(mid.jac, mid.x, mid.y, mid.d, mid.c)
    for n in (5000, 3, 600001, 1025, 1024):
        c = V.reduction_case(n)
        _same(host_model_terms(c.jac, c.x, c.y), models[n]["mt"], f"zf_host_model_terms n = {n} in the sequence")
        _same(dev_model_terms(jt, xt, yt), models[70000]["mt"], f"zf_dev_model_terms n = 70000 after n = {n}")
        _same(host_asum(c.x), models[n]["asum"], f"zf_host_asum n = {n} in the sequence")
        _same(eval_diag(xt, dt, ct, V.LAM), models[70000]["diag"], f"zf_eval_diag_l1 n = 70000 after n = {n}")


def test_workspace_keeps_nothing_of_an_earlier_call(workspace_models):
    """Shrinking and growing sizes on one thread, the device-pointer forms (which share the partials and the result block)
    in between: every result has the bits of the call made alone, before and after zf_shutdown()."""
    _workspace_sequence(workspace_models)
    assert _lib().zf_shutdown() == 0
    _workspace_sequence(workspace_models)
    assert _lib().zf_shutdown() == 0
    c = V.reduction_case(1024)   # the first call of a fresh workspace is the smallest one
    _same(host_asum(c.x), workspace_models[1024]["asum"], "zf_host_asum after zf_shutdown()")


def test_two_threads_have_a_workspace_each(workspace_models):
    import torch

    results, errors = {65537: [], 1025: []}, []
    start = threading.Barrier(2)

    def loop(n):
        try:
            torch.cuda.set_device(0)
            c = V.reduction_case(n)
            jac, x, y = c.jac, c.x, c.y
            start.wait(timeout=60)
            for _ in range(20):
                results[n].append(host_model_terms(jac, x, y))
        except Exception as exc:   # reported by the main thread
            errors.append(exc)

    V.reduction_case(65537), V.reduction_case(1025)   # (both in the cache before the threads start)
    threads = [threading.Thread(target=loop, args=(n,)) for n in results]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for n, got in results.items():
        assert len(got) == 20
        for k, g in enumerate(got):
            _same(g, workspace_models[n]["mt"], f"thread n = {n}, call {k}")


def test_a_thread_that_ended_took_its_workspace_with_it(workspace_models):
    import torch

    got = []

    def once():
        torch.cuda.set_device(0)
        c = V.reduction_case(1025)
        got.append(host_model_terms(c.jac, c.x, c.y))

    t = threading.Thread(target=once)
    t.start()
    t.join()
    _same(got[0], workspace_models[1025]["mt"], "the thread's own call")
    assert _lib().zf_shutdown() == 0
    c = V.reduction_case(5000)
    _same(host_model_terms(c.jac, c.x, c.y), workspace_models[5000]["mt"], "the main thread afterwards")


# ---- (e) -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 65537, 524289])
def test_a_fresh_stream_gives_the_bits_of_the_default_stream(n):
    import torch

    from zfista_amd.proximal_gradient import _DevOps

    ops = _DevOps()
    c = V.reduction_case(n)
    a, b, _ = V.elementwise_inputs(n)
    at, bt, jt, xt, yt, dt, ct = _dev(a, b, c.jac, c.x, c.y, c.d, c.c)
    rng = np.random.default_rng(n)
    J, w = rng.standard_normal((3, n)), rng.random(3)
    Jt = _dev(J)

    def calls():
        v, ss = ops.mo_combine(yt, Jt, w, V.LR)
        return [ops.grad_step(at, bt, V.LR), ops.momentum(at, bt, 0.25), torch.from_numpy(np.array(ops.model_terms(jt, xt, yt))),
                ops.model_terms_dev(jt, xt, yt), torch.from_numpy(eval_diag(xt, dt, ct, V.LAM)), v, ss, ops.mo_post_terms(Jt, yt, xt, v)]

    torch.cuda.synchronize()
    base = [t.cpu().numpy() for t in calls()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream().cuda_stream == s.cuda_stream != 0
        out = calls()
        s.synchronize()
        got = [t.cpu().numpy() for t in out]
    names = ["grad_step", "momentum", "model_terms", "model_terms_async", "eval_diag_l1", "mo_combine v", "mo_combine |wJ|^2", "mo_post_terms"]
    for name, g, want in zip(names, got, base):
        _same(g, want, f"{name} n = {n} on a fresh stream")
    _same(base[0], V.grad_step(a, b, V.LR), "grad_step")
    _same(base[2], V.emulate_model_terms(c.jac, c.x, c.y), "model_terms")


# ---- (f) -------------------------------------------------------------------------------------------------------------------------------
def test_n_zero_leaves_outputs_alone_and_scalars_zero():
    import torch

    lib = _lib()
    a, b, c = (np.arange(4.0) + k for k in range(3))
    at, bt, ct = _dev(a, b, c)
    fresh = lambda: np.full(4, -7.0)
    st = _stream()
    for name, call in [
        ("zf_host_grad_step", lambda o: lib.zf_host_grad_step(_p(o), _p(a), _p(b), 0.5, 0)),
        ("zf_host_momentum", lambda o: lib.zf_host_momentum(_p(o), _p(a), _p(b), 0.5, 0)),
        ("zf_host_prox_l1_box", lambda o: lib.zf_host_prox_l1_box(_p(o), _p(a), 0.5, -1.0, 1.0, 0)),
        ("zf_host_prox_enet_box", lambda o: lib.zf_host_prox_enet_box(_p(o), _p(a), 0.5, 0.5, -1.0, 1.0, 0)),
        ("zf_host_diag_grad", lambda o: lib.zf_host_diag_grad(_p(o), _p(a), _d(bt), _d(ct), 0)),
    ]:
        out = fresh()
        assert call(out) == 0, name
        assert (out == -7.0).all(), name
    for name, call in [("zf_dev_grad_step", lambda o: lib.zf_dev_grad_step(_d(o), _d(at), _d(bt), 0.5, 0, st)),
                       ("zf_dev_momentum", lambda o: lib.zf_dev_momentum(_d(o), _d(at), _d(bt), 0.5, 0, st))]:
        out = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
        assert call(out) == 0, name
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -7.0).all(), name
    out = fresh()
    assert lib.zf_host_model_terms(_p(a), _p(b), _p(c), 0, _p(out)) == 0 and out.tolist() == [0.0, 0.0, 0.0, -7.0]
    out = fresh()
    assert lib.zf_dev_model_terms(_d(at), _d(bt), _d(ct), 0, _p(out), st) == 0 and out.tolist() == [0.0, 0.0, 0.0, -7.0]
    s = C.c_double(-7.0)
    assert lib.zf_host_asum(_p(a), 0, C.byref(s)) == 0 and s.value == 0.0
    s = C.c_double(-7.0)
    assert lib.zf_host_enet_g(_p(a), 0, 0.5, 0.5, C.byref(s)) == 0 and s.value == 0.0


def test_refusals_carry_a_message():
    import torch

    lib = _lib()
    n = 8
    at, bt, ct = _dev(np.ones(n), np.ones(n), np.ones(n))
    Jt = _dev(np.ones((2, n)))
    out3 = torch.full((3,), -7.0, dtype=torch.float64, device="cuda")
    host = np.full(3, -7.0)
    w = np.full(8, 0.125)
    st, null = _stream(), C.c_void_p(None)

    def refused(rc, name):
        msg = lib.zf_last_error().decode(errors="replace")
        assert rc != 0 and name in msg, (name, rc, msg)

    refused(lib.zf_dev_model_terms_async(_d(at), _d(bt), _d(ct), 0, _d(out3), st), "zf_dev_model_terms_async")
    refused(lib.zf_dev_model_terms_async(null, _d(bt), _d(ct), n, _d(out3), st), "zf_dev_model_terms_async")
    refused(lib.zf_dev_model_terms_async(_d(at), _d(bt), _d(ct), n, null, st), "zf_dev_model_terms_async")
    refused(lib.zf_eval_diag_l1(_d(at), _d(bt), _d(ct), 0.5, 0, _p(host), st), "zf_eval_diag_l1")
    refused(lib.zf_eval_diag_l1(_d(at), null, _d(ct), 0.5, n, _p(host), st), "zf_eval_diag_l1")
    refused(lib.zf_eval_diag_l1(_d(at), _d(bt), _d(ct), 0.5, n, null, st), "zf_eval_diag_l1")
    for m, size, first in ((2, 0, _d(at)), (2, n, null), (0, n, _d(at)), (9, n, _d(at))):
        refused(lib.zf_dev_mo_combine(first, _d(bt), _d(Jt), _p(w), 0.5, m, size, _d(out3), st), "zf_dev_mo_combine")
        refused(lib.zf_dev_mo_post_terms(_d(Jt), _d(bt), _d(ct), first, m, size, _d(out3), st), "zf_dev_mo_post_terms")
    refused(lib.zf_host_model_terms(null, _p(host), _p(host), 3, _p(host)), "zf_host_model_terms")
    refused(lib.zf_host_asum(_p(host), -1, C.byref(C.c_double(0.0))), "zf_host_asum")
    torch.cuda.synchronize()
    assert (out3.cpu().numpy() == -7.0).all() and (host == -7.0).all(), "a refused call writes nothing"
    # and the library goes on working
    assert lib.zf_dev_model_terms_async(_d(at), _d(bt), _d(ct), n, _d(out3), st) == 0
    assert out3.cpu().numpy().tolist() == [0.0, 0.0, 0.0]


# ---- (g) -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["host", "tensor"])
def test_one_solve_past_the_grid_cap_against_the_oracle(engine):
    """n = 524288 + 257: every vector kernel of the solve takes a second trip.  lr = 4 is halved three times in the first line
    search (d <= 2).  Element-wise callbacks round like NumPy, so the iterates are the oracle's bit for bit; the weights handed
    to prox_wsum_g are the lr of every trial: the lr and the trial sequences at once."""
    import torch

    from oracle import cpu_ref, problems_ref as P
    from zfista_amd import minimize_proximal_gradient

    n = V.CAP + 257
    assert V.trips(n) == 2
    d, c, lam = P.make_pdiag(n, seed=6)
    kw = dict(lr=4.0, nesterov=True, tol=0.0, max_iter=6, return_all=True)
    ref = P.DiagQuadL1Ref(d, c, lam)
    seen = {"oracle": [], "engine": []}

    def recording(prox, who):
        def wrapped(weight, v):
            seen[who].append(float(weight))
            return prox(weight, v)
        return wrapped

    f, g, jac_f, prox = ref.callbacks()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = cpu_ref.minimize_proximal_gradient(f, g, jac_f, recording(prox, "oracle"), np.zeros(n), **kw)
        if engine == "host":
            res = minimize_proximal_gradient(f, g, jac_f, recording(prox, "engine"), np.zeros(n), **kw)
            x, vecs = res.x, res.allvecs
        else:
            tf, tg, tjac, tprox = _torch_diag(d, c, lam)
            res = minimize_proximal_gradient(tf, tg, tjac, recording(tprox, "engine"),
                                             torch.zeros(n, dtype=torch.float64, device="cuda"), **kw)
            x, vecs = res.x.cpu().numpy(), [v.cpu().numpy() for v in res.allvecs]
    assert res.nit == exp.nit == 6 and res.message == exp.message and res.success == exp.success
    assert exp.alltrials[0] > 1 and exp.alllrs[0] < 4.0 and sum(exp.alltrials) == len(seen["oracle"]), "the first line search must backtrack"
    assert seen["engine"] == seen["oracle"], "lr of every trial"
    accepted = np.cumsum(exp.alltrials) - 1   # the last trial of every line search is the accepted one
    assert [seen["engine"][k] for k in accepted] == [float(lr) for lr in exp.alllrs]
    _same(x, exp.x, "the final iterate")
    _same(vecs[3], exp.allvecs[3], "the third iterate")
    np.testing.assert_allclose(np.asarray(res.allfuns, dtype=float), np.asarray(exp.allfuns, dtype=float), rtol=1e-10, atol=0)
    _same(np.asarray(res.allerrs, dtype=float), np.asarray(exp.allerrs, dtype=float), "allerrs (a maximum has no order)")
