"""GPU: acceptance="remainder" - the sufficient-decrease test of zfista/proximal_gradient.py:303 for the least-squares
classes, evaluated on the Taylor remainder.

For f(x) = scale |A x - b|^2 the remainder R = f(x+) - f(y) - <grad f(y), x+ - y> is exactly scale |A (x+ - y)|^2 =
scale sum_i (s+_i - s_y,i)^2 with s_y = s_k + beta (s_k - s_{k-1}): a sum of squares over margins that are in HBM already.
With F(x_k) and g(x+) cancelled :303 reads  R - |x+ - y|^2 / 2 / lr <= tol_internal  - nothing of the size of F in it.
The residual kernels at x+ have a second instantiation that leaves R beside f(x+) (zf_resid_x_rem_kernel, the chunked
pair behind zf_launch_spmv_resid_x_rem, zf_ls_small_rows_kernel<true>); pack slot 7 carries it to zf_eval_trial.

Three overdetermined problems on which the reference's evaluation drowns in rounding (F ~ 7.7e6, 9e7, 2.9e8):
  D   make_plasso(2048, 512, seed=0, lam_frac=0.01, n_informative=200, noise=100)     dense: small path / MFMA / VALU
  S1  sparse 20000 x 2000, density 0.005, seed 7                                       narrow residual kernels
  S2  sparse 60000 x 3000, density 0.004, seed 11                                      wide residual kernels (m > 32768)
all from lr = 1, FISTA (0, 1/4), x0 = 0.  The checker is the oracle's f_diff= hook fed R + <grad f(y), x+ - y>."""
import ctypes as C
import json
import os
import threading
import warnings
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
BASE = dict(lr=1, tol=0.0, tol_internal=1e-12, max_iter=400, max_backtrack_iter=100, decay_rate=0.5,
            nesterov=True, nesterov_ratio=(0, 0.25), deprecated=False, return_all=False)
# the 400-iteration runs of the cancellation-free test on the CPU oracle: total trials and the final step size
EXPECT = {"D": (412, 2.0 ** -12), "S1": (408, 2.0 ** -8), "S2": (409, 2.0 ** -9)}
EXPECT_NIT_TOL9 = {"D": 179, "S1": 179, "S2": 104}


# ---------------------------------------------------------------------------------------------------------------------
# the problems and their CPU references (computed once, shared, never modified)
# ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _data(name):
    import scipy.sparse as sp

    from oracle import problems_ref as P

    if name == "D":
        A, b, lam = P.make_plasso(2048, 512, seed=0, lam_frac=0.01, n_informative=200, noise=100.0)
        return A, b, lam
    if name == "small":
        return P.make_plasso(512, 1024, seed=0)
    m, n, density, seed = {"S1": (20000, 2000, 0.005, 7), "S2": (60000, 3000, 0.004, 11)}[name]
    # (scipy.sparse.random draws its positions without replacement from m * n candidates: seconds at these shapes, paid once)
    rng = np.random.default_rng(seed)
    S = sp.random(m, n, density=density, random_state=np.random.RandomState(seed), data_rvs=rng.standard_normal).tocsr()
    x_true = np.zeros(n)
    x_true[:300] = rng.standard_normal(300)
    b = S @ x_true + 100.0 * rng.standard_normal(m)
    lam = 0.01 * np.max(np.abs(S.T @ b))
    return S, b, lam


def _ref(name, bounds=None):
    from oracle import problems_ref as P
    from sparse_cases import SparseLeastSquaresL1Ref

    A, b, lam = _data(name)
    if isinstance(A, np.ndarray):
        return P.LeastSquaresL1Ref(A, b, lam, bounds=bounds)

    class _Ref(SparseLeastSquaresL1Ref):
        """... with A^T stored as a CSR matrix of its own (SciPy's product with the transposed view of a CSR matrix scatters)"""

        def jac_f(self, x):
            return (2 * self.scale) * (self.At @ (self.A @ x - self.b))

    ref = _Ref(A, b, lam, bounds=bounds)
    ref.At = ref.A.T.tocsr()
    return ref


def _f_diff(ref):
    """f(x+) - f(y) with the cancellation taken out: R + <grad f(y), x+ - y>, R = scale |A (x+ - y)|^2 (the oracle then
    subtracts the same dot product again: what is left is R and its rounding)."""
    last = [None, None]    # (grad f(y) is the same for every trial of a line search)

    def f_diff(x_new, y):
        if last[0] is not y:
            last[:] = [y, ref.jac_f(y)]
        step = x_new - y
        a = ref.A @ step
        return ref.scale * float(a @ a) + float(last[1] @ step)
    return f_diff


@lru_cache(maxsize=None)
def _oracle(name, tol=0.0, max_iter=400):
    from oracle import cpu_ref

    ref = _ref(name)
    n = ref.A.shape[1]

    def memo(fn, keep=4):
        """The oracle evaluates f and jac_f at the same array objects (x_k, y) several times per trial: the same values,
        computed once (the last `keep` arguments are held, so their ids stay theirs)."""
        seen = []

        def wrapped(x):
            for arg, val in seen:
                if arg is x:
                    return val
            val = fn(x)
            seen.append((x, val))
            del seen[:-keep]
            return val
        return wrapped

    ref.f, ref.jac_f = memo(ref.f), memo(ref.jac_f)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = cpu_ref.minimize_proximal_gradient(*ref.callbacks(), np.zeros(n), lr=1, tol=tol, nesterov=True, max_iter=max_iter,
                                                 return_all=True, f_diff=_f_diff(ref))
    for v in res.allvecs:
        v.setflags(write=False)
    return res


def _prob(name, **kw):
    from zfista_amd.problems import LeastSquaresL1, SparseLeastSquaresL1

    A, b, lam = _data(name)
    return (LeastSquaresL1 if isinstance(A, np.ndarray) else SparseLeastSquaresL1)(A, b, lam, **kw)


def _run(prob, opts=None, acceptance="remainder", chunk=64, stop_after=None, resume=None):
    """One device-resident solve (behind a communicator: the host-driven trial / exchange / decide sequence): trace rows, iterates (return_all), final control block."""
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    o = dict(BASE, **(opts or {}))
    o["acceptance"] = acceptance
    n = prob.n_features
    run = NativeRun(prob, np.zeros(n), o) if resume is None else NativeRun.from_snapshot(prob, resume, o)
    rows = [np.zeros((0, _lib.ZF_TRACE_COLS))]
    passes = 0
    state = None
    while run.status == _lib.ZF_RUNNING:
        if stop_after is not None and state is None:
            if passes >= stop_after:
                state = run.snapshot()
            else:
                rows.append(run.advance(min(16, stop_after - passes)))   # (16 passes: within what one chunk may enqueue)
                passes += 16
                continue
        rows.append(run.advance(chunk))
    ctl = run.solver.ctl
    out = dict(rows=np.concatenate(rows), x=run.solver.get_x(), nit=int(ctl.nit), status=int(ctl.status), lr=ctl.lr, F=ctl.F_old,
               trials=int(ctl.total_trials), mode=int(ctl.accept_mode), state=state,
               allvecs=[np.array(v) for v in run.history()] if o["return_all"] else None)
    run.solver.close()
    return out


def _same(a, b):
    assert (a["nit"], a["status"], a["lr"], a["F"], a["trials"]) == (b["nit"], b["status"], b["lr"], b["F"], b["trials"])
    assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["x"], b["x"])


# ---------------------------------------------------------------------------------------------------------------------
# the inequality in extended precision
# ---------------------------------------------------------------------------------------------------------------------
class _ExactOp:
    """A v and A^T v in np.longdouble for a dense or a CSR matrix (SciPy has no extended-precision sparse product: the row
    sums are np.add.reduceat over the non-empty rows)."""

    def __init__(self, A):
        import scipy.sparse as sp

        self.dense = isinstance(A, np.ndarray)
        if self.dense:
            self.A = A.astype(LD)
        else:
            self.m, self.n = A.shape
            self.fwd = self._plan(sp.csr_matrix(A))
            self.bwd = self._plan(sp.csr_matrix(A.T))

    @staticmethod
    def _plan(M):
        M.sort_indices()
        lens = np.diff(M.indptr)
        rows = np.flatnonzero(lens > 0)
        return M.data.astype(LD), M.indices, M.indptr[:-1][rows], rows, M.shape[0]

    @staticmethod
    def _apply(plan, v):
        data, idx, starts, rows, m = plan
        out = np.zeros(m, LD)
        if len(rows):
            out[rows] = np.add.reduceat(data * v[idx], starts)
        return out

    def mul(self, v):
        return self.A @ v if self.dense else self._apply(self.fwd, v)

    def tmul(self, v):
        return self.A.T @ v if self.dense else self._apply(self.bwd, v)


def _check_every_decision(name, res, tol_internal=1e-12, scale=0.5):
    """R - |x+ - y|^2 / 2 / lr <= tol in np.longdouble at the recorded iterates, for EVERY trial of the run: the accepted
    one of each iteration (x+ recorded) and every rejected one before it (x+ = prox(y - lr grad f(y)) at the larger step
    sizes, formed in extended precision).  Returns the relative margins (R - q) / q of accepted and rejected trials."""
    from oracle import cpu_ref
    from zfista_amd import _lib

    if np.finfo(LD).nmant < 63:
        pytest.skip("needs an extended-precision long double on the host")
    A, b, lam = _data(name)
    op = _ExactOp(A)
    bL = b.astype(LD)
    nit = res["nit"]
    betas = cpu_ref.momentum_sequence(nit + 1)
    lrs, trials = res["rows"][:, _lib.TR_LR], res["rows"][:, _lib.TR_TRIALS].astype(int)
    xs = res["allvecs"]
    acc, rej = [], []
    decisions = 0
    x_prev = xs[0]
    y = xs[0].copy()
    for k in range(1, nit + 1):
        yL = y.astype(LD)
        x_new = xs[k]

        def margin(xp, lr):
            step = xp - yL
            a = op.mul(step)
            R = LD(scale) * np.sum(a * a)
            q = np.sum(step * step) / 2 / LD(lr)
            return R - q, q

        val, q = margin(x_new.astype(LD), lrs[k - 1])
        assert val <= LD(tol_internal), f"iteration {k}: accepted although the test fails in extended precision ({float(val):.3e})"
        acc.append(float(val / q))
        decisions += 1
        if trials[k - 1] > 1:
            grad = 2 * LD(scale) * op.tmul(op.mul(yL) - bL)
            for j in range(1, trials[k - 1]):
                lr = lrs[k - 1] * 2.0 ** j
                v = yL - LD(lr) * grad
                cand = np.sign(v) * np.maximum(np.abs(v) - LD(lam) * LD(lr), 0)
                val, q = margin(cand, lr)
                assert val > LD(tol_internal), f"iteration {k}, lr {lr}: rejected although the test holds in extended precision"
                rej.append(float(val / q))
                decisions += 1
        y = x_new + betas[k - 1] * (x_new - x_prev)   # beta_k: the factor applied after outer iteration k
        x_prev = x_new
    assert decisions == res["trials"], "a decision was left out"
    return max(acc), (min(rej) if rej else np.inf)


# ---------------------------------------------------------------------------------------------------------------------
# 1. across the noise floor
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", [
    ("D", {}),                                              # the fused small-matrix path
    ("D", {"ZF_LS_SMALL": "0"}),                            # the general path, A^T r on the matrix cores
    ("D", {"ZF_LS_SMALL": "0", "ZF_GEMV_MFMA": "0"}),       # ... on the VALU
    ("S1", {}),                                             # narrow residual kernels
    ("S2", {}),                                             # wide ones
])
def test_across_the_noise_floor(name, env, monkeypatch):
    from conftest import rel_err
    from zfista_amd import _lib

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = _prob(name)
    res = _run(prob, dict(return_all=True))
    exp = _oracle(name)
    trials, lr = EXPECT[name]
    print(f"{name} {env}: status {res['status']} nit {res['nit']} trials {res['trials']} lr {res['lr']}")
    assert res["mode"] == _lib.ZF_ACCEPT_REMAINDER
    assert (res["status"], res["nit"], res["trials"], res["lr"]) == (_lib.ZF_MAXITER, 400, trials, lr)
    # the oracle's run of the cancellation-free test: the same line search ...
    assert exp.nit == 400 and sum(exp.alltrials) == trials
    assert list(res["rows"][:, _lib.TR_TRIALS].astype(int)) == list(exp.alltrials)
    assert np.array_equal(res["rows"][:, _lib.TR_LR], np.asarray(exp.alllrs))
    # ... and the same iterates and traces, to the project's bar
    for k in range(0, 401):
        assert rel_err(res["allvecs"][k], exp.allvecs[k]) <= 1e-10, k
    np.testing.assert_allclose(res["rows"][:, _lib.TR_F], exp.allfuns[1:], rtol=1e-10)
    np.testing.assert_allclose(res["rows"][:, _lib.TR_ERR], exp.allerrs, rtol=1e-10, atol=1e-10 * np.max(np.abs(exp.x)))
    acc, rej = _check_every_decision(name, res)
    print(f"{name} {env}: relative margins (R - q) / q: accepted <= {acc:.3f}, rejected >= {rej:.3f}")
    # the reference's evaluation on the same problem: "Backtracking failed", or rejections by rounding noise
    ref = _run(prob, acceptance="reference")
    print(f"{name} {env}: reference mode: status {ref['status']} nit {ref['nit']} trials {ref['trials']} lr {ref['lr']}")
    assert ref["status"] == _lib.ZF_BACKTRACK_FAILED or ref["trials"] > res["trials"]


# ---------------------------------------------------------------------------------------------------------------------
# 2. below the noise floor
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [
    dict(),
    dict(env={"ZF_LS_SMALL": "0"}),
    dict(nesterov=False),
    dict(bounds=(-0.05, 0.08)),
    dict(deprecated=True),
    dict(sparse=0),
])
def test_below_the_noise_floor_both_modes_are_bit_identical(case, monkeypatch):
    """Where the reference's evaluation resolves the test both modes decide alike, and then everything is the same bits:
    f(x+) is the same sum in both instantiations of the kernels."""
    from zfista_amd import _lib
    from zfista_amd.problems import SparseLeastSquaresL1

    c = dict(case)
    for k, v in c.pop("env", {}).items():
        monkeypatch.setenv(k, v)
    bounds = c.pop("bounds", None)
    if "sparse" in c:
        import sparse_cases as SC

        prob = SparseLeastSquaresL1(*SC.make_sparse(*SC.SMALL[c.pop("sparse")]))
    else:
        prob = _prob("small", bounds=bounds)
    opts = dict(max_iter=600, **c)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = _run(prob, opts, acceptance="reference")
        b = _run(prob, opts, acceptance="remainder")
    assert (a["mode"], b["mode"]) == (_lib.ZF_ACCEPT_REFERENCE, _lib.ZF_ACCEPT_REMAINDER)
    assert a["nit"] == 600 and a["trials"] > a["nit"]      # (there is a line search to agree on)
    _same(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 3. a tolerance the reference's evaluation cannot reach
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["D", "S1", "S2"])
def test_tol_1e_9_converges_where_the_oracle_does(name):
    from conftest import rel_err
    from zfista_amd import minimize_proximal_gradient

    # (the oracle's run with tol = 1e-9 is its run with tol = 0 up to the first iteration whose err is below 1e-9: :525)
    full = _oracle(name)
    nit9 = 1 + int(np.flatnonzero(np.asarray(full.allerrs) < 1e-9)[0])
    assert nit9 == EXPECT_NIT_TOL9[name]
    prob = _prob(name)
    res = minimize_proximal_gradient(*prob.callbacks(), np.zeros(prob.n_features), lr=1, tol=1e-9, nesterov=True, max_iter=400,
                                     acceptance="remainder")
    print(f"{name}: nit {res.nit} (oracle {nit9}), success {res.success}, rel_err {rel_err(res.x, full.allvecs[nit9]):.3e}")
    assert res.success and res.nit == nit9 and res["acceptance"] == "remainder"
    assert rel_err(res.x, full.allvecs[nit9]) <= 1e-10
    np.testing.assert_allclose(res.fun, full.allfuns[nit9], rtol=1e-10)


# ---------------------------------------------------------------------------------------------------------------------
# 4. every way of running agrees
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shard", ["columns", "rows"])
def test_one_rank_communicator_is_bit_equal_to_unsharded(shard, monkeypatch):
    import torch

    from zfista_amd.comm import LibComm

    monkeypatch.setenv("ZF_LS_SMALL", "0")     # (the sequence behind a communicator is the general one)
    plain = _run(_prob("D"))
    comm = LibComm(0, 1, LibComm.new_unique_id())
    sharded = _run(_prob("D", group=comm, shard=shard))
    torch.cuda.synchronize()
    comm.close()
    assert sharded["trials"] == EXPECT["D"][0]
    _same(sharded, plain)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("shard", ["columns", "rows"])
def test_thread_ranks_against_the_unsharded_remainder_solve(shard, world, monkeypatch):
    """The library's multi-rank sequence with `world` thread ranks on this GPU, 160 iterations of D (the reference's
    evaluation differs from iteration 120 on and fails at 140): every rank reports the same bits; against the unsharded
    remainder solve the iterates and objective values agree to 1e-10 (the row sums are added in another order), iteration
    count and step sizes exactly - what tests/test_gpu_sharded.py holds the reference mode to."""
    import torch

    from conftest import rel_err
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.comm import LibComm
    from zfista_amd.problems import LeastSquaresL1

    A, b, lam = _data("D")
    m, n = A.shape
    kw = dict(lr=1, tol=0.0, nesterov=True, max_iter=160, return_all=True, acceptance="remainder")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full = minimize_proximal_gradient(*_prob("D").callbacks(), np.zeros(n), **kw)
    comms = LibComm.local_group(world, cap_doubles=8192)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                if shard == "rows":
                    r0, r1 = r * m // world, (r + 1) * m // world
                    lo, hi = 0, n
                    prob = LeastSquaresL1(np.ascontiguousarray(A[r0:r1]), b[r0:r1], lam, group=comms[r], shard="rows")
                else:
                    lo, hi = r * n // world, (r + 1) * n // world
                    prob = LeastSquaresL1(np.ascontiguousarray(A[:, lo:hi]), b, lam, group=comms[r])
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    out[r] = minimize_proximal_gradient(*prob.callbacks(), np.zeros(hi - lo), **kw)
                torch.cuda.current_stream().synchronize()
        except Exception as exc:   # pragma: no cover - reported below
            errs.append(exc)

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    for c_ in comms:
        c_.close()
    assert not errs, errs
    assert all(o is not None for o in out), "a rank thread did not finish"
    for res in out:
        assert res.nit == full.nit == 160 and res.fun == out[0].fun and res["acceptance"] == "remainder"
        assert np.array_equal(np.asarray(res.allerrs), np.asarray(out[0].allerrs)), "ranks must agree bit for bit"
    cat = (lambda vs: vs[0]) if shard == "rows" else np.concatenate
    for k in (1, 40, 119, 120, 140, 160):
        assert rel_err(cat([o.allvecs[k] for o in out]), full.allvecs[k]) <= 1e-10, k
    np.testing.assert_allclose(out[0].allfuns, full.allfuns, rtol=1e-10)


@pytest.mark.parametrize("name,env", [("D", {"ZF_LS_SMALL": "0"}), ("S2", {}), ("D", {})])
def test_snapshot_and_resume_continue_bit_identically(name, env, monkeypatch):
    """A snapshot in the middle of a run of test 1 and its continuation.  The control block carries the mode; beta_next and
    the margins s_k, s_{k-1} the remainder kernels read are rebuilt by the resume code as for every solve: each in the
    order of the kernel that left it (the fused small-matrix path: its rows kernel's one wave per row, not the general row
    sweep - zf_solver_restore).  On all three paths - general dense, sparse, fused small-matrix - the continuation is the
    uninterrupted solve bit for bit, here past the point where the reference's evaluation of the test has stalled and one
    other ulp in a margin can turn a decision."""
    from zfista_amd import _lib

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = _prob(name)
    whole = _run(prob, stop_after=144)        # (144 passes = trials in: beyond where the reference's evaluation fails)
    state = whole["state"]
    saved = _lib.Control.from_buffer_copy(np.asarray(state["control"], dtype=np.uint8).tobytes())
    assert saved.accept_mode == _lib.ZF_ACCEPT_REMAINDER and 100 < saved.nit < 400
    with warnings.catch_warnings():
        warnings.simplefilter("error")        # the same mode: nothing to warn about
        cont = _run(prob, resume=state)
    assert cont["mode"] == _lib.ZF_ACCEPT_REMAINDER
    assert (cont["nit"], cont["status"], cont["lr"], cont["trials"]) == (whole["nit"], whole["status"], whole["lr"], whole["trials"])
    tail = whole["rows"][saved.nit:]
    assert cont["F"] == whole["F"] and np.array_equal(cont["x"], whole["x"]) and np.array_equal(cont["rows"], tail)
    with pytest.warns(UserWarning, match="acceptance='remainder'.*acceptance='reference'"):
        other = _run(prob, dict(max_iter=int(saved.nit) + 2), acceptance="reference", resume=state)
    assert other["mode"] == _lib.ZF_ACCEPT_REFERENCE


def test_two_solves_on_streams_give_the_same_bits():
    from zfista_amd.replicas import solve_on_streams

    prob = _prob("S1")
    kw = dict(lr=1, tol=0.0, nesterov=True, max_iter=150, return_all=True, acceptance="remainder")
    x0 = np.zeros(prob.n_features)
    a, b = solve_on_streams([(prob, x0, kw), (prob, x0, kw)], streams=2)
    assert a.nit == b.nit == 150 and a.fun == b.fun and a["acceptance"] == "remainder"
    assert np.array_equal(a.x, b.x) and np.array_equal(np.asarray(a.allerrs), np.asarray(b.allerrs))
    assert np.array_equal(np.asarray(a.allfuns), np.asarray(b.allfuns))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the kernels, element-wise
# ---------------------------------------------------------------------------------------------------------------------
def _depth(m, wide):
    """Additions a term passes through on its way into the sum (the kernels' fixed orders)."""
    if not wide:       # 1024 threads walk the rows with stride 1024; wave tree (6); 16 wave sums in order
        return -(-m // 1024) + 6 + 15
    chunks = min(max(-(-m // 1024), 1), 1024)
    per = -(-m // chunks)   # 256 threads on a contiguous chunk; wave tree; 4 wave sums; then the chunk sums likewise
    return (-(-per // 256) + 6 + 3) + (-(-chunks // 256) + 6 + 3)


def _remainder_bound(sp_, sk, so, beta, scale, wide):
    """|computed R - R| for IEEE double without contraction, u = 2^-53, first order, doubled (SAFETY = 2 as
    tests/operator_exact.py, nothing else added):
        s_y = s_k + beta (s_k - s_o):   E_y = 2 u |beta (s_k - s_o)| + u |s_y|        (difference, product; sum)
        d   = s+ - s_y:                 E_d = E_y + u |d|
        d^2:                            2 |d| E_d + u d^2
        the sum of m non-negative terms through `depth` additions, and the factor scale: (depth + 1) u sum d^2"""
    sy = sk.astype(LD) + LD(beta) * (sk.astype(LD) - so.astype(LD))
    d = np.abs(sp_.astype(LD) - sy)
    e_y = 2 * U * np.abs(LD(beta) * (sk.astype(LD) - so.astype(LD))) + U * np.abs(sy)
    e_d = e_y + U * d
    exact = LD(scale) * np.sum(d * d)
    bound = LD(scale) * (np.sum(2 * d * e_d + U * d * d) + (_depth(len(sk), wide) + 1) * U * np.sum(d * d))
    return exact, 2.0 * float(bound)


def _eval_R(sp_, sk, so, beta, nesterov, scale, wide):
    from zfista_amd import _lib

    lib = _lib.require_gpu()
    out = C.c_double(np.nan)
    arrs = [np.ascontiguousarray(v, dtype=np.float64) for v in (sp_, sk, so)]
    _lib.check(lib.zf_ls_remainder_eval(*(C.c_void_p(_lib.ptr(v)) for v in arrs), len(sk), float(beta), int(nesterov), float(scale),
                                        int(wide), C.byref(out)), "zf_ls_remainder_eval")
    return out.value


@pytest.mark.parametrize("m", [1, 63, 4096, 32768, 32769, 200000])
def test_the_remainder_kernels_element_wise(m):
    """zf_resid_x_rem_kernel (one workgroup) and the chunked pair on caller-supplied margins against np.longdouble, held to
    the rounding bound of their own arithmetic; margins shaped like a late iterate (s+ - s_y seven orders below |s|)."""
    from conftest import ROOT

    if np.finfo(LD).nmant < 63:
        pytest.skip("needs an extended-precision long double on the host")
    rng = np.random.default_rng(m)
    sk = 50.0 * rng.standard_normal(m)
    so = sk + 1e-4 * rng.standard_normal(m)
    worst = {}
    for wide in (0, 1):
        for nesterov, beta in ((1, 0.8731), (0, 0.0), (1, 0.0)):
            sy = sk + beta * (sk - so) if nesterov else sk
            for amp in (1e-5, 3.0):
                sp_ = sy + amp * rng.standard_normal(m)
                got = _eval_R(sp_, sk, so, beta, nesterov, 0.5, wide)
                exact, bound = _remainder_bound(sp_, sk, so, beta if nesterov else 0.0, 0.5, wide)
                ratio = float(abs(LD(got) - exact)) / bound
                key = f"wide={wide} nesterov={nesterov} beta={beta} amp={amp}"
                worst[key] = ratio
                assert ratio <= 1.0, (key, got, float(exact), bound)
            # s+ = s_y as the kernel rounds it: every difference is 0, so is R
            assert _eval_R(sy, sk, so, beta, nesterov, 0.5, wide) == 0.0
        # ISTA ignores beta and s_{k-1}
        sp_ = sk + 1e-3 * rng.standard_normal(m)
        assert _eval_R(sp_, sk, so, 0.9, 0, 0.5, wide) == _eval_R(sp_, sk, sk, 0.0, 0, 0.5, wide)
    print(f"m = {m}: worst error / bound {max(worst.values()):.3f}")
    # one line per m in profiles/accept_remainder_bounds.jsonl (a line of an earlier run is replaced)
    path = os.path.join(ROOT, "profiles", "accept_remainder_bounds.jsonl")
    line = json.dumps(dict(test="remainder_kernels_element_wise", m=m, worst_error_to_bound=round(max(worst.values()), 4),
                           by_case={k: round(v, 4) for k, v in worst.items()}))
    try:
        old = [ln for ln in open(path).read().splitlines() if ln.strip()] if os.path.exists(path) else []
        keep = [ln for ln in old if json.loads(ln).get("m") != m]
        with open(path, "w") as fh:
            fh.write("\n".join(sorted(keep + [line], key=lambda ln: json.loads(ln)["m"])) + "\n")
    except OSError:   # (a read-only checkout: the figure is printed above)
        pass


def test_the_entry_point_refuses_bad_arguments():
    from zfista_amd import _lib

    lib = _lib.load()
    v = np.zeros(4)
    P, out = C.c_void_p(_lib.ptr(v)), C.c_double()
    assert lib.zf_ls_remainder_eval(None, P, P, 4, 0.0, 0, 0.5, 0, C.byref(out)) == -2 and b"zf_ls_remainder_eval" in lib.zf_last_error()
    assert lib.zf_ls_remainder_eval(P, P, P, 0, 0.0, 0, 0.5, 0, C.byref(out)) == -2
    assert lib.zf_ls_remainder_eval(P, P, P, 4, 0.0, 0, 0.5, 2, C.byref(out)) == -2 and b"wide" in lib.zf_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def _others():
    import scipy.sparse as sp

    from oracle import problems_ref as P
    from zfista_amd.problems import BlurHaarL1, DiagQuadL1, LogisticL1, SparseLogisticL1

    rng = np.random.default_rng(0)
    d, c, lam = P.make_pdiag(1000, seed=1)
    M = rng.standard_normal((40, 64))
    y = np.sign(rng.standard_normal(40))
    k = np.outer([1, 2, 1], [1, 2, 1]) / 16.0
    return {
        "DiagQuadL1": (DiagQuadL1(d, c, lam), 1000),
        "LogisticL1": (LogisticL1(M, y, 0.1), 64),
        "SparseLogisticL1": (SparseLogisticL1(sp.csr_matrix(M), y, 0.1), 64),
        "BlurHaarL1": (BlurHaarL1(k, rng.random((16, 16)), 0.01), 256),
    }


def test_the_mode_is_refused_where_it_does_not_exist(monkeypatch):
    import torch

    from zfista_amd import _lib, minimize_proximal_gradient
    from zfista_amd.engine import DeviceSolver
    from zfista_amd.problems import JOS1

    monkeypatch.delenv("ZF_ACCEPT", raising=False)
    names = "LeastSquaresL1.*SparseLeastSquaresL1"
    options = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=3, max_backtrack_iter=100, nesterov=1, deprecated=0)
    for cls, (prob, n) in _others().items():
        with pytest.raises(ValueError, match=names):
            minimize_proximal_gradient(*prob.callbacks(), np.zeros(n), acceptance="remainder", max_iter=3)
        fields, keep = prob._descriptor()
        with pytest.raises(_lib.ZfError, match="accept_mode"):       # the C level, whatever the caller's language
            DeviceSolver(fields, dict(options, accept_mode=_lib.ZF_ACCEPT_REMAINDER), keepalive=keep)
    with pytest.raises(ValueError, match=names):                       # a multi-objective problem
        JOS1(50, l1_ratios=[0.1, 0.2]).minimize_proximal_gradient(np.zeros(50), acceptance="remainder", max_iter=3)
    ref = _ref("small")
    with pytest.raises(ValueError, match=names):                       # plain NumPy callbacks
        minimize_proximal_gradient(*ref.callbacks(), np.zeros(1024), acceptance="remainder", max_iter=3)
    A = torch.from_numpy(ref.A).cuda()
    bt = torch.from_numpy(ref.b).cuda()
    cbs = (lambda x: 0.5 * torch.sum((A @ x - bt) ** 2), lambda x: ref.lam * torch.sum(torch.abs(x)),
           lambda x: A.T @ (A @ x - bt), lambda w, x: torch.sign(x) * torch.clamp(torch.abs(x) - ref.lam * w, min=0.0))
    with pytest.raises(ValueError, match=names):                       # tensor callbacks
        minimize_proximal_gradient(*cbs, torch.zeros(1024, dtype=torch.float64, device="cuda"), acceptance="remainder", max_iter=3)
    # the least-squares kinds: every value but the three is refused, "resolved" stays refused, "remainder" is taken
    for name in ("small", "S1"):
        prob = _prob(name)
        fields, keep = prob._descriptor()
        for mode in (3, -1, _lib.ZF_ACCEPT_RESOLVED):
            with pytest.raises(_lib.ZfError, match="accept_mode"):
                DeviceSolver(fields, dict(options, accept_mode=mode), keepalive=keep)
        DeviceSolver(fields, dict(options, accept_mode=_lib.ZF_ACCEPT_REMAINDER), keepalive=keep).close()
        with pytest.raises(ValueError, match="separable"):
            minimize_proximal_gradient(*prob.callbacks(), np.zeros(prob.n_features), acceptance="resolved", max_iter=3)


def test_the_environment_falls_back_where_the_problem_has_no_such_mode(monkeypatch):
    from zfista_amd import minimize_proximal_gradient

    monkeypatch.setenv("ZF_ACCEPT", "remainder")
    prob, n = _others()["DiagQuadL1"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = minimize_proximal_gradient(*prob.callbacks(), np.zeros(n), max_iter=20, lr=0.45)
        ls = _prob("small")
        took = minimize_proximal_gradient(*ls.callbacks(), np.zeros(1024), max_iter=20)
    assert "acceptance" not in res and res["overrides"]["ZF_ACCEPT"] == "remainder"
    assert took["acceptance"] == "remainder (from the environment: ZF_ACCEPT)"
