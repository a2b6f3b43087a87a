"""CPU: acceptance="remainder" without a GPU - the decision (zf_decide_host with accept_mode = ZF_ACCEPT_REMAINDER) and
the keyword check.

Pack slot 7 carries the Taylor remainder R = f(x+) - f(y) - <grad f(y), x+ - y> (least squares: scale |A (x+ - y)|^2).
zfista/proximal_gradient.py:303 with F(x_k) and g(x+) cancelled reads R - |x+ - y|^2 / 2 / lr <= tol_internal; :301
(deprecated) reads R <= g(x+) + |x+ - y|^2 / 2 / lr + tol_internal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from zfista_amd import _lib

REM = 2


def _ctl(**kw):
    c = _lib.Control()
    c.lr, c.tol, c.tol_internal, c.decay_rate = 1.0, 1e-5, 1e-12, 0.5
    c.max_iter, c.max_backtrack, c.world, c.F_old = 100, 3, 1, 10.0
    c.accept_mode = REM
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _decide(c, pack):
    lib = _lib.load()
    trace = np.zeros((_lib.ZF_RING, _lib.ZF_TRACE_COLS))
    p = np.ascontiguousarray(np.asarray(pack, float))
    _lib.check(lib.zf_decide_host(C.byref(c), C.sizeof(c), C.c_void_p(_lib.ptr(p)), C.c_void_p(_lib.ptr(trace))))
    return trace


def test_the_constant_is_the_headers():
    src = open(os.path.join(ROOT, "include", "zfista_hip.h")).read()
    m = re.search(r"^#define\s+ZF_ACCEPT_REMAINDER\s+(\d+)\s*$", src, flags=re.M)
    assert m and int(m.group(1)) == _lib.ZF_ACCEPT_REMAINDER == REM
    assert _lib.ACCEPT_MODES == {"reference": 0, "resolved": 1, "remainder": 2}
    assert "zf_ls_remainder_eval" in _lib.SIGNATURES


def test_a_small_remainder_is_accepted_where_the_difference_of_F_would_reject():
    # pack: f_y, dot, ss, g_x, f_x, err, stamp, R.   The reference's test on this pack: F_x - F_old = 10.5 - 10 = 0.5 against
    # fun = (-2 + 1) + 0.5 + (10 - 10) = -0.5 -> rejected (tests/test_host_logic.py).  R = 0.25 <= ss / 2 / lr = 0.5 -> accepted
    pack = [10.0, -2.0, 1.0, 1.0, 9.5, 0.5, 0, 0.25]
    c = _ctl(accept_mode=0)
    _decide(c, pack)
    assert (c.nit, c.trial, c.lr) == (0, 1, 0.5)
    c = _ctl()
    tr = _decide(c, pack)
    assert (c.nit, c.trial, c.lr, c.status) == (1, 0, 1.0, _lib.ZF_RUNNING)
    # what is reported is untouched by the mode: F(x+) = f(x+) + g(x+), the model value in the reference's order
    assert c.F_old == 10.5 and tr[0, _lib.TR_F] == 10.5 and tr[0, _lib.TR_FX] == 9.5
    assert tr[0, _lib.TR_FUN] == (-2.0 + 1.0) + np.sqrt(1.0) ** 2 / 2 / 1.0 + (10.0 - 10.0)


def test_a_large_remainder_is_rejected_although_F_decreases():
    # F_x = 9 < F_old = 10 and the reference's test accepts (test_host_logic); R = 0.75 > 0.5 + tol -> rejected, lr decays
    pack = [10.2, -2.0, 1.0, 1.0, 8.0, 0.5, 0, 0.75]
    c = _ctl(accept_mode=0)
    _decide(c, pack)
    assert c.nit == 1
    c = _ctl()
    _decide(c, pack)
    assert (c.nit, c.trial, c.lr, c.need_grad, c.F_old) == (0, 1, 0.5, 0, 10.0)
    _decide(c, pack)   # (the same sums at lr = 0.5: 0.75 <= 1 / 2 / 0.5 = 1 -> accepted at the second step size)
    assert c.nit == 1 and c.lr == 0.5 and c.total_trials == 2


def test_the_boundary_is_tol_internal():
    # R - ss / 2 / lr <= tol_internal, not-strict
    c = _ctl(tol_internal=0.125)
    _decide(c, [0.0, 0.0, 1.0, 0.0, 0.0, 0.5, 0, 0.625])
    assert c.nit == 1
    c = _ctl(tol_internal=0.125)
    _decide(c, [0.0, 0.0, 1.0, 0.0, 0.0, 0.5, 0, 0.625 + 2.0 ** -50])
    assert c.nit == 0
    c = _ctl()
    _decide(c, [0.0, 0.0, 1.0, 0.0, 0.0, 0.5, 0, np.nan])   # NaN never satisfies <=
    assert c.nit == 0 and c.trial == 1


def test_the_deprecated_inequality_keeps_g():
    # :301  R <= g(x+) + ss / 2 / lr + tol: 1.25 <= 1 + 0.5 accepted; without g(x+) it would not be
    pack = [10.0, -2.0, 1.0, 1.0, 9.5, 0.5, 0, 1.25]
    c = _ctl(deprecated=1)
    _decide(c, pack)
    assert c.nit == 1 and c.fun == (-2.0 + 1.0) + 0.5
    c = _ctl(deprecated=0)
    _decide(c, pack)
    assert c.nit == 0
    c = _ctl(deprecated=1)
    _decide(c, pack[:7] + [1.75])
    assert c.nit == 0 and c.lr == 0.5


def test_decay_rate_one_accepts_and_an_infinite_F_old_does_not():
    c = _ctl(decay_rate=1.0)
    _decide(c, [0.0, 0.0, 0.0, 0.0, 99.0, 1.0, 0, 1e300])
    assert c.nit == 1
    # F(x_k) = inf: the reference's expression accepts everything (-inf <= -inf); this mode still tests the smooth part
    c = _ctl(F_old=np.inf)
    _decide(c, [1.0, 0.0, 1.0, 0.0, 5.0, 1.0, 0, 0.75])
    assert c.nit == 0
    c = _ctl(F_old=np.inf)
    _decide(c, [1.0, 0.0, 1.0, 0.0, 5.0, 1.0, 0, 0.25])
    assert c.nit == 1


def test_packs_of_several_ranks_are_summed_in_rank_order_slot_7_included():
    # three ranks; 0.1 + 0.2 + 0.3 in rank order is 0.6000000000000001, in another order 0.6: the boundary tells which ran
    r = [0.1, 0.2, 0.3]
    in_order = (r[0] + r[1]) + r[2]
    assert in_order != r[0] + (r[1] + r[2])
    packs = []
    for k in range(3):
        packs += [0.0, 0.0, 0.0, 0.0, 1.0, 0.25 * (k + 1), 0, r[k]]
    c = _ctl(world=3, tol_internal=in_order)      # ss = 0: R <= tol_internal exactly
    tr = _decide(c, packs)
    assert c.nit == 1 and tr[0, _lib.TR_ERR] == 0.75 and tr[0, _lib.TR_FX] == 3.0
    c = _ctl(world=3, tol_internal=r[0] + (r[1] + r[2]))
    _decide(c, packs)
    assert c.nit == 0


def _numpy_lasso():
    rng = np.random.default_rng(0)
    A, b = rng.standard_normal((8, 5)), rng.standard_normal(8)
    f = lambda x: 0.5 * np.sum((A @ x - b) ** 2)                                # noqa: E731
    g = lambda x: 0.1 * np.sum(np.abs(x))                                       # noqa: E731
    jac = lambda x: A.T @ (A @ x - b)                                           # noqa: E731
    prox = lambda w, x: np.sign(x) * np.maximum(np.abs(x) - 0.1 * w, 0.0)        # noqa: E731
    return f, g, jac, prox


def test_the_keyword_is_refused_for_plain_callables(monkeypatch):
    from zfista_amd import minimize_proximal_gradient

    monkeypatch.delenv("ZF_ACCEPT", raising=False)
    with pytest.raises(ValueError, match="LeastSquaresL1.*SparseLeastSquaresL1"):
        minimize_proximal_gradient(*_numpy_lasso(), np.zeros(5), acceptance="remainder", max_iter=3)
    with pytest.raises(ValueError, match="acceptance must be 'reference' or 'resolved'"):
        minimize_proximal_gradient(*_numpy_lasso(), np.zeros(5), acceptance="exact", max_iter=3)


def test_the_classes_that_have_the_mode():
    from zfista_amd import problems

    have = {c.__name__ for c in vars(problems).values()
            if isinstance(c, type) and getattr(c, "taylor_remainder", False)}
    assert have == {"LeastSquaresL1", "SparseLeastSquaresL1"}
