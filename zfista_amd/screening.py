"""Gap-safe screening for the l1 problems: solve on the columns the duality gap cannot rule out.

A gap evaluation holds everything a gap-safe rule needs - g = grad f(x), alpha and the gap are on the device - so
``problem.screen(x)`` returns, beside the gap, the mask of the columns that may be non-zero at an optimum
(csrc/zf_kernels_screen.h).  The design is restriction, not masking: ``problem.restrict(keep)`` builds, on the device, a
smaller ordinary problem of the same class, and the unchanged solver runs on it.  ``solve_screened`` alternates the two.

A round: (1) screen the FULL problem at the current x; (2) stop when the full gap is at most ``gap_tol``; (3) restrict to
the kept columns - from the original matrix, and only when the kept set is not a subset of the current one or has shrunk
to ``screen_shrink`` times its size - and solve the restricted problem from x[keep] with the solver's own ``gap_tol=``
stopping, down to ``screen_ratio`` times the round's starting gap or to the restricted target; (4) scatter x back.  Every
round screens all n columns afresh, so a column dropped by mistake comes back, and the certificate of the result is the
FULL problem's gap at the returned x - it never depends on the rule having been safe.  When a restricted solve reaches
its target while the full gap stays above ``gap_tol`` the restricted target halves (the two gaps coincide at the optimum).
"""
from __future__ import annotations

import inspect
import time

import numpy as np
from scipy.optimize import OptimizeResult

from .proximal_gradient import _MSG_GAP, _MSG_MAXITER, minimize_proximal_gradient

_MSG_ROUNDS = "Maximum number of screening rounds reached"
_DEFAULT_MAX_ITER = inspect.signature(minimize_proximal_gradient).parameters["max_iter"].default


def solve_screened(problem, x0, gap_tol, screen_ratio=0.1, screen_shrink=0.5, max_rounds=50, **solver_kwargs):
    """Minimise ``problem`` (a ``LeastSquaresL1``, ``SparseLeastSquaresL1``, ``LogisticL1`` or ``SparseLogisticL1`` without
    bounds or a process group) from ``x0`` to a duality gap of at most ``gap_tol`` by rounds of screening and restricted
    solves.  ``solver_kwargs`` go to ``minimize_proximal_gradient`` for every restricted solve (``max_iter`` is the budget
    of the whole call).

    Returns an ``OptimizeResult`` of length n_features: ``x``, ``fun`` = P(x), ``nit`` (summed over the rounds), ``dual_gap``
    (the full problem's gap at ``x``, bit for bit ``problem.duality_gap(x).gap``), ``dual_gap_checks`` (restricted and full
    evaluations), ``success`` / ``status`` / ``message`` and ``screen``: one dict per round with ``nit``, ``gap`` (the full
    gap the round started from), ``kept`` and ``restricted`` (whether a restriction was made in that round)."""
    if not getattr(problem, "has_duality_gap", False):
        raise ValueError("solve_screened needs a LeastSquaresL1, SparseLeastSquaresL1, LogisticL1 or SparseLogisticL1")
    why = problem._screen_refusal()
    if why:
        raise ValueError(f"solve_screened is not available: {why}")
    if solver_kwargs.get("return_all"):
        raise ValueError("solve_screened does not record iterates (return_all): the rounds run on problems of different sizes")
    if gap_tol is None or not gap_tol >= 0:
        raise ValueError(f"gap_tol must be >= 0, got {gap_tol!r}")
    if not (0 < screen_ratio < 1) or not (0 < screen_shrink <= 1) or int(max_rounds) != max_rounds or max_rounds < 1:
        raise ValueError("screen_ratio must lie in (0, 1), screen_shrink in (0, 1] and max_rounds must be an integer >= 1")
    t0 = time.time()
    n = problem.n_features
    x = np.array(np.asarray(x0, dtype=np.float64).reshape(-1), copy=True)
    if x.size != n:
        raise ValueError(f"len(x) should be equal to n_features, got {x}.")
    kw = dict(solver_kwargs)
    budget = int(kw.pop("max_iter", _DEFAULT_MAX_ITER))
    cur, cols = problem, None      # the problem the rounds solve and the columns it holds (None: all)
    target = float(gap_tol)        # the gap the restricted solves aim at
    nit = checks = 0
    rounds, status, message, sc = [], 0, _MSG_ROUNDS, None
    for _ in range(int(max_rounds)):
        sc = problem.screen(x)
        checks += 1
        gap = float(sc.gap.gap)
        if gap <= gap_tol:
            status, message = 1, _MSG_GAP
            break
        if nit >= budget:
            message = _MSG_MAXITER
            break
        mask = sc.keep.cpu().numpy()
        kept = int(sc.count)
        entry = dict(nit=0, gap=gap, kept=kept, restricted=False)
        rounds.append(entry)
        if kept == 0:              # every column is ruled out: the optimum is x = 0 (handled on the host)
            x = np.zeros(n)
            cur, cols = problem, None
            continue
        size = n if cols is None else cols.size
        inside = cols is None or bool(np.isin(np.flatnonzero(mask), cols, assume_unique=True).all())
        if not inside or kept <= screen_shrink * size:
            cols = np.flatnonzero(mask)
            cur = problem.restrict(sc) if kept < n else problem
            cols = cols if kept < n else None
            entry["restricted"] = kept < n
        inner = max(screen_ratio * gap, target)
        res = minimize_proximal_gradient(*cur.callbacks(), x if cols is None else x[cols], gap_tol=inner, max_iter=budget - nit, **kw)
        nit += int(res.nit)
        checks += int(res.get("dual_gap_checks", 0))
        entry["nit"] = int(res.nit)
        if cols is None:
            x = np.asarray(res.x, dtype=np.float64)
        else:
            x = np.zeros(n)
            x[cols] = res.x
        if res.get("dual_gap", np.inf) > inner:
            # the restricted solve ended for a reason of its own (tol, max_iter, a failed line search): that is this solve's end
            sc = None
            status, message = int(res.get("status", 0)), res.message
            break
        if res.dual_gap <= target:
            target *= 0.5          # (the next screen decides; if the full gap is still above gap_tol, aim lower)
    else:
        sc = None                  # max_rounds restricted solves: x has moved since the last screen
    final = sc.gap if sc is not None else problem.duality_gap(x)
    checks += sc is None
    if message == _MSG_ROUNDS and final.gap <= gap_tol:
        status, message = 1, _MSG_GAP
    out = OptimizeResult()
    out.update(x0=x0, x=x, fun=np.float64(final.primal), nit=nit, status=status, message=message, success=bool(status == 1),
               dual_gap=final.gap, dual_gap_checks=checks, screen=rounds, time=time.time() - t0)
    return out
