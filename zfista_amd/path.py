"""Regularisation paths of the l1 problems: one device-resident matrix, a sequence of l1 weights.

A new ``lam`` used to mean a new problem object and a new upload of A.  ``problem.with_lam(lam)`` is a sibling that shares
the device matrix, b and (sparse classes) the matrix handle; ``l1_path`` solves such siblings in order, each warm-started
from the solution before it and stopped on its duality gap - the usual way of solving a LASSO / sparse logistic regression
for a grid of weights from ``problem.lam_max()`` downward (at ``lam_max`` and above the solution is x = 0).
"""
from __future__ import annotations

import numpy as np

from .proximal_gradient import minimize_proximal_gradient


def l1_path(problem, lams, x0=None, gap_tol=1e-6, screen=False, l2=None, **solver_kwargs):
    """Solve ``problem.with_lam(l)`` for each ``l`` of ``lams`` in the order given, each from the solution of the one
    before (the first from ``x0``; default zeros), with ``minimize_proximal_gradient(..., gap_tol=gap_tol, **solver_kwargs)``.
    ``l2``: the ridge weight of an elastic-net path - a scalar, or one value per ``l`` - and the points are
    ``problem.with_penalty(l, l2)``; None (default) keeps the problem's own ``l2``.  Not with ``screen=True`` while ``l2 > 0``.
    ``screen=True``: each point is solved by ``zfista_amd.screening.solve_screened`` instead - gap-safe screening, and solves
    on the kept columns only (``solver_kwargs`` may then carry its ``screen_ratio``, ``screen_shrink`` and ``max_rounds``).

    ``problem``: a ``LeastSquaresL1``, ``SparseLeastSquaresL1``, ``LogisticL1`` or ``SparseLogisticL1`` without bounds or a
    process group; ``gap_tol``: the absolute duality gap every point is solved to (None: the solver's own ``tol`` only).
    Returns the list of results, one per ``l``, each with an extra field ``lam``."""
    if not getattr(problem, "has_duality_gap", False):
        raise ValueError("l1_path needs a LeastSquaresL1, SparseLeastSquaresL1, LogisticL1 or SparseLogisticL1")
    x = np.zeros(problem.n_features) if x0 is None else x0
    lams = list(lams)
    if l2 is None:
        l2s = [None] * len(lams)
    elif np.ndim(l2) == 0:
        l2s = [float(l2)] * len(lams)
    else:
        l2s = [float(v) for v in np.asarray(l2, dtype=np.float64).reshape(-1)]
        if len(l2s) != len(lams):
            raise ValueError(f"l2 must be a scalar or hold one value per lam ({len(lams)}), got {len(l2s)}")
    if screen and any((problem.l2 if v is None else v) > 0 for v in l2s):
        raise ValueError("l1_path(screen=True) is not available with l2 > 0: the gap-safe rule of the elastic net and its rounding "
                         "guard are not built yet")
    out = []
    for lam, ridge in zip(lams, l2s):
        sib = problem.with_lam(lam) if ridge is None else problem.with_penalty(lam, ridge)
        if screen:
            from .screening import solve_screened

            res = solve_screened(sib, x, gap_tol, **solver_kwargs)
        else:
            res = minimize_proximal_gradient(*sib.callbacks(), x, gap_tol=gap_tol, **solver_kwargs)
        res["lam"] = float(lam)
        if sib.l2 > 0:
            res["l2"] = float(sib.l2)
        out.append(res)
        x = res.x
    return out
