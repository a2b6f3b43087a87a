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
    if screen and getattr(problem, "sample_weight", None) is not None:
        raise ValueError("l1_path(screen=True) is not available with sample_weight: the weighted screening rule needs "
                         "sum_i w_i a_ij^2 for |a_j|^2 and a re-derived rounding guard, which are not built yet")
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


def cv_fold_ids(m, folds, seed=0):
    """The fold number of each of ``m`` rows.  ``folds``: an int K >= 2 - ``p = numpy.random.default_rng(seed).permutation(m)``
    and fold k takes the rows ``p[k::K]`` - or an integer array of m fold numbers, used as given."""
    if np.ndim(folds) == 0:
        K = int(folds)
        if K != folds or K < 2 or K > m:
            raise ValueError(f"folds must be an integer in [2, m = {m}] or an array of m fold numbers, got {folds!r}")
        perm = np.random.default_rng(seed).permutation(m)
        ids = np.empty(m, dtype=np.int64)
        for k in range(K):
            ids[perm[k::K]] = k
        return ids
    ids = np.asarray(folds)
    if ids.dtype.kind not in "iu" or ids.shape != (m,):
        raise ValueError(f"fold numbers must be an integer array of m = {m} values, got dtype {ids.dtype}, shape {ids.shape}")
    return ids.astype(np.int64)


class L1CV:
    """What ``l1_cv`` returns: ``lams``, ``fold_ids`` (m), ``folds`` (the fold numbers, in the order of the rows of ``scores``),
    ``scores`` and ``nnz`` (K x L: the held-out loss per unit of held-out weight, and the number of non-zeros, of fold k at
    ``lams[l]``), ``mean`` and ``se`` (over the folds: the mean and its standard error, ``std(ddof=1) / sqrt(K)``), ``best``
    (the index of the smallest mean; the first, i.e. the largest lam of the order given, on a tie), ``lam_best``, ``lam_1se``
    (the largest lam whose mean is <= ``mean[best] + se[best]``), ``path`` (``l1_path`` on all rows at ``lams``, or None) and
    ``paths`` (the K fold paths when asked for, else None) and, with them, ``problems`` (the K training siblings and, last, the
    problem of ``path``: all on one device matrix)."""

    __slots__ = ("lams", "fold_ids", "folds", "scores", "nnz", "mean", "se", "best", "lam_best", "lam_1se", "path", "paths", "problems")

    def __repr__(self):
        return f"L1CV(lam_best={self.lam_best!r}, lam_1se={self.lam_1se!r}, folds={len(self.folds)}, lams={len(self.lams)})"


def cv_summary(lams, scores):
    """(mean, se, best, lam_best, lam_1se) of a K x L score table: see ``L1CV``."""
    lams = np.asarray(lams, dtype=np.float64)
    scores = np.asarray(scores, dtype=np.float64)
    K = scores.shape[0]
    mean = scores.mean(axis=0)
    se = scores.std(axis=0, ddof=1) / np.sqrt(K) if K > 1 else np.zeros_like(mean)
    best = int(np.argmin(mean))
    lam_1se = float(lams[mean <= mean[best] + se[best]].max())
    return mean, se, best, float(lams[best]), lam_1se


def l1_cv(problem, lams, folds=5, seed=0, x0=None, gap_tol=1e-6, refit=True, return_paths=False, **solver_kwargs):
    """K-fold cross-validation of the l1 weight on ONE resident matrix: a fold is the same device matrix with 0 / 1 row
    weights (``problem.with_sample_weight``), so nothing but K pairs of m-vectors is uploaded.

    ``folds``: an int K, or an integer array of m fold numbers (``cv_fold_ids``).  For each fold number k the training
    weights are ``w_base * (ids != k)`` (``w_base``: the problem's own ``sample_weight``, or ones) and ``l1_path`` runs on that
    sibling over ``lams`` (warm-started along the path from ``x0``; ``gap_tol`` and ``solver_kwargs`` as in ``l1_path``;
    ``gap_tol=None`` is allowed).  The score of each point is the unpenalised loss on the held-out rows per unit of held-out
    weight, ``with_sample_weight(w_base * (ids == k)).f(x) / sum(w_base[ids == k])``.  Every fold must leave positive training
    weight and hold positive weight itself.  ``refit``: also solve the path on all rows (``path``).  Returns an ``L1CV``.
    The folds run one after the other; there is no intercept; screening is not available with weights."""
    if not getattr(problem, "has_duality_gap", False) or not hasattr(problem, "with_sample_weight"):
        raise ValueError("l1_cv needs one of the margins classes (LeastSquaresL1, SparseLeastSquaresL1, LogisticL1, "
                         "SparseLogisticL1, HuberL1, SparseHuberL1, PoissonL1, SparsePoissonL1)")
    if solver_kwargs.get("screen"):
        raise ValueError("l1_cv(screen=True) is not available: a fold is a sample_weight sibling, and the weighted screening rule "
                         "is not built yet")
    lams = [float(v) for v in lams]
    if not lams:
        raise ValueError("lams must hold at least one value")
    m = problem.m_rows
    ids = cv_fold_ids(m, folds, seed)
    base = problem.sample_weight
    w_base = np.ones(m) if base is None else base
    labels = [int(k) for k in np.unique(ids)]
    if len(labels) < 2:
        raise ValueError("l1_cv needs at least two folds")
    for k in labels:   # (before any solve)
        if not np.any(w_base * (ids != k) > 0):
            raise ValueError(f"fold {k} leaves no training weight: every row with a positive weight lies in it")
    for k in labels:
        if not np.any(w_base * (ids == k) > 0):
            raise ValueError(f"fold {k} holds no weight: no held-out row to score on")
    scores = np.empty((len(labels), len(lams)))
    nnz = np.zeros((len(labels), len(lams)), dtype=np.int64)
    paths, sibs = [], []
    for r, k in enumerate(labels):
        w_test = w_base * (ids == k)
        train = problem.with_sample_weight(w_base * (ids != k))
        test = problem.with_sample_weight(w_test)
        wsum = w_test.sum()
        path = l1_path(train, lams, x0=x0, gap_tol=gap_tol, **solver_kwargs)
        for l, res in enumerate(path):
            scores[r, l] = test.f(res.x) / wsum
            nnz[r, l] = int(np.count_nonzero(res.x))
        if return_paths:
            paths.append(path)
            sibs.append(train)
    out = L1CV()
    out.lams = np.asarray(lams, dtype=np.float64)
    out.fold_ids, out.folds = ids, labels
    out.scores, out.nnz = scores, nnz
    out.mean, out.se, out.best, out.lam_best, out.lam_1se = cv_summary(lams, scores)
    out.path = l1_path(problem, lams, x0=x0, gap_tol=gap_tol, **solver_kwargs) if refit else None
    out.paths = paths if return_paths else None
    out.problems = sibs + [problem] if return_paths else None
    return out


def l1_cv_lockstep(problem, lams, folds=5, seed=0, x0=None, gap_tol=1e-6, refit=True, **solver_kwargs):
    """``l1_cv`` with all folds solved TOGETHER: the K folds of a ``LeastSquaresL1`` / ``LogisticL1`` (dense) or a
    ``SparseLeastSquaresL1`` / ``SparseLogisticL1`` are the K responses
    of one ``problem.with_responses(B, W)`` - B holds b in every column, ``W[:, k] = w_base * (ids != k)`` - and one ``l1_path``
    over ``lams`` solves them in lockstep, every sweep reading the matrix once for all folds (K <= 16 folds).

    Fold numbers (``cv_fold_ids``), scores (the held-out loss per unit of held-out weight, taken with the plain class's
    ``with_sample_weight(w_base * (ids == k)).f``) and the summary (``cv_summary``) are ``l1_cv``'s; so is the returned ``L1CV``
    (``paths`` holds the one joint path, ``problems`` the joint problem and ``problem``; ``path`` is the plain refit on all rows
    when ``refit``).

    Stopping: the joint problem is stopped on ITS duality gap.  Its dual point scales the candidates of all folds by one alpha -
    the smallest any fold needs - so it is feasible for every fold, and the joint gap is the sum of the K non-negative gaps of
    the folds at that point: ``gap_tol`` on the joint gap certifies every fold to ``gap_tol``.  (A fold's own certificate, with
    its own alpha, is at most that.)  The folds share one step size and one stopping time, so a fold is solved at least as far
    as ``l1_cv`` would solve it, not to the same iterate.  ``gap_tol=None`` is refused: without the certificate nothing says when
    the slowest fold is done."""
    from .problems import MAX_RESPONSES, LeastSquaresL1, LogisticL1, SparseLeastSquaresL1, SparseLogisticL1

    if not isinstance(problem, (LeastSquaresL1, LogisticL1, SparseLeastSquaresL1, SparseLogisticL1)):
        raise ValueError("l1_cv_lockstep needs a dense LeastSquaresL1 or LogisticL1, or a SparseLeastSquaresL1 or SparseLogisticL1 (the "
                         "K-response sweeps read a dense fp64 matrix or a CSR matrix, under the squared or the logistic loss)")
    if gap_tol is None:
        raise ValueError("l1_cv_lockstep needs gap_tol: the joint duality gap is what certifies every fold (use l1_cv for gap_tol=None)")
    if solver_kwargs.get("screen"):
        raise ValueError("l1_cv_lockstep(screen=True) is not available: the K-response problem has no screening")
    lams = [float(v) for v in lams]
    if not lams:
        raise ValueError("lams must hold at least one value")
    m, n = problem.m_rows, problem.n_features
    ids = cv_fold_ids(m, folds, seed)
    base = problem.sample_weight
    w_base = np.ones(m) if base is None else base
    labels = [int(k) for k in np.unique(ids)]
    K = len(labels)
    if K < 2:
        raise ValueError("l1_cv_lockstep needs at least two folds")
    if K > MAX_RESPONSES:
        raise ValueError(f"l1_cv_lockstep runs at most {MAX_RESPONSES} folds at once (one response each), got {K}")
    for k in labels:   # (before anything is uploaded)
        if not np.any(w_base * (ids != k) > 0):
            raise ValueError(f"fold {k} leaves no training weight: every row with a positive weight lies in it")
    for k in labels:
        if not np.any(w_base * (ids == k) > 0):
            raise ValueError(f"fold {k} holds no weight: no held-out row to score on")
    W = np.stack([w_base * (ids != k) for k in labels], axis=1)
    b = problem.b.detach().cpu().numpy()
    joint = problem.with_responses(np.repeat(b.reshape(m, 1), K, axis=1), sample_weight=W)
    if x0 is None:
        start = np.zeros(n * K)
    else:
        start = np.asarray(x0, dtype=np.float64)
        start = np.repeat(start.reshape(n, 1), K, axis=1).reshape(-1) if start.shape == (n,) else start.reshape(-1)
    path = l1_path(joint, lams, x0=start, gap_tol=gap_tol, **solver_kwargs)
    scores = np.empty((K, len(lams)))
    nnz = np.zeros((K, len(lams)), dtype=np.int64)
    for r, k in enumerate(labels):
        w_test = w_base * (ids == k)
        test = problem.with_sample_weight(w_test)
        wsum = w_test.sum()
        for l, res in enumerate(path):
            xk = np.ascontiguousarray(joint.coef(res.x)[:, r])
            scores[r, l] = test.f(xk) / wsum
            nnz[r, l] = int(np.count_nonzero(xk))
    out = L1CV()
    out.lams = np.asarray(lams, dtype=np.float64)
    out.fold_ids, out.folds = ids, labels
    out.scores, out.nnz = scores, nnz
    out.mean, out.se, out.best, out.lam_best, out.lam_1se = cv_summary(lams, scores)
    out.path = l1_path(problem, lams, x0=x0, gap_tol=gap_tol, **solver_kwargs) if refit else None
    out.paths = [path]   # (the one joint path: res.x holds the K fold solutions as the columns of joint.coef(res.x))
    out.problems = [joint, problem]
    return out
