#!/usr/bin/env python3
"""An L1 path of multinomial (softmax) regression: K classes, one resident sparse matrix, every point stopped on its duality gap.

``SparseMultinomialL1(A, y, lam)`` takes the m class labels 0 .. K-1 as they are (or an (m, K) matrix of probabilities); the
coefficients are an (n, K) matrix, ``coef(res.x)``, and ``predict_proba(res.x)`` gives the fitted class probabilities.  The matrix
goes to HBM once: every point of the path is a sibling (``with_lam``) that shares it, warm-started from the point before.  Each sweep
over the matrix serves all K classes.  The one-vs-rest model of the same labels (``SparseMultiResponseLogisticL1``) is fitted beside
it at the last weight for comparison: its K probabilities do not sum to one.

    python examples/multinomial_path.py [--m 20000 --n 2000 --classes 5 --density 0.01 --points 6]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zfista_amd.path import l1_path  # noqa: E402
from zfista_amd.problems import SparseMultinomialL1, SparseMultiResponseLogisticL1  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=20000)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--points", type=int, default=6)
    args = ap.parse_args()
    K = args.classes
    rng = np.random.default_rng(0)
    A = sp.random(args.m, args.n, density=args.density, random_state=rng, data_rvs=rng.standard_normal, format="csr")
    X_true = np.zeros((args.n, K))
    support = rng.choice(args.n, 20, replace=False)
    X_true[support] = 2.0 * rng.standard_normal((20, K))
    y = np.argmax(A @ X_true + rng.gumbel(size=(args.m, K)), axis=1)   # a draw from the softmax model
    prob = SparseMultinomialL1(A, y, 1.0, scale=1.0 / args.m, n_classes=K)
    lam_max = float(prob.lam_max())
    lams = lam_max * np.logspace(0, -1.5, args.points)
    gap_tol = 1e-6 * float(prob.with_lam(lams[-1]).duality_gap(np.zeros(args.n * K)).primal)
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=5000)
    print(f"{args.m} x {args.n}, nnz {A.nnz}, {K} classes with counts {np.bincount(y, minlength=K).tolist()}")
    t0 = time.time()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        path = l1_path(prob, lams, gap_tol=gap_tol, **kw)
    print(f"\npath: lam_max {lam_max:.6g}, gap_tol {gap_tol:.3g}, {time.time() - t0:.2f} s")
    print(f"{'lam / lam_max':>14} {'nit':>6} {'gap':>12} {'rows of X != 0':>15} {'of the true support':>19} {'accuracy':>9}")
    for r in path:
        X = prob.coef(r.x)
        nz = np.flatnonzero(np.any(X != 0, axis=1))
        acc = float(np.mean(np.argmax(prob.predict_proba(r.x, A=A), axis=1) == y))
        print(f"{r.lam / lam_max:14.5f} {r.nit:6d} {r.dual_gap:12.4e} {nz.size:15d} {int(np.isin(nz, support).sum()):19d} {acc:9.4f}")
    # one-vs-rest on the same labels at the last weight
    B = -np.ones((args.m, K))
    B[np.arange(args.m), y] = 1.0
    ovr = SparseMultiResponseLogisticL1(A, B, lams[-1], scale=1.0 / args.m)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = ovr.minimize_proximal_gradient(np.zeros(args.n * K), gap_tol=gap_tol, **kw)
    P1 = 1.0 / (1.0 + np.exp(-(A @ ovr.coef(res.x))))
    Pm = prob.predict_proba(path[-1].x, A=A)
    print(f"\none-vs-rest at the last weight: nit {res.nit}, accuracy {float(np.mean(np.argmax(P1, axis=1) == y)):.4f}; its K "
          f"probabilities sum to {P1.sum(axis=1).min():.3f} .. {P1.sum(axis=1).max():.3f}, the softmax model's to "
          f"{Pm.sum(axis=1).min():.6f} .. {Pm.sum(axis=1).max():.6f}")


if __name__ == "__main__":
    main()
