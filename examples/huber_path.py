#!/usr/bin/env python3
"""A robust regularisation path on data with outliers, beside the least-squares path on the same data.

A tenth of the rows of b carries a gross error.  The squared loss pays for such a row with its square, so the LASSO bends
the coefficients towards it; Huber's loss charges it linearly beyond delta and the path recovers the support of x_true.  The
matrix goes to HBM once per class; every point is a sibling problem (``with_lam``) that shares it, warm-started from the
point before and stopped on its duality gap.

    python examples/huber_path.py [--m 20000 --n 2000 --density 0.01 --points 8]
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
from zfista_amd.problems import SparseHuberL1, SparseLeastSquaresL1  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=20000)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--points", type=int, default=8)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    A = sp.random(args.m, args.n, density=args.density, random_state=rng, data_rvs=rng.standard_normal, format="csr")
    x_true = np.zeros(args.n)
    support = rng.choice(args.n, 20, replace=False)
    x_true[support] = rng.standard_normal(20)
    clean = A @ x_true + 0.01 * rng.standard_normal(args.m)
    b = clean.copy()
    bad = rng.choice(args.m, args.m // 10, replace=False)
    b[bad] += rng.choice([-1.0, 1.0], bad.size) * 5.0 * np.std(clean)
    delta = float(np.median(np.abs(b)))
    probs = {"least squares": SparseLeastSquaresL1(A, b, 1.0), f"huber, delta = {delta:.3g}": SparseHuberL1(A, b, 1.0, delta)}
    print(f"{args.m} x {args.n}, nnz {A.nnz}; {bad.size} rows with an outlier of 5 std(b)")
    for name, prob in probs.items():
        lam_max = float(prob.lam_max())
        lams = lam_max * np.logspace(0, -1.5, args.points)
        gap_tol = 1e-5 * float(prob.with_lam(lams[-1]).duality_gap(np.zeros(args.n)).primal)
        t0 = time.time()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            path = l1_path(prob, lams, gap_tol=gap_tol, lr=1.0, nesterov=True, tol=0.0, max_iter=5000)
        print(f"\n{name}: lam_max {lam_max:.6g}, gap_tol {gap_tol:.3g}, {time.time() - t0:.2f} s")
        print(f"{'lam / lam_max':>14} {'nit':>6} {'gap':>12} {'nonzeros':>9} {'of the true support':>19} {'|x - x_true|_2':>15}")
        for r in path:
            nz = np.flatnonzero(r.x)
            hit = int(np.isin(nz, support).sum())
            print(f"{r.lam / lam_max:14.5f} {r.nit:6d} {r.dual_gap:12.4e} {nz.size:9d} {hit:19d} {np.linalg.norm(r.x - x_true):15.6f}")


if __name__ == "__main__":
    main()
