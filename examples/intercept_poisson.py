#!/usr/bin/env python3
"""L1 Poisson regression WITH an intercept: a regularisation path on one device-resident matrix.

An intercept is a column of ones that is not penalised: ``add_intercept(A)`` returns the widened matrix and the penalty factors
``[0, 1, ..., 1]``, and ``penalty_factor=`` hands them to the problem - g(x) = lam sum_j p_j |x_j|.  A count model without an
intercept has to explain the base rate with its features; with one, x[0] carries log(base rate) and the l1 weight acts on the
features alone.  An unpenalised column has no duality-gap certificate by scaling (the dual point would need a_0^T theta = 0
exactly), so the path runs with ``gap_tol=None`` and every point stops on the solver's own ``tol``.

    python examples/intercept_poisson.py [--m 20000 --n 2000 --density 0.01 --points 8]
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
from zfista_amd.problems import SparsePoissonL1, add_intercept  # noqa: E402


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
    x_true[support] = 0.5 * rng.standard_normal(20)
    base = np.log(3.0)                                   # the base rate: 3 events per unit of exposure
    t = 0.5 + 1.5 * rng.random(args.m)                   # exposure per row
    counts = rng.poisson(t * np.exp(base + A @ x_true)).astype(np.float64)
    A1, p = add_intercept(A)                             # (m, n + 1) and [0, 1, ..., 1]
    prob = SparsePoissonL1(A1, counts / t, 1.0, sample_weight=t, penalty_factor=p)   # the RATE with exposure as the weight
    lam_max = float(prob.lam_max())                      # the intercept alone is fitted first: the smallest lam with x[1:] = 0
    lams = lam_max * np.logspace(-0.05, -2.0, args.points)
    print(f"{args.m} x {args.n} + intercept, nnz {A1.nnz}; lam_max {lam_max:.6g} (without an intercept it would be "
          f"{float(prob.with_penalty_factor(None).lam_max()):.6g})")
    t0 = time.time()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        path = l1_path(prob, lams, gap_tol=None, lr=1.0, nesterov=True, tol=1e-9, max_iter=20000)
    print(f"{args.points} points: {time.time() - t0:.2f} s on one upload of A\n")
    print(f"{'lam / lam_max':>14} {'intercept':>10} {'nonzeros':>9} {'of the true support':>19} {'iterations':>11}")
    for r in path:
        nz = np.flatnonzero(r.x[1:])
        print(f"{r.lam / lam_max:14.5f} {r.x[0]:10.5f} {nz.size:9d} {int(np.isin(nz, support).sum()):19d} {r.nit:11d}")
    print(f"\nthe true intercept is log 3 = {base:.5f}")


if __name__ == "__main__":
    main()
