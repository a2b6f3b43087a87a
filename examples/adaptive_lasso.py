#!/usr/bin/env python3
"""The adaptive lasso in two stages on ONE device-resident matrix.

Stage 1 is a plain lasso fit x1.  Stage 2 penalises column j by p_j = 1 / (|x1_j| + eps)^gamma at a smaller l1 weight: columns
the first fit found large are penalised little, columns it set to zero are penalised heavily - less shrinkage bias than the
lasso at the first weight, without the false positives the lasso lets in at the second.  ``problem.with_penalty_factor(p)`` is
a sibling on the same device matrix, b and matrix handle: only the n-vector p is uploaded between the stages.  With p > 0 the
duality-gap certificate exists, so every solve stops on ``gap_tol``.

    python examples/adaptive_lasso.py [--m 5000 --n 20000 --density 0.01 --gamma 1.0 --shrink 0.2]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zfista_amd import minimize_proximal_gradient  # noqa: E402
from zfista_amd.problems import SparseLeastSquaresL1  # noqa: E402


def report(tag, x, x_true, support):
    nz = np.flatnonzero(x)
    err = np.linalg.norm(x - x_true) / np.linalg.norm(x_true)
    print(f"{tag:>14}: {nz.size:5d} nonzeros, {int(np.isin(nz, support).sum()):3d} of the {support.size} true ones, "
          f"{int((~np.isin(nz, support)).sum()):5d} false; |x - x_true| / |x_true| = {err:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=5000)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--shrink", type=float, default=0.2, help="lam of stage 2 over lam of stage 1")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    A = sp.random(args.m, args.n, density=args.density, random_state=rng, data_rvs=rng.standard_normal, format="csr")
    x_true = np.zeros(args.n)
    support = rng.choice(args.n, 30, replace=False)
    x_true[support] = rng.choice([-1.0, 1.0], 30) * (0.5 + rng.random(30))
    b = A @ x_true + 0.1 * rng.standard_normal(args.m)
    prob = SparseLeastSquaresL1(A, b, 1.0)
    lam = 0.05 * float(prob.lam_max())
    stage1 = prob.with_lam(lam)
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=20000)
    gap_tol = 1e-7 * float(stage1.duality_gap(np.zeros(args.n)).primal)
    t0 = time.time()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r1 = minimize_proximal_gradient(*stage1.callbacks(), np.zeros(args.n), gap_tol=gap_tol, **kw)
        # stage 2: the factors from the first fit; eps keeps them finite where x1 = 0 (those columns are penalised lam2 / eps^gamma:
        # out for good).  A column with |x1| = 1 keeps factor 1, so the smaller l1 weight lam2 acts on the survivors alone.
        eps = 1e-3 * float(np.max(np.abs(r1.x)))
        p = 1.0 / (np.abs(r1.x) + eps) ** args.gamma
        lam2 = args.shrink * lam
        stage2 = stage1.with_lam(lam2).with_penalty_factor(p)   # the same device matrix: only p is uploaded
        r2 = minimize_proximal_gradient(*stage2.callbacks(), r1.x, gap_tol=gap_tol, **kw)
        # for comparison: the plain lasso at the smaller weight, which lets false positives in
        r3 = minimize_proximal_gradient(*stage1.with_lam(lam2).callbacks(), r1.x, gap_tol=gap_tol, **kw)
    same = stage2._spmat is stage1._spmat
    print(f"{args.m} x {args.n}, nnz {A.nnz}; lam = 0.05 lam_max = {lam:.5g}; two stages and the comparison solve in {time.time() - t0:.2f} s, "
          f"one upload of A ({'shared handle' if same else 'NOT shared'})")
    report("lasso", r1.x, x_true, support)
    report("adaptive", r2.x, x_true, support)
    report(f"lasso {args.shrink:g} lam", r3.x, x_true, support)
    print(f"gaps: {float(r1.dual_gap):.3g}, {float(r2.dual_gap):.3g}, {float(r3.dual_gap):.3g} (<= {gap_tol:.3g}); iterations {r1.nit}, {r2.nit}, {r3.nit}")


if __name__ == "__main__":
    main()
