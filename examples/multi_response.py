#!/usr/bin/env python3
"""Several right-hand sides on one resident matrix: a multi-output LASSO, and a one-vs-rest classifier cross-validated in lockstep.

``MultiResponseLeastSquaresL1(A, B, lam)`` with B of shape (m, K) solves the K LASSO problems of the columns of B as ONE problem:
the decision vector is the (n, K) coefficient matrix flattened in C order, and both sweeps of a trial multiply A into K columns
while reading A once - K solves for about one solve's HBM traffic (sklearn's ``Lasso.fit(X, Y)`` with 2-D ``Y``).  Part 1 solves
such a problem and K plain problems and compares time and solutions.

Part 2: K classes, one-vs-rest: the labels of class c are +1 on its rows and -1 elsewhere, ``MultiResponseLogisticL1`` fits all K
classifiers at once.  For ONE of them ``l1_cv_lockstep`` then cross-validates the l1 weight with all folds solved together (a fold
is a response with 0 / 1 row weights), stopped on the joint duality gap, which certifies every fold.

    python examples/multi_response.py [--m 2048 --n 8192 --k 8]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zfista_amd.path import l1_cv_lockstep  # noqa: E402
from zfista_amd.problems import LeastSquaresL1, LogisticL1, MultiResponseLogisticL1  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=2048)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--k", type=int, default=8)
    args = ap.parse_args()
    m, n, K = args.m, args.n, args.k
    warnings.simplefilter("ignore")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    A = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
    X_true = torch.zeros(n, K, dtype=torch.float64, device="cuda")
    X_true[:20] = torch.randn(20, K, dtype=torch.float64, device="cuda", generator=gen)
    Z = A @ X_true
    B = (Z + 0.01 * torch.randn(m, K, dtype=torch.float64, device="cuda", generator=gen)).cpu().numpy()

    # ---- 1. a multi-output LASSO ----------------------------------------------------------------------------------------------
    plain = LeastSquaresL1(A, B[:, 0].copy(), 1.0)
    multi = plain.with_responses(B)            # shares the device matrix: only B is uploaded
    lam = 0.1 * float(multi.lam_max())
    multi, plain = multi.with_lam(lam), plain.with_lam(lam)
    P0 = float(multi.duality_gap(np.zeros(multi.n_features)).primal)
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=5000)
    t0 = time.time()
    res = multi.minimize_proximal_gradient(np.zeros((n, K)), gap_tol=1e-6 * P0, **kw)
    t_multi = time.time() - t0
    X = multi.coef(res.x)
    t0 = time.time()
    cols = []
    for k in range(K):
        q = LeastSquaresL1(A, B[:, k].copy(), lam)
        cols.append(q.minimize_proximal_gradient(np.zeros(n), gap_tol=1e-6 * P0 / K, **kw).x)
    t_plain = time.time() - t0
    dist = max(np.linalg.norm(X[:, k] - cols[k]) / np.linalg.norm(cols[k]) for k in range(K))
    print(f"multi-output LASSO {m} x {n}, K = {K}: one solve {t_multi:.2f} s ({res.nit} iterations, gap {res.dual_gap:.2e}), "
          f"{K} plain solves {t_plain:.2f} s; largest relative distance of a column {dist:.1e}; "
          f"non-zeros per response {[int(np.count_nonzero(X[:, k])) for k in range(K)]}")

    # ---- 2. one-vs-rest labels, and a lockstep cross-validation ----------------------------------------------------------------
    classes = torch.argmax(Z, dim=1).cpu().numpy()
    Y = np.where(classes[:, None] == np.arange(K)[None, :], 1.0, -1.0)
    ovr = MultiResponseLogisticL1(A, Y, 1.0)
    ovr = ovr.with_lam(0.1 * float(ovr.lam_max()))
    res = ovr.minimize_proximal_gradient(np.zeros(ovr.n_features), lr=1.0, nesterov=True, tol=0.0, max_iter=300)
    pred = np.argmax((A @ torch.from_numpy(ovr.coef(res.x)).cuda()).cpu().numpy(), axis=1)
    print(f"one-vs-rest, {K} classes: training accuracy {np.mean(pred == classes):.3f} after {res.nit} iterations")
    one = LogisticL1(A, Y[:, 0].copy(), 1.0)
    lams = float(one.lam_max()) * np.logspace(-0.3, -1.5, 5)
    P1 = float(one.duality_gap(np.zeros(n)).primal)
    t0 = time.time()
    cv = l1_cv_lockstep(one, lams, folds=5, gap_tol=1e-4 * P1, refit=False, lr=1.0, nesterov=True, tol=0.0, max_iter=3000)
    print(f"l1_cv_lockstep, 5 folds x {len(lams)} weights in {time.time() - t0:.2f} s: lam_best {cv.lam_best:.4g}, lam_1se {cv.lam_1se:.4g}; "
          f"mean held-out loss {np.array2string(cv.mean, precision=4)}")


if __name__ == "__main__":
    main()
