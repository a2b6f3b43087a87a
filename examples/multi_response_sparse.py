#!/usr/bin/env python3
"""Several right-hand sides on one resident SPARSE matrix: a multi-output LASSO, a one-vs-rest classifier, and a cross-validation
whose folds are solved in lockstep.

``SparseMultiResponseLeastSquaresL1(A, B, lam)`` with a scipy.sparse ``A`` and ``B`` of shape (m, K) solves the K LASSO problems
of the columns of B as ONE problem on the CSR of A as it is stored: the decision vector is the (n, K) coefficient matrix
flattened in C order, so the K values a stored element needs are contiguous - one index, one value and one gathered cache line
serve K responses.  The alternative before was K solves, or the plain class on ``sp.kron(A, sp.identity(K))``, which stores and
streams K copies of the indices and values; the new class computes, bit for bit, what that one computes.  Part 1 solves such a
problem, the Kronecker form and K plain problems and compares time and solutions.

Part 2: K classes, one-vs-rest, ``SparseMultiResponseLogisticL1``; then ``l1_cv_lockstep`` on a plain ``SparseLogisticL1``: the
folds are responses with 0 / 1 row weights, stopped on the joint duality gap, which certifies every fold.

    python examples/multi_response_sparse.py [--m 20000 --n 50000 --density 0.001 --k 8]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zfista_amd.path import l1_cv_lockstep  # noqa: E402
from zfista_amd.problems import SparseLeastSquaresL1, SparseLogisticL1, SparseMultiResponseLogisticL1  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=20000)
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--density", type=float, default=0.001)
    ap.add_argument("--k", type=int, default=8)
    args = ap.parse_args()
    m, n, K = args.m, args.n, args.k
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(0)
    A = sp.random(m, n, density=args.density, random_state=rng, data_rvs=rng.standard_normal, format="csr")
    X_true = np.zeros((n, K))
    X_true[:20] = rng.standard_normal((20, K))
    Z = A @ X_true
    B = Z + 0.01 * rng.standard_normal((m, K))

    # ---- 1. a multi-output LASSO ----------------------------------------------------------------------------------------------
    plain = SparseLeastSquaresL1(A, B[:, 0].copy(), 1.0)
    multi = plain.with_responses(B)            # shares the matrix handle: only B is uploaded, nothing is planned again
    lam = 0.1 * float(multi.lam_max())
    multi, plain = multi.with_lam(lam), plain.with_lam(lam)
    P0 = float(multi.duality_gap(np.zeros(multi.n_features)).primal)
    kw = dict(lr=1.0, nesterov=True, tol=0.0, max_iter=5000)
    t0 = time.time()
    res = multi.minimize_proximal_gradient(np.zeros((n, K)), gap_tol=1e-6 * P0, **kw)
    t_multi = time.time() - t0
    X = multi.coef(res.x)
    kron = SparseLeastSquaresL1(sp.kron(A, sp.identity(K), format="csr"), B.reshape(-1), lam)
    t0 = time.time()
    res_k = kron.minimize_proximal_gradient(np.zeros(n * K), gap_tol=1e-6 * P0, **kw)
    t_kron = time.time() - t0
    t0 = time.time()
    cols = []
    for k in range(K):
        q = plain.with_responses(B[:, k:k + 1])   # (one response: the plain sparse class, bit for bit)
        cols.append(q.minimize_proximal_gradient(np.zeros(n), gap_tol=1e-6 * P0 / K, **kw).x)
    t_plain = time.time() - t0
    dist = max(np.linalg.norm(X[:, k] - cols[k]) / np.linalg.norm(cols[k]) for k in range(K))
    print(f"multi-output LASSO {m} x {n}, nnz {A.nnz}, K = {K}: one solve {t_multi:.2f} s ({res.nit} iterations, gap {res.dual_gap:.2e}); "
          f"the Kronecker matrix {t_kron:.2f} s, the same bits: {bool(np.array_equal(res.x, res_k.x))}; {K} plain solves {t_plain:.2f} s, "
          f"largest relative distance of a column {dist:.1e}; non-zeros per response {[int(np.count_nonzero(X[:, k])) for k in range(K)]}")

    # ---- 2. one-vs-rest labels, and a lockstep cross-validation ----------------------------------------------------------------
    classes = np.argmax(Z, axis=1)
    Y = np.where(classes[:, None] == np.arange(K)[None, :], 1.0, -1.0)
    ovr = SparseMultiResponseLogisticL1(A, Y, 1.0)
    ovr = ovr.with_lam(0.1 * float(ovr.lam_max()))
    res = ovr.minimize_proximal_gradient(np.zeros(ovr.n_features), lr=1.0, nesterov=True, tol=0.0, max_iter=300)
    pred = np.argmax(A @ ovr.coef(res.x), axis=1)
    print(f"one-vs-rest, {K} classes: training accuracy {np.mean(pred == classes):.3f} after {res.nit} iterations")
    one = SparseLogisticL1(A, Y[:, 0].copy(), 1.0)
    lams = float(one.lam_max()) * np.logspace(-0.3, -1.5, 5)
    P1 = float(one.duality_gap(np.zeros(n)).primal)
    t0 = time.time()
    cv = l1_cv_lockstep(one, lams, folds=5, gap_tol=1e-4 * P1, refit=False, lr=1.0, nesterov=True, tol=0.0, max_iter=3000)
    print(f"l1_cv_lockstep, 5 folds x {len(lams)} weights in {time.time() - t0:.2f} s: lam_best {cv.lam_best:.4g}, lam_1se {cv.lam_1se:.4g}; "
          f"mean held-out loss {np.array2string(cv.mean, precision=4)}")


if __name__ == "__main__":
    main()
