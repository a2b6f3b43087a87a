"""Seeded L1 logistic-regression inputs and NumPy / SciPy-sparse reference closures shared by the logistic tests and their
fixture script (no test in here).

    f(x) = scale sum_i softplus(t_i),  t_i = -b_i (A x)_i,  b_i in {-1, +1};   grad f = scale A^T rho,  rho_i = -b_i sigma(t_i)

The matrices are sparse_cases.make_sparse on its four SMALL shapes (a dense row, a dense column, an empty row and an empty
column), as CSR and as .toarray(); labels sign(A x_true + 0.1 noise); scale 1; lam = 0.1 scale max |A^T (b / 2)| (a tenth of
the smallest lam for which x = 0 is the solution: grad f(0) = -scale A^T b / 2).  From lr = 1 the line search backtracks
5 - 9 times on every case; with scale = 1 / m nothing backtracks.  The inputs were checked on the CPU for equal trial and
lr sequences under two evaluation forms and summation orders (test_oracle_golden_logistic.py keeps that check)."""
import numpy as np
import scipy.sparse as sp

import sparse_cases as S
from oracle import problems_ref as P

SMALL = S.SMALL
TALL = S.TALL


def make_logistic(m, n, density, seed, scale=1.0):
    """(A csr, labels, lam) on the matrix of sparse_cases.make_sparse(m, n, density, seed)."""
    A = S.make_sparse(m, n, density, seed)[0]
    rng = np.random.default_rng(seed + 1000)
    x_true = np.zeros(n)
    k = max(1, min(20, n // 4))
    x_true[:k] = rng.standard_normal(k)
    b = np.sign(A @ x_true + 0.1 * rng.standard_normal(m))
    b[b == 0] = 1.0
    return A, b, 0.1 * scale * np.max(np.abs(A.T @ (b / 2)))


def stable_terms(t):
    """(softplus(t), sigma(t)) from ONE e = exp(-|t|): finite for every finite t."""
    e = np.exp(-np.abs(t))
    return np.maximum(t, 0.0) + np.log1p(e), np.where(t >= 0, 1.0, e) / (1.0 + e)


class LogisticL1Ref:
    """The closures of L1 logistic regression for a dense ndarray or a scipy.sparse A, in the stable form above
    (form="stable") or as np.logaddexp / scipy.special.expit with the loss summed in reverse order (form="library"):
    the second evaluation form of the decision test."""

    def __init__(self, A, b, lam, scale=1.0, bounds=None, form="stable"):
        self.A = sp.csr_matrix(A, dtype=np.float64) if sp.issparse(A) else np.asarray(A, float)
        self.b = np.asarray(b, float)
        self.lam, self.scale = float(lam), float(scale)
        self.bounds = None if bounds is None else (float(bounds[0]), float(bounds[1]))
        self.form = form

    def _t(self, x):
        return -self.b * (self.A @ x)

    def f(self, x):
        t = self._t(x)
        if self.form == "library":
            return self.scale * np.sum(np.logaddexp(0.0, t)[::-1])
        return self.scale * np.sum(stable_terms(t)[0])

    def jac_f(self, x):
        t = self._t(x)
        if self.form == "library":
            from scipy.special import expit

            sig = expit(t)
        else:
            sig = stable_terms(t)[1]
        return self.scale * (self.A.T @ (-self.b * sig))

    def g(self, x):
        if self.bounds is not None and ((x < self.bounds[0]).any() or (x > self.bounds[1]).any()):
            return np.inf
        return self.lam * np.linalg.norm(x, ord=1)

    def prox_wsum_g(self, weight, x):
        x = P.soft_threshold(x, self.lam * weight)
        if self.bounds is not None:
            x = P.clip_box(x, self.bounds[0], self.bounds[1])
        return x

    def callbacks(self):
        return self.f, self.g, self.jac_f, self.prox_wsum_g


# the fixture's solver variants (80 iterations from lr = 1, return_all), on every SMALL case in both storage forms
GOLDEN_VARIANTS = {
    "ista": dict(nesterov=False),
    "fista": dict(nesterov=True, nesterov_ratio=(0, 0.25)),
}
GOLDEN_CASES = [0, 1, 2, 3]
GOLDEN_KW = dict(lr=1, tol=0.0, max_iter=80, return_all=True)
GOLDEN_STRIDE = 7          # stored iterates: every 10th, elements [::GOLDEN_STRIDE]
GOLDEN_FORMS = ("csr", "dense")


def golden_matrix(A, storage):
    return A if storage == "csr" else A.toarray()
