"""Seeded sparse LASSO inputs and SciPy-sparse reference closures shared by the sparse tests and their fixture script
(no test in here).  The shapes and seeds were checked on the CPU for equal accept / reject sequences under two summation
orders (SciPy-sparse closures against the dense oracle class) before they were fixed."""
import numpy as np
import scipy.sparse as sp

from oracle import problems_ref as P

# (m, n, density, seed): the four small cases
SMALL = [(300, 1000, 0.02, 1), (2000, 5000, 0.01, 2), (1000, 257, 0.05, 3), (64, 4099, 0.03, 4)]
# a tall case: more rows than one workgroup walks (the residual kernels take many), a column of 39 999 > 2 x the split threshold
TALL = (40000, 500, 0.004, 5)
BIG = (200_000, 1_000_003, 8, 7)


def make_sparse(m, n, density, seed):
    """Small cases: a dense row, a dense column, an empty row and an empty column."""
    rng = np.random.default_rng(seed)
    A = sp.random(m, n, density=density, random_state=rng, data_rvs=rng.standard_normal, format="lil")
    A[m // 3, :] = rng.standard_normal(n)
    A[:, n // 5] = rng.standard_normal(m).reshape(-1, 1)
    A = A.tocsr().tolil()
    A[m // 2, :] = 0
    A[:, n // 2] = 0
    A = A.tocsr()
    A.eliminate_zeros()
    A.sum_duplicates()
    A.sort_indices()
    x_true = np.zeros(n)
    k = max(1, min(20, n // 4))
    x_true[:k] = rng.standard_normal(k)
    b = A @ x_true + 0.01 * rng.standard_normal(m)
    return A, b, 0.1 * np.max(np.abs(A.T @ b))


def make_sparse_big(m, n, per_col, seed):
    """Large case: per_col draws per column, duplicates summed."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, m, n * per_col)
    cols = np.repeat(np.arange(n), per_col)
    A = sp.csr_matrix((rng.standard_normal(n * per_col), (rows, cols)), shape=(m, n))
    A.sum_duplicates()
    A.sort_indices()
    x_true = np.zeros(n)
    x_true[rng.choice(n, 200, replace=False)] = rng.standard_normal(200)
    b = A @ x_true + 0.01 * rng.standard_normal(m)
    return A, b, 0.1 * np.max(np.abs(A.T @ b))


class SparseLeastSquaresL1Ref:
    """oracle.problems_ref.LeastSquaresL1Ref with a scipy.sparse A: the same expressions, SciPy's summation order."""

    def __init__(self, A, b, lam, scale=0.5, bounds=None):
        self.A = sp.csr_matrix(A, dtype=np.float64)
        self.b = np.asarray(b, float)
        self.lam, self.scale = float(lam), float(scale)
        self.bounds = None if bounds is None else (float(bounds[0]), float(bounds[1]))

    def f(self, x):
        return self.scale * np.linalg.norm(self.A @ x - self.b) ** 2

    def g(self, x):
        if self.bounds is not None and ((x < self.bounds[0]).any() or (x > self.bounds[1]).any()):
            return np.inf
        return self.lam * np.linalg.norm(x, ord=1)

    def jac_f(self, x):
        return (2 * self.scale) * (self.A.T @ (self.A @ x - self.b))

    def prox_wsum_g(self, weight, x):
        x = P.soft_threshold(x, self.lam * weight)
        if self.bounds is not None:
            x = P.clip_box(x, self.bounds[0], self.bounds[1])
        return x

    def callbacks(self):
        return self.f, self.g, self.jac_f, self.prox_wsum_g


# the fixture's solver variants (80 iterations from lr = 1, return_all)
GOLDEN_VARIANTS = {
    "ista": dict(nesterov=False),
    "fista": dict(nesterov=True, nesterov_ratio=(0, 0.25)),
    "fista_ab": dict(nesterov=True, nesterov_ratio=(0.5, 1 / 16)),
}
GOLDEN_CASES = [0, 1, 3]   # indices into SMALL: "cases 1, 2, 4"
GOLDEN_KW = dict(lr=1, tol=0.0, max_iter=80, return_all=True)
GOLDEN_STRIDE = 7          # stored iterates: every 10th, elements [::GOLDEN_STRIDE]


def azero_problem():
    """The reference's first LASSO test with A = 0 (x0 = 0.3, scale 1/6, b = (-1, 0, 1), lam 0.1: x = 0)."""
    return sp.csr_matrix((3, 1)), np.array([-1.0, 0.0, 1.0]), 0.1, 1.0 / 6.0, np.array([0.3])
