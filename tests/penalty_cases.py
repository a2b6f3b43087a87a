"""Per-column penalty factors: NumPy reference closures in the step kernel's arithmetic, factor generators, and the long-double
value of the certificate with its widened rounding bounds - shared by the penalty tests and their fixture script (no test in
here; tests/test_penalty_reference.py proves the closures on the CPU).

    g(x) = lam sum_j p_j |x_j| (+ box),  p_j >= 0;   p_j = 0: column j is not penalised (an intercept: a column of ones, p = 0)
    prox_{w g}(v)_j = clip(sign(v_j) max(|v_j| - (lam w) p_j, 0), lo, hi):  t = lam w ONCE, then tau_j = t * p_j per element
    the loss side is weight_cases.row_terms (square, logistic, huber) / poisson_cases.poisson_terms, with or without row weights

The reference project has no penalty factors.  The yardsticks are its SOLVER on these closures (fixture G19) and two exact
statements: p = 1 is the unfactored problem bit for bit (t * 1 == t), and the factored problem on A is the unfactored problem on
A diag(1 / p) in the variable p o x (p > 0).

The certificate (p > 0).  The dual constraint is |a_j^T theta| <= lam p_j.  With g'_j = g_j / p_j and x'_j = x_j p_j every quantity
of the unfactored certificate - alpha = min(1, lam / |g'|_inf), columns = sum (lam |x'_j| + alpha g'_j x'_j), lam |x'|_1 = g(x) - is
that of the unfactored problem with the matrix A' = A diag(1 / p) at x'.  ``gap_longdouble`` therefore calls the existing
long-double restatements (weight_cases / poisson_cases) on (A', x') with A' = fl(A / p) and x' = fl(x p) in fp64.

Widening of the bounds.  The restatements bound the error of an fp64 evaluation of THEIR inputs (A', x').  The device evaluates
(A, x, p), which differs from that in two roundings per column:
  * x'_j = fl(x_j p_j) is formed by the device with the same single rounding as here: the same bits, nothing to add;
  * a'_ij = fl(a_ij / p_j) exists only here.  The margin of the restatement, z'_i = sum_j a'_ij x'_j, differs from the device's
    exact margin sum_j a_ij x_j by two relative roundings per term (one in a', one in x'): |z' - z| <= 2 u (|A| |x|)_i to first
    order.  Every bound of the restatements is a sum of non-negative terms that are either independent of the margin error
    ds_i = gamma_n (|A| |x|)_i or linear in it, so multiplying a bound by (n + 2) / n covers a margin error of gamma_(n+2) (|A| |x|)_i;
  * g'_j: the restatement sums a'_ij rho_i (one rounding per term more than the device's a_ij rho_i: gamma_(m+2) -> gamma_(m+3)),
    and the device divides its g_j by p_j once (u |g'_j| <= u gfac (|A'|^T |rho|)_j more): both are covered by multiplying the
    bound, whose gradient part carries gamma_(m+2) gfac (|A'|^T |rho|)_j, by (m + 4) / (m + 2).
So every bound is multiplied by WIDEN(m, n) = (1 + 2 / n) (1 + 2 / (m + 2)).  The safety factor 2 of gap_cases stays on top."""
import numpy as np
import scipy.sparse as sp

import poisson_cases as PC
import sparse_cases as S
import weight_cases as W
from oracle import problems_ref as P

U = W.U
KEYS8 = W.KEYS8
FORMS = ("csr", "dense")
LOSSES = ("square", "logistic", "huber", "poisson")
LOSS_CODE = {"square": 0, "logistic": 1, "huber": 2, "poisson": 3}   # ZF_LOSS_*
SCALE = dict(W.SCALE, poisson=PC.SCALE)
GPU_SMALL = W.GPU_SMALL   # 300 x 1000, 1000 x 257, 64 x 4099


def make_problem(case, loss):
    """(A csr, b, lam, delta) of one (m, n, density, seed)."""
    if loss == "poisson":
        A, b, lam = PC.make_poisson(*case)
        return A, b, lam, 0.0
    return W.make_problem(case, loss)


def make_factors(n, seed, kind="real"):
    """``real``: in (0.25, 4), about 10 % exact zeros; ``positive``: the same draw without the zeros; ``intercept``: [0, 1, ..., 1];
    ``ones``."""
    if kind == "ones":
        return np.ones(n)
    if kind == "intercept":
        p = np.ones(n)
        p[0] = 0.0
        return p
    rng = np.random.default_rng(seed + 9000)
    p = 0.25 + 3.75 * rng.random(n)
    zero = rng.random(n) < 0.1
    if kind == "real":
        p[zero] = 0.0
    elif kind != "positive":
        raise ValueError(kind)
    return p


def matrix(A, storage):
    return A if storage == "csr" else A.toarray()


def prox_pf(v, t, p, bounds=None):
    """The step kernel's prox, NumPy operation by operation: tau_j = t * p_j, then the soft threshold, then the clip."""
    out = P.soft_threshold(v, t * p)
    if bounds is not None:
        out = P.clip_box(out, bounds[0], bounds[1])
    return out


class PenaltyRef:
    """The four closures of a margins problem with penalty factors on either storage form, NumPy / SciPy in fp64."""

    def __init__(self, A, b, lam, p, loss, delta=0.0, scale=None, bounds=None, w=None):
        self.A = sp.csr_matrix(A, dtype=np.float64) if sp.issparse(A) else np.asarray(A, float)
        self.b, self.p = np.asarray(b, float), np.asarray(p, float)
        self.w = None if w is None else np.asarray(w, float)
        self.loss, self.delta, self.lam = loss, float(delta), float(lam)
        self.scale = float(SCALE[loss] if scale is None else scale)
        self.gfac = 2 * self.scale if loss in ("square", "huber") else self.scale
        self.bounds = None if bounds is None else (float(bounds[0]), float(bounds[1]))

    def _rows(self, x):
        with np.errstate(invalid="ignore", over="ignore"):
            z = self.A @ x
            psi, phi = PC.poisson_terms(z, self.b) if self.loss == "poisson" else W.row_terms(z, self.b, self.loss, self.delta)
        if self.w is not None:
            if self.loss == "poisson":   # (the select of PoissonRef: the value is taken out before the product)
                on = self.w != 0.0
                return np.where(on, self.w * np.where(on, psi, 0.0), 0.0), np.where(on, self.w * np.where(on, phi, 0.0), 0.0)
            return W.weighted(self.w, psi), W.weighted(self.w, phi)
        return psi, phi

    def f(self, x):
        return self.scale * np.sum(self._rows(x)[1])

    def jac_f(self, x):
        return self.gfac * (self.A.T @ self._rows(x)[0])

    def g(self, x):
        if self.bounds is not None and ((x < self.bounds[0]).any() or (x > self.bounds[1]).any()):
            return np.inf
        return self.lam * np.sum(self.p * np.abs(x))

    def prox_wsum_g(self, weight, x):
        return prox_pf(x, self.lam * weight, self.p, self.bounds)

    def callbacks(self):
        return self.f, self.g, self.jac_f, self.prox_wsum_g


def scaled(A, p, x=None):
    """(A diag(1 / p) as CSR, p o x): the unfactored problem the factored one is (p > 0), each entry rounded once."""
    p = np.asarray(p, float)
    assert np.all(p > 0)
    A = sp.csr_matrix(A, dtype=np.float64)
    A1 = sp.csr_matrix((A.data / p[A.indices], A.indices.copy(), A.indptr.copy()), shape=A.shape)
    return A1, (None if x is None else np.asarray(x, float) * p)


def widen(m, n):
    return (1.0 + 2.0 / n) * (1.0 + 2.0 / (m + 2))


def gap_longdouble(A, b, p, x, lam, loss, delta=0.0, scale=None, w=None):
    """(values, bounds, extra) of the certificate with factors p > 0 at x: the existing restatements on (A diag(1 / p), p o x), every
    bound multiplied by ``widen(m, n)`` (module docstring)."""
    A1, x1 = scaled(A, p, x)
    m, n = A1.shape
    scale = SCALE[loss] if scale is None else scale
    if loss == "poisson":
        vals, bounds, extra = PC.gap_longdouble(A1, b, x1, lam, scale=scale, w=w)
    else:
        vals, bounds, extra = W.gap_longdouble(A1, b, np.ones(m) if w is None else w, x1, lam, loss, delta, scale)
    k = widen(m, n)
    vals = {key: vals[key] for key in KEYS8}
    return vals, {key: k * bounds[key] for key in KEYS8}, extra


def primal_longdouble(A, b, p, x, lam, loss, delta=0.0, scale=None, w=None):
    """P(x) = f(x) + lam sum p_j |x_j| in long double, on (A, x) itself (valid for p >= 0)."""
    ld = np.longdouble
    scale = SCALE[loss] if scale is None else scale
    A = sp.csr_matrix(A, dtype=np.float64)
    m = A.shape[0]
    rows = np.repeat(np.arange(m), np.diff(A.indptr))
    xl = np.asarray(x, np.float64).astype(ld)
    z = np.zeros(m, dtype=ld)
    np.add.at(z, rows, A.data.astype(ld) * xl[A.indices])
    bl = np.asarray(b, np.float64).astype(ld)
    if loss == "poisson":
        phi = np.exp(z) - bl * z
    else:
        phi = W.row_terms(z, bl, loss, ld(delta))[1]
    wl = np.ones(m, dtype=ld) if w is None else np.asarray(w, np.float64).astype(ld)
    f = ld(scale) * np.sum(np.where(wl != 0, wl * np.where(wl != 0, phi, ld(0)), ld(0)))
    return f + ld(lam) * np.sum(np.asarray(p, np.float64).astype(ld) * np.abs(xl))


worst_ratio = W.worst_ratio

# ---- the fixture G19 (tests/golden/make_golden_penalty.py) -------------------------------------------------------------------
GOLDEN_CASES = [0, 3]                       # indices into sparse_cases.SMALL: 300 x 1000, 64 x 4099
GOLDEN_LOSSES = ("square", "logistic")
GOLDEN_VARIANTS = {
    "ista": dict(nesterov=False),
    "fista": dict(nesterov=True, nesterov_ratio=(0, 0.25)),
}
GOLDEN_KW = dict(lr=1, tol=0.0, max_iter=80, return_all=True)
GOLDEN_STRIDE = 7
GOLDEN_SOLVES = [(loss, ci, st, tag) for loss in GOLDEN_LOSSES for ci in GOLDEN_CASES for st in FORMS for tag in GOLDEN_VARIANTS]


def golden_prefix(loss, ci, storage, tag):
    return f"penalty.{loss}.c{ci}.{storage}.{tag}"


def golden_ref(loss, ci, storage):
    case = S.SMALL[ci]
    A, b, lam, delta = make_problem(case, loss)
    return PenaltyRef(matrix(A, storage), b, lam, make_factors(case[1], case[3], "real"), loss, delta), A, b, lam
