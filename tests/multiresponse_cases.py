"""K responses on one dense matrix: the case tables of the multi-response tests, their inputs and their reference closures (no
test in here; tests/test_multiresponse_cases.py keeps the table honest on the CPU).

    X in R^{n x K}, B in R^{m x K}, flattened in C order:  x[j K + k] = X[j, k],  b[i K + k] = B[i, k]
    f(X) = scale sum_ik W_ik phi((A x_k)_i ; B_ik),   g(X) = lam sum_jk P_jk |X_jk| (+ (l2 / 2) |X|^2) (+ box)

is the existing margins problem on np.kron(A, np.eye(K)).  The REFERENCE of a case is therefore what the project already has:
the reference solver (oracle.cpu_ref) on the closures the existing case modules build - oracle.problems_ref.LeastSquaresL1Ref,
logistic_cases.LogisticL1Ref, weight_cases.WeightedRef (weights, l2), penalty_cases.PenaltyRef (factors) - over the Kronecker
matrix (``kron_ref``).  ``MRRef`` is the second evaluation of the same problem, per response (A @ X, A.T @ R): another order of
the same sums, which is what the device computes; the CPU test requires both to decide alike and to stay within 3e-15.

Shapes are small on purpose - the Kronecker matrix is (m K) x (n K) doubles, at most 1200 x 2100 here - and sit on the edges of
the kernels (csrc/zf_kernels_mr.h): n odd / = 2 mod 4 / = 0 mod 4 (scalar and 16-byte loads), one and several column chunks
(64 V columns) and column panels (256 V), m below / at / above the rows of a workgroup (16, 24, 32 for K <= 8, <= 12, <= 16),
slices with a short last one.

Seeds: a case whose two evaluations parted by more than 3e-15, or decided a trial differently, was given the next seed; the
number of replaced seeds is REPLACED below (counted when the table was drawn)."""
import numpy as np

import logistic_cases as L
import penalty_cases as PC
import weight_cases as W
from oracle import problems_ref as P

SCALE = {"square": 0.5, "logistic": 1.0}
KS = tuple(range(2, 17))    # every K is a kernel instantiation of its own (ZF_MR_EACH_K): the element-wise tests run them all
REPLACED = 11  # seeds replaced when the table was drawn: nine of the box endings (iterates of at most 0.3: a few ulps there are 1e-15 of the
               # largest entry), two of the boxed K = 16 cases of the main table; none of ALL_K
ITER_TOL = 3e-15


def rows_per_wg(K):
    """Rows a workgroup of the K-response row sweep owns (csrc/zf_kernels_mr.h: 8 waves x zf_mr_rt(K) rows)."""
    return 8 * (2 if K <= 8 else 3 if K <= 12 else 4)


def slices_of(m, n):
    """(slices, rows per slice) of the column sweep: zf_view_slices (csrc/zf_matview.h) for a K-response view, restated."""
    V = 2 if n % 2 == 0 else 1
    panels = (n // V + 255) // 256
    s = min((2048 + panels - 1) // panels, (m + 7) // 8, 64)
    s = max(s, 1)
    rps = (m + s - 1) // s
    return (m + rps - 1) // rps, rps


def sweep_shapes(K):
    """(m, n) of the element-wise sweep test for one K: every load width and remainder path of the two kernels."""
    r = rows_per_wg(K)
    return [(1, 7),              # one row, odd n below one chunk: scalar loads, the tail-row loop of the column sweep
            (r - 1, 131),        # one below the rows of a workgroup; odd n, three chunks of 64 with a short last one
            (r, 130),            # exactly one workgroup; n = 2 mod 4: 16-byte loads, a second chunk of one unit
            (r + 1, 132),        # one row into the second workgroup; n = 0 mod 4
            (100, 518),          # 13 slices of 8 rows, the last of 4; two column panels; five chunks
            (17, 64),            # 3 slices of 6 rows (one unrolled group + 2 tail rows), the last of 5
            (2048 * r + r + 1, 6)]   # more row groups than the capped grid of 2048 workgroups: the grid-stride loop


def make(loss, m, n, K, seed, lam_frac=0.1, col_decades=0.0):
    """(A, B, lam): B = A X_true + noise (square) or its sign (logistic); lam = lam_frac lam_max (a tenth unless told).
    ``col_decades`` d > 0 scales column j of A by 10^(-d j / (n - 1)): a tall matrix that is not solved in a handful of iterations."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    if col_decades > 0:
        A = A * np.logspace(0.0, -col_decades, n)
    k = max(1, min(10, n // 4))
    X = np.zeros((n, K))
    X[:k] = rng.standard_normal((k, K))
    if loss == "logistic":
        B = np.sign(A @ X + 0.1 * rng.standard_normal((m, K)))
        B[B == 0] = 1.0
        lam = lam_frac * SCALE[loss] * np.max(np.abs(A.T @ (B / 2)))
    else:
        B = A @ X + 0.01 * rng.standard_normal((m, K))
        lam = lam_frac * 2 * SCALE[loss] * np.max(np.abs(A.T @ B))
    return A, B, float(lam)


def make_weights(m, K, seed, kind):
    """None | ``real``: (m,) with zero rows, broadcast | ``mask``: a 0 / 1 mask per response, (m, K)."""
    if kind is None:
        return None
    rng = np.random.default_rng(seed + 7000)
    if kind == "mask":
        Wt = (rng.random((m, K)) >= 0.3).astype(np.float64)
        Wt[0] = 1.0
        return Wt
    w = np.where(rng.random(m) < 0.2, 0.0, 0.25 + 2.0 * rng.random(m))
    w[0] = 1.0
    return w


def make_factors(n, K, seed, kind):
    """None | ``pos``: (n, K) in (0.5, 2) | ``zero``: (n,) with p_0 = 0 (an unpenalised row of X), broadcast."""
    if kind is None:
        return None
    rng = np.random.default_rng(seed + 9000)
    if kind == "zero":
        p = 0.5 + 1.5 * rng.random(n)
        p[0] = 0.0
        return p
    return 0.5 + 1.5 * rng.random((n, K))


def wide(v, rows, K):
    """(rows,) or (rows, K) as (rows, K)."""
    v = np.asarray(v, float)
    return np.repeat(v.reshape(rows, 1), K, axis=1) if v.ndim == 1 else v


class Case:
    def __init__(self, loss, K, m, n, seed, weights=None, factors=None, l2fac=0.0, box=None, opts=None, x0="zeros", lam_frac=0.1, col_decades=0.0):
        self.loss, self.K, self.m, self.n, self.seed, self.lam_frac, self.col_decades = loss, K, m, n, seed, lam_frac, col_decades
        self.weights, self.factors, self.l2fac, self.box, self.x0kind = weights, factors, l2fac, box, x0
        self.opts = dict(lr=1.0, tol=0.0, max_iter=60, nesterov=True)
        self.opts.update(opts or {})

    @property
    def id(self):
        extra = "".join(f"-{t}" for t in (self.weights and "w" + self.weights, self.factors and "p" + self.factors,
                                            self.l2fac and "l2", self.box and "box", self.tag) if t)
        return f"{self.loss}-K{self.K}-{self.m}x{self.n}{extra}-s{self.seed}"

    tag = ""

    def data(self):
        A, B, lam = make(self.loss, self.m, self.n, self.K, self.seed, self.lam_frac, self.col_decades)
        Wt = make_weights(self.m, self.K, self.seed, self.weights)
        Pf = make_factors(self.n, self.K, self.seed, self.factors)
        return A, B, lam, Wt, Pf, self.l2fac * lam

    def x0(self):
        if self.x0kind == "outside":   # outside the box: g(x0) = inf
            return np.full(self.n * self.K, 0.5) + 0.1 * np.random.default_rng(self.seed + 1).standard_normal(self.n * self.K)
        return np.zeros(self.n * self.K)


def kron_ref(case):
    """The case on np.kron(A, I_K) through the closures the project already has."""
    A, B, lam, Wt, Pf, l2 = case.data()
    K = case.K
    big, b = np.kron(A, np.eye(K)), B.reshape(-1)
    scale = SCALE[case.loss]
    w = None if Wt is None else wide(Wt, case.m, K).reshape(-1)
    if Pf is not None:
        return PC.PenaltyRef(big, b, lam, wide(Pf, case.n, K).reshape(-1), case.loss, scale=scale, bounds=case.box, w=w)
    if w is not None or l2 > 0:
        return W.WeightedRef(big, b, lam, np.ones(b.size) if w is None else w, case.loss, scale=scale, bounds=case.box, l2=l2)
    if case.loss == "logistic":
        return L.LogisticL1Ref(big, b, lam, scale=scale, bounds=case.box)
    return P.LeastSquaresL1Ref(big, b, lam, scale=scale, bounds=case.box)


class MRRef:
    """The same problem evaluated per response: Z = A @ X, G = gfac A.T @ (W o psi(Z)); g and the prox are element-wise."""

    def __init__(self, case):
        A, B, lam, Wt, Pf, l2 = case.data()
        self.A, self.B, self.lam, self.l2, self.K, self.n, self.m = A, B, lam, l2, case.K, case.n, case.m
        self.W = None if Wt is None else wide(Wt, case.m, case.K)
        self.p = None if Pf is None else wide(Pf, case.n, case.K).reshape(-1)
        self.loss, self.scale, self.bounds = case.loss, SCALE[case.loss], case.box
        self.gfac = self.scale if case.loss == "logistic" else 2 * self.scale

    def _rows(self, x):
        with np.errstate(invalid="ignore", over="ignore"):
            psi, phi = W.row_terms(self.A @ x.reshape(self.n, self.K), self.B, self.loss)
        if self.W is not None:
            return W.weighted(self.W, psi), W.weighted(self.W, phi)
        return psi, phi

    def f(self, x):
        return self.scale * np.sum(self._rows(x)[1])

    def jac_f(self, x):
        return (self.gfac * (self.A.T @ self._rows(x)[0])).reshape(-1)

    def g(self, x):
        if self.bounds is not None and ((x < self.bounds[0]).any() or (x > self.bounds[1]).any()):
            return np.inf
        if self.p is not None:
            return self.lam * np.sum(self.p * np.abs(x))
        out = self.lam * np.linalg.norm(x, ord=1)
        return out + (self.l2 / 2) * np.sum(x * x) if self.l2 > 0 else out

    def prox_wsum_g(self, weight, x):
        if self.p is not None:
            return PC.prox_pf(x, self.lam * weight, self.p, self.bounds)
        x = P.soft_threshold(x, self.lam * weight)
        if self.l2 > 0:
            x = x * (1.0 / (1.0 + self.l2 * weight))
        if self.bounds is not None:
            x = P.clip_box(x, self.bounds[0], self.bounds[1])
        return x

    def callbacks(self):
        return self.f, self.g, self.jac_f, self.prox_wsum_g


BOX = (-0.05, 0.3)


def _table():
    out = []
    for loss, s0 in (("square", 100), ("logistic", 200)):
        out += [
            Case(loss, 2, 300, 518, s0 + 0),
            Case(loss, 2, 17, 131, s0 + 1, weights="real"),
            Case(loss, 5, 100, 130, s0 + 2, factors="pos"),
            Case(loss, 5, 33, 67, s0 + 3, l2fac=0.01),
            Case(loss, 16, 31, 131, s0 + 4),
            Case(loss, 16, 33, 130, s0 + 8, weights="mask", box=BOX),
            Case(loss, 5, 64, 132, s0 + 6, factors="zero"),
            Case(loss, 16, 32, 128, s0 + 7, weights="real", factors="pos"),
            Case(loss, 2, 100, 518, s0 + 5, weights="mask", l2fac=0.01),
        ]
    for loss, s0 in (("square", 100), ("logistic", 200)):   # K = 9 .. 12: the three-row tile (behind the others: their indices are used)
        out += [Case(loss, 9, 25, 66, s0 + 9), Case(loss, 12, 23, 131, s0 + 10, weights="real")]
    return out


def _lr(loss, K, m, n, seed, lam_frac, c):
    """c / L with L = gfac |A|_2^2 (logistic: a quarter of it): the step as a multiple of the safe one."""
    A = make(loss, m, n, K, seed, lam_frac)[0]
    return float(c / ((1.0 if loss == "square" else 0.25) * np.linalg.norm(A, 2) ** 2))


# "Backtracking failed" AFTER accepted iterations, with one trial per iteration (max_backtrack_iter = 1): a large lam keeps the first
# iterates on a few columns, where a step of 3 .. 4 / L passes the sufficient-decrease test; it fails once more columns are active.
# (loss, K, m, n, seed, lam_frac, c) - found by a scan on the CPU; the oracle accepts 2 .. 12 iterations on them.
_FAILK = {"square": [(5, 33, 67, 310, 0.8, 4.0), (16, 17, 34, 320, 0.8, 3.0), (2, 40, 66, 301, 0.8, 4.0)],
          "logistic": [(2, 40, 66, 400, 0.5, 3.5), (5, 33, 67, 410, 0.5, 4.0), (2, 40, 66, 404, 0.5, 4.0)]}
# F(x0) = inf under a box: (K, m, n, seed) that kept the two evaluations within ITER_TOL (see REPLACED)
_INF = {"square": [(2, 40, 66, 300), (5, 33, 67, 313), (16, 17, 34, 323)], "logistic": [(2, 40, 66, 400), (5, 24, 40, 416), (16, 17, 34, 421)]}


def _endings():
    """Every way a run ends, three times per loss (the CPU test counts them): by tol; "Backtracking failed" at once and after
    accepted iterations; one iteration; F(x0) = inf under a box."""
    out = []
    for loss, s0 in (("square", 300), ("logistic", 400)):
        for j, (K, m, n) in enumerate(((2, 40, 66), (5, 33, 67), (16, 17, 34))):
            s = s0 + 10 * j
            for tag, sd, kw in (("tol", s, dict(opts=dict(tol=1e-1 if loss == "square" else 3e-2, max_iter=200))),
                                ("fail0", s, dict(opts=dict(lr=1e3, max_backtrack_iter=1))),
                                ("one", s, dict(opts=dict(max_iter=1)))):
                c = Case(loss, K, m, n, sd, **kw)
                c.tag = tag
                out.append(c)
        for K, m, n, sd in _INF[loss]:
            c = Case(loss, K, m, n, sd, box=BOX, x0="outside", opts=dict(max_iter=12))
            c.tag = "inf"
            out.append(c)
        for K, m, n, sd, frac, cc in _FAILK[loss]:
            c = Case(loss, K, m, n, sd, lam_frac=frac, opts=dict(lr=_lr(loss, K, m, n, sd, frac, cc), max_backtrack_iter=1, max_iter=200))
            c.tag = "failk"
            out.append(c)
    return out


def _all_k():
    """One short solve per loss and per K = 2 .. 16 through the solver's ring-indexed launches: m one row into the second workgroup
    of the row sweep; n = 67 (scalar loads, V = 1) under one loss and 130 (16-byte loads, V = 2) under the other, swapped with
    K // 2, so every K meets both widths; none / weights / factors by K % 3."""
    out = []
    for loss, s0 in (("square", 600), ("logistic", 700)):
        for K in range(2, 17):
            n = (67, 130)[((K // 2) + (loss == "logistic")) % 2]
            extra = (dict(), dict(weights="real"), dict(factors="pos"))[K % 3]
            c = Case(loss, K, rows_per_wg(K) + 1, n, s0 + K, opts=dict(max_iter=30), **extra)
            c.tag = "allk"
            out.append(c)
    return out


CASES = _table()
ENDINGS = _endings()
ALL_K = _all_k()
# m K > 32768 rows of margins, unweighted squared loss: the solver forms r(y), f(y) and f(x+) with many workgroups there (the wide
# residual kernels of the sparse kind), which no case above reaches.  Tall and narrow, so the reference closures stay cheap; eight
# iterations: the columns are scaled over 1.5 decades, yet the few active coefficients are found within ten iterations, after
# which the acceptance test decides on rounding noise.
TALL = [Case("square", K, 4100, 6, 500 + K, opts=dict(max_iter=8), col_decades=1.5, lam_frac=0.02) for K in (8, 16)]
SNAPSHOT_CASES = [0, 5, 9, 16]   # indices into CASES: snapshot and resume across the last chunk
