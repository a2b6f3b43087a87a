"""Multinomial (softmax) regression: inputs, NumPy reference closures in both forms, the long-double restatement of the row kernels
and of the certificate with first-order rounding bounds, and the case tables of the multinomial tests (no test in here;
tests/test_multinomial_cases.py keeps them honest on the CPU).

    Y (m, K) rows on the simplex, X (n, K), flattened in C order:  x[j K + k] = X[j, k],  y[i K + k] = Y[i, k]
    f(X) = scale sum_i w_i [logsumexp(z_i) - <y_i, z_i>],  z_i = (A X)_i,     grad f = scale A^T (w o (softmax(Z) - Y)),   scale = 1
    g(X) = lam sum_jk P_jk |X_jk| (+ (l2 / 2) |X|^2) (+ box)

The arithmetic of one row - every kernel of csrc/zf_kernels_softmax.h and ``row_terms`` below:
    mx = max_k z_k;  d_k = z_k - mx;  e_k = exp(d_k);  S = sum_k e_k (k order);  rS = 1 / S;  p_k = e_k rS
    psi_k = p_k - y_k;   phi = log S + sum_k y_k (-d_k)   (k order, log S first)
a row with w_i = 0 is a row that is not there (a select, whatever y_i holds); w_i multiplies the K entries of psi and phi once.
``MultinomialRef`` evaluates per row (A @ X, A.T @ R); ``KronRef`` the same problem on np.kron(A, I_K) with flat vectors: another
order of the sums of the two sweeps, the same rows.

The certificate.  The conjugate of logsumexp(z) - <y, z> at theta is sum_k v_k log v_k with v = theta + y on the simplex (+inf off it).
theta = alpha psi, alpha = min(1, lam / |g|_inf):  v = alpha p + (1 - alpha) y, a convex combination - feasible for every alpha.
    D = -scale sum_i w_i sum_k v_ik log v_ik (0 log 0 = 0)
    Fenchel-Young gap of row i = KL(v_i || p_i) = sum_k v_k (log v_k - log p_k),  log p_k = d_k - log S   (>= 0; 0 at alpha = 1)
    rows = scale sum_i w_i [that];  columns, alpha, 1 - alpha, the ridge part, gt = g + l2 x and the factors: gap_cases / enet_cases
    / penalty_cases.  gap = rows (+ ridge) + columns.

Rounding bounds: the symbols of tests/gap_cases.py (u = 2^-53, gamma_k, ds_ik the error of the device's margin, the safety factor 2
on every bound); the device's exp and log carry 1 ulp <= 2 u relative, as in tests/poisson_cases.py.  dsr_i = max_k ds_ik.
  d     the maximum is a selection (exact on the device's margins, within dsr of the true one); one subtraction:
                                                                                        dd_k = ds_k + dsr + u |d_k|
  e     exp(d^)(1 + 2u), exp(d + dd) = e (1 + dd):                                      de_k = e_k (dd_k + 2 u)
  S     K terms >= 0:                                                                   dS = sum_k de_k + gamma_K S
  p     rS = 1 / S: dS / S + u relative; one product:                                   dp_k = p_k (dd_k + dS / S + 5 u)
  psi   one subtraction:                                                                dpsi_k = dp_k + u |psi_k|
  phi   log S: dS / S + 2 u log S; K products y_k (-d_k): y_k dd_k + u y_k |d_k|; K + 1 terms >= 0:
                                                      dphi = dS / S + 2 u log S + sum_k y_k (dd_k + u |d_k|) + gamma_(K+1) phi
  weights, f, g   poisson_cases' lines with m rows: d(w t) = w dt + u |w t|;  d(f) = scale (sum d(w phi) + gamma_m sum w phi) + u f;
                  dg_jk = scale ((|A|^T d(w psi))_jk + gamma_(m+2) (|A|^T |w psi|)_jk)
  factors   g' = g / P, x' = x P: one rounding each:  dg' = dg / P + u |g'|,  and u |x'| carried into the column terms
  v     alpha p + oma y:                                                                dv_k = d(alpha) p_k + alpha dp_k + d(oma) y_k + 2 u v_k
  ent   c_k = v log v, dc/dv = log v + 1, log 2 u relative, one product:                d(c_k) = dv (|log v| + 1) + 3 u |c_k|
        row: + gamma_K sum |c_k|;  D: scale (sum w d(row) + gamma_(m+1) sum w |row|) + u |D|
  KL    lp_k = d_k - log S:  d(lp) = dd_k + dS / S + 2 u log S + u |lp_k|;  q = log v - lp:  dq = dv / v + 2 u |log v| + d(lp) + u |q|
        t_k = v q:  dt_k = dv |q| + v dq + u |t_k|;  row: sum dt_k + gamma_K sum |t_k| (the clamp at 0 moves towards the true value)
        alpha = 1 in exact arithmetic but not certainly on the device: its 1 - alpha is at most d(oma) and a row is of second order in
        it; the bound keeps the first-order expression d(oma) sum_k (y_k (1 + |lp_k|) + p_k), which is larger.
  P, gap   gap_cases' / enet_cases' lines.
  underflow  exp below 2^-1022 loses its relative accuracy: m K 2^-1022 is added to every bound a row sum enters.

Seeds: a case whose two evaluations (per row / Kronecker) decided a trial differently or parted by more than ITER_TOL would be given
the next seed; REPLACED counts them."""
import numpy as np
import scipy.sparse as sp

import gap_cases as GC
from oracle import problems_ref as P

U = GC.U
KEYS8 = GC.KEYS
KEYS10 = GC.KEYS + ("g_l2", "ridge_gap")
SCALE = 1.0
KS = tuple(range(2, 17))   # every K is a kernel instantiation of its own
REPLACED = 0               # seeds replaced when the tables were drawn
ITER_TOL = 3e-15
WIDE = 32768               # flattened entries m K above which the rows kernels take the many-workgroup shape (zf_rows_wide)
BOX = (-0.05, 0.3)


# ---- one row ------------------------------------------------------------------------------------------------------------------------
def row_terms(Z, Y):
    """(psi (m, K), phi (m,)) of margins Z (m, K) in the arithmetic of the kernels, any float dtype."""
    Z, Y = np.asarray(Z), np.asarray(Y)
    K = Z.shape[1]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d = Z - np.max(Z, axis=1, keepdims=True)
        e = np.exp(d)
        S = e[:, 0].copy()
        for k in range(1, K):
            S = S + e[:, k]
        rS = 1.0 / S
        psi = e * rS[:, None] - Y
        phi = np.log(S)
        for k in range(K):
            phi = phi + Y[:, k] * (-d[:, k])
    return psi, phi


def weighted(w, psi, phi):
    """The two outputs with one weight per row: a select for w_i = 0 (+0 whatever the row holds), one product otherwise."""
    if w is None:
        return psi, phi
    on = np.asarray(w) != 0.0
    with np.errstate(invalid="ignore"):
        return (np.where(on[:, None], w[:, None] * np.where(on[:, None], psi, 0.0), 0.0),
                np.where(on, w * np.where(on, phi, 0.0), 0.0))


def one_hot(labels, K):
    Y = np.zeros((len(labels), K))
    Y[np.arange(len(labels)), labels] = 1.0
    return Y


# ---- the closures -------------------------------------------------------------------------------------------------------------------
class _PenaltyMixin:
    def g(self, x):
        if self.bounds is not None and ((x < self.bounds[0]).any() or (x > self.bounds[1]).any()):
            return np.inf
        if self.p is not None:
            return self.lam * np.sum(self.p * np.abs(x))
        out = self.lam * np.linalg.norm(x, ord=1)
        return out + (self.l2 / 2) * np.sum(x * x) if self.l2 > 0 else out

    def prox_wsum_g(self, weight, x):
        if self.p is not None:
            x = np.sign(x) * np.maximum(np.abs(x) - (self.lam * weight) * self.p, 0.0)
        else:
            x = P.soft_threshold(x, self.lam * weight)
            if self.l2 > 0:
                x = x * (1.0 / (1.0 + self.l2 * weight))
        if self.bounds is not None:
            x = P.clip_box(x, self.bounds[0], self.bounds[1])
        return x

    def callbacks(self):
        return self.f, self.g, self.jac_f, self.prox_wsum_g

    def _init(self, A, Y, lam, scale, bounds, l2, w, p):
        self.Y = np.asarray(Y, float)
        self.m, self.K = self.Y.shape
        self.n = A.shape[1]
        self.lam, self.scale, self.l2 = float(lam), float(scale), float(l2)
        self.bounds = None if bounds is None else (float(bounds[0]), float(bounds[1]))
        self.w = None if w is None else np.asarray(w, float)
        self.p = None if p is None else wide(p, self.n, self.K).reshape(-1)


class MultinomialRef(_PenaltyMixin):
    """The four closures, per row: Z = A @ X (dense or scipy.sparse A), G = scale A.T @ (w o psi)."""

    def __init__(self, A, Y, lam, scale=SCALE, bounds=None, l2=0.0, w=None, p=None):
        self.A = sp.csr_matrix(A, dtype=np.float64) if sp.issparse(A) else np.asarray(A, float)
        self._init(self.A, Y, lam, scale, bounds, l2, w, p)

    def _rows(self, x):
        Z = np.asarray(self.A @ np.asarray(x, float).reshape(self.n, self.K))
        return weighted(self.w, *row_terms(Z, self.Y))

    def f(self, x):
        return self.scale * np.sum(self._rows(x)[1])

    def jac_f(self, x):
        return np.asarray(self.scale * (self.A.T @ self._rows(x)[0])).reshape(-1)


class KronRef(_PenaltyMixin):
    """The same problem on np.kron(A, I_K) with flat vectors: the form DESIGN 4.5m states every K-response class in."""

    def __init__(self, A, Y, lam, scale=SCALE, bounds=None, l2=0.0, w=None, p=None):
        A = A.toarray() if sp.issparse(A) else np.asarray(A, float)
        self._init(A, Y, lam, scale, bounds, l2, w, p)
        self.big = np.kron(A, np.eye(self.K))

    def _rows(self, x):
        return weighted(self.w, *row_terms((self.big @ x).reshape(self.m, self.K), self.Y))

    def f(self, x):
        return self.scale * np.sum(self._rows(x)[1])

    def jac_f(self, x):
        return self.scale * (self.big.T @ self._rows(x)[0].reshape(-1))


def wide(v, rows, K):
    """(rows,) or (rows, K) as (rows, K)."""
    v = np.asarray(v, float)
    return np.repeat(v.reshape(rows, 1), K, axis=1) if v.ndim == 1 else v


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def make(m, n, K, seed, labels="hot", absent=False, lam_frac=0.1, density=None):
    """(A, Y, lam): labels drawn from softmax(A X_true + noise); ``hot``: one-hot rows, ``soft``: that distribution mixed with the
    one-hot row (rows on the simplex to an ulp, renormalised); ``absent``: class K - 1 never occurs (its column of Y is 0).
    lam = lam_frac lam_max, lam_max = scale |A^T (1 / K - Y)|_inf.  ``density``: A with that share of stored elements (dense array)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    if density is not None:
        A = A * (rng.random((m, n)) < density)
    k = max(1, min(10, n // 4))
    X = np.zeros((n, K))
    X[:k] = rng.standard_normal((k, K))
    Z = A @ X + 0.5 * rng.standard_normal((m, K))
    Kc = K - 1 if absent and K > 2 else K
    Pm = np.exp(Z[:, :Kc] - Z[:, :Kc].max(axis=1, keepdims=True))
    Pm /= Pm.sum(axis=1, keepdims=True)
    lab = np.array([rng.choice(Kc, p=Pm[i]) for i in range(m)])
    Y = one_hot(lab, K)
    if labels == "soft":
        Y[:, :Kc] = 0.75 * Y[:, :Kc] + 0.25 * Pm
        Y /= Y.sum(axis=1, keepdims=True)
    lam = lam_frac * SCALE * float(np.max(np.abs(A.T @ (1.0 / K - Y))))
    return A, Y, lam


def make_weights(m, seed, kind):
    """None | ``real``: (m,) with zero rows | ``nan``: the same, and the rows with w = 0 get a NaN y (``poison``)."""
    if kind is None:
        return None
    rng = np.random.default_rng(seed + 7000)
    w = np.where(rng.random(m) < 0.2, 0.0, 0.25 + 2.0 * rng.random(m))
    w[0], w[m - 1] = 1.0, 0.0
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


class Case:
    tag = ""

    def __init__(self, K, m, n, seed, weights=None, factors=None, l2fac=0.0, box=None, labels="hot", absent=False, opts=None, lam_frac=0.1):
        self.K, self.m, self.n, self.seed, self.lam_frac = K, m, n, seed, lam_frac
        self.weights, self.factors, self.l2fac, self.box, self.labels, self.absent = weights, factors, l2fac, box, labels, absent
        self.opts = dict(lr=1.0, tol=0.0, max_iter=60, nesterov=True)
        self.opts.update(opts or {})

    @property
    def id(self):
        extra = "".join(f"-{t}" for t in (self.weights and "w" + self.weights, self.factors and "p" + self.factors, self.l2fac and "l2",
                                            self.box and "box", self.labels == "soft" and "soft", self.absent and "absent", self.tag) if t)
        return f"K{self.K}-{self.m}x{self.n}{extra}-s{self.seed}"

    def data(self):
        """(A, Y, lam, w, factors, l2); with weights ``nan`` the rows of Y whose weight is 0 hold NaN."""
        A, Y, lam = make(self.m, self.n, self.K, self.seed, self.labels, self.absent, self.lam_frac)
        w = make_weights(self.m, self.seed, self.weights)
        if self.weights == "nan":
            Y = Y.copy()
            Y[w == 0.0] = np.nan
        return A, Y, lam, w, make_factors(self.n, self.K, self.seed, self.factors), self.l2fac * lam

    def x0(self):
        return np.zeros(self.n * self.K)

    def ref(self, cls=None):
        A, Y, lam, w, Pf, l2 = self.data()
        return (cls or MultinomialRef)(A, Y, lam, SCALE, self.box, l2, w, Pf)


def _table():
    """K in {2, 3, 5, 8, 12, 16} x weights none / real with zero rows / a zero-weight row whose y is NaN x factors none / positive / an
    exact-zero row x l2 in {0, lam / 100} x a box x one-hot and soft labels x a class that never occurs."""
    return [
        Case(2, 300, 130, 100),
        Case(2, 17, 131, 101, weights="real"),
        Case(3, 100, 66, 102, labels="soft"),
        Case(3, 40, 67, 103, weights="nan", labels="soft"),
        Case(5, 100, 130, 104, factors="pos"),
        Case(5, 33, 67, 105, l2fac=0.01),
        Case(5, 64, 132, 106, factors="zero", absent=True),
        Case(8, 50, 66, 107, weights="real", l2fac=0.01, labels="soft"),
        Case(8, 31, 131, 108, box=BOX),
        Case(12, 23, 131, 109, weights="real", factors="pos"),
        Case(12, 25, 66, 110, absent=True, labels="soft"),
        Case(16, 31, 131, 111),
        Case(16, 33, 130, 112, weights="nan", box=BOX),
        Case(16, 32, 128, 113, weights="real", factors="pos", labels="soft"),
    ]


def _endings():
    """By tol, "Backtracking failed" (a step of 1e3 and one trial), and one iteration - for three K each."""
    out = []
    for j, (K, m, n) in enumerate(((2, 40, 66), (5, 33, 67), (16, 17, 34))):
        s = 300 + 10 * j
        for tag, kw in (("tol", dict(opts=dict(tol=3e-2, max_iter=200))), ("fail0", dict(opts=dict(lr=1e3, max_backtrack_iter=1))),
                        ("one", dict(opts=dict(max_iter=1)))):
            c = Case(K, m, n, s, **kw)
            c.tag = tag
            out.append(c)
    return out


def _all_k():
    """One 30-iteration solve per K = 2 .. 16 through the solver's ring-indexed launches: m = 33, n = 67 / 130 alternating with K;
    none / weights / factors by K % 3; soft labels for odd K."""
    out = []
    for K in KS:
        extra = (dict(), dict(weights="real"), dict(factors="pos"))[K % 3]
        c = Case(K, 33, (67, 130)[K % 2], 600 + K, opts=dict(max_iter=30), labels="soft" if K % 2 else "hot", **extra)
        c.tag = "allk"
        out.append(c)
    return out


CASES = _table()
ENDINGS = _endings()
ALL_K = _all_k()
SNAPSHOT_CASES = [0, 7, 12]   # indices into CASES: snapshot and resume across the last chunk
GAP_CASE = Case(3, 200, 40, 900, lam_frac=0.2)   # tall: a first-order method brings it to a small gap (gap_tol, l1_path, lam_max)
# the golden fixture (tests/golden/make_golden_multinomial.py -> g20_multinomial.npz): the reference's solver on MultinomialRef for three
# small problems, 60 FISTA iterations from lr = 1 with return_all; every 10th iterate is kept, its elements [::GOLDEN_STRIDE]
GOLDEN_CASES = [Case(3, 40, 67, 950, labels="soft"), Case(5, 33, 130, 951, weights="real"), Case(16, 31, 66, 952, l2fac=0.01, absent=True)]
GOLDEN_STRIDE = 7
GOLDEN_KEPT = list(range(0, 61, 10))


def golden_prefix(ci):
    return f"multinomial.c{ci}"


def eval_rows(K):
    """Row counts of the element-wise test for one K: around a wave and a workgroup of either shape, the last narrow count and the
    first wide one (m K > 32768) for K = 2 and 16, and one wide count whose last chunk is short."""
    out = [1, 63, 64, 65, 1023, 1024, 1025, 2049]
    if K in (2, 16):
        first = WIDE // K + 1
        out += [first - 1, first, first + 1000 // K + 7]
    return out


# ---- the long-double restatement ----------------------------------------------------------------------------------------------------
def _need_longdouble():
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError("np.longdouble carries fewer than 63 mantissa bits here: an fp64 evaluation cannot be checked against it")


def _f64(v):
    return np.asarray(v, dtype=np.float64)


def _row_parts(Z, Y, ds):
    """Everything of the rows in longdouble with its first-order bound (fp64): a dict."""
    ld = np.longdouble
    K = Z.shape[1]
    dsr = ds.max(axis=1, keepdims=True)
    d = Z - Z.max(axis=1, keepdims=True)
    e = np.exp(d)
    S = e.sum(axis=1)
    p = e / S[:, None]
    logS = np.log(S)
    dd = ds + dsr + U * _f64(np.abs(d))
    de = _f64(e) * (dd + 2 * U)
    dS = de.sum(axis=1) + GC._gamma(K) * _f64(S)
    rel = dS / _f64(S)
    dp = _f64(p) * (dd + rel[:, None] + 5 * U)
    psi = p - Y
    dpsi = dp + U * _f64(np.abs(psi))
    phi = logS + np.sum(Y * (-d), axis=1)
    dphi = rel + 2 * U * _f64(logS) + np.sum(_f64(Y) * (dd + U * _f64(np.abs(d))), axis=1) + GC._gamma(K + 1) * _f64(np.abs(phi))
    lp = d - logS[:, None]
    dlp = dd + (rel + 2 * U * _f64(logS))[:, None] + U * _f64(np.abs(lp))
    return dict(d=d, e=e, S=S, p=p, logS=logS, psi=psi, phi=phi, dd=dd, dp=dp, dpsi=dpsi, dphi=dphi, lp=lp, dlp=dlp, ld=ld)


def _weights(w, Y, m):
    ld = np.longdouble
    on = np.ones(m, bool) if w is None else np.asarray(w) != 0.0
    wl = np.ones(m, dtype=ld) if w is None else np.asarray(w, np.float64).astype(ld)
    Yl = np.where(on[:, None], np.asarray(Y, np.float64), 0.0).astype(ld)   # (a row that is not there: its y never reaches an output)
    return on, wl, Yl


def loss_longdouble(Z, Y, scale=SCALE, w=None, ds=None):
    """The outputs of the rows kernel at margins Z (m, K) (fp64 values, taken as exact unless ``ds`` bounds their error):
    (f, bound of f, w o psi (m, K), bound of every element of it), the values in longdouble, the bounds with the safety factor 2."""
    _need_longdouble()
    Z64 = np.asarray(Z, np.float64)
    m, K = Z64.shape
    ds = np.zeros((m, K)) if ds is None else np.asarray(ds, np.float64)
    on, wl, Yl = _weights(w, Y, m)
    R = _row_parts(Z64.astype(np.longdouble), Yl, ds)
    w64 = _f64(wl)
    wpsi = np.where(on[:, None], wl[:, None] * R["psi"], np.longdouble(0))
    wphi = np.where(on, wl * R["phi"], np.longdouble(0))
    dwpsi = np.where(on[:, None], w64[:, None] * R["dpsi"] + U * _f64(np.abs(wpsi)), 0.0)
    dwphi = np.where(on, w64 * R["dphi"] + U * _f64(np.abs(wphi)), 0.0)
    f = np.longdouble(scale) * np.sum(wphi)
    d_f = scale * (float(np.sum(dwphi)) + GC._gamma(m) * float(np.sum(np.abs(wphi)))) + U * abs(float(f)) + m * K * 2.0 ** -1022
    return f, 2 * d_f, wpsi, 2 * dwpsi


def gap_longdouble(A, Y, X, lam, scale=SCALE, l2=0.0, w=None, pf=None):
    """(values, bounds, extra): the certificate at X (n, K) or flat, over KEYS8 when l2 = 0 and KEYS10 otherwise, values in longdouble,
    bounds in fp64 with the safety factor 2.  extra: ``gap_pd`` = P - D in longdouble, ``grad`` (n, K), ``terms`` (the weighted row
    gaps), ``wpsi``, ``dgrad``."""
    _need_longdouble()
    ld = np.longdouble
    _gamma = GC._gamma
    A = A.toarray() if sp.issparse(A) else np.asarray(A, np.float64)
    m, n = A.shape
    K = np.asarray(Y).shape[1]
    Al, absA = A.astype(ld), np.abs(A)
    Xl = np.asarray(X, np.float64).reshape(n, K).astype(ld)
    X64 = _f64(Xl)
    on, wl, Yl = _weights(w, Y, m)
    w64, Y64 = _f64(wl), _f64(Yl)
    lam_l, sc, l2_l = ld(lam), ld(scale), ld(l2)
    tiny = m * K * 2.0 ** -1022
    Z = Al @ Xl
    ds = _gamma(n) * (absA @ np.abs(X64))
    R = _row_parts(Z, Yl, ds)
    p64 = _f64(R["p"])
    # ---- rows: w o psi, f
    wpsi = np.where(on[:, None], wl[:, None] * R["psi"], ld(0))
    wphi = np.where(on, wl * R["phi"], ld(0))
    dwpsi = np.where(on[:, None], w64[:, None] * R["dpsi"] + U * _f64(np.abs(wpsi)), 0.0)
    dwphi = np.where(on, w64 * R["dphi"] + U * _f64(np.abs(wphi)), 0.0)
    f = sc * np.sum(wphi)
    d_f = scale * (float(np.sum(dwphi)) + _gamma(m) * float(np.sum(np.abs(wphi)))) + U * abs(float(f)) + tiny
    # ---- g = scale A^T (w psi), the factors, gt = g + l2 x, the scaling
    g = sc * (Al.T @ wpsi)
    dg = float(scale) * (absA.T @ dwpsi + _gamma(m + 2) * (absA.T @ _f64(np.abs(wpsi)))) + tiny
    xs, dxs = Xl, np.zeros((n, K))
    if pf is not None:
        pl = wide(pf, n, K).astype(ld)
        g = g / pl
        dg = dg / _f64(pl) + U * _f64(np.abs(g))
        xs = Xl * pl
        dxs = U * _f64(np.abs(xs))
    if l2 > 0:
        gt = g + l2_l * xs
        dgt = dg + U * _f64(np.abs(gt))
    else:
        gt, dgt = g, dg
    G = np.max(np.abs(gt))
    dG = float(np.max(dgt))
    if G > lam_l:
        alpha, oma = lam_l / G, (G - lam_l) / G
    else:
        alpha, oma = ld(1), ld(0)
    big = max(float(G), float(lam))
    d_alpha = (dG / big + U) if big > 0 else 0.0
    d_oma = (2 * dG / big + 2 * U * float(oma)) if big > 0 else 0.0
    if float(G) * (1 + 2 * U) + dG <= float(lam):
        d_alpha = d_oma = 0.0   # no fp64 evaluation inside dG of g can leave the branch alpha = 1, 1 - alpha = 0: both are exact
    a64, o64 = float(alpha), float(oma)
    # ---- columns, g_l1, the ridge part
    ax = _f64(np.abs(xs))
    tj = lam_l * np.abs(xs) + alpha * gt * xs
    cols = np.sum(tj)
    d_t = (ax * (d_alpha * _f64(np.abs(gt)) + a64 * dgt + U * a64 * _f64(np.abs(gt)) + U * float(lam)) + U * _f64(np.abs(tj))
           + dxs * (float(lam) + a64 * _f64(np.abs(gt))))
    d_cols = float(np.sum(d_t)) + _gamma(n * K) * float(np.sum(np.abs(tj)))
    asum = np.sum(np.abs(xs))
    g_l1 = lam_l * asum
    d_gl1 = float(lam) * (_gamma(n * K + 1) * float(asum) + float(np.sum(dxs)))
    xx = np.sum(xs * xs)
    g_l2 = l2_l / 2 * xx
    d_gl2 = float(l2) / 2 * _gamma(n * K + 1) * float(xx) + U * float(g_l2)
    ridge = oma * oma * g_l2
    d_ridge = 2 * o64 * d_oma * float(g_l2) + o64 ** 2 * d_gl2 + 4 * U * float(ridge)
    # ---- the conjugate and the dual
    v = alpha * R["p"] + oma * Yl
    v64 = _f64(v)
    dv = d_alpha * p64 + a64 * R["dp"] + d_oma * Y64 + 2 * U * v64
    with np.errstate(divide="ignore", invalid="ignore"):
        logv = np.where(v > 0, np.log(np.where(v > 0, v, ld(1))), ld(0))
        lv_b = np.abs(np.log(np.maximum(v64, 2.0 ** -1074)))   # (|log| where the device may hold a denormal for an exact 0)
    c = v * logv
    d_c = dv * (lv_b + 1) + 3 * U * _f64(np.abs(c))
    ent = np.sum(c, axis=1)
    d_ent = np.sum(d_c, axis=1) + _gamma(K) * _f64(np.sum(np.abs(c), axis=1))
    D_loss = -sc * np.sum(np.where(on, wl * ent, ld(0)))
    d_Dl = (scale * (float(np.sum(np.where(on, w64 * d_ent + U * w64 * _f64(np.abs(ent)), 0.0)))
                     + _gamma(m + 1) * float(np.sum(np.where(on, w64 * _f64(np.abs(ent)), 0.0)))) + U * abs(float(D_loss)) + tiny)
    # ---- the row gaps
    alp = _f64(np.abs(R["lp"]))
    if oma > 0:
        q = logv - R["lp"]
        t = np.where(v > 0, v * q, ld(0))
        kl = np.maximum(np.sum(t, axis=1), ld(0))
        q64 = _f64(np.abs(q))
        with np.errstate(divide="ignore", invalid="ignore"):
            dq = np.where(v64 > 0, dv / np.where(v64 > 0, v64, 1.0), 0.0) + 2 * U * lv_b + R["dlp"] + U * q64
        dt = np.where(v64 > 0, dv * q64 + v64 * dq + U * _f64(np.abs(t)), dv * (lv_b + alp + 1))
        d_kl = np.sum(dt, axis=1) + _gamma(K) * _f64(np.sum(np.abs(t), axis=1))
    else:
        kl = np.zeros(m, dtype=ld)
        d_kl = np.zeros(m) if d_oma == 0.0 else d_oma * np.sum(Y64 * (1 + alp) + p64, axis=1)
    wt = np.where(on, wl * kl, ld(0))
    rows_gap = sc * np.sum(wt)
    d_rows = scale * (float(np.sum(np.where(on, w64 * d_kl + U * w64 * _f64(kl), 0.0))) + _gamma(m + 1) * float(np.sum(wt))) + U * float(rows_gap)
    d_rows += tiny if float(d_rows) > 0 else 0.0
    if l2 > 0:
        Pv = f + g_l1 + g_l2
        d_P = d_f + d_gl1 + d_gl2 + 2 * U * abs(float(Pv))
        D = D_loss - alpha * alpha * g_l2
        d_D = d_Dl + 2 * a64 * d_alpha * float(g_l2) + a64 ** 2 * d_gl2 + 3 * U * a64 ** 2 * float(g_l2) + U * abs(float(D))
        gap = rows_gap + ridge + cols
        d_gap = d_rows + d_ridge + d_cols + 2 * U * float(gap)
    else:
        Pv = f + g_l1
        d_P = d_f + d_gl1 + U * abs(float(Pv))
        D, d_D = D_loss, d_Dl
        gap = rows_gap + cols
        d_gap = d_rows + d_cols + U * float(gap)
    vals = dict(primal=Pv, dual=D, gap=gap, alpha=alpha, grad_inf=G, f=f, g_l1=g_l1, rows_gap=rows_gap)
    bounds = dict(primal=d_P, dual=d_D, gap=d_gap, alpha=d_alpha, grad_inf=dG + U * float(G), f=d_f, g_l1=d_gl1, rows_gap=d_rows)
    if l2 > 0:
        vals.update(g_l2=g_l2, ridge_gap=ridge)
        bounds.update(g_l2=d_gl2, ridge_gap=d_ridge)
    bounds = {k: 2 * float(b) for k, b in bounds.items()}
    extra = dict(gap_pd=Pv - D, grad=gt, dgrad=2 * dgt, terms=wt, wpsi=wpsi, dwpsi=2 * dwpsi, Z=Z, oma=oma)
    return vals, bounds, extra


def worst_ratio(got, vals, bounds):
    """{key: |got - value| / bound} over the keys of ``vals`` (0 / 0 counts as 0); ``got``: an object with the keys as attributes or a dict."""
    out = {}
    for k in vals:
        have = got[k] if isinstance(got, dict) else getattr(got, k)
        err = abs(float(np.longdouble(have) - vals[k]))
        out[k] = 0.0 if err == 0.0 else (err / bounds[k] if bounds[k] > 0 else np.inf)
    return out


def gap_numpy(ref, x):
    """The certificate in plain fp64 NumPy from the closures of ``ref`` (MultinomialRef, no factors): a dict over KEYS8 (KEYS10 with
    l2 > 0), rows and D in the kernel's forms."""
    X = np.asarray(x, float).reshape(ref.n, ref.K)
    Z = np.asarray(ref.A @ X)
    d = Z - Z.max(axis=1, keepdims=True)
    e = np.exp(d)
    S = e.sum(axis=1)
    p = e / S[:, None]
    on = np.ones(ref.m, bool) if ref.w is None else ref.w != 0
    wv = np.ones(ref.m) if ref.w is None else ref.w
    Yv = np.where(on[:, None], ref.Y, 0.0)
    g = ref.jac_f(x)
    gt = g + ref.l2 * X.reshape(-1) if ref.l2 > 0 else g
    G = np.max(np.abs(gt))
    alpha, oma = (ref.lam / G, (G - ref.lam) / G) if G > ref.lam else (1.0, 0.0)
    v = alpha * p + oma * Yv
    with np.errstate(divide="ignore", invalid="ignore"):
        lv = np.where(v > 0, np.log(np.where(v > 0, v, 1.0)), 0.0)
        kl = np.maximum(np.sum(np.where(v > 0, v * (lv - (d - np.log(S)[:, None])), 0.0), axis=1), 0.0) if oma != 0 else np.zeros(ref.m)
    rows = ref.scale * np.sum(np.where(on, wv * kl, 0.0))
    D = -ref.scale * np.sum(np.where(on, wv * np.sum(v * lv, axis=1), 0.0))
    xf = X.reshape(-1)
    cols = np.sum(np.maximum(ref.lam * np.abs(xf) + alpha * gt * xf, 0.0))
    f, g1 = ref.f(x), ref.lam * np.sum(np.abs(xf))
    out = dict(primal=f + g1, dual=D, gap=rows + cols, alpha=alpha, grad_inf=G, f=f, g_l1=g1, rows_gap=rows)
    if ref.l2 > 0:
        g2 = ref.l2 / 2 * np.sum(xf * xf)
        out.update(primal=f + g1 + g2, dual=D - alpha * alpha * g2, gap=rows + oma * oma * g2 + cols, g_l2=g2, ridge_gap=oma * oma * g2)
    return out
