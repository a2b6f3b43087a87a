"""Poisson-regression inputs, NumPy reference closures, the long-double restatement of the row kernels and of the certificate
with first-order rounding bounds for every output - shared by the Poisson tests and their fixture script (no test in here;
tests/test_poisson_reference.py proves the restatements on the CPU).

    f(x) = scale sum_i w_i (exp(z_i) - b_i z_i),  z = A x,  counts b_i >= 0   (the constant log b! is dropped),   scale = 1
    grad f = scale A^T (w o psi),   psi_i = exp(z_i) - b_i
    the arithmetic of every kernel and of PoissonRef:   e = exp(z),  psi = e - b,  phi = e - b * z,  a plain sum, times scale once
    a margin beyond the range of exp: e = phi = f = +inf (never NaN); a NaN margin: NaN
    g(x) = lam |x|_1 + (l2 / 2) sum x^2 (+ box) as enet_cases.EnetRef

Inputs (make_poisson): A of sparse_cases.make_sparse; rng = default_rng(seed + 2000); x_true[:k] = 0.3 N(0, 1) with k as in
make_sparse; b = rng.poisson(exp(clip(A x_true, -30, 6))); lam = 0.1 |A^T (1 - b)|_inf (= 0.1 lam_max at scale 1).

The certificate.  h(z) = e^z - b z,  h' = e^z - b,  h^*(u) = v log v - v with v = u + b >= 0 (0 log 0 = 0; +inf for v < 0).
nu = alpha grad phi(z), alpha = min(1, lam / |g|_inf):  v = alpha e^z + (1 - alpha) b >= 0 always, so nu is feasible.

    D = -scale sum w_i (v_i log v_i - v_i)
    Fenchel-Young gap of row i:  h(z) + h^*(u) - u z = e^z - v + v (log v - z) = e^z ((1 + d) log1p(d) - d),
                                 d = v / e^z - 1 = (1 - alpha)(b - e^z) / e^z >= -1        (>= 0; exactly 0 when alpha = 1: d = 0)
                                 b = 0:  e^z (alpha log alpha + 1 - alpha)
    rows = scale sum w_i [that];   columns, alpha, 1 - alpha, alpha log alpha, the ridge part and gt = g + l2 x: gap_cases / enet_cases
    gap = rows (+ ridge) + columns

Rounding bounds: the symbols of tests/gap_cases.py (u = 2^-53, gamma_k, ds_i the error of the device's margin, the safety factor 2
on every bound).  The device's exp carries the allowance of the logistic bound (tests/test_gpu_logistic.py): 1 ulp <= 2 u relative.

  e         e^ = exp(z^) (1 + eps), |eps| <= 2 u, and exp(z + ds) = e (1 + ds) to first order:      de_i = e_i (ds_i + 2 u)
  psi       one subtraction:                                                                         dpsi_i = de_i + u |psi_i|
  phi       b z^: |b| ds + u |b z|; one subtraction:                                  dphi_i = de_i + |b_i| ds_i + u |b_i z_i| + u |phi_i|
  weights   one product each: d(w psi)_i = w_i dpsi_i + u |w_i psi_i|, d(w phi)_i = w_i dphi_i + u |w_i phi_i|  (w = 1: no product, same bound kept)
  f         scale sum:   d(f) = scale (sum d(w phi)_i + gamma_m sum |w_i phi_i|) + u |f|        (phi_i may be negative: absolute values)
  g         scale A^T (w psi):   dg_j = scale ((|A|^T d(w psi))_j + gamma_(m+2) (|A|^T |w psi|)_j)
  scaling   gap_cases: d(alpha), d(oma), d(aloga) = d(alpha) |log alpha| + d(oma) + 4 u |alpha log alpha|
  v         alpha e + oma b, two products and one sum of non-negative terms:   dv_i = d(alpha) e + alpha de + d(oma) b + 2 u v
  conjugate c_i = v log v - v, dc/dv = log v; log: 2 u relative; one product, one subtraction:
            d(c_i) = dv |log v| + 3 u |v log v| + u |c_i|;    D = -scale sum w c:  d(D) = scale (sum w d(c_i) + gamma_(m+1) sum w |c_i|) + u |D|
  row gap   the kernel's three forms (zf_kernels_gap.h), each bounded in its own terms:
            b = 0      t = e (aloga + oma):        dt = de |aloga + oma| + e (d(aloga) + d(oma) + u (|aloga| + oma)) + u t
            d <= 1     d = oma (b - e) / e:        d(d) = (d(oma) |b - e| + oma (de + u |b - e|)) / e + |d| de / e + 2 u |d|
                       vr = alpha + oma (b / e):   d(vr) = d(alpha) + d(oma) b / e + oma (b / e)(de / e + u) + 2 u vr
                       L = log1p(d), vr = 1 + d:   d(vr L) = d(vr) |L| + d(d) + 2 u |vr L|   (vr dL = vr d(d) / (1 + d) = d(d))
                       inner = vr L - d:           d(inner) = d(vr) |L| + 2 d(d) + 3 u |vr L| + u |inner|
                       t = e inner:                dt = de |inner| + e d(inner) + u t
            d > 1      t = (e - v) + v (log v - z):  q = log v - z, dq = dv / v + 2 u |log v| + ds + u |q|
                                                   dt = de + dv + u |e - v| + dv |q| + v dq + u |v q| + u t
            a row within d(d) of the branch point d = 1 may take either form on the device: the larger of the two bounds.
            rows = scale sum w t:  d(rows) = scale (sum w dt_i + gamma_(m+1) sum w t_i) + u rows
            alpha = 1 in exact arithmetic (G <= lam) but not certainly on the device (G + dG > lam): the device's 1 - alpha is at
            most d(oma), and a row term is of second order in it, e d^2 / 2 with |d| <= d(oma) |b - e| / e; the bound keeps the
            first-order expression e (d(aloga) + d(oma)) + d(oma) |b - e| (1 + |z|), which is larger.
            (the parts of (1 + d) log1p(d) - d cancel to second order in d; the bound is in those parts - the gap's own terms)
  P, gap    l2 = 0: gap_cases' lines (one addition each); l2 > 0: enet_cases' (two)
  underflow exp below 2^-1022 loses its relative accuracy: m 2^-1022 is added to every bound a row sum enters.
"""
import numpy as np
import scipy.sparse as sp

import gap_cases as GC
import sparse_cases as S
from oracle import problems_ref as P

U = GC.U
KEYS8 = GC.KEYS
KEYS10 = GC.KEYS + ("g_l2", "ridge_gap")
SMALL, TALL = S.SMALL, S.TALL
FORMS = ("csr", "dense")
SCALE = 1.0
LAM_FRACTION = 0.1
OVERFLOW_CASE = SMALL[1]   # 2000 x 5000: the first trial from lr = 1 has a margin beyond the range of exp (f = +inf)
GAP_CASE = SMALL[2]        # 1000 x 257: the case a first-order method brings to a small gap (gap_tol, l1_path, l1_cv)


def poisson_terms(z, b):
    """(psi, phi) of margins z in the arithmetic of the kernels (any float dtype): ONE exp per row."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(z)
        return e - b, e - b * z


def make_poisson(m, n, density, seed):
    """(A csr, counts b, lam) of one (m, n, density, seed)."""
    A, _, _ = S.make_sparse(m, n, density, seed)
    rng = np.random.default_rng(seed + 2000)
    x_true = np.zeros(n)
    k = max(1, min(20, n // 4))
    x_true[:k] = 0.3 * rng.standard_normal(k)
    b = rng.poisson(np.exp(np.clip(A @ x_true, -30.0, 6.0))).astype(np.float64)
    lam = LAM_FRACTION * float(np.max(np.abs(A.T @ (1.0 - b))))
    return A, b, lam


def matrix(A, storage):
    return A if storage == "csr" else A.toarray()


class PoissonRef:
    """The four closures of a Poisson problem on either storage form, NumPy / SciPy in fp64.  ``reverse``: the rows in reversed
    order - the same numbers summed the other way round (f and A^T psi)."""

    def __init__(self, A, b, lam, scale=SCALE, bounds=None, l2=0.0, sample_weight=None, reverse=False):
        self.A = sp.csr_matrix(A, dtype=np.float64) if sp.issparse(A) else np.asarray(A, float)
        self.b = np.asarray(b, float)
        self.w = None if sample_weight is None else np.asarray(sample_weight, float)
        if reverse:
            self.A, self.b = self.A[::-1], self.b[::-1].copy()
            if sp.issparse(self.A):
                self.A = sp.csr_matrix(self.A)
            if self.w is not None:
                self.w = self.w[::-1].copy()
        self.lam, self.scale, self.l2 = float(lam), float(scale), float(l2)
        self.bounds = None if bounds is None else (float(bounds[0]), float(bounds[1]))

    def _rows(self, x):
        psi, phi = poisson_terms(self.A @ x, self.b)
        if self.w is not None:   # (a row with w_i = 0 is a row that is not there)
            on = self.w != 0.0
            psi, phi = np.where(on, self.w * np.where(on, psi, 0.0), 0.0), np.where(on, self.w * np.where(on, phi, 0.0), 0.0)
        return psi, phi

    def f(self, x):
        return self.scale * np.sum(self._rows(x)[1])

    def jac_f(self, x):
        return self.scale * (self.A.T @ self._rows(x)[0])

    def g(self, x):
        if self.bounds is not None and ((x < self.bounds[0]).any() or (x > self.bounds[1]).any()):
            return np.inf
        out = self.lam * np.linalg.norm(x, ord=1)
        return out + (self.l2 / 2) * np.sum(x * x) if self.l2 > 0 else out

    def prox_wsum_g(self, weight, x):
        x = P.soft_threshold(x, self.lam * weight)
        if self.l2 > 0:
            x = x * (1.0 / (1.0 + self.l2 * weight))
        if self.bounds is not None:
            x = P.clip_box(x, self.bounds[0], self.bounds[1])
        return x

    def callbacks(self):
        return self.f, self.g, self.jac_f, self.prox_wsum_g


def case_weights(case):
    """Seeded row weights of a case: an exposure in [0.5, 2) with a tenth of the rows switched off (w = 0)."""
    rng = np.random.default_rng(case[3] + 3000)
    w = 0.5 + 1.5 * rng.random(case[0])
    w[rng.choice(case[0], max(1, case[0] // 10), replace=False)] = 0.0
    return w


# the fixture's solves (80 iterations from lr = 1, return_all): every SMALL shape x storage form x ISTA / FISTA with l2 = 0, and
# one elastic-net variant per shape - FISTA with l2 = lam on the CSR matrix (the layout of G17)
GOLDEN_VARIANTS = {
    "ista": dict(nesterov=False),
    "fista": dict(nesterov=True, nesterov_ratio=(0, 0.25)),
}
GOLDEN_KW = dict(lr=1, tol=0.0, max_iter=80, return_all=True)
GOLDEN_STRIDE = 7
GOLDEN_SOLVES = [(0, st, tag) for st in FORMS for tag in GOLDEN_VARIANTS] + [(1, "csr", "fista")]   # (fi, storage, tag): l2 = fi * lam


def golden_prefix(ci, fi, storage, tag):
    return f"poisson.c{ci}.l{fi}.{storage}.{tag}"


def _need_longdouble():
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError("np.longdouble carries fewer than 63 mantissa bits here: an fp64 evaluation cannot be checked against it")


# ---- the row kernels ---------------------------------------------------------------------------------------------------------------
def loss_longdouble(z, b, scale, w=None, ds=None):
    """The outputs of the row kernels at margins z (fp64 values, taken as exact unless ``ds`` bounds their error):
    (f, bound of f, w o psi, bound of every element of it), f and psi in longdouble, the bounds with the safety factor 2."""
    _need_longdouble()
    ld = np.longdouble
    z64, b64 = np.asarray(z, np.float64), np.asarray(b, np.float64)
    m = z64.size
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    ds = np.zeros(m) if ds is None else np.asarray(ds, np.float64)
    on = np.ones(m, bool) if w is None else np.asarray(w) != 0.0
    wl = np.ones(m, dtype=ld) if w is None else np.asarray(w, np.float64).astype(ld)
    zl, bl = z64.astype(ld), np.where(on, b64, 0.0).astype(ld)
    e = np.exp(zl)
    psi, phi = e - bl, e - bl * zl
    de = f64(e) * (ds + 2 * U)
    dpsi = de + U * f64(np.abs(psi))
    dphi = de + f64(np.abs(bl)) * ds + U * f64(np.abs(bl * zl)) + U * f64(np.abs(phi))
    wpsi, wphi = np.where(on, wl * psi, ld(0)), np.where(on, wl * phi, ld(0))
    dwpsi = np.where(on, f64(wl) * dpsi + U * f64(np.abs(wpsi)), 0.0)
    dwphi = np.where(on, f64(wl) * dphi + U * f64(np.abs(wphi)), 0.0)
    f = ld(scale) * np.sum(wphi)
    d_f = scale * (float(np.sum(dwphi)) + GC._gamma(m) * float(np.sum(np.abs(wphi)))) + U * abs(float(f)) + m * 2.0 ** -1022
    return f, 2 * d_f, wpsi, 2 * dwpsi


def psi_allowance(z, b):
    """How far the device's psi may lie from NumPy's np.exp(z) - b: both exps within 1 ulp <= 2 u of the exact one (4 u e
    between them), and one rounding of the subtraction on either side."""
    with np.errstate(over="ignore"):
        e = np.exp(np.asarray(z, np.float64))
    return 4 * U * e + 2 * U * np.abs(e - b)


# ---- the certificate ---------------------------------------------------------------------------------------------------------------
def row_gap_longdouble(e, z, bl, alpha, oma, aloga):
    """(terms, d, v): the Fenchel-Young gap of every row in the cancellation-free form, longdouble."""
    ld = np.longdouble
    v = alpha * e + oma * bl
    d = oma * (bl - e) / e
    with np.errstate(divide="ignore", invalid="ignore"):
        vr = alpha + oma * (bl / e)
        inner = np.where(vr > 0, vr * np.log1p(np.maximum(d, ld(-1))), ld(0)) - d
        direct = (e - v) + v * (np.log(np.where(v > 0, v, ld(1))) - z)
    t = np.where(bl == 0, e * (aloga + oma), np.where(d <= 1, e * inner, direct))
    return np.maximum(t, ld(0)), d, v


def gap_longdouble(A, b, x, lam, scale=SCALE, l2=0.0, w=None):
    """(values, bounds, extra) as huber_cases.gap_longdouble for the Poisson loss: over KEYS8 when l2 = 0, KEYS10 otherwise.
    extra: ``gap_pd`` = P - D in longdouble, ``grad`` (gt), ``cols``, ``col_terms``, ``terms`` (the row gaps), ``z``."""
    _need_longdouble()
    ld = np.longdouble
    _gamma = GC._gamma
    A = GC._csr(A)
    m, n = A.shape
    rows = np.repeat(np.arange(m), np.diff(A.indptr))
    data = A.data.astype(ld)
    on = np.ones(m, bool) if w is None else np.asarray(w) != 0.0
    wl = np.ones(m, dtype=ld) if w is None else np.asarray(w, np.float64).astype(ld)
    w64 = np.asarray(wl, dtype=np.float64)
    xl = np.asarray(x, np.float64).astype(ld)
    bl = np.where(on, np.asarray(b, np.float64), 0.0).astype(ld)
    lam_l, sc, l2_l = ld(lam), ld(scale), ld(l2)
    z = np.zeros(m, dtype=ld)
    np.add.at(z, rows, data * xl[A.indices])
    absA = abs(A)
    ax = np.abs(np.asarray(x, np.float64))
    ds = _gamma(n) * (absA @ ax)
    tiny = m * 2.0 ** -1022
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    # ---- rows: psi, phi, f
    e = np.exp(z)
    psi, phi = e - bl, e - bl * z
    e64 = f64(e)
    de = e64 * (ds + 2 * U)
    dpsi = de + U * f64(np.abs(psi))
    dphi = de + f64(np.abs(bl)) * ds + U * f64(np.abs(bl * z)) + U * f64(np.abs(phi))
    wpsi, wphi = np.where(on, wl * psi, ld(0)), np.where(on, wl * phi, ld(0))
    dwpsi = np.where(on, w64 * dpsi + U * f64(np.abs(wpsi)), 0.0)
    dwphi = np.where(on, w64 * dphi + U * f64(np.abs(wphi)), 0.0)
    f = sc * np.sum(wphi)
    d_f = scale * (float(np.sum(dwphi)) + _gamma(m) * float(np.sum(np.abs(wphi)))) + U * abs(float(f)) + tiny
    # ---- g = scale A^T (w psi), gt = g + l2 x, the scaling
    g = np.zeros(n, dtype=ld)
    np.add.at(g, A.indices, data * wpsi[rows])
    g *= sc
    dg = float(scale) * (absA.T @ dwpsi + _gamma(m + 2) * (absA.T @ f64(np.abs(wpsi)))) + tiny
    if l2 > 0:
        gt = g + l2_l * xl
        dgt = dg + U * f64(np.abs(gt))
    else:
        gt, dgt = g, dg
    G = np.max(np.abs(gt)) if n else ld(0)
    dG = float(np.max(dgt)) if n else 0.0
    if G > lam_l:
        alpha, oma = lam_l / G, (G - lam_l) / G
    else:
        alpha, oma = ld(1), ld(0)
    big = max(float(G), float(lam))
    d_alpha = (dG / big + U) if big > 0 else 0.0
    d_oma = (2 * dG / big + 2 * U * float(oma)) if big > 0 else 0.0
    if float(G) * (1 + 2 * U) + dG <= float(lam):
        d_alpha = d_oma = 0.0   # no fp64 evaluation inside dG of g can leave the branch alpha = 1, 1 - alpha = 0: both are exact
    aloga = alpha * np.log(alpha) if alpha > 0 else ld(0)
    d_aloga = d_alpha * abs(float(np.log(alpha))) + d_oma + 4 * U * abs(float(aloga)) if alpha > 0 else 0.0
    # ---- columns, g_l1, the ridge part
    tj = lam_l * np.abs(xl) + alpha * gt * xl
    cols = np.sum(tj)
    d_t = ax * (d_alpha * f64(np.abs(gt)) + float(alpha) * dgt + U * float(alpha) * f64(np.abs(gt)) + U * float(lam)) + U * f64(np.abs(tj))
    d_cols = float(np.sum(d_t)) + _gamma(n) * float(np.sum(np.abs(tj)))
    asum = np.sum(np.abs(xl))
    g_l1 = lam_l * asum
    d_gl1 = float(lam) * _gamma(n + 1) * float(asum)
    xx = np.sum(xl * xl)
    g_l2 = l2_l / 2 * xx
    d_gl2 = float(l2) / 2 * _gamma(n + 1) * float(xx) + U * float(g_l2)
    ridge = oma * oma * g_l2
    d_ridge = 2 * float(oma) * d_oma * float(g_l2) + float(oma) ** 2 * d_gl2 + 4 * U * float(ridge)
    # ---- the conjugate and the dual
    a64, o64, al64 = float(alpha), float(oma), float(aloga)
    b64 = f64(bl)
    v = alpha * e + oma * bl
    v64 = f64(v)
    dv = d_alpha * e64 + a64 * de + d_oma * b64 + 2 * U * v64
    with np.errstate(divide="ignore", invalid="ignore"):
        logv = np.where(v > 0, np.log(np.where(v > 0, v, ld(1))), ld(0))
    lv64 = f64(np.abs(logv))
    conj = v * logv - v
    d_conj = dv * lv64 + 3 * U * f64(np.abs(v * logv)) + U * f64(np.abs(conj))
    D_loss = -sc * np.sum(np.where(on, wl * conj, ld(0)))
    d_Dl = (scale * (float(np.sum(np.where(on, w64 * d_conj, 0.0))) + _gamma(m + 1) * float(np.sum(np.where(on, w64 * f64(np.abs(conj)), 0.0))))
            + U * abs(float(D_loss)) + tiny)
    # ---- the row gaps
    if oma > 0:
        t_i, d, _ = row_gap_longdouble(e, z, bl, alpha, oma, aloga)
        d64, t64 = f64(d), f64(t_i)
        bme = f64(np.abs(bl - e))
        boe = b64 / e64
        # b = 0
        dt_zero = de * abs(al64 + o64) + e64 * (d_aloga + d_oma + U * (abs(al64) + o64)) + U * t64
        # d <= 1
        d_d = (d_oma * bme + o64 * (de + U * bme)) / e64 + np.abs(d64) * de / e64 + 2 * U * np.abs(d64)
        vr = a64 + o64 * boe
        d_vr = d_alpha + d_oma * boe + o64 * boe * (de / e64 + U) + 2 * U * vr
        with np.errstate(divide="ignore", invalid="ignore"):
            L = np.where(d64 > -1, np.abs(np.log1p(np.maximum(d64, -1.0))), 0.0)
        vrL = np.where(vr > 0, vr * L, 0.0)
        inner = np.abs(f64(t_i / e))
        d_inner = d_vr * L + 2 * d_d + 3 * U * vrL + U * inner
        dt_small = de * inner + e64 * d_inner + U * t64
        # d > 1
        q = f64(np.abs(logv - z))
        with np.errstate(divide="ignore", invalid="ignore"):
            dq = np.where(v64 > 0, dv / np.where(v64 > 0, v64, 1.0), 0.0) + 2 * U * lv64 + ds + U * q
        dt_direct = de + dv + U * f64(np.abs(e - v)) + dv * q + v64 * dq + U * v64 * q + U * t64
        with np.errstate(invalid="ignore"):
            near = np.abs(d64 - 1.0) <= 2 * d_d
            dt = np.where(b64 == 0, dt_zero, np.where(near, np.maximum(dt_small, dt_direct), np.where(d64 <= 1, dt_small, dt_direct)))
    else:
        t_i = np.zeros(m, dtype=ld)
        # alpha = 1 exactly on every evaluation inside dG when d_oma = 0; otherwise the device may form terms of the size d_oma allows
        dt = np.zeros(m) if d_oma == 0.0 else e64 * (d_aloga + d_oma) + d_oma * f64(np.abs(bl - e)) * (1 + f64(np.abs(z)))
    wt = np.where(on, wl * t_i, ld(0))
    rows_gap = sc * np.sum(wt)
    d_rows = scale * (float(np.sum(np.where(on, w64 * dt, 0.0))) + _gamma(m + 1) * float(np.sum(wt))) + U * float(rows_gap)
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
    bounds = {k: 2 * float(v) for k, v in bounds.items()}
    extra = dict(gap_pd=Pv - D, grad=gt, cols=cols, col_terms=tj, terms=wt, z=z, zero_share=float(np.mean(f64(bl) == 0)))
    return vals, bounds, extra


def primal_longdouble(A, b, x, lam, scale=SCALE, l2=0.0, w=None):
    return gap_longdouble(A, b, x, lam, scale, l2, w)[0]["primal"]


def worst_ratio(got, vals, bounds):
    """{key: |got - value| / bound} over the keys of ``vals`` (0 / 0 counts as 0)."""
    out = {}
    for k in vals:
        err = abs(float(np.longdouble(getattr(got, k)) - vals[k]))
        out[k] = 0.0 if err == 0.0 else (err / bounds[k] if bounds[k] > 0 else np.inf)
    return out


def lam_max(A, b, scale=SCALE, w=None):
    """scale |A^T (w o (1 - b))|_inf in longdouble."""
    return float(gap_longdouble(A, b, np.zeros(A.shape[1]), 1.0, scale, 0.0, w)[0]["grad_inf"])


def fista(A, b, lam, x0, iters, scale=SCALE, record=()):
    """Backtracking FISTA in fp64 (exp is not globally Lipschitz: the step halves until the quadratic model holds, and a
    non-finite trial is rejected).  Returns (x, {k: x_k})."""
    A = GC._csr(A)
    At = A.T.tocsr()
    b = np.asarray(b, dtype=np.float64)
    fval = lambda v: scale * float(np.sum(poisson_terms(A @ v, b)[1]))
    x = np.array(x0, dtype=np.float64)
    y, t, kept, step = x.copy(), 1.0, {}, 1.0
    for k in range(1, iters + 1):
        grad = scale * (At @ poisson_terms(A @ y, b)[0])
        fy = fval(y)
        while True:
            wv = y - step * grad
            xn = np.sign(wv) * np.maximum(np.abs(wv) - step * lam, 0.0)
            dx = xn - y
            if fval(xn) <= fy + float(grad @ dx) + float(dx @ dx) / (2 * step) + 1e-12 * abs(fy):
                break
            step *= 0.5
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        y = xn + ((t - 1.0) / tn) * (xn - x)
        x, t = xn, tn
        if k in record:
            kept[k] = x.copy()
    return x, kept
