"""Huber-loss inputs, NumPy reference closures, the long-double restatement of the certificate with first-order rounding bounds
for every output, and the exact screening rule with its guard - shared by the Huber tests and their fixture script (no test in
here; tests/test_huber_reference.py proves the restatements on the CPU).

    f(x) = scale sum_i H(r_i),  r = A x - b,   H(r) = r^2 (|r| <= delta) | delta (2 |r| - delta) (beyond),   scale = 1/2
    grad f = 2 scale A^T c,   c = clip(r, -delta, delta)
    the arithmetic of every kernel and of HuberRef:   c = copysign(min(|r|, delta), r),   H = c (2 r - c)
    g(x) = lam |x|_1 + (l2 / 2) sum x^2 (+ box) as enet_cases.EnetRef

Inputs: A and b of sparse_cases.make_sparse; a seeded tenth of the rows of b gets an outlier of +-5 std(b); delta is a quantile
of |b| (the median unless QUANTILE says otherwise); lam = LAM_FRACTION lam_max with lam_max = 2 scale |A^T clip(-b)|_inf.

The certificate.  phi_i(z) = scale H(z - b_i),  phi_i' = 2 scale c_i,  phi_i^*(nu) = nu b_i + nu^2 / (4 scale) on |nu| <= 2 scale
delta (+inf beyond).  nu = alpha 2 scale c stays inside that interval because |c_i| <= delta and alpha <= 1:

    D = -sum phi_i^*(nu_i) = -scale (alpha^2 sum c^2 + 2 alpha sum b c)
    Fenchel-Young gap of row i:  phi(z) + phi^*(nu) - nu z = scale (H + alpha^2 c^2 - 2 alpha c r)
                                 = scale (1 - alpha) ((1 - alpha) c^2 + 2 |c| (|r| - |c|))        (H = 2 c r - c^2, c r = |c| |r|)
    rows = scale (1 - alpha) ((1 - alpha) sum c^2 + 2 T),   T = sum |c_i| (|r_i| - |c_i|)   (every term >= 0; 0 on an unclipped row)
    columns, alpha, 1 - alpha, the ridge part and gt = g + l2 x:  gap_cases / enet_cases;   gap = rows (+ ridge) + columns

Rounding bounds: the lines of tests/gap_cases.py and tests/enet_cases.py (same symbols, u = 2^-53, gamma_k, the safety factor 2),
with the least-squares lines replaced by these.  dr_i = ds_i + u |r_i| is the error of the device's r_i (gap_cases).  Every
function of r below is evaluated at the device's r^, so its error is (a Lipschitz constant on [r - dr, r + dr]) dr plus its
own roundings; cu_i = min(|r_i| + dr_i, delta) >= |c| on that interval - it covers a row whose perturbation crosses delta.

  c         the clip is exact (min and copysign round nothing) and 1-Lipschitz:   dc_i = dr_i
  H         H' = 2 c:  |H(r^) - H(r)| <= 2 cu dr.  H = c (2 r^ - c): 2 r^ exact, one subtraction, one product, and 2 r - c has
            the sign of c and at least its size (no cancellation):  dH_i = 2 cu_i dr_i + 2 u H_i
  f         scale sum H:   d(f) = scale (sum dH_i + gamma_m sum H) + u f
  sum c^2   d(cc) = sum 2 cu_i dr_i + gamma_(m+1) cc;      sum b c:  d(bc) = sum |b_i| dr_i + gamma_(m+1) sum |b_i c_i|
  T         t(r) = |c| (|r| - |c|) is cu-Lipschitz (0 inside, slope delta beyond); |r^| - |c| and the product round once each:
            d(T) = sum (cu_i dr_i + 2 u t_i) + gamma_m T
  g         2 scale A^T c:  dg_j = 2 scale ((|A|^T dc)_j + gamma_(m+2) (|A|^T |c|)_j)         (gap_cases' line with c for r)
  rows      scale oma (oma cc + 2 T): inner = oma cc + 2 T, d(inner) = d(oma) cc + oma d(cc) + 2 d(T);
            d(rows) = scale (d(oma) inner + oma d(inner)) + 4 u rows
  D         gap_cases' least-squares line with cc, bc for rr, br
  P, gap    l2 = 0: gap_cases' lines (one addition each); l2 > 0: enet_cases' (two)

The screening rule is tests/screen_cases.py's with L = 2 scale (H' = 2 c is 2-Lipschitz, so phi' is 2 scale-Lipschitz).  The
guard, line by line, with c = clip(r) for the dual candidate:

  margins   |dz|_2 <= R u |A|_F S1                                                  (the matrix alone: unchanged)
  candidate the device forms r^_i = fl(z^_i - b_i) and clips it exactly.  The clip is 1-Lipschitz, so the error of the margins
            passes at most unchanged: |clip(z^ - b) - clip(z - b)| <= dz_i.  The rounding of the subtraction moves r by at
            most u |r^_i|, and the clip passes at most min(that, what is left of the interval): if |r^_i| <= delta then
            |c^_i| = |r^_i| and the contribution is u |c^_i|; if |r^_i| > delta and the unrounded value too, it is 0; if the
            rounding crossed delta, the unrounded value lies in [delta (1 - u), delta] and the contribution is at most
            u delta = u |c^_i|.  In every case  dc_i <= dz_i + u |c_i|  (first order), so
                |dc|_2 <= |dz|_2 + u |c|_2,   |c|_2 = sqrt(sum c^2)
            - the least-squares line with c in place of r.
  gradient, scaling, left side, radius:  the lines of screen_cases with gfac = 2 scale and |c|_2 = sqrt(sum c^2)
  E = 2 X + 2^-20 r
"""
import numpy as np
import scipy.sparse as sp

import gap_cases as GC
import screen_cases as SC
import sparse_cases as S
from oracle import problems_ref as P

U = GC.U
KEYS8 = GC.KEYS
KEYS10 = GC.KEYS + ("g_l2", "ridge_gap")
SMALL, TALL = S.SMALL, S.TALL
FORMS = ("csr", "dense")
SCALE = 0.5
LAM_FRACTION = 0.1
QUANTILE = {}            # case -> quantile of |b| for delta where the median leaves the clipped share outside SHARE
SHARE = (0.05, 0.95)     # the clipped share every case must have at x0 = 0 and at the fixture's last iterate


def huber_terms(r, delta):
    """(c, H) of residuals r in the arithmetic of the kernels (any float dtype)."""
    c = np.copysign(np.minimum(np.abs(r), delta), r)
    return c, c * (2 * r - c)


def make_huber(case):
    """(A csr, b with outliers, lam, delta) of one (m, n, density, seed)."""
    A, b, _ = S.make_sparse(*case)
    m = A.shape[0]
    rng = np.random.default_rng(case[3] + 1000)
    rows = rng.choice(m, max(1, m // 10), replace=False)
    b = b.copy()
    b[rows] += rng.choice([-1.0, 1.0], rows.size) * 5.0 * np.std(b)
    delta = float(np.quantile(np.abs(b), QUANTILE.get(tuple(case), 0.5)))
    c0, _ = huber_terms(-b, delta)
    lam = LAM_FRACTION * float(np.max(np.abs((2 * SCALE) * (A.T @ c0))))
    return A, b, lam, delta


def matrix(A, storage):
    return A if storage == "csr" else A.toarray()


def clipped_share(A, b, x, delta):
    return float(np.mean(np.abs(A @ np.asarray(x, float) - b) > delta))


class HuberRef:
    """The four closures of a Huber problem on either storage form, NumPy / SciPy in fp64."""

    def __init__(self, A, b, lam, delta, scale=SCALE, bounds=None, l2=0.0):
        self.A = sp.csr_matrix(A, dtype=np.float64) if sp.issparse(A) else np.asarray(A, float)
        self.b = np.asarray(b, float)
        self.lam, self.delta, self.scale, self.l2 = float(lam), float(delta), float(scale), float(l2)
        self.bounds = None if bounds is None else (float(bounds[0]), float(bounds[1]))

    def f(self, x):
        r = self.A @ x - self.b
        return self.scale * np.sum(huber_terms(r, self.delta)[1])

    def jac_f(self, x):
        r = self.A @ x - self.b
        return (2 * self.scale) * (self.A.T @ huber_terms(r, self.delta)[0])

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


# the fixture's solves (80 iterations from lr = 1, return_all): every SMALL shape x storage form x ISTA / FISTA with l2 = 0, and
# one elastic-net variant per shape - FISTA with l2 = lam on the CSR matrix
GOLDEN_VARIANTS = {
    "ista": dict(nesterov=False),
    "fista": dict(nesterov=True, nesterov_ratio=(0, 0.25)),
}
GOLDEN_KW = dict(lr=1, tol=0.0, max_iter=80, return_all=True)
GOLDEN_STRIDE = 7
GOLDEN_SOLVES = [(0, st, tag) for st in FORMS for tag in GOLDEN_VARIANTS] + [(1, "csr", "fista")]   # (fi, storage, tag): l2 = fi * lam


def golden_prefix(ci, fi, storage, tag):
    return f"huber.c{ci}.l{fi}.{storage}.{tag}"


# ---- the row kernels ---------------------------------------------------------------------------------------------------------------
def loss_longdouble(z, b, delta, scale, ds=None):
    """The outputs of the row kernels at margins z (fp64 values, taken as exact unless ``ds`` bounds their error):
    (f, bound of f, c, bound of every c_i), f and c in longdouble, the bounds with the safety factor 2."""
    ld = np.longdouble
    z64 = np.asarray(z, np.float64)
    m = z64.size
    r = z64.astype(ld) - np.asarray(b, np.float64).astype(ld)
    c, H = huber_terms(r, ld(delta))
    f = ld(scale) * np.sum(H)
    ds = np.zeros(m) if ds is None else np.asarray(ds, np.float64)
    dr = ds + U * np.abs(r).astype(np.float64)
    cu = np.minimum(np.abs(r).astype(np.float64) + dr, delta)
    dH = 2 * cu * dr + 2 * U * H.astype(np.float64)
    d_f = scale * (float(np.sum(dH)) + GC._gamma(m) * float(np.sum(H))) + U * float(f)
    return f, 2 * d_f, c, 2 * dr


# ---- the certificate ---------------------------------------------------------------------------------------------------------------
def gap_longdouble(A, b, x, lam, delta, scale=SCALE, l2=0.0):
    """(values, bounds, extra) as enet_cases.gap_longdouble for Huber's loss: over KEYS8 when l2 = 0, KEYS10 otherwise.  extra:
    ``gap_pd`` = P - D in longdouble, ``grad`` (gt), ``cols``, ``cc`` = sum c^2, ``T``, ``share`` (the clipped rows' share)."""
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError("np.longdouble carries fewer than 63 mantissa bits here: an fp64 evaluation cannot be checked against it")
    ld = np.longdouble
    _gamma = GC._gamma
    A = GC._csr(A)
    m, n = A.shape
    rows = np.repeat(np.arange(m), np.diff(A.indptr))
    data = A.data.astype(ld)
    xl, bl = np.asarray(x, np.float64).astype(ld), np.asarray(b, np.float64).astype(ld)
    lam_l, sc, l2_l, dl = ld(lam), ld(scale), ld(l2), ld(delta)
    z = np.zeros(m, dtype=ld)
    np.add.at(z, rows, data * xl[A.indices])
    absA = abs(A)
    ax = np.abs(np.asarray(x, np.float64))
    ds = _gamma(n) * (absA @ ax)
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    # ---- rows: c, H and the four sums
    r = z - bl
    c, H = huber_terms(r, dl)
    ac = np.abs(c)
    t_i = ac * (np.abs(r) - ac)
    hs, cc, bc, T = np.sum(H), np.sum(c * c), np.sum(bl * c), np.sum(t_i)
    f = sc * hs
    dr = ds + U * f64(np.abs(r))
    cu = np.minimum(f64(np.abs(r)) + dr, float(delta))
    d_f = scale * (float(np.sum(2 * cu * dr + 2 * U * f64(H))) + _gamma(m) * float(hs)) + U * float(f)
    d_cc = float(np.sum(2 * cu * dr)) + _gamma(m + 1) * float(cc)
    d_bc = float(np.sum(np.abs(f64(bl)) * dr)) + _gamma(m + 1) * float(np.sum(np.abs(bl * c)))
    d_T = float(np.sum(cu * dr + 2 * U * f64(t_i))) + _gamma(m) * float(T)
    # ---- g = 2 scale A^T c, gt = g + l2 x, the scaling
    gfac = 2 * sc
    g = np.zeros(n, dtype=ld)
    np.add.at(g, A.indices, data * c[rows])
    g *= gfac
    dg = float(gfac) * (absA.T @ dr + _gamma(m + 2) * (absA.T @ f64(ac)))
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
        d_alpha = d_oma = 0.0
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
    # ---- rows gap and the dual
    inner = oma * cc + 2 * T
    rows_gap = sc * oma * inner
    d_inner = d_oma * float(cc) + float(oma) * d_cc + 2 * d_T
    d_rows = scale * (d_oma * float(inner) + float(oma) * d_inner) + 4 * U * float(rows_gap)
    D_loss = -sc * (alpha * alpha * cc + 2 * alpha * bc)
    d_Dl = (scale * (2 * float(alpha) * d_alpha * float(cc) + float(alpha) ** 2 * d_cc + 2 * d_alpha * abs(float(bc)) + 2 * float(alpha) * d_bc)
            + 4 * U * scale * (float(alpha) ** 2 * float(cc) + 2 * float(alpha) * abs(float(bc))))
    if l2 > 0:
        Pv = f + g_l1 + g_l2
        d_P = d_f + d_gl1 + d_gl2 + 2 * U * abs(float(Pv))
        D = D_loss - alpha * alpha * g_l2
        d_D = d_Dl + 2 * float(alpha) * d_alpha * float(g_l2) + float(alpha) ** 2 * d_gl2 + 3 * U * float(alpha) ** 2 * float(g_l2) + U * abs(float(D))
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
    extra = dict(gap_pd=Pv - D, grad=gt, cols=cols, cc=cc, T=T, share=float(np.mean(f64(np.abs(r)) > delta)), terms=t_i)
    return vals, bounds, extra


def primal_longdouble(A, b, x, lam, delta, scale=SCALE, l2=0.0):
    return gap_longdouble(A, b, x, lam, delta, scale, l2)[0]["primal"]


def worst_ratio(got, vals, bounds):
    """{key: |got - value| / bound} over the keys of ``vals`` (0 / 0 counts as 0)."""
    out = {}
    for k in vals:
        err = abs(float(np.longdouble(getattr(got, k)) - vals[k]))
        out[k] = 0.0 if err == 0.0 else (err / bounds[k] if bounds[k] > 0 else np.inf)
    return out


# ---- screening -------------------------------------------------------------------------------------------------------------------
def screen_longdouble(A, b, x, lam, delta, scale=SCALE, dense=False):
    """screen_cases.screen_longdouble for Huber's loss (l2 = 0): the exact rule with L = 2 scale and the guard E with c for r."""
    ld = np.longdouble
    vals, bounds, extra = gap_longdouble(A, b, x, lam, delta, scale)
    norms, _ = SC.column_norms_ld(A)
    radius = np.sqrt(ld(2) * ld(SC.lipschitz(scale, False)) * vals["gap"])
    g = extra["grad"]
    left = vals["alpha"] * np.abs(g) + radius * norms
    E, eg = SC.guard(A, x, lam, scale, False, norms, radius, extra["cc"], dense)   # (its `rr` enters as |c|_2^2 only)
    return dict(vals=vals, bounds=bounds, grad=g, norms=norms, radius=radius, left=left, discard=left < ld(lam), E=E, Eg=eg)


def lam_max(A, b, delta, scale=SCALE):
    """2 scale |A^T clip(-b)|_inf in longdouble."""
    return float(gap_longdouble(A, b, np.zeros(A.shape[1]), 1.0, delta, scale)[0]["grad_inf"])


def fista(A, b, lam, delta, x0, iters, scale=SCALE, record=()):
    """Plain FISTA with the step 1 / (1.05 L |A|_2^2), L = 2 scale, in fp64 (screen_cases.fista for this loss).  Returns (x, {k: x_k})."""
    A = GC._csr(A)
    At = A.T.tocsr()
    b = np.asarray(b, dtype=np.float64)
    v = np.random.default_rng(0).standard_normal(A.shape[1])
    for _ in range(100):
        v = At @ (A @ v)
        v /= np.linalg.norm(v)
    step = 1.0 / (1.05 * 2.0 * scale * float(np.linalg.norm(At @ (A @ v))))
    x = np.array(x0, dtype=np.float64)
    y, t, kept = x.copy(), 1.0, {}
    for k in range(1, iters + 1):
        grad = (2.0 * scale) * (At @ huber_terms(A @ y - b, delta)[0])
        w = y - step * grad
        xn = np.sign(w) * np.maximum(np.abs(w) - step * lam, 0.0)
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        y = xn + ((t - 1.0) / tn) * (xn - x)
        x, t = xn, tn
        if k in record:
            kept[k] = x.copy()
    return x, kept
