"""Elastic-net inputs, NumPy reference closures and the long-double restatement of the elastic-net certificate, shared by the
elastic-net tests and their fixture script (no test in here).

    g(x) = lam |x|_1 + (l2 / 2) sum x_j^2  (+inf outside the box),   prox_{w g}(v) = clip(soft_threshold(v, lam w) * shrink),
    shrink = 1.0 / (1.0 + l2 w)  - a scalar, formed once; the element is multiplied by it

The matrices, right-hand sides, labels and lam are those of sparse_cases / logistic_cases (least squares: scale 1/2; logistic:
scale 1), in both storage forms; l2 is lam or lam / 100.

The certificate treats the ridge term as n more rows with phi(t) = (l2 / 2) t^2 at z = x:

    gt = grad f(x) + l2 x,   alpha = min(1, lam / |gt|_inf) (1 when gt = 0),   1 - alpha = max(0, (|gt|_inf - lam) / |gt|_inf)
    P = f + lam |x|_1 + (l2 / 2) sum x^2            D = D_loss(alpha) - (l2 / 2) alpha^2 sum x^2
    rows = the loss part of gap_cases               ridge = (l2 / 2) (1 - alpha)^2 sum x^2
    columns = sum_j (lam |x_j| + alpha gt_j x_j)    gap = rows + ridge + columns  (== P - D in exact arithmetic)

Rounding bounds: those of tests/gap_cases.py (same symbols, same safety factor 2), with these lines added or changed -

  gt        gt_j = fma(l2, x_j, g_j): one rounding on top of the error of g_j:   d(gt_j) = dg_j + u |gt_j|
  scaling   G = |gt|_inf, dG = max_j d(gt_j); d(alpha), d(oma), d(aloga) from G and dG as there
  columns   t_j = fma(alpha gt_j, x_j, lam |x_j|):  the line of gap_cases with gt for g and d(gt) for dg
  sum x^2   xx = sum fma(x_j, x_j, .) in any order:  d(xx) = gamma_(n+1) xx
  g_l2      (0.5 l2) xx, 0.5 l2 exact:  d(g_l2) = (l2 / 2) d(xx) + u g_l2
  ridge     (oma oma) g_l2:  d(ridge) = 2 oma d(oma) g_l2 + oma^2 d(g_l2) + 4 u ridge
  P         (f + g_l1) + g_l2:  d(P) = d(f) + d(g_l1) + d(g_l2) + 2 u |P|
  D         D_loss - (alpha alpha) g_l2:  d(D) = d(D_loss) + 2 alpha d(alpha) g_l2 + alpha^2 d(g_l2) + 3 u alpha^2 g_l2 + u |D|
  gap       (rows + ridge) + columns:  d(gap) = d(rows) + d(ridge) + d(columns) + 2 u gap
"""
import numpy as np
import scipy.sparse as sp

import gap_cases as GC
import logistic_cases as L
import sparse_cases as S
from oracle import problems_ref as P

U = GC.U
KEYS = GC.KEYS + ("g_l2", "ridge_gap")
SMALL, TALL = S.SMALL, S.TALL
LOSSES = ("ls", "logit")
FORMS = ("csr", "dense")
L2_FACTORS = (1.0, 0.01)          # l2 = factor * lam
LS_SCALE, LOGIT_SCALE = 0.5, 1.0


def make_case(loss, case):
    """(A csr, b, lam, scale) of one loss on one (m, n, density, seed)."""
    if loss == "ls":
        A, b, lam = S.make_sparse(*case)
        return A, b, lam, LS_SCALE
    A, b, lam = L.make_logistic(*case)
    return A, b, lam, LOGIT_SCALE


def matrix(A, storage):
    return A if storage == "csr" else A.toarray()


class EnetRef:
    """The four closures of an elastic-net problem: f and jac_f of the l1 reference closures of the loss
    (sparse_cases.SparseLeastSquaresL1Ref on either storage form, logistic_cases.LogisticL1Ref), g and prox_wsum_g with the
    ridge term."""

    def __init__(self, loss, A, b, lam, l2, scale=None, bounds=None):
        scale = (LS_SCALE if loss == "ls" else LOGIT_SCALE) if scale is None else scale
        if loss == "ls":
            self.base = S.SparseLeastSquaresL1Ref(A, b, lam, scale) if sp.issparse(A) else P.LeastSquaresL1Ref(np.asarray(A, float), b, lam, scale)
        else:
            self.base = L.LogisticL1Ref(A, b, lam, scale)
        self.lam, self.l2 = float(lam), float(l2)
        self.bounds = None if bounds is None else (float(bounds[0]), float(bounds[1]))
        self.f, self.jac_f = self.base.f, self.base.jac_f

    def g(self, x):
        if self.bounds is not None and ((x < self.bounds[0]).any() or (x > self.bounds[1]).any()):
            return np.inf
        return self.lam * np.linalg.norm(x, ord=1) + (self.l2 / 2) * np.sum(x * x)

    def prox_wsum_g(self, weight, x):
        x = P.soft_threshold(x, self.lam * weight) * (1.0 / (1.0 + self.l2 * weight))
        if self.bounds is not None:
            x = P.clip_box(x, self.bounds[0], self.bounds[1])
        return x

    def callbacks(self):
        return self.f, self.g, self.jac_f, self.prox_wsum_g


# the fixture's solver variants (80 iterations from lr = 1, return_all), every loss x SMALL shape x l2 x storage form
GOLDEN_VARIANTS = {
    "ista": dict(nesterov=False),
    "fista": dict(nesterov=True, nesterov_ratio=(0, 0.25)),
}
GOLDEN_KW = dict(lr=1, tol=0.0, max_iter=80, return_all=True)
GOLDEN_STRIDE = 7


def golden_prefix(loss, ci, fi, storage, tag):
    return f"{loss}.c{ci}.l{fi}.{storage}.{tag}"


def g_longdouble(x, lam, l2):
    xl = np.asarray(x, np.float64).astype(np.longdouble)
    return np.longdouble(lam) * np.sum(np.abs(xl)) + np.longdouble(l2) / 2 * np.sum(xl * xl)


def primal_longdouble(A, b, x, lam, l2, scale, logistic):
    """P(x) in np.longdouble."""
    ld = np.longdouble
    A = GC._csr(A)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    xl, bl = np.asarray(x, np.float64).astype(ld), np.asarray(b, np.float64).astype(ld)
    z = np.zeros(A.shape[0], dtype=ld)
    np.add.at(z, rows, A.data.astype(ld) * xl[A.indices])
    if logistic:
        t = -bl * z
        f = ld(scale) * np.sum(np.maximum(t, ld(0)) + np.log1p(np.exp(-np.abs(t))))
    else:
        f = ld(scale) * np.sum((z - bl) ** 2)
    return f + g_longdouble(x, lam, l2)


def gap_longdouble(A, b, x, lam, l2, scale, logistic):
    """(values, bounds, extra) over KEYS as gap_cases.gap_longdouble, for the elastic-net certificate (the header's formulas
    and bounds).  With l2 = 0 every value is the one gap_cases.gap_longdouble gives."""
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError("np.longdouble carries fewer than 63 mantissa bits here: an fp64 evaluation cannot be checked against it")
    ld = np.longdouble
    _gamma = GC._gamma
    A = GC._csr(A)
    m, n = A.shape
    rows = np.repeat(np.arange(m), np.diff(A.indptr))
    data = A.data.astype(ld)
    xl, bl = np.asarray(x, np.float64).astype(ld), np.asarray(b, np.float64).astype(ld)
    lam_l, sc, l2_l = ld(lam), ld(scale), ld(l2)
    z = np.zeros(m, dtype=ld)
    np.add.at(z, rows, data * xl[A.indices])
    absA = abs(A)
    ax = np.abs(np.asarray(x, np.float64))
    ds = _gamma(n) * (absA @ ax)
    tiny = m * 2.0 ** -1022
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    if logistic:
        t = -bl * z
        e = np.exp(-np.abs(t))
        soft = np.maximum(t, ld(0)) + np.log1p(e)
        q = np.where(t >= 0, ld(1), e) / (ld(1) + e)
        q1 = np.where(t >= 0, e, ld(1)) / (ld(1) + e)
        cand = -bl * q
        f = sc * np.sum(soft)
        d_f = scale * (ds.sum() + _gamma(m + 7) * float(np.sum(soft))) + tiny
        dq = f64(q * q1) * ds + 5 * U * f64(q)
        dq1 = f64(q * q1) * ds + 5 * U * f64(q1)
        dcand = dq
        gfac, gk = sc, m + 1
    else:
        r = z - bl
        cand = r
        rr, br = np.sum(r * r), np.sum(bl * r)
        f = sc * rr
        dr = ds + U * f64(np.abs(r))
        d_rr = float(np.sum(2 * f64(np.abs(r)) * dr)) + _gamma(m + 1) * float(rr)
        d_br = float(np.sum(np.abs(f64(bl)) * dr)) + _gamma(m + 1) * float(np.sum(np.abs(bl * r)))
        d_f = scale * d_rr + 4 * U * float(f)
        dcand = dr
        gfac, gk = 2 * sc, m + 2
    g = np.zeros(n, dtype=ld)
    np.add.at(g, A.indices, data * cand[rows])
    g *= gfac
    dg = float(gfac) * (absA.T @ dcand + _gamma(gk) * (absA.T @ f64(np.abs(cand)))) + (tiny if logistic else 0.0)
    # ---- the ridge rows enter here: gt = g + l2 x ----
    gt = g + l2_l * xl
    dgt = dg + U * f64(np.abs(gt))
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
    Pv = f + g_l1 + g_l2
    d_P = d_f + d_gl1 + d_gl2 + 2 * U * abs(float(Pv))
    if logistic:
        aloga = alpha * np.log(alpha) if alpha > 0 else ld(0)
        d_aloga = d_alpha * abs(float(np.log(alpha))) + d_oma + 4 * U * abs(float(aloga)) if alpha > 0 else 0.0
        omp = q1 + oma * q
        d_omp = dq1 + d_oma * f64(q) + float(oma) * dq + 2 * U * f64(omp)
        if oma > 0:
            Lv = np.log(omp / q1)
            L_closed = np.where(t <= 0, np.log1p(oma * np.exp(np.minimum(t, ld(0)))), t + np.log(oma + np.exp(-np.maximum(t, ld(0)))))
            Lv = np.where(np.isfinite(Lv), Lv, L_closed)
        else:
            Lv = np.zeros(m, dtype=ld)
        et = f64(np.exp(np.minimum(t, ld(0))))
        emt = f64(np.exp(-np.maximum(t, ld(0))))
        w = float(oma) * et
        dL_neg = d_oma * et + w * (ds + 3 * U) + 2 * U * f64(np.abs(Lv))
        v = float(oma) + emt
        with np.errstate(divide="ignore", invalid="ignore"):
            dL_pos = ds + (d_oma + emt * (ds + 2 * U) + U * v) / v + 2 * U * np.abs(np.log(v)) + U * f64(np.abs(Lv))
        dL = np.where(f64(t) <= 0, dL_neg, dL_pos) if oma > 0 else d_oma * np.where(f64(t) <= 0, et, 1.0 / np.maximum(emt, 2.0 ** -1022))
        kl_i = q * aloga + omp * Lv
        d_kl_i = (dq * abs(float(aloga)) + f64(q) * d_aloga + d_omp * f64(np.abs(Lv)) + f64(omp) * dL
                  + 2 * U * (f64(np.abs(q * aloga)) + f64(np.abs(omp * Lv))) + U * f64(np.abs(kl_i)))
        rows_gap = sc * np.sum(kl_i)
        d_rows = scale * (float(np.sum(d_kl_i)) + _gamma(m) * float(np.sum(np.abs(kl_i)))) + U * abs(float(rows_gap)) + tiny
        p = alpha * q
        dp = d_alpha * f64(q) + float(alpha) * dq + U * f64(p)
        with np.errstate(divide="ignore", invalid="ignore"):
            plogp = np.where(p > 0, p * np.log(np.where(p > 0, p, ld(1))), ld(0))
            ologo = np.where(omp > 0, omp * np.log(np.where(omp > 0, omp, ld(1))), ld(0))
            lp = np.where(p > 0, np.abs(np.log(np.where(p > 0, p, ld(1)))), ld(0))
            lo = np.where(omp > 0, np.abs(np.log(np.where(omp > 0, omp, ld(1)))), ld(0))
        ent = plogp + ologo
        d_ent = dp * (f64(lp) + 1) + 3 * U * f64(np.abs(plogp)) + d_omp * (f64(lo) + 1) + 3 * U * f64(np.abs(ologo))
        D_loss = -sc * np.sum(ent)
        d_Dl = scale * (float(np.sum(d_ent)) + _gamma(m) * float(np.sum(np.abs(ent)))) + U * abs(float(D_loss)) + tiny
    else:
        rows_gap = sc * oma * oma * rr
        d_rows = scale * (2 * float(oma) * d_oma * float(rr) + float(oma) ** 2 * d_rr) + 4 * U * float(rows_gap)
        D_loss = -sc * (alpha * alpha * rr + 2 * alpha * br)
        d_Dl = (scale * (2 * float(alpha) * d_alpha * float(rr) + float(alpha) ** 2 * d_rr + 2 * d_alpha * abs(float(br)) + 2 * float(alpha) * d_br)
                + 4 * U * scale * (float(alpha) ** 2 * float(rr) + 2 * float(alpha) * abs(float(br))))
    D = D_loss - alpha * alpha * g_l2
    d_D = (d_Dl + 2 * float(alpha) * d_alpha * float(g_l2) + float(alpha) ** 2 * d_gl2 + 3 * U * float(alpha) ** 2 * float(g_l2)
           + U * abs(float(D)))
    gap = rows_gap + ridge + cols
    d_gap = d_rows + d_ridge + d_cols + 2 * U * float(gap)
    vals = dict(primal=Pv, dual=D, gap=gap, alpha=alpha, grad_inf=G, f=f, g_l1=g_l1, rows_gap=rows_gap, g_l2=g_l2, ridge_gap=ridge)
    bounds = dict(primal=d_P, dual=d_D, gap=d_gap, alpha=d_alpha, grad_inf=dG + U * float(G), f=d_f, g_l1=d_gl1, rows_gap=d_rows,
                  g_l2=d_gl2, ridge_gap=d_ridge)
    bounds = {k: 2 * float(v) for k, v in bounds.items()}
    return vals, bounds, dict(gap_pd=Pv - D, grad=gt, cols=cols)


def worst_ratio(got, vals, bounds):
    """{key: |got - value| / bound} over the ten KEYS (0 / 0 counts as 0)."""
    out = {}
    for k in KEYS:
        err = abs(float(np.longdouble(getattr(got, k)) - vals[k]))
        out[k] = 0.0 if err == 0.0 else (err / bounds[k] if bounds[k] > 0 else np.inf)
    return out
