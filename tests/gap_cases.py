"""The duality gap of the four L1 margins problems, restated in np.longdouble with first-order fp64 rounding bounds for every
output of the device evaluation (no test in here; tests/test_gap_reference.py proves this restatement on the CPU).

    P(x) = sum_i phi_i(z_i) + lam |x|_1,  z = A x,   phi_i(z) = scale (z - b_i)^2   or   scale softplus(-b_i z)
    nu = alpha grad phi(z),  g = A^T grad phi(z),  alpha = min(1, lam / |g|_inf) (1 when g = 0),  D = -sum_i phi_i^*(nu_i)
    least squares:  r = z - b,  D = -scale (alpha^2 |r|^2 + 2 alpha b.r),                rows = scale (1 - alpha)^2 |r|^2
    logistic:       q = sigma(-b z), p = alpha q,  D = -scale sum [p log p + (1 - p) log(1 - p)],  rows = scale sum KL(p || q)
    columns = sum_j (lam |x_j| + alpha g_j x_j);   gap = rows + columns  (== P - D in exact arithmetic)

The reference project has no duality gap: these formulas, in extended precision, are the yardstick.

Rounding bounds (u = 2^-53, gamma_k = k u / (1 - k u), c = |A| |x|; every sum may be taken in ANY order; first order, and
every bound carries the safety factor 2 of the other element-wise tests for second-order terms and its own rounding):

  margins   ds_i = |z^_i - z_i| <= gamma_n c_i                                              (as tests/test_gpu_logistic.py)
  LS        dr_i = ds_i + u |r_i|;   d(rr) = sum 2 |r_i| dr_i + gamma_(m+1) rr;   d(br) = sum |b_i| dr_i + gamma_(m+1) sum |b_i r_i|
            f = scale sqrt(rr)^2: d(f) = scale d(rr) + 4 u f;   dg_j = 2 scale ((|A|^T dr)_j + gamma_(m+2) (|A|^T |r|)_j)
  logistic  d(f) = scale (sum ds_i + gamma_(m+7) sum softplus_i);  dq_i = q_i (1 - q_i) ds_i + 5 u q_i, and the same with the
            factor 5 u (1 - q_i) for 1 - q_i;  drho_i = dq_i;   dg_j = scale ((|A|^T drho)_j + gamma_(m+1) (|A|^T |rho|)_j)
  scaling   G = |g|_inf: dG = max_j dg_j (the maximum is 1-Lipschitz).  alpha = min(1, lam / G) and 1 - alpha =
            max(0, (G - lam) / G) are Lipschitz in G across the kink at G = lam:
                d(alpha) = dG / max(G, lam) + u,      d(oma) = 2 dG / max(G, lam) + 2 u (1 - alpha)
            (both 0 when G + dG <= lam: every evaluation inside dG then takes the branch alpha = 1, 1 - alpha = 0 exactly)
            alpha log alpha = alpha log1p(-(1 - alpha)):  d(aloga) = d(alpha) |log alpha| + d(oma) + 4 u |alpha log alpha|
  columns   t_j = fma(alpha g_j, x_j, lam |x_j|), clamped at 0 (t_j >= 0 in exact arithmetic, so the clamp only helps):
                d(t_j) = |x_j| (d(alpha) |g_j| + alpha dg_j + u alpha |g_j| + u lam) + u t_j;   d(cols) = sum d(t_j) + gamma_n cols
            Each column term is lam |x_j| against alpha g_j x_j - the gap's own two terms - and g_j is known to u relative
            at best, so the column part resolves u lam |x|_1 times the condition of g: nothing here is of the size of
            f or of P (forming P - D would add u P).
  LS rows   scale oma^2 rr:   d(rows) = scale (2 oma d(oma) rr + oma^2 d(rr)) + 4 u rows            (all scaled by 1 - alpha)
  KL rows   omp = (1 - q) + oma q:  d(omp) = d(1 - q) + d(oma) q + oma dq + 2 u omp
            L = log1p(oma e^t) (t <= 0):  w = oma e^t, dw = d(oma) e^t + w (ds + 3 u),  dL = dw + 2 u L
            L = t + log(oma + e^-t) (t > 0):  v = oma + e^-t, dv = d(oma) + e^-t (ds + 2 u) + u v,
                                              dL = ds + dv / v + 2 u |log v| + u |L|
            KL_i = q aloga + omp L:  d(KL_i) = dq |aloga| + q d(aloga) + d(omp) |L| + omp dL + 2 u (|q aloga| + |omp L|) + u KL_i
            d(rows) = scale (sum d(KL_i) + gamma_m sum KL_i) + u rows.  (The two parts of KL_i cancel to first order in
            1 - alpha; the bound is in those two parts - the gap's own terms - and nothing larger.)
  entropy   p = alpha q: dp = d(alpha) q + alpha dq + u p;   d(p log p) = dp (|log p| + 1) + 3 u |p log p|, likewise for omp;
            D = -scale sum:  d(D) = scale (sum of those + gamma_m sum |ent_i|) + u |D|
  LS dual   d(D) = scale (2 alpha d(alpha) rr + alpha^2 d(rr) + 2 d(alpha) |br| + 2 alpha d(br)) + 4 u scale (alpha^2 rr + 2 alpha |br|)
  P         d(P) = d(f) + lam gamma_(n+1) |x|_1 + u |P|;   gap:  d(gap) = d(rows) + d(cols) + u gap
  underflow exp(-|t|) below 2^-1022 loses its relative accuracy: m 2^-1022 is added to every bound a row sum enters.
"""
import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
KEYS = ("primal", "dual", "gap", "alpha", "grad_inf", "f", "g_l1", "rows_gap")


def _gamma(k):
    return k * U / (1 - k * U)


def _csr(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sum_duplicates()
    A.sort_indices()
    return A


def gap_longdouble(A, b, x, lam, scale, logistic):
    """(values, bounds, extra): dicts over KEYS in np.longdouble / float64; extra holds ``gap_pd`` = P - D formed in
    longdouble (the other form of the same number) and ``grad`` (g, longdouble)."""
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError("np.longdouble carries fewer than 63 mantissa bits here: an fp64 evaluation cannot be checked against it")
    ld = np.longdouble
    A = _csr(A)
    m, n = A.shape
    rows = np.repeat(np.arange(m), np.diff(A.indptr))
    data = A.data.astype(ld)
    xl, bl = np.asarray(x, np.float64).astype(ld), np.asarray(b, np.float64).astype(ld)
    lam_l, sc = ld(lam), ld(scale)
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
    G = np.max(np.abs(g)) if n else ld(0)
    dG = float(np.max(dg)) if n else 0.0
    if G > lam_l:
        alpha, oma = lam_l / G, (G - lam_l) / G
    else:
        alpha, oma = ld(1), ld(0)
    big = max(float(G), float(lam))
    d_alpha = (dG / big + U) if big > 0 else 0.0
    d_oma = (2 * dG / big + 2 * U * float(oma)) if big > 0 else 0.0
    if float(G) * (1 + 2 * U) + dG <= float(lam):
        d_alpha = d_oma = 0.0   # no fp64 evaluation inside dG of g can leave the branch alpha = 1, 1 - alpha = 0: both are exact
    # columns
    tj = lam_l * np.abs(xl) + alpha * g * xl
    cols = np.sum(tj)
    d_t = ax * (d_alpha * f64(np.abs(g)) + float(alpha) * dg + U * float(alpha) * f64(np.abs(g)) + U * float(lam)) + U * f64(np.abs(tj))
    d_cols = float(np.sum(d_t)) + _gamma(n) * float(np.sum(np.abs(tj)))
    asum = np.sum(np.abs(xl))
    g_l1 = lam_l * asum
    d_gl1 = float(lam) * _gamma(n + 1) * float(asum)
    P = f + g_l1
    d_P = d_f + d_gl1 + U * abs(float(P))
    if logistic:
        aloga = alpha * np.log(alpha) if alpha > 0 else ld(0)
        d_aloga = d_alpha * abs(float(np.log(alpha))) + d_oma + 4 * U * abs(float(aloga)) if alpha > 0 else 0.0
        omp = q1 + oma * q
        d_omp = dq1 + d_oma * f64(q) + float(oma) * dq + 2 * U * f64(omp)
        if oma > 0:
            L = np.log(omp / q1)
            # (t > 750 would underflow 1 - q even here; the closed forms agree with log(omp / (1 - q)) where that is finite)
            L_closed = np.where(t <= 0, np.log1p(oma * np.exp(np.minimum(t, ld(0)))), t + np.log(oma + np.exp(-np.maximum(t, ld(0)))))
            L = np.where(np.isfinite(L), L, L_closed)
        else:
            L = np.zeros(m, dtype=ld)
        et = f64(np.exp(np.minimum(t, ld(0))))      # e^t for t <= 0
        emt = f64(np.exp(-np.maximum(t, ld(0))))    # e^-t for t > 0
        w = float(oma) * et
        dL_neg = d_oma * et + w * (ds + 3 * U) + 2 * U * f64(np.abs(L))
        v = float(oma) + emt
        with np.errstate(divide="ignore", invalid="ignore"):
            dL_pos = ds + (d_oma + emt * (ds + 2 * U) + U * v) / v + 2 * U * np.abs(np.log(v)) + U * f64(np.abs(L))
        dL = np.where(f64(t) <= 0, dL_neg, dL_pos) if oma > 0 else d_oma * np.where(f64(t) <= 0, et, 1.0 / np.maximum(emt, 2.0 ** -1022))
        kl_i = q * aloga + omp * L
        d_kl_i = (dq * abs(float(aloga)) + f64(q) * d_aloga + d_omp * f64(np.abs(L)) + f64(omp) * dL
                  + 2 * U * (f64(np.abs(q * aloga)) + f64(np.abs(omp * L))) + U * f64(np.abs(kl_i)))
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
        D = -sc * np.sum(ent)
        d_D = scale * (float(np.sum(d_ent)) + _gamma(m) * float(np.sum(np.abs(ent)))) + U * abs(float(D)) + tiny
    else:
        rows_gap = sc * oma * oma * rr
        d_rows = scale * (2 * float(oma) * d_oma * float(rr) + float(oma) ** 2 * d_rr) + 4 * U * float(rows_gap)
        D = -sc * (alpha * alpha * rr + 2 * alpha * br)
        d_D = (scale * (2 * float(alpha) * d_alpha * float(rr) + float(alpha) ** 2 * d_rr + 2 * d_alpha * abs(float(br)) + 2 * float(alpha) * d_br)
               + 4 * U * scale * (float(alpha) ** 2 * float(rr) + 2 * float(alpha) * abs(float(br))))
    gap = rows_gap + cols
    d_gap = d_rows + d_cols + U * float(gap)
    vals = dict(primal=P, dual=D, gap=gap, alpha=alpha, grad_inf=G, f=f, g_l1=g_l1, rows_gap=rows_gap)
    bounds = dict(primal=d_P, dual=d_D, gap=d_gap, alpha=d_alpha, grad_inf=dG + U * float(G), f=d_f, g_l1=d_gl1, rows_gap=d_rows)
    bounds = {k: 2 * float(v) for k, v in bounds.items()}
    return vals, bounds, dict(gap_pd=P - D, grad=g, cols=cols)


def worst_ratio(got, vals, bounds):
    """{key: |got - value| / bound} (0 / 0 counts as 0: an exact value met exactly); ``got``: an object with the KEYS as attributes."""
    out = {}
    for k in KEYS:
        err = abs(float(np.longdouble(getattr(got, k)) - vals[k]))
        out[k] = 0.0 if err == 0.0 else (err / bounds[k] if bounds[k] > 0 else np.inf)
    return out
