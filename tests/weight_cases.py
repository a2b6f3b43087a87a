"""Per-row sample weights: inputs, NumPy reference closures in the kernels' arithmetic, the long-double restatement of f and of
the certificate with first-order rounding bounds for every output, and fold numbers - shared by the weight tests (no test in
here; tests/test_weight_cases.py proves the closures on the CPU).

    f(x) = scale sum_i w_i phi_i(z_i),  z = A x,   grad f = gfac A^T (w o psi(z)),   gfac = 2 scale (square, huber) | scale (logistic)
    square    r = z - b                psi = r                              phi = r r
    huber     r = z - b                psi = c = copysign(min(|r|, delta), r)  phi = c (2 r - c)
    logistic  t = -b z, e = exp(-|t|)  psi = -b sigma(t)                     phi = max(t, 0) + log1p(e)
    per row one product for each output: rho_i = w_i psi_i, term_i = w_i phi_i; a row with w_i == 0 gives +0 for both, whatever
    b_i holds (csrc/zf_kernels_loss.h).  The sum is a plain sum, times scale once.

The reference project has no sample weights.  The yardsticks are its SOLVER on these closures and two exact equivalences:
0 / 1 weights are the row subset, integer weights are duplicated rows (tests/test_weight_cases.py).

The certificate.  (w phi)^*(w u) = w phi^*(u): with nu_i = alpha w_i phi_i'(z_i) every row term of the unweighted certificate
(tests/gap_cases.py, tests/huber_cases.py) is multiplied by w_i; the n-passes, alpha and the compositions are unchanged:

    square    rr = sum w r^2, br = sum w b r:       D = -scale (alpha^2 rr + 2 alpha br),   rows = scale (1 - alpha)^2 rr
    huber     hs = sum w H, cc = sum w c^2, bc = sum w b c, T = sum w |c| (|r| - |c|):
              D = -scale (alpha^2 cc + 2 alpha bc),   rows = scale (1 - alpha) ((1 - alpha) cc + 2 T)
    logistic  D = -scale sum w [p log p + (1 - p) log(1 - p)],   rows = scale sum w KL(alpha q || q)

Rounding bounds (u = 2^-53, gamma_k = k u / (1 - k u); first order; every bound carries the safety factor 2 of gap_cases).  The
per-row lines are those of gap_cases / huber_cases, restated here as (value v_i, bound dv_i of the fp64 v_i, its own roundings
included):

  margins   ds_i <= gamma_n (|A| |x|)_i;   dr_i = ds_i + u |r_i|;   cu_i = min(|r_i| + dr_i, delta)
  square    r r: 2 |r| dr + u r^2;      b r: |b| dr + u |b r|;      psi = r: dr
  huber     H: 2 cu dr + 2 u H;         c^2: 2 cu dr + u c^2;       b c: |b| dr + u |b c|;     t = |c| (|r| - |c|): cu dr + 2 u t;   psi = c: dr
  logistic  softplus: ds + 7 u softplus;   q: q (1 - q) ds + 5 u q (the same with 1 - q);   psi = -b q: dq;   KL_i, ent_i: gap_cases
  weighted sum of m such values, sum_i w_i v_i, each product rounded once and the sum in any order:
            d = sum w_i dv_i + (u + gamma_m) sum w_i |v_i|                                                    (the line `wsum`)
  f         scale (that sum of phi):  d(f) = scale d(sum) + u f
  rho       w psi, one product:  drho_i = w_i dpsi_i + u w_i |psi_i|
  g         gfac A^T rho:  dg_j = gfac ((|A|^T drho)_j + gamma_(m+2) (|A|^T |rho|)_j)
  scaling, columns, ridge, P, D, rows, gap:  the lines of gap_cases / enet_cases / huber_cases with the weighted sums in place of
            the unweighted ones
  underflow (logistic) m 2^-1022 max(1, max w) is added to every bound a row sum enters.
"""
import numpy as np
import scipy.sparse as sp

import gap_cases as GC
import huber_cases as H
import logistic_cases as L
import sparse_cases as S
from oracle import problems_ref as P

U = GC.U
KEYS8 = GC.KEYS
KEYS10 = GC.KEYS + ("g_l2", "ridge_gap")
SMALL, TALL = S.SMALL, S.TALL
GPU_SMALL = [S.SMALL[0], S.SMALL[2], S.SMALL[3]]   # 300 x 1000, 1000 x 257, 64 x 4099
FORMS = ("csr", "dense")
LOSSES = ("square", "logistic", "huber")
LOSS_CODE = {"square": 0, "logistic": 1, "huber": 2}   # ZF_LOSS_*
SCALE = {"square": 0.5, "logistic": 1.0, "huber": 0.5}


def make_problem(case, loss):
    """(A csr, b, lam, delta) of one (m, n, density, seed): the inputs of sparse_cases / logistic_cases / huber_cases (delta 0.0
    where the loss has none)."""
    if loss == "logistic":
        A, b, lam = L.make_logistic(*case)
        return A, b, lam, 0.0
    if loss == "huber":
        return H.make_huber(case)
    A, b, lam = S.make_sparse(*case)
    return A, b, lam, 0.0


def make_weights(m, seed, kind="real"):
    """``real``: about 20 % zeros, the rest in (0.25, 2.25); ``mask``: 0 / 1 with about 30 % zeros; ``int``: integers 0 .. 2.
    As for the matrices of sparse_cases, the draws were checked on the CPU before they were fixed: two NumPy forms of the same
    problem (weights against repeated rows) must stay together over 80 iterations from lr = 1.  Integers 0 .. 3 did not on the
    Huber cases 300 x 1000 and 2000 x 5000 (three draws of six): the line search settles on a step at which the momentum
    iteration amplifies a rounding difference by about 1.3 per iteration - 1e-16 to 3e-10 and 2e-5, with equal decisions
    throughout - which says nothing about either form: on those two draws the UNWEIGHTED repeated-rows problem, with no weight
    anywhere, moves by 5e-5 and 1.5e-9 from itself when its rows are merely permuted (another order of the same sums, equal
    decisions).  The instance is ill-conditioned, not the weights.  Integers 0 .. 2 stay within 2e-14 on every case, loss and
    draw tried; weights above 2 are covered by the element tests (w = 3) and by the real-valued weights up to 2.25."""
    rng = np.random.default_rng(seed + 7000 + {"real": 0, "mask": 1, "int": 2}[kind])
    if kind == "mask":
        w = (rng.random(m) >= 0.3).astype(np.float64)
    elif kind == "int":
        w = rng.integers(0, 3, m).astype(np.float64)
    else:
        w = np.where(rng.random(m) < 0.2, 0.0, 0.25 + 2.0 * rng.random(m))
    if not w.any():
        w[0] = 1.0
    return w


def matrix(A, storage):
    return A if storage == "csr" else A.toarray()


def row_terms(z, b, loss, delta=0.0):
    """(psi, phi) per row in the arithmetic of the kernels (any float dtype)."""
    if loss == "logistic":
        t = -b * z
        soft, sig = L.stable_terms(t)
        return -b * sig, soft
    r = z - b
    if loss == "huber":
        return H.huber_terms(r, delta)
    return r, r * r


def weighted(w, v):
    """w o v with the kernels' select: exactly +0 on a row with w == 0, whatever v holds."""
    with np.errstate(invalid="ignore"):
        return np.where(w != 0, w * v, 0.0)


class WeightedRef:
    """The four closures of a weighted margins problem on either storage form, NumPy / SciPy in fp64."""

    def __init__(self, A, b, lam, w, loss, delta=0.0, scale=None, bounds=None, l2=0.0):
        self.A = sp.csr_matrix(A, dtype=np.float64) if sp.issparse(A) else np.asarray(A, float)
        self.b, self.w = np.asarray(b, float), np.asarray(w, float)
        self.loss, self.delta = loss, float(delta)
        self.lam, self.l2 = float(lam), float(l2)
        self.scale = float(SCALE[loss] if scale is None else scale)
        self.gfac = self.scale if loss == "logistic" else 2 * self.scale
        self.bounds = None if bounds is None else (float(bounds[0]), float(bounds[1]))

    def f(self, x):
        with np.errstate(invalid="ignore", over="ignore"):
            phi = row_terms(self.A @ x, self.b, self.loss, self.delta)[1]
        return self.scale * np.sum(weighted(self.w, phi))

    def jac_f(self, x):
        with np.errstate(invalid="ignore", over="ignore"):
            psi = row_terms(self.A @ x, self.b, self.loss, self.delta)[0]
        return self.gfac * (self.A.T @ weighted(self.w, psi))

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


def subset_ref(A, b, lam, w, loss, delta=0.0, l2=0.0):
    """The UNWEIGHTED closures on the rows with w > 0, each repeated w_i times (w: non-negative integers): the problem that
    integer weights - 0 / 1 weights among them - stand for.  The closures are the unit-weight WeightedRef's, whose sums are the
    unweighted classes' own expressions (1 * v = v exactly)."""
    w = np.asarray(w, float)
    assert np.all(w == np.round(w)) and np.all(w >= 0)
    rows = np.repeat(np.arange(w.size), w.astype(np.int64))
    A = sp.csr_matrix(A)[rows]
    return WeightedRef(A, np.asarray(b, float)[rows], lam, np.ones(rows.size), loss, delta, l2=l2), rows


def fold_ids(m, K, seed=0):
    """Fold numbers as zfista_amd.path.l1_cv draws them: fold k takes positions k::K of default_rng(seed).permutation(m)."""
    perm = np.random.default_rng(seed).permutation(m)
    ids = np.full(m, -1, dtype=np.int64)
    for pos, row in enumerate(perm):
        ids[row] = pos % K
    return ids


# ---- long-double forms --------------------------------------------------------------------------------------------------------------
def _rows_ld(z, ds, b, w, loss, delta):
    """Per-row long-double values and fp64 error bounds at margins z (long double; ds bounds the error of the device's).  Rows
    with w == 0 are taken out first: their b may be anything."""
    ld = np.longdouble
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    on = np.asarray(w) != 0
    w = np.where(on, w, 0.0)
    b = np.where(on, b, 1.0 if loss == "logistic" else 0.0)
    z = np.where(on, z, ld(0))
    wl, bl = w.astype(ld), b.astype(ld)
    m = w.size
    gm = GC._gamma(m)

    def wsum(v, dv):
        """(sum w v in long double, bound of the fp64 sum)"""
        return np.sum(wl * v), float(np.sum(w * dv)) + (U + gm) * float(np.sum(w * f64(np.abs(v))))

    out = dict(w=w, wl=wl, b=bl, wsum=wsum, m=m)
    if loss == "logistic":
        t = -bl * z
        e = np.exp(-np.abs(t))
        soft = np.maximum(t, ld(0)) + np.log1p(e)
        q = np.where(t >= 0, ld(1), e) / (ld(1) + e)
        q1 = np.where(t >= 0, e, ld(1)) / (ld(1) + e)
        dq = f64(q * q1) * ds + 5 * U * f64(q)
        dq1 = f64(q * q1) * ds + 5 * U * f64(q1)
        out.update(t=t, q=q, q1=q1, dq=dq, dq1=dq1, psi=-bl * q, dpsi=dq, phi=soft, dphi=ds + 7 * U * f64(soft))
        return out
    r = z - bl
    dr = ds + U * f64(np.abs(r))
    if loss == "huber":
        c, Hv = H.huber_terms(r, ld(delta))
        cu = np.minimum(f64(np.abs(r)) + dr, float(delta))
        out.update(r=r, dr=dr, cu=cu, psi=c, dpsi=dr, phi=Hv, dphi=2 * cu * dr + 2 * U * f64(Hv))
    else:
        out.update(r=r, dr=dr, psi=r, dpsi=dr, phi=r * r, dphi=2 * f64(np.abs(r)) * dr + U * f64(r * r))
    return out


def _tiny(R, loss):
    return R["m"] * 2.0 ** -1022 * max(1.0, float(np.max(R["w"]))) if loss == "logistic" else 0.0


def loss_longdouble(z, b, w, loss, delta=0.0, scale=None, ds=None):
    """(f, bound of f, rho, bound of every rho_i) at margins z (fp64 values, taken as exact unless ``ds`` bounds their error)."""
    ld = np.longdouble
    scale = SCALE[loss] if scale is None else scale
    z64 = np.asarray(z, np.float64)
    ds = np.zeros(z64.size) if ds is None else np.asarray(ds, np.float64)
    R = _rows_ld(z64.astype(ld), ds, np.asarray(b, np.float64), np.asarray(w, np.float64), loss, delta)
    s, d_s = R["wsum"](R["phi"], R["dphi"])
    f = ld(scale) * s
    d_f = scale * d_s + U * float(f) + _tiny(R, loss)
    rho = R["wl"] * R["psi"]
    drho = R["w"] * R["dpsi"] + U * np.asarray(np.abs(rho), np.float64)
    return f, 2 * d_f, rho, 2 * drho


def gap_longdouble(A, b, w, x, lam, loss, delta=0.0, scale=None, l2=0.0):
    """(values, bounds, extra) of the weighted certificate: dicts over KEYS8 (l2 = 0) or KEYS10 in np.longdouble / float64;
    extra: ``gap_pd`` = P - D in long double, ``grad`` (gt)."""
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError("np.longdouble carries fewer than 63 mantissa bits here: an fp64 evaluation cannot be checked against it")
    ld = np.longdouble
    _gamma = GC._gamma
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    scale = SCALE[loss] if scale is None else scale
    A = GC._csr(A)
    m, n = A.shape
    rows = np.repeat(np.arange(m), np.diff(A.indptr))
    data = A.data.astype(ld)
    xl = np.asarray(x, np.float64).astype(ld)
    lam_l, sc, l2_l = ld(lam), ld(scale), ld(l2)
    z = np.zeros(m, dtype=ld)
    np.add.at(z, rows, data * xl[A.indices])
    absA = abs(A)
    ax = np.abs(np.asarray(x, np.float64))
    ds = _gamma(n) * (absA @ ax)
    R = _rows_ld(z, ds, np.asarray(b, np.float64), np.asarray(w, np.float64), loss, delta)
    wsum, wv = R["wsum"], R["w"]
    tiny = _tiny(R, loss)
    # ---- f, the candidate, g, gt, the scaling
    s, d_s = wsum(R["phi"], R["dphi"])
    f = sc * s
    d_f = scale * d_s + U * float(f) + tiny
    rho = R["wl"] * R["psi"]
    drho = wv * R["dpsi"] + U * f64(np.abs(rho))
    gfac = sc if loss == "logistic" else 2 * sc
    g = np.zeros(n, dtype=ld)
    np.add.at(g, A.indices, data * rho[rows])
    g *= gfac
    dg = float(gfac) * (absA.T @ drho + _gamma(m + 2) * (absA.T @ f64(np.abs(rho)))) + tiny
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
    if loss == "logistic":
        t, q, q1, dq, dq1 = R["t"], R["q"], R["q1"], R["dq"], R["dq1"]
        aloga = alpha * np.log(alpha) if alpha > 0 else ld(0)
        d_aloga = d_alpha * abs(float(np.log(alpha))) + d_oma + 4 * U * abs(float(aloga)) if alpha > 0 else 0.0
        omp = q1 + oma * q
        d_omp = dq1 + d_oma * f64(q) + float(oma) * dq + 2 * U * f64(omp)
        if oma > 0:
            with np.errstate(divide="ignore", invalid="ignore"):
                Lr = np.log(omp / q1)
            L_closed = np.where(t <= 0, np.log1p(oma * np.exp(np.minimum(t, ld(0)))), t + np.log(oma + np.exp(-np.maximum(t, ld(0)))))
            Lr = np.where(np.isfinite(Lr), Lr, L_closed)
        else:
            Lr = np.zeros(m, dtype=ld)
        et = f64(np.exp(np.minimum(t, ld(0))))
        emt = f64(np.exp(-np.maximum(t, ld(0))))
        wv_ = float(oma) * et
        dL_neg = d_oma * et + wv_ * (ds + 3 * U) + 2 * U * f64(np.abs(Lr))
        v = float(oma) + emt
        with np.errstate(divide="ignore", invalid="ignore"):
            dL_pos = ds + (d_oma + emt * (ds + 2 * U) + U * v) / v + 2 * U * np.abs(np.log(v)) + U * f64(np.abs(Lr))
        dL = np.where(f64(t) <= 0, dL_neg, dL_pos) if oma > 0 else d_oma * np.where(f64(t) <= 0, et, 1.0 / np.maximum(emt, 2.0 ** -1022))
        kl_i = q * aloga + omp * Lr
        d_kl_i = (dq * abs(float(aloga)) + f64(q) * d_aloga + d_omp * f64(np.abs(Lr)) + f64(omp) * dL
                  + 2 * U * (f64(np.abs(q * aloga)) + f64(np.abs(omp * Lr))) + U * f64(np.abs(kl_i)))
        kl, d_kl = wsum(kl_i, d_kl_i)
        rows_gap = sc * kl
        d_rows = scale * d_kl + U * abs(float(rows_gap)) + tiny
        p = alpha * q
        dp = d_alpha * f64(q) + float(alpha) * dq + U * f64(p)
        with np.errstate(divide="ignore", invalid="ignore"):
            plogp = np.where(p > 0, p * np.log(np.where(p > 0, p, ld(1))), ld(0))
            ologo = np.where(omp > 0, omp * np.log(np.where(omp > 0, omp, ld(1))), ld(0))
            lp = np.where(p > 0, np.abs(np.log(np.where(p > 0, p, ld(1)))), ld(0))
            lo = np.where(omp > 0, np.abs(np.log(np.where(omp > 0, omp, ld(1)))), ld(0))
        ent_i = plogp + ologo
        d_ent_i = dp * (f64(lp) + 1) + 3 * U * f64(np.abs(plogp)) + d_omp * (f64(lo) + 1) + 3 * U * f64(np.abs(ologo))
        ent, d_ent = wsum(ent_i, d_ent_i)
        D_loss = -sc * ent
        d_Dl = scale * d_ent + U * abs(float(D_loss)) + tiny
    else:
        r, dr, bl = R["r"], R["dr"], R["b"]
        if loss == "huber":
            c, cu = R["psi"], R["cu"]
            ac = np.abs(c)
            t_i = ac * (np.abs(r) - ac)
            cc, d_cc = wsum(c * c, 2 * cu * dr + U * f64(c * c))
            bc, d_bc = wsum(bl * c, np.abs(f64(bl)) * dr + U * f64(np.abs(bl * c)))
            T, d_T = wsum(t_i, cu * dr + 2 * U * f64(t_i))
            inner = oma * cc + 2 * T
            rows_gap = sc * oma * inner
            d_inner = d_oma * float(cc) + float(oma) * d_cc + 2 * d_T
            d_rows = scale * (d_oma * float(inner) + float(oma) * d_inner) + 4 * U * float(rows_gap)
        else:
            cc, d_cc = s, d_s   # sum w r^2: the sum f is made of
            bc, d_bc = wsum(bl * r, np.abs(f64(bl)) * dr + U * f64(np.abs(bl * r)))
            rows_gap = sc * oma * oma * cc
            d_rows = scale * (2 * float(oma) * d_oma * float(cc) + float(oma) ** 2 * d_cc) + 4 * U * float(rows_gap)
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
    return vals, bounds, dict(gap_pd=Pv - D, grad=gt, cols=cols)


def primal_longdouble(A, b, w, x, lam, loss, delta=0.0, scale=None, l2=0.0):
    return gap_longdouble(A, b, w, x, lam, loss, delta, scale, l2)[0]["primal"]


def lam_max(A, b, w, loss, delta=0.0, scale=None):
    """|grad f(0)|_inf in long double."""
    return float(gap_longdouble(A, b, w, np.zeros(A.shape[1]), 1.0, loss, delta, scale)[0]["grad_inf"])


def worst_ratio(got, vals, bounds):
    """{key: |got - value| / bound} over the keys of ``vals`` (0 / 0 counts as 0)."""
    out = {}
    for k in vals:
        err = abs(float(np.longdouble(getattr(got, k)) - vals[k]))
        out[k] = 0.0 if err == 0.0 else (err / bounds[k] if bounds[k] > 0 else np.inf)
    return out
