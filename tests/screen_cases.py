"""Gap-safe screening restated in np.longdouble: column norms, the radius, the exact rule and the fp64 guard E (no test in
here; tests/test_screen_reference.py proves this restatement on the CPU).  Built on gap_cases.gap_longdouble (its ``grad``
and its bounds); notation as there:

    P(x) = sum_i phi_i(z_i) + lam |x|_1,  z = A x,   nu = alpha grad phi(z),  g = A^T grad phi(z)

phi_i' is L-Lipschitz - least squares L = 2 scale, logistic L = scale / 4 - so the dual D is (1/L)-strongly concave, and since
the dual optimum nu^ maximises D over the feasible set, D(nu^) - D(nu) >= |nu - nu^|^2 / (2 L) for every feasible nu; with
D(nu^) <= P(x):   |nu - nu^|_2 <= r = sqrt(2 L gap).   |a_j . nu^| <= |a_j . nu| + r |a_j|_2 = alpha |g_j| + r |a_j|_2, and
a column with |a_j . nu^| < lam is zero at every optimum:

    the exact rule:   column j is discarded when   alpha |g_j| + r |a_j|_2 < lam

The guard.  The device evaluates the left side in fp64 and widens the radius to r_eff = r + E.  E |a_j|_2 bounds everything that
evaluation loses (u = 2^-53, first order, with the safety factor 2 of the other element-wise tests), every vector error
reaching column j through Cauchy-Schwarz, (|A|^T v)_j <= |a_j|_2 |v|_2:

  R, C      stored elements of the longest row / column of A (dense storage: n and m);  S1 = sum |x_j|;
            |A|_F = sqrt(sum_j |a_j|^2);  amax = max_j |a_j|_2
  margins   dz_i <= R u (|A| |x|)_i (a row sum of at most R products),  |dz|_2 <= R u |A|_F |x|_2 <= R u |A|_F S1
  candidate least squares  c = r = z - b:  dc_i = dz_i + u |r_i|,   |dc|_2 <= |dz|_2 + u |r|_2,   |c|_2 = sqrt(sum r^2)
            logistic       c = rho:        dc_i = dz_i / 4 + 5 u     (gap_cases: dq = q (1 - q) ds + 5 u q),
                                           |dc|_2 <= |dz|_2 / 4 + 5 u sqrt(m),   |c|_2 <= sqrt(m)   (|rho_i| <= 1)
  gradient  g_j = gfac a_j . c (a sum of at most C products, times the factor: gfac = 2 scale | scale):
            dg_j <= |a_j|_2 Eg,   Eg = gfac (|dc|_2 + (C + 2) u |c|_2)  (+ m 2^-1022, logistic: gap_cases' underflow term);
            also |g_j| <= gfac |c|_2 |a_j|_2
  scaling   alpha = min(1, lam / |g|_inf), |g|_inf within max_j dg_j <= Eg amax:  d(alpha) <= Eg amax / lam + u   (gap_cases)
  left side alpha |g_j| + r_eff |a_j|: two products and a sum, and the norm itself - a sum of at most C squares and a square root -
            is within (C / 2 + 2) u:
            d(left)_j <= |a_j|_2 X,   X = Eg (1 + gfac |c|_2 amax / lam) + u (4 gfac |c|_2 + (C / 2 + 4) r)
  radius    a gap known to the relative error rho moves r by rho / 2.  The tests assert rho <= 2^-20 at every point they use,
            from gap_cases' own bound (a gap that close to its rounding error certifies nothing): dr <= 2^-21 r
  E = 2 X + 2^-20 r

Safety: a column the device discards has (exact left side) <= (device left side) + (X + 2^-21 r) |a_j| - E |a_j| < lam.
Tightness: the device's left side exceeds the exact one by at most (X + 2^-21 r + E) |a_j| <= 2 E |a_j|."""
import numpy as np
import scipy.sparse as sp

import gap_cases as G

U = G.U


def lipschitz(scale, logistic):
    return 0.25 * scale if logistic else 2.0 * scale


def column_norms_ld(A):
    """|a_j|_2 in longdouble, and the stored elements of every column."""
    C = sp.csc_matrix(G._csr(A))
    sq = (C.data.astype(np.longdouble)) ** 2
    out = np.zeros(C.shape[1], dtype=np.longdouble)
    np.add.at(out, np.repeat(np.arange(C.shape[1]), np.diff(C.indptr)), sq)
    return np.sqrt(out), np.diff(C.indptr)


def guard(A, x, lam, scale, logistic, norms, radius, rr, dense=False):
    """E (float64) from exact quantities; ``dense``: the storage form decides R and C."""
    A = G._csr(A)
    m, n = A.shape
    R = n if dense else int(np.diff(A.indptr).max(initial=0))
    Cc = m if dense else int(np.diff(sp.csc_matrix(A).indptr).max(initial=0))
    fro = float(np.sqrt(np.sum(norms * norms)))
    amax = float(np.max(norms)) if n else 0.0
    s1 = float(np.sum(np.abs(np.asarray(x, dtype=np.longdouble))))
    gfac = scale if logistic else 2.0 * scale
    dz = R * U * fro * s1
    if logistic:
        cn = np.sqrt(float(m))
        dc = 0.25 * dz + 5.0 * U * cn
    else:
        cn = np.sqrt(float(rr))
        dc = dz + U * cn
    eg = gfac * (dc + (Cc + 2) * U * cn) + (m * 2.0 ** -1022 if logistic else 0.0)
    with np.errstate(divide="ignore"):
        X = eg * (1.0 + gfac * cn * amax / np.float64(lam)) + U * (4.0 * gfac * cn + (0.5 * Cc + 4.0) * float(radius))
    return 2.0 * X + 2.0 ** -20 * float(radius), eg


def screen_longdouble(A, b, x, lam, scale, logistic, dense=False):
    """dict: ``vals`` / ``bounds`` (gap_longdouble's), ``grad`` (g), ``norms``, ``radius`` (longdouble), ``left`` = alpha |g_j| +
    r |a_j| (longdouble), ``discard`` (the exact rule), ``E`` and ``Eg`` (float64)."""
    ld = np.longdouble
    vals, bounds, extra = G.gap_longdouble(A, b, x, lam, scale, logistic)
    norms, _ = column_norms_ld(A)
    radius = np.sqrt(ld(2) * ld(lipschitz(scale, logistic)) * vals["gap"])
    g = extra["grad"]
    left = vals["alpha"] * np.abs(g) + radius * norms
    rr = vals["f"] / ld(scale)   # least squares: f = scale sum r^2
    E, eg = guard(A, x, lam, scale, logistic, norms, radius, rr, dense)
    return dict(vals=vals, bounds=bounds, grad=g, norms=norms, radius=radius, left=left, discard=left < ld(lam), E=E, Eg=eg)


def grad_fp64(A, b, x, scale, logistic):
    """g in plain fp64 (SciPy's sweeps): an evaluation whose error E must dominate."""
    A = G._csr(A)
    z = A @ np.asarray(x, dtype=np.float64)
    if logistic:
        t = -b * z
        e = np.exp(-np.abs(t))
        return scale * (A.T @ (-b * (np.where(t >= 0, 1.0, e) / (1.0 + e))))
    return (2.0 * scale) * (A.T @ (z - b))


def lam_max(A, b, scale, logistic):
    return float(G.gap_longdouble(A, b, np.zeros(A.shape[1]), 1.0, scale, logistic)[0]["grad_inf"])


def fista(A, b, lam, scale, logistic, x0, iters, record=()):
    """Plain FISTA with the step 1 / (L |A|_2^2) in fp64 (soft-thresholding leaves exact zeros).  Returns (x, {k: x_k for k in
    record}); stops early once the step is exactly zero over 100 iterations."""
    A = G._csr(A)
    At = A.T.tocsr()
    b = np.asarray(b, dtype=np.float64)
    v = np.random.default_rng(0).standard_normal(A.shape[1])
    for _ in range(100):
        v = At @ (A @ v)
        v /= np.linalg.norm(v)
    step = 1.0 / (1.05 * lipschitz(scale, logistic) * float(np.linalg.norm(At @ (A @ v))))
    x = np.array(x0, dtype=np.float64)
    y, t, still, kept = x.copy(), 1.0, 0, {}
    for k in range(1, iters + 1):
        z = A @ y
        if logistic:
            tt = -b * z
            e = np.exp(-np.abs(tt))
            grad = scale * (At @ (-b * (np.where(tt >= 0, 1.0, e) / (1.0 + e))))
        else:
            grad = (2.0 * scale) * (At @ (z - b))
        w = y - step * grad
        xn = np.sign(w) * np.maximum(np.abs(w) - step * lam, 0.0)
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        y = xn + ((t - 1.0) / tn) * (xn - x)
        still = still + 1 if np.array_equal(xn, x) else 0
        x, t = xn, tn
        if k in record:
            kept[k] = x.copy()
        if still >= 100 and k > max(record, default=0):
            break
    return x, kept
