"""Inputs and exact references for the multi-objective kernels of csrc/zf_multiobj.hip (no test in here; tests/test_mo_cases.py
proves on the CPU that the table reaches what it claims, tests/test_gpu_mo_kernels.py runs it on the device).  NumPy only.

The engine is the HOST-f kind (zf_mo_create(ZF_MO_GENERIC)): J is uploaded (set_jac), f(y) and F(x_k) are supplied.

g variants (VARIANTS), m = 2 .. 8:
  plain      no l1, no box: the prox is the identity
  l1         ratios (8 + 4 i) / 64, shifts ((3 i + 6) % 7 - 3) / 8: shift 0 is 3 / 8, so stage 0, x + tail - s0 + s0, rounds twice
  box        the scalar box [-3/4, 5/4]
  boxv       per-coordinate bound arrays
  l1_boxv    l1 with per-coordinate bounds

Branches.  lr = 1 / 2, the weight W_INT[m] has entries k / 32 and the ratios are j / 64, so coef_i = (lr w_i) ratio_i, the tail
and the shifts are multiples of 2^-12 and every operation of the staged prox on an x = k 2^-12, |x| <= 4, is exact.  Among these
32 769 candidates exactly two sit on the threshold of a stage (|u_i| == coef_i, one per sign): designated() takes NEED = 3 copies
of them per stage and then covers "strictly inside" (|u_i| < coef_i) greedily until every stage has 3; "strictly outside" comes
with those and with the seeded rest.  They are written into y at seeded places (0 and n - 1 among them, 262143 and 262144 where
they exist) and their columns of J are zeroed: w @ J = 0 and v = y - lr 0 = y exactly, so they take the same branch through
prox_host(lr w, y), recover(lr, w) and dual_eval(lr, w).  Three elements each of +0 and -0 follow and, for a box, three each
strictly below the lower bound, exactly on it, exactly on the upper bound and strictly above it (a per-coordinate bound is set
to the element's own value before the clip, or half a unit beside it; with l1 + per-coordinate bounds the designated elements of
the stages take these roles, so that a case of 64 elements holds them all).  Everything else is seeded N(0, 1) (y: 1.5 N(0, 1)).
branch_counts counts, per case, how many elements take each branch.  A case of fewer than 64 elements holds the first n // 2 of
the designated elements (n = 1: the first - on the threshold of stage 0, or on the lower bound, or a zero).

Sizes.  Grid-stride kernels (256 threads, min(ceil(n / 256), MO_GRID_MAX = 1024) workgroups: the second trip of the stride loop
starts at element 262144): N_GRID.  The persistent search k_dual_solve (512 threads, min(ceil(n / 512), G) workgroups for G CUs,
element (e, tid) of workgroup b is b 512 + tid + e stride, stride = grid 512; mo_trial_launch, zf_multiobj.hip): n_solve(G, m) and
n_streamed(G, m).  resident_rows = min(rows per workgroup, cap), cap = (min(160 KiB - static LDS - 512, 156 KiB)) / ((m + 1) 512 8)
<= capmax(m) = floor((160 KiB - 512) / ((m + 1) 512 8)) whatever the static part is: 13, 9, 7, 6, 5, 4, 4 for m = 2 .. 8.  A size
of more than capmax(m) rows per workgroup streams at least one row for certain, a size of one row per workgroup is resident.

Element-wise references, bit for bit.  The library is built with -ffp-contract=off: a multiply-add is two roundings, and every
expression below is the kernel's, operation by operation, in float64:
    wJ = ((0 + w0 J0) + w1 J1) + ...           v = y - lr wJ            y = xk + beta (xk - xo)
    coef_i = (lr w_i) ratio_i,  tail = ((0 + coef_1) + coef_2) + ...
    prox: x <- st(x + tail - s0 + s0, coef_0);  x <- st(x - coef_i - s_i, coef_i) + s_i, i = 1 .. m - 1;  x <- clip(x, lo, hi)
with st(u, t) = copysign(max(|u| - t, 0), u) - the value of oracle.problems_ref.soft_threshold with the sign of u on a zero
result (the project's convention, tests/test_gpu_soft_threshold_bits.py: the oracle's sign(u) gives +0 at u = -0 only).

Sum references.  The terms of a sum are formed element-wise as above - bit for bit what a thread adds to its accumulator - and
added with math.fsum: S, the exact sum rounded once.  A device sum adds the same N terms in an order of its own; the additions
of an exact zero (idle threads, fresh accumulators) are exact, so at most N - 1 additions on the path of any term round and
    |device - S| <= N u sum |t_j| / (1 - N u) + u |S|,      u = 2^-53                                              (sum_ref)
(the last term: S itself is rounded once).  A quantity the library multiplies on the host afterwards (g_i = ratio_i sum_i, the
Hessian's lr) carries that product's rounding on top: scaled().  Two kinds of term are not the kernel's bit for bit:
  * Hessian terms.  The kernel forms acc <- fma(a_i, b_k, acc), a_i = ratio_i sign(p - s_i) + J_i and b_k = P J_k - ratio_k c_k
    (the comment above mo_dual_terms_h; sign, P and c_k are 0 or +-1, so a_i and b_k round once, fused or not).  The reference
    takes the exact products a_i b_k (an error-free TwoProduct) and sums them exactly; the fused accumulate rounds once per
    element where two roundings would round twice, N roundings at most on any path instead of N - 1: the same bound with N.
  * Terms with exp (FDS).  The device's exp and NumPy's are each within 1 ulp (<= 2 u relative) of e^x: a term conv exp(-x)
    of the reference is within 4 u |t| of the device's before its own product rounds, 5 u |t| after; sum_ref(extra=5) adds
    5 u sum |t_j|.  Element-wise the rows of the FDS Jacobian that hold an exp are compared with np.longdouble values, in
    float64 ulps (2 at most: the device's exp and the two roundings of the row; the distance is reported).
The composed dual value (zfista/proximal_gradient.py:161-177, zf_multiobj.hip mo_dual_fn) is at most 2 m + 10 roundings of
intermediates no larger than A = sum_i w_i g_i + S_pv / (2 lr) + lr S_wJ / 2 + sum_i |w_i (F_old_i - f_y_i)| on top of the bounds
of its sums: dual_ref.  No bound is fitted to device output.

Mutants (prox(..., mutant=), jac_rows(..., stride), grid_stride_visits, solve_visits): see tests/test_mo_cases.py."""
import functools
import math

import numpy as np

U = 2.0 ** -53
X_K, Y, X_NEW = 0, 1, 2
MS = (2, 3, 4, 5, 6, 7, 8)
VARIANTS = ("plain", "l1", "box", "boxv", "l1_boxv")
N_GRID = [1, 63, 64, 65, 255, 256, 257, 1000, 262143, 262144, 262145, 524289]
N_SMALL = [n for n in N_GRID if n <= 1000]
N_LARGE = [n for n in N_GRID if n > 1000]
M_LARGE = (2, 5, 8)
LR = 0.5
BOX = (-0.75, 1.25)
MO_GRID_MAX, ZF_BLOCK, MO_SOLVE_TPB = 1024, 256, 512
W_INT = {2: (12, 20), 3: (8, 14, 10), 4: (6, 10, 9, 7), 5: (5, 8, 7, 6, 6), 6: (4, 7, 6, 5, 6, 4), 7: (3, 6, 5, 4, 6, 4, 4),
         8: (3, 5, 4, 4, 5, 4, 4, 3)}
NEED = 3   # designated elements per branch


def capmax(m):
    return (160 * 1024 - 512) // ((m + 1) * MO_SOLVE_TPB * 8)


def solve_grid(n, G):
    return max(1, min(-(-n // MO_SOLVE_TPB), G))


def rows_per_workgroup(n, G):
    """per_wg of mo_trial_launch: rows of 512 elements a workgroup owns."""
    return -(-n // (solve_grid(n, G) * MO_SOLVE_TPB))


def n_solve(G, m):
    return [1, 511, 512, 513, G * 512 - 1, G * 512, G * 512 + 1, 2 * G * 512 + 1]


def n_streamed(G, m):
    return [capmax(m) * G * 512 + 1, capmax(m) * G * 512 + G * 256 + 3]


def grid_of(n):
    return max(1, min(-(-n // ZF_BLOCK), MO_GRID_MAX))


def weights(m):
    """The three weights of the sums: uniform, interior (W_INT / 32), and the interior one with w_1 moved onto w_0."""
    wi = np.array(W_INT[m], dtype=np.float64) / 32.0
    wz = wi.copy()
    wz[0] += wz[1]
    wz[1] = 0.0
    return {"uniform": np.full(m, 1.0 / m), "interior": wi, "zero": wz}


# ---- g ----------------------------------------------------------------------------------------------------------------------------------
class GSpec:
    """ratios / shifts (None without l1) and lo / hi: None, scalars or arrays of n."""

    def __init__(self, m, ratios, shifts, lo, hi):
        self.m, self.ratios, self.shifts, self.lo, self.hi = m, ratios, shifts, lo, hi
        self.l1 = ratios is not None
        self.box = lo is not None
        self.arrays = self.box and np.ndim(lo) > 0

    def s(self):
        return self.shifts if self.shifts is not None else np.zeros(self.m)

    def oracle(self, n):
        from oracle.problems_ref import ProblemRef

        return ProblemRef(n, self.m, self.ratios, self.shifts, (self.lo, self.hi) if self.box else None)


def l1_params(m):
    i = np.arange(m)
    return (8.0 + 4.0 * i) / 64.0, ((3 * i + 6) % 7 - 3) / 8.0


def coefs(g, lr, w):
    """mo_fill_w: coef_i = (lr w_i) ratio_i (0 without l1), tail = ((0 + coef_1) + coef_2) + ..."""
    w = np.asarray(w, dtype=np.float64)
    coef = (lr * w) * g.ratios if g.l1 else np.zeros(g.m)
    tail = 0.0
    for i in range(1, g.m):
        tail = tail + float(coef[i])
    return coef, tail


def soft(u, tau):
    with np.errstate(invalid="ignore"):
        a = np.abs(u) - tau
        a = np.where(a < 0.0, 0.0, a)
    return np.copysign(a, u)


def clip(u, lo, hi):
    with np.errstate(invalid="ignore"):
        t = np.where(u < lo, lo, u)
        return np.where(t > hi, hi, t)


def prox(g, coef, tail, x, mutant=None, before_clip=False):
    """mo_prox / mo_prox_t.  mutants: "no-shift-back", "no-tail", "lo0"."""
    x = np.asarray(x, dtype=np.float64)
    if g.l1:
        s = g.shifts
        t = 0.0 if mutant == "no-tail" else tail
        x = soft(x + t - s[0] + s[0], coef[0])
        for i in range(1, g.m):
            x = soft(x - coef[i] - s[i], coef[i])
            if mutant != "no-shift-back":
                x = x + s[i]
    if g.box and not before_clip:
        lo = g.lo[0] if (mutant == "lo0" and g.arrays) else g.lo
        x = clip(x, lo, g.hi)
    return x


def branch_counts(g, coef, tail, x):
    """How many elements of x take each branch of prox(g, coef, tail, .)."""
    x = np.asarray(x, dtype=np.float64)
    out = {("zero", "+0"): int(((x == 0) & ~np.signbit(x)).sum()), ("zero", "-0"): int(((x == 0) & np.signbit(x)).sum())}
    if g.l1:
        s = g.shifts
        u = x + tail - s[0] + s[0]
        for i in range(g.m):
            if i:
                u = x - coef[i] - s[i]
            a = np.abs(u)
            out[("stage", i, "inside")] = int((a < coef[i]).sum())
            out[("stage", i, "on")] = int((a == coef[i]).sum())
            out[("stage", i, "outside")] = int((a > coef[i]).sum())
            x = soft(u, coef[i]) + (s[i] if i else 0.0)
    if g.box:
        for name, hit in (("below", x < g.lo), ("on_lo", x == g.lo), ("inside", (x > g.lo) & (x < g.hi)), ("on_hi", x == g.hi),
                          ("above", x > g.hi)):
            out[("clip", name)] = int(np.sum(hit))
    return out


@functools.lru_cache(maxsize=None)
def designated(m):
    """Candidates k 2^-12 such that every stage has NEED elements on and strictly inside its threshold under the weight
    lr W_INT[m] / 32.  The first is on the threshold of stage 0."""
    ratios, shifts = l1_params(m)
    g = GSpec(m, ratios, shifts, None, None)
    coef, tail = coefs(g, LR, weights(m)["interior"])
    cand = np.arange(-2 ** 14, 2 ** 14 + 1, dtype=np.float64) / 4096.0
    hits = np.zeros((cand.size, 3 * m), dtype=bool)
    x = cand
    u = x + tail - shifts[0] + shifts[0]
    for i in range(m):
        if i:
            u = x - coef[i] - shifts[i]
        a = np.abs(u)
        hits[:, 3 * i], hits[:, 3 * i + 1], hits[:, 3 * i + 2] = a == coef[i], a < coef[i], a > coef[i]
        x = soft(u, coef[i]) + (shifts[i] if i else 0.0)
    # the two candidates on a threshold (+ and -) are the only ones: NEED copies of them, then a greedy cover of "inside"
    picked = []
    for i in range(m):
        on = np.flatnonzero(hits[:, 3 * i])
        assert on.size >= 1, f"no candidate sits on the threshold of stage {i}"
        picked += [on[k % on.size] for k in range(NEED)]
    need = np.maximum(NEED - hits[picked][:, 1::3].sum(axis=0), 0)
    order = np.random.default_rng(m).permutation(cand.size)   # (ties: not always the smallest candidate)
    inside = hits[order][:, 1::3]
    free = np.ones(cand.size, dtype=bool)
    while need.any():
        gain = inside[:, need > 0].sum(axis=1) * free
        k = int(np.argmax(gain))
        assert gain[k] > 0, "no candidate is strictly inside the threshold of some stage"
        picked.append(order[k])
        free[k] = False
        need = np.maximum(need - inside[k], 0)
    return cand[picked]


class Case:
    pass


@functools.lru_cache(maxsize=6)
def case(m, variant, n):
    """The inputs of one case: J (m x n), y, xk, xo (n), g (GSpec), the places of the designated elements."""
    assert m in MS and variant in VARIANTS and n >= 1
    rng = np.random.default_rng([m, VARIANTS.index(variant), n])
    c = Case()
    c.m, c.variant, c.n, c.lr = m, variant, n, LR
    c.J = rng.standard_normal((m, n))
    c.y = 1.5 * rng.standard_normal(n)
    c.xk, c.xo = rng.standard_normal(n), rng.standard_normal(n)
    l1 = variant in ("l1", "l1_boxv")
    ratios, shifts = l1_params(m) if l1 else (None, None)
    # designated values and their clip roles (None: no role)
    vals, roles = [], []
    if l1:
        d = designated(m)
        vals += list(d)
        roles += [None] * d.size
    clip_roles = ["on_lo", "on_hi", "below", "above"] * 3
    if variant == "box":
        where = {"on_lo": BOX[0], "on_hi": BOX[1], "below": BOX[0] - 0.5, "above": BOX[1] + 0.5}
        vals += [where[r] for r in clip_roles]
        roles += clip_roles
    elif variant == "boxv":
        vals += list(np.round(rng.standard_normal(len(clip_roles)) * 1024.0) / 1024.0)
        roles += clip_roles
    elif variant == "l1_boxv":   # the designated elements of the stages take the clip roles as well (a case of 64 holds them all)
        roles[1:1 + len(clip_roles)] = clip_roles
    zeros = [0.0, -0.0] * 3
    if l1:   # keep the first (the element of n = 1) in front, then alternate the kinds so that a short case holds all of them
        vals, roles = vals[:1] + zeros[:2] + vals[1:] + zeros[2:], roles[:1] + [None] * 2 + roles[1:] + [None] * 4
    else:
        vals, roles = vals + zeros, roles + [None] * 6
    if variant in ("box", "boxv"):
        vals, roles = vals[::-1], roles[::-1]   # (n = 1: an element on a bound)
        k0 = roles.index("on_lo")
        vals[0], vals[k0], roles[0], roles[k0] = vals[k0], vals[0], roles[k0], roles[0]
    K = len(vals) if n >= 64 else min(len(vals), max(1, n // 2))
    assert K <= n, (m, variant, n, K)
    vals, roles = np.array(vals[:K], dtype=np.float64), roles[:K]
    fixed = [j for j in (0, n - 1, 262143, 262144) if 0 <= j < n]
    fixed = list(dict.fromkeys(fixed))[:K]
    others = np.setdiff1d(np.arange(n), fixed)
    pos = np.array(fixed + list(rng.choice(others, K - len(fixed), replace=False)), dtype=np.int64)
    c.pos, c.roles = pos, roles
    c.y[pos] = vals
    c.J[:, pos] = 0.0
    lo = hi = None
    if variant == "box":
        lo, hi = BOX
    elif variant in ("boxv", "l1_boxv"):
        lo, hi = -rng.uniform(0.2, 1.5, n), rng.uniform(0.2, 2.0, n)
        g0 = GSpec(m, ratios, shifts, None, None)
        coef, tail = coefs(g0, LR, weights(m)["interior"])
        z = prox(g0, coef, tail, c.y[pos])
        for k, role in enumerate(roles):
            j = pos[k]
            if role == "on_lo":
                lo[j], hi[j] = z[k], z[k] + 1.0
            elif role == "on_hi":
                lo[j], hi[j] = z[k] - 1.0, z[k]
            elif role == "below":
                lo[j], hi[j] = z[k] + 0.5, z[k] + 1.0
            elif role == "above":
                lo[j], hi[j] = z[k] - 1.0, z[k] - 0.5
    c.g = GSpec(m, ratios, shifts, lo, hi)
    for a in (c.J, c.y, c.xk, c.xo):
        a.setflags(write=False)
    return c


def engine(c, kind=0):
    """A device engine holding the case: x_k = x_{k-1} = xk, y, J.  The caller closes it."""
    from zfista_amd.multiobjective import MoEngine

    g = c.g
    eng = MoEngine(kind, c.m, c.n, g.ratios, g.shifts if g.l1 else None, (g.lo, g.hi) if (g.box and not g.arrays) else None)
    if g.arrays:
        eng.set_bounds(g.lo, g.hi)
    eng.set_x0(c.xk)
    eng.put(Y, c.y)
    eng.set_jac(c.J)
    return eng


# ---- element-wise references ------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def jac_rows(J, stride=None):
    """The rows of J as the kernels index the uploaded m x n block: row i starts i * stride doubles in (stride = n; the
    mutant: n_pad, reading past the block's end as zeros)."""
    m, n = J.shape
    if stride is None or stride == n:
        return J
    flat = np.concatenate([J.reshape(-1), np.zeros(m * (stride - n) + 64)])
    return np.stack([flat[i * stride:i * stride + n] for i in range(m)])


def w_dot_J(w, J):
    acc = np.zeros(J.shape[1])
    for i in range(J.shape[0]):
        acc = acc + w[i] * J[i]
    return acc


def trial_point(c, lr, w, mutant=None, stride=None):
    """wJ, v, p = prox(lr w, v) and err = max |p - y| as k_recover / k_dual_solve form them."""
    J = jac_rows(c.J, stride)
    wJ = w_dot_J(w, J)
    v = c.y - lr * wJ
    coef, tail = coefs(c.g, lr, w)
    p = prox(c.g, coef, tail, v, mutant)
    with np.errstate(invalid="ignore"):
        d = np.abs(p - c.y)
    err = float(np.max(np.where(np.isnan(d), 0.0, d), initial=0.0))   # (fmax drops a NaN)
    return wJ, v, p, err


def commit_ref(xk, xo, beta, nesterov):
    return xk + beta * (xk - xo) if nesterov else xk.copy()


def jos1_jac(y, n=None):
    dn = float(y.size if n is None else n)
    return np.stack([2 * y / dn, 2 * (y - 2) / dn])


# ---- sums ------------------------------------------------------------------------------------------------------------------------------
def sum_ref(t, extra=0.0, count=None):
    """(S, bound): the exact sum of the terms rounded once, and the bound of the module's text for ANY order of adding them.
    ``extra``: further roundings every term may carry (in units of u |t_j|).  ``count``: N, if not len(t)."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    N = t.size if count is None else count
    S = math.fsum(t)
    A = float(np.sum(np.abs(t))) * (1.0 + 1e-9)   # (sum |t_j|, rounded up: NumPy's pairwise sum is within log2(N) u of it)
    return S, N * U * A / (1.0 - N * U) + extra * U * A + U * abs(S)


def scaled(S, B, factor):
    """A sum and its bound after ONE more floating-point product with ``factor``."""
    return factor * S, abs(factor) * B + U * abs(factor) * (abs(S) + B)


def g_terms(g, x):
    """m x n: |x_j - s_i|; and the number of box violations."""
    x = np.asarray(x, dtype=np.float64)
    t = np.abs(x[None, :] - g.s()[:, None])
    with np.errstate(invalid="ignore"):
        viol = int(np.sum((x < g.lo) | (x > g.hi))) if g.box else 0
    return t, viol


def g_ref(g, x, visits=None):
    """g(x) as mo_g_values: (values, bounds); inf with a violation, 0 without l1."""
    t, viol = g_terms(g, x)
    if visits is not None:
        t = t * visits
    if viol:
        return np.full(g.m, np.inf), np.zeros(g.m)
    if not g.l1:
        return np.zeros(g.m), np.zeros(g.m)
    out = [scaled(*sum_ref(t[i]), g.ratios[i]) for i in range(g.m)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def dual_terms(c, lr, w, mutant=None, stride=None):
    """The 2m + 2 rows of terms of k_dual_eval: [0, m) |p - s_i|, [m] (p - v)^2, [m + 1] wJ^2, [m + 2, 2m + 2) J_i (p - y)."""
    J = jac_rows(c.J, stride)
    wJ, v, p, _ = trial_point(c, lr, w, mutant, stride)
    dv, dy = p - v, p - c.y
    return np.concatenate([np.abs(p[None, :] - c.g.s()[:, None]), (dv * dv)[None, :], (wJ * wJ)[None, :], J * dy[None, :]])


def dual_sums(c, lr, w, terms=None, visits=None, padded=0):
    """dual_eval(lr, w) as the library returns it: 2m + 2 values (the first m times their ratio, 0 without l1) and bounds.
    ``visits`` / ``padded``: the mutants of the partition (how often each element is taken; elements of J = 0, y = 0 added)."""
    m, g = c.m, c.g
    t = dual_terms(c, lr, w) if terms is None else terms
    if visits is not None:
        t = t * visits[None, :]
    if padded:
        assert not g.arrays
        zero = Case()
        zero.J, zero.y, zero.g = np.zeros((m, 1)), np.zeros(1), g
        t = np.concatenate([t, np.repeat(dual_terms(zero, lr, w), padded, axis=1)], axis=1)
    S, B = np.zeros(2 * m + 2), np.zeros(2 * m + 2)
    for q in range(2 * m + 2):
        S[q], B[q] = sum_ref(t[q])
        if q < m:
            S[q], B[q] = scaled(S[q], B[q], g.ratios[q]) if g.l1 else (0.0, 0.0)
    return S, B


def post_sums(c, lr, w, p):
    """post_terms(lr, w, p): [0, m) J_i (p - y), [m] |p - (y - lr wJ)|^2 and bounds."""
    wJ = w_dot_J(w, c.J)
    v = c.y - lr * wJ
    dy, dv = p - c.y, p - v
    rows = list(c.J * dy[None, :]) + [dv * dv]
    out = [sum_ref(r) for r in rows]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def dual_ref(c, lr, w, f_y, F_old, S=None, B=None):
    """The negated dual and its gradient at w as zfista/proximal_gradient.py:161-177 compose them from the 2m + 2 sums
    (mo_dual_fn; the same lines inside k_dual_solve): (fun, bound, jac, bounds)."""
    m = c.m
    if S is None:
        S, B = dual_sums(c, lr, w)
    w = np.asarray(w, dtype=np.float64)
    LD = np.longdouble
    dF = np.asarray(F_old, dtype=LD) - np.asarray(f_y, dtype=LD)
    gp, pv, wj, dots = S[:m].astype(LD), LD(S[m]), LD(S[m + 1]), S[m + 2:].astype(LD)
    fun = -np.sum(w * gp) - pv / 2 / LD(lr) + LD(lr) / 2 * wj + np.sum(w * dF)
    A = float(np.sum(np.abs(w * gp)) + abs(pv) / 2 / lr + lr / 2 * abs(wj) + np.sum(np.abs(w * dF)))
    bound = float(np.sum(np.abs(w) * B[:m]) + B[m] / 2 / lr + lr / 2 * B[m + 1]) + (2 * m + 10) * U * A
    jac = -gp - dots + dF
    jb = B[:m] + B[m + 2:] + 4 * U * (np.abs(gp) + np.abs(dots) + np.abs(dF)).astype(float)
    return float(fun), bound, jac.astype(float), jb


# ---- the Hessian -----------------------------------------------------------------------------------------------------------------------
def prox_ad(g, coef, tail, x):
    """mo_prox_ad: the prox, d prox / d x (P) and d prox / d coef_k (c, m x n), all 0 / +-1 patterns."""
    m = g.m
    x = np.asarray(x, dtype=np.float64)
    P, c = np.ones_like(x), np.zeros((m,) + x.shape)
    if g.l1:
        s = g.shifts
        u = x + tail - s[0] + s[0]
        act, sg = (np.abs(u) > coef[0]).astype(float), np.where(u < 0.0, -1.0, 1.0)
        x = soft(u, coef[0])
        P = act
        c[0] = -sg * act
        c[1:] = act
        for i in range(1, m):
            u = x - coef[i] - s[i]
            act, sg = (np.abs(u) > coef[i]).astype(float), np.where(u < 0.0, -1.0, 1.0)
            x = soft(u, coef[i]) + s[i]
            P = P * act
            c[i] = c[i] - 1.0
            c = c * act
            c[i] = c[i] - sg * act
    if g.box:
        inside = ((x >= g.lo) & (x <= g.hi)).astype(float)
        x = clip(x, g.lo, g.hi)
        P, c = P * inside, c * inside
    return x, P, c


def two_prod(a, b):
    """a b = p + e exactly (Dekker / Veltkamp; no overflow or underflow at the sizes used here)."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, al * bl - (((p - ah * bh) - al * bh) - ah * bl)


def hessian_ref(c, lr, w):
    """dual_hessian(lr, w): (H, bounds), m x m; H_ik = lr sum_j a_ij b_kj."""
    m, g = c.m, c.g
    wJ = w_dot_J(w, c.J)
    v = c.y - lr * wJ
    coef, tail = coefs(g, lr, w)
    p, P, cc = prox_ad(g, coef, tail, v)
    e = p[None, :] - g.s()[:, None]
    sg = np.where(e > 0.0, 1.0, np.where(e < 0.0, -1.0, 0.0))
    if g.l1:
        a = g.ratios[:, None] * sg + c.J
        b = -g.ratios[:, None] * cc + P[None, :] * c.J
    else:
        a, b = c.J, P[None, :] * c.J
    H, Bd = np.zeros((m, m)), np.zeros((m, m))
    for i in range(m):
        for k in range(m):
            pr, er = two_prod(a[i], b[k])
            S = math.fsum(np.concatenate([pr, er]))
            N, A = c.n, float(np.sum(np.abs(pr))) * (1.0 + 1e-9)
            H[i, k], Bd[i, k] = scaled(S, N * U * A / (1.0 - N * U) + 2 * U * A + U * abs(S), lr)
    return H, Bd


# ---- the built-in problems ------------------------------------------------------------------------------------------------------
def jos1_f_ref(y):
    """f(y) of JOS1 from the two sums (mo_f_from_sums: sqrt, square, / n): (f, bounds)."""
    dn = float(y.size)
    t = y - 2
    out = []
    for terms in (y * y, t * t):
        S, B = sum_ref(terms)
        out.append((S / dn, (B + 4 * U * abs(S)) / dn))
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def fds_ref(y):
    """FDS (zfista/problems.py:309-328) at y, unsharded: f (3) with bounds, the Jacobian rows - row 0 (no exp) in float64 in the
    kernel's order, rows 1 and 2 in np.longdouble (the reference's own exp and roundings are then 2^-11 of a float64 ulp and do
    not count against the kernel) - and the allowance of row 1 for the order of sum(y) behind exp(sum(y) / n)."""
    n = y.size
    dn = float(n)
    LD = np.longdouble
    idx = np.arange(1, n + 1, dtype=np.float64)
    conv = (np.arange(1, n + 1, dtype=np.int64) * (n - np.arange(n, dtype=np.int64))).astype(np.float64)
    t = y - idx
    t2 = t * t
    ex = np.exp(-y)
    S0, B0 = sum_ref(idx * (t2 * t2))
    S1, B1 = sum_ref(y)
    S2, B2 = sum_ref(y * y)
    S3, B3 = sum_ref(conv * ex, extra=5)
    e_mean = float(np.exp(LD(S1) / LD(dn)))
    rel_e = (B1 + U * abs(S1)) / dn * 1.0000001 + 4 * U        # exp of a perturbed argument + its own ulp (+ NumPy's)
    f = np.array([S0 / (dn * dn), e_mean + S2, S3 / (dn * (dn + 1))])
    fb = np.array([(B0 + 3 * U * abs(S0)) / (dn * dn), e_mean * rel_e + B2 + 4 * U * abs(S2) + U * abs(f[1]),
                   (B3 + 3 * U * abs(S3)) / (dn * (dn + 1))])
    c1, den = 4 / (dn * dn), dn * (dn + 1)
    yl = y.astype(LD)
    rows = [c1 * idx * (t * t * t), np.exp(LD(S1) / LD(dn)) / LD(dn) + 2 * yl, -conv.astype(LD) * np.exp(-yl) / LD(den)]
    row1_extra = e_mean / dn * (rel_e + U)
    return f, fb, rows, row1_extra


def ulp_distance(a, b, allow=0.0):
    """max(|a - b| - allow, 0) in units of the float64 spacing at b, element-wise (b may be np.longdouble)."""
    d = np.abs(np.asarray(a, dtype=np.longdouble) - np.asarray(b, dtype=np.longdouble)) - allow
    return (np.maximum(d, 0) / np.spacing(np.abs(np.asarray(b, dtype=np.float64)))).astype(np.float64)


# ---- models of the element partitions and their mutants ----------------------------------------------------------------------
def grid_stride_visits(n, mutant=None):
    """How often the 256-thread grid-stride loop takes each element.  mutants: "drop-last", "drop-second-trip-first"."""
    stride = grid_of(n) * ZF_BLOCK
    visits = np.zeros(n, dtype=np.int64)
    j0 = np.arange(stride, dtype=np.int64)   # blockIdx * 256 + threadIdx
    trip = 0
    while trip * stride < n:
        j = j0 + trip * stride
        j = j[j < n]
        if mutant == "drop-last":
            j = j[j != n - 1]
        if mutant == "drop-second-trip-first" and trip == 1:
            j = j[1:]
        np.add.at(visits, j, 1)
        trip += 1
    return visits


def solve_visits(n, G, ER, mutant=None):
    """How often k_dual_solve takes each element with ER resident rows: (visits, padded) - padded counts resident slots past n
    (zeros in LDS) that were taken.  mutants: "count-padded" (the j >= n guard of the resident loop dropped), "skip-streamed-row"."""
    stride = solve_grid(n, G) * MO_SOLVE_TPB
    visits = np.zeros(n, dtype=np.int64)
    j0 = np.arange(stride, dtype=np.int64)
    padded = 0
    for e in range(ER):
        j = j0 + e * stride
        if mutant == "count-padded":
            padded += int((j >= n).sum())
        np.add.at(visits, j[j < n], 1)
    e = ER + (1 if mutant == "skip-streamed-row" else 0)
    while e * stride < n:
        j = j0 + e * stride
        np.add.at(visits, j[j < n], 1)
        e += 1
    return visits, padded


def resident_rows(n, G, cap):
    return min(rows_per_workgroup(n, G), cap)


# ---- the state of a persistent search -------------------------------------------------------------------------------------------
def solve_inputs(c):
    """f(y), F(x_k) for solve_dual_device on the case: the interior weight W_INT / 32 is the minimiser of the negated dual
    (its gradient there is the constant vector 1, so the KKT conditions of the simplex hold; the dual is strongly convex for
    n >> m, rows of J being independent N(0, 1)).  n < 64: objective 0 is made to dominate by 100, the minimiser is the
    vertex e_0 whatever the rank of J."""
    m = c.m
    f_y = np.arange(1, m + 1) / 4.0
    if c.n < 64:
        dF = np.zeros(m)
        dF[0] = -100.0
    else:
        w = weights(m)["interior"]
        S, _ = dual_sums(c, c.lr, w)
        dF = 1.0 + S[:m] + S[m + 2:]
    return f_y, f_y + dF
