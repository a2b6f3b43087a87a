"""Inputs, exact references and a model of the summation order for the vector kernels of csrc/zf_vecops.hip (no test in here;
tests/test_vecops_cases.py proves on the CPU that the table reaches what it claims, tests/test_gpu_vecops.py runs it on the
device).  NumPy only, no library.

Sizes (SIZES, each with its reason).  Every kernel of the file is a grid-stride loop of ZF_BLOCK = 256 threads (4 waves of 64)
in g = min(ZF_MAX_GRID = 2048, ceil(n / 256)) blocks: element i belongs to thread i mod (256 g), trip i div (256 g).  The second
trip starts at element 524288, the third at 1048576.  k_reduce_partials folds the g block values with 256 threads, thread t
taking b = t, t + 256, ...: its own loop wraps from g = 257, n > 65536.  The staging workspace grows in units of 1024 elements.

Element-wise references, bit for bit.  The library is built with -ffp-contract=off: a multiply-add is two roundings, and every
expression below is NumPy's, operation by operation, in float64:
    grad_step   y - lr * jac                      (zfista/proximal_gradient.py:148)
    momentum    x + beta * (x - x_old)            (:534)
    diag_grad   d * (x - c)
    prox_l1_box   clip(copysign(max(|u| - tau, 0), u), lo, hi): the oracle's sign(u) * maximum(|u| - tau, 0) with the sign of u on
                  a zero result (tests/test_gpu_soft_threshold_bits.py::expected), then np.clip
    prox_enet_box clip(sign(u) * maximum(|u| - tau, 0) * shrink, lo, hi) with np.sign (+0 at u = -0): the ``want`` expression
                  of tests/test_gpu_enet.py
Special values (specials): +-0, +-denormal, +-1e300, +-inf, NaN and, for the prox forms, tau +- 0 .. 3 ulp with both signs,
planted in windows of WINDOW elements at the first, the last, the last first-trip, the first second-trip and the first
third-trip positions (those that exist) and at seeded places in between; a NaN compares equal to a NaN, everything else by bits.

Sums.  Magnitudes of x - y, jac, d, x and x - c are drawn from [1/2, 2] with seeded signs, so that every term is at least 1/8
in size (1/4 but for d (x - c)^2).  The reference value is formed from the inputs in np.longdouble; the bound is the first-order one for a float64 sum of
N terms in ANY order, each term carrying k roundings of its own, times the project's safety factor 2 (second-order terms, the
reference's own 2^-64 roundings):
    |device - exact| <= 2 gamma_(N + k) sum |t_j|,     gamma_q = q u / (1 - q u),  u = 2^-53
    <jac, x - y>            k = 2 (the difference, the product)
    |x - y|^2               k = 3 (the difference enters twice, the product)
    1/2 sum d (x - c)^2     k = 4 (the difference twice, the square, the product; the factor 1/2 is exact)
    lam sum |x|             k = 1 (the host's product with lam)
    sum |x|                 k = 0
    sum lam |x| + (l2/2) x^2  two fused accumulates per element: N = 2 n, k = 2 (the product (l2/2) x, its fused accumulate)
At the largest size the bounds are about 2 (1.05e6)^2 2^-53 E|t| = 2.3e-4 .. 4.3e-4 (7.3e-4 for the elastic-net sum, N = 2 n):
a missing, doubled or foreign term of size >= 1/8 lies more than two orders of magnitude outside.  max |x - y| has no order: bits.

The documented summation order (emulate_*), which predicts the bits of every sum:
  * thread (b, t) of the g blocks adds its elements b 256 + t, + 256 g, ... in that order onto 0.0 (k_enet_g: with two explicit
    fused multiply-adds per element, fma(lam, |x|, acc) then fma((l2/2) x, x, acc) - fma() below is their exact emulation);
  * each wave folds its 64 values with the halving tree of offsets 32 .. 1, v[:off] += v[off:2 off] (what __shfl_down leaves in
    lane 0), thread k adds the four wave values in wave order (zf_block_reduce);
  * k_reduce_partials does the same over the g block values of each quantity (row k of the partials starts k g doubles in):
    256 threads, thread t takes b = t, t + 256, ... onto 0.0, then the wave tree, then the four waves in order;
  * a maximum takes fmax where a sum takes +: fmax drops a NaN operand;
  * zf_eval_diag_l1 multiplies by 0.5 and by lam on the host, after the sums.

Mutants (visits(), emulate_*(..., visit=, drop_block=, row_stride=)): see tests/test_vecops_cases.py."""
import functools

import numpy as np

U = 2.0 ** -53
ZF_BLOCK, ZF_MAX_GRID, WAVE, ZF_WAVES, WS_UNIT, REDUCE_THREADS = 256, 2048, 64, 4, 1024, 256
CAP = ZF_BLOCK * ZF_MAX_GRID   # 524288: elements of one trip of the full grid
WINDOW = 32

SIZES = [
    (1, "one element: 255 idle threads"),
    (63, "one lane short of a wave"), (64, "one wave"), (65, "first lane of wave 1"),
    (255, "one thread short of a block"), (256, "one block"), (257, "first element of block 1"),
    (1023, "workspace rounding: below the unit"), (1024, "exactly one workspace unit"), (1025, "first element of unit 2"),
    (65535, "256 blocks, the last one short"), (65536, "256 blocks: one partial per reduce thread"),
    (65537, "257 blocks: k_reduce_partials wraps"),
    (524287, "grid cap 2048 blocks, the last thread idle"), (524288, "grid cap, one full trip"),
    (524289, "first element of the second trip"),
    (2 * 524288 + 257, "a partial third trip: one block and one element"),
]
N_ALL = [n for n, _ in SIZES]
N_SMALL = [n for n in N_ALL if n <= 65537]
N_LARGE = [n for n in N_ALL if n > 65537]


def size_class(n):
    for limit, name in ((65, "wave"), (257, "block"), (1025, "workspace-unit"), (65537, "reduce-wrap"), (CAP + 1, "second-trip")):
        if n <= limit:
            return name
    return "third-trip"


def grid_of(n):
    """zf_grid_for."""
    return max(1, min(-(-n // ZF_BLOCK), ZF_MAX_GRID))


def trips(n):
    return -(-n // (grid_of(n) * ZF_BLOCK))


def workspace_capacity(n):
    """zf_ws_reserve: the capacity a first call of n elements allocates."""
    return (n + WS_UNIT - 1) & ~(WS_UNIT - 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """Equal in every bit; a NaN equals a NaN (whatever its payload)."""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def differing(a, b):
    """Indices where same_bits fails."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return np.flatnonzero((na != nb) | (~na & ~nb & (bits(a) != bits(b))))


# ---- special values ---------------------------------------------------------------------------------------------------------------------
TINY = 5e-324
TAUS = (0.0, 0.1 * 0.45, 0.3)   # (0.1 * 0.45: lam * lr of the benchmark)
BOXES = ((-np.inf, np.inf), (-0.3, 0.4), (0.0, np.inf), (0.25, 0.25))
BETAS = (0.0, 0.25, 1.0)
LR = 0.37


def ulps(x, k):
    y = np.float64(x)
    for _ in range(abs(k)):
        y = np.nextafter(y, np.inf if k > 0 else -np.inf)
    return y


def specials(tau=None):
    vals = [0.0, -0.0, TINY, -TINY, 1e300, -1e300, np.inf, -np.inf, np.nan]
    if tau is not None:
        for k in range(-3, 4):
            vals += [ulps(tau, k), -ulps(tau, k)]
    return np.array(vals, dtype=np.float64)


def windows(n):
    """The planted windows as (name, first, last + 1), those that exist for n."""
    out = [("first", 0, min(WINDOW, n)), ("last", max(0, n - WINDOW), n)]
    if n > CAP:
        out += [("end of trip 1", CAP - WINDOW, CAP), ("start of trip 2", CAP, min(CAP + WINDOW, n))]
    if n > 2 * CAP:
        out += [("start of trip 3", 2 * CAP, min(2 * CAP + WINDOW, n))]
    return out


def plant(a, vals, shift, rng, step=1):
    """Writes vals cyclically (from index ``shift``, every ``step``-th - coprime to their number -, a different phase per window) at 64 seeded places and then into the windows
    of ``a``; where windows overlap the later one wins."""
    n = a.size
    if n > 4 * WINDOW:
        where = rng.choice(n, 64, replace=False)
        a[where] = rng.choice(vals, 64)
    for w, (_, lo, hi) in enumerate(windows(n)):
        k = np.arange(hi - lo)
        a[lo:hi] = vals[(k * step + shift + 7 * w) % vals.size]
    return a


@functools.lru_cache(maxsize=2)
def elementwise_inputs(n):
    """Three vectors of N(0, 1) with the special values planted at different phases, and every pair of them in the first two."""
    rng = np.random.default_rng([11, n])
    vals = specials()
    out = [plant(rng.standard_normal(n), vals, (4 * k) % 9 if n > 1 else 6 + k, rng, step=2 ** k) for k in range(3)]   # (n = 1: 1e300, -1e300, inf)
    free = np.ones(n, dtype=bool)
    for _, lo, hi in windows(n):
        free[lo:hi] = False
    if free.sum() >= vals.size ** 2:   # (n >= 255) every pair of special values in the first two vectors, outside the windows
        where = rng.choice(np.flatnonzero(free), vals.size ** 2, replace=False)
        k = np.arange(vals.size ** 2)
        out[0][where], out[1][where], out[2][where] = vals[k // vals.size], vals[k % vals.size], vals[(2 * k) % vals.size]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=4)
def prox_input(n, tau):
    """N(0, 1/4) - about half of it below the largest tau, both sides of every box - with the special values and the neighbours
    of +-tau planted."""
    rng = np.random.default_rng([13, n, TAUS.index(tau)])
    u = plant(0.5 * rng.standard_normal(n), specials(tau), 9 if n == 1 else 0, rng)   # (n = 1: the element is -tau)
    u.setflags(write=False)
    return u


# ---- element-wise references ----------------------------------------------------------------------------------------------------------
def grad_step(y, jac, lr):
    with np.errstate(invalid="ignore", over="ignore"):
        return y - lr * jac


def momentum(x, xo, beta):
    with np.errstate(invalid="ignore", over="ignore"):
        return x + beta * (x - xo)


def diag_grad(x, d, c):
    with np.errstate(invalid="ignore", over="ignore"):
        return d * (x - c)


def clip(u, lo, hi):
    """zf_clip, np.clip: minimum(maximum(u, lo), hi); a NaN stays."""
    with np.errstate(invalid="ignore"):
        t = np.where(u < lo, lo, u)
        return np.where(t > hi, hi, t)


def prox_l1_box(u, tau, lo, hi):
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(u) - tau
        a = np.where(a < 0.0, 0.0, a)
        return clip(np.copysign(a, u), lo, hi)


def prox_enet_box(u, tau, shrink, lo, hi):
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(u) - tau
        a = np.where(a < 0.0, 0.0, a)
        return clip(np.sign(u) * a * shrink, lo, hi)


# ---- inputs of the sums ----------------------------------------------------------------------------------------------------------------
class Case:
    pass


LAM, L2 = 0.75, 0.625


@functools.lru_cache(maxsize=6)
def reduction_case(n):
    """jac, x, y (model terms), d, c (P-diag), x (the l1 and elastic-net values): every magnitude of jac, x - y, d, x - c and x
    in [1/2, 2] (x - y and x - c: before the one rounding of y = x - delta), signs seeded."""
    rng = np.random.default_rng([7, n])

    def mag():
        return rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)

    c = Case()
    c.n = n
    c.jac, c.d, c.x = mag(), mag(), mag()
    c.y = c.x - mag()
    c.c = c.x - mag()
    for a in (c.jac, c.d, c.x, c.y, c.c):
        a.setflags(write=False)
    return c


def gamma(q):
    return q * U / (1.0 - q * U)


def _ref(terms, N, k):
    """(value, bound) of a sum of np.longdouble terms."""
    return float(np.sum(terms)), 2.0 * gamma(N + k) * float(np.sum(np.abs(terms)))


def model_terms_ref(jac, x, y):
    """(<jac, x - y>, |x - y|^2, max |x - y|) and their bounds (0 for the maximum: exact in any order)."""
    L = np.longdouble
    dx = x.astype(L) - y.astype(L)
    dot, b0 = _ref(jac.astype(L) * dx, x.size, 2)
    ss, b1 = _ref(dx * dx, x.size, 3)
    return np.array([dot, ss, float(np.max(np.abs(x - y)))]), np.array([b0, b1, 0.0])


def eval_diag_ref(x, d, c, lam):
    """(1/2 sum d (x - c)^2, lam sum |x|) and their bounds."""
    L = np.longdouble
    r = x.astype(L) - c.astype(L)
    f, b0 = _ref(d.astype(L) * r * r, x.size, 4)
    a, b1 = _ref(np.abs(x.astype(L)), x.size, 1)
    return np.array([0.5 * f, float(L(lam) * L(a))]), np.array([0.5 * b0, abs(lam) * b1])


def asum_ref(x):
    return _ref(np.abs(x.astype(np.longdouble)), x.size, 0)


def enet_g_ref(x, lam, l2):
    L = np.longdouble
    xl = x.astype(L)
    return _ref(L(lam) * np.abs(xl) + L(l2) / 2 * xl * xl, 2 * x.size, 2)


# ---- the summation order ---------------------------------------------------------------------------------------------------------------
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def two_prod(a, b):
    """a b = p + e exactly (Dekker / Veltkamp; no overflow or underflow at the sizes used here)."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, al * bl - (((p - ah * bh) - al * bh) - ah * bl)


def fma(a, b, c):
    """round(a b + c), one rounding, element-wise (Boldo and Melquiond, Emulation of a FMA and correctly rounded sums: proved
    algorithms using rounding to odd, 2008): a b = uh + ul and c + uh = th + tl exactly, v = tl + ul rounded to ODD, th + v."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    uh, ul = two_prod(a, b)
    th, tl = two_sum(c, uh)
    vh, vl = two_sum(tl, ul)
    fix = (vl != 0.0) & ((bits(vh).reshape(vh.shape) & np.uint64(1)) == 0)
    vh = np.where(fix, np.nextafter(vh, np.where(vl > 0.0, np.inf, -np.inf)), vh)
    return th + vh


def visits(n, mutant=None):
    """How often the grid-stride loop takes each element.  mutants: "drop-last", "drop-second-trip-first" (n > 256 g only),
    "twice" (element n // 2)."""
    v = np.ones(n, dtype=np.int64)
    if mutant == "drop-last":
        v[n - 1] = 0
    elif mutant == "drop-second-trip-first":
        assert trips(n) >= 2
        v[grid_of(n) * ZF_BLOCK] = 0
    elif mutant == "twice":
        v[n // 2] = 2
    else:
        assert mutant is None
    return v


def thread_values(n, step, visit=None):
    """(g, 256): what every thread holds after its stride loop; step(acc, elements) is one trip for a run of threads."""
    g = grid_of(n)
    stride = g * ZF_BLOCK
    acc = np.zeros(stride)
    for lo in range(0, n, stride):
        hi = min(n, lo + stride)
        sl = slice(lo, hi)
        old = acc[:hi - lo]
        new = step(old, sl)
        if visit is not None:
            new = np.where(visit[sl] == 0, old, np.where(visit[sl] == 2, step(new, sl), new))
        acc[:hi - lo] = new
    return acc.reshape(g, ZF_BLOCK)


def _op(is_max):
    return np.fmax if is_max else np.add


def wave_tree(v, is_max=False):
    """Lane 0 of the shuffle tree over the last axis (64 values)."""
    v = np.array(v, dtype=np.float64)
    op = _op(is_max)
    off = WAVE // 2
    while off:
        v[..., :off] = op(v[..., :off], v[..., off:2 * off])
        off //= 2
    return v[..., 0]


def block_values(acc, is_max=False):
    """zf_block_reduce over (g, 256) thread values: (g,)."""
    w = wave_tree(acc.reshape(acc.shape[0], ZF_WAVES, WAVE), is_max)
    op = _op(is_max)
    out = w[:, 0]
    for k in range(1, ZF_WAVES):
        out = op(out, w[:, k])
    return out


def reduce_partials(P, max_index=-1, drop_block=None, row_stride=None):
    """k_reduce_partials over the (nq, g) block values.  mutants: ``drop_block`` (that block's partials are not read),
    ``row_stride`` (row k read k * row_stride doubles in; the kernel's is g; past the end: zeros)."""
    nq, g = P.shape
    flat = np.concatenate([P.reshape(-1), np.zeros(nq * REDUCE_THREADS + nq * abs((row_stride or g) - g))])
    out = np.zeros(nq)
    for k in range(nq):
        row = flat[k * (row_stride or g):k * (row_stride or g) + g]
        is_max = k == max_index
        op = _op(is_max)
        v = np.zeros(REDUCE_THREADS)
        for lo in range(0, g, REDUCE_THREADS):
            chunk = row[lo:lo + REDUCE_THREADS]
            new = op(v[:chunk.size], chunk)
            if drop_block is not None and lo <= drop_block < lo + chunk.size:
                new[drop_block - lo] = v[drop_block - lo]
            v[:chunk.size] = new
        w = wave_tree(v.reshape(REDUCE_THREADS // WAVE, WAVE), is_max)
        acc = w[0]
        for q in range(1, REDUCE_THREADS // WAVE):
            acc = op(acc, w[q])
        out[k] = acc
    return out


def _sum_step(t):
    return lambda acc, sl: acc + t[sl]


def _max_step(t):
    return lambda acc, sl: np.fmax(acc, t[sl])


def emulate_model_terms(jac, x, y, visit=None, **reduce_mutant):
    """The three values of k_model_terms + k_reduce_partials, bit for bit."""
    n = x.size
    with np.errstate(invalid="ignore", over="ignore"):
        dx = x - y
        rows = [(_sum_step(jac * dx), False), (_sum_step(dx * dx), False), (_max_step(np.abs(dx)), True)]
        P = np.stack([block_values(thread_values(n, step, visit), is_max) for step, is_max in rows])
        return reduce_partials(P, max_index=2, **reduce_mutant)


def emulate_eval_diag(x, d, c, lam, visit=None, **reduce_mutant):
    """The two values of zf_eval_diag_l1."""
    n = x.size
    r = x - c
    rows = [_sum_step(d * (r * r)), _sum_step(np.abs(x))]
    P = np.stack([block_values(thread_values(n, step, visit)) for step in rows])
    tmp = reduce_partials(P, **reduce_mutant)
    return np.array([0.5 * tmp[0], lam * tmp[1]])


def emulate_asum(x, visit=None, **reduce_mutant):
    P = block_values(thread_values(x.size, _sum_step(np.abs(x)), visit))[None, :]
    return float(reduce_partials(P, **reduce_mutant)[0])


def emulate_enet_g(x, lam, l2, visit=None, **reduce_mutant):
    hl2 = 0.5 * l2

    def step(acc, sl):
        xv = x[sl]
        return fma(hl2 * xv, xv, fma(lam, np.abs(xv), acc))

    P = block_values(thread_values(x.size, step, visit))[None, :]
    return float(reduce_partials(P, **reduce_mutant)[0])
