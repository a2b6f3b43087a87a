"""Row counts beyond the chunk cap of the rows passes: the launch shape restated, the sizes that sit on its edges, and margins
with special values where the cap changes the walk - shared by tests/test_row_chunk_cases.py (CPU: the sizes are on their edges
and the bounds would notice a wrong walk) and tests/test_gpu_row_chunk_cap.py (GPU).  No test in here.

Every rows pass of the margins family (the loss kernels, the gap rows kernels, zf_spmv_resid_kernel) is launched on
zf_spmv_resid_chunks(m) = min(ceil(m / 1024), 1024) workgroups of 256 threads; workgroup k walks rows [k per, min((k + 1) per, m))
with per = ceil(m / chunks), thread t taking lo + t, lo + t + 256, ... .  Up to m = 2^20 a chunk has at most 1024 rows - four trips;
beyond it the chunk grows, threads make a fifth trip and more, and the last chunk becomes short."""
import numpy as np

BLOCK = 256
CHUNK_ROWS = 1024
MAX_CHUNKS = 1024            # ZF_SPMV_RESID_MAX_CHUNKS
M0, M1, M2 = 2 ** 20, 2 ** 20 + 1, 2 ** 21 + 3
SIZES = (M0, M1, M2)
DELTA = 0.75
SCALE = {"square": 0.5, "logistic": 1.0, "huber": 0.5, "poisson": 1.0}   # gfac = 1: the gradient on the identity is w o psi itself
LOSSES = tuple(SCALE)
BIG = 700.0


def chunks(m):
    """zf_spmv_resid_chunks (zfista_amd/csrc/zf_spmv.hip), restated."""
    return max(1, min((m + CHUNK_ROWS - 1) // CHUNK_ROWS, MAX_CHUNKS))


def per_chunk(m):
    c = chunks(m)
    return (m + c - 1) // c


def chunk_range(m, k):
    """[lo, hi) of workgroup k."""
    per = per_chunk(m)
    lo = k * per
    return lo, max(lo, min(lo + per, m))


def trips(m, k, thread=0):
    lo, hi = chunk_range(m, k)
    return len(range(lo + thread, hi, BLOCK))


def fifth_trip_rows(m, k=0):
    """The rows of chunk k that a thread reaches on its fifth trip (none up to m = 2^20)."""
    lo, hi = chunk_range(m, k)
    return np.arange(min(lo + 4 * BLOCK, hi), min(lo + 5 * BLOCK, hi))


def special_rows(m):
    """{name: row}: where the margins below put their special values - ``fifth`` (thread 0's fifth trip in the first chunk; at
    M0, which has none, the last row of its fourth), ``last_lo`` (the first row of the last chunk), ``last`` (the last row), and
    two rows for the zeros of both signs: in the last chunk where it has room, else on the fifth trip of chunks 1 and 2."""
    per, lo_last = per_chunk(m), chunk_range(m, chunks(m) - 1)[0]
    fifth = 4 * BLOCK if per > 4 * BLOCK else 4 * BLOCK - 1
    if m - lo_last > 4:
        zero, neg_zero = lo_last + 1, lo_last + 2
    else:
        zero, neg_zero = fifth + per, fifth + 2 * per
    return dict(fifth=fifth, last_lo=lo_last, last=m - 1, zero=zero, neg_zero=neg_zero)


def margins(loss, m, heavy=True):
    """(z, b): the margins of the per-loss row tests (``_margins`` of tests/test_gpu_poisson.py; of tests/test_gpu_weights.py for
    the other three - a grid of 2^-6), extended: zeros of both signs and, with ``heavy``, margins of +-700 on the special rows.
    Each heavy row carries far more of f than the bound of f allows to be wrong (tests/test_row_chunk_cases.py), so a walk that
    misses the last chunk, the last row or the fifth trip cannot stay inside the bound.  For Poisson exp(700) ~ 1e304: the three
    rows at +700 (one is the generator's own, at m // 2) leave f finite."""
    if loss == "poisson":
        from test_gpu_poisson import _margins

        z, b = _margins(m, seed=m)
        if not heavy:   # (the certificate's test: no row near the range of exp)
            z = np.clip(z, -3.0, 3.0)
    else:
        from test_gpu_weights import _margins

        z, b, _, _ = _margins(m, loss, seed=m)
    at = special_rows(m)
    z[at["zero"]], z[at["neg_zero"]] = 0.0, -0.0
    if heavy:
        if loss == "logistic":   # t = -b z = +700 on all three: softplus = 700, sigma = 1
            z[at["fifth"]], b[at["fifth"]] = BIG, -1.0
            z[at["last_lo"]], b[at["last_lo"]] = -BIG, 1.0
            z[at["last"]], b[at["last"]] = BIG, -1.0
        else:
            z[at["fifth"]], z[at["last_lo"]], z[at["last"]] = BIG, -BIG, BIG
            if loss == "poisson":   # (exp(-700) is nothing: in the last chunk the heavy row is the last one)
                b[at["fifth"]], b[at["last_lo"]], b[at["last"]] = 2.0, 3.0, 2.0
    return z, b


def weights(m):
    """Exposure-like weights in [0.5, 2) with a tenth of the rows switched off - the last row among them, the two other special
    rows not."""
    rng = np.random.default_rng(m + 5)
    w = 0.5 + 1.5 * rng.random(m)
    w[rng.random(m) < 0.1] = 0.0
    at = special_rows(m)
    w[at["fifth"]], w[at["last_lo"]], w[at["last"]] = 1.5, 0.75, 0.0
    return w


def loop_problem(loss, m=M1, n=64, seed=3):
    """(A csr m x n with two stored elements per row, b, lam, delta): the matrix of the in-the-loop solves."""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    i = np.arange(m)
    cols = np.stack([i % n, (7 * i + 3) % n + 0 * i], axis=1)
    cols[:, 1] = np.where(cols[:, 1] == cols[:, 0], (cols[:, 1] + 1) % n, cols[:, 1])
    vals = 0.05 * rng.standard_normal((m, 2))
    A = sp.csr_matrix((vals.ravel(), cols.ravel(), 2 * np.arange(m + 1)), shape=(m, n))
    A.sort_indices()
    x_true = np.zeros(n)
    x_true[: n // 4] = rng.standard_normal(n // 4)
    s = A @ x_true
    if loss == "logistic":
        b = np.where(s + 0.05 * rng.standard_normal(m) > 0, 1.0, -1.0)
        g0 = 0.5 * np.abs(A.T @ b)
    elif loss == "poisson":
        b = rng.poisson(np.exp(s)).astype(np.float64)
        g0 = np.abs(A.T @ (1.0 - b))
    else:
        b = s + 0.05 * rng.standard_normal(m)
        b[::97] += 3.0   # (outliers: Huber's linear branch)
        g0 = np.abs(A.T @ np.clip(b, -DELTA, DELTA)) if loss == "huber" else np.abs(A.T @ b)
    return A, b, 0.1 * float(g0.max()), DELTA if loss == "huber" else 0.0


def loss_reference(loss, z, b, w=None):
    """(f, bound of f, rho = w o psi, bound of every rho_i) at margins z in np.longdouble / float64, from the existing
    restatements: problems_ref.ls_longdouble (the m x 2 matrix [z, 0] at (1, 0)), logistic_longdouble of
    tests/test_gpu_logistic.py (the sparse identity at x = z), huber_cases.loss_longdouble, poisson_cases.loss_longdouble, and
    weight_cases.loss_longdouble for the weighted three.  The scale is SCALE[loss], so the gradient on the identity is rho."""
    import scipy.sparse as sp

    import huber_cases as H
    import poisson_cases as PC
    import weight_cases as W
    from oracle import problems_ref as P

    scale, m = SCALE[loss], z.size
    if loss == "poisson":
        return PC.loss_longdouble(z, b, scale, w=w)
    if w is not None:
        return W.loss_longdouble(z, b, w, loss, DELTA, scale)
    if loss == "huber":
        return H.loss_longdouble(z, b, DELTA, scale)
    if loss == "logistic":
        from test_gpu_logistic import logistic_longdouble

        f, g, f_bound, g_bound = logistic_longdouble(sp.identity(m, format="csr", dtype=np.float64), b, z, scale)
        return f, f_bound, g, g_bound
    f, _, f_bound, _ = P.ls_longdouble(np.stack([z, np.zeros(m)], axis=1), b, np.array([1.0, 0.0]), scale, grad=False)
    _, _, rho, rho_bound = W.loss_longdouble(z, b, np.ones(m), loss, DELTA, scale)   # (r = z - b: one rounding, inside this bound)
    return f, f_bound, rho, rho_bound
