"""K responses on one CSR matrix: the case tables of the sparse multi-response tests, their inputs and their reference closures
(no test in here; tests/test_sparse_multiresponse_cases.py keeps the tables honest on the CPU).

    X in R^{n x K}, B in R^{m x K}, flattened in C order:  x[j K + k] = X[j, k],  b[i K + k] = B[i, k]

is the existing sparse margins problem on sp.kron(A, sp.identity(K)): row i K + k of that matrix holds the elements of row i of
A, in the same order, at columns j K + k, so mean row length, lanes per row, split rows and segments are those of A, per
response - for the transpose too (``kron``, ``plan_claim``).  The K-response sweeps (csrc/zf_kernels_spmm.h) sum response k
exactly as the plain sweeps sum a vector, so the existing device classes on the Kronecker matrix are the EXACT yardstick of the
new ones (bit for bit), and the reference solver (oracle.cpu_ref) on the SciPy-sparse closures of the Kronecker matrix
(``kron_ref``: sparse_cases.SparseLeastSquaresL1Ref, weight_cases.WeightedRef, penalty_cases.PenaltyRef) is the independent one
(1e-10).  ``second_ref`` is the second CPU evaluation of the same problem: per response, on the dense form of A.

Shapes: SHAPES covers the five lane widths in both sweeps (asserted on the CPU); the sweep matrices cover every remainder path
per lane width, the split threshold from both sides and more split rows than one tail workgroup holds.

Seeds: a case whose two CPU evaluations decided a trial differently was given the next seed; the number of replaced seeds is
REPLACED below (counted when the table was drawn)."""
import numpy as np
import scipy.sparse as sp

import multiresponse_cases as M
import penalty_cases as PC
import sparse_cases as S
import weight_cases as W

SCALE = M.SCALE
KS = tuple(range(2, 17))           # the sweeps, element-wise: every K is a kernel instantiation of its own (ZF_SPMM_CASE)
MANY_SPLIT_KS = (2, 4, 7, 16)      # ... on `many-split` (1.2e6 elements per sweep): both gather forms at both pipeline depths
SOLVE_KS = (2, 5, 9, 12, 16)       # the solves of CASES (ALL_K: every K)
THRESHOLD = 4096                   # zfista_amd.sparse.SPLIT_THRESHOLD (asserted on the CPU)
LANES = (4, 8, 16, 32, 64)
REPLACED = 0   # seeds replaced when the tables were drawn (ALL_K included)
BOX = M.BOX
# (m, n, density): lanes per row of A / of A^T = 8 / 8, 64 / 8, 4 / 16, 32 / 16
SHAPES = {"a": (60, 90, 0.15), "b": (40, 300, 0.25), "c": (200, 50, 0.1), "d": (33, 67, 0.6)}
SHAPE_LANES = {"a": (8, 8), "b": (64, 8), "c": (4, 16), "d": (32, 16)}


def lanes_of(A):
    """Lanes per row of the sweep over A: zfista_amd.sparse.lanes_for restated (the largest power of two in [4, 64] that is at
    most the mean row length)."""
    A = sp.csr_matrix(A)
    mean = A.nnz / max(A.shape[0], 1)
    L = 4
    while 2 * L <= min(mean, 64):
        L *= 2
    return L


def kron(A, K):
    """sp.kron(A, I_K) as canonical CSR."""
    big = sp.kron(sp.csr_matrix(A), sp.identity(K, format="csr"), format="csr")
    big.sum_duplicates()
    big.sort_indices()
    return big


def make(loss, shape, K, seed, lam_frac=0.1):
    """(A csr, B, lam): B = A X_true + noise (square) or its sign (logistic); lam = lam_frac lam_max.  An empty row and an empty
    column are kept."""
    m, n, density = SHAPES[shape] if isinstance(shape, str) else shape
    rng = np.random.default_rng(seed)
    A = sp.random(m, n, density=density, random_state=rng, data_rvs=rng.standard_normal, format="lil")
    A[m // 2, :] = 0
    A[:, n // 2] = 0
    A = A.tocsr()
    A.eliminate_zeros()
    A.sum_duplicates()
    A.sort_indices()
    k = max(1, min(10, n // 4))
    X = np.zeros((n, K))
    X[:k] = rng.standard_normal((k, K))
    if loss == "logistic":
        B = np.sign(A @ X + 0.1 * rng.standard_normal((m, K)))
        B[B == 0] = 1.0
        lam = lam_frac * SCALE[loss] * np.max(np.abs(A.T @ (B / 2)))
    else:
        B = A @ X + 0.01 * rng.standard_normal((m, K))
        lam = lam_frac * 2 * SCALE[loss] * np.max(np.abs(A.T @ B))
    return A, B, float(lam)


class Case(M.Case):
    """multiresponse_cases.Case with a sparse A: ``shape`` names an entry of SHAPES."""

    def __init__(self, loss, K, shape, seed, **kw):
        m, n, _ = SHAPES[shape]
        super().__init__(loss, K, m, n, seed, **kw)
        self.shape = shape

    @property
    def id(self):
        return "sp-" + super().id

    def data(self):
        A, B, lam = make(self.loss, self.shape, self.K, self.seed, self.lam_frac)
        Wt = M.make_weights(self.m, self.K, self.seed, self.weights)
        Pf = M.make_factors(self.n, self.K, self.seed, self.factors)
        return A, B, lam, Wt, Pf, self.l2fac * lam


def kron_ref(case):
    """The case on sp.kron(A, I_K) through the SciPy-sparse closures the project already has."""
    A, B, lam, Wt, Pf, l2 = case.data()
    K = case.K
    big, b = kron(A, K), B.reshape(-1)
    scale = SCALE[case.loss]
    w = None if Wt is None else M.wide(Wt, case.m, K).reshape(-1)
    if Pf is not None:
        return PC.PenaltyRef(big, b, lam, M.wide(Pf, case.n, K).reshape(-1), case.loss, scale=scale, bounds=case.box, w=w)
    if w is not None or l2 > 0 or case.loss == "logistic":   # (unit weights: 1 * v = v exactly)
        return W.WeightedRef(big, b, lam, np.ones(b.size) if w is None else w, case.loss, scale=scale, bounds=case.box, l2=l2)
    return S.SparseLeastSquaresL1Ref(big, b, lam, scale=scale, bounds=case.box)


def second_ref(case):
    """The second CPU evaluation of a case: multiresponse_cases.MRRef per response (A @ X, A.T @ R) on the DENSE form of A - BLAS's
    order of the same sums (SciPy's CSR products on A and on the Kronecker matrix add the same products in the same order)."""
    ref = M.MRRef(case)
    ref.A = ref.A.toarray()
    return ref


def _table():
    out = []
    for loss, s0 in (("square", 100), ("logistic", 200)):
        out += [
            Case(loss, 2, "a", s0 + 0),
            Case(loss, 2, "d", s0 + 1, weights="real"),
            Case(loss, 5, "b", s0 + 2, factors="pos"),
            Case(loss, 5, "d", s0 + 3, l2fac=0.01),
            Case(loss, 9, "c", s0 + 4),
            Case(loss, 16, "d", s0 + 5, weights="mask", box=BOX),
            Case(loss, 5, "a", s0 + 6, factors="zero"),
            Case(loss, 12, "a", s0 + 7, weights="real", factors="pos"),
            Case(loss, 16, "c", s0 + 8, weights="mask", l2fac=0.01),
        ]
    return out


def lr_of(loss, shape, K, seed, lam_frac, c):
    """c / L with L = gfac |A|_2^2 (logistic: a quarter of it): the step as a multiple of the safe one."""
    A = make(loss, shape, K, seed, lam_frac)[0]
    return float(c / ((1.0 if loss == "square" else 0.25) * np.linalg.norm(A.toarray(), 2) ** 2))


# "Backtracking failed" AFTER accepted iterations, with one trial per iteration (max_backtrack_iter = 1): a step of c / L with c
# beyond 2 passes the sufficient-decrease test while few columns are active and fails once more are.  (K, shape, seed, lam_frac, c) -
# found by a scan on the CPU (tests/test_sparse_multiresponse_cases.py asserts that the oracle accepts iterations first).
FAILK = {"square": [(5, "d", 308, 0.8, 3.8), (16, "a", 313, 0.8, 3.0)],
         "logistic": [(2, "a", 404, 0.5, 2.2), (5, "d", 407, 0.5, 3.2)]}


def _endings():
    """Every way a run ends, twice per loss: by tol; "Backtracking failed" at once and after accepted iterations; one iteration."""
    out = []
    for loss, s0 in (("square", 300), ("logistic", 400)):
        for j, (K, shape) in enumerate(((2, "a"), (9, "d"))):
            s = s0 + 10 * j
            for tag, kw in (("tol", dict(opts=dict(tol=1e-1 if loss == "square" else 3e-2, max_iter=200))),
                            ("fail0", dict(opts=dict(lr=1e3, max_backtrack_iter=1))),
                            ("one", dict(opts=dict(max_iter=1)))):
                c = Case(loss, K, shape, s, **kw)
                c.tag = tag
                out.append(c)
        for K, shape, sd, frac, cc in FAILK[loss]:
            c = Case(loss, K, shape, sd, lam_frac=frac, opts=dict(lr=lr_of(loss, shape, K, sd, frac, cc), max_backtrack_iter=1, max_iter=200))
            c.tag = "failk"
            out.append(c)
    return out


def _all_k():
    """One short solve per loss and per K = 2 .. 16 through the solver's own launches: the shape, hence the two lane widths, by
    K % 4; none / weights / factors by K % 3 (multiresponse_cases.ALL_K's seeds and options)."""
    out = []
    for loss, s0 in (("square", 600), ("logistic", 700)):
        for K in range(2, 17):
            extra = (dict(), dict(weights="real"), dict(factors="pos"))[K % 3]
            c = Case(loss, K, "abcd"[K % 4], s0 + K, opts=dict(max_iter=30), **extra)
            c.tag = "allk"
            out.append(c)
    return out


CASES = _table()
ENDINGS = _endings()
ALL_K = _all_k()
SNAPSHOT_CASES = [0, 5, 13]   # indices into CASES
TALL_K = 8                    # sparse_cases.TALL with K = 8: 320 000 rows of margins (the wide residual kernels), a split row of A^T


def make_tall(K=TALL_K):
    """(A, B, lam) of sparse_cases.TALL with K right-hand sides: column k of B is b scaled and shifted by k (distinct responses)."""
    A, b, lam = S.make_sparse(*S.TALL)
    rng = np.random.default_rng(S.TALL[3] + 50)
    B = b[:, None] * (1.0 + 0.25 * np.arange(K)) + 0.01 * rng.standard_normal((b.size, K))
    return A, B, float(0.1 * np.max(np.abs(A.T @ B)))


# ---- the sweep matrices -----------------------------------------------------------------------------------------------------------
def rows_matrix(lengths, n, seed):
    """A CSR matrix whose row i holds lengths[i] elements at random distinct columns (sorted), standard normal values."""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(n, int(l), replace=False)) for l in lengths] + [np.zeros(0, np.int64)])
    return sp.csr_matrix((rng.standard_normal(idx.size), idx.astype(np.int32), indptr), shape=(len(lengths), n))


def edge_lengths(L):
    """Row lengths 0, 1, L - 1, L, L + 1, 2L, 2L + 1, 4L, 4L + 1, 4L + 3 - the four-way (K <= 4) and two-way bodies of a lane and
    their 1 .. 3 remainders - then rows of L + L / 2 until the mean row length lies in [L, 2L): the plan then picks L lanes."""
    head = [0, 1, L - 1, L, L + 1, 2 * L, 2 * L + 1, 4 * L, 4 * L + 1, 4 * L + 3]
    fill = L + L // 2
    out = list(head)
    while not (L <= sum(out) / len(out) < 2 * L) or len(out) < 40:
        out.append(fill)
    return out


def sweep_matrices():
    """[(name, csr)]: the hand-built matrices of the element-wise sweep test (the SMALL and TALL matrices are added by the test)."""
    out = []
    for L in LANES:
        A = rows_matrix(edge_lengths(L), 4 * L + 40, 7000 + L)
        out.append((f"edges-L{L}", A))
        out.append((f"edges-L{L}-T", sp.csr_matrix(A.T)))
    out.append(("empty", sp.csr_matrix((5, 7))))
    out.append(("one-row", rows_matrix([37], 50, 7101)))
    out.append(("one-column", sp.csr_matrix(rows_matrix([37], 50, 7102).T)))
    # a row of threshold + 3 elements (two segments, the last of 3), a row of exactly threshold elements (not split), a short row
    out.append(("threshold", rows_matrix([THRESHOLD + 3, THRESHOLD, 5], THRESHOLD + 40, 7103)))
    # 300 split rows (two segments each, the last of one element): more than the 256 threads of one tail workgroup
    out.append(("many-split", rows_matrix([THRESHOLD + 1] * 300, THRESHOLD + 1, 7104)))
    return out


def plan_claim(A, K):
    """What the oracle rests on, checked for one matrix: (plan of kron(A, I_K) == plan of A per response, row contents equal) for A
    and for A^T.  Returns the two lane widths and the split-row counts of A and A^T."""
    from zfista_amd import sparse

    A = sp.csr_matrix(A)
    A.sort_indices()
    out = []
    for mat in (A, sp.csr_matrix(A.T)):
        mat.sort_indices()
        big = kron(mat, K)
        p, q = sparse.plan_rows(mat.indptr.astype(np.int64)), sparse.plan_rows(big.indptr.astype(np.int64))
        assert p["lanes"] == q["lanes"] and p["threshold"] == q["threshold"] == THRESHOLD
        assert np.array_equal(np.repeat(np.diff(mat.indptr), K), np.diff(big.indptr)), "row i K + k is as long as row i"
        assert np.array_equal(q["split_row"], (p["split_row"][:, None] * K + np.arange(K)).reshape(-1))
        segs = np.diff(p["split_first"]) if p["split_row"].size else np.zeros(0, np.int64)
        assert np.array_equal(np.diff(q["split_first"]) if q["split_row"].size else np.zeros(0, np.int64), np.repeat(segs, K))
        # row contents: the same values in the same order at columns j K + k
        rows = np.repeat(np.arange(mat.shape[0]), np.diff(mat.indptr))
        for k in (0, K - 1):
            sub = big[k::K]
            assert np.array_equal(sub.indptr, mat.indptr) and np.array_equal(sub.data, mat.data)
            assert np.array_equal(sub.indices, mat.indices.astype(np.int64) * K + k)
        del rows
        out.append((p["lanes"], int(p["split_row"].size)))
    return out
