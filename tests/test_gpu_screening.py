"""GPU: gap-safe screening and device-side column restriction (csrc/zf_kernels_screen.h, zfista_amd/screening.py).

(1) Column norms element-wise against np.longdouble: |norm^ - norm| <= 2 (len / 2 + 2) u norm (a sum of len squares in any order
and a square root, with the project's factor 2); an empty column has norm 0 exactly.
(2) The mask, two-sided, against the exact rule of tests/screen_cases.py at three points of a FISTA trajectory (x = 0, 20 and
400 iterations), both losses, both storage forms, n = 257, 1000 and 4099 (beyond the one-workgroup size 4096):
    safety     every column the device discards is discarded by the exact rule (exact g, exact gap);
    tightness  every column the exact rule discards with a slack above 2 E |a_j| + lam 2^-40 is discarded by the device
with the precondition of E's derivation, d_gap / gap <= 2^-20, asserted from gap_cases' own bound.  The l1 weights were chosen on
the CPU oracle's trajectory so that this holds with a margin of 4 or more at every point (0.2 lam_max on the two SMALL cases;
0.1 lam_max on a 100 x 257 matrix - the overdetermined SMALL case of n = 257 converges so fast that after 400 iterations its gap
is of the size of its own rounding bound).  The scan is np.cumsum's, the count the mask's sum, the eight gap outputs the bits of
duality_gap(x).
(3) Restriction bit for bit against sparse.prepare(A[:, keep]) - six device arrays, both plans - and the dense gather.
(4) solve_screened against the unscreened gap_tol solve.  (5) The path, determinism, sharing, refusals, the C entry points.
ZF_SCREEN_BOUNDS_RECORD=1 appends the worst ratios of (1) and (2) to profiles/screening_bounds.jsonl (any other value: that path)."""
import ctypes as C
import functools
import json
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import gap_cases as G
import logistic_cases as L
import screen_cases as SC
import sparse_cases as S
from conftest import ROOT
from restrict_cases import _callbacks_agree, _same_as_prepare

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
KW = dict(lr=1.0, nesterov=True, tol=0.0)


def _cls(logistic, storage):
    from zfista_amd import problems as Z

    return {(False, "dense"): Z.LeastSquaresL1, (False, "csr"): Z.SparseLeastSquaresL1,
            (True, "dense"): Z.LogisticL1, (True, "csr"): Z.SparseLogisticL1}[(bool(logistic), storage)]


def _make(A, b, lam, logistic, storage):
    return _cls(logistic, storage)(A if storage == "csr" else A.toarray(), b, lam, scale=1.0 if logistic else 0.5)


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _record(**rec):
    where = os.environ.get("ZF_SCREEN_BOUNDS_RECORD", "")
    if where in ("", "0"):
        return
    path = os.path.join(ROOT, "profiles", "screening_bounds.jsonl") if where == "1" else where
    with open(path, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


@functools.lru_cache(maxsize=None)
def _data(shape, logistic):
    """(A, b, scale, lam_max) - read-only - of a sparse_cases / logistic_cases matrix."""
    if logistic:
        A, b, _ = L.make_logistic(*shape)
        scale = 1.0
    else:
        A, b, _ = S.make_sparse(*shape)
        scale = 0.5
    return A, b, scale, SC.lam_max(A, b, scale, logistic)


# ---- (1) column norms ----------------------------------------------------------------------------------------------------------
def _norms_held(name, prob, A):
    exact, lens = SC.column_norms_ld(A)
    got = prob.column_norms().cpu().numpy()
    assert got.shape == (A.shape[1],)
    assert (got[lens == 0] == 0.0).all(), "an empty column has norm 0 exactly"
    bound = 2.0 * (lens / 2.0 + 2.0) * U * exact.astype(float)
    err = np.abs(got.astype(np.longdouble) - exact).astype(float)
    ratio = float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-300))))
    print(f"norms {name}: worst error / bound {ratio:.3g}; longest column {int(lens.max())}")
    _record(test="norms", case=name, ratio=ratio, longest=int(lens.max()))
    assert ratio <= 1.0
    assert prob.column_norms().data_ptr() == prob.with_lam(2.0 * prob.lam).column_norms().data_ptr()


@pytest.mark.parametrize("case", range(4))
def test_column_norms_sparse_small(case):
    A, b, scale, _ = _data(S.SMALL[case], False)
    assert (np.diff(A.tocsc().indptr) == 0).any() and np.diff(A.tocsc().indptr).max() == A.shape[0] - 1
    _norms_held(f"small-{case}", _make(A, b, 1.0, False, "csr"), A)


def test_column_norms_tall_takes_the_segment_path():
    A, b, scale, _ = _data(S.TALL, False)
    prob = _make(A, b, 1.0, False, "csr")
    assert np.diff(A.tocsc().indptr).max() == 39999 and prob.plan[1]["split_row"].size == 1 and prob.plan[1]["seg_start"].size == 10
    _norms_held("tall", prob, A)


@pytest.mark.parametrize("shape", [(40, 64), (37, 65)])
def test_column_norms_dense(shape):
    rng = np.random.default_rng(shape[1])
    A = rng.standard_normal(shape)
    A[:, 3] = 0.0
    b = rng.standard_normal(shape[0])
    from zfista_amd.problems import LeastSquaresL1

    exact, _ = SC.column_norms_ld(sp.csr_matrix(A))
    prob = LeastSquaresL1(A, b, 1.0)
    got = prob.column_norms().cpu().numpy()
    bound = 2.0 * (shape[0] / 2.0 + 2.0) * U * exact.astype(float)
    err = np.abs(got.astype(np.longdouble) - exact).astype(float)
    assert got[3] == 0.0 and (err <= bound).all()
    _record(test="norms", case=f"dense-{shape[0]}x{shape[1]}", ratio=float(np.max(err[bound > 0] / bound[bound > 0])))


# ---- (2) the mask ----------------------------------------------------------------------------------------------------------------
MASK_SHAPES = {257: ((100, 257, 0.1, 11), 0.1), 1000: (S.SMALL[0], 0.2), 4099: (S.SMALL[3], 0.2)}


@pytest.mark.parametrize("storage", ["csr", "dense"])
@pytest.mark.parametrize("logistic", [False, True], ids=["ls", "logistic"])
@pytest.mark.parametrize("n", [257, 1000, 4099])
def test_the_mask_is_safe_and_tight(n, logistic, storage):
    from zfista_amd import minimize_proximal_gradient as solve

    shape, frac = MASK_SHAPES[n]
    A, b, scale, lmax = _data(shape, logistic)
    assert A.shape[1] == n
    lam = frac * lmax
    prob = _make(A, b, lam, logistic, storage)
    discarded = []
    for its in (0, 20, 400):
        x = np.zeros(n) if its == 0 else _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=its, **KW).x
        ref = SC.screen_longdouble(A, b, x, lam, scale, logistic, dense=storage == "dense")
        gap, d_gap = float(ref["vals"]["gap"]), ref["bounds"]["gap"]
        print(f"n={n} {storage} its={its}: gap {gap:.4g}, d_gap / gap = {d_gap / gap * 2.0 ** 20:.3g} x 2^-20")
        assert gap > 0 and d_gap / gap <= 2.0 ** -20, "the precondition of E (from gap_cases' own bound)"
        sc = prob.screen(x)
        gp, keep_dev, count = sc
        keep = keep_dev.cpu().numpy()
        assert keep.dtype == np.bool_ and keep.shape == (n,)
        out = ~keep
        # safety
        wrong = out & ~ref["discard"]
        assert not wrong.any(), ("the device discards a column the exact rule keeps", np.flatnonzero(wrong))
        # tightness
        norms = ref["norms"]
        slack = np.longdouble(lam) - ref["left"]
        must = slack > np.longdouble(2.0 * ref["E"]) * norms + np.longdouble(lam * 2.0 ** -40)
        missed = must & keep
        assert not missed.any(), ("the device keeps a column the exact rule discards with slack", np.flatnonzero(missed))
        # the worst slack among the kept columns the exact rule discards, in units of what the device may lose
        amb = keep & ref["discard"]
        ratio = float(np.max((slack[amb] / (np.longdouble(2.0 * ref["E"]) * norms[amb] + np.longdouble(lam * 2.0 ** -40))).astype(float), initial=0.0))
        # the radius and the guard the device used against the restatement
        assert abs(float(sc.radius) - float(ref["radius"])) <= 2.0 ** -20 * float(ref["radius"])
        assert 0.5 * ref["E"] <= float(sc.guard) <= 2.0 * ref["E"]
        # scan and count
        index = sc.index.cpu().numpy()
        assert index.dtype == np.int32 and np.array_equal(index, np.cumsum(keep) - keep) and count == int(keep.sum())
        # the eight gap outputs
        alone = prob.duality_gap(x)
        assert np.array_equal(np.array([getattr(gp, k) for k in G.KEYS]).view(np.uint64), np.array([getattr(alone, k) for k in G.KEYS]).view(np.uint64))
        _record(test="mask", n=n, logistic=bool(logistic), storage=storage, its=its, gap=gap, precondition=d_gap / gap * 2.0 ** 20,
                discarded=int(out.sum()), exact_discarded=int(ref["discard"].sum()), tightness_ratio=ratio, E=float(sc.guard), E_ref=ref["E"])
        discarded.append(int(out.sum()))
    print(f"n={n} {storage} {'logistic' if logistic else 'ls'}: discarded {discarded}")
    assert discarded[-1] > discarded[0] and discarded[-1] > n // 2, "the rule must bite along the trajectory"


def test_a_non_finite_point_keeps_everything():
    A, b, scale, lmax = _data(S.SMALL[0], False)
    prob = _make(A, b, 0.5 * lmax, False, "csr")
    x = np.zeros(A.shape[1])
    assert prob.screen(x).count < A.shape[1]
    x[5] = np.nan
    gp, keep, count = prob.screen(x)
    assert np.isnan(gp.gap) and count == A.shape[1] and bool(keep.all())
    assert prob.with_lam(0.0).screen(np.zeros(A.shape[1])).count == A.shape[1]


# ---- (3) restriction ---------------------------------------------------------------------------------------------------------------
def _keep_sets_small0(m, n):
    rng = np.random.default_rng(12)
    dense_col = n // 5
    return {
        "all": np.arange(n),
        "one": np.array([7]),
        "alternating": np.arange(0, n, 2),
        "tenth": np.sort(rng.choice(n, n // 10, replace=False)),
        "dense-column-only": np.array([dense_col]),
        "all-but-dense-column": np.delete(np.arange(n), dense_col),
        "empties-rows": np.array([3, n // 2, n - 2]),   # (n // 2 is the empty column: most rows lose everything)
    }


@pytest.mark.parametrize("logistic", [False, True], ids=["ls", "logistic"])
def test_restriction_is_prepare_of_the_kept_columns_bit_for_bit(logistic):
    import torch

    A, b, scale, lmax = _data(S.SMALL[0], logistic)
    m, n = A.shape
    prob = _make(A, b, 0.2 * lmax, logistic, "csr")
    for k, (name, cols) in enumerate(_keep_sets_small0(m, n).items()):
        mask = np.zeros(n, dtype=bool)
        mask[cols] = True
        keep = (torch.from_numpy(mask).cuda(), mask, cols)[k % 3]   # a device mask, a host mask, column numbers
        sub = prob.restrict(keep)
        assert type(sub) is type(prob) and sub.b.data_ptr() == prob.b.data_ptr() and sub.lam == prob.lam and prob.n_features == n
        want = _same_as_prepare(sub, A, cols)
        if name == "empties-rows":
            assert (np.diff(want["indptr"]) == 0).sum() > m // 2
        _callbacks_agree(prob, sub, cols, k)
    with pytest.raises(ValueError, match="no column is kept"):
        prob.restrict(np.zeros(n, dtype=bool))
    for bad in (np.zeros(n - 1, dtype=bool), np.array([0, 0]), np.array([n]), np.array([0.5])):
        with pytest.raises(ValueError):
            prob.restrict(bad)


def test_restriction_of_a_split_row_and_of_a_split_column():
    A, b, scale, lmax = _data(S.SMALL[1], False)
    m, n = A.shape
    prob = _make(A, b, 0.2 * lmax, False, "csr")
    assert prob.plan[0]["split_row"].size == 1 and n == 5000, "the dense row of 5000 elements is split"
    stays = np.flatnonzero(np.arange(n) % 10 != 0)     # 4500 > 4096: still split
    sub = prob.restrict(stays)
    assert sub.plan[0]["split_row"].size == 1 and sub.plan[0]["seg_start"].size == 2
    _same_as_prepare(sub, A, stays)
    _callbacks_agree(prob, sub, stays, 1)
    leaves = np.arange(1, n, 2)                        # 2500: one ordinary row
    sub = prob.restrict(leaves)
    assert sub.plan[0]["split_row"].size == 0
    _same_as_prepare(sub, A, leaves)
    again = sub.restrict(np.arange(0, leaves.size, 3))   # a restricted problem restricts like any other
    _same_as_prepare(again, A, leaves[::3])
    A, b, scale, lmax = _data(S.TALL, False)
    m, n = A.shape
    prob = _make(A, b, 0.2 * lmax, False, "csr")
    cols = np.union1d(np.random.default_rng(3).choice(n, n // 10, replace=False), [n // 5])
    sub = prob.restrict(cols)
    assert sub.plan[1]["split_row"].size == 1 and sub.plan[1]["seg_start"].size == 10, "the column of 39 999 elements is kept"
    _same_as_prepare(sub, A, cols)
    _callbacks_agree(prob, sub, cols, 2)
    assert np.allclose(sub.column_norms().cpu().numpy(), prob.column_norms().cpu().numpy()[cols], rtol=1e-13, atol=0), "whole rows of A^T"


@pytest.mark.parametrize("shape", [(40, 64), (37, 65)])
def test_dense_restriction_is_the_column_gather(shape):
    from zfista_amd.problems import LeastSquaresL1, LogisticL1

    rng = np.random.default_rng(shape[0])
    A = rng.standard_normal(shape)
    m, n = shape
    for cls, b in ((LeastSquaresL1, rng.standard_normal(m)), (LogisticL1, np.where(rng.random(m) < 0.5, -1.0, 1.0))):
        prob = cls(A, b, 0.1)
        for k, cols in enumerate((np.arange(n), np.array([n - 1]), np.arange(0, n, 2), np.sort(rng.choice(n, 7, replace=False)))):
            mask = np.zeros(n, dtype=bool)
            mask[cols] = True
            sub = prob.restrict(mask if k % 2 else cols)
            assert type(sub) is cls and sub.n_features == cols.size and sub.A.shape == (m, cols.size) and sub.A.is_contiguous()
            assert np.array_equal(sub.A.cpu().numpy().view(np.uint64), np.ascontiguousarray(A[:, cols]).view(np.uint64))
            assert sub.b.data_ptr() == prob.b.data_ptr() and prob.A.shape == (m, n)
            _callbacks_agree(prob, sub, cols, k)


# ---- (4) solves ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_solution(shape, logistic, frac):
    A, b, scale, lmax = _data(shape, logistic)
    return SC.fista(A, b, frac * lmax, scale, logistic, np.zeros(A.shape[1]), 20000)[0]


@pytest.fixture
def masks(monkeypatch):
    """The mask of every screen call."""
    from zfista_amd import problems as Z

    seen = []
    orig = Z._GapMixin.screen

    def spy(self, x):
        sc = orig(self, x)
        seen.append(sc.keep.cpu().numpy())
        return sc

    monkeypatch.setattr(Z._GapMixin, "screen", spy)
    return seen


@pytest.mark.parametrize("logistic", [False, True], ids=["ls", "logistic"])
@pytest.mark.parametrize("case", [0, 3])
def test_screened_and_unscreened_solves_agree(case, logistic, masks):
    from zfista_amd import minimize_proximal_gradient as solve
    from zfista_amd.screening import solve_screened

    A, b, scale, lmax = _data(S.SMALL[case], logistic)
    n = A.shape[1]
    prob = _make(A, b, 1.0, logistic, "csr").with_lam(0.2 * _make(A, b, 1.0, logistic, "csr").lam_max())
    lam = prob.lam
    assert abs(lam - 0.2 * lmax) <= 1e-12 * lmax
    gap_tol = 1e-6 * float(prob.duality_gap(np.zeros(n)).primal)
    plain = _quiet(solve, *prob.callbacks(), np.zeros(n), gap_tol=gap_tol, **KW)
    res = _quiet(solve_screened, prob, np.zeros(n), gap_tol, **KW)
    assert plain.success and res.success and res.message == "Duality gap reached gap_tol" and res.x.shape == (n,)
    for r in (plain, res):
        vals, bounds, _ = G.gap_longdouble(A, b, r.x, lam, scale, logistic)
        assert float(vals["gap"]) <= gap_tol + bounds["gap"]
    assert abs(res.fun - plain.fun) <= gap_tol
    assert res.dual_gap == prob.duality_gap(res.x).gap <= gap_tol
    assert res.fun == prob.duality_gap(res.x).primal
    x_long = _long_solution(S.SMALL[case], logistic, 0.2)
    dropped = np.zeros(n, dtype=bool)
    for mask in masks:
        dropped |= ~mask
    assert dropped.any() and not x_long[dropped].any(), "a column dropped in any round is zero in the long CPU solution"
    rounds = res.screen
    print(f"case {case} {'logistic' if logistic else 'ls'}: screened nit {res.nit} (plain {plain.nit}), rounds {rounds}")
    assert len(masks) == len(rounds) + 1 and [r["kept"] for r in rounds] == [int(mk.sum()) for mk in masks[:-1]]
    assert any(r["restricted"] and r["kept"] < n // 2 for r in rounds)
    assert res.nit == sum(r["nit"] for r in rounds) and res.dual_gap_checks >= len(masks)
    assert np.count_nonzero(res.x) <= min(r["kept"] for r in rounds)


# ---- (5) the path and the interface ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,logistic", [("csr", False), ("dense", True)])
def test_l1_path_screened_against_unscreened(storage, logistic):
    from zfista_amd.path import l1_path

    A, b, scale, lmax = _data(S.SMALL[0], logistic)
    n = A.shape[1]
    prob = _make(A, b, 1.0, logistic, storage)
    lams = float(prob.lam_max()) * np.array([1.0 + 1e-9, 0.6, 0.35, 0.2])
    gap_tol = 1e-6 * float(prob.duality_gap(np.zeros(n)).primal)
    plain = _quiet(l1_path, prob, lams, gap_tol=gap_tol, **KW)
    scr = _quiet(l1_path, prob, lams, None, gap_tol, True, **KW)
    assert [r.lam for r in scr] == [float(v) for v in lams]
    assert not scr[0].x.any() and scr[0].dual_gap == 0.0 and scr[0].nit == 0
    for lam, p, s in zip(lams, plain, scr):
        assert p.success and s.success and s.dual_gap <= gap_tol and abs(s.fun - p.fun) <= gap_tol
        vals, bounds, _ = G.gap_longdouble(A, b, s.x, lam, scale, logistic)
        assert float(vals["gap"]) <= gap_tol + bounds["gap"]
    assert any(r["restricted"] for s in scr[1:] for r in s.screen)
    with pytest.raises(ValueError):
        l1_path(prob, lams, gap_tol=None, screen=True)


def test_interface():
    import torch

    from zfista_amd import _lib, minimize_proximal_gradient as solve
    from zfista_amd.path import l1_path
    from zfista_amd.problems import DiagQuadL1, LeastSquaresL1
    from zfista_amd.proximal_gradient import NativeRun
    from zfista_amd.screening import solve_screened

    A, b, scale, lmax = _data(S.SMALL[0], False)
    n = A.shape[1]
    prob = _make(A, b, 0.2 * lmax, False, "csr")
    base = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=100000, max_backtrack_iter=100, nesterov=True,
                nesterov_ratio=(0, 0.25), deprecated=False, return_all=False, verbose=False)

    def counts():
        run = NativeRun(prob, np.zeros(n), dict(base))
        run.advance(24)
        out = run.solver.launch_counts(), run.solver.get_x()
        run.solver.close()
        return out

    before = counts()
    gap_tol = 1e-6 * float(prob.duality_gap(np.zeros(n)).primal)
    # lam >= lam_max from a non-zero warm start: x = 0
    warm = _quiet(solve, *prob.callbacks(), np.zeros(n), max_iter=50, **KW).x
    assert warm.any()
    res = _quiet(solve_screened, prob.with_lam(1.5 * lmax), warm, gap_tol, **KW)
    assert res.success and not res.x.any() and res.dual_gap == 0.0
    # two screened solves: the same bits
    one = _quiet(solve_screened, prob, np.zeros(n), gap_tol, **KW)
    two = _quiet(solve_screened, prob, np.zeros(n), gap_tol, **KW)
    assert np.array_equal(one.x, two.x) and one.nit == two.nit and one.dual_gap == two.dual_gap and one.screen == two.screen
    # siblings share one norms vector; a restricted problem has its own
    sib = prob.with_lam(0.3)
    assert sib.column_norms().data_ptr() == prob.column_norms().data_ptr()
    assert prob.restrict(np.arange(10)).column_norms().data_ptr() != prob.column_norms().data_ptr()
    # a solve without the keyword launches what it launched, and computes what it computed
    after = counts()
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    print("launch counts of 24 passes:", before[0])
    # refusals
    boxed = _cls(False, "csr")(A, b, 0.2 * lmax, bounds=(-1.0, 1.0))
    grouped = LeastSquaresL1(A.toarray(), b, 0.2 * lmax, group=object())
    for bad in (boxed, grouped):
        for call in (lambda: solve_screened(bad, np.zeros(n), gap_tol), lambda: bad.screen(np.zeros(n)), lambda: bad.restrict(np.arange(3)),
                     lambda: l1_path(bad, [0.1], screen=True)):
            with pytest.raises(ValueError, match="not available"):
                call()
    diag = DiagQuadL1(np.ones(100), np.ones(100), 0.1)
    with pytest.raises(ValueError):
        solve_screened(diag, np.zeros(100), 1e-6)
    with pytest.raises(ValueError):
        l1_path(diag, [0.1], screen=True)
    with pytest.raises(ValueError, match="return_all"):
        solve_screened(prob, np.zeros(n), gap_tol, return_all=True)
    with pytest.raises(ValueError):
        solve_screened(prob, np.zeros(n - 1), gap_tol)
    with pytest.raises(ValueError):
        prob.screen(np.zeros(n - 1))
    # the C entry points: NULL and size errors are ZF_ERR_ARG (-2)
    lib = _lib.require_gpu()
    P = C.c_void_p
    h = prob._spmat.value
    norms, stats = prob.column_norms(), prob._norms.stats
    keep = torch.ones(n, dtype=torch.uint8, device="cuda")
    index = torch.empty(n, dtype=torch.int32, device="cuda")
    lens = torch.empty(n + prob.m_rows, dtype=torch.int64, device="cuda")
    x, out, k = np.zeros(n), np.zeros(12), C.c_int64(0)
    dp = lambda t: P(t.data_ptr())
    dense = LeastSquaresL1(A.toarray(), b, 0.2 * lmax)
    assert lib.zf_spmat_col_norms(None, dp(norms), dp(stats)) == -2 and lib.zf_spmat_col_norms(h, None, dp(stats)) == -2
    assert lib.zf_dense_col_norms(None, 3, 3, dp(norms), dp(stats)) == -2 and lib.zf_dense_col_norms(dp(dense.A), 0, n, dp(norms), dp(stats)) == -2
    import evaldesc as E

    fields = dict(spmat=h, b=dp(prob.b), scale=0.5, lam=0.1)   # (the squared loss, K = 1)
    args = [P(_lib.ptr(x)), P(_lib.ptr(out)), 12, dp(norms), dp(stats), 10, 10, dp(keep), dp(index)]
    assert E.screen(E.desc(**fields), *args) == 0
    for pos, bad in ((2, 11), (3, None), (4, None), (5, -1), (7, None), (8, None)):   # count, norms, stats, max_row, keep, index
        assert E.screen(E.desc(**fields), *(args[:pos] + [bad] + args[pos + 1:])) == -2, pos
    for name, bad in (("spmat", None), ("scale", 0.0)):
        assert E.screen(E.desc(**{**fields, name: bad}), *args) == -2, name
    fields = dict(A=dp(dense.A), b=dp(dense.b), m_rows=prob.m_rows, n=n, scale=0.5, lam=0.1)
    dargs = [P(_lib.ptr(x)), P(_lib.ptr(out)), 12, dp(norms), dp(stats), 0, 0, dp(keep), dp(index)]   # (max_row / max_col: a handle's)
    assert E.screen(E.desc(**fields), *dargs) == 0
    for pos, bad in ((2, 8), (3, None), (7, None), (8, None)):   # count, norms, keep, index
        assert E.screen(E.desc(**fields), *(dargs[:pos] + [bad] + dargs[pos + 1:])) == -2, pos
    for name, bad in (("A", None), ("n", 0)):
        assert E.screen(E.desc(**{**fields, name: bad}), *dargs) == -2, name
    assert lib.zf_screen_scan(None, n, dp(index), C.byref(k)) == -2 and lib.zf_screen_scan(dp(keep), 0, dp(index), C.byref(k)) == -2
    keep.fill_(1)   # (the screen calls above wrote their mask here)
    torch.cuda.synchronize()
    assert lib.zf_screen_scan(dp(keep), n, dp(index), C.byref(k)) == 0 and k.value == n
    assert lib.zf_spmat_restrict_count(h, None, dp(index), dp(lens), dp(lens), None, C.byref(k)) == -2
    assert lib.zf_spmat_restrict_count(None, dp(keep), dp(index), dp(lens), dp(lens), None, C.byref(k)) == -2
    assert lib.zf_spmat_restrict_fill(h, dp(keep), dp(index), None, 0, 0, dp(lens), None, None, dp(lens), None, None) == -2
    assert lib.zf_spmat_restrict_fill(h, dp(keep), dp(index), None, n, prob.nnz + 1, dp(lens), None, None, dp(lens), None, None) == -2
    assert lib.zf_dense_restrict(None, 3, 3, dp(keep), dp(index), 3, dp(norms)) == -2
    assert lib.zf_dense_restrict(dp(dense.A), prob.m_rows, n, dp(keep), dp(index), n - 1, dp(norms)) == -2, "k must be the kept count"
