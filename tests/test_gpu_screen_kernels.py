"""GPU: the 14 kernels of csrc/zf_kernels_screen.h at every lane width and at their edges (tests/restrict_cases.py: the table, the
references and the bound of sum |a_j|^2; tests/test_restrict_cases.py proves on the CPU that the table reaches what it claims).

(a) Sparse restriction bit for bit against sparse.prepare(A[:, keep]) - six device arrays, both plans - for the ten lane-width
    matrices (every instantiation of rcount, fill_A, fill_At and norms_rows on both sides) under ten lane-aimed keep patterns; a
    pattern that keeps nothing is refused, one that keeps only empty columns gives a problem of nnz 0.
(b) The same for the two segment matrices, with the patterns at the segment borders and the split rows that must remain.
(c) zf_screen_scan on raw tensors at the chunk edges: n = 4096 | 4097 (one workgroup | chunks of 2048), 6143 | 6145 (a chunk
    border that is no multiple of 256), 2^21 | 2^21 + 1 (1024 chunks of 2048 | longer chunks), chunks that keep nothing.
(d) The wide matrix: n past the 1024-chunk cap of the mask count and the scan and past the 2048-workgroup cap of tlen.
(e) Dense: column norms element-wise and the gather bit for bit at m = 1 .. 3 (no unrolled group of four rows), m around the
    1024 rows of gridDim.y, n around 256 and 4096 and n past the grid cap.
(f) stats = [sum |a_j|^2, max |a_j|] of every problem above: the maximum is the largest device norm bit for bit, the sum within
    2 n u of the exact sum of the squares of the device's own norms.
Every bound is a-priori (restrict_cases, test_gpu_screening).  ZF_SCREEN_BOUNDS_RECORD=1 appends the worst ratios of (d), (e) and
(f) to profiles/screening_bounds.jsonl (any other value: that path)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import restrict_cases as R
import screen_cases as SC
from conftest import ROOT
from restrict_cases import _callbacks_agree, _same_as_prepare

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
T = R.T
LD = np.longdouble


def _record(**rec):
    where = os.environ.get("ZF_SCREEN_BOUNDS_RECORD", "")
    if where in ("", "0"):
        return
    path = os.path.join(ROOT, "profiles", "screening_bounds.jsonl") if where == "1" else where
    with open(path, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


def _ratio(err, bound):
    """The worst err / bound; an error where the bound is 0 is infinite."""
    err, bound = np.atleast_1d(np.asarray(err, dtype=float)), np.atleast_1d(np.asarray(bound, dtype=float))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0.0, 0.0, err / bound), initial=0.0))


def _stats_ratio(prob):
    """(f): the worst error / bound of stats[0]; stats[1] asserted here."""
    norms = prob.column_norms().cpu().numpy()
    stats = prob._norms.stats.cpu().numpy()
    assert stats.dtype == np.float64 and stats.shape == (2,) and norms.shape == (prob.n_features,)
    assert stats[1:].view(np.uint64)[0] == np.array([norms.max()]).view(np.uint64)[0], ("max |a_j|", stats[1], norms.max())
    total, bound = R.stats_ld(norms)
    ratio = _ratio(abs(LD(stats[0]) - total), bound)
    assert ratio <= 1.0, ("sum |a_j|^2", stats[0], float(total), ratio)
    return ratio


def _norms_ratio(prob, exact, lens):
    """Column norms against np.longdouble within 2 (len / 2 + 2) u norm; a column without elements has norm +0 exactly."""
    got = prob.column_norms().cpu().numpy()
    assert got.dtype == np.float64 and got.shape == exact.shape
    empty = np.asarray(exact == 0)
    assert (got[empty] == 0.0).all() and not np.signbit(got[empty]).any(), "an empty or zero column has norm +0 exactly"
    ratio = _ratio(np.abs(got.astype(LD) - exact).astype(float), 2.0 * (np.asarray(lens) / 2.0 + 2.0) * U * exact.astype(float))
    assert ratio <= 1.0, ratio
    return ratio


def _sparse_norms_and_stats(prob, A):
    exact, lens = SC.column_norms_ld(A)
    return _norms_ratio(prob, exact, lens), _stats_ratio(prob)


def _labels(m, seed):
    return np.where(np.random.default_rng(seed).random(m) < 0.5, -1.0, 1.0)


def _restrictions_held(name, logistic=False, split_counts=None):
    """(a), (b): every pattern of the case ``name``; returns the restricted problems by pattern."""
    import torch

    from zfista_amd.problems import SparseLeastSquaresL1, SparseLogisticL1

    c = R.case(name)
    m, n = c.A.shape
    scale = 1.0 if logistic else 0.5
    b = _labels(m, 5) if logistic else c.b
    prob = (SparseLogisticL1 if logistic else SparseLeastSquaresL1)(c.A, b, 0.1, scale=scale)
    assert R.plan_of(prob.plan) == c.plan, "the parent must run the instantiations the table claims"
    print(f"{name}: {m} x {n}, plan (lanes A, lanes A^T, split rows, split rows^T, segments, segments^T) = {R.plan_of(prob.plan)}")
    worst_norms, worst_stats = _sparse_norms_and_stats(prob, c.A)
    subs = {}
    for k, pattern in enumerate(c.pattern_names):
        mask, cols, want = R.restricted_case(name, pattern)
        keep = (torch.from_numpy(mask.copy()).cuda(), mask.copy(), cols.copy())[k % 3]   # a device mask, a host mask, column numbers
        if want is None:
            with pytest.raises(ValueError, match="no column is kept"):
                prob.restrict(keep)
            print(f"  {pattern}: keeps nothing, refused")
            continue
        sub = prob.restrict(keep)
        assert type(sub) is type(prob) and sub.b.data_ptr() == prob.b.data_ptr() and prob.n_features == n
        _same_as_prepare(sub, c.A, cols, want)
        print(f"  {pattern}: k {cols.size}, nnz {want['nnz']}, plan {R.plan_of(sub.plan)}")
        if split_counts is not None:
            assert (sub.plan[0]["split_row"].size, sub.plan[1]["split_row"].size) == split_counts(pattern, mask, cols), pattern
        _callbacks_agree(prob, sub, cols, k)
        if want["nnz"] == 0:
            x = np.random.default_rng(k).standard_normal(cols.size)
            if logistic:   # m terms log 2, each within 2 u, summed in any order: (m / 2 + 4) u with the project's factor 2
                exact, tol = LD(scale) * m * np.log(LD(2)), 2.0 * (m / 2.0 + 4.0) * U
            else:
                exact, tol = LD(scale) * np.sum(b.astype(LD) ** 2), 1e-15
            assert abs(LD(sub.f(x)) - exact) <= tol * exact, (sub.f(x), float(exact))
            grad = sub.jac_f(x)
            assert grad.shape == (cols.size,) and (grad == 0.0).all() and not np.signbit(grad).any(), "jac_f must be +0.0"
        rn, rs = _sparse_norms_and_stats(sub, c.A[:, cols])
        worst_norms, worst_stats = max(worst_norms, rn), max(worst_stats, rs)
        subs[pattern] = sub
    print(f"{name}: worst norms error / bound {worst_norms:.3g}, worst stats error / bound {worst_stats:.3g}")
    _record(test="screen-kernels-stats", case=name + ("-logistic" if logistic else ""), norms_ratio=worst_norms, stats_ratio=worst_stats)
    return prob, subs


# ---- (a) every lane width ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.LANE_CASES)
def test_sparse_restriction_at_every_lane_width(name):
    prob, subs = _restrictions_held(name)
    assert subs["empty-columns"].nnz == 0 and subs["empty-columns"].n_features >= 2
    if not name.endswith("-T"):
        assert subs["empty-columns"].n_features == 3


@pytest.mark.parametrize("name", ["lanes-8", "lanes-8-T"])
def test_sparse_restriction_logistic(name):
    _restrictions_held(name, logistic=True)


def test_a_restricted_problem_restricts_again():
    """The parent arrays of the second restriction were written by the fill kernels."""
    from zfista_amd.problems import SparseLeastSquaresL1

    c = R.case("lanes-8")
    prob = SparseLeastSquaresL1(c.A, c.b, 0.1)
    assert R.plan_of(prob.plan) == c.plan
    mask, cols, want = R.restricted_case("lanes-8", "alternating")
    sub = prob.restrict(mask.copy())
    _same_as_prepare(sub, c.A, cols, want)
    again_mask = np.arange(cols.size) % 2 == 0
    again = sub.restrict(again_mask)
    print("plans:", R.plan_of(prob.plan), R.plan_of(sub.plan), R.plan_of(again.plan))
    assert np.array_equal(cols[again_mask], np.arange(0, c.A.shape[1], 4))
    _same_as_prepare(again, c.A, cols[again_mask])
    _callbacks_agree(sub, again, np.flatnonzero(again_mask), 3)
    _sparse_norms_and_stats(again, c.A[:, cols[again_mask]])


# ---- (b) segments --------------------------------------------------------------------------------------------------------------------
# the split rows that remain, by hand from the lengths T, T + 1, 2T, 2T + 1, 2T + 63 ("alternating" un-splits T + 1 and 2T, "not-first-
# segment" leaves T + 1 and T + 63 of 2T + 1 and 2T + 63, "not-first-round" leaves 2T - 64, 2T - 63 and 2T - 1)
SEGMENT_SPLITS = {"all": 4, "not-first-segment": 2, "alternating": 2, "segment-borders": 0, "empty-columns": 0, "first-round": 0,
                  "not-first-round": 3}


def test_segment_rows_restrict_bit_for_bit():
    c = R.case("segments")

    def splits(pattern, mask, cols):
        kept = np.array([int(mask[:k].sum()) for k in c.lens])
        if pattern in SEGMENT_SPLITS:
            assert int((kept > T).sum()) == SEGMENT_SPLITS[pattern], pattern
        return int((kept > T).sum()), 0

    prob, subs = _restrictions_held("segments", split_counts=splits)
    assert set(subs) == set(R.PATTERNS) | set(R.SEGMENT_PATTERNS)
    lens = np.diff(subs["not-first-segment"]._spmat.dev["indptr"].cpu().numpy())
    assert sorted(lens[[1, 2, 3, 8]]) == [1, T, T + 1, T + 63], "rows of T + 1 and T + 63 stay split behind an empty first segment"


def test_segment_columns_restrict_bit_for_bit():
    base = R.case("segments")
    prob, subs = _restrictions_held("segments-T", split_counts=lambda pattern, mask, cols: (0, int((base.lens[cols] > T).sum())))
    assert subs["all"].plan[1]["split_row"].size == 4 and subs["all"].plan[1]["seg_start"].size == 10
    assert subs["alternating"].plan[1]["split_row"].size == 2   # (columns 0, 2, 4, 6, 8: the rows of T, 2T, 0, 64, 2T + 63)


# ---- (c) the scan alone ----------------------------------------------------------------------------------------------------------------
SCAN_N = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 6143, 6145, 2 ** 21, 2 ** 21 + 1, 3 * 2 ** 20 + 5)


def _scan_masks(n):
    rng = np.random.default_rng(n)
    one = lambda at: np.bincount([at], minlength=n).astype(np.uint8)
    return {
        "ones": np.ones(n, dtype=np.uint8),
        "zeros": np.zeros(n, dtype=np.uint8),
        "first": one(0),
        "last": one(n - 1),
        "alternating": (np.arange(n) % 2 == 0).astype(np.uint8),
        "bernoulli-0.5": (rng.random(n) < 0.5).astype(np.uint8),
        "bernoulli-0.01": (rng.random(n) < 0.01).astype(np.uint8),
        "last-quarter": (np.arange(n) >= n - (n + 3) // 4).astype(np.uint8),
        "any-non-zero-byte": rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), n),
    }


@pytest.mark.parametrize("n", SCAN_N)
def test_the_scan_at_the_chunk_edges(n):
    import torch

    from zfista_amd import _lib

    lib = _lib.require_gpu()
    pad = 64   # elements behind the n the scan may write: they must stay what they were
    for name, mask in _scan_masks(n).items():
        want, count = R.scan_ref(mask)
        if name == "zeros":
            assert count == 0 and not want.any()
        keep = torch.from_numpy(mask).cuda()
        index = torch.full((n + pad,), -7, dtype=torch.int32, device="cuda")
        k = C.c_int64(-1)
        rc = lib.zf_screen_scan(C.c_void_p(keep.data_ptr()), n, C.c_void_p(index.data_ptr()), C.byref(k))
        assert rc == 0, (name, rc)
        got = index.cpu().numpy()
        assert k.value == count, (name, k.value, count)
        assert got.dtype == np.int32 and np.array_equal(got[:n], want), (name, np.flatnonzero(got[:n] != want)[:8])
        assert (got[n:] == -7).all(), name
        assert np.array_equal(keep.cpu().numpy(), mask), "the mask is read, not written"


# ---- (d) the wide matrix -----------------------------------------------------------------------------------------------------------------
def test_wide_matrix_past_the_chunk_and_grid_caps():
    import torch

    from zfista_amd.problems import SparseLeastSquaresL1

    c = R.case("wide")
    n = c.A.shape[1]
    assert n > 1024 * 2048 and n > 2048 * 256
    prob = SparseLeastSquaresL1(c.A, c.b, 0.1)
    assert R.plan_of(prob.plan) == c.plan
    exact, lens = SC.column_norms_ld(c.A)
    norms_ratio, stats_ratio = _norms_ratio(prob, exact, lens), _stats_ratio(prob)
    mask, cols, want = R.restricted_case("wide", "bernoulli-0.5")
    sub = prob.restrict(torch.from_numpy(mask.copy()).cuda())
    _same_as_prepare(sub, c.A, cols, want)
    assert sub.plan[0]["split_row"].size == 1 and sub.n_features > 1024 * 1024 - 4096
    _callbacks_agree(prob, sub, cols, 4)
    sub_stats = _stats_ratio(sub)
    print(f"wide: plan {R.plan_of(prob.plan)} -> {R.plan_of(sub.plan)}, k {cols.size}, nnz {want['nnz']}; norms error / bound "
          f"{norms_ratio:.3g}, stats {stats_ratio:.3g} and {sub_stats:.3g}")
    _record(test="screen-kernels-wide", n=n, norms_ratio=norms_ratio, stats_ratio=max(stats_ratio, sub_stats))


# ---- (e) dense ---------------------------------------------------------------------------------------------------------------------------
DENSE_SHAPES = ((1, 1), (3, 5), (4, 256), (5, 257), (1023, 70), (1024, 70), (1025, 300), (2049, 257), (7, 4097), (2, 2 ** 21 + 3))


@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dense_norms_and_gather(shape):
    from zfista_amd.problems import LeastSquaresL1

    m, n = shape
    rng = np.random.default_rng(1000 * m + n)
    A = rng.standard_normal(shape)
    zero = n // 2
    A[:, zero] = 0.0
    prob = LeastSquaresL1(A, rng.standard_normal(m), 0.1)
    exact, _ = SC.column_norms_ld(sp.csr_matrix(A))
    norms_ratio = _norms_ratio(prob, exact, np.full(n, m))
    assert prob.column_norms().cpu().numpy()[zero] == 0.0
    stats_ratio = _stats_ratio(prob)
    if n > 2 ** 21:
        keeps = (np.arange(0, n, 2), np.flatnonzero(rng.random(n) < 0.5))
    else:
        keeps = (np.arange(n), np.array([n - 1]), np.arange(0, n, 2), np.sort(rng.choice(n, 7, replace=False)) if n >= 7 else np.arange(n))
    for k, cols in enumerate(keeps):
        mask = np.zeros(n, dtype=bool)
        mask[cols] = True
        sub = prob.restrict(mask if k % 2 else cols)
        assert type(sub) is LeastSquaresL1 and sub.n_features == cols.size and sub.A.shape == (m, cols.size) and sub.A.is_contiguous()
        got, want = sub.A.cpu().numpy(), np.ascontiguousarray(A[:, cols])
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (shape, k)
        assert prob.A.shape == (m, n) and sub.b.data_ptr() == prob.b.data_ptr()
        stats_ratio = max(stats_ratio, _stats_ratio(sub))
    print(f"dense {m} x {n}: norms error / bound {norms_ratio:.3g}, stats {stats_ratio:.3g}")
    _record(test="screen-kernels-dense", m=m, n=n, norms_ratio=norms_ratio, stats_ratio=stats_ratio)
