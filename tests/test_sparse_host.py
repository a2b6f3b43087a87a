"""CPU: the host part of sparse least squares (zfista_amd/sparse.py) - canonical CSR arrays of A and A^T, the row plan
the SpMV kernels index with, the ValueErrors of SparseLeastSquaresL1 - and the additive C ABI around it.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import evaldesc as E
from conftest import ROOT
from zfista_amd import _lib, sparse


def _canon(A):
    A = sp.csr_matrix(A, dtype=np.float64, copy=True)
    A.sum_duplicates()
    A.sort_indices()
    return A


def _variants():
    rng = np.random.default_rng(5)
    m, n, k = 37, 53, 400
    rows, cols = rng.integers(0, m, k), rng.integers(0, n, k)     # duplicates among 400 draws on 1961 cells
    vals = np.round(rng.standard_normal(k) * 8) / 8               # (exact in float32: every variant holds the same numbers)
    coo = sp.coo_matrix((vals, (rows, cols)), shape=(m, n))
    assert coo.nnz > _canon(coo).nnz, "the COO input should hold duplicates"
    ref = _canon(coo)
    unsorted = ref.copy()
    for i in range(m):   # reverse every row: unsorted indices
        lo, hi = unsorted.indptr[i], unsorted.indptr[i + 1]
        unsorted.indices[lo:hi] = unsorted.indices[lo:hi][::-1].copy()
        unsorted.data[lo:hi] = unsorted.data[lo:hi][::-1].copy()
    unsorted.has_sorted_indices = False
    wide = ref.copy()
    wide.indices = wide.indices.astype(np.int64)
    wide.indptr = wide.indptr.astype(np.int64)
    return ref, {"coo-duplicates": coo, "csr-unsorted": unsorted, "csc": ref.tocsc(), "int64-indices": wide,
                 "float32": ref.astype(np.float32), "lil": ref.tolil(), "sparse-array": sp.csr_array(ref)}


def test_every_input_format_gives_the_same_canonical_arrays():
    ref, variants = _variants()
    refT = _canon(ref.T.tocsr())
    for name, A in variants.items():
        p = sparse.prepare(A, np.zeros(ref.shape[0]))
        assert (p["m"], p["n"], p["nnz"]) == (*ref.shape, ref.nnz), name
        for key, want in (("indptr", ref.indptr), ("indices", ref.indices), ("data", ref.data),
                          ("t_indptr", refT.indptr), ("t_indices", refT.indices), ("t_data", refT.data)):
            assert np.array_equal(p[key], want), (name, key)
        assert p["indptr"].dtype == p["t_indptr"].dtype == np.int64, name
        assert p["indices"].dtype == p["t_indices"].dtype == np.int32, name
        assert p["data"].dtype == p["t_data"].dtype == np.float64, name
        assert all(p[k].flags.c_contiguous for k in ("indptr", "indices", "data", "t_indptr", "t_indices", "t_data")), name


def test_dense_inputs_are_accepted():
    """A dense 2-D array or a nested list is converted like any other input (the shape is the canonical matrix's)."""
    rows = [[0, 5, 0], [2, 0, -3]]   # (whole numbers: the int32 variant holds the same values)
    ref = _canon(sp.csr_matrix(np.array(rows, dtype=float)))
    for A in (rows, np.array(rows), np.array(rows, dtype=np.int32)):
        p = sparse.prepare(A, [0.0, 1.0])
        assert (p["m"], p["n"], p["nnz"]) == (2, 3, 3)
        assert np.array_equal(p["indices"], ref.indices) and np.array_equal(p["data"], ref.data)
    with pytest.raises(ValueError):
        sparse.prepare([[1.0, 2.0], [3.0]], [0.0, 0.0])   # ragged: no 2-D numeric array


def test_a_matrix_without_stored_elements_is_legal():
    for A in (sp.csr_matrix((3, 1)), sp.coo_matrix((4, 7)), sp.csc_matrix((1, 1))):
        p = sparse.prepare(A, np.zeros(A.shape[0]))
        assert p["nnz"] == 0 and p["data"].size == 0 and p["indices"].size == 0
        assert np.array_equal(p["indptr"], np.zeros(A.shape[0] + 1)) and np.array_equal(p["t_indptr"], np.zeros(A.shape[1] + 1))
        for plan in (p["plan"], p["t_plan"]):
            assert plan["lanes"] == 4 and plan["split_row"].size == 0 and plan["seg_start"].size == 0
            assert np.array_equal(plan["split_first"], [0])


def test_value_errors():
    from zfista_amd.problems import SparseLeastSquaresL1

    A = sp.random(5, 8, density=0.5, random_state=np.random.default_rng(0), format="csr")
    b = np.zeros(5)
    bad_value = A.copy()
    bad_value.data[3] = np.inf
    nan_value = A.copy()
    nan_value.data[0] = np.nan
    cases = {
        "1-D A": (np.ones(4), np.zeros(4)),
        "3-D A": (np.ones((2, 2, 2)), np.zeros(2)),
        "b too long": (A, np.zeros(6)),
        "b too short": (A, np.zeros(4)),
        "b 2-D": (A, np.zeros((5, 1))),
        "inf in A": (bad_value, b),
        "nan in A": (nan_value, b),
        "nan in b": (A, np.array([0, 0, np.nan, 0, 0.0])),
        "n = 2^31": (sp.csr_matrix((1, 2 ** 31)), np.zeros(1)),
        "m = 2^31": (sp.csc_matrix((2 ** 31, 1)), np.zeros(1)),
        "complex": (A.astype(np.complex128), b),
    }
    for name, (M, rhs) in cases.items():
        with pytest.raises(ValueError):
            sparse.prepare(M, rhs)
        with pytest.raises(ValueError):   # the class checks on the host, before it needs a device
            SparseLeastSquaresL1(M, rhs, 0.1)
    with pytest.raises(TypeError):
        SparseLeastSquaresL1(A, b, 0.1, group=None)   # single GPU: no group= / shard= keyword


def _check_plan(indptr, plan):
    """Every stored element of a split row lies in exactly one segment; segments of a row are consecutive, in order and
    at most `threshold` long; rows that are not split are at most `threshold` long."""
    T = plan["threshold"]
    lengths = np.diff(indptr)
    split, first, start = plan["split_row"], plan["split_first"], plan["seg_start"]
    assert np.array_equal(split, np.flatnonzero(lengths > T))
    assert first.size == split.size + 1 and first[0] == 0 and first[-1] == start.size
    assert split.dtype == first.dtype == start.dtype == np.int64
    covered = 0
    for j, row in enumerate(split):
        lo, hi = indptr[row], indptr[row + 1]
        segs = start[first[j]:first[j + 1]]
        assert segs.size >= 2 and segs[0] == lo
        ends = np.minimum(segs + T, hi)
        assert np.array_equal(segs[1:], ends[:-1]), "segments of a row must be consecutive and in order"
        assert ends[-1] == hi and np.all(ends - segs >= 1) and np.all(ends - segs <= T)
        covered += int(np.sum(ends - segs))
    assert covered == int(lengths[split].sum())
    assert plan["lanes"] in (4, 8, 16, 32, 64)


def test_segment_plan_on_row_length_profiles():
    rng = np.random.default_rng(9)
    profiles = {
        "all empty": np.zeros(1000, dtype=np.int64),
        "one row of 1e6": np.array([3, 0, 10 ** 6, 7]),
        "geometric": np.minimum(rng.geometric(1e-4, 3000), 200_000),
        "exactly at the threshold": np.array([sparse.SPLIT_THRESHOLD, sparse.SPLIT_THRESHOLD + 1, 2 * sparse.SPLIT_THRESHOLD,
                                              2 * sparse.SPLIT_THRESHOLD + 1, 1]),
        "one element per row": np.ones(777, dtype=np.int64),
        "single empty row": np.zeros(1, dtype=np.int64),
    }
    for name, lengths in profiles.items():
        indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        plan = sparse.plan_rows(indptr)
        _check_plan(indptr, plan)
        # a function of the lengths alone: the same lengths behind other offsets, in other dtypes, give the same plan
        again = sparse.plan_rows(indptr.astype(np.int32) if indptr[-1] < 2 ** 31 else indptr)
        assert again["lanes"] == plan["lanes"] and np.array_equal(again["seg_start"], plan["seg_start"]), name
        assert plan["lanes"] == sparse.lanes_for(lengths) == sparse.lanes_for(lengths[::-1]), name
    p = sparse.plan_rows(np.concatenate([[0], np.cumsum(profiles["exactly at the threshold"])]))
    assert list(p["split_row"]) == [1, 2, 3] and list(np.diff(p["split_first"])) == [2, 2, 3]
    assert sparse.plan_rows(np.array([0, 10 ** 6]))["seg_start"].size == -(-10 ** 6 // sparse.SPLIT_THRESHOLD)
    # a small threshold cuts short rows too (the rule does not depend on the constant)
    indptr = np.concatenate([[0], np.cumsum(rng.integers(0, 40, 200))])
    _check_plan(indptr, sparse.plan_rows(indptr, threshold=7))


def test_lanes_follow_the_mean_row_length():
    # the largest power of two in [4, 64] that is at most nnz / rows
    for mean, want in ((0, 4), (1, 4), (7.99, 4), (8, 8), (15, 8), (16, 16), (31.5, 16), (32, 32), (63, 32), (64, 64), (5000, 64)):
        rows = 200
        lengths = np.full(rows, int(mean), dtype=np.int64)
        lengths[: int(round((mean - int(mean)) * rows))] += 1
        assert sparse.lanes_for(lengths) == want, (mean, lengths.sum() / rows)


def test_plan_summation_order_reproduces_the_row_sums():
    """The kernels' order restated in NumPy (L lanes with stride L, the shuffle tree, segments of a split row added in
    order) sums every element once: equal to A @ x up to rounding, on a matrix with split and empty rows."""
    rng = np.random.default_rng(3)
    A = sp.random(40, 300, density=0.3, random_state=rng, data_rvs=rng.standard_normal, format="lil")
    A[7, :] = rng.standard_normal(300)
    A[11, :] = 0
    A = _canon(A.tocsr())
    x = rng.standard_normal(300)
    plan = sparse.plan_rows(A.indptr, threshold=64)
    assert 7 in plan["split_row"]

    def lanes_sum(lo, hi, L):
        part = np.array([np.sum((A.data[lo + l:hi:L] * x[A.indices[lo + l:hi:L]])) for l in range(L)])
        while part.size > 1:
            part = part[: part.size // 2] + part[part.size // 2:]
        return part[0]

    out = np.zeros(40)
    split = set(plan["split_row"].tolist())
    for i in range(40):
        if i not in split:
            out[i] = lanes_sum(A.indptr[i], A.indptr[i + 1], plan["lanes"])
    for j, row in enumerate(plan["split_row"]):
        segs = plan["seg_start"][plan["split_first"][j]:plan["split_first"][j + 1]]
        out[row] = sum(lanes_sum(s, min(s + 64, A.indptr[row + 1]), 64) for s in segs)
    np.testing.assert_allclose(out, A @ x, rtol=0, atol=1e-12)
    assert out[11] == 0.0


def test_abi_additions():
    src = open(os.path.join(ROOT, "include", "zfista_hip.h")).read()
    assert re.search(r"#define\s+ZF_PROBLEM_SPARSE_LS_L1\s+4\b", src) and _lib.ZF_PROBLEM_SPARSE_LS_L1 == 4
    assert re.search(r"#define\s+ZF_ABI_VERSION\s+7\b", src)
    for name in ("zf_spmat_create", "zf_spmat_destroy", "zf_margins_eval", "zf_solver_create_sparse"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\s*\(", src), name
    assert C.sizeof(_lib.SpmvPlan) == 56 and C.sizeof(_lib.ProblemDesc) == 128 and C.sizeof(_lib.Options) == 64
    lib = _lib.load()
    assert lib.zf_abi_version() == 7 and lib.zf_sizeof_control() == 424
    # size and null checks come before anything is dereferenced or any device is touched
    h = C.c_void_p()
    plan = _lib.SpmvPlan(lanes=4, threshold=4096)
    dummy = (C.c_ubyte * 4096)()
    P = C.addressof(dummy)
    args = lambda **kw: [kw.get("out", C.byref(h)), kw.get("m", 3), kw.get("n", 2), 1, P, P, P, C.byref(plan), P, P, P, C.byref(plan),
                         kw.get("bytes", C.sizeof(plan))]
    assert lib.zf_spmat_create(*args(bytes=48)) == -2 and b"plan_bytes" in lib.zf_last_error()
    assert lib.zf_spmat_create(*args(out=None)) == -2 and b"null" in lib.zf_last_error()
    assert lib.zf_spmat_create(*args(m=0)) == -2 and lib.zf_spmat_create(*args(n=2 ** 31)) == -2
    assert h.value is None
    assert lib.zf_spmat_destroy(None) == 0
    fval = C.c_double(0.0)
    assert E.point(E.sparse(None), P, C.byref(fval)) == -2 and b"zf_margins_eval" in lib.zf_last_error()
    d, o, s = _lib.ProblemDesc(kind=4, world=1, n=2, m_rows=3), _lib.Options(lr=1.0, decay_rate=0.5, max_iter=1), C.c_void_p()
    assert lib.zf_solver_create_sparse(C.byref(s), C.byref(d), None, C.byref(o), None) == -2
    d.kind = 2
    assert lib.zf_solver_create_sparse(C.byref(s), C.byref(d), P, C.byref(o), None) == -2 and b"kind" in lib.zf_last_error()
    d.kind = 4   # the matrix of this kind comes through zf_solver_create_sparse only
    assert lib.zf_solver_create(C.byref(s), C.byref(d), C.byref(o), None) == -2 and b"zf_solver_create_sparse" in lib.zf_last_error()
    assert s.value is None
