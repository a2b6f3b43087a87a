"""Host side of sparse least squares: canonical CSR arrays and the row plan of the SpMV kernels.

Pure NumPy / SciPy - nothing here needs the library or a GPU.  ``SparseLeastSquaresL1`` (problems.py) uploads what
``prepare`` returns; ``csrc/zf_kernels_spmv.h`` describes how the kernels use the plan.
"""
from __future__ import annotations

import numpy as np

# rows longer than this are cut into segments of this many elements, each summed by a wave of its own
SPLIT_THRESHOLD = 4096
MIN_LANES, MAX_LANES = 4, 64
_INDEX_LIMIT = 2 ** 31


def canonical_csr(A):
    """(indptr int64, indices int32, data float64, (m, n)) of ``A`` as canonical CSR: duplicates summed, column indices sorted,
    explicit zeros kept.  ``A``: a 2-D scipy.sparse matrix / array of any format and real numeric dtype (or a dense 2-D
    array or nested list)."""
    import scipy.sparse as sp

    if not sp.issparse(A):
        A = np.asarray(A)
    if A.ndim != 2:
        raise ValueError(f"A must be 2-D, got {A.ndim} dimension(s)")
    if np.dtype(A.dtype).kind not in "biuf":
        raise ValueError(f"A must have a real numeric dtype, got {A.dtype}")
    m, n = A.shape
    if m >= _INDEX_LIMIT or n >= _INDEX_LIMIT:
        raise ValueError("A must have fewer than 2**31 rows and columns (32-bit indices on the device)")
    C = sp.csr_matrix(A, dtype=np.float64, copy=True)
    C.sum_duplicates()
    C.sort_indices()
    data = np.ascontiguousarray(C.data, dtype=np.float64)
    if not np.isfinite(data).all():
        raise ValueError("A holds non-finite values")
    return (np.ascontiguousarray(C.indptr, dtype=np.int64), np.ascontiguousarray(C.indices, dtype=np.int32), data,
            (int(m), int(n)))


def lanes_for(lengths):
    """Lanes that walk one row: the largest power of two in [4, 64] that is at most the mean row length."""
    lengths = np.asarray(lengths, dtype=np.int64)
    rows, nnz = max(int(lengths.size), 1), int(lengths.sum())
    lanes = MIN_LANES
    while 2 * lanes <= MAX_LANES and 2 * lanes * rows <= nnz:
        lanes *= 2
    return lanes


def plan_rows(indptr, threshold=SPLIT_THRESHOLD):
    """The plan of one CSR matrix, a function of its row lengths alone: ``lanes``; the rows longer than ``threshold``
    (``split_row``, increasing), cut into segments of ``threshold`` elements - segment ``s`` covers the elements
    ``seg_start[s] .. min(seg_start[s] + threshold, end of its row)``; the segments of ``split_row[j]`` are
    ``split_first[j] .. split_first[j + 1]``, consecutive and in element order."""
    indptr = np.asarray(indptr, dtype=np.int64)
    threshold = int(threshold)
    if threshold < 1:
        raise ValueError("threshold must be >= 1")
    lengths = np.diff(indptr)
    split_row = np.flatnonzero(lengths > threshold).astype(np.int64)
    per_row = (lengths[split_row] + threshold - 1) // threshold
    split_first = np.zeros(split_row.size + 1, dtype=np.int64)
    np.cumsum(per_row, out=split_first[1:])
    nseg = int(split_first[-1])
    within = np.arange(nseg, dtype=np.int64) - np.repeat(split_first[:-1], per_row)
    seg_start = np.repeat(indptr[split_row], per_row) + threshold * within
    return dict(lanes=lanes_for(lengths), threshold=threshold, split_row=split_row, split_first=split_first,
                seg_start=np.ascontiguousarray(seg_start, dtype=np.int64))


def prepare(A, b=None):
    """Everything the device needs of ``A`` (m x n): the canonical CSR arrays of A and of A^T (``A.T.tocsr()``, made
    canonical the same way) and their plans.  ``b``, when given, is checked against m.  Raises ValueError for a non-2-D
    A, m or n >= 2**31, non-finite values, a ``b`` that is not a finite vector of m values."""
    import scipy.sparse as sp

    indptr, indices, data, (m, n) = canonical_csr(A)
    if b is not None:
        b = np.asarray(b)
        if b.ndim != 1 or b.shape[0] != m:
            raise ValueError(f"b must be a vector of {m} values (the rows of A), got shape {b.shape}")
        if not np.isfinite(b).all():
            raise ValueError("b holds non-finite values")
    T = sp.csr_matrix((data, indices, indptr), shape=(m, n)).T.tocsr()
    t_indptr, t_indices, t_data, _ = canonical_csr(T)
    return dict(m=m, n=n, nnz=int(data.size),
                indptr=indptr, indices=indices, data=data, plan=plan_rows(indptr),
                t_indptr=t_indptr, t_indices=t_indices, t_data=t_data, t_plan=plan_rows(t_indptr))
