"""CPU: the host part of LogisticL1 / SparseLogisticL1 - label, shape and dtype rejections before anything touches a device,
the descriptor fields, the additive C ABI - and that nothing under zfista_amd/ imports the oracle.  No GPU."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import evaldesc as E
from conftest import ROOT
from zfista_amd import _lib


def _inputs():
    A = sp.random(5, 8, density=0.5, random_state=np.random.default_rng(0), format="csr")
    return A, np.array([1.0, -1.0, 1.0, 1.0, -1.0])


BAD_LABELS = {
    "zero": [1.0, -1.0, 0.0, 1.0, -1.0],
    "0/1 labels": [1.0, 0.0, 1.0, 1.0, 0.0],
    "almost one": [1.0, -1.0, 1.0 + 2.0 ** -52, 1.0, -1.0],
    "two": [1.0, -1.0, 2.0, 1.0, -1.0],
    "nan": [1.0, -1.0, np.nan, 1.0, -1.0],
    "inf": [1.0, -1.0, np.inf, 1.0, -1.0],
    "too long": [1.0, -1.0, 1.0, 1.0, -1.0, 1.0],
    "too short": [1.0, -1.0, 1.0, 1.0],
    "2-D": [[1.0], [-1.0], [1.0], [1.0], [-1.0]],
    "strings": ["1", "-1", "1", "1", "-1"],
    "complex": np.array([1, -1, 1, 1, -1], dtype=np.complex128),
}


@pytest.mark.parametrize("name", list(BAD_LABELS))
def test_labels_other_than_plus_minus_one_raise_on_the_host(name, monkeypatch):
    from zfista_amd import problems

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the labels were checked")

    monkeypatch.setattr(_lib, "require_gpu", no_device)
    A, _ = _inputs()
    b = np.asarray(BAD_LABELS[name])
    for cls, M in ((problems.SparseLogisticL1, A), (problems.LogisticL1, A.toarray())):
        with pytest.raises(ValueError):
            cls(M, b, 0.1)


def test_shape_and_keyword_rejections(monkeypatch):
    from zfista_amd import problems

    A, b = _inputs()
    monkeypatch.setattr(_lib, "require_gpu", lambda: (_ for _ in ()).throw(AssertionError("device touched")))
    for M in (np.ones(5), np.ones((5, 2, 2))):
        with pytest.raises(ValueError):
            problems.LogisticL1(M, b, 0.1)
        with pytest.raises(ValueError):
            problems.SparseLogisticL1(M, b, 0.1)
    bad = A.copy()
    bad.data[0] = np.nan
    with pytest.raises(ValueError):
        problems.SparseLogisticL1(bad, b, 0.1)
    with pytest.raises(ValueError):
        problems.SparseLogisticL1(sp.csr_matrix((1, 2 ** 31)), np.ones(1), 0.1)
    for cls, M in ((problems.SparseLogisticL1, A), (problems.LogisticL1, A.toarray())):
        with pytest.raises(TypeError):
            cls(M, b, 0.1, group=None)   # single GPU: no group= / shard= keyword
        with pytest.raises(TypeError):
            cls(M, b, 0.1, shard="rows")


def test_integer_and_bool_typed_labels_pass_the_host_check():
    from zfista_amd.problems import _check_labels

    for b in (np.array([1, -1, 1], dtype=np.int8), np.array([1.0, -1.0, -1.0], dtype=np.float32), [1, -1, 1]):
        assert _check_labels(b, 3).shape == (3,)
    with pytest.raises(ValueError):
        _check_labels(np.array([True, False, True]), 3)   # False is 0: no label


def test_descriptor_fields_and_class_layout():
    """The descriptor of the new kinds (built without a device: the classes' _descriptor on stand-in fields), the defaults and
    the class relations the engine relies on."""
    import inspect

    from zfista_amd import problems

    assert problems.LogisticL1.kind == _lib.ZF_PROBLEM_LOGISTIC_L1 == 5
    assert problems.SparseLogisticL1.kind == _lib.ZF_PROBLEM_SPARSE_LOGISTIC_L1 == 6
    for cls in (problems.LogisticL1, problems.SparseLogisticL1):
        assert issubclass(cls, problems.NativeProblem) and not getattr(cls, "separable", False)
        sig = inspect.signature(cls.__init__)
        assert list(sig.parameters) == ["self", "A", "b", "lam", "scale", "bounds"]
        assert sig.parameters["scale"].default == 1.0 and sig.parameters["bounds"].default is None
    # a logistic problem is no least-squares problem (the shared plumbing is a base without a loss) and cannot be sharded
    assert not issubclass(problems.LogisticL1, problems.LeastSquaresL1) and not hasattr(problems.LogisticL1, "shard")
    assert not issubclass(problems.SparseLogisticL1, problems.SparseLeastSquaresL1)
    assert problems.LogisticL1._loss == problems.SparseLogisticL1._loss == _lib.ZF_LOSS_LOGISTIC

    class _T:   # what _descriptor reads of a device tensor
        def data_ptr(self):
            return 4096

    class _H:
        value = C.c_void_p(8192)

    p = object.__new__(problems.LogisticL1)
    p.A, p.b, p.lam, p.scale, p.box, p.m_rows, p.n_features, p.group = _T(), _T(), 0.25, 1.0, (-np.inf, np.inf), 5, 8, None
    fields, _ = p._descriptor()
    assert fields["kind"] == 5 and fields["world"] == 1 and fields["rank"] == 0 and fields["row_sharded"] == 0
    assert (fields["n"], fields["m_rows"], fields["A"], fields["b"], fields["scale"], fields["lam"]) == (8, 5, 4096, 4096, 1.0, 0.25)
    e = p._eval_desc()
    assert (e.A, e.A32, e.spmat, e.m_rows, e.n, e.b, e.loss, e.K) == (4096, None, None, 5, 8, 4096, _lib.ZF_LOSS_LOGISTIC, 1)
    q = object.__new__(problems.SparseLogisticL1)
    q.b, q.lam, q.scale, q.box, q.m_rows, q.n_features, q._spmat = _T(), 0.25, 1.0, (-1.0, 2.0), 5, 8, _H()
    fields, _ = q._descriptor()
    assert fields["kind"] == 6 and fields["A"] is None and fields["spmat"] == 8192 and (fields["box_lo"], fields["box_hi"]) == (-1.0, 2.0)
    e = q._eval_desc()
    assert (e.A, e.A32, e.spmat, e.b, e.loss, e.K) == (None, None, 8192, 4096, _lib.ZF_LOSS_LOGISTIC, 1)
    d = _lib.ProblemDesc()
    for k, v in fields.items():
        if k != "spmat":
            setattr(d, k, v)
    assert d.kind == 6 and d.m_rows == 5 and d.n == 8 and d.scale == 1.0


def test_abi_additions():
    src = open(os.path.join(ROOT, "include", "zfista_hip.h")).read()
    assert re.search(r"#define\s+ZF_PROBLEM_LOGISTIC_L1\s+5\b", src) and re.search(r"#define\s+ZF_PROBLEM_SPARSE_LOGISTIC_L1\s+6\b", src)
    assert re.search(r"#define\s+ZF_ABI_VERSION\s+7\b", src)
    assert "zf_margins_eval" in _lib.SIGNATURES and re.search(r"\bzf_margins_eval\s*\(", src)
    assert re.search(r"ZF_LOSS_LOGISTIC\s*=\s*1\b", src) and _lib.ZF_LOSS_LOGISTIC == 1
    assert C.sizeof(_lib.ProblemDesc) == 128 and C.sizeof(_lib.Options) == 64
    lib = _lib.load()
    assert lib.zf_abi_version() == 7 and lib.zf_sizeof_control() == 424
    # argument checks come before anything is dereferenced or any device is touched
    dummy = (C.c_ubyte * 4096)()
    P = C.addressof(dummy)
    fval = C.c_double(0.0)
    assert E.point(E.dense(None, loss=1), P, C.byref(fval)) == -2 and b"zf_margins_eval" in lib.zf_last_error()
    assert E.point(E.dense(P, loss=1, m_rows=0), P, C.byref(fval)) == -2
    assert E.point(E.dense(P + 8, loss=1), P, C.byref(fval)) == -2 and b"aligned" in lib.zf_last_error()
    assert E.point(E.sparse(None, loss=1), P, C.byref(fval)) == -2 and b"zf_margins_eval" in lib.zf_last_error()
    # kind / creator mismatches
    o, s = _lib.Options(lr=1.0, decay_rate=0.5, max_iter=1), C.c_void_p()
    d = _lib.ProblemDesc(kind=6, world=1, n=2, m_rows=3)
    assert lib.zf_solver_create(C.byref(s), C.byref(d), C.byref(o), None) == -2 and b"zf_solver_create_sparse" in lib.zf_last_error()
    d.kind = 5
    assert lib.zf_solver_create_sparse(C.byref(s), C.byref(d), P, C.byref(o), None) == -2 and b"kind" in lib.zf_last_error()
    assert lib.zf_solver_create(C.byref(s), C.byref(d), C.byref(o), None) == -2   # (no A, no b)
    d.kind = 7
    assert lib.zf_solver_create(C.byref(s), C.byref(d), C.byref(o), None) == -2 and b"unknown" in lib.zf_last_error()
    assert s.value is None


def test_the_product_does_not_import_the_oracle():
    pat = re.compile(r"^\s*(from|import)\s+oracle\b|^\s*from\s+\.*\s*import\s+oracle\b|importlib\.import_module\(\s*['\"]oracle", re.M)
    files = sorted(glob.glob(os.path.join(ROOT, "zfista_amd", "**", "*.py"), recursive=True))
    assert len(files) >= 8
    for path in files:
        assert not pat.search(open(path).read()), f"{os.path.relpath(path, ROOT)} imports the oracle"
