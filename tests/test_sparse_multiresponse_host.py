"""CPU: the interface of the sparse multi-response classes without a GPU - header, ctypes table and the built library (the
struct sizes as they were, no problem kind), the argument checks of the new entry points before any device is
touched, the ValueErrors of the host classes (each before anything is uploaded), shape broadcasting, the descriptor, the siblings."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import evaldesc as E
from conftest import ROOT
from zfista_amd import _lib, path, problems, screening
from zfista_amd.proximal_gradient import minimize_proximal_gradient

NEW = ("zf_solver_create_sparse_responses", "zf_margins_eval", "zf_margins_gap", "zf_spmat_mr_apply")
MR = [problems.SparseMultiResponseLeastSquaresL1, problems.SparseMultiResponseLogisticL1]


def test_header_ctypes_table_and_library_hold_the_new_entry_points_and_nothing_else_moved():
    src = open(os.path.join(ROOT, "include", "zfista_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(zf_[A-Za-z0-9_]+)\s*\(", src))), "header = ctypes table"
    assert lib.zf_abi_version() == 7 and lib.zf_sizeof_control() == 424 == C.sizeof(_lib.Control)
    assert C.sizeof(_lib.ProblemDesc) == 128 and C.sizeof(_lib.Options) == 64, "additive exports only: no struct field"
    assert max(v for k, v in vars(_lib).items() if k.startswith("ZF_PROBLEM_")) == 6, "no new problem kind"
    assert len(_lib.SIGNATURES["zf_solver_create_sparse_responses"][1]) == len(_lib.SIGNATURES["zf_solver_create_sparse"][1]) + 1
    mk = open(os.path.join(ROOT, "zfista_amd", "csrc", "Makefile")).read()
    assert "zf_spmm.hip" in mk and "zf_kernels_spmm.h" in mk, "a translation unit of its own, a header the objects depend on"


def test_new_entry_points_refuse_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    out = np.full(12, -7.0)
    P = C.c_void_p(_lib.ptr(out))
    f = C.c_double(-7.0)
    d, o, h = _lib.ProblemDesc(), _lib.Options(), C.c_void_p()
    d.kind = _lib.ZF_PROBLEM_SPARSE_LS_L1
    assert lib.zf_solver_create_sparse_responses(C.byref(h), C.byref(d), None, 2, C.byref(o), None) == -2
    assert b"zf_solver_create_sparse_responses" in lib.zf_last_error()
    for bad in (1, 0, -3, 17):   # (K is checked before the handle is read: P is no handle)
        assert lib.zf_solver_create_sparse_responses(C.byref(h), C.byref(d), P, bad, C.byref(o), None) == -2 and b"2 .. 16" in lib.zf_last_error()
    for bad in (0, -3, 17):   # (K = 1 is the plain problem; K is checked before the handle is read)
        assert E.point(E.sparse(P, K=bad), P, C.byref(f)) == -2 and b"K must be 1 .. 16" in lib.zf_last_error()
        assert E.gap(E.sparse(P, K=bad), P, P, 10) == -2 and b"K must be 1 .. 16" in lib.zf_last_error()
    d.kind = _lib.ZF_PROBLEM_LEAST_SQUARES_L1
    assert lib.zf_solver_create_sparse_responses(C.byref(h), C.byref(d), P, 2, C.byref(o), None) == -2
    assert b"ZF_PROBLEM_SPARSE_LS_L1 or ZF_PROBLEM_SPARSE_LOGISTIC_L1" in lib.zf_last_error()
    for bad in (2, 3, -1, 7):   # Huber, Poisson, unknown
        assert E.point(E.sparse(P, K=2, loss=bad, delta=1.0), P, C.byref(f)) == -2 and b"ZF_LOSS_SQUARE or ZF_LOSS_LOGISTIC" in lib.zf_last_error()
        assert E.gap(E.sparse(P, K=2, loss=bad, delta=1.0), P, P, 10) == -2
    assert E.point(E.sparse(None, K=2), P, C.byref(f)) == -2 and b"zf_margins_eval" in lib.zf_last_error()
    assert E.point(E.sparse(P, K=2, b=None), P, C.byref(f)) == -2
    assert E.point(E.sparse(P, K=2), None, C.byref(f)) == -2
    assert E.gap(E.sparse(None, K=2), P, P, 10) == -2 and b"zf_margins_gap" in lib.zf_last_error()
    assert E.gap(E.sparse(P, K=2), P, P, 7) == -2 and b"fewer than 8" in lib.zf_last_error()
    assert E.gap(E.sparse(P, K=2, scale=0.0), P, P, 10) == -2 and b"scale > 0" in lib.zf_last_error()
    for bad in (-1e-9, float("inf"), float("nan")):
        assert E.gap(E.sparse(P, K=2, l2=bad), P, P, 10) == -2 and b"l2" in lib.zf_last_error()
    for bad in (0, -1, 17):
        assert lib.zf_spmat_mr_apply(P, 0, bad, 1.0, P, P) == -2 and b"1 .. 16" in lib.zf_last_error()
    assert lib.zf_spmat_mr_apply(None, 0, 2, 1.0, P, P) == -2 and lib.zf_spmat_mr_apply(P, 0, 2, 1.0, None, P) == -2
    assert (out == -7.0).all() and f.value == -7.0 and not h.value


@pytest.mark.parametrize("cls", MR)
def test_the_constructors_refuse_before_anything_touches_a_device(cls, monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "require_gpu", touched)
    monkeypatch.setattr(_lib, "load", touched)
    logistic = cls is problems.SparseMultiResponseLogisticL1
    A = sp.csr_matrix(np.ones((4, 3)))
    B = np.ones((4, 2))
    with pytest.raises(ValueError, match=r"B \(m, K\)"):
        cls(A, np.ones(4), 0.1)
    with pytest.raises(ValueError, match=r"B \(m, K\)"):
        cls(A, np.ones((5, 2)), 0.1)
    with pytest.raises(ValueError, match="at most 16 responses"):
        cls(A, np.ones((4, 17)), 0.1)
    with pytest.raises(ValueError, match="l2 must be finite"):
        cls(A, B, 0.1, l2=-1.0)
    for bad in (np.full(4, np.nan), -np.ones((4, 2)), np.zeros(4)):
        with pytest.raises(ValueError, match="sample_weight"):
            cls(A, B, 0.1, sample_weight=bad)
    with pytest.raises(ValueError, match=r"sample_weight must have shape \(4,\) or \(4, 2\)"):
        cls(A, B, 0.1, sample_weight=np.ones((4, 3)))
    with pytest.raises(ValueError, match=r"penalty_factor must have shape \(3,\) or \(3, 2\)"):
        cls(A, B, 0.1, penalty_factor=np.ones(4))
    with pytest.raises(ValueError, match="penalty_factor must be finite and >= 0"):
        cls(A, B, 0.1, penalty_factor=-np.ones((3, 2)))
    with pytest.raises(ValueError, match="penalty_factor is not available with l2 > 0"):
        cls(A, B, 0.1, l2=0.5, penalty_factor=np.ones(3))
    with pytest.raises(ValueError, match="non-finite"):
        cls(sp.csr_matrix(np.array([[np.inf, 1.0, 0.0]] * 4)), B, 0.1)
    if logistic:
        with pytest.raises(ValueError, match="exactly -1 or \\+1"):
            cls(A, 0.5 * B, 0.1)
    else:
        with pytest.raises(ValueError, match="B holds non-finite"):
            cls(A, np.full((4, 2), np.nan), 0.1)
    params = inspect.signature(cls.__init__).parameters
    assert list(params)[:7] == ["self", "A", "B", "lam", "scale", "bounds", "l2"]
    assert params["scale"].default == (1.0 if logistic else 0.5) and params["l2"].default == 0.0
    assert params["sample_weight"].kind is inspect.Parameter.KEYWORD_ONLY and params["penalty_factor"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "group" not in params and "matrix_dtype" not in params


class _H:   # what the host logic reads of a matrix handle
    class value:
        value = 8192


class _T:   # ... and of a device tensor
    def data_ptr(self):
        return 4096

    def numel(self):
        return 35


def _standin(cls, K=3):
    """A problem object without a device: the attributes the host logic reads."""
    p = object.__new__(cls)
    p._spmat, p.b = _H(), _T()
    p.lam, p.scale, p.box, p.group = 0.3, 0.5, (-np.inf, np.inf), None
    p._m, p._n, p.n_responses = 5, 7, K
    p.m_rows, p.n_features = 5 * K, 7 * K
    p._norms = problems._ColumnNorms()
    return p


@pytest.mark.parametrize("cls", MR)
def test_the_descriptor_carries_the_handle_the_responses_and_no_new_kind(cls):
    base = problems.SparseLogisticL1 if cls is problems.SparseMultiResponseLogisticL1 else problems.SparseLeastSquaresL1
    assert cls.kind == base.kind and cls._loss == base._loss and issubclass(cls, problems._SparseMarginsL1)
    assert issubclass(cls, problems._MultiResponseMixin) and not issubclass(cls, problems._DenseMarginsL1)
    p = _standin(cls)
    fields, keep = p._descriptor()
    assert fields["responses"] == 3 and fields["m_rows"] == 15 and fields["n"] == 21 and fields["kind"] == cls.kind
    assert fields["spmat"] == 8192 and fields["A"] is None and keep[0] is p._spmat
    assert "responses" not in _standin(cls, 1)._descriptor()[0], "K = 1 is the plain problem: the plain creator"
    fields, _ = p.with_penalty(0.3, 0.25)._descriptor()
    assert fields["responses"] == 3 and fields["l2"] == 0.25
    q = p.with_lam(0.2)
    assert type(q) is cls and q._spmat is p._spmat and q.b is p.b and q.n_responses == 3 and p.lam == 0.3
    assert problems.match_native(*q.callbacks()) is q
    e = p._eval_desc()
    assert (e.spmat, e.A, e.A32, e.b, e.w, e.p, e.K, e.loss) == (8192, None, None, 4096, None, None, 3, cls._loss), "the handle, b, K; no weights"
    assert p.coef(np.arange(21.0)).shape == (7, 3) and p.coef(np.arange(21.0))[2, 1] == 7.0
    assert p._flat(np.zeros((7, 3))).shape == (21,) and p._flat(np.zeros(21)).shape == (21,)
    assert p.has_duality_gap and p._gap_refusal() is None
    assert hasattr(base, "with_responses") and not hasattr(problems.SparseHuberL1, "with_responses")
    assert not hasattr(problems.SparsePoissonL1, "with_responses")


def test_shapes_broadcast_as_for_the_dense_classes():
    w = problems._broadcast_columns(np.arange(1.0, 6.0), 5, 3, "sample_weight", "row")
    assert w.shape == (5, 3) and np.array_equal(w[:, 0], w[:, 2]) and w.reshape(-1)[4] == 2.0
    p = _standin(MR[0])
    with pytest.raises(ValueError, match=r"sample_weight must have shape \(5,\) or \(5, 3\)"):
        p.with_sample_weight(np.ones(7))
    with pytest.raises(ValueError, match=r"penalty_factor must have shape \(7,\) or \(7, 3\)"):
        p.with_penalty_factor(np.ones((7, 2)))
    assert p.with_sample_weight(None)._w is None and p.with_penalty_factor(None)._pf is None


@pytest.mark.parametrize("cls", MR)
def test_what_has_no_k_response_form_is_refused_with_its_message(cls, monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "require_gpu", touched)
    p = _standin(cls)
    x = np.zeros(21)
    for call in (lambda: p.screen(x), lambda: p.column_norms(), lambda: p.restrict(np.arange(3)),
                 lambda: screening.solve_screened(p, x, 1e-6), lambda: path.l1_path(p, [0.1], screen=True)):
        with pytest.raises(ValueError, match="several responses"):
            call()
    for bad in ("remainder", "resolved"):
        with pytest.raises(ValueError, match=f"acceptance='{bad}' is not available with several responses"):
            minimize_proximal_gradient(*p.callbacks(), x, acceptance=bad)
    with pytest.raises(ValueError, match="sparse matrix is stored as fp64"):
        p.with_matrix_dtype("float32")
    boxed = _standin(cls)
    boxed.box = (-1.0, 1.0)
    with pytest.raises(ValueError, match="bounds are set"):
        boxed.duality_gap(x)
    with pytest.raises(ValueError, match="n_features"):
        p.duality_gap(np.zeros(20))


def test_with_responses_checks_b_against_the_shared_handle_before_a_device():
    base = object.__new__(problems.SparseLeastSquaresL1)
    base._spmat, base.b = _H(), _T()
    base.m_rows, base.n_features, base.nnz, base.plan, base._longest = 5, 7, 11, (None, None), (3, 4)
    base.lam, base.scale, base.box, base.group, base.l2 = 0.3, 0.5, (-1.0, 1.0), None, 0.0
    with pytest.raises(ValueError, match="at most 16 responses"):
        base.with_responses(np.ones((5, 17)))
    with pytest.raises(ValueError, match=r"B \(m, K\)"):
        base.with_responses(np.ones((4, 2)))
    with pytest.raises(ValueError, match=r"sample_weight must have shape \(5,\) or \(5, 2\)"):
        base.with_responses(np.ones((5, 2)), sample_weight=np.ones(4))
    logit = object.__new__(problems.SparseLogisticL1)
    logit.__dict__.update(base.__dict__)
    with pytest.raises(ValueError, match="exactly -1 or \\+1"):
        logit.with_responses(np.zeros((5, 2)))


def test_l1_cv_lockstep_accepts_the_sparse_classes_at_its_gate():
    with pytest.raises(ValueError, match="SparseLeastSquaresL1 or SparseLogisticL1"):
        path.l1_cv_lockstep(object(), [0.1])
    with pytest.raises(ValueError, match="SparseLeastSquaresL1 or SparseLogisticL1"):
        path.l1_cv_lockstep(object.__new__(problems.SparseHuberL1), [0.1])
    for cls in (problems.SparseLeastSquaresL1, problems.SparseLogisticL1):
        base = object.__new__(cls)
        base.m_rows, base.n_features, base._w_host = 40, 7, None
        with pytest.raises(ValueError, match="needs gap_tol"):   # (behind the gate)
            path.l1_cv_lockstep(base, [0.1], gap_tol=None)
        with pytest.raises(ValueError, match="at most 16 folds"):
            path.l1_cv_lockstep(base, [0.1], folds=17)


def test_the_classes_are_exported_and_documented():
    for cls in MR:
        assert issubclass(cls, problems.NativeProblem) and cls.n_responses == 1 and cls.taylor_remainder is False
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "SparseMultiResponseLeastSquaresL1(A, B, lam" in readme and "SparseMultiResponseLogisticL1" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.5n" in design and "zf_spmm_rows_kernel" in design
    for rel in ("examples/multi_response_sparse.py", "tools/bench_sparse_multiresponse.py"):
        assert os.path.exists(os.path.join(ROOT, rel)), rel
