"""CPU: the interface of the multi-response classes without a GPU - header and ctypes table (the struct sizes
as they were, no problem kind), the argument checks of the new entry points before any device is touched, the ValueErrors of the
host classes (each with its message, each before anything is uploaded), the descriptor, the siblings."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import evaldesc as E
from conftest import ROOT
from zfista_amd import _lib, path, problems, screening
from zfista_amd.proximal_gradient import minimize_proximal_gradient

NEW = ("zf_solver_set_responses", "zf_margins_eval", "zf_margins_gap")
MR = [problems.MultiResponseLeastSquaresL1, problems.MultiResponseLogisticL1]


def test_header_and_ctypes_table_declare_the_new_entry_points_and_nothing_else_moved():
    src = open(os.path.join(ROOT, "include", "zfista_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(zf_[A-Za-z0-9_]+)\s*\(", src))), "header = ctypes table"
    assert lib.zf_abi_version() == 7 and lib.zf_sizeof_control() == 424 == C.sizeof(_lib.Control)
    assert C.sizeof(_lib.ProblemDesc) == 128 and C.sizeof(_lib.Options) == 64, "additive exports only: no struct field"
    assert "responses" not in [f[0] for f in _lib.ProblemDesc._fields_]
    assert max(v for k, v in vars(_lib).items() if k.startswith("ZF_PROBLEM_")) == 6, "no new problem kind"
    assert "K" in [f[0] for f in _lib.EvalDesc._fields_], "K is a field of the evaluation descriptor"


def test_new_entry_points_refuse_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    out = np.full(12, -7.0)
    P = C.c_void_p(_lib.ptr(out))
    f = C.c_double(-7.0)
    assert lib.zf_solver_set_responses(None, 2) == -2 and b"zf_solver_set_responses" in lib.zf_last_error()
    for bad in (0, -3, 17):
        assert E.point(E.dense(P, K=bad), P, C.byref(f)) == -2 and b"K must be 1 .. 16" in lib.zf_last_error()
        assert E.gap(E.dense(P, K=bad), P, P, 10) == -2 and b"K must be 1 .. 16" in lib.zf_last_error()
    for bad in (2, 3, -1, 7):   # Huber, Poisson, unknown
        assert E.point(E.dense(P, K=2, loss=bad, delta=1.0), P, C.byref(f)) == -2 and b"ZF_LOSS_SQUARE or ZF_LOSS_LOGISTIC" in lib.zf_last_error()
        assert E.gap(E.dense(P, K=2, loss=bad, delta=1.0), P, P, 10) == -2
    assert E.point(E.dense(None, K=2), P, C.byref(f)) == -2 and b"zf_margins_eval" in lib.zf_last_error()
    assert E.point(E.dense(P, K=2, b=None), P, C.byref(f)) == -2
    assert E.point(E.dense(P, K=2, m_rows=0), P, C.byref(f)) == -2
    assert E.point(E.dense(P, K=2), None, C.byref(f)) == -2
    assert E.gap(E.dense(None, K=2), P, P, 10) == -2 and b"zf_margins_gap" in lib.zf_last_error()
    assert E.gap(E.dense(P, K=2), P, P, 7) == -2 and b"fewer than 8" in lib.zf_last_error()
    assert E.gap(E.dense(P, K=2, scale=0.0), P, P, 10) == -2 and b"scale > 0" in lib.zf_last_error()
    assert E.gap(E.dense(P, K=2, lam=-0.1), P, P, 10) == -2 and b"lam >= 0" in lib.zf_last_error()
    for bad in (-1e-9, float("inf"), float("nan")):
        assert E.gap(E.dense(P, K=2, l2=bad), P, P, 10) == -2 and b"l2" in lib.zf_last_error()
    assert E.gap(E.dense(P, K=2, p=P, l2=0.25), P, P, 10) == -2 and b"penalty factors and l2" in lib.zf_last_error()
    assert (out == -7.0).all() and f.value == -7.0


@pytest.mark.parametrize("cls", MR)
def test_the_constructors_refuse_before_anything_touches_a_device(cls):
    logistic = cls is problems.MultiResponseLogisticL1
    A = np.ones((4, 3))
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
    if logistic:
        with pytest.raises(ValueError, match="exactly -1 or \\+1"):
            cls(A, 0.5 * B, 0.1)
    params = inspect.signature(cls.__init__).parameters
    assert list(params)[:7] == ["self", "A", "B", "lam", "scale", "bounds", "l2"]
    assert params["scale"].default == (1.0 if logistic else 0.5) and params["l2"].default == 0.0
    assert params["sample_weight"].kind is inspect.Parameter.KEYWORD_ONLY and params["penalty_factor"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "group" not in params and "matrix_dtype" not in params


class _T:   # what the host logic reads of a device tensor
    shape = (5, 7)

    def data_ptr(self):
        return 4096

    def numel(self):
        return 35


def _standin(cls, K=3):
    """A problem object without a device: the attributes the host logic reads."""
    p = object.__new__(cls)
    p.A = p.b = _T()
    p.lam, p.scale, p.box, p.group = 0.3, 0.5, (-np.inf, np.inf), None
    p._m, p._n, p.n_responses = 5, 7, K
    p.m_rows, p.n_features = 5 * K, 7 * K
    p._norms = problems._ColumnNorms()
    return p


@pytest.mark.parametrize("cls", MR)
def test_the_descriptor_carries_the_responses_and_no_new_kind(cls):
    base = problems.LogisticL1 if cls is problems.MultiResponseLogisticL1 else problems.LeastSquaresL1
    assert cls.kind == base.kind and cls._loss == base._loss and issubclass(cls, problems._DenseMarginsL1)
    p = _standin(cls)
    fields, _ = p._descriptor()
    assert fields["responses"] == 3 and fields["m_rows"] == 15 and fields["n"] == 21 and fields["kind"] == cls.kind
    assert "responses" not in _standin(cls, 1)._descriptor()[0], "K = 1 is the plain problem: the setter is not called"
    fields, _ = p.with_penalty(0.3, 0.25)._descriptor()
    assert fields["responses"] == 3 and fields["l2"] == 0.25
    q = p.with_lam(0.2)
    assert type(q) is cls and q.A is p.A and q.b is p.b and q.n_responses == 3 and p.lam == 0.3
    assert problems.match_native(*q.callbacks()) is q
    assert p.coef(np.arange(21.0)).shape == (7, 3) and p.coef(np.arange(21.0))[2, 1] == 7.0
    assert p._flat(np.zeros((7, 3))).shape == (21,) and p._flat(np.zeros(21)).shape == (21,)
    assert p.has_duality_gap and p._gap_refusal() is None
    plain = object.__new__(base)
    assert not hasattr(plain, "n_responses") and hasattr(base, "with_responses")


@pytest.mark.parametrize("cls", MR)
def test_what_has_no_k_response_form_is_refused_with_its_message(cls):
    p = _standin(cls)
    x = np.zeros(21)
    for call in (lambda: p.screen(x), lambda: p.column_norms(), lambda: p.restrict(np.arange(3)),
                 lambda: screening.solve_screened(p, x, 1e-6), lambda: path.l1_path(p, [0.1], screen=True)):
        with pytest.raises(ValueError, match="several responses"):
            call()
    for bad in ("remainder", "resolved"):
        with pytest.raises(ValueError, match=f"acceptance='{bad}' is not available with several responses"):
            minimize_proximal_gradient(*p.callbacks(), x, acceptance=bad)
    with pytest.raises(ValueError, match="matrix_dtype='float32' is not available with several responses"):
        p.with_matrix_dtype("float32")
    boxed = _standin(cls)
    boxed.box = (-1.0, 1.0)
    with pytest.raises(ValueError, match="bounds are set"):
        boxed.duality_gap(x)
    with pytest.raises(ValueError, match="n_features"):
        p.duality_gap(np.zeros(20))


def test_with_responses_is_refused_on_fp32_and_sharded_problems_only():
    base = object.__new__(problems.LeastSquaresL1)
    base.A = base.b = _T()
    base.lam, base.scale, base.box, base.group, base.l2 = 0.3, 0.5, (-1.0, 1.0), None, 0.0
    base._f32 = True
    with pytest.raises(ValueError, match="with_responses is not available with matrix_dtype='float32'"):
        base.with_responses(np.ones((5, 2)))
    base._f32, base.group = False, object()
    with pytest.raises(ValueError, match="with_responses is not available with group="):
        base.with_responses(np.ones((5, 2)))
    base.group = None
    with pytest.raises(ValueError, match="at most 16 responses"):   # (a boxed problem gets as far as the checks of B)
        base.with_responses(np.ones((5, 17)))
    with pytest.raises(ValueError, match=r"B \(m, K\)"):
        base.with_responses(np.ones((4, 2)))


def test_l1_cv_lockstep_refuses_before_anything_is_solved():
    p = _standin(problems.MultiResponseLeastSquaresL1)
    with pytest.raises(ValueError, match="needs a dense LeastSquaresL1 or LogisticL1"):
        path.l1_cv_lockstep(object(), [0.1])
    base = object.__new__(problems.LeastSquaresL1)
    base.m_rows, base.n_features, base._w_host = 40, 7, None
    with pytest.raises(ValueError, match="needs gap_tol"):
        path.l1_cv_lockstep(base, [0.1], gap_tol=None)
    with pytest.raises(ValueError, match="screen=True"):
        path.l1_cv_lockstep(base, [0.1], screen=True)
    with pytest.raises(ValueError, match="at least one value"):
        path.l1_cv_lockstep(base, [])
    with pytest.raises(ValueError, match="at most 16 folds"):
        path.l1_cv_lockstep(base, [0.1], folds=17)
    assert "certifies every fold" in path.l1_cv_lockstep.__doc__
    del p


def test_the_classes_are_exported_and_documented():
    for cls in MR:
        assert issubclass(cls, problems.NativeProblem) and cls.n_responses == 1 and cls.taylor_remainder is False
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "MultiResponseLeastSquaresL1(A, B, lam" in readme and "MultiResponseLogisticL1" in readme and "l1_cv_lockstep" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.5m" in design and "zf_mr_rows_kernel" in design
