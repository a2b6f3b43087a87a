"""CPU: the interface of the Huber classes without a GPU - header and ctypes table (the struct sizes as they
were, no problem kind), the argument checks of the new entry points before any device is touched, the ValueErrors of the host
classes, the siblings, and that the product does not import the oracle."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import evaldesc as E
from conftest import ROOT
from zfista_amd import _lib, path, problems, screening
from zfista_amd.proximal_gradient import minimize_proximal_gradient

NEW = ("zf_solver_set_huber", "zf_margins_eval", "zf_margins_gap", "zf_margins_screen")
HUBER_LOSS = dict(loss=_lib.ZF_LOSS_HUBER, delta=1.0)
BAD_DELTAS = (0.0, -1.0, float("inf"), float("-inf"), float("nan"))


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
    fields = [f[0] for f in _lib.ProblemDesc._fields_]
    assert "huber_delta" not in fields and "delta" not in fields
    kinds = sorted(v for k, v in vars(_lib).items() if k.startswith("ZF_PROBLEM_"))
    assert max(kinds) == 6, "no new problem kind"
    assert "delta" in [f[0] for f in _lib.EvalDesc._fields_], "delta is a field of the evaluation descriptor"


def test_new_entry_points_refuse_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    out = np.full(12, -7.0)
    P = C.c_void_p(_lib.ptr(out))
    f = C.c_double(-7.0)
    assert lib.zf_solver_set_huber(None, 1.0) == -2 and b"zf_solver_set_huber" in lib.zf_last_error()
    # f / grad
    H = HUBER_LOSS
    assert E.point(E.dense(None, **H), P, C.byref(f)) == -2 and b"zf_margins_eval" in lib.zf_last_error()
    assert E.point(E.dense(P, m_rows=0, **H), P, C.byref(f)) == -2
    assert E.point(E.sparse(None, **H), P, C.byref(f)) == -2 and b"zf_margins_eval" in lib.zf_last_error()
    for bad in BAD_DELTAS:
        B = dict(loss=_lib.ZF_LOSS_HUBER, delta=bad)
        assert E.point(E.dense(P, **B), P, C.byref(f)) == -2 and b"delta" in lib.zf_last_error()
        assert E.point(E.sparse(P, **B), P, C.byref(f)) == -2 and b"delta" in lib.zf_last_error()
        assert E.gap(E.dense(P, **B), P, P, 10) == -2 and b"delta" in lib.zf_last_error()
        assert E.gap(E.sparse(P, **B), P, P, 10) == -2 and b"delta" in lib.zf_last_error()
        assert E.screen(E.dense(P, **B), P, P, 12, P, P, 0, 0, P, P) == -2 and b"delta" in lib.zf_last_error()
        assert E.screen(E.sparse(P, **B), P, P, 12, P, P, 2, 3, P, P) == -2 and b"delta" in lib.zf_last_error()
    # the certificate
    assert E.gap(E.dense(None, **H), P, P, 10) == -2 and b"zf_margins_gap" in lib.zf_last_error()
    assert E.gap(E.dense(P, **H), P, P, 7) == -2 and b"fewer than 8" in lib.zf_last_error()
    assert E.gap(E.sparse(None, **H), P, P, 10) == -2
    assert E.gap(E.sparse(P, **H), P, P, 3) == -2 and b"fewer than 8" in lib.zf_last_error()
    for bad in (-1e-9, float("inf"), float("nan")):
        assert E.gap(E.dense(P, l2=bad, **H), P, P, 10) == -2 and b"l2" in lib.zf_last_error()
        assert E.gap(E.sparse(P, l2=bad, **H), P, P, 10) == -2 and b"l2" in lib.zf_last_error()
    assert E.gap(E.dense(P, lam=-0.1, **H), P, P, 10) == -2 and b"lam >= 0" in lib.zf_last_error()
    assert E.gap(E.dense(P, scale=0.0, **H), P, P, 10) == -2 and b"scale > 0" in lib.zf_last_error()
    # the screen
    assert E.screen(E.dense(None, **H), P, P, 12, P, P, 0, 0, P, P) == -2
    assert E.screen(E.dense(P, **H), P, P, 11, P, P, 0, 0, P, P) == -2 and b"fewer than 12" in lib.zf_last_error()
    assert E.screen(E.dense(P, **H), P, P, 12, None, P, 0, 0, P, P) == -2 and b"null" in lib.zf_last_error()
    assert E.screen(E.sparse(None, **H), P, P, 12, P, P, 2, 3, P, P) == -2
    assert E.screen(E.sparse(P, **H), P, P, 12, P, P, -1, 3, P, P) == -2 and b">= 0" in lib.zf_last_error()
    assert (out == -7.0).all() and f.value == -7.0


class _T:   # what the host logic reads of a device tensor
    def data_ptr(self):
        return 4096


def _standin(cls, l2=0.0, delta=0.75):
    """A problem object without a device: the attributes the host logic reads."""
    p = object.__new__(cls)
    p.A = p.b = _T()
    p.lam, p.scale, p.box, p.m_rows, p.n_features, p.group = 0.3, 0.5, (-np.inf, np.inf), 5, 7, None
    p._norms = problems._ColumnNorms()
    p._spmat = type("H", (), {"value": C.c_void_p(8192)})()
    p.delta = delta
    if l2:
        p.l2 = l2
    return p


HUBER = [problems.HuberL1, problems.SparseHuberL1]


def test_the_constructors_refuse_before_anything_touches_a_device():
    import scipy.sparse as sp

    for cls, A in ((problems.HuberL1, np.eye(2)), (problems.SparseHuberL1, sp.eye(2, format="csr"))):
        for bad in BAD_DELTAS:
            with pytest.raises(ValueError, match="delta must be finite and > 0"):
                cls(A, np.zeros(2), 0.1, bad)
        with pytest.raises(ValueError, match="group="):
            cls(A, np.zeros(2), 0.1, 1.0, group=object())
        with pytest.raises(ValueError, match="l2 must be finite"):
            cls(A, np.zeros(2), 0.1, 1.0, l2=-1.0)
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[:8] == ["self", "A", "b", "lam", "delta", "scale", "bounds", "l2"]
        assert params["scale"].default == 0.5 and params["l2"].default == 0.0 and params["bounds"].default is None
        assert params["delta"].default is inspect.Parameter.empty
    assert problems._check_delta(np.float32(0.5)) == 0.5


@pytest.mark.parametrize("cls", HUBER)
def test_the_classes_are_least_squares_kinds_with_huber_delta_in_the_descriptor(cls):
    p = _standin(cls)
    base = problems.LeastSquaresL1 if cls is problems.HuberL1 else problems.SparseLeastSquaresL1
    assert cls.kind == base.kind and cls.kind in (2, 4), "no new problem kind"
    assert issubclass(cls, problems._GapMixin) and issubclass(cls, problems._DenseMarginsL1 if cls.kind == 2 else problems._SparseMarginsL1)
    fields, _ = p._descriptor()
    assert fields["huber_delta"] == 0.75 and fields["kind"] == cls.kind and "l2" not in fields
    fields, _ = p.with_penalty(0.3, 0.25)._descriptor()
    assert fields["huber_delta"] == 0.75 and fields["l2"] == 0.25
    sib = _standin(base)
    sib.shard = "columns"
    assert "huber_delta" not in sib._descriptor()[0], "a least-squares problem hands the engine what it handed it before"
    assert not hasattr(_lib.ProblemDesc(), "huber_delta")
    d = p._eval_desc()
    assert p.has_duality_gap and (d.loss, d.delta) == (_lib.ZF_LOSS_HUBER, 0.75)


@pytest.mark.parametrize("cls", HUBER)
def test_siblings_share_the_matrix_and_keep_delta(cls):
    p = _standin(cls)
    q = p.with_lam(0.2)
    assert type(q) is cls and (q.lam, q.delta, q.l2) == (0.2, 0.75, 0.0) and p.lam == 0.3
    assert q.A is p.A and q.b is p.b and q._spmat is p._spmat and q._norms is p._norms, "same holder: nothing is uploaded"
    r = q.with_penalty(0.1, 0.05)
    assert (r.lam, r.l2, r.delta) == (0.1, 0.05, 0.75) and r.A is p.A and r.with_lam(0.4).l2 == 0.05
    with pytest.raises(ValueError, match="l2 must be finite"):
        p.with_penalty(0.1, -1.0)
    assert problems.match_native(*q.callbacks()) is q, "the bound methods of a Huber problem are recognised"
    assert problems.match_native(q.f, p.g, q.jac_f, q.prox_wsum_g) is None


@pytest.mark.parametrize("cls", HUBER)
def test_the_remainder_and_resolved_acceptances_are_refused(cls, monkeypatch):
    p = _standin(cls)
    assert not getattr(p, "taylor_remainder", False) and not getattr(p, "separable", False)
    with pytest.raises(ValueError, match="acceptance='remainder' needs a native least-squares problem"):
        minimize_proximal_gradient(*p.callbacks(), np.zeros(7), acceptance="remainder")
    with pytest.raises(ValueError, match="acceptance='resolved' needs a separable native problem"):
        minimize_proximal_gradient(*p.callbacks(), np.zeros(7), acceptance="resolved")


@pytest.mark.parametrize("cls", HUBER)
def test_screening_is_refused_with_l2_and_the_gap_with_a_box(cls):
    p = _standin(cls, l2=0.1)
    assert p._gap_refusal() is None, "the certificate exists"
    for call in (lambda: p.screen(np.zeros(7)), lambda: screening.solve_screened(p, np.zeros(7), 1e-6),
                 lambda: path.l1_path(p, [0.1], screen=True), lambda: path.l1_path(_standin(cls), [0.1], screen=True, l2=0.2)):
        with pytest.raises(ValueError, match="l2 > 0"):
            call()
    boxed = _standin(cls)
    boxed.box = (-1.0, 1.0)
    for call in (lambda: boxed.duality_gap(np.zeros(7)), lambda: boxed.screen(np.zeros(7)), lambda: boxed.restrict(np.arange(3)),
                 lambda: minimize_proximal_gradient(*boxed.callbacks(), np.zeros(7), gap_tol=1e-6)):
        with pytest.raises(ValueError, match="bounds are set"):
            call()
    with pytest.raises(ValueError, match="n_features"):
        _standin(cls).duality_gap(np.zeros(6))


def test_the_classes_are_exported_beside_the_other_problem_classes():
    for name in ("HuberL1", "SparseHuberL1", "LeastSquaresL1", "SparseLogisticL1"):
        assert inspect.isclass(getattr(problems, name)) and issubclass(getattr(problems, name), problems.NativeProblem)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "HuberL1(A, b, lam, delta" in readme and "SparseHuberL1" in readme


def test_the_product_does_not_import_the_oracle():
    code = ("import sys; import zfista_amd, zfista_amd.problems, zfista_amd.path, zfista_amd.screening, zfista_amd.engine; "
            "bad = [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.') or m.endswith('_cases')]; "
            "assert not bad, bad")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    for name in ("problems.py", "engine.py", "path.py", "screening.py", "_lib.py"):
        src = open(os.path.join(ROOT, "zfista_amd", name)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), name
