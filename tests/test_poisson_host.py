"""CPU: the interface of the Poisson classes without a GPU - header and ctypes table (the struct sizes as they
were, no problem kind), the argument checks of the new entry points before any device is touched, the ValueErrors of the host
classes, the siblings, and the refusals of screening."""
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

NEW = ("zf_solver_set_poisson", "zf_margins_eval", "zf_margins_gap")


def test_header_and_ctypes_table_declare_the_new_entry_points_and_nothing_else_moved():
    src = open(os.path.join(ROOT, "include", "zfista_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(zf_[A-Za-z0-9_]+)\s*\(", src))), "header = ctypes table"
    assert re.search(r"ZF_LOSS_POISSON\s*=\s*3\b", src) and _lib.ZF_LOSS_POISSON == 3
    assert lib.zf_abi_version() == 7 and lib.zf_sizeof_control() == 424 == C.sizeof(_lib.Control)
    assert C.sizeof(_lib.ProblemDesc) == 128 and C.sizeof(_lib.Options) == 64, "additive exports only: no struct field"
    assert "poisson" not in [f[0] for f in _lib.ProblemDesc._fields_]
    kinds = sorted(v for k, v in vars(_lib).items() if k.startswith("ZF_PROBLEM_"))
    assert max(kinds) == 6, "no new problem kind"
    assert _lib.SIGNATURES["zf_solver_set_poisson"][1] == [C.c_void_p]


def test_new_entry_points_refuse_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    out = np.full(12, -7.0)
    P = C.c_void_p(_lib.ptr(out))
    odd = C.c_void_p(_lib.ptr(out) + 8)   # not 16-byte aligned
    assert _lib.ptr(out) % 16 == 0
    f = C.c_double(-7.0)
    assert lib.zf_solver_set_poisson(None) == -2 and b"zf_solver_set_poisson" in lib.zf_last_error()
    # f / grad: null pointers, bad sizes, a misaligned A - with and without the weights
    PO = _lib.ZF_LOSS_POISSON
    for w in (None, P):
        D = lambda **kw: E.dense(P, **{**dict(loss=PO, w=w, scale=1.0), **kw})    # noqa: E731
        S = lambda **kw: E.sparse(P, **{**dict(loss=PO, w=w, scale=1.0), **kw})   # noqa: E731
        assert E.point(D(A=None), P, C.byref(f)) == -2 and b"zf_margins_eval" in lib.zf_last_error()
        assert E.point(D(b=None), P, C.byref(f)) == -2
        assert E.point(D(), None, C.byref(f)) == -2
        assert E.point(D(), P, None) == -2
        assert E.point(D(m_rows=0), P, C.byref(f)) == -2
        assert E.point(D(n=0), P, C.byref(f)) == -2
        assert E.point(D(A=odd), P, C.byref(f)) == -2 and b"aligned" in lib.zf_last_error()
        assert E.point(S(spmat=None), P, C.byref(f)) == -2 and b"zf_margins_eval" in lib.zf_last_error()
        # the certificate
        assert E.gap(D(A=None), P, P, 10) == -2 and b"zf_margins_gap" in lib.zf_last_error()
        assert E.gap(D(), None, P, 10) == -2
        assert E.gap(D(), P, None, 10) == -2
        assert E.gap(D(m_rows=-3), P, P, 10) == -2
        assert E.gap(D(A=odd), P, P, 10) == -2 and b"aligned" in lib.zf_last_error()
        assert E.gap(S(spmat=None), P, P, 10) == -2 and b"zf_margins_gap" in lib.zf_last_error()
        for short in (0, 3, 7):
            assert E.gap(D(), P, P, short) == -2 and b"fewer than 8" in lib.zf_last_error()
            assert E.gap(S(), P, P, short) == -2 and b"fewer than 8" in lib.zf_last_error()
        for bad in (-1e-9, float("inf"), float("nan")):
            assert E.gap(D(l2=bad), P, P, 10) == -2 and b"l2" in lib.zf_last_error()
            assert E.gap(S(l2=bad), P, P, 10) == -2 and b"l2" in lib.zf_last_error()
        assert E.gap(D(lam=-0.1), P, P, 10) == -2 and b"lam >= 0" in lib.zf_last_error()
        assert E.gap(D(scale=0.0), P, P, 10) == -2 and b"scale > 0" in lib.zf_last_error()
    # every unknown loss code is refused, with weights too (the message names the four codes)
    for bad_loss in (-1, 4, 7):
        for d in (E.dense(P, w=P, loss=bad_loss, delta=1.0), E.sparse(P, w=P, loss=bad_loss, delta=1.0)):
            assert E.point(d, P, C.byref(f)) == -2 and b"ZF_LOSS_POISSON" in lib.zf_last_error()
            assert E.gap(d, P, P, 10) == -2 and b"ZF_LOSS_POISSON" in lib.zf_last_error()
    assert (out == -7.0).all() and f.value == -7.0


class _T:   # what the host logic reads of a device tensor
    def data_ptr(self):
        return 4096

    def numel(self):
        return 5


def _standin(cls, l2=0.0):
    """A problem object without a device: the attributes the host logic reads."""
    p = object.__new__(cls)
    p.A = p.b = _T()
    p.lam, p.scale, p.box, p.m_rows, p.n_features, p.group = 0.3, 1.0, (-np.inf, np.inf), 5, 7, None
    p._norms = problems._ColumnNorms()
    p._spmat = type("H", (), {"value": C.c_void_p(8192)})()
    if l2:
        p.l2 = l2
    return p


POISSON = [problems.PoissonL1, problems.SparsePoissonL1]


def test_the_constructors_refuse_before_anything_touches_a_device():
    import scipy.sparse as sp

    for cls, A in ((problems.PoissonL1, np.eye(2)), (problems.SparsePoissonL1, sp.eye(2, format="csr"))):
        for bad in ([1.0, -1.0], [np.nan, 0.0], [np.inf, 2.0], [-0.5, 0.5]):
            with pytest.raises(ValueError, match="counts b must be finite and >= 0"):
                cls(A, np.array(bad), 0.1)
        with pytest.raises(ValueError, match="group="):
            cls(A, np.zeros(2), 0.1, group=object())
        with pytest.raises(ValueError, match="l2 must be finite"):
            cls(A, np.zeros(2), 0.1, l2=-1.0)
        with pytest.raises(ValueError, match="sample_weight"):
            cls(A, np.zeros(2), 0.1, sample_weight=np.array([1.0, -1.0]))
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[:7] == ["self", "A", "b", "lam", "scale", "bounds", "l2"]
        assert params["scale"].default == 1.0 and params["l2"].default == 0.0 and params["bounds"].default is None
        assert params["sample_weight"].kind is inspect.Parameter.KEYWORD_ONLY
    assert np.array_equal(problems._check_counts(np.array([0, 3, 2])), [0, 3, 2]), "integer arrays are counts too"
    assert problems._check_counts(np.array([0.5, 0.0]))[0] == 0.5, "a rate count / exposure need not be an integer"


@pytest.mark.parametrize("cls", POISSON)
def test_the_classes_are_least_squares_kinds_with_poisson_in_the_descriptor(cls):
    p = _standin(cls)
    base = problems.LeastSquaresL1 if cls is problems.PoissonL1 else problems.SparseLeastSquaresL1
    assert cls.kind == base.kind and cls.kind in (2, 4), "no new problem kind"
    assert cls._loss == _lib.ZF_LOSS_POISSON == 3
    assert issubclass(cls, problems._GapMixin) and issubclass(cls, problems._DenseMarginsL1 if cls.kind == 2 else problems._SparseMarginsL1)
    fields, _ = p._descriptor()
    assert fields["poisson"] is True and fields["kind"] == cls.kind and "l2" not in fields and "huber_delta" not in fields
    fields, _ = p.with_penalty(0.3, 0.25)._descriptor()
    assert fields["poisson"] is True and fields["l2"] == 0.25
    sib = _standin(base)
    sib.shard = "columns"
    assert "poisson" not in sib._descriptor()[0], "a least-squares problem hands the engine what it handed it before"
    d = p._eval_desc()
    assert p.has_duality_gap and (d.loss, d.delta, d.w, d.p) == (_lib.ZF_LOSS_POISSON, 0.0, None, None)
    assert (bool(d.A), bool(d.spmat)) == (cls.kind == 2, cls.kind == 4) and not d.A32


@pytest.mark.parametrize("cls", POISSON)
def test_siblings_share_the_matrix(cls):
    p = _standin(cls)
    q = p.with_lam(0.2)
    assert type(q) is cls and (q.lam, q.l2) == (0.2, 0.0) and p.lam == 0.3
    assert q.A is p.A and q.b is p.b and q._spmat is p._spmat, "same holder: nothing is uploaded"
    r = q.with_penalty(0.1, 0.05)
    assert (r.lam, r.l2) == (0.1, 0.05) and r.A is p.A and r.with_lam(0.4).l2 == 0.05
    assert problems.match_native(*q.callbacks()) is q, "the bound methods of a Poisson problem are recognised"


@pytest.mark.parametrize("cls", POISSON)
def test_the_remainder_and_resolved_acceptances_are_refused(cls):
    p = _standin(cls)
    assert not getattr(p, "taylor_remainder", False) and not getattr(p, "separable", False)
    with pytest.raises(ValueError, match="acceptance='remainder' needs a native least-squares problem"):
        minimize_proximal_gradient(*p.callbacks(), np.zeros(7), acceptance="remainder")
    with pytest.raises(ValueError, match="acceptance='resolved' needs a separable native problem"):
        minimize_proximal_gradient(*p.callbacks(), np.zeros(7), acceptance="resolved")


@pytest.mark.parametrize("cls", POISSON)
def test_screening_is_refused_and_the_gap_with_a_box(cls):
    p = _standin(cls)
    assert p._gap_refusal() is None, "the certificate exists"
    for call in (lambda: p.column_norms(), lambda: p.screen(np.zeros(7)), lambda: p.restrict(np.arange(3)),
                 lambda: screening.solve_screened(p, np.zeros(7), 1e-6), lambda: path.l1_path(p, [0.1], screen=True)):
        with pytest.raises(ValueError, match="globally Lipschitz"):
            call()
    boxed = _standin(cls)
    boxed.box = (-1.0, 1.0)
    for call in (lambda: boxed.duality_gap(np.zeros(7)),
                 lambda: minimize_proximal_gradient(*boxed.callbacks(), np.zeros(7), gap_tol=1e-6)):
        with pytest.raises(ValueError, match="bounds are set"):
            call()
    with pytest.raises(ValueError, match="n_features"):
        _standin(cls).duality_gap(np.zeros(6))


def test_the_classes_are_exported_and_documented():
    for name in ("PoissonL1", "SparsePoissonL1"):
        assert inspect.isclass(getattr(problems, name)) and issubclass(getattr(problems, name), problems.NativeProblem)
        assert "exposure" in getattr(problems, "PoissonL1").__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "PoissonL1(A, b, lam" in readme and "SparsePoissonL1" in readme and "exposure" in readme
    assert "nine device-resident" in readme.lower() or "nine device-resident" in open(os.path.join(ROOT, "DESIGN.md")).read().lower()
