"""CPU: the interface of the elastic-net feature without a GPU - header and ctypes table (the struct sizes as they were), the argument checks of the new entry points, the ValueErrors of the host classes, and the siblings."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import evaldesc as E
from conftest import ROOT
from zfista_amd import _lib, path, problems, screening

NEW = ("zf_solver_set_l2", "zf_margins_gap", "zf_host_prox_enet_box", "zf_host_enet_g")


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
    assert "l2" not in [f[0] for f in _lib.ProblemDesc._fields_] and "l2" in [f[0] for f in _lib.EvalDesc._fields_]


def test_new_entry_points_refuse_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    out = np.full(10, -7.0)
    P = C.c_void_p(_lib.ptr(out))
    assert lib.zf_solver_set_l2(None, 0.1) == -2 and b"zf_solver_set_l2" in lib.zf_last_error()
    assert E.gap(E.dense(None, l2=0.1), P, P, 10) == -2 and b"zf_margins_gap" in lib.zf_last_error()
    assert E.gap(E.dense(P, l2=0.1), P, P, 7) == -2 and b"fewer than 8" in lib.zf_last_error()
    for bad in (-1e-9, float("inf"), float("nan")):
        assert E.gap(E.dense(P, l2=bad), P, P, 10) == -2 and b"l2" in lib.zf_last_error()
        assert E.gap(E.sparse(P, l2=bad), P, P, 10) == -2 and b"l2" in lib.zf_last_error()
    assert E.gap(E.dense(P, lam=-0.1, l2=0.1, loss=1), P, P, 10) == -2 and b"lam >= 0" in lib.zf_last_error()
    assert E.gap(E.sparse(None, l2=0.1), P, P, 10) == -2
    assert E.gap(E.sparse(P, l2=0.1), P, P, 3) == -2 and b"fewer than 8" in lib.zf_last_error()
    assert lib.zf_host_prox_enet_box(None, P, 0.1, 1.0, -1.0, 1.0, 4) == -2 and lib.zf_host_enet_g(None, 4, 0.1, 0.1, None) == -2
    assert (out == -7.0).all()


class _T:   # what the host logic reads of a device tensor
    def data_ptr(self):
        return 4096


def _standin(cls, l2=0.0):
    """A problem object without a device: the attributes the host logic reads."""
    p = object.__new__(cls)
    p.A = p.b = _T()
    p.lam, p.scale, p.box, p.m_rows, p.n_features, p.group = 0.3, 0.5, (-np.inf, np.inf), 5, 7, None
    p._norms = problems._ColumnNorms()
    p._spmat = object()
    if l2:
        p.l2 = l2
    return p


def test_l2_is_validated():
    for bad in (-1e-12, float("inf"), float("-inf"), float("nan")):
        with pytest.raises(ValueError, match="l2 must be finite and >= 0"):
            problems._check_l2(bad)
        with pytest.raises(ValueError, match="l2 must be finite and >= 0"):
            _standin(problems.LogisticL1).with_penalty(0.1, bad)
    with pytest.raises(ValueError, match="group="):
        problems._check_l2(0.5, group=object())
    assert problems._check_l2(0.0, group=object()) == 0.0 and problems._check_l2(np.float32(0.5)) == 0.5
    # the constructors check l2 before anything touches a device
    with pytest.raises(ValueError, match="l2 must be finite"):
        problems.LeastSquaresL1(np.eye(2), np.zeros(2), 0.1, l2=-1.0)
    with pytest.raises(ValueError, match="group="):
        problems.LeastSquaresL1(np.eye(2), np.zeros(2), 0.1, l2=0.5, group=object())
    for cls in (problems.LeastSquaresL1, problems.SparseLeastSquaresL1):
        assert inspect.signature(cls.__init__).parameters["l2"].default == 0.0


@pytest.mark.parametrize("cls", [problems.LeastSquaresL1, problems.SparseLeastSquaresL1, problems.LogisticL1, problems.SparseLogisticL1])
def test_siblings_share_the_matrix_and_carry_l2(cls):
    p = _standin(cls)
    assert p.l2 == 0.0
    q = p.with_penalty(0.2, 0.05)
    assert type(q) is cls and (q.lam, q.l2) == (0.2, 0.05) and (p.lam, p.l2) == (0.3, 0.0)
    assert q.A is p.A and q.b is p.b and q._spmat is p._spmat and q._norms is p._norms, "same holder: nothing is uploaded"
    r = q.with_lam(0.1)
    assert (r.lam, r.l2) == (0.1, 0.05) and r.A is p.A, "with_lam keeps l2"
    assert q.with_penalty(0.2, 0.0).l2 == 0.0
    assert problems.match_native(*q.callbacks()) is q, "the bound methods of an elastic-net problem are recognised"
    assert problems.match_native(q.f, p.g, q.jac_f, q.prox_wsum_g) is None


def test_the_descriptor_names_l2_only_when_it_is_set():
    p = _standin(problems.LogisticL1)
    fields, _ = p._descriptor()
    assert "l2" not in fields, "an l1 problem hands the engine what it handed it before"
    fields, _ = p.with_penalty(0.3, 0.25)._descriptor()
    assert fields["l2"] == 0.25 and fields["lam"] == 0.3
    d = _lib.ProblemDesc()
    assert not hasattr(d, "l2")


def test_screening_is_refused_with_l2():
    p = _standin(problems.SparseLeastSquaresL1, l2=0.1)
    assert p._gap_refusal() is None, "the certificate exists"
    for call in (lambda: p.screen(np.zeros(7)), lambda: screening.solve_screened(p, np.zeros(7), 1e-6),
                 lambda: path.l1_path(p, [0.1], screen=True), lambda: path.l1_path(_standin(problems.LogisticL1), [0.1], screen=True, l2=0.2)):
        with pytest.raises(ValueError, match="l2 > 0"):
            call()
    with pytest.raises(ValueError, match="one value per lam"):
        path.l1_path(_standin(problems.LogisticL1), [0.3, 0.2, 0.1], l2=[0.1, 0.2])
    with pytest.raises(ValueError, match="l2 must be finite"):
        path.l1_path(_standin(problems.LogisticL1), [0.3], l2=-1.0)
    assert list(inspect.signature(path.l1_path).parameters)[:6] == ["problem", "lams", "x0", "gap_tol", "screen", "l2"]


def test_duality_gap_fields():
    g = problems.DualityGap(np.arange(8.0))
    assert (g.rows_gap, g.g_l2, g.ridge_gap) == (7.0, 0.0, 0.0)
    g = problems.DualityGap(np.arange(10.0))
    assert (g.primal, g.rows_gap, g.g_l2, g.ridge_gap) == (0.0, 7.0, 8.0, 9.0) and "ridge_gap=" in repr(g)
