"""CPU: the interface of the duality-gap feature without a GPU - header and ctypes table, the argument checks of the new
entry points (before anything touches a device or is dereferenced), and the keyword checks of gap_tol / gap_every."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import evaldesc as E
from conftest import ROOT
from zfista_amd import _lib, minimize_proximal_gradient

NEW = ("zf_margins_gap", "zf_solver_duality_gap")


def test_header_and_ctypes_table_declare_the_new_entry_points():
    src = open(os.path.join(ROOT, "include", "zfista_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.zf_abi_version() == 7 and lib.zf_sizeof_control() == 424, "no struct change"
    assert len(_lib.SIGNATURES["zf_margins_gap"][1]) == 5
    assert _lib.ACCEPT_MODES == {"reference": 0, "resolved": 1, "remainder": 2}


def test_new_entry_points_refuse_null_and_short_arguments():
    lib = _lib.load()
    out = np.full(8, -7.0)
    P = C.c_void_p(_lib.ptr(out))
    assert E.gap(E.dense(None), P, P, 8) == -2 and b"zf_margins_gap" in lib.zf_last_error()
    assert E.gap(E.dense(P, m_rows=0), P, P, 8) == -2
    assert E.gap(E.dense(P), P, P, 7) == -2 and b"fewer than 8" in lib.zf_last_error()
    assert E.gap(E.dense(P, scale=0.0), P, P, 8) == -2 and b"scale > 0" in lib.zf_last_error()
    assert E.gap(E.dense(P, lam=-0.1, loss=1), P, P, 8) == -2 and b"lam >= 0" in lib.zf_last_error()
    assert E.gap(E.dense(_lib.ptr(out) + 8), P, P, 8) == -2 and b"aligned" in lib.zf_last_error()
    assert E.gap(E.sparse(None), P, P, 8) == -2 and b"zf_margins_gap" in lib.zf_last_error()
    assert E.gap(E.sparse(P), P, P, 3) == -2 and b"fewer than 8" in lib.zf_last_error()
    assert lib.zf_solver_duality_gap(None, P, 8) == -2 and b"zf_solver_duality_gap" in lib.zf_last_error()
    # a short buffer is refused before the handle is read or written through: a patterned region stands in for it
    dummy = (C.c_ubyte * (1 << 20))()
    C.memset(dummy, 0xA5, len(dummy))
    assert lib.zf_solver_duality_gap(C.c_void_p(C.addressof(dummy)), P, 7) == -2 and b"fewer than 8" in lib.zf_last_error()
    assert (np.frombuffer(dummy, dtype=np.uint8) == 0xA5).all() and (out == -7.0).all()


_PLAIN = (lambda x: 0.5 * float(x @ x), lambda x: 0.0, lambda x: x, lambda w, x: x)


def test_gap_tol_with_plain_callables_raises():
    with pytest.raises(ValueError, match="gap_tol is not available"):
        minimize_proximal_gradient(*_PLAIN, np.ones(3), gap_tol=1e-6)
    with pytest.raises(ValueError, match="gap_tol is not available"):
        minimize_proximal_gradient(*_PLAIN, np.ones(3), gap_tol=0.0, gap_every=1)


@pytest.mark.parametrize("kw", [dict(gap_tol=-1e-9), dict(gap_tol=float("nan")), dict(gap_every=0), dict(gap_every=-3),
                                dict(gap_every=2.5), dict(gap_tol=1e-3, gap_every=0)])
def test_bad_gap_keywords_raise(kw):
    with pytest.raises(ValueError, match="gap_tol|gap_every"):
        minimize_proximal_gradient(*_PLAIN, np.ones(3), **kw)


def test_the_keywords_are_keyword_only_and_the_classes_carry_the_methods():
    import inspect

    from zfista_amd import path, problems

    sig = inspect.signature(minimize_proximal_gradient)
    assert sig.parameters["gap_tol"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["gap_tol"].default is None
    assert sig.parameters["gap_every"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["gap_every"].default == 16
    for cls in (problems.LeastSquaresL1, problems.SparseLeastSquaresL1, problems.LogisticL1, problems.SparseLogisticL1):
        for name in ("duality_gap", "lam_max", "with_lam"):
            assert callable(getattr(cls, name)), (cls, name)
    assert not hasattr(problems.DiagQuadL1, "duality_gap") and not hasattr(problems.BlurHaarL1, "duality_gap")
    assert [p for p in inspect.signature(path.l1_path).parameters][:4] == ["problem", "lams", "x0", "gap_tol"]
    with pytest.raises(ValueError):
        path.l1_path(object(), [1.0])
