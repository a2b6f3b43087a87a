"""CPU: the interface of per-column penalty factors without a GPU - header and ctypes table (the struct sizes
as they were), the argument checks of the new entry points and of the two host functions before any device is touched, every
ValueError of the host classes, the siblings, and add_intercept."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
import evaldesc as E
from zfista_amd import _lib, path, problems, screening
from zfista_amd.proximal_gradient import minimize_proximal_gradient

NEW = ("zf_solver_set_penalty_factors", "zf_margins_gap", "zf_host_prox_pf_box", "zf_host_pf_g")
EIGHT = [problems.LeastSquaresL1, problems.SparseLeastSquaresL1, problems.LogisticL1, problems.SparseLogisticL1, problems.HuberL1,
         problems.SparseHuberL1, problems.PoissonL1, problems.SparsePoissonL1]
WITH_KEYWORD = [c for c in EIGHT if "Logistic" not in c.__name__]


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
    assert "penalty_factors" not in [f[0] for f in _lib.ProblemDesc._fields_]
    assert "p" in [f[0] for f in _lib.EvalDesc._fields_], "the factors are a field of the evaluation descriptor"
    assert len(_lib.SIGNATURES["zf_host_prox_pf_box"][1]) == len(_lib.SIGNATURES["zf_host_prox_l1_box"][1]) + 1


def test_new_entry_points_refuse_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    out = np.full(12, -7.0)
    P = C.c_void_p(_lib.ptr(out))
    s = C.c_double(-7.0)
    assert lib.zf_solver_set_penalty_factors(None, P) == -2 and b"zf_solver_set_penalty_factors" in lib.zf_last_error()
    # the certificate: a null pointer in every place but the weights (NULL: unweighted), short buffers, scale, lam, the loss, delta
    for field in ("A", "b"):
        assert E.gap(E.dense(P, w=P, p=P, **{field: None}), P, P, 8) == -2 and b"zf_margins_gap" in lib.zf_last_error(), field
    for field in ("spmat", "b"):
        assert E.gap(E.sparse(P, w=P, p=P, **{field: None}), P, P, 8) == -2 and b"zf_margins_gap" in lib.zf_last_error(), field
    for d in (E.dense(P, w=P, p=P), E.sparse(P, w=P, p=P)):
        assert E.gap(d, None, P, 8) == -2 and b"zf_margins_gap" in lib.zf_last_error()
        assert E.gap(d, P, None, 8) == -2 and b"zf_margins_gap" in lib.zf_last_error()
    assert E.gap(E.dense(P, p=P, m_rows=0), P, P, 8) == -2
    assert E.gap(E.dense(P, p=P, n=0), P, P, 8) == -2
    for short in (0, 3, 7):
        assert E.gap(E.dense(P, p=P), P, P, short) == -2 and b"fewer than 8" in lib.zf_last_error()
        assert E.gap(E.sparse(P, p=P, loss=1), P, P, short) == -2 and b"fewer than 8" in lib.zf_last_error()
    for bad_loss in (-1, 4, 7):
        assert E.gap(E.dense(P, p=P, loss=bad_loss, delta=1.0), P, P, 8) == -2 and b"ZF_LOSS_" in lib.zf_last_error()
        assert E.gap(E.sparse(P, p=P, loss=bad_loss, delta=1.0), P, P, 8) == -2 and b"ZF_LOSS_" in lib.zf_last_error()
    for bad in (0.0, -1.0, float("inf"), float("nan")):   # delta: checked for Huber's loss only
        assert E.gap(E.dense(P, p=P, loss=2, delta=bad), P, P, 8) == -2 and b"delta" in lib.zf_last_error()
        assert E.gap(E.sparse(P, p=P, loss=2, delta=bad), P, P, 8) == -2 and b"delta" in lib.zf_last_error()
    assert E.gap(E.dense(P, p=P, lam=-0.1), P, P, 8) == -2 and b"lam >= 0" in lib.zf_last_error()
    assert E.gap(E.dense(P, p=P, scale=0.0), P, P, 8) == -2 and b"scale > 0" in lib.zf_last_error()
    odd = C.c_void_p(_lib.ptr(out) + 8)
    assert E.gap(E.dense(odd, p=P), P, P, 8) == -2 and b"16-byte" in lib.zf_last_error()
    for d in (E.dense(P, p=P, l2=0.25), E.sparse(P, p=P, l2=0.25)):   # the ridge term would need the factors too
        assert E.gap(d, P, P, 10) == -2 and b"penalty factors and l2" in lib.zf_last_error()
    # the two host functions: null pointers, a negative length; n = 0 is legal and touches nothing
    for k in (0, 1, 2):
        args = [P, P, P, 0.1, -1.0, 1.0, 4]
        args[k] = None
        assert lib.zf_host_prox_pf_box(*args) == -2 and b"zf_host_prox_pf_box" in lib.zf_last_error(), k
    assert lib.zf_host_prox_pf_box(P, P, P, 0.1, -1.0, 1.0, -1) == -2
    assert lib.zf_host_prox_pf_box(P, P, P, 0.1, -1.0, 1.0, 0) == 0
    for args in ([None, P, 4, 0.1, C.byref(s)], [P, None, 4, 0.1, C.byref(s)], [P, P, 4, 0.1, None], [P, P, -1, 0.1, C.byref(s)]):
        assert lib.zf_host_pf_g(*args) == -2 and b"zf_host_pf_g" in lib.zf_last_error()
    assert (out == -7.0).all() and s.value == -7.0, "nothing was written"
    assert lib.zf_host_pf_g(P, P, 0, 0.1, C.byref(s)) == 0 and s.value == 0.0


class _T:   # what the host logic reads of a device tensor
    def __init__(self, p=4096):
        self.p = p

    def data_ptr(self):
        return self.p


def _standin(cls, n=7):
    """A problem object without a device: the attributes the host logic reads."""
    p = object.__new__(cls)
    p.A = p.b = _T()
    p.lam, p.scale, p.box, p.m_rows, p.n_features, p.group = 0.3, 0.5, (-np.inf, np.inf), 5, n, None
    p._norms = problems._ColumnNorms()
    p._spmat = type("H", (), {"value": C.c_void_p(8192)})()
    p.delta = 0.75
    p.shard = "columns"
    return p


def _factored(cls, pf, monkeypatch):
    monkeypatch.setattr(problems, "_to_device", lambda a, name: _T(12288 if name == "penalty_factor" else 16384))
    return _standin(cls, n=len(pf)).with_penalty_factor(pf)


BADS = {"finite": [1.0, np.nan], "finite and >= 0": [1.0, -0.5], "vector of 2": [1.0, 1.0, 1.0], "real numbers": np.array(["a", "b"]),
        "must be finite": [np.inf, 1.0], "got shape": [[1.0, 1.0]]}


def test_bad_factors_are_refused_before_anything_touches_a_device():
    for cls in WITH_KEYWORD:
        A = sp.eye(2, format="csr") if "Sparse" in cls.__name__ else np.eye(2)
        extra = (1.0,) if "Huber" in cls.__name__ else ()
        for match, pf in BADS.items():
            with pytest.raises(ValueError, match=match):
                cls(A, np.zeros(2), 0.1, *extra, penalty_factor=pf)
        with pytest.raises(ValueError, match="l2 > 0"):
            cls(A, np.zeros(2), 0.1, *extra, l2=0.5, penalty_factor=[1.0, 1.0])
        params = inspect.signature(cls.__init__).parameters
        assert params["penalty_factor"].kind is inspect.Parameter.KEYWORD_ONLY and params["penalty_factor"].default is None
    for cls in (problems.LogisticL1, problems.SparseLogisticL1):   # (their parameter lists are pinned: the sibling form only)
        assert "penalty_factor" not in inspect.signature(cls.__init__).parameters
    with pytest.raises(ValueError, match="group="):
        problems.LeastSquaresL1(np.eye(2), np.zeros(2), 0.1, group=object(), penalty_factor=[1.0, 1.0])
    for cls in EIGHT:
        p = _standin(cls, n=2)
        for match, pf in BADS.items():
            with pytest.raises(ValueError, match=match):
                p.with_penalty_factor(pf)
        assert p.penalty_factor is None and p.with_penalty_factor(None).penalty_factor is None
        p.l2 = 0.25
        with pytest.raises(ValueError, match="l2 > 0"):
            p.with_penalty_factor([1.0, 1.0])
    assert problems._check_penalty_factor([0.0, 0.0], 2).tolist() == [0.0, 0.0], "all columns unpenalised is a legal (smooth) problem"
    assert problems._check_penalty_factor(np.array([1, 2]), 2).dtype == np.float64


@pytest.mark.parametrize("cls", EIGHT)
def test_siblings_share_the_matrix_and_keep_the_factors(cls, monkeypatch):
    pf = np.array([0.0, 0.5, 1.0, 3.0, 0.25, 1.0, 2.0])
    p = _standin(cls)
    q = _factored(cls, pf, monkeypatch)
    assert type(q) is cls
    assert np.array_equal(q.penalty_factor, pf) and p.penalty_factor is None
    q.penalty_factor[0] = 9.0
    assert q.penalty_factor[0] == 0.0, "a copy"
    assert q.A.data_ptr() == 4096 and q.b.data_ptr() == 4096, "the matrix and b of the standin: nothing but p was uploaded"
    fields, keep = q._descriptor()
    assert fields["penalty_factors"] == 12288 and q._pf in keep and "penalty_factors" not in p._descriptor()[0]
    assert not hasattr(_lib.ProblemDesc(), "penalty_factors")
    w = q.with_sample_weight(np.ones(5))
    for sib in (q.with_lam(0.2), w, w.with_lam(0.1), q.with_penalty(0.2, 0.0)):
        assert sib._pf is q._pf and sib.A is q.A and sib.b is q.b and sib._spmat is q._spmat, "nothing is uploaded"
        assert sib._descriptor()[0]["penalty_factors"] == 12288 and np.array_equal(sib.penalty_factor, pf)
    assert w._descriptor()[0]["row_weights"] == 16384 and w.with_penalty_factor(None)._w is w._w
    back = q.with_penalty_factor(None)
    assert back.penalty_factor is None and "penalty_factors" not in back._descriptor()[0] and back.A is q.A
    assert problems.match_native(*q.callbacks()) is q
    assert problems.match_native(q.f, back.g, q.jac_f, q.prox_wsum_g) is None


@pytest.mark.parametrize("cls", EIGHT)
def test_refusals_with_factors(cls, monkeypatch):
    q = _factored(cls, np.array([0.5, 1.0, 2.0, 1.0, 1.0, 1.0, 3.0]), monkeypatch)
    word = "Poisson|penalty_factor" if "Poisson" in cls.__name__ else "penalty_factor"
    for call in (lambda: q.screen(np.zeros(7)), lambda: q.column_norms(), lambda: q.restrict(np.arange(3)),
                 lambda: screening.solve_screened(q, np.zeros(7), 1e-6), lambda: path.l1_path(q, [0.1], screen=True)):
        with pytest.raises(ValueError, match=word):
            call()
    for call in (lambda: q.with_penalty(0.1, 0.5), lambda: path.l1_path(q, [0.1], l2=0.5)):
        with pytest.raises(ValueError, match="l2 > 0 is not available with penalty_factor"):
            call()
    assert q._gap_refusal() is None, "strictly positive factors: the certificate exists"
    # an unpenalised column: no certificate, and the message says what to do
    z = _factored(cls, np.array([0.0, 1.0, 2.0, 1.0, 1.0, 1.0, 3.0]), monkeypatch)
    for call in (lambda: z.duality_gap(np.zeros(7)), lambda: minimize_proximal_gradient(*z.callbacks(), np.zeros(7), gap_tol=1e-6),
                 lambda: path.l1_path(z, [0.1])):
        with pytest.raises(ValueError, match=r"unpenalised column.*gap_tol=None"):
            call()


def test_add_intercept():
    rng = np.random.default_rng(0)
    D = rng.standard_normal((5, 3)) * (rng.random((5, 3)) < 0.6)
    A1, p = problems.add_intercept(D)
    assert isinstance(A1, np.ndarray) and A1.flags.c_contiguous and A1.shape == (5, 4)
    assert np.array_equal(A1[:, 0], np.ones(5)) and np.array_equal(A1[:, 1:], D) and p.tolist() == [0.0, 1.0, 1.0, 1.0]
    for form in (sp.csr_matrix, sp.csc_matrix, sp.coo_matrix):
        S1, ps = problems.add_intercept(form(D))
        assert sp.issparse(S1) and S1.format == "csr" and S1.shape == (5, 4) and np.array_equal(S1.toarray(), A1)
        assert np.array_equal(ps, p)
    with pytest.raises(ValueError, match="A must be"):
        problems.add_intercept(np.zeros(3))
    assert problems._check_penalty_factor(p, 4).tolist() == p.tolist()
