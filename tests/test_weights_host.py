"""CPU: the interface of per-row sample weights without a GPU - header and ctypes table (the struct sizes as
they were), the argument checks of the new entry points before any device is touched, the ValueErrors of the host classes, the
siblings, the fold numbers of l1_cv and its refusals."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import evaldesc as E
import weight_cases as W
from conftest import ROOT
from zfista_amd import _lib, path, problems, screening
from zfista_amd.proximal_gradient import minimize_proximal_gradient

NEW = ("zf_solver_set_row_weights", "zf_margins_eval", "zf_margins_gap")
SIX = [problems.LeastSquaresL1, problems.SparseLeastSquaresL1, problems.LogisticL1, problems.SparseLogisticL1, problems.HuberL1,
       problems.SparseHuberL1]


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
    assert re.search(r"enum\s*\{\s*ZF_LOSS_SQUARE\s*=\s*0,\s*ZF_LOSS_LOGISTIC\s*=\s*1,\s*ZF_LOSS_HUBER\s*=\s*2\s*\}", src)
    assert (_lib.ZF_LOSS_SQUARE, _lib.ZF_LOSS_LOGISTIC, _lib.ZF_LOSS_HUBER) == (0, 1, 2) == tuple(W.LOSS_CODE[k] for k in ("square", "logistic", "huber"))
    assert "row_weights" not in [f[0] for f in _lib.ProblemDesc._fields_]
    assert {"w", "loss"} <= {f[0] for f in _lib.EvalDesc._fields_}, "w and loss are fields of the evaluation descriptor"


def test_new_entry_points_refuse_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    out = np.full(12, -7.0)
    P = C.c_void_p(_lib.ptr(out))
    f = C.c_double(-7.0)
    assert lib.zf_solver_set_row_weights(None, P) == -2 and b"zf_solver_set_row_weights" in lib.zf_last_error()
    # f / grad: a null pointer in every place (but w: NULL weights are the unweighted problem), sizes, the loss, delta
    for field in ("A", "b"):
        assert E.point(E.dense(P, w=P, **{field: None}), P, C.byref(f)) == -2 and b"zf_margins_eval" in lib.zf_last_error(), field
    for field in ("spmat", "b"):
        assert E.point(E.sparse(P, w=P, **{field: None}), P, C.byref(f)) == -2 and b"zf_margins_eval" in lib.zf_last_error(), field
    for d in (E.dense(P, w=P), E.sparse(P, w=P)):
        assert E.point(d, None, C.byref(f)) == -2 and b"zf_margins_eval" in lib.zf_last_error()
        assert E.point(d, P, None) == -2 and b"zf_margins_eval" in lib.zf_last_error()
    assert E.point(E.dense(P, w=P, m_rows=0), P, C.byref(f)) == -2
    assert E.point(E.dense(P, w=P, n=0), P, C.byref(f)) == -2
    for bad_loss in (-1, 4, 7):
        for d in (E.dense(P, w=P, loss=bad_loss, delta=1.0), E.sparse(P, w=P, loss=bad_loss, delta=1.0)):
            assert E.point(d, P, C.byref(f)) == -2 and b"ZF_LOSS_" in lib.zf_last_error()
            assert E.gap(d, P, P, 10) == -2 and b"ZF_LOSS_" in lib.zf_last_error()
    for bad in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):   # delta: checked for Huber's loss only
        for d in (E.dense(P, w=P, loss=2, delta=bad), E.sparse(P, w=P, loss=2, delta=bad)):
            assert E.point(d, P, C.byref(f)) == -2 and b"delta" in lib.zf_last_error()
            assert E.gap(d, P, P, 10) == -2 and b"delta" in lib.zf_last_error()
            assert E.point(E.dense(P, w=P, loss=0, delta=bad, m_rows=0), P, C.byref(f)) == -2 and b"delta" not in lib.zf_last_error()
    # the certificate: null pointers, short buffers, scale, lam, l2
    for field in ("A", "b"):
        assert E.gap(E.dense(P, w=P, **{field: None}), P, P, 10) == -2 and b"zf_margins_gap" in lib.zf_last_error(), field
    for field in ("spmat", "b"):
        assert E.gap(E.sparse(P, w=P, **{field: None}), P, P, 10) == -2 and b"zf_margins_gap" in lib.zf_last_error(), field
    for d in (E.dense(P, w=P), E.sparse(P, w=P, loss=1)):
        assert E.gap(d, None, P, 10) == -2 and b"zf_margins_gap" in lib.zf_last_error()
        assert E.gap(d, P, None, 10) == -2 and b"zf_margins_gap" in lib.zf_last_error()
        for short in (0, 3, 7):
            assert E.gap(d, P, P, short) == -2 and b"fewer than 8" in lib.zf_last_error()
    for bad in (-1e-9, float("inf"), float("nan")):
        assert E.gap(E.dense(P, w=P, l2=bad), P, P, 10) == -2 and b"l2" in lib.zf_last_error()
        assert E.gap(E.sparse(P, w=P, l2=bad), P, P, 10) == -2 and b"l2" in lib.zf_last_error()
    assert E.gap(E.dense(P, w=P, lam=-0.1), P, P, 10) == -2 and b"lam >= 0" in lib.zf_last_error()
    assert E.gap(E.dense(P, w=P, scale=0.0), P, P, 10) == -2 and b"scale > 0" in lib.zf_last_error()
    assert (out == -7.0).all() and f.value == -7.0, "nothing was written"


class _T:   # what the host logic reads of a device tensor
    def __init__(self, p=4096):
        self.p = p

    def data_ptr(self):
        return self.p


def _standin(cls, m=5):
    """A problem object without a device: the attributes the host logic reads."""
    p = object.__new__(cls)
    p.A = p.b = _T()
    p.lam, p.scale, p.box, p.m_rows, p.n_features, p.group = 0.3, 0.5, (-np.inf, np.inf), m, 7, None
    p._norms = problems._ColumnNorms()
    p._spmat = type("H", (), {"value": C.c_void_p(8192)})()
    p.delta = 0.75
    p.shard = "columns"
    return p


def _weighted(cls, w, monkeypatch):
    monkeypatch.setattr(problems, "_to_device", lambda a, name: _T(12288))
    return _standin(cls, m=len(w)).with_sample_weight(w)


def test_bad_weights_are_refused_before_anything_touches_a_device():
    import scipy.sparse as sp

    bads = {"finite": [1.0, np.nan], "finite and >= 0": [1.0, -0.5], "at least one": [0.0, 0.0], "vector of 2": [1.0, 1.0, 1.0],
            "real numbers": np.array(["a", "b"]), "must be finite": [np.inf, 1.0]}
    for cls, A in ((problems.LeastSquaresL1, np.eye(2)), (problems.SparseLeastSquaresL1, sp.eye(2, format="csr")),
                   (problems.HuberL1, np.eye(2)), (problems.SparseHuberL1, sp.eye(2, format="csr"))):
        extra = (1.0,) if "Huber" in cls.__name__ else ()
        for match, w in bads.items():
            with pytest.raises(ValueError, match=match):
                cls(A, np.zeros(2), 0.1, *extra, sample_weight=w)
        params = inspect.signature(cls.__init__).parameters
        assert params["sample_weight"].kind is inspect.Parameter.KEYWORD_ONLY and params["sample_weight"].default is None
    with pytest.raises(ValueError, match="group="):
        problems.LeastSquaresL1(np.eye(2), np.zeros(2), 0.1, group=object(), sample_weight=[1.0, 1.0])
    for cls in SIX:   # the sibling form - the logistic classes' only one: their constructor's parameter list is pinned
        p = _standin(cls, m=2)
        for match, w in bads.items():
            with pytest.raises(ValueError, match=match):
                p.with_sample_weight(w)
        assert p.sample_weight is None and p.with_sample_weight(None).sample_weight is None


@pytest.mark.parametrize("cls", SIX)
def test_siblings_share_the_matrix_and_keep_the_weights(cls, monkeypatch):
    w = np.array([0.0, 0.5, 1.0, 3.0, 0.25])
    p = _standin(cls)
    q = _weighted(cls, w, monkeypatch)
    assert type(q) is cls and q.A is not None and np.array_equal(q.sample_weight, w) and p.sample_weight is None
    q.sample_weight[0] = 9.0
    assert q.sample_weight[0] == 0.0, "a copy"
    fields, keep = q._descriptor()
    assert fields["row_weights"] == 12288 and q._w in keep and "row_weights" not in p._descriptor()[0]
    assert not hasattr(_lib.ProblemDesc(), "row_weights")
    for sib in (q.with_lam(0.2), q.with_penalty(0.2, 0.1)):
        assert sib._w is q._w and sib.A is q.A and sib.b is q.b and sib._spmat is q._spmat, "nothing is uploaded"
        assert sib._descriptor()[0]["row_weights"] == 12288
    back = q.with_sample_weight(None)
    assert back.sample_weight is None and "row_weights" not in back._descriptor()[0] and back.A is q.A
    assert getattr(back, "taylor_remainder", False) == getattr(p, "taylor_remainder", False)
    assert not getattr(q, "taylor_remainder", False)
    assert problems.match_native(*q.callbacks()) is q
    assert q._loss == {"Logistic": 1, "Huber": 2}.get(next((k for k in ("Logistic", "Huber") if k in cls.__name__), ""), 0)


@pytest.mark.parametrize("cls", SIX)
def test_refusals_with_weights(cls, monkeypatch):
    q = _weighted(cls, np.ones(5), monkeypatch)
    for call in (lambda: q.screen(np.zeros(7)), lambda: q.column_norms(), lambda: q.restrict(np.arange(3)),
                 lambda: screening.solve_screened(q, np.zeros(7), 1e-6), lambda: path.l1_path(q, [0.1], screen=True),
                 lambda: path.l1_cv(q, [0.1], folds=2, screen=True)):
        with pytest.raises(ValueError, match="sample_weight"):
            call()
    for bad in ("remainder", "resolved"):
        with pytest.raises(ValueError, match=f"acceptance='{bad}' is not available with sample_weight"):
            minimize_proximal_gradient(*q.callbacks(), np.zeros(7), acceptance=bad)
    assert q._gap_refusal() is None, "the certificate exists"


def test_l1_cv_fold_ids_are_exact():
    ids = path.cv_fold_ids(7, 3, seed=0)
    perm = np.random.default_rng(0).permutation(7)
    want = np.empty(7, dtype=np.int64)
    for k in range(3):
        want[perm[k::3]] = k
    assert np.array_equal(ids, want) and np.array_equal(ids, W.fold_ids(7, 3, 0)) and ids.dtype == np.int64
    assert [int((ids == k).sum()) for k in range(3)] == [3, 2, 2]
    assert not np.array_equal(path.cv_fold_ids(7, 3, seed=1), ids)
    given = np.array([2, 0, 1, 1, 0, 2, 2])
    assert np.array_equal(path.cv_fold_ids(7, given), given)
    for bad in (1, 8, 2.5, np.zeros(6, dtype=int), np.zeros(7)):
        with pytest.raises(ValueError, match="fold"):
            path.cv_fold_ids(7, bad)


def test_l1_cv_refuses_a_fold_without_training_weight_before_any_solve(monkeypatch):
    w = np.array([0.0, 0.0, 1.0, 0.0, 2.0])
    q = _weighted(problems.SparseLeastSquaresL1, w, monkeypatch)
    with pytest.raises(ValueError, match="fold 1 leaves no training weight"):
        path.l1_cv(q, [0.1], folds=np.array([0, 0, 1, 0, 1]))
    with pytest.raises(ValueError, match="fold 0 holds no weight"):
        path.l1_cv(q, [0.1], folds=np.array([0, 0, 1, 0, 2]))
    with pytest.raises(ValueError, match=f"fold {W.fold_ids(3, 3, 0)[2]} leaves no training weight"):
        path.l1_cv(_weighted(problems.LogisticL1, [0.0, 0.0, 3.0], monkeypatch), [0.1], folds=3, seed=0)
    with pytest.raises(ValueError, match="at least two folds"):
        path.l1_cv(q, [0.1], folds=np.zeros(5, dtype=int))
    with pytest.raises(ValueError, match="at least one value"):
        path.l1_cv(q, [], folds=2)
    with pytest.raises(ValueError, match="margins classes"):
        path.l1_cv(object(), [0.1])


def test_cv_summary():
    lams = [1.0, 0.5, 0.25, 0.125]
    scores = np.array([[3.0, 2.0, 1.0, 1.5], [3.2, 1.0, 1.2, 1.7], [2.8, 1.5, 0.8, 1.6]])
    mean, se, best, lam_best, lam_1se = path.cv_summary(lams, scores)
    assert np.allclose(mean, scores.mean(0)) and np.allclose(se, scores.std(0, ddof=1) / np.sqrt(3))
    assert best == 2 and lam_best == 0.25
    assert lam_1se == max(l for l, m_ in zip(lams, mean) if m_ <= mean[2] + se[2]) == 0.25
    flat = np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0]])
    assert path.cv_summary([3.0, 2.0, 1.0], flat)[2:] == (0, 3.0, 3.0)
