"""CPU: the evaluation descriptor without a GPU.  (1) The dispatch table: for every margins class as a device-less stand-in, with
and without weights, penalty factors, l2, an fp32 matrix (dense) and K responses (multi-response), ``_eval_desc()`` holds exactly
the fields the three entries must see - what six branches over entry names used to decide.  (2) The refusals that only the one
screen entry can make, and K > 1 with an fp32 matrix."""
import ctypes as C
import itertools

import numpy as np
import pytest

import evaldesc as E
from zfista_amd import _lib, problems

A_PTR, B_PTR, W_PTR, P_PTR, H_PTR = 4096, 8192, 12288, 16384, 20480
M, N = 5, 7


class _T:   # what the host logic reads of a device tensor
    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


class _H:   # ... and of a matrix handle
    value = C.c_void_p(H_PTR)


def _margins_classes():
    out, todo = [], [problems._GapMixin]
    while todo:
        c = todo.pop()
        todo += c.__subclasses__()
        if getattr(c, "kind", None) is not None and c not in out:
            out.append(c)
    return sorted(out, key=lambda c: c.__name__)


CLASSES = _margins_classes()
LOSS = {"Logistic": _lib.ZF_LOSS_LOGISTIC, "Huber": _lib.ZF_LOSS_HUBER, "Poisson": _lib.ZF_LOSS_POISSON}


def test_every_margins_class_is_in_the_table():
    names = {c.__name__ for c in CLASSES}
    assert len(CLASSES) == 12, names
    for loss in ("LeastSquares", "Logistic"):
        assert {f"{loss}L1", f"Sparse{loss}L1", f"MultiResponse{loss}L1", f"SparseMultiResponse{loss}L1"} <= names
    for loss in ("Huber", "Poisson"):
        assert {f"{loss}L1", f"Sparse{loss}L1"} <= names


def _standin(cls, K, w, p, l2, f32):
    q = object.__new__(cls)
    q.b, q.lam, q.scale, q.box, q.group = _T(B_PTR), 0.3, 0.5, (-np.inf, np.inf), None
    if issubclass(cls, problems._SparseMarginsL1):
        q._spmat = _H()
    else:
        q.A, q._f32 = _T(A_PTR), f32
    if issubclass(cls, problems._MultiResponseMixin):
        q._m, q._n, q.n_responses = M, N, K
    q.m_rows, q.n_features = M * K, N * K   # (the flattened lengths)
    if cls._loss == _lib.ZF_LOSS_HUBER:
        q.delta = 0.75
    if w:
        q._w = _T(W_PTR)
    if p:
        q._pf = _T(P_PTR)
    if l2:
        q.l2 = l2
    return q


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_the_descriptor_holds_exactly_the_expected_fields(cls):
    sparse = issubclass(cls, problems._SparseMarginsL1)
    mr = issubclass(cls, problems._MultiResponseMixin)
    loss = next((code for name, code in LOSS.items() if name in cls.__name__), _lib.ZF_LOSS_SQUARE)
    assert cls._loss == loss
    seen = 0
    for K, w, p, l2, f32 in itertools.product((1, 3) if mr else (1,), (False, True), (False, True), (0.0, 0.25),
                                              (False,) if sparse or mr else (False, True)):
        if p and l2:
            continue   # (refused together, on the host and in the library)
        d = _standin(cls, K, w, p, l2, f32)._eval_desc()
        assert isinstance(d, _lib.EvalDesc)
        # exactly one of the three matrix pointers
        want = (None, None, H_PTR) if sparse else (None, A_PTR, None) if f32 else (A_PTR, None, None)
        assert (d.A, d.A32, d.spmat) == want, (K, w, p, l2, f32)
        # the MATRIX's sizes, not the flattened lengths (a handle knows its own: the fields stay 0)
        assert (d.m_rows, d.n) == ((0, 0) if sparse else (M, N)), (K, d.m_rows, d.n)
        assert (d.loss, d.K) == (loss, K)
        assert d.delta == (0.75 if loss == _lib.ZF_LOSS_HUBER else 0.0)
        assert d.b == B_PTR and d.w == (W_PTR if w else None) and d.p == (P_PTR if p else None)
        assert (d.scale, d.lam, d.l2) == (0.5, 0.3, l2)
        seen += 1
    assert seen == 6 * (1 if sparse and not mr else 2)


def test_a_stale_delta_attribute_does_not_reach_another_loss():
    q = _standin(problems.LeastSquaresL1, 1, False, False, 0.0, False)
    q.delta = 0.75
    assert q._eval_desc().delta == 0.0


def _buffers():
    out = np.full(12, -7.0)
    return out, C.c_void_p(_lib.ptr(out))


def test_the_screen_entry_refuses_what_the_rule_is_not_built_for():
    lib = _lib.load()
    out, P = _buffers()
    tail = (P, P, 12, P, P, 2, 3, P, P)
    for make in (E.dense, E.sparse):
        assert E.screen(make(P, loss=_lib.ZF_LOSS_POISSON), *tail) == -2 and b"ZF_LOSS_POISSON" in lib.zf_last_error()
        assert E.screen(make(P, w=P), *tail) == -2 and b"row weights" in lib.zf_last_error()
        assert E.screen(make(P, p=P), *tail) == -2 and b"penalty factors" in lib.zf_last_error()
        assert E.screen(make(P, l2=0.25), *tail) == -2 and b"l2 > 0" in lib.zf_last_error()
        assert E.screen(make(P, K=2), *tail) == -2 and b"K > 1" in lib.zf_last_error()
        for loss in (_lib.ZF_LOSS_SQUARE, _lib.ZF_LOSS_LOGISTIC, _lib.ZF_LOSS_HUBER):   # a short buffer is "fewer than 12" for every loss
            for short in (0, 8, 11):
                assert E.screen(make(P, loss=loss, delta=1.0), P, P, short, P, P, 2, 3, P, P) == -2 and b"fewer than 12" in lib.zf_last_error()
    assert E.screen(E.dense32(P), *tail) == -2 and b"fp32" in lib.zf_last_error()
    assert E.screen(E.dense(P, n=2 ** 31), *tail) == -2 and b"2^31" in lib.zf_last_error()
    for k in (3, 4, 7, 8):   # norms, stats, keep, index
        args = list(tail)
        args[k] = None
        assert E.screen(E.dense(P), *args) == -2 and b"null" in lib.zf_last_error(), k
        assert E.screen(E.sparse(P), *args) == -2 and b"null" in lib.zf_last_error(), k
    for bad in ((-1, 3), (2, -1)):   # the longest row / column: read for a handle only
        assert E.screen(E.sparse(P), P, P, 12, P, P, *bad, P, P) == -2 and b">= 0" in lib.zf_last_error()
    assert (out == -7.0).all(), "nothing was written"


def test_several_responses_on_an_fp32_matrix_are_refused():
    lib = _lib.load()
    out, P = _buffers()
    f = C.c_double(-7.0)
    for K in (2, 16):
        assert E.point(E.dense32(P, K=K), P, C.byref(f)) == -2 and b"fp32" in lib.zf_last_error()
        assert E.gap(E.dense32(P, K=K), P, P, 10) == -2 and b"fp32" in lib.zf_last_error()
    assert (out == -7.0).all() and f.value == -7.0


def test_exactly_one_matrix_is_required():
    lib = _lib.load()
    out, P = _buffers()
    f = C.c_double(-7.0)
    for d in (E.desc(b=P, m_rows=3, n=2), E.dense(P, A32=P), E.dense(P, spmat=P), E.dense32(P, spmat=P), E.dense(P, A32=P, spmat=P)):
        assert E.point(d, P, C.byref(f)) == -2 and b"exactly one" in lib.zf_last_error()
        assert E.gap(d, P, P, 10) == -2 and b"exactly one" in lib.zf_last_error()
        assert E.screen(d, P, P, 12, P, P, 2, 3, P, P) == -2 and b"exactly one" in lib.zf_last_error()
    assert (out == -7.0).all() and f.value == -7.0
