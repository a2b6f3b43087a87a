"""CPU: the interface of the multinomial classes without a GPU - header and ctypes table (one enumerator, one entry, no struct
change, ABI 7), the argument checks of the setter and of the three evaluation entries before any device is touched (with poisoned
pointers that nothing may read), label expansion, every ValueError of the host classes, the descriptor fields and the engine's
call order."""
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

MN = _lib.ZF_LOSS_MULTINOMIAL
CLASSES = [problems.MultinomialL1, problems.SparseMultinomialL1]


def test_header_and_ctypes_table_declare_one_enumerator_and_one_entry():
    src = open(os.path.join(ROOT, "include", "zfista_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    assert re.search(r"\bint\s+zf_solver_set_multinomial\s*\(\s*zf_solver\s*\*\s*s\s*\)", src)
    assert "zf_solver_set_multinomial" in _lib.SIGNATURES and hasattr(lib, "zf_solver_set_multinomial")
    assert _lib.SIGNATURES["zf_solver_set_multinomial"] == (C.c_int, [C.c_void_p])
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(zf_[A-Za-z0-9_]+)\s*\(", src))), "header = ctypes table"
    assert re.search(r"ZF_LOSS_MULTINOMIAL\s*=\s*4\b", src) and MN == 4
    assert lib.zf_abi_version() == 7 and lib.zf_sizeof_control() == 424 == C.sizeof(_lib.Control)
    assert C.sizeof(_lib.ProblemDesc) == 128 and C.sizeof(_lib.Options) == 64 and lib.zf_sizeof_eval_desc() == C.sizeof(_lib.EvalDesc)
    assert "multinomial" not in [f[0] for f in _lib.ProblemDesc._fields_]
    assert max(v for k, v in vars(_lib).items() if k.startswith("ZF_PROBLEM_")) == 6, "no new problem kind"


def test_the_entries_refuse_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    out = np.full(12, -7.0)
    P = C.c_void_p(_lib.ptr(out))
    odd = C.c_void_p(_lib.ptr(out) + 8)
    assert _lib.ptr(out) % 16 == 0
    f = C.c_double(-7.0)
    assert lib.zf_solver_set_multinomial(None) == -2 and b"zf_solver_set_multinomial" in lib.zf_last_error()
    for make in (E.dense, E.sparse):
        # K = 1: refused, and the text keeps listing the codes
        d = make(P, loss=MN, K=1, scale=1.0)
        assert E.point(d, P, C.byref(f)) == -2 and b"ZF_LOSS_MULTINOMIAL" in lib.zf_last_error() and b"ZF_LOSS_POISSON" in lib.zf_last_error()
        assert E.gap(d, P, P, 10) == -2 and b"K = 2 .. 16" in lib.zf_last_error()
        for K in (0, 17, -3):
            assert E.point(make(P, loss=MN, K=K), P, C.byref(f)) == -2 and b"K must be 1 .. 16" in lib.zf_last_error()
        for K in (2, 16):
            D = lambda **kw: make(P, **{**dict(loss=MN, K=K, scale=1.0), **kw})   # noqa: E731
            assert E.point(D(b=None), P, C.byref(f)) == -2 and b"null" in lib.zf_last_error()
            assert E.point(D(), None, C.byref(f)) == -2 and E.point(D(), P, None) == -2
            assert E.point(D(b=odd), P, C.byref(f)) == -2 and b"16-byte aligned" in lib.zf_last_error()
            assert E.gap(D(b=odd), P, P, 10) == -2 and b"16-byte aligned" in lib.zf_last_error()
            assert E.gap(D(), P, P, 7) == -2 and b"fewer than 8" in lib.zf_last_error()
            assert E.gap(D(scale=0.0), P, P, 10) == -2 and b"scale > 0" in lib.zf_last_error()
            assert E.gap(D(lam=-1.0), P, P, 10) == -2 and b"lam >= 0" in lib.zf_last_error()
            assert E.gap(D(p=P, l2=0.5), P, P, 10) == -2 and b"penalty factors and l2" in lib.zf_last_error()
            assert E.point(D(), P, C.byref(f), desc_bytes=C.sizeof(D()) - 8) == -2 and b"desc_bytes" in lib.zf_last_error()
            # screening is refused for this loss before anything else of the rule is looked at
            assert E.screen(D(), P, P, 12, P, P, 2, 3, P, P) == -2 and b"ZF_LOSS_MULTINOMIAL" in lib.zf_last_error()
    # an fp32 matrix: refused for K = 1 and for K > 1
    for K in (1, 2, 16):
        assert E.point(E.dense32(P, loss=MN, K=K), P, C.byref(f)) == -2
        assert E.gap(E.dense32(P, loss=MN, K=K), P, P, 10) == -2
    assert E.point(E.dense32(P, loss=MN, K=2), P, C.byref(f)) == -2 and b"fp32" in lib.zf_last_error()
    assert E.point(E.dense(P, loss=MN, K=2, A=odd), P, C.byref(f)) == -2 and b"aligned" in lib.zf_last_error()
    # the other losses with K > 1 keep their refusal, and the text names the three that are served
    for loss in (_lib.ZF_LOSS_HUBER, _lib.ZF_LOSS_POISSON):
        assert E.point(E.dense(P, loss=loss, K=2, delta=1.0), P, C.byref(f)) == -2 and b"ZF_LOSS_MULTINOMIAL" in lib.zf_last_error()
    assert (out == -7.0).all() and f.value == -7.0, "nothing was written"


def test_label_expansion():
    Y, classes = problems._check_classes(np.array([2, 0, 1, 2]), 4)
    assert np.array_equal(Y, np.eye(3)[[2, 0, 1, 2]]) and np.array_equal(classes, [0, 1, 2]) and Y.dtype == np.float64
    Y, classes = problems._check_classes(np.array([0, 1, 1], dtype=np.uint8), 3, n_classes=5)
    assert Y.shape == (3, 5) and not Y[:, 2:].any() and np.array_equal(classes, np.arange(5)), "a class that never occurs"
    Y, _ = problems._check_classes([True, False], 2)
    assert np.array_equal(Y, [[0.0, 1.0], [1.0, 0.0]])
    soft = np.array([[0.25, 0.75], [1.0, 0.0], [0.5, 0.5 + 5e-13]])
    Y, classes = problems._check_classes(soft, 3)
    assert np.array_equal(Y, soft) and Y is not soft and np.array_equal(classes, [0, 1])
    # a row whose weight is 0 is not checked
    bad = soft.copy()
    bad[1] = np.nan
    Y, _ = problems._check_classes(bad, 3, weights=np.array([1.0, 0.0, 2.0]))
    assert np.isnan(Y[1]).all()
    for y, why in (([0, 1, -1], ">= 0"), ([0.0, 1.0, 2.0], "INTEGER"), ([0, 0, 0], "2 .. 16"), (np.arange(3) * 8, "2 .. 16"),
                   ([0, 1], "3 class labels"), (["a", "b", "c"], "dtype"), (np.zeros((3, 1)), "2 .. 16"), (np.full((3, 17), 1 / 17), "2 .. 16"),
                   (np.zeros((2, 2)), "3 class labels or"), (np.zeros((3, 2, 1)), "3 class labels or"),
                   ([[0.5, 0.5], [0.5, 0.5 + 1e-11], [1, 0]], "sum to 1"), ([[1.5, -0.5], [1, 0], [0, 1]], "finite and >= 0"),
                   ([[np.nan, 1], [1, 0], [0, 1]], "finite and >= 0"), ([[np.inf, 0], [1, 0], [0, 1]], "finite and >= 0"), (bad, "finite and >= 0")):
        with pytest.raises(ValueError, match=why):
            problems._check_classes(np.asarray(y), 3)
    for nc in (1, 17, 2.5):
        with pytest.raises(ValueError, match="n_classes"):
            problems._check_classes(np.array([0, 1, 1]), 3, n_classes=nc)
    with pytest.raises(ValueError, match="outside 0 .. n_classes"):
        problems._check_classes(np.array([0, 1, 3]), 3, n_classes=3)
    with pytest.raises(ValueError, match="n_classes = 3 but y has 2"):
        problems._check_classes(soft, 3, n_classes=3)


def test_the_constructors_refuse_before_anything_touches_a_device(monkeypatch):
    import scipy.sparse as sp

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(problems, "_to_device", no_device)
    monkeypatch.setattr(problems, "_SpmatHandle", no_device)
    y = np.array([0, 1, 2])
    for cls, A in ((problems.MultinomialL1, np.eye(3)), (problems.SparseMultinomialL1, sp.eye(3, format="csr"))):
        for bad, why in (([0, 0, 0], "2 .. 16"), ([0, 1, 40], "2 .. 16"), ([0.5, 0.5, 0.0], "INTEGER"), ([0, 1], "3 class labels"),
                         (np.full((3, 2), 0.6), "sum to 1")):
            with pytest.raises(ValueError, match=why):
                cls(A, np.asarray(bad), 0.1)
        with pytest.raises(ValueError, match="group="):
            cls(A, y, 0.1, group=object())
        with pytest.raises(ValueError, match="l2 must be finite"):
            cls(A, y, 0.1, l2=-1.0)
        with pytest.raises(ValueError, match="sample_weight must be a vector of 3"):
            cls(A, y, 0.1, sample_weight=np.ones((3, 3)))
        with pytest.raises(ValueError, match="sample_weight must be finite"):
            cls(A, y, 0.1, sample_weight=np.array([1.0, -1.0, 1.0]))
        with pytest.raises(ValueError, match="penalty_factor must have shape"):
            cls(A, y, 0.1, penalty_factor=np.ones(4))
        with pytest.raises(ValueError, match="penalty_factor is not available with l2"):
            cls(A, y, 0.1, l2=0.5, penalty_factor=np.ones(3))
        with pytest.raises(ValueError, match="n_classes"):
            cls(A, y, 0.1, n_classes=2)
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[:7] == ["self", "A", "y", "lam", "scale", "bounds", "l2"]
        assert params["scale"].default == 1.0 and params["l2"].default == 0.0 and params["bounds"].default is None
        for kw in ("sample_weight", "penalty_factor", "n_classes"):
            assert params[kw].kind is inspect.Parameter.KEYWORD_ONLY and params[kw].default is None


class _T:   # what the host logic reads of a device tensor
    def data_ptr(self):
        return 4096

    def numel(self):
        return 5


def _standin(cls, K=3, m=5, n=7):
    """A problem object without a device: the attributes the host logic reads."""
    p = object.__new__(cls)
    if issubclass(cls, problems._MultinomialMixin):
        p.kind = cls._ls_kind   # (what _set_multinomial does first)
    p.A = p.b = _T()
    p._f32 = False
    p.lam, p.scale, p.box, p.group = 0.3, 1.0, (-np.inf, np.inf), None
    p._m, p._n, p.n_responses, p.m_rows, p.n_features = m, n, K, m * K, n * K
    p.classes = np.arange(K)
    p._norms = problems._ColumnNorms()
    p._spmat = type("H", (), {"value": C.c_void_p(8192)})()
    return p


@pytest.mark.parametrize("cls", CLASSES)
def test_the_classes_are_least_squares_kinds_with_multinomial_in_the_descriptor(cls):
    p = _standin(cls)
    base = problems.LeastSquaresL1 if cls is problems.MultinomialL1 else problems.SparseLeastSquaresL1
    assert cls.kind is None and p.kind == cls._ls_kind == base.kind and p.kind in (2, 4), "no new problem kind; the instance carries it"
    assert cls._loss == MN == 4 and not p.taylor_remainder and not getattr(p, "separable", False)
    mixin = problems._SparseMultiResponseMixin if p.kind == 4 else problems._MultiResponseMixin
    assert issubclass(cls, mixin) and issubclass(cls, problems._GapMixin)
    fields, _ = p._descriptor()
    assert fields["multinomial"] is True and fields["responses"] == 3 and fields["kind"] == p.kind
    assert (fields["m_rows"], fields["n"]) == (15, 21) and "poisson" not in fields and "huber_delta" not in fields and "l2" not in fields
    fields, _ = p.with_penalty(0.3, 0.25)._descriptor()
    assert fields["multinomial"] is True and fields["l2"] == 0.25
    for other in (problems.MultiResponseLeastSquaresL1, problems.MultiResponseLogisticL1, problems.SparseMultiResponseLeastSquaresL1):
        assert "multinomial" not in _standin(other)._descriptor()[0], "the other K-response classes hand the engine what they did"
    d = p._eval_desc()
    assert p.has_duality_gap and (d.loss, d.K, d.delta, d.w, d.p) == (MN, 3, 0.0, None, None)
    assert (bool(d.A), bool(d.spmat)) == (p.kind == 2, p.kind == 4) and not d.A32
    if p.kind == 2:
        assert (d.m_rows, d.n) == (5, 7), "the MATRIX's sizes"
    X = np.arange(21.0).reshape(7, 3)
    assert np.array_equal(p.coef(X.reshape(-1)), X) and np.array_equal(p._flat(X), X.reshape(-1))
    q = p.with_lam(0.2)
    assert type(q) is cls and q.A is p.A and q.b is p.b and q._spmat is p._spmat and q.classes is p.classes
    assert problems.match_native(*q.callbacks()) is q


def test_the_engine_calls_the_setter_after_the_responses(monkeypatch):
    """Call order: create, ..., zf_solver_set_responses, then zf_solver_set_multinomial (the setter refuses a solver without them)."""
    from zfista_amd import engine

    calls = []

    class _Lib:
        def __getattr__(self, name):
            def fn(*a):
                calls.append(name)
                if name == "zf_solver_sub_iters":
                    a[1]._obj.value = 1
                return 0
            return fn

    monkeypatch.setattr(engine._lib, "require_gpu", lambda: _Lib())
    for cls in CLASSES:
        del calls[:]
        fields, keep = _standin(cls)._descriptor()
        try:
            engine.DeviceSolver(fields, dict(lr=1.0), keepalive=keep, stream=0)
        except Exception:
            pass   # (whatever follows the setters needs a device)
        assert "zf_solver_set_multinomial" in calls
        first = "zf_solver_set_responses" if cls._ls_kind == 2 else "zf_solver_create_sparse_responses"
        assert calls.index(first) < calls.index("zf_solver_set_multinomial"), calls
        assert "zf_solver_set_poisson" not in calls and "zf_solver_set_huber" not in calls


@pytest.mark.parametrize("cls", CLASSES)
def test_what_the_classes_refuse(cls):
    p = _standin(cls)
    x = np.zeros(21)
    for bad, why in (("remainder", "several responses"), ("resolved", "several responses")):
        with pytest.raises(ValueError, match=why):
            minimize_proximal_gradient(*p.callbacks(), x, acceptance=bad)
    for call in (lambda: p.column_norms(), lambda: p.screen(x), lambda: p.restrict(np.arange(3)),
                 lambda: screening.solve_screened(p, x, 1e-6), lambda: path.l1_path(p, [0.1], screen=True)):
        with pytest.raises(ValueError, match="several responses"):
            call()
    with pytest.raises(ValueError):
        p.with_matrix_dtype("float32")
    with pytest.raises(ValueError, match="l1_cv_lockstep needs"):
        path.l1_cv_lockstep(p, [0.1], folds=3)
    with pytest.raises(ValueError, match="sample_weight must be a vector of 5"):
        p.with_sample_weight(np.ones((5, 3)))
    with pytest.raises(ValueError, match="sample_weight must be a vector of 5"):
        p.with_sample_weight(np.ones(15))
    with pytest.raises(ValueError, match="penalty_factor must have shape"):
        p.with_penalty_factor(np.ones(21))
    boxed = _standin(cls)
    boxed.box = (-1.0, 1.0)
    for call in (lambda: boxed.duality_gap(x), lambda: minimize_proximal_gradient(*boxed.callbacks(), x, gap_tol=1e-6)):
        with pytest.raises(ValueError, match="bounds are set"):
            call()
    zero = _standin(cls)
    zero._pf, zero._pf_host = _T(), np.r_[0.0, np.ones(20)]
    for call in (lambda: zero.duality_gap(x), lambda: minimize_proximal_gradient(*zero.callbacks(), x, gap_tol=1e-6)):
        with pytest.raises(ValueError, match="unpenalised column"):
            call()
    with pytest.raises(ValueError, match="n_features"):
        p.duality_gap(np.zeros(20))


def test_with_classes_is_offered_by_both_logistic_classes_and_refuses_on_the_host():
    for cls in (problems.LogisticL1, problems.SparseLogisticL1):
        assert callable(cls.with_classes)
        p = object.__new__(cls)
        p.A, p.b, p._f32, p.group = _T(), _T(), False, None
        p.A.shape = (3, 2)
        p.lam, p.scale, p.box, p.m_rows, p.n_features, p.l2 = 0.3, 1.0, (-np.inf, np.inf), 3, 2, 0.0
        with pytest.raises(ValueError, match="2 .. 16"):
            p.with_classes(np.array([0, 0, 0]))
        with pytest.raises(ValueError, match="3 class labels"):
            p.with_classes(np.array([0, 1]))
        with pytest.raises(ValueError, match="sample_weight must be a vector of 3"):
            p.with_classes(np.array([0, 1, 2]), sample_weight=np.ones((3, 3)))
    f32 = object.__new__(problems.LogisticL1)
    f32._f32, f32.group = True, None
    with pytest.raises(ValueError, match="float32"):
        f32.with_classes(np.array([0, 1, 2]))


def test_the_classes_are_exported_and_documented():
    for name in ("MultinomialL1", "SparseMultinomialL1"):
        cls = getattr(problems, name)
        assert inspect.isclass(cls) and issubclass(cls, problems.NativeProblem) and callable(cls.predict_proba) and callable(cls.coef)
    assert "softmax" in problems.MultinomialL1.__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "MultinomialL1(A, y, lam" in readme and "SparseMultinomialL1" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.5o" in design and "zf_softmax_rows_kernel" in design
    assert "zf_solver_set_multinomial" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(ROOT, "examples", "multinomial_path.py"))


@pytest.mark.parametrize("cls", CLASSES)
def test_dropping_the_weights_checks_the_rows_they_hid(cls):
    """A zero-weight row may hold anything in y; the unweighted sibling has that row again, so with_sample_weight(None) checks it."""
    import torch

    p = _standin(cls)
    Y = np.tile([0.2, 0.3, 0.5], (5, 1))
    p.b = torch.from_numpy(Y.reshape(-1).copy())
    p._w = p._w_host = None
    q = p.with_sample_weight(None)
    assert type(q) is cls and q._w is None and q.b is p.b
    Y[2] = np.nan
    p.b = torch.from_numpy(Y.reshape(-1).copy())
    with pytest.raises(ValueError, match="finite"):
        p.with_sample_weight(None)
    with pytest.raises(ValueError, match="sum to 1|finite"):
        p.with_sample_weight(np.array([1.0, 1.0, 1.0, 0.0, 1.0]))   # (the NaN row keeps a weight)
