"""The sequences of zf_solver_set_* calls that tests/golden/solver_options_parent.jsonl records, and the code that drives a library
through one of them.  No solve is run: the matrices are zero-filled device buffers (the CSR bases: an identity), and an entry is

    base, calls -> the 6 values of zf_solver_ls_plan at creation, then (return code, the 6 values) after every call.

A call is a string: "l2=0.5", "l2=0", "pf" (n ones as penalty factors), "huber=0.5", "poisson", "multinomial", "roww" (m_rows ones),
"f32" (the matrix buffer as fp32), "K=2" - the nine option values - and, for the refusals of arguments, other numbers behind the
"=", "pf=NULL" / "roww=NULL" / "f32=NULL", "pf+8" / "f32+8" (the pointer offset by 8 bytes).  decode() gives (option index of
csrc/zf_solver_options.h, value, pointer class, K) for the replay without a device (tests/test_solver_options_cpp.py).
"""
import itertools
import json
import math
import os

OPTIONS = ("l2", "pf", "huber", "poisson", "multinomial", "roww", "f32", "K")   # (the order of enum zf_option)
ENTRY = {"l2": "zf_solver_set_l2", "pf": "zf_solver_set_penalty_factors", "huber": "zf_solver_set_huber", "poisson": "zf_solver_set_poisson",
         "multinomial": "zf_solver_set_multinomial", "roww": "zf_solver_set_row_weights", "f32": "zf_solver_set_matrix_f32",
         "K": "zf_solver_set_responses"}
NINE = ("l2=0.5", "l2=0", "pf", "huber=0.5", "poisson", "multinomial", "roww", "f32", "K=2")

# id -> kind (ZF_PROBLEM_*), accept mode (ZF_ACCEPT_*), world, m_rows, n (flattened), K of zf_solver_create_sparse_responses (0: another
# creator), b offset in bytes.  The first twelve are the bases of the pairs.
BASES = {
    "dense-ls": dict(kind=2, accept=0, world=1, m_rows=64, n=64, K0=0, b_off=0),        # eligible for the fused small-matrix path
    "dense-ls-rem": dict(kind=2, accept=2, world=1, m_rows=64, n=64, K0=0, b_off=0),
    "dense-logistic": dict(kind=5, accept=0, world=1, m_rows=64, n=64, K0=0, b_off=0),
    "csr-ls": dict(kind=4, accept=0, world=1, m_rows=64, n=64, K0=0, b_off=0),
    "csr-ls-rem": dict(kind=4, accept=2, world=1, m_rows=64, n=64, K0=0, b_off=0),
    "csr-logistic": dict(kind=6, accept=0, world=1, m_rows=64, n=64, K0=0, b_off=0),
    "csr-ls-k2": dict(kind=4, accept=0, world=1, m_rows=64, n=64, K0=2, b_off=0),        # a 32 x 32 handle
    "csr-logistic-k2": dict(kind=6, accept=0, world=1, m_rows=64, n=64, K0=2, b_off=0),
    "diag": dict(kind=1, accept=0, world=1, m_rows=0, n=64, K0=0, b_off=0),
    "diag-resolved": dict(kind=1, accept=1, world=1, m_rows=0, n=64, K0=0, b_off=0),
    "operator": dict(kind=3, accept=0, world=1, m_rows=64, n=64, K0=0, b_off=0),         # an 8 x 8 image, 3 x 3 taps
    "dense-ls-world2": dict(kind=2, accept=0, world=2, m_rows=64, n=64, K0=0, b_off=0),  # rank 0 of 2, created directly
    "dense-ls-b8": dict(kind=2, accept=0, world=1, m_rows=64, n=64, K0=0, b_off=8),
    "dense-ls-regrow": dict(kind=2, accept=0, world=1, m_rows=1024, n=20000, K0=0, b_off=0),   # on a buffer of 512 x 20000 doubles
}
PAIR_BASES = tuple(BASES)[:12]
BAD = (["l2=-1", "l2=inf", "l2=nan", "huber=0", "huber=-1", "huber=inf", "huber=nan", "K=1", "K=0", "K=-1", "K=17", "K=3",
        "pf=NULL", "roww=NULL", "f32=NULL", "pf+8", "f32+8"])


def entries():
    """[(group, base id, initialised before the calls, calls)]: the group is the id of tests/test_gpu_solver_options.py."""
    out = []
    for base in PAIR_BASES:
        out += [(base, base, False, list(pair)) for pair in itertools.product(NINE, repeat=2)]
    eight = [v for v in NINE if v != "l2=0"]
    out += [("triples", "dense-ls", False, list(t)) for t in itertools.permutations(eight, 3)]
    out += [("after-init", "dense-ls", True, [v]) for v in NINE]
    out += [("regrow-and-bad-arguments", "dense-ls-regrow", False, [v]) for v in ("f32", "K=2")]
    out += [("regrow-and-bad-arguments", "dense-ls", False, [v]) for v in BAD]
    out += [("regrow-and-bad-arguments", "dense-ls-b8", False, ["K=2", "multinomial"])]
    return out


def load_golden():
    """(the head line: the parent commit, [[group, base, initialised, calls, [plan at creation, [code, plan] per call]]])"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_options_parent.jsonl")) as f:
        head, *lines = [json.loads(line) for line in f]
    return head, lines


def option_of(call):
    return call.replace("+", "=").split("=")[0]


def decode(call):
    """(option index, value, pointer: 0 none / NULL, 1 aligned, 2 offset by 8 bytes, K)"""
    name = option_of(call)
    arg = call[len(name):]
    value, ptr, K = 0.0, 0, 0
    if name in ("l2", "huber"):
        value = float(arg[1:])
    elif name == "K":
        K = int(arg[1:])
    elif name in ("pf", "roww", "f32"):
        ptr = {"": 1, "=NULL": 0, "+8": 2}[arg]
    return OPTIONS.index(name), value, ptr, K


# ---- with a device ----------------------------------------------------------------------------------------------------------------
SOLVER_OPTIONS = dict(lr=1.0, tol=0.0, tol_internal=1e-12, decay_rate=0.5, max_iter=3, max_backtrack_iter=10)


class Driver:
    """Creates the base solvers on buffers of its own and applies calls to them through the C ABI of `lib` (zfista_amd._lib.load())."""

    def __init__(self):
        import ctypes as C

        import numpy as np
        import scipy.sparse as sp
        import torch

        from zfista_amd import _lib
        from zfista_amd import problems as Z

        self.C, self.torch, self._lib = C, torch, _lib
        self.lib = _lib.require_gpu()
        f64 = dict(dtype=torch.float64, device="cuda")
        self.A = torch.zeros(512 * 20000, **f64)     # every dense matrix, and every matrix stored in fp32
        self.b = torch.zeros(1024 + 2, **f64)
        self.ones = torch.ones(20000 + 2, **f64)     # factors and weights
        self.x0 = torch.zeros(64, **f64)
        self.taps = torch.zeros(9, **f64)
        self.taps[4] = 1.0
        eye = lambda n: sp.identity(n, format="csr")   # noqa: E731
        self.sparse = {   # (the problem classes own the handles)
            4: Z.SparseLeastSquaresL1(eye(64), np.zeros(64), 0.1), 6: Z.SparseLogisticL1(eye(64), np.ones(64), 0.1),
            (4, 2): Z.SparseMultiResponseLeastSquaresL1(eye(32), np.zeros((32, 2)), 0.1),
            (6, 2): Z.SparseMultiResponseLogisticL1(eye(32), np.ones((32, 2)), 0.1)}

    def create(self, base):
        C, _lib, B = self.C, self._lib, BASES[base]
        kind = B["kind"]
        fields = dict(kind=kind, world=B["world"], rank=0, n=B["n"], m_rows=B["m_rows"], row_sharded=0, d=None, c=None, A=None,
                      b=self.b.data_ptr() + B["b_off"], scale=0.5, lam=0.1, box_lo=-math.inf, box_hi=math.inf)
        if kind in (2, 5):
            fields["A"] = self.A.data_ptr()
        elif kind == 1:
            fields.update(d=self.ones.data_ptr(), c=self.b.data_ptr(), b=None)
        elif kind == 3:
            fields.update(op_h=8, op_w=8, op_k=3, op_taps=self.taps.data_ptr())
        d, o, h = _lib.ProblemDesc(), _lib.Options(), C.c_void_p()
        for k, v in fields.items():
            setattr(d, k, v)
        for k, v in dict(SOLVER_OPTIONS, accept_mode=B["accept"]).items():
            setattr(o, k, v)
        stream = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        if kind in (4, 6) and B["K0"]:
            spmat = C.c_void_p(self.sparse[kind, B["K0"]]._spmat.value.value)
            rc = self.lib.zf_solver_create_sparse_responses(C.byref(h), C.byref(d), spmat, B["K0"], C.byref(o), stream)
        elif kind in (4, 6):
            rc = self.lib.zf_solver_create_sparse(C.byref(h), C.byref(d), C.c_void_p(self.sparse[kind]._spmat.value.value), C.byref(o), stream)
        else:
            rc = self.lib.zf_solver_create(C.byref(h), C.byref(d), C.byref(o), stream)
        assert rc == 0, (base, self.lib.zf_last_error())
        return h

    def plan(self, h):
        out = (self.C.c_int64 * 6)()
        assert self.lib.zf_solver_ls_plan(h, out, 6) == 0
        return list(out)

    def call(self, h, call):
        C, lib = self.C, self.lib
        index, value, ptr, K = decode(call)
        name = OPTIONS[index]
        fn = getattr(lib, ENTRY[name])
        if name in ("l2", "huber"):
            return fn(h, C.c_double(value))
        if name == "K":
            return fn(h, C.c_int32(K))
        if name in ("poisson", "multinomial"):
            return fn(h)
        buf = self.A if name == "f32" else self.ones
        return fn(h, C.c_void_p(buf.data_ptr() + (8 if ptr == 2 else 0)) if ptr else None)

    def run(self, base, init, calls):
        """[plan at creation, [rc, plan] per call]"""
        h = self.create(base)
        try:
            out = [self.plan(h)]
            if init:
                assert self.lib.zf_solver_enqueue_init(h, self.C.c_void_p(self.x0.data_ptr())) == 0, self.lib.zf_last_error()
            for c in calls:
                rc = self.call(h, c)
                out.append([rc, self.plan(h)])
            return out
        finally:
            self.lib.zf_solver_destroy(h)
