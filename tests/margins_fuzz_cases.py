"""Seeded option sweep of the six margins classes (SparseLeastSquaresL1 / LeastSquaresL1, SparseLogisticL1 / LogisticL1,
SparseHuberL1 / HuberL1): the case table shared by tests/test_margins_fuzz_cases.py (CPU: the table is sound) and
tests/test_gpu_fuzz_margins.py (GPU: the classes against the oracle on it).  No test in here.

A case is (class, seed).  ``draw`` turns it into a shape, the problem options (scale, box, l2), a starting point and the solver
options - draws only, no matrix - and ``build`` adds the matrix in CSR form, the right-hand side or labels and lam.  Each case
runs on both storage forms against ONE oracle run (``oracle``: the closures over the CSR matrix).

What decides which kernels and which branches of the trial state machine run is laid out over the seed, so that 24 consecutive
seeds hold every combination whatever the random draws give (tests/test_margins_fuzz_cases.py counts them):

  shape       SHAPES[seed % 5]
  l2          L2_FACTORS[(seed // 5) % 3] lam: every shape meets every l2 within 15 seeds (the small dense form needs l2 = 0)
  deprecated  seed % 5 == (seed // 5) % 5: a fifth, on another shape each time
  decay_rate  DECAY_RATES[(seed + seed // 4) % 4]: a quarter each, and each kind below meets all four
  seed % 4    0  few trials: max_backtrack_iter 1, 2 or 5 and lr from the upper half of its range - "Backtracking failed" at once or
                 after some accepted iterations, or a line search that just gets by
              1  the box (-0.05, 0.3); two of three start at 0.5 + 0.1 N(0, 1), outside it: g(x0) = inf
              2  a run meant to end by tol: tol 3e-2 or 1e-1 (the solutions' |x|_inf is 0.3 .. 3), max_iter 60, 100 trials.  The
                 existing fuzz's {0, 1e-4, 1e-7} hardly ever end a run of <= 60 iterations of these problems
              3  max_iter 1 or 2

The rest is drawn as ``_options`` of tests/test_gpu_fuzz_parity.py draws it, with these differences:

  lr        10^U(lo, hi) with (lo, hi) per class (LR_RANGE).  From lr = 1 the least-squares matrices backtrack 5 - 12 times at
            decay_rate 0.5: acceptable steps lie in 2^-12 .. 2^-5, the lower third of the range is accepted at once and the upper
            end needs ~70 trials at decay_rate 0.9.  The logistic loss (curvature <= scale / 4) and Huber's (a bounded gradient)
            accept steps 3 and 10 times as long, so their ranges are moved up by as much.  With decay_rate 0.9 lr comes from the
            upper half and max_backtrack_iter is 100 in 6 of 10 draws: a decay rate only shows where trials are rejected, and it
            is there that trials are rejected in later iterations too.
  max_iter  3 .. 60 (kinds 0 - 2).  decay_rate = 1 accepts every trial whatever lr is, and an lr beyond 2 / L multiplies the iterate
            by up to lr L ~ 1e4 per iteration: those runs are limited to 12 iterations, where F is far from overflow.
  tol       0, 1e-7, 1e-4, 1e-2, 1e-1
  x0        zeros, 0.1 N(0, 1) or 0.5 + 0.1 N(0, 1)

The stagnation rule is the existing fuzz's, unchanged: a run is cut one iteration before F first stops changing at
64 eps max(1, |F|) - beyond that point the reference's own acceptance test compares rounding residues."""
import contextlib
import functools
import io
import warnings
from collections import namedtuple

import numpy as np

import enet_cases as E
import huber_cases as H
import logistic_cases as L
import sparse_cases as S
from oracle import cpu_ref, problems_ref as P

CLASSES = ("ls", "logit", "huber")
FORMS = ("csr", "dense")
# (m, n, density, seed).  As dense matrices the three SMALL shapes reach the VALU column sweeps only (n % 32 != 0); 48 x 96 takes
# the fused small-matrix form (least squares without l2) and 4097 x 64 the MFMA sweep one row beyond what that form allows.
SHAPES = [S.SMALL[0], S.SMALL[2], S.SMALL[3], (48, 96, 0.2, 5), (4097, 64, 0.05, 6)]
SCALES = {"ls": (0.5, 1 / 6), "logit": (1.0, 1 / 3), "huber": (H.SCALE,)}   # what each class's own tests use
BOX = (-0.05, 0.3)
LR_RANGE = {"ls": (-3.5, 0.5), "logit": (-3.0, 1.0), "huber": (-2.5, 1.5)}   # log10 of lr
L2_FACTORS = (0.0, 0.01, 1.0)
STARTS = ("zero", "near", "shifted")
DECAY_RATES = (0.3, 0.5, 0.9, 1.0)
SEED_BASE = {"ls": 7000, "logit": 8000, "huber": 9000}
BLOCK = 24                      # seeds per class of the fixed table, and of every further ZF_FUZZ_SCALE block
# The fixed table: the first BLOCK seeds per class, counted from 0, that tests/test_margins_fuzz_cases.py accepts.  82 seeds were
# examined and 10 replaced (ls 12, 19, 22, 25; logit 6, 17; huber 6, 20, 21, 25).  None of the 10 was decided differently by the
# two CPU evaluations - lr and trial sequences agree on all 82 - but one iterate of theirs differs by 3.2e-15 .. 9.3e-15 of its norm
# between the two, beyond the 3e-15 the table asks for: steps with lr |grad f| >> |x| (the rounding of the gradient is multiplied
# by lr), among them runs at decay_rate = 1 with an lr of several times 2 / L.
SEEDS = {
    "ls": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 20, 21, 23, 24, 26, 27],
    "logit": [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 19, 20, 21, 22, 23, 24, 25],
    "huber": [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 22, 23, 24, 26, 27],
}
TABLE = [(cls, seed) for cls in CLASSES for seed in SEEDS[cls]]

# zf_solver_ls_plan out[0] (tests/test_gpu_dense_ls_paths.py); CSR = the sparse classes
SMALL_FORM, MFMA, VALU2, VALU1, CSR = 1, 2, 3, 4, 5
FORM_NAMES = {SMALL_FORM: "small", MFMA: "mfma", VALU2: "valu2", VALU1: "valu1", CSR: "csr"}

Spec = namedtuple("Spec", "cls seed shape scale bounds l2fac start x0_seed options")
Case = namedtuple("Case", "spec A b lam delta l2 x0")


def solver_options(rng, cls, decay_rate, kind=None):
    lo, hi = LR_RANGE[cls]
    late = decay_rate == 0.9    # (the module docstring: lr)
    o = dict(
        lr=float(10 ** rng.uniform((lo + hi) / 2 if late else lo, hi)),
        tol=float(rng.choice([0.0, 1e-7, 1e-4, 1e-2, 1e-1])),
        max_iter=int(rng.integers(1, 3)) if kind == "short" else int(rng.integers(3, 61)),
        max_backtrack_iter=int(rng.choice([1, 2, 5, 100], p=(0.1, 0.1, 0.2, 0.6) if late else (0.2, 0.2, 0.2, 0.4))),
        decay_rate=decay_rate,
        nesterov=bool(rng.integers(0, 2)),
        nesterov_ratio=tuple(map(float, rng.choice([(0, 0.25), (0.5, 0.25), (0.25, 1 / 64)]))),
        tol_internal=float(rng.choice([1e-12, 1e-6, 0.0])),
    )
    if kind == "few_trials":
        o.update(lr=float(10 ** rng.uniform((lo + hi) / 2, hi)), max_backtrack_iter=int(rng.choice([1, 2, 5])))
    if kind == "to_tol":
        o.update(tol=float(rng.choice([3e-2, 1e-1])), max_iter=60, max_backtrack_iter=100)
    if decay_rate == 1.0:
        o["max_iter"] = min(o["max_iter"], 12)
    return o


KINDS = {0: "few_trials", 2: "to_tol", 3: "short"}   # by seed % 4 (1: the box)


def draw(cls, seed):
    """The case's draws (no matrix is built): the module docstring's layout over the seed, the rest from the seeded generator."""
    rng = np.random.default_rng(SEED_BASE[cls] + seed)
    shape = SHAPES[seed % 5]
    l2fac = L2_FACTORS[(seed // 5) % 3]
    bounds = BOX if seed % 4 == 1 else None
    deprecated = seed % 5 == (seed // 5) % 5
    decay_rate = DECAY_RATES[(seed + seed // 4) % 4]
    scale = float(rng.choice(SCALES[cls]))
    if bounds is not None:
        start = "shifted" if (seed // 4) % 3 != 1 else STARTS[(seed // 12) % 2]
    else:
        start = STARTS[int(rng.integers(3))]
    x0_seed = int(rng.integers(1 << 31))
    options = dict(solver_options(rng, cls, decay_rate, KINDS.get(seed % 4)), deprecated=deprecated)
    return Spec(cls, seed, shape, scale, bounds, l2fac, start, x0_seed, options)


@functools.lru_cache(maxsize=None)
def data(cls, shape):
    """(A csr, b, lam, delta or None) of one class on one shape - read-only, shared by every case on it."""
    if cls == "ls":
        return S.make_sparse(*shape) + (None,)
    if cls == "logit":
        return L.make_logistic(*shape) + (None,)
    return H.make_huber(shape)


@functools.lru_cache(maxsize=None)
def dense(cls, shape):
    return data(cls, shape)[0].toarray()


def start_point(spec):
    n = spec.shape[1]
    z = np.random.default_rng(spec.x0_seed).standard_normal(n)
    return np.zeros(n) if spec.start == "zero" else 0.1 * z if spec.start == "near" else 0.5 + 0.1 * z


def build(spec):
    A, b, lam, delta = data(spec.cls, spec.shape)
    return Case(spec, A, b, lam, delta, spec.l2fac * lam, start_point(spec))


def outside_box(case):
    lo, hi = case.spec.bounds or (-np.inf, np.inf)
    return bool((case.x0 < lo).any() or (case.x0 > hi).any())


def dense_form(spec):
    """zf_solver_create's choice for the dense class of this case (zfista_amd/csrc/zf_solver.hip), restated: the fused
    small-matrix kernels hold the l1 step of the squared loss only."""
    m, n = spec.shape[:2]
    if n % 32 == 0:
        small = spec.cls == "ls" and spec.l2fac == 0.0 and m <= 4096 and m * n <= 1 << 22
        return SMALL_FORM if small else MFMA
    return VALU2 if n % 2 == 0 else VALU1


def case_id(spec):
    """class - seed - shape - storage forms (CSR and the dense form the shape takes) - box - l2"""
    tags = ["box"] * (spec.bounds is not None) + ["l2"] * (spec.l2fac > 0)
    return "-".join([spec.cls, f"s{spec.seed:02d}", f"{spec.shape[0]}x{spec.shape[1]}", "csr+" + FORM_NAMES[dense_form(spec)]] + tags)


def make_ref(case, storage, form="stable"):
    """The reference closures of a case over the CSR matrix or its .toarray(); ``form``: logistic_cases.LogisticL1Ref's."""
    sp_ = case.spec
    A = case.A if storage == "csr" else dense(sp_.cls, sp_.shape)
    if sp_.cls == "huber":
        return H.HuberRef(A, case.b, case.lam, case.delta, sp_.scale, sp_.bounds, case.l2)
    if case.l2 > 0:
        ref = E.EnetRef(sp_.cls, A, case.b, case.lam, case.l2, sp_.scale, sp_.bounds)
        if sp_.cls == "logit":
            ref.base.form = form
        return ref
    if sp_.cls == "logit":
        return L.LogisticL1Ref(A, case.b, case.lam, sp_.scale, sp_.bounds, form)
    cls = S.SparseLeastSquaresL1Ref if storage == "csr" else P.LeastSquaresL1Ref
    return cls(A, case.b, case.lam, sp_.scale, sp_.bounds)


def make_problem(case, storage):
    """The device problem of a case in one storage form."""
    from zfista_amd import problems as Z

    sp_ = case.spec
    A = case.A if storage == "csr" else dense(sp_.cls, sp_.shape)
    if sp_.cls == "huber":
        cls = Z.SparseHuberL1 if storage == "csr" else Z.HuberL1
        return cls(A, case.b, case.lam, case.delta, scale=sp_.scale, bounds=sp_.bounds, l2=case.l2)
    if sp_.cls == "ls":
        cls = Z.SparseLeastSquaresL1 if storage == "csr" else Z.LeastSquaresL1
        return cls(A, case.b, case.lam, scale=sp_.scale, bounds=sp_.bounds, l2=case.l2)
    cls = Z.SparseLogisticL1 if storage == "csr" else Z.LogisticL1
    prob = cls(A, case.b, case.lam, scale=sp_.scale, bounds=sp_.bounds)
    return prob.with_penalty(case.lam, case.l2) if case.l2 > 0 else prob


def run_ref(case, storage, form, options):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):   # ("An error occurred: ...")
            return cpu_ref.minimize_proximal_gradient(*make_ref(case, storage, form).callbacks(), case.x0, return_all=True, **options)


def stagnation_cut(exp):
    """The existing fuzz's rule: None (no cut), or the max_iter that ends the run one iteration before F first stagnates
    (0: x0 is already at the resolution limit of the acceptance test - such a case has nothing left)."""
    F = np.asarray(exp.allfuns, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        stalled = np.flatnonzero(np.abs(np.diff(F)) <= 64 * np.finfo(float).eps * np.maximum(1.0, np.abs(F[1:])))
    if stalled.size and stalled[0] + 1 <= exp.nit:
        return int(stalled[0])
    return None


_ORACLE = {}


def oracle(spec):
    """(case, options after the stagnation cut, the oracle's result on the stable closures over the CSR matrix): one run per
    case, shared by both storage forms and both test files; read-only."""
    key = (spec.cls, spec.seed)
    if key not in _ORACLE:
        case = build(spec)
        o = dict(spec.options)
        exp = run_ref(case, "csr", "stable", o)
        cut = stagnation_cut(exp)
        if cut is not None:
            o["max_iter"] = cut
            exp = run_ref(case, "csr", "stable", o) if cut >= 1 else None
        _ORACLE[key] = (case, o, exp)
    return _ORACLE[key]


def other_form(spec):
    """The second CPU evaluation of a case, under the cut options: the closures over .toarray() (logistic: np.logaddexp /
    expit with the loss summed in reverse)."""
    case, o, _ = oracle(spec)
    return run_ref(case, "dense", "library", o)


def disagreement(a, b):
    """None if two oracle runs took the same decisions and stayed within the bound of tests/test_oracle_golden_logistic.py for
    the same comparison (3e-15, norm-relative, every iterate); else what differs."""
    for k in ("nit", "success", "message"):
        if a[k] != b[k]:
            return f"{k}: {a[k]!r} != {b[k]!r}"
    if ("status" in a) != ("status" in b) or a.get("status") != b.get("status"):
        return "status"
    if list(a.alllrs) != list(b.alllrs):
        return "alllrs"
    if list(a.alltrials) != list(b.alltrials):
        return "alltrials"
    for k, (u, v) in enumerate(zip(list(a.allvecs) + [a.x], list(b.allvecs) + [b.x])):
        if not np.linalg.norm(u - v) <= 3e-15 * max(np.linalg.norm(v), 1.0):
            return f"iterate {k}: {np.linalg.norm(u - v) / max(np.linalg.norm(v), 1.0):.3g}"
    return None


def ending(exp):
    """"error" (the error-shaped result), "tol" or "max_iter"."""
    if exp.message.startswith("Error: "):
        return "error"
    return "tol" if exp.success else "max_iter"


def resume_cases():
    """[(spec, kind)]: per class the table's longest run that ends by tol and its longest that ends in the error path - the cases
    whose snapshot / resume the GPU test checks."""
    out = []
    for cls in CLASSES:
        runs = [(draw(c, s), oracle(draw(c, s))[2]) for c, s in TABLE if c == cls]
        for kind in ("tol", "error"):
            nit, spec = max(((exp.nit, sp) for sp, exp in runs if ending(exp) == kind), key=lambda t: (t[0], -t[1].seed))
            out.append((spec, kind))
    return out


def extra_block(k):
    """Block k >= 1 of further seeds (ZF_FUZZ_SCALE): outside the CPU-checked table, so a case whose two CPU evaluations disagree,
    or that the stagnation cut leaves without a run, is dropped here - before any GPU work."""
    keep = []
    for cls in CLASSES:
        for seed in range(1000 * k, 1000 * k + BLOCK):
            spec = draw(cls, seed)
            _, _, exp = oracle(spec)
            if exp is None or (ending(exp) != "error" and exp.nit < 1) or disagreement(exp, other_form(spec)) is not None:
                continue
            keep.append((cls, seed))
    return keep
