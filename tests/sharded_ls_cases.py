"""Sharded dense least squares (LeastSquaresL1 with world > 1, column blocks and row blocks): the case tables, the CPU closures
that sum in rank order, and the one-thread lockstep driver shared by tests/test_sharded_ls_cases.py (CPU: the tables are sound)
and tests/test_gpu_sharded_ls.py (GPU: the kernels against the oracle on them).  No test in here.

SHAPE_CASES   ten shapes with uneven splits.  Each names, per rank, the zf_solver_ls_plan it must report: ``dispatch`` restates
              zf_solver_create's rule for world > 1 (the small form is world-1 only; a column block is seen as m x n_p, a row
              block as m_p x n).
SWEEP         2 x 24 seeded option cases.  Case i of a layout takes shape SWEEP_SHAPES[i % 6] and the levels LAYOUT[layout][i]
              of world, split kind, box and starting point; everything else is drawn from the seed SEEDS[layout][i] as
              ``_options`` of tests/test_gpu_fuzz_parity.py draws it, with the lr range of its least-squares sweep.  The levels
              are laid out so that every pair of levels of two different factors occurs per layout, with two exceptions that 24
              cases cannot hold: shape x split kind has 30 pairs (24 distinct ones occur: no pair twice), and a world larger
              than the dimension that is split does not exist ((3, 1) by rows: world <= 3; (3, 4) by columns: world <= 4 -
              the case then takes the dimension as its world).
THREAD_CASES  three cases per layout for the library's own sequence through LibComm.local_group.

The stagnation rule is the existing fuzz's, unchanged and applied HERE, on the CPU: a run is cut one iteration before F first
stops changing at 64 eps max(1, |F|) (tests/margins_fuzz_cases.py: stagnation_cut).  A seed the cut would empty, or whose two CPU
evaluations (LeastSquaresL1Ref, and ShardedLSRef with its rank-ordered sums) do not decide alike, is replaced in SEEDS."""
import contextlib
import functools
import io
import warnings
from collections import namedtuple

import numpy as np

from margins_fuzz_cases import disagreement, ending, stagnation_cut   # noqa: F401  (re-exported: one criterion, one rule)
from oracle import cpu_ref, problems_ref as P

U = 2.0 ** -53
SMALL, MFMA, VALU2, VALU1 = 1, 2, 3, 4          # zf_solver_ls_plan out[0] (tests/test_gpu_dense_ls_paths.py)
ROWS_SMALL, ROWS_V2, ROWS_V1 = 1, 2, 3          # out[1]
ROW_SWEEP_LOOPS = 32768                         # zf_gemv_rows_kernel loops over rows beyond this many
BOXES = (None, (-0.05, 0.08), (0.01, 0.5))      # none, active on many coordinates, excludes 0 (test_gpu_dense_ls_paths.py)


def dispatch(m, n, world=1):
    """zf_solver_create's choice for an m x n block of a solve over ``world`` ranks (zfista_amd/csrc/zf_solver.hip), restated
    from ``dispatch`` of tests/test_gpu_dense_ls_paths.py with no switch set: the small form needs world == 1."""
    V = 2 if n % 2 == 0 else 1
    panels = -(-(n // V) // 256)
    slices = max(1, min(-(-2048 // panels), -(-m // 8), 64)) if panels else 1
    rps = -(-m // slices)
    slices = -(-m // rps)
    small = world == 1 and n % 32 == 0 and m <= 4096 and m * n <= 1 << 22
    form = SMALL if small else MFMA if n % 32 == 0 else VALU2 if V == 2 else VALU1
    rows = ROWS_SMALL if small else ROWS_V2 if V == 2 else ROWS_V1
    return form, rows, slices, rps


def bounds_of(parts):
    return [0] + [int(v) for v in np.cumsum(parts)]


def block_shapes(shape, parts, layout):
    m, n = shape
    return [(m, p) if layout == "columns" else (p, n) for p in parts]


ShapeCase = namedtuple("ShapeCase", "name layout shape parts scale plans what")

# name, layout, (m, n), n_p (columns) or m_p (rows) of each rank, scale, ls_plan of each rank, what the case reaches
SHAPE_CASES = [
    ShapeCase("C1", "columns", (200, 224), (128, 33, 62, 1), 0.5,
              ((MFMA, ROWS_V2, 25, 8), (VALU1, ROWS_V1, 25, 8), (VALU2, ROWS_V2, 25, 8), (VALU1, ROWS_V1, 25, 8)),
              "MFMA, VALU1, VALU2 and a one-column rank in one solve"),
    ShapeCase("C2", "columns", (40003, 66), (64, 2), 1 / 6,
              ((MFMA, ROWS_V2, 64, 626), (VALU2, ROWS_V2, 64, 626)),
              "the row sweep loops on both ranks; MFMA beside VALU2; the parts are added over 40003 rows"),
    ShapeCase("C3", "columns", (5, 8256), (4128, 4128), 0.5,
              ((MFMA, ROWS_V2, 1, 5), (MFMA, ROWS_V2, 1, 5)),
              "one rank alone would take the small form: each of two reports MFMA"),
    ShapeCase("C4", "columns", (300, 1000), (7, 961, 32), 1 / 6,
              ((VALU1, ROWS_V1, 38, 8), (VALU1, ROWS_V1, 38, 8), (MFMA, ROWS_V2, 38, 8)),
              "a split far from even"),
    ShapeCase("C5", "columns", (1, 3), (1, 1, 1), 0.5,
              ((VALU1, ROWS_V1, 1, 1),) * 3,
              "smallest"),
    ShapeCase("R1", "rows", (70001, 34), (40000, 30001), 1 / 6,
              ((VALU2, ROWS_V2, 64, 625), (VALU2, ROWS_V2, 64, 469)),
              "rank 0's sweeps loop over rows; VALU2"),
    ShapeCase("R2", "rows", (131, 4001), (1, 65, 65), 0.5,
              ((VALU1, ROWS_V1, 1, 1), (VALU1, ROWS_V1, 9, 8), (VALU1, ROWS_V1, 9, 8)),
              "VALU1; a one-row rank with one slice"),
    ShapeCase("R3", "rows", (1509, 128), (1500, 9), 0.5,
              ((MFMA, ROWS_V2, 63, 24), (MFMA, ROWS_V2, 2, 5)),
              "MFMA; 63 slices of 24 rows beside 2 slices"),
    ShapeCase("R4", "rows", (300, 1000), (3, 97, 100, 100), 1 / 6,
              ((VALU2, ROWS_V2, 1, 3), (VALU2, ROWS_V2, 13, 8), (VALU2, ROWS_V2, 13, 8), (VALU2, ROWS_V2, 13, 8)),
              "an uneven row split"),
    ShapeCase("R5", "rows", (2, 1), (1, 1), 0.5,
              ((VALU1, ROWS_V1, 1, 1),) * 2,
              "smallest"),
]
SHAPE_BY_NAME = {c.name: c for c in SHAPE_CASES}


@functools.lru_cache(maxsize=None)
def shape_data(shape):
    """(A, b, lam, ||A||_2^2) of one shape - read-only, shared by every test on it.  ||A||_2^2 is the largest eigenvalue of the
    smaller Gram matrix (exact to rounding: the step sizes of the element checks must lie on the right side of 1 / L).

    make_plasso's data as tests/test_gpu_dense_ls_paths.py draws it, but lam = 1e-5 max|A^T b| where A is tall.  A tall A is well
    conditioned: its FISTA reaches rounding level within 15 - 25 of the 30 iterations, and from there on the acceptance test
    compares residues of size eps |F| with tol_internal = 1e-12.  With lam_frac = 0.1 F stays at 5e3 .. 4e4 (lam |x|_1 with lam ~
    m / 10), the residues exceed the tolerance and the line search decides on the summation order - the two CPU evaluations
    already disagree on R1.  With 1e-5, F(x*) < 8 and the residues stay 500 times below the tolerance."""
    m, n = shape
    A, b, lam = P.make_plasso(m, n, seed=11, n_informative=max(1, min(20, n // 4)), lam_frac=1e-5 if m > n else 0.1)
    G = A @ A.T if m <= n else A.T @ A
    return A, b, lam, float(np.linalg.eigvalsh(G)[-1])


def accepted_lr(shape, scale):
    """A power of two <= 1 / (2 L), L = 2 scale ||A||_2^2: the first trial is accepted whatever the rounding."""
    sigma2 = shape_data(shape)[3]
    lr = 2.0 ** -int(np.ceil(np.log2(2 * 2 * scale * sigma2)))
    assert lr <= 1 / (2 * 2 * scale * sigma2)
    return lr


SOLVE_OPTIONS = dict(lr=1.0, tol=0.0, max_iter=30, nesterov=True)   # the solve of every shape case: FISTA, lr = 1 backtracks


def solve_x0(case):
    m, n = case.shape
    return 0.1 * np.random.default_rng(n * 31 + m).standard_normal(n)


@functools.lru_cache(maxsize=None)
def shape_oracle(name):
    """The oracle's 30 iterations on the UNSHARDED problem of a shape case: one run, shared by both test files; read-only."""
    case = SHAPE_BY_NAME[name]
    A, b, lam, _ = shape_data(case.shape)
    return run_ref(P.LeastSquaresL1Ref(A, b, lam, scale=case.scale), solve_x0(case), SOLVE_OPTIONS)


# --------------------------------------------------------------------------------------------------------------------------
# NumPy closures that sum the way the sharded solver does
# --------------------------------------------------------------------------------------------------------------------------
class ShardedLSRef:
    """f(x) = scale |Ax - b|^2, g = lam |x|_1 (+ box), evaluated block by block and added in RANK order: column blocks form A x
    as the sum of A_p x_p and g as the sum of the shards' g; row blocks form A^T r as the sum of A_p^T r_p and f as the sum of
    scale |r_p|^2 (x is replicated: g is rank 0's, the whole vector's).  A second summation order of LeastSquaresL1Ref."""

    def __init__(self, A, b, lam, splits, layout, scale=0.5, bounds=None):
        self.A, self.b = np.asarray(A, float), np.asarray(b, float)
        self.lam, self.scale, self.layout = float(lam), float(scale), layout
        self.bounds = None if bounds is None else (float(bounds[0]), float(bounds[1]))
        self.cut = [(int(lo), int(hi)) for lo, hi in zip(splits[:-1], splits[1:])]
        assert self.cut[0][0] == 0 and self.cut[-1][1] == self.A.shape[1 if layout == "columns" else 0]
        blocks = [self.A[:, lo:hi] if layout == "columns" else self.A[lo:hi] for lo, hi in self.cut]
        self.blocks = [np.ascontiguousarray(B) for B in blocks]

    def _Ax(self, x):
        parts = [B @ x[lo:hi] for B, (lo, hi) in zip(self.blocks, self.cut)]
        s = parts[0]
        for p in parts[1:]:
            s = s + p
        return s

    def _resid_rows(self, x):
        return [B @ x - self.b[lo:hi] for B, (lo, hi) in zip(self.blocks, self.cut)]

    def f(self, x):
        if self.layout == "columns":
            return self.scale * np.linalg.norm(self._Ax(x) - self.b) ** 2
        vals = [self.scale * np.linalg.norm(r) ** 2 for r in self._resid_rows(x)]
        f = vals[0]
        for v in vals[1:]:
            f = f + v
        return f

    def _g_of(self, x):
        if self.bounds is not None and ((x < self.bounds[0]).any() or (x > self.bounds[1]).any()):
            return np.inf
        return self.lam * np.linalg.norm(x, ord=1)

    def g(self, x):
        if self.layout == "rows":
            return self._g_of(x)
        vals = [self._g_of(x[lo:hi]) for lo, hi in self.cut]
        g = vals[0]
        for v in vals[1:]:
            g = g + v
        return g

    def jac_f(self, x):
        if self.layout == "columns":
            r = self._Ax(x) - self.b
            return (2 * self.scale) * np.concatenate([B.T @ r for B in self.blocks])
        parts = [(2 * self.scale) * (B.T @ r) for B, r in zip(self.blocks, self._resid_rows(x))]
        s = parts[0]
        for p in parts[1:]:
            s = s + p
        return s

    def prox_wsum_g(self, weight, x):
        x = P.soft_threshold(x, self.lam * weight)
        if self.bounds is not None:
            x = P.clip_box(x, self.bounds[0], self.bounds[1])
        return x

    def callbacks(self):
        return self.f, self.g, self.jac_f, self.prox_wsum_g


def run_ref(ref, x0, options):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):   # ("An error occurred: ...")
            return cpu_ref.minimize_proximal_gradient(*ref.callbacks(), x0, return_all=True, **options)


# --------------------------------------------------------------------------------------------------------------------------
# the option sweep
# --------------------------------------------------------------------------------------------------------------------------
SWEEP_SHAPES = {"rows": [(3, 1), (8, 5), (16, 33), (40, 64), (64, 128), (33, 257)],
                "columns": [(3, 4), (8, 5), (16, 33), (40, 64), (64, 128), (33, 257)]}   # (3, 1) has one column to split
WORLDS = (2, 3, 4, 5)
SPLIT_KINDS = ("even", "pm1", "one-first", "one-last", "random")
BOX_NAMES = ("nobox", "active", "excl0")
STARTS = ("zero", "random", "outside")
SEED_BASE = {"columns": 11000, "rows": 12000}
# per case i: the indices of (world, split kind, box, start) - found once by a search for pair coverage, fixed here
LAYOUT = {
    "rows": [(0, 2, 2, 2), (1, 2, 0, 0), (2, 2, 0, 0), (3, 0, 0, 1), (0, 4, 0, 2), (1, 0, 0, 2), (1, 0, 1, 1), (2, 4, 2, 1),
             (3, 4, 1, 1), (0, 1, 0, 1), (1, 3, 2, 1), (2, 1, 2, 2), (2, 4, 1, 0), (3, 3, 1, 2), (0, 0, 2, 2), (1, 4, 2, 2),
             (2, 0, 1, 0), (3, 2, 1, 1), (3, 3, 0, 2), (0, 1, 1, 1), (1, 1, 0, 0), (2, 3, 1, 0), (3, 1, 2, 0), (0, 3, 1, 0)],
    "columns": [(0, 3, 0, 0), (1, 2, 1, 2), (2, 3, 1, 1), (3, 0, 1, 0), (0, 4, 0, 2), (1, 3, 0, 0), (1, 0, 1, 2), (2, 1, 1, 1),
                (3, 4, 0, 2), (0, 1, 1, 1), (1, 3, 1, 0), (2, 4, 2, 1), (2, 1, 2, 1), (3, 3, 2, 2), (0, 2, 2, 2), (1, 4, 2, 1),
                (2, 0, 2, 1), (3, 1, 1, 2), (3, 4, 1, 0), (0, 0, 0, 0), (1, 1, 0, 0), (2, 2, 0, 2), (3, 2, 0, 1), (0, 2, 2, 0)],
}
# The seed of case i: i itself, or i + 24 k where i was replaced.  Two seeds were replaced because the two CPU evaluations, which
# decide alike on every seed examined, differ in one iterate by more than the 3e-15 the table asks for (rows 3: 3.2e-15, rows 23:
# 9.3e-15).  Thirteen more (columns 3, 6, 10, 18, 21, 23; rows 0, 6, 8, 12, 13, 16, 22) were replaced by the first later seed of
# their slot that is sound AND reaches a situation the plain draws reach fewer than three times per layout (a run ended by tol,
# a line search that fails after accepted iterations, a run of one iteration): ``_options`` draws those rarely.  616 seeds were
# examined in all (50 for the first pass over the 48 slots, 566 in the search for those situations).
SEEDS = {
    "columns": [0, 1, 2, 27, 4, 5, 150, 7, 8, 9, 154, 11, 12, 13, 14, 15, 16, 17, 138, 19, 20, 69, 22, 95],
    "rows": [48, 1, 2, 27, 4, 5, 102, 7, 104, 9, 10, 11, 36, 37, 14, 15, 64, 17, 18, 19, 20, 21, 118, 47],
}

Spec = namedtuple("Spec", "layout index seed shape world split_kind parts bounds start options")


def split_parts(kind, total, world, rng):
    """``world`` positive block sizes that add up to ``total``."""
    base, extra = divmod(total, world)
    if kind == "even":          # r * total // world, as every earlier test splits
        cut = [r * total // world for r in range(world + 1)]
        parts = [hi - lo for lo, hi in zip(cut[:-1], cut[1:])]
    elif kind == "pm1":         # sizes that differ by one at most, the larger blocks FIRST (the even split has them last)
        parts = [base + (1 if r < extra else 0) for r in range(world)]
    elif kind in ("one-first", "one-last"):
        rest = list(split_parts("pm1", total - 1, world - 1, rng)) if world > 1 else []
        parts = [1] + rest if kind == "one-first" else rest + [1]
    else:                       # a seeded random composition
        cuts = np.sort(rng.choice(np.arange(1, total), size=world - 1, replace=False)) if world > 1 else np.zeros(0, int)
        parts = [int(v) for v in np.diff(np.concatenate([[0], cuts, [total]]))]
    assert len(parts) == world and min(parts) >= 1 and sum(parts) == total, (kind, total, world, parts)
    return tuple(parts)


def _fuzz_options(rng):
    from test_gpu_fuzz_parity import _options

    o = _options(rng)
    o["lr"] = float(10 ** rng.uniform(-4, 0))   # the lr range of test_fuzz_least_squares_l1
    return o


def draw(layout, index, seed=None):
    """Case ``index`` of a layout: levels from LAYOUT, draws from its seed."""
    seed = SEEDS[layout][index] if seed is None else seed
    rng = np.random.default_rng(SEED_BASE[layout] + seed)
    shape = SWEEP_SHAPES[layout][index % 6]
    wi, ki, bi, xi = LAYOUT[layout][index]
    total = shape[1] if layout == "columns" else shape[0]
    world = min(WORLDS[wi], total)
    options = _fuzz_options(rng)
    parts = split_parts(SPLIT_KINDS[ki], total, world, rng)
    return Spec(layout, index, seed, shape, world, SPLIT_KINDS[ki], parts, BOXES[bi], STARTS[xi], options)


def spec_id(spec):
    box = BOX_NAMES[BOXES.index(spec.bounds)]
    return f"{spec.layout[:3]}-{spec.index:02d}-s{spec.seed}-{spec.shape[0]}x{spec.shape[1]}-w{spec.world}-{spec.split_kind}-{box}-{spec.start}"


@functools.lru_cache(maxsize=None)
def sweep_data(shape, seed):
    m, n = shape
    return P.make_plasso(m, n, seed=seed, n_informative=min(n, 5))   # as test_fuzz_least_squares_l1 builds it


def start_point(spec):
    """zero; random (inside the box where there is one, N(0, 1) otherwise); outside: the random point with coordinates pushed
    beyond the upper bound - in the column layout those of exactly ONE rank's shard, so that g = inf from one rank meets finite
    values from the others (no box: 0.5 + 0.1 N(0, 1), there is nothing to be outside of)."""
    n = spec.shape[1]
    rng = np.random.default_rng(SEED_BASE[spec.layout] + 500 + spec.seed)
    if spec.start == "zero":
        return np.zeros(n)
    z = rng.standard_normal(n)
    if spec.bounds is None:
        return z if spec.start == "random" else 0.5 + 0.1 * z
    lo, hi = spec.bounds
    x = rng.uniform(lo, hi, n)
    if spec.start == "outside":
        if spec.layout == "columns":
            cut = bounds_of(spec.parts)
            r = int(rng.integers(spec.world))
            sel = np.arange(cut[r], cut[r + 1])
        else:
            sel = np.flatnonzero(rng.random(n) < 0.5)
            sel = sel if sel.size else np.arange(1)
        x[sel] = hi + 0.1 * np.abs(z[sel]) + 0.01
    return x


def ranks_outside(spec, x0):
    """The ranks whose part of x0 (columns) lies outside the box; rows: every rank holds the whole x0."""
    if spec.bounds is None:
        return []
    lo, hi = spec.bounds
    bad = (x0 < lo) | (x0 > hi)
    if spec.layout == "rows":
        return list(range(spec.world)) if bad.any() else []
    cut = bounds_of(spec.parts)
    return [r for r in range(spec.world) if bad[cut[r]:cut[r + 1]].any()]


_ORACLE = {}


def oracle(spec):
    """(A, b, lam, x0, options after the stagnation cut, the oracle's result on the UNSHARDED problem - None if the cut leaves
    nothing): one run per case, shared by both test files; read-only."""
    key = (spec.layout, spec.index, spec.seed)
    if key not in _ORACLE:
        A, b, lam = sweep_data(spec.shape, spec.seed)
        x0 = start_point(spec)
        ref = P.LeastSquaresL1Ref(A, b, lam, bounds=spec.bounds)
        o = dict(spec.options)
        exp = run_ref(ref, x0, o)
        cut = stagnation_cut(exp)
        if cut is not None:
            o["max_iter"] = cut
            exp = run_ref(ref, x0, o) if cut >= 1 else None
        _ORACLE[key] = (A, b, lam, x0, o, exp)
    return _ORACLE[key]


def other_order(spec):
    """The second CPU evaluation of a case, under the cut options: ShardedLSRef on the case's own split."""
    A, b, lam, x0, o, _ = oracle(spec)
    return run_ref(ShardedLSRef(A, b, lam, bounds_of(spec.parts), spec.layout, bounds=spec.bounds), x0, o)


def sound(spec):
    """None if the case can stand in the table, else why not."""
    exp = oracle(spec)[5]
    if exp is None:
        return "x0 is already at the resolution limit of the acceptance test"
    if ending(exp) != "error" and exp.nit < 1:
        return "the stagnation cut left no iteration"
    if not (np.all(np.isfinite(np.asarray(exp.allfuns[1:], float))) and np.all(np.isfinite(exp.x))):
        return "the run overflows"
    other = other_order(spec)
    return disagreement(exp, other) or disagreement(other, exp)


def situations(spec):
    """What the case reaches, after the stagnation cut."""
    _, _, _, x0, o, exp = oracle(spec)
    end = ending(exp)
    got = {
        "ended by tol": end == "tol",
        "backtracking failed at once": end == "error" and exp.nit == 0,
        "backtracking failed after accepted iterations": end == "error" and exp.nit > 0,
        "one iteration": end != "error" and exp.nit == 1,
        "F(x0) = inf": not np.isfinite(exp.allfuns[0]),
        "decay_rate = 1": o["decay_rate"] == 1.0,
    }
    return {k for k, v in got.items() if v}


SITUATIONS = ("ended by tol", "backtracking failed at once", "backtracking failed after accepted iterations", "one iteration",
              "F(x0) = inf", "decay_rate = 1")
SWEEP = [draw(layout, i) for layout in ("columns", "rows") for i in range(24)]

# --------------------------------------------------------------------------------------------------------------------------
# the library's own sequence: thread ranks through LibComm.local_group
# --------------------------------------------------------------------------------------------------------------------------
ThreadCase = namedtuple("ThreadCase", "name layout shape parts scale bounds start options")
THREAD_CASES = [
    ThreadCase("split", "columns", (200, 224), (128, 33, 62, 1), 0.5, None, "zero", dict(lr=1.0, nesterov=True, tol=0.0, max_iter=25)),
    ThreadCase("box-ista", "columns", (96, 190), (95, 1, 94), 0.5, (-0.05, 0.08), "inside", dict(lr=1.0, nesterov=False, tol=0.0, max_iter=25)),
    ThreadCase("x0-tol", "columns", (96, 190), (63, 64, 63), 1 / 6, None, "random", dict(lr=1.0, nesterov=True, tol=1e-2, max_iter=200)),
    ThreadCase("split", "rows", (300, 1000), (3, 97, 100, 100), 1 / 6, None, "zero", dict(lr=1.0, nesterov=True, tol=0.0, max_iter=25)),
    ThreadCase("box-ista", "rows", (97, 190), (1, 48, 48), 0.5, (-0.05, 0.08), "inside", dict(lr=1.0, nesterov=False, tol=0.0, max_iter=25)),
    ThreadCase("x0-tol", "rows", (97, 190), (33, 32, 32), 1 / 6, None, "random", dict(lr=1.0, nesterov=True, tol=1e-2, max_iter=200)),
]


def thread_inputs(case):
    """(A, b, lam, x0) of a thread case."""
    m, n = case.shape
    A, b, lam = P.make_plasso(m, n, seed=2)
    rng = np.random.default_rng(m + n)
    if case.start == "zero":
        x0 = np.zeros(n)
    elif case.start == "inside":
        x0 = rng.uniform(case.bounds[0], case.bounds[1], n)
    else:
        x0 = 0.1 * rng.standard_normal(n)
    return A, b, lam, x0


# --------------------------------------------------------------------------------------------------------------------------
# the lockstep driver (GPU)
# --------------------------------------------------------------------------------------------------------------------------
Result = namedtuple("Result", "nit status success message x xs allvecs allfuns allerrs alllrs alltrials ctls steps")


class Lockstep:
    """``world`` DeviceSolver objects of one sharded least-squares solve, stepped in lockstep from ONE thread on one stream: the
    exchanges are device-to-device copies of _s_part -> _s_all and _pack_local -> _pack_all, in the order of DeviceSolver.init
    and DeviceSolver.enqueue.  No communicator, no barrier: a wrong kernel yields a wrong number, never a waiting rank.

    The constructor ends after init_begin (column blocks: every rank's _s_part holds A_p x0_p); ``finish_init`` does the rest
    of the initialisation, ``trial`` / ``finish_trial`` are the two halves of a step around the exchange of the s vectors, and
    ``run`` steps until the solve ends, polling every rank after each chunk."""

    def __init__(self, A, b, lam, parts, layout, x0, options, scale=0.5, bounds=None, timing=False):
        import torch

        from zfista_amd import _lib
        from zfista_amd.engine import DeviceSolver

        self._lib = _lib
        self.layout, self.rows = layout, layout == "rows"
        self.world = len(parts)
        self.cut = bounds_of(parts)
        m, n = A.shape
        assert self.cut[-1] == (m if self.rows else n) and min(parts) >= 1 and self.world >= 2
        o = dict(lr=1.0, tol=1e-5, tol_internal=1e-12, max_iter=1000, max_backtrack_iter=100, decay_rate=0.5, nesterov=False,
                 nesterov_ratio=(0, 0.25), deprecated=False) | dict(options)
        self.options = o
        opts = dict(lr=float(o["lr"]), tol=float(o["tol"]), tol_internal=float(o["tol_internal"]), decay_rate=float(o["decay_rate"]),
                    max_iter=int(o["max_iter"]), max_backtrack_iter=int(o["max_backtrack_iter"]), nesterov=int(bool(o["nesterov"])),
                    deprecated=int(bool(o["deprecated"])))
        # one trial per step: a solve that needs more steps than this does not end (a failure, not a wait)
        self.max_steps = int(o["max_iter"]) * int(o["max_backtrack_iter"])
        assert int(o["max_iter"]) + 1 <= _lib.ZF_RING, "the driver uploads every momentum factor up front"
        lo, hi = (-np.inf, np.inf) if bounds is None else bounds
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        self.solvers, self._keep = [], []
        b_full = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64)).cuda()
        for r in range(self.world):
            c0, c1 = self.cut[r], self.cut[r + 1]
            if self.rows:
                Ap = torch.from_numpy(np.ascontiguousarray(A[c0:c1])).cuda()
                bp = torch.from_numpy(np.ascontiguousarray(b[c0:c1], dtype=np.float64)).cuda()
                xp = torch.from_numpy(x0).cuda()
            else:
                Ap = torch.from_numpy(np.ascontiguousarray(A[:, c0:c1])).cuda()
                bp = b_full
                xp = torch.from_numpy(np.ascontiguousarray(x0[c0:c1])).cuda()
            fields = dict(kind=_lib.ZF_PROBLEM_LEAST_SQUARES_L1, world=self.world, rank=r, row_sharded=int(self.rows),
                          n=int(Ap.shape[1]), m_rows=int(Ap.shape[0]), d=None, c=None, A=Ap.data_ptr(), b=bp.data_ptr(),
                          scale=float(scale), lam=float(lam), box_lo=float(lo), box_hi=float(hi))
            s = DeviceSolver(fields, opts, keepalive=(Ap, bp), timing=timing)
            self._keep += [Ap, bp, xp]
            self.solvers.append(s)
        for s, xp in zip(self.solvers, self._keep[2::3]):
            s.init_begin(xp.data_ptr())
        self.initialised = False
        self.steps = 0
        self.seen = 0
        self.rows_seen = []      # trace rows of the accepted iterations, in order
        self.allvecs = [x0.copy()]
        self.F0 = None

    # -- the exchanges, as device-to-device copies (rank-major, as the all-gather lays them out) ------------------------------
    def exchange_svec(self):
        import torch

        allp = torch.cat([s._s_part for s in self.solvers])
        for s in self.solvers:
            s._s_all.copy_(allp)

    def exchange_pack(self):
        import torch

        allp = torch.cat([s._pack_local for s in self.solvers])
        for s in self.solvers:
            s._pack_all.copy_(allp)

    def s_parts(self):
        """Every rank's _s_part on the host."""
        import torch

        torch.cuda.synchronize()
        return [s._s_part.cpu().numpy().copy() for s in self.solvers]

    def finish_init(self):
        if not self.rows:        # (row blocks: A_p x0 is local, nothing to exchange at the start)
            self.exchange_svec()
        for s in self.solvers:
            s.init_finish()
        self.exchange_pack()
        for s in self.solvers:
            s.init_commit()
        o = self.options
        if o["nesterov"]:
            from zfista_amd.engine import momentum_factors

            K = int(o["max_iter"])
            betas = np.concatenate([[0.0], momentum_factors(K, tuple(o["nesterov_ratio"]))[0]])[:K + 1]
            for s in self.solvers:
                s.set_beta(0, betas)
        self.initialised = True
        ctls = self.poll()
        self.F0 = float(ctls[0].F_old)
        return ctls

    def trial(self):
        for s in self.solvers:
            s.enqueue_trial()

    def finish_trial(self):
        self.exchange_svec()
        for s in self.solvers:
            s.trial_finish()
        self.exchange_pack()
        for s in self.solvers:
            s.enqueue_decide()
        self.steps += 1

    def step(self):
        self.trial()
        self.finish_trial()

    def xs(self):
        return [s.get_x() for s in self.solvers]

    def x(self):
        xs = self.xs()
        return xs[0] if self.rows else np.concatenate(xs)

    def poll(self):
        """Poll every rank; all must hold the same control scalars and trace rows (row blocks: the same x too).  Collects the
        trace rows of the iterations accepted since the last poll; returns the control blocks."""
        L = self._lib
        got = [s.poll() for s in self.solvers]
        c0, t0 = got[0]
        key0 = (c0.nit, c0.status, c0.lr, c0.cur, c0.total_trials)
        for r, (ck, tk) in enumerate(got[1:], 1):
            key = (ck.nit, ck.status, ck.lr, ck.cur, ck.total_trials)
            assert key == key0, f"rank {r} holds (nit, status, lr, cur, total_trials) = {key}, rank 0 {key0}"
            assert np.array_equal(tk, t0, equal_nan=True), f"the trace rows of rank {r} differ from rank 0's"
        if self.rows:
            xs = self.xs()
            for r in range(1, self.world):
                assert np.array_equal(xs[r], xs[0], equal_nan=True), f"the replicated x of rank {r} differs from rank 0's"
        nit = int(c0.nit)
        if nit > self.seen:
            self.rows_seen += [t0[k % L.ZF_RING].copy() for k in range(self.seen, nit)]
            if nit == self.seen + 1 and len(self.allvecs) == self.seen + 1:
                self.allvecs.append(self.x())      # (chunk = 1: every iterate)
            self.seen = nit
        return [c for c, _ in got]

    def run(self, chunk=1):
        """Step until the solve ends.  chunk = 1 records every iterate."""
        L = self._lib
        if not self.initialised:
            self.finish_init()
        ctls = self.poll()
        while int(ctls[0].status) == L.ZF_RUNNING:
            assert self.steps < self.max_steps, (f"the solve has not ended after {self.steps} steps "
                                                 f"(max_iter x max_backtrack_iter = {self.max_steps})")
            for _ in range(min(chunk, self.max_steps - self.steps)):
                self.step()
            ctls = self.poll()
        return self.result(ctls)

    def result(self, ctls):
        L = self._lib
        c0 = ctls[0]
        status = int(c0.status)
        rows = np.array(self.rows_seen).reshape(-1, L.ZF_TRACE_COLS)
        if status == L.ZF_BACKTRACK_FAILED:
            success, message = False, "Error: " + cpu_ref.MSG_BACKTRACK
        elif status == L.ZF_CONVERGED:
            success, message = True, cpu_ref.MSG_SUCCESS
        else:
            assert status == L.ZF_MAXITER, status
            success, message = False, cpu_ref.MSG_MAXITER
        xs = self.xs()
        x = xs[0] if self.rows else np.concatenate(xs)
        vecs = self.allvecs if len(self.allvecs) == self.seen + 1 else None
        return Result(int(c0.nit), status, success, message, x, xs, vecs, [self.F0] + list(rows[:, L.TR_F]),
                      list(rows[:, L.TR_ERR]), list(rows[:, L.TR_LR]), [int(v) for v in rows[:, L.TR_TRIALS]], ctls, self.steps)

    def close(self):
        for s in self.solvers:
            s.close()
        self.solvers, self._keep = [], []


def compare_with_oracle(res, exp, tol=1e-10):
    """A driver Result against cpu_ref's result on the unsharded problem: decisions exactly, numbers to ``tol``."""
    assert res.message == exp.message and res.success == exp.success, (res.message, exp.message)
    assert res.nit == exp.nit, (res.nit, exp.nit)
    if ending(exp) == "error":
        assert res.status == 3 and "status" not in exp
    else:
        assert (res.status == 1) == (exp.status == 1)
    k = exp.nit
    assert list(res.alllrs) == [float(v) for v in exp.alllrs[:k]], "the lr sequence differs"
    assert list(res.alltrials) == [int(v) for v in exp.alltrials[:k]], "the trial sequence differs"
    scale = max(np.linalg.norm(exp.x), 1e-300)
    assert np.linalg.norm(res.x - exp.x) <= tol * scale or np.array_equal(res.x, exp.x)
    F_exp = np.asarray(exp.allfuns[:k + 1], float)
    F_got = np.asarray(res.allfuns, float)
    assert F_got.shape == F_exp.shape
    fin = np.isfinite(F_exp)
    assert np.array_equal(F_got[~fin], F_exp[~fin]), "F = inf (x0 outside the box) must be inf on the device too"
    np.testing.assert_allclose(F_got[fin], F_exp[fin], rtol=tol, atol=0)
    if k:
        # err = max|x+ - y| is a difference of iterates that agree to 1e-10 of their size
        xmax = max(1e-300, float(np.max(np.abs(np.stack(exp.allvecs[:k + 1])))))
        np.testing.assert_allclose(res.allerrs, exp.allerrs[:k], rtol=1e-9, atol=tol * xmax)
    if res.allvecs is not None:
        assert len(res.allvecs) == k + 1
        for j, (a, e) in enumerate(zip(res.allvecs, exp.allvecs)):
            assert np.linalg.norm(a - e) <= tol * max(np.linalg.norm(e), 1e-300) or np.array_equal(a, e), f"iterate {j}"
