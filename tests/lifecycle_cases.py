"""The lifecycle calls of a live solve - snapshot / from_snapshot (zf_solver_restore), set_max_iter, the streaming return_all ring
(zf_solver_set_history) with its host spill - on every path that decides or records in a kernel of its own: the case tables, their
inputs and their reference closures (no test in here; tests/test_lifecycle_cases.py keeps the tables honest on the CPU,
tests/test_gpu_lifecycle_paths.py runs them on the device).

    RESUME_SMALL   B1  the fused small-matrix path (zf_ls_small_step_kernel + zf_ls_small_rows_kernel): shapes that walk the loop
                       structure of the rows kernel's row dot, crossed with FISTA / ISTA, box, acceptance; and a small-eligible
                       shape whose passes do not run those kernels (tags split, comm)
    RESUME_OP      B2  the operator problem BlurHaarL1: every tile form, prox step fused into the adjoint kernel and apart
    RING           B3  a history ring smaller than the solve on every recording kernel outside the separable chains
    MAXITER        B4  set_max_iter on a live solve and a finished solve resumed with a larger max_iter

The REFERENCE of a case is oracle.cpu_ref.minimize_proximal_gradient on the closures the project already has
(oracle.problems_ref, oracle.operator_ref, sparse_cases, enet_cases, penalty_cases; K responses: LeastSquaresL1Ref on np.kron(A, I_K),
the problem multiresponse_cases states).  ``second`` is
the same problem evaluated in another order of the same sums - the matrix products in np.longdouble, rounded once; the
correlation of the operator problem on the transposed image with the transposed taps (SciPy then walks the window column by
column).  A case is in a table only if both evaluations decide every trial alike: what a device run departs from then is not a
summation order.

Seeds: a case whose two evaluations decided a trial differently was given the next seed (seed + 1); the number of replaced seeds
is REPLACED below (counted when the tables were drawn; the CPU test holds it to a tenth of the cases)."""
import contextlib
import io
import warnings

import numpy as np

import enet_cases as EN
import multiresponse_cases as M
import operator_exact as E
import penalty_cases as PC
import sparse_cases as S
from oracle import cpu_ref, operator_ref as O, problems_ref as P

LD = np.longdouble
BASE = dict(lr=1, tol=1e-5, tol_internal=1e-12, max_iter=1000000, max_iter_internal=100000, max_backtrack_iter=100,
            warm_start=False, decay_rate=0.5, nesterov=False, nesterov_ratio=(0, 0.25), return_all=False, verbose=False,
            deprecated=False)
# every switch that selects another kernel path for the problems of these tables: a test clears them all, then sets its case's
SWITCHES = ("ZF_LS_SMALL", "ZF_GEMV_MFMA", "ZF_OP_SEPARABLE", "ZF_OP_FUSE_PROX", "ZF_OP_PERSIST", "ZF_SUB_ITERS", "ZF_FORCE_SPLIT",
            "ZF_ACCEPT")
REPLACED = 1   # seeds replaced when the tables were drawn (_NEXT_SEED)
BOX = (-0.05, 0.08)
LR_REJECT = 64.0   # B1: a first step far beyond 1 / L - the first passes all reject

# ls_plan()[0] of the dense least-squares forms (zf_solver_ls_plan)
SMALL, MFMA, VALU2, VALU1, CSR = 1, 2, 3, 4, 5


# ---------------------------------------------------------------------------------------------------------------------------
# the rows kernel's row dot, restated: which loops a lane of the wave takes (csrc/zf_kernels_ls_small.h, zf_ls_small_row_dot)
# ---------------------------------------------------------------------------------------------------------------------------
def row_dot_walk(n):
    """{lane: (rounds of the unrolled loop, rounds of the tail loop)} for the n / 2 pairs of a row: lane l starts at pair l, takes
    eight pairs 64 apart per unrolled round while j + 448 < n / 2, then single pairs 64 apart."""
    out = {}
    for lane in range(64):
        j, un, tail = lane, 0, 0
        while j + 64 * 7 < n // 2:
            j += 64 * 8
            un += 1
        while j < n // 2:
            j += 64
            tail += 1
        out[lane] = (un, tail)
    return out


def small_path(m, n):
    """zf_solver_create's rule for the fused small-matrix path (world 1, plain least squares, the switch at its default)."""
    return n % 32 == 0 and m <= 4096 and m * n <= 1 << 22


# ---------------------------------------------------------------------------------------------------------------------------
# evaluations in another order
# ---------------------------------------------------------------------------------------------------------------------------
class _Closures:
    """Four callbacks and, for acceptance="remainder", the product A v the Taylor remainder is formed from."""

    def __init__(self, f, g, jac_f, prox, Ax=None, scale=None, f_diff=None):
        self.f, self.g, self.jac_f, self.prox_wsum_g, self.Ax, self.scale, self.f_diff = f, g, jac_f, prox, Ax, scale, f_diff

    def callbacks(self):
        return self.f, self.g, self.jac_f, self.prox_wsum_g


def _longdouble_square(ref, A, b, scale):
    """The squared loss of `ref` with every sum over A in np.longdouble, rounded to fp64 once; g and the prox are ref's."""
    Al = np.asarray(A.toarray() if hasattr(A, "toarray") else A, float).astype(LD)
    bl = np.asarray(b, float).astype(LD)

    def Ax(x):
        return (Al @ np.asarray(x, float).astype(LD)).astype(np.float64)

    def f(x):
        r = Al @ np.asarray(x, float).astype(LD) - bl
        return float(LD(scale) * np.sum(r * r))

    def jac_f(x):
        r = Al @ np.asarray(x, float).astype(LD) - bl
        return ((2 * LD(scale)) * (r @ Al)).astype(np.float64)

    return _Closures(f, ref.g, jac_f, ref.prox_wsum_g, Ax, scale)


def _remainder_diff(cl):
    """f(x+) - f(y) with the cancellation taken out, as tests/test_gpu_accept_remainder.py feeds the oracle's f_diff hook:
    R + <grad f(y), x+ - y>, R = scale |A (x+ - y)|^2 (the oracle subtracts the same dot product again)."""
    last = [None, None]

    def f_diff(x_new, y):
        if last[0] is not y:
            last[:] = [y, np.asarray(cl.jac_f(y)).reshape(-1)]
        step = x_new - y
        a = cl.Ax(step)
        return cl.scale * float(a @ a) + float(last[1] @ step)
    return f_diff


def _memo(fn, keep=4):
    """The oracle evaluates f and jac_f at the same array objects (x_k, y) several times per trial: the same values, computed
    once (the last `keep` arguments are held, so their ids stay theirs)."""
    seen = []

    def wrapped(x):
        for arg, val in seen:
            if arg is x:
                return val
        val = fn(x)
        seen.append((x, val))
        del seen[:-keep]
        return val
    return wrapped


# ---------------------------------------------------------------------------------------------------------------------------
# a case: one problem, one set of solver options, the path it must run on
# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """family: small | dense | csr | mr | enet | pf | diag | op.  ``shape``: (m, n) of the matrix families, (n,) of diag, (H, W, k, kind)
    of the operator.  ``x0``: zeros, or "random" (seeded, inside the box).  ``opts``: solver options on top of BASE.  ``env``: switches set for the device run.  ``snap``: B1 / B2, the
    snapshot points of the case - each one of "nit0" (three passes in: between a rejected trial and its retry), "nit1", "nit2"
    (the pass that accepted the first / second iterate), "mid" (the pass that accepted half of the run's iterates), or a number of passes; two of them: a
    resume of a resumed solve."""

    def __init__(self, family, shape, seed, opts, box=None, env=None, snap=(), tag="", make=None, x0="zeros"):
        self.x0kind = x0
        self.family, self.shape, self.seed, self.box, self.snap, self.tag = family, tuple(shape), seed, box, tuple(snap), tag
        self.opts = dict(opts)
        self.env = dict(env or {})
        self.make = dict(make or {})
        self._data = self._oracle = None

    @property
    def id(self):
        o = self.opts
        bits = [self.family, "x".join(str(s) for s in self.shape), "fista" if o.get("nesterov") else "ista"]
        if self.box:
            bits.append("box")
        if o.get("acceptance", "reference") != "reference":
            bits.append(o["acceptance"])
        bits += [f"{k[3:].lower()}{v}" for k, v in self.env.items()]
        if self.snap:
            bits.append("+".join(str(s) for s in self.snap))
        if self.tag:
            bits.append(self.tag)
        return "-".join(bits) + f"-s{self.seed}"

    # -- inputs ----------------------------------------------------------------------------------------------------------------
    def data(self):
        if self._data is None:
            self._data = self._make_data()
        return self._data

    def _make_data(self):
        fam, sh, seed = self.family, self.shape, self.seed
        if fam in ("small", "dense"):
            m, n = sh
            kw = dict(n_informative=max(1, min(20, n // 4)))
            kw.update(self.make)
            A, b, lam = P.make_plasso(m, n, seed=seed, **kw)
            return dict(A=A, b=b, lam=float(lam), scale=0.5)
        if fam in ("csr", "enet", "pf"):
            m, n, density = sh
            A, b, lam = S.make_sparse(m, n, density, seed)
            out = dict(A=A if fam == "csr" else A.toarray(), b=b, lam=float(lam), scale=0.5)
            if fam == "enet":
                out["l2"] = float(lam)
            if fam == "pf":
                p = PC.make_factors(n, seed, "positive")
                p[3] = 0.0   # one unpenalised column
                out["p"] = p
            return out
        if fam == "mr":
            m, n, K = sh
            A, B, lam = M.make("square", m, n, K, seed)
            return dict(A=A, B=B, lam=float(lam), scale=0.5, K=K)
        if fam == "diag":
            d, c, lam = P.make_pdiag(sh[0], seed=seed)
            return dict(d=d, c=c, lam=float(lam))
        if fam == "op":
            H, W, k, kind = sh
            rng = np.random.default_rng(seed)
            taps = E.make_self_adjoint_taps(rng, k, kind)
            return dict(taps=taps, observed=rng.standard_normal((H, W)), lam=0.5, scale=1.0)
        raise ValueError(fam)

    @property
    def n_features(self):
        fam, sh = self.family, self.shape
        return sh[0] if fam == "diag" else sh[0] * sh[1] if fam == "op" else sh[1] * sh[2] if fam == "mr" else sh[1]

    def x0(self):
        if self.family == "op":   # the notebook's start: the coefficients of the observed image (clipped into the box)
            x0 = O.dwt(self.data()["observed"])
            return np.clip(x0, *self.box) if self.box else x0
        if self.x0kind == "random":   # inside the box.  (A 0 = 0 in every summation order: a restore that rebuilds A x_0 with the
            rng = np.random.default_rng(self.seed + 5000)   # wrong kernel shows only from a start other than 0)
            return rng.uniform(0.8 * self.box[0], 0.8 * self.box[1], self.n_features) if self.box else 0.1 * rng.standard_normal(self.n_features)
        return np.zeros(self.n_features)

    # -- the reference closures and their second evaluation --------------------------------------------------------------------
    def ref(self):
        D, fam = self.data(), self.family
        if fam in ("small", "dense"):
            r = P.LeastSquaresL1Ref(D["A"], D["b"], D["lam"], D["scale"], self.box)
        elif fam == "csr":
            r = S.SparseLeastSquaresL1Ref(D["A"], D["b"], D["lam"], D["scale"], self.box)
        elif fam == "enet":
            r = EN.EnetRef("ls", D["A"], D["b"], D["lam"], D["l2"], D["scale"], self.box)
        elif fam == "pf":
            r = PC.PenaltyRef(D["A"], D["b"], D["lam"], D["p"], "square", scale=D["scale"], bounds=self.box)
        elif fam == "mr":
            r = P.LeastSquaresL1Ref(np.kron(D["A"], np.eye(D["K"])), D["B"].reshape(-1), D["lam"], D["scale"], self.box)
        elif fam == "diag":
            r = P.DiagQuadL1Ref(D["d"], D["c"], D["lam"])
            g, prox = _boxed(r.g, r.prox_wsum_g, self.box)
            return _Closures(r.f, g, r.jac_f, prox, f_diff=r.f_diff)
        else:
            return _Closures(*_operator_closures(D["taps"], D["observed"], D["lam"], D["scale"], self.box, transposed=False))
        A = r.A if hasattr(r, "A") else r.base.A
        return _Closures(r.f, r.g, r.jac_f, r.prox_wsum_g, (lambda v: A @ v), D["scale"])

    def second(self):
        D, fam = self.data(), self.family
        first = self.ref()
        if fam == "diag":
            d, c = D["d"].astype(LD), D["c"].astype(LD)

            def f(x):
                r = x.astype(LD) - c
                return float(LD(0.5) * np.sum(d * (r * r)))

            def f_diff(x_new, y):
                r, rn = y.astype(LD) - c, x_new.astype(LD) - c
                return float(LD(0.5) * np.sum((d * (x_new.astype(LD) - y.astype(LD))) * (rn + r)))

            return _Closures(f, first.g, first.jac_f, first.prox_wsum_g, f_diff=f_diff)
        if fam == "op":
            return _Closures(*_operator_closures(D["taps"], D["observed"], D["lam"], D["scale"], self.box, transposed=True))
        if fam == "mr":
            return _longdouble_square(first, np.kron(D["A"], np.eye(D["K"])), D["B"].reshape(-1), D["scale"])
        return _longdouble_square(first, D["A"], D["b"], D["scale"])

    # -- the oracle's run ------------------------------------------------------------------------------------------------------
    def solve(self, closures, **over):
        """oracle.cpu_ref on `closures` under the case's options (return_all; the device-only keys taken out; acceptance
        "remainder" / "resolved" through the oracle's f_diff hook)."""
        o = dict(BASE, **self.opts)
        o.update(over)
        mode = o.pop("acceptance", "reference")
        o.pop("sub_iters", None)
        f, g, jac_f, prox = closures.callbacks()
        cl = _Closures(_memo(f), g, _memo(jac_f), prox, closures.Ax, closures.scale, closures.f_diff)
        f_diff = _remainder_diff(cl) if mode == "remainder" else closures.f_diff if mode == "resolved" else None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with contextlib.redirect_stdout(io.StringIO()):
                res = cpu_ref.minimize_proximal_gradient(*cl.callbacks(), self.x0(), **dict(o, return_all=True), f_diff=f_diff)
        for v in res.allvecs:
            np.asarray(v).setflags(write=False)
        return res

    def oracle(self):
        """The reference run of the case, computed once and never modified."""
        if self._oracle is None:
            self._oracle = self.solve(self.ref())
        return self._oracle

    def passes_at(self, point):
        """Passes (= trials: these paths run one trial per pass) after which the snapshot `point` is taken."""
        exp = self.oracle()
        trials = list(exp.alltrials)
        if point == "nit0":   # (the first iterate takes at least two trials in every case of these tables: the CPU test says so)
            return min(3, trials[0] - 1)
        if point == "nit1":
            return trials[0]
        if point == "nit2":
            return trials[0] + trials[1]
        if point == "mid":   # the pass that accepted iterate nit / 2
            return sum(trials[:exp.nit // 2])
        return int(point)

    def nit_after(self, passes):
        """(accepted iterations after `passes` trials, whether the next trial is a retry) by the oracle's trial sequence."""
        done = 0
        for k, t in enumerate(self.oracle().alltrials):
            if done + t > passes:
                return k, passes > done
            done += t
        return len(self.oracle().alltrials), False

    # -- the device problem ----------------------------------------------------------------------------------------------------
    def problem(self, group=None):
        """The device problem; ``group``: a one-rank communicator (the small family only)."""
        from zfista_amd import problems as Z

        D, fam = self.data(), self.family
        if fam in ("small", "dense"):
            return Z.LeastSquaresL1(D["A"], D["b"], D["lam"], D["scale"], bounds=self.box, group=group)
        if fam == "csr":
            return Z.SparseLeastSquaresL1(D["A"], D["b"], D["lam"], D["scale"], bounds=self.box)
        if fam == "enet":
            return Z.LeastSquaresL1(D["A"], D["b"], D["lam"], D["scale"], bounds=self.box, l2=D["l2"])
        if fam == "pf":
            return Z.LeastSquaresL1(D["A"], D["b"], D["lam"], D["scale"], bounds=self.box, penalty_factor=D["p"])
        if fam == "mr":
            return Z.MultiResponseLeastSquaresL1(D["A"], D["B"], D["lam"], D["scale"], self.box)
        if fam == "diag":
            return Z.DiagQuadL1(D["d"], D["c"], D["lam"], bounds=self.box)
        return Z.BlurHaarL1(D["taps"], D["observed"], D["lam"], scale=D["scale"], bounds=self.box)

    def plan_ok(self, plan, responses=(1, 0)):
        """Whether ls_plan() (and responses_plan()) of the solver that ran the case show the path the case is about."""
        fam = self.family
        if fam == "small":
            return plan[0] == SMALL and plan[1] == 1
        if fam == "dense":
            return plan[0] == self.make_plan
        if fam == "csr":
            return plan[0] == CSR
        if fam == "op":
            H, W, k, kind = self.shape
            return plan[1] == int(kind == "separable") and plan[0] == self.tile_height
        if fam == "mr":   # the K-response sweeps: 9 / 10 - 16-byte / scalar loads of A - and K itself
            return plan[0] == (9 if self.shape[1] % 2 == 0 else 10) and responses[0] == self.shape[2]
        if fam in ("enet", "pf"):   # their setters take the solver off the small-matrix path: the general dense forms
            n = self.shape[1]
            return plan[0] == (MFMA if n % 32 == 0 else VALU2 if n % 2 == 0 else VALU1)
        if fam == "diag":
            return tuple(plan) == (0, 0, 0, 0)
        return False

    make_plan = None

    @property
    def tile_height(self):
        """zf_op_make_plan: 64 x 32 tiles once the image has 256 of them, else 64 x 8."""
        H, W = self.shape[:2]
        return 32 if -(-W // 64) * -(-H // 32) >= 256 else 8


def _boxed(g, prox, bounds):
    """g and the prox of a reference without a box, with one: g is inf outside it, the prox clips the thresholded point into it (as
    oracle.problems_ref.LeastSquaresL1Ref and _operator_closures do)."""
    if bounds is None:
        return g, prox

    def g_box(x):
        return np.inf if ((x < bounds[0]).any() or (x > bounds[1]).any()) else g(x)

    return g_box, (lambda weight, x: P.clip_box(prox(weight, x), bounds[0], bounds[1]))


def _operator_closures(taps, observed, lam, scale, bounds, transposed):
    """oracle.operator_ref's callbacks with scale and a box around them (as tests/test_gpu_operator_kernels.py); `transposed`:
    the correlation on the transposed image with the transposed taps - the same sums, SciPy's window walked column by column."""
    from scipy.signal import correlate2d

    ref = O.BlurHaarL1Ref(taps, observed, l1_ratio=lam)
    if transposed:
        tT = np.ascontiguousarray(ref.kernel.T)
        ref.blur = lambda img: np.ascontiguousarray(correlate2d(np.ascontiguousarray(img.T), tT, mode="same", boundary="symm").T)

    def g(x):
        if bounds is not None and ((x < bounds[0]).any() or (x > bounds[1]).any()):
            return np.array([np.inf])
        return ref.g(x)

    def prox(weight, x):
        p = ref.prox_wsum_g(weight, x)
        return p if bounds is None else np.clip(p, *bounds)

    return (lambda x: scale * ref.f(x)), g, (lambda x: scale * ref.jac_f(x)), prox


# ---------------------------------------------------------------------------------------------------------------------------
# B1: resume on the small-matrix path
# ---------------------------------------------------------------------------------------------------------------------------
# (m, n), max_iter, what the shape reaches in the row dot (tests/test_lifecycle_cases.py asserts it through row_dot_walk)
SMALL_SHAPES = [
    ((1, 32), 40, "16 pairs: lanes 0 .. 15 one tail round, the others none; one row, one wave of eight at work"),
    ((65, 128), 40, "one tail round per lane; the last workgroup holds one row of eight"),
    ((200, 960), 40, "lanes < 32 take the unrolled loop, the others seven tail rounds"),
    ((512, 1024), 30, "one unrolled round, no tail (BASELINE cfg1)"),
    ((96, 1056), 40, "an unrolled round, then a tail round for lanes < 16"),
    ((4096, 1024), 10, "both size limits at once (tall: ten iterations, before its line search decides on rounding noise)"),
]
_SNAPS = ("nit0", "nit1", "nit2", "mid")
# (m, n, nesterov, box, acceptance): the seed of a case whose two evaluations parted on seed 11 (counted in REPLACED).  The tall shape
# under the reference's test is at its resolution limit within ten iterations: one evaluation rejected a trial the other accepted.
_NEXT_SEED = {(4096, 1024, False, False, "reference"): 12}


def _resume_small():
    out = []
    for si, ((m, n), iters, _) in enumerate(SMALL_SHAPES):
        # the full cross: on every shape FISTA and ISTA each meet all four snapshot points (box x acceptance are the four
        # combinations of one momentum setting; the cycle starts one further on each shape, so a point meets every combination)
        for nest in (True, False):
            for j, (box, acc) in enumerate(((False, "reference"), (True, "remainder"), (True, "reference"), (False, "remainder"))):
                opts = dict(lr=LR_REJECT, nesterov=nest, tol=0.0, max_iter=iters, acceptance=acc)
                seed = _NEXT_SEED.get((m, n, nest, box, acc), 11)
                out.append(Case("small", (m, n), seed, opts, box=BOX if box else None, snap=(_SNAPS[(j + si) % 4],), x0="random"))
    # a resume of a resumed solve: snapshot, resume, snapshot again, resume again
    o = dict(lr=LR_REJECT, nesterov=True, tol=0.0, max_iter=40)
    out.append(Case("small", (65, 128), 12, dict(o, acceptance="reference"), snap=("nit1", "mid"), x0="random"))
    out.append(Case("small", (200, 960), 12, dict(o, acceptance="remainder"), box=BOX, snap=("nit2", "mid"), x0="random"))
    # a small-eligible shape whose passes do NOT run the fused kernels: the host-driven sequence trial / gather / decide
    # (ZF_FORCE_SPLIT=1) and a one-rank communicator.  Their margins all come from the general row sweep, and the restore must
    # rebuild them with it.
    for tag, env in (("split", {"ZF_FORCE_SPLIT": "1"}), ("comm", {})):
        for nest, snap in ((True, "mid"), (True, "nit2"), (False, "nit1")):
            out.append(Case("small", (200, 960), 13, dict(o, nesterov=nest, acceptance="reference"), env=env, snap=(snap,), x0="random",
                            tag=tag))
    # past the point where the reference's evaluation of the test has stalled (tests/test_gpu_accept_remainder.py, problem "D":
    # F ~ 7.7e6, decisions at the noise floor from about pass 120 on): 144 passes in, FISTA from lr = 1
    out.append(Case("small", (2048, 512), 0, dict(lr=1.0, nesterov=True, tol=0.0, max_iter=200, acceptance="remainder"), snap=(144,),
                    tag="stalled", make=dict(lam_frac=0.01, n_informative=200, noise=100.0)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# B2: resume of the operator problem
# ---------------------------------------------------------------------------------------------------------------------------
# (H, W, k, kind), max_iter, lr (the safe step of these taps is 0.5: sum |taps| = 1, scale 1), what the image reaches
OP_IMAGES = [
    ((100, 200, 9, "separable"), 12, 256.0, "52 tiles of 64 x 8"),
    ((100, 200, 7, "general"), 12, 256.0, "52 tiles of 64 x 8, the general correlation"),
    ((566, 950, 5, "separable"), 6, 64.0, "270 tall tiles, 54 columns / 22 rows in the last ones"),
    ((544, 960, 9, "separable"), 6, 64.0, "1020 tiles of 64 x 8: the workgroups of the apply kernel may walk (plan[2] recorded only)"),
    ((2, 2, 3, "general"), 12, 256.0, "one 2 x 2 block"),
    ((8, 8, 15, "separable"), 12, 256.0, "halo = image - 1: every row and column mirrored"),
]


def _resume_op():
    out = []
    k = 0
    for ii, (shape, iters, lr, _) in enumerate(OP_IMAGES):
        for nest in (True, False):
            for fuse in ("1", "0"):
                box = (-0.4, 0.4) if (ii == 1 and nest) else None
                opts = dict(lr=lr, nesterov=nest, tol=0.0, max_iter=iters)
                out.append(Case("op", shape, 21 + ii, opts, box=box, env={"ZF_OP_FUSE_PROX": fuse}, snap=(_SNAPS[k % 4],)))
                k += 1
            k += 1   # (fused and unfused of one image must not always share a snapshot point)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# B3: a ring that wraps.  One row per family x nesterov x box; every row is run with history_slots None, 5 and 1.
# ---------------------------------------------------------------------------------------------------------------------------
RING_SLOTS = (None, 5, 1)
# family, shape, seed, lr, tol, env, sub_iters, acceptance, the recording kernel of the family
RING_FAMILIES = [
    ("dense", (33, 70), 31, 8.0, 1e-4, {}, None, None, "the vector step ZF_LAUNCH_TRIAL(false, N, B, true, 1, true, 0, 0), VALU shape"),
    ("csr", S.SMALL[0][:3], S.SMALL[0][3], 8.0, 1e-4, {}, None, None, "the vector step behind the CSR sweeps"),
    ("mr", (33, 67, 3), 33, 8.0, 1e-4, {}, None, None, "the vector step on n K = 201 elements (stride 256)"),
    ("small", (65, 128), 34, 8.0, 1e-4, {}, None, None, "zf_ls_small_step_kernel (P.hist)"),
    ("enet", S.SMALL[0][:3], S.SMALL[0][3], 8.0, 1e-4, {}, None, None, "zf_trial_enet_kernel<N, B, true>"),
    ("pf", S.SMALL[0][:3], S.SMALL[0][3], 8.0, 1e-4, {}, None, None, "zf_trial_pf_kernel<N, B, true>"),
    ("diag", (10007,), 1, 4.0, 1e-6, {}, 1, "resolved", "zf_launch_res_single(v, true, ...)"),
    ("op", (100, 200, 9, "separable"), 38, 256.0, 2e-3, {}, None, None, "the operator's unfused step (fuse_prox && !s->hist)"),
]
RING_BOX = {"diag": (-1.0, 1.5), "op": (-0.4, 0.4)}   # (coefficients of unit size: BOX would pin them all within two iterations)


def _ring():
    out = []
    for fam, shape, seed, lr, tol, env, sub, acc, _ in RING_FAMILIES:
        for nest in (True, False):
            for boxed in (False, True):
                box = RING_BOX.get(fam, BOX) if boxed else None
                opts = dict(lr=lr, nesterov=nest, tol=tol, max_iter=400)
                if sub:
                    opts["sub_iters"] = sub
                if acc:
                    opts["acceptance"] = acc
                c = Case(fam, shape, seed, opts, box=box, env=env, tag="ring")
                if fam == "dense":
                    c.make_plan = VALU2
                out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# B4: set_max_iter and finished solves - 20 iterations, then 50
# ---------------------------------------------------------------------------------------------------------------------------
def _maxiter():
    o = dict(lr=1.0, nesterov=True, tol=0.0)
    mf = Case("dense", (33, 64), 41, o, env={"ZF_LS_SMALL": "0"}, tag="maxiter")
    mf.make_plan = MFMA
    return [Case("small", (65, 128), 40, o, tag="maxiter"), mf,
            Case("csr", S.SMALL[0][:3], S.SMALL[0][3], o, tag="maxiter"),
            Case("op", (100, 200, 9, "separable"), 43, dict(o, lr=0.5), tag="maxiter")]


# solves that end ZF_CONVERGED: resumed with a larger max_iter they stay converged and advance nothing
def _converged():
    return [Case("small", (65, 128), 44, dict(lr=1.0, nesterov=True, tol=1e-3, max_iter=300), tag="converged"),
            Case("op", (100, 200, 9, "separable"), 45, dict(lr=0.5, nesterov=True, tol=2e-3, max_iter=300), tag="converged")]


RESUME_SMALL = _resume_small()
RESUME_OP = _resume_op()
RING = _ring()
MAXITER = _maxiter()
CONVERGED = _converged()
MAXITER_FIRST, MAXITER_THEN = 20, 50
ALL = RESUME_SMALL + RESUME_OP + RING + MAXITER + CONVERGED
