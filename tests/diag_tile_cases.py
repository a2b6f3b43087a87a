"""Case tables of the multi-tile workgroup walk of the P-diag trial kernels (csrc/zf_kernels_step.h: zf_trial_body), shared
by tests/test_diag_tile_cases.py (CPU: the tables are what they claim, the oracle alone meets the margin conditions) and
tests/test_gpu_diag_tile_walk.py (the kernels against the oracle).  No test in here.

A workgroup walks T = tiles_per_wg interleaved tiles of 2048 doubles, then - one workgroup - the ragged remainder.  The
library picks T = 1 up to n = 1 048 576; ZF_TILES_PER_WG (read when a solver is created, clamped to 1 .. 24) produces every
multi-tile geometry at n ~ 1e4 .. 1e5, where the CPU oracle is cheap.

Everything here restates a rule of the library in Python - the launch geometry (`geometry`), the chain lengths and the
replays of a pass (`fresh_len`, `expected_passes`: csrc/zf_decide.h) - or is the oracle's own arithmetic (`oracle_run`)."""
import contextlib
import functools
import io
import warnings

import numpy as np

from oracle import cpu_ref, problems_ref as P

TILE = 2048            # doubles per tile (ZF_TILE_UNITS = 1024 units of 16 bytes)
MAX_T = 24             # ZF_MAX_TILES_PER_WG
SUB = 16               # chain length of the scenarios (ZF_DEFAULT_SUB_ITERS)
MARGIN = 1e-9          # the decisions of a case miss equality by this much (relative), in the oracle's own arithmetic


def geometry(n, T):
    """The host's and the kernel's rules: n2 units of 16 bytes, ntiles tiles (the last one ragged), `full` full tiles, G
    workgroups; workgroup b owns the full tiles b, b + G, ... (at most T); the workgroup next in the round-robin takes what
    is left behind the full tiles."""
    T = max(1, min(int(T), MAX_T))
    n2 = n // 2
    ntiles = max(1, -(-n2 // (TILE // 2)))
    full = n2 // (TILE // 2)
    G = -(-ntiles // T)
    my_tiles = []
    for b in range(G):
        m = 0
        for t in range(T):
            if t * G + b < full:
                m = t + 1
        my_tiles.append(m)
    rem = n - TILE * full
    return dict(T=T, n2=n2, ntiles=ntiles, full=full, G=G, my_tiles=my_tiles, owner=(full % G) if rem else None, rem=rem)


# id -> (T, n, what the row claims: full tiles, G, tiles per workgroup, remainder owner, remainder length)
GEOMETRIES = {
    # 5 full tiles on 3 workgroups: 2, 2, 1; the remainder is ONE element (odd n, no full unit), owned by the short workgroup
    "t2-odd-short-owner": (2, 10_241, dict(full=5, G=3, my_tiles=[2, 2, 1], owner=2, rem=1)),
    # 4 full tiles on 2 workgroups, no remainder; the third tile row is empty for every workgroup
    "t3-empty-last-row": (3, 8_192, dict(full=4, G=2, my_tiles=[2, 2], owner=None, rem=0)),
    # one workgroup: 3 tiles (< T), then a remainder of tile - 1 elements (odd)
    "t8-one-wg": (8, 8_191, dict(full=3, G=1, my_tiles=[3], owner=0, rem=2047)),
    # 11 full tiles on 3 workgroups: 4, 4, 3; the remainder is exactly one 16-byte unit, owned by the short workgroup
    "t5-one-unit-rem": (5, 22_530, dict(full=11, G=3, my_tiles=[4, 4, 3], owner=2, rem=2)),
    # the longest pipelines: 50 full tiles on 3 workgroups, 17, 17, 16; remainder of 1030 elements
    "t24-max": (24, 103_430, dict(full=50, G=3, my_tiles=[17, 17, 16], owner=2, rem=1030)),
    # no full tile: only the remainder path runs
    "t4-no-full-tile": (4, 1_000, dict(full=0, G=1, my_tiles=[0], owner=0, rem=1000)),
    # clamped to 24: one workgroup, 11 tiles (fewer than 24), then the remainder
    "t100-clamped": (100, 22_530, dict(full=11, G=1, my_tiles=[11], owner=0, rem=2)),
}
GEOMETRY_IDS = list(GEOMETRIES)
AXIS_GEOMETRIES = ["t2-odd-short-owner", "t5-one-unit-rem", "t24-max"]
HIST_GEOMETRIES = ["t2-odd-short-owner", "t8-one-wg", "t5-one-unit-rem"]

BASE = dict(lr=1, tol=1e-5, tol_internal=1e-12, max_iter=1000000, max_backtrack_iter=100, decay_rate=0.5,
            nesterov=False, nesterov_ratio=(0, 0.25), deprecated=False, return_all=False)


# id -> (options, bounds, pass shapes (fresh trials, lagging iterations) the solve must run on every geometry; a lag of None
# stands for "behind one lagging iteration or more", fresh trials of None for any number of them)
SCENARIOS = {}


def _add(name, opts, shapes, bounds=None, ista=False):
    SCENARIOS[name] = (dict(opts), bounds, list(shapes))
    if ista:
        SCENARIOS[name + "-ista"] = (dict(opts, nesterov=False), bounds, list(shapes))


# Step sizes, lengths and tolerances are chosen so that the ORACLE's decisions keep the margins test_diag_tile_cases.py
# asserts (MARGIN).  On these data (d in [0.5, 2]) a step contracts the error by up to 1 - lr / 2, and the slack of the
# sufficient-decrease test - of the size |x+ - y|^2 - falls below 1e-9 |F| after ~30 iterations at lr = 0.45 and after
# ~60 at lr = 0.2; a box the iterates run into shortens that further.  Hence, measured with the oracle alone:
#   * lr = 0.45 where the solve is at most 26 iterations long, 0.3 for 37, 0.2 for 45 and 58, 0.01 .. 0.15 inside a box;
#   * lr = 4 halves to 0.5 and keeps the margin for 27 iterations (not 60); lr = 64 for 23;
#   * a stopping tolerance of 1e-3 (at 1e-6 the steps, and with them the slack, are far below the margin);
#   * a rejection in the MIDDLE of a chain - replayed iterations - does not happen with decay_rate = 0.5 on this problem
#     (after the first line search lr <= 0.5 <= 1 / max d holds for good): decay_rate = 0.95 leaves the step size next to
#     the largest the test accepts, and momentum makes it reject again a few iterations on; with the narrow box
#     lr = 44.8 -> 0.35 does the same.
# full chains and a shared tail: 16 + 11 + 10
_add("full37", dict(lr=0.3, nesterov=True, tol=0.0, max_iter=37), [(16, 0), (11, 0), (10, 0)], ista=True)
# every mid-chain length 9 .. 15 (register loads up to 10 trials, LDS-DMA from 11)
MID_LENGTHS = {18: (9, 9), 20: (10, 10), 22: (11, 11), 24: (12, 12), 26: (13, 13), 45: (16, 15, 14), 58: (16, 16, 13, 13)}
for _k, _l in MID_LENGTHS.items():
    _add(f"mid{_k}", dict(lr=0.45 if _k <= 26 else 0.2, nesterov=True, tol=0.0, max_iter=_k), [(f, 0) for f in _l], ista=True)
# rejections first, then chains (every pass of the first line search ends at its first trial)
_add("rej-lr64", dict(lr=64.0, nesterov=True, tol=0.0, max_iter=23), [(12, 0), (11, 0)], ista=True)
_add("rej-lr4", dict(lr=4.0, nesterov=True, tol=0.0, max_iter=27), [(14, 0), (13, 0)], ista=True)
# a fine backtracking factor: the step size settles next to the largest the test accepts, and momentum makes the test
# reject again a few iterations later, in the middle of a chain - replayed iterations (lag > 0) in front of 8 fresh trials
_add("rej-decay95", dict(lr=4.0, nesterov=True, tol=0.0, max_iter=24, decay_rate=0.95), [(12, 0), (8, None)])
_add("backtrack-fails", dict(lr=1e6, nesterov=True, tol=0.0, max_iter=50, max_backtrack_iter=3), [(16, 0)], ista=True)
# termination inside a chain: the accepted iterations of the broken chain are materialised by a replay-only pass
_add("tol1e-3", dict(lr=0.45, nesterov=True, tol=1e-3, max_iter=10000), [(16, 0), (0, None)])
_add("decay1", dict(lr=0.45, nesterov=True, tol=0.0, max_iter=37, decay_rate=1.0), [(16, 0), (11, 0), (10, 0)])
_add("deprecated", dict(lr=4.0, nesterov=True, tol=0.0, max_iter=37, deprecated=True), [(16, 0), (11, 0), (10, 0)])
# a box: its own kernels; no mid chains (9 .. 15 fresh trials take the general body)
BOX, POS = (-0.05, 0.07), (0.0, np.inf)
_add("full37-box", dict(lr=0.02, nesterov=True, tol=0.0, max_iter=37), [(16, 0), (11, 0), (10, 0)], bounds=BOX)
_add("full48-box", dict(lr=0.01, nesterov=True, tol=0.0, max_iter=48), [(16, 0)], bounds=BOX)   # three full chains in a row
_add("full37-pos", dict(lr=0.15, nesterov=True, tol=0.0, max_iter=37), [(16, 0), (11, 0), (10, 0)], bounds=POS)
# (lr = 44.8 halves to 0.35 and - two or three iterations later, in the middle of a chain - to 0.175)
_add("rej-lr45-box", dict(lr=44.8, nesterov=True, tol=0.0, max_iter=8), [(8, 0), (None, None)], bounds=BOX)
_add("rej-lr45-pos", dict(lr=44.8, nesterov=True, tol=0.0, max_iter=23), [(12, 0)], bounds=POS)
_add("rej-lr4-pos", dict(lr=4.0, nesterov=True, tol=0.0, max_iter=20), [(10, 0)], bounds=POS)
_add("rej-decay95-pos", dict(lr=4.0, nesterov=True, tol=0.0, max_iter=12, decay_rate=0.95), [(12, 0), (8, None)], bounds=POS)
SCENARIO_IDS = list(SCENARIOS)
SUB_SCENARIOS = ["full37", "mid45", "rej-decay95", "tol1e-3"]         # sub_iters 1, 2, 4, 8 against 16 and the oracle
LAUNCH_SCENARIOS = ["mid58", "mid45-ista", "rej-decay95", "full48-box"]   # run-ahead / one launch per pass / passes ahead
RESOLVED_SCENARIOS = ["full37", "rej-decay95", "tol1e-3", "backtrack-fails"]
HIST_SCENARIOS = ["rej-decay95", "tol1e-3"]


def shapes_ran(named, passes):
    """Every named shape is among the passes (fresh, lag) of a solve."""
    return all(any((f is None or f == pf) and (pl > 0 if lag is None else pl == lag) for pf, pl in passes) for f, lag in named)


class BoxRef(P.DiagQuadL1Ref):
    """P-diag with a box: g is inf outside it, the prox clips the soft-thresholded point into it."""

    def __init__(self, d, c, lam, lo, hi):
        super().__init__(d, c, lam)
        self.lo, self.hi = float(lo), float(hi)

    def g(self, x):
        if (x < self.lo).any() or (x > self.hi).any():
            return np.inf
        return super().g(x)

    def prox_wsum_g(self, w, x):
        return P.clip_box(super().prox_wsum_g(w, x), self.lo, self.hi)


def seed_of(geom, scen):
    return 7000 + 100 * GEOMETRY_IDS.index(geom) + SCENARIO_IDS.index(scen)


def inputs(geom, scen):
    """(d, c, lam, bounds, x0, options) of a pair.  x0 is random - an element a kernel leaves untouched cannot pass - and,
    with a box, inside it (F(x0) is finite)."""
    T, n, _ = GEOMETRIES[geom]
    opts, bounds, _ = SCENARIOS[scen]
    seed = seed_of(geom, scen)
    d, c, lam = P.make_pdiag(n, seed=seed)
    x0 = np.random.default_rng(seed).standard_normal(n)
    if bounds is not None:
        x0 = np.clip(x0, bounds[0], bounds[1])
    return d, c, lam, bounds, x0, dict(BASE) | opts


def reference(geom, scen):
    d, c, lam, bounds, _, _ = inputs(geom, scen)
    return P.DiagQuadL1Ref(d, c, lam) if bounds is None else BoxRef(d, c, lam, *bounds)


def fresh_len(nit, lag, max_iter, sub):
    """zf_fresh_len: the fresh trials of the next pass (no status pending)."""
    left = max_iter - nit
    n = sub // 2 if sub >= 16 else sub
    if lag == 0:
        if left >= 2 * sub or left == sub:
            return sub
        n = (left + 1) // 2 if left > sub else left
    return int(max(1, min(n, 2 * sub - 1 - lag, left)))


def expected_passes(alltrials, nit, end, max_iter, max_backtrack, sub=SUB):
    """The passes (fresh trials, lagging iterations) of a solve whose line search took `alltrials` trials per iteration and
    ended after `nit` iterations with `end` in {"converged", "maxiter", "failed"} (zf_decide_pass restated: a chain
    that breaks leaves its accepted iterations lagging; a final status behind lagging iterations first materialises them)."""
    outcomes = []
    for t in alltrials[:nit]:
        outcomes += [False] * (t - 1) + [True]
    if end == "failed":
        outcomes += [False] * max_backtrack
    passes, k, lag, trial, pos, done = [], 0, 0, 0, 0, False
    while not done:
        nf = fresh_len(k, lag, max_iter, sub)
        accepted, final = 0, False
        for _ in range(nf):
            ok = outcomes[pos]
            pos += 1
            if not ok:
                trial += 1
                final = trial >= max_backtrack
                break
            k, accepted, trial = k + 1, accepted + 1, 0
            if (end == "converged" and k == nit) or k >= max_iter:
                final = True
                break
        passes.append((nf, lag))
        if accepted == nf:
            lag = 0
            done = final
        else:
            lag += accepted
            if final:
                if lag > 0:
                    passes.append((0, lag))   # the materialise-only pass
                done = True
    assert pos == len(outcomes)
    return passes


class OracleRun:
    """What the tests need of one oracle solve (the iterates themselves are dropped: x_nit and x_{nit-1} stay)."""


@functools.lru_cache(maxsize=None)
def oracle_run(geom, scen, acceptance="reference", keep_vecs=False):
    """The oracle's solve of a pair, and every trial of its line search evaluated once more for the two margins:
    `accept_margin` - the least |rhs - lhs| / max(1, |F|) of the sufficient-decrease test over all trials (inf where no
    test decides: decay_rate = 1); `err_margin` - the least |err - tol| / tol (inf for tol = 0)."""
    d, c, lam, bounds, x0, o = inputs(geom, scen)
    ref = reference(geom, scen)
    f, g, jac_f, prox = ref.callbacks()
    kw = {k: v for k, v in o.items() if k != "return_all"}
    if acceptance == "resolved":
        kw["f_diff"] = ref.f_diff
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with contextlib.redirect_stdout(io.StringIO()):   # ("An error occurred": the reference reports, the tests compare)
            exp = cpu_ref.minimize_proximal_gradient(f, g, jac_f, prox, x0, return_all=True, **kw)
    r = OracleRun()
    r.nit, r.success, r.message, r.status = int(exp.nit), bool(exp.success), exp.message, exp.get("status")
    r.end = "converged" if exp.success else "maxiter" if "status" in exp else "failed"
    r.alllrs = np.asarray(exp.alllrs, float)
    r.alltrials = np.asarray(exp.alltrials, np.int64)
    r.allfuns = np.asarray(exp.allfuns, float)
    r.allerrs = np.asarray(exp.allerrs, float)
    r.x = exp.allvecs[r.nit]
    r.x_prev = exp.allvecs[r.nit - 1] if r.nit >= 1 else None
    r.fun = float(exp.fun)
    assert np.array_equal(r.x, exp.x)
    r.allvecs = list(exp.allvecs) if keep_vecs else None
    r.passes = {s: expected_passes(r.alltrials, r.nit, r.end, o["max_iter"], o["max_backtrack_iter"], s) for s in (1, 2, 4, 8, 16)}
    # -- every trial once more ------------------------------------------------------------------------------------------
    betas = cpu_ref.momentum_sequence(r.nit + 1, o["nesterov_ratio"])
    vecs = exp.allvecs
    accept_margin = err_margin = np.inf
    decisions = []
    iterations = r.nit + (1 if r.end == "failed" else 0)
    lr = o["lr"]
    for k in range(1, iterations + 1):
        x_prev = vecs[k - 1]
        y = x_prev
        if o["nesterov"] and k >= 2:
            y = x_prev + betas[k - 2] * (x_prev - vecs[k - 2])
        F_prev = f(x_prev) + g(x_prev)
        trials = int(r.alltrials[k - 1]) if k <= r.nit else o["max_backtrack_iter"]
        for t in range(trials):
            sub = cpu_ref.trial_single(f, g, jac_f, prox, lr, x_prev, y, o["deprecated"])
            x_new = sub.x
            if o["decay_rate"] == 1:
                gap = np.inf
            elif acceptance == "resolved":
                step = x_new - y
                nrm = np.linalg.norm(step)
                lhs = ref.f_diff(x_new, y) if o["deprecated"] else (ref.f_diff(x_new, y) - float(jac_f(y) @ step)) - nrm * nrm / 2 / lr
                gap = (sub.fun if o["deprecated"] else 0.0) + o["tol_internal"] - lhs
            elif o["deprecated"]:
                gap = sub.fun + o["tol_internal"] - (f(x_new) - f(y))
            else:
                gap = sub.fun + o["tol_internal"] - ((f(x_new) + g(x_new)) - F_prev)
            decisions.append(bool(gap >= 0))
            accept_margin = min(accept_margin, abs(gap) / max(1.0, abs(F_prev)))
            if o["tol"] > 0:
                err_margin = min(err_margin, abs(np.max(np.abs(x_new - y)) - o["tol"]) / o["tol"])
            if t + 1 < trials or k > r.nit:
                lr = lr * o["decay_rate"]
        if k <= r.nit:
            assert lr == r.alllrs[k - 1] and np.array_equal(x_new, vecs[k]), (geom, scen, k)
    r.decisions = decisions
    r.accept_margin, r.err_margin = float(accept_margin), float(err_margin)
    # the stagnation region (test_gpu_fuzz_parity._compare): F no longer changes at double resolution
    F = r.allfuns
    r.stalled = np.flatnonzero(np.abs(np.diff(F)) <= 64 * np.finfo(float).eps * np.maximum(1.0, np.abs(F[1:])))
    return r
