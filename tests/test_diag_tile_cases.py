"""CPU: the case tables of tests/diag_tile_cases.py are what they claim to be, and the oracle ALONE - NumPy's arithmetic,
no device - runs every (geometry, scenario) pair of tests/test_gpu_diag_tile_walk.py clear of every decision that could
fall differently under another order of summation: the GPU file compares iterates bit for bit and decision sequences
exactly, so no decision of a case may hinge on the last bits of a sum."""
import numpy as np
import pytest

import diag_tile_cases as D


def test_geometry_rows_have_the_properties_they_claim():
    for name, (T, n, claim) in D.GEOMETRIES.items():
        g = D.geometry(n, T)
        assert {k: g[k] for k in claim} == claim, name
        assert n <= 103_430 and g["T"] == min(T, D.MAX_T)
        # the round-robin: every full tile has exactly one owner, workgroup b walks b, b + G, ...
        owned = sorted(t * g["G"] + b for b in range(g["G"]) for t in range(g["my_tiles"][b]))
        assert owned == list(range(g["full"])), name
        assert g["rem"] == n - D.TILE * g["full"] and 0 <= g["rem"] < D.TILE
    g = {name: D.geometry(n, T) for name, (T, n, _) in D.GEOMETRIES.items()}
    n_of = {name: n for name, (_, n, _) in D.GEOMETRIES.items()}
    # one odd element, no full unit, owned by the workgroup that has fewer than T tiles
    a = g["t2-odd-short-owner"]
    assert n_of["t2-odd-short-owner"] % 2 == 1 and a["rem"] == 1 and a["n2"] * 2 == D.TILE * a["full"]
    assert a["my_tiles"][a["owner"]] == 1 < a["T"] == max(a["my_tiles"])
    # no remainder; no workgroup has a tile in the last row
    a = g["t3-empty-last-row"]
    assert a["rem"] == 0 and a["owner"] is None and max(a["my_tiles"]) == a["T"] - 1
    assert all((a["T"] - 1) * a["G"] + b >= a["full"] for b in range(a["G"]))
    # one workgroup, fewer tiles than T, a remainder of tile - 1 elements
    a = g["t8-one-wg"]
    assert a["G"] == 1 and a["my_tiles"] == [3] and 3 < a["T"] and a["rem"] == D.TILE - 1 and a["rem"] % 2 == 1
    # exactly one 16-byte unit behind the full tiles, with the short workgroup
    a = g["t5-one-unit-rem"]
    assert a["rem"] == 2 and a["n2"] == a["full"] * (D.TILE // 2) + 1 and a["my_tiles"][a["owner"]] == min(a["my_tiles"]) < a["T"]
    # the largest T: pipelines of 17 and 16 tiles
    a = g["t24-max"]
    assert a["T"] == D.MAX_T and sorted(set(a["my_tiles"])) == [16, 17] and a["rem"] == 1030 and a["my_tiles"][a["owner"]] == 16
    # nothing but the remainder
    a = g["t4-no-full-tile"]
    assert a["full"] == 0 and a["my_tiles"] == [0] and a["owner"] == 0 and a["rem"] == n_of["t4-no-full-tile"]
    # the clamp
    a = g["t100-clamped"]
    assert D.GEOMETRIES["t100-clamped"][0] > D.MAX_T == a["T"] and a["G"] == 1 and a["my_tiles"] == [11] and 11 < a["T"]
    # the axes of the GPU file name rows of the tables; the history axis holds the two remainders whose stores into a ring
    # slot cannot be 16-byte stores (one odd element; tile - 1 elements)
    assert set(D.AXIS_GEOMETRIES) | set(D.HIST_GEOMETRIES) <= set(D.GEOMETRIES)
    assert {"t2-odd-short-owner", "t8-one-wg"} <= set(D.HIST_GEOMETRIES)
    for names in (D.SUB_SCENARIOS, D.LAUNCH_SCENARIOS, D.RESOLVED_SCENARIOS, D.HIST_SCENARIOS):
        assert set(names) <= set(D.SCENARIOS)


def test_pass_plan_restated():
    """`expected_passes` against passes worked out by hand from zf_fresh_len / zf_decide_pass."""
    clean = lambda k: D.expected_passes([1] * k, k, "maxiter", k, 100)
    assert clean(37) == [(16, 0), (11, 0), (10, 0)]        # 16, then the 21 left are shared
    assert clean(5) == [(5, 0)] and clean(16) == [(16, 0)] and clean(32) == [(16, 0), (16, 0)] and clean(33) == [(16, 0), (9, 0), (8, 0)]
    for k, lengths in D.MID_LENGTHS.items():
        assert clean(k) == [(f, 0) for f in lengths], k
    assert {f for lengths in D.MID_LENGTHS.values() for f in lengths} >= set(range(9, 17))
    # a rejection at the third trial of a chain: two iterations lag, 8 fresh trials behind them, then 30 = 15 + 15
    assert D.expected_passes([1, 1, 2] + [1] * 37, 40, "maxiter", 40, 100) == [(16, 0), (8, 2), (15, 0), (15, 0)]
    # rejections at the first trial of a pass leave nothing lagging
    assert D.expected_passes([3] + [1] * 19, 20, "maxiter", 20, 100) == [(10, 0)] * 4
    # termination at the 9th trial of the second chain: a replay-only pass materialises the 9 iterations
    assert D.expected_passes([1] * 25, 25, "converged", 10000, 100) == [(16, 0), (16, 0), (0, 9)]
    assert D.expected_passes([1] * 32, 32, "converged", 10000, 100) == [(16, 0), (16, 0)]
    # the line search fails at once / behind three accepted iterations
    assert D.expected_passes([], 0, "failed", 50, 3) == [(16, 0)] * 3
    assert D.expected_passes([1, 1, 1], 3, "failed", 50, 2) == [(16, 0), (8, 3), (0, 3)]
    # shorter chains: S fresh trials behind lagging iterations too
    assert D.expected_passes([1, 2, 1, 1, 1, 1], 6, "maxiter", 6, 100, sub=4) == [(3, 0), (4, 1), (1, 0)]
    assert D.expected_passes([1] * 7, 7, "maxiter", 7, 100, sub=1) == [(1, 0)] * 7


def _check(r, geom, scen):
    opts, _, named = D.SCENARIOS[scen]
    assert r.nit <= 120, "a pair ends within 120 iterations"
    # out of the stagnation region (the `stalled` rule of test_gpu_fuzz_parity._compare)
    assert not (r.stalled.size and r.stalled[0] + 1 <= r.nit), (r.stalled[:3], r.nit)
    # every trial of the line search, evaluated once more, decides as the oracle did ...
    want = []
    for t in r.alltrials:
        want += [False] * (int(t) - 1) + [True]
    if r.end == "failed":
        want += [False] * D.SCENARIOS[scen][0].get("max_backtrack_iter", 100)
    assert r.decisions == want
    # ... and by a margin: |right - left| >= 1e-9 max(1, |F|) at every trial, |err - tol| >= 1e-9 tol
    assert r.accept_margin >= D.MARGIN, r.accept_margin
    if opts["tol"] > 0:
        assert r.end == "converged" and r.err_margin >= D.MARGIN, r.err_margin
    assert D.shapes_ran(named, r.passes[D.SUB]), (named, r.passes[D.SUB])


@pytest.mark.parametrize("geom", D.GEOMETRY_IDS)
@pytest.mark.parametrize("scen", D.SCENARIO_IDS)
def test_oracle_keeps_every_decision_clear_of_the_summation_order(scen, geom):
    _check(D.oracle_run(geom, scen), geom, scen)


@pytest.mark.parametrize("geom", D.AXIS_GEOMETRIES)
@pytest.mark.parametrize("scen", D.RESOLVED_SCENARIOS)
def test_oracle_keeps_the_resolved_decisions_clear_too(scen, geom):
    """acceptance="resolved" (the oracle's f_diff form): the same conditions, and the same decisions as the reference's
    form takes on these pairs (both tests resolve them)."""
    r = D.oracle_run(geom, scen, "resolved")
    _check(r, geom, scen)
    ref = D.oracle_run(geom, scen)
    assert r.nit == ref.nit and np.array_equal(r.alltrials, ref.alltrials) and np.array_equal(r.x, ref.x)


def test_scenarios_reach_what_they_are_there_for():
    passes = lambda scen, sub=D.SUB: [D.oracle_run(g, scen).passes[sub] for g in D.GEOMETRY_IDS]
    # every chain length 9 .. 16 with nothing lagging, over the clean scenarios
    clean = {p for scen in D.SCENARIOS if scen.startswith(("mid", "full37")) for ps in passes(scen) for p in ps}
    assert {(f, 0) for f in range(9, 17)} <= clean
    # replayed iterations in front of 8 fresh trials (the replay + S body), on every geometry; a replay-only pass
    assert all(any(f == 8 and lag > 0 for f, lag in ps) for ps in passes("rej-decay95"))
    assert all(any(f == 8 and lag > 0 for f, lag in ps) for ps in passes("rej-decay95-pos"))
    assert all(ps[-1][0] == 0 and ps[-1][1] > 0 for ps in passes("tol1e-3"))
    # a failed line search; a solve that ends by max_iter
    assert all(D.oracle_run(g, "backtrack-fails").end == "failed" for g in D.GEOMETRY_IDS)
    assert all(D.oracle_run(g, "full37").end == "maxiter" for g in D.GEOMETRY_IDS)
    # the last pass of most solves stores two iterates (x_{k-1} is compared then): at least one such scenario per geometry
    for g in D.GEOMETRY_IDS:
        assert sum(sum(D.oracle_run(g, scen).passes[D.SUB][-1]) >= 2 for scen in D.SCENARIO_IDS) >= 10
    # chains of 8 (the software-pipelined register path): full chains on the sub_iters axis
    assert all(any(p == (8, 0) for p in D.oracle_run(g, scen).passes[8]) for g in D.AXIS_GEOMETRIES for scen in D.SUB_SCENARIOS)
