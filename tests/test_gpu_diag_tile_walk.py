"""GPU: the multi-tile workgroup walk of the P-diag trial kernels (csrc/zf_kernels_step.h, zf_trial_body) against the CPU
oracle, bit for bit in the iterates.

A workgroup walks T = tiles_per_wg interleaved tiles, then - one of them - the ragged remainder.  The library picks T = 1
up to n = 1 048 576, so every other oracle comparison of the suite runs one tile per workgroup, and the code that runs for
T > 1 only - the LDS-DMA pipeline whose units cross tile boundaries, the register pipeline that prefetches across them, the
tile count of a workgroup that owns fewer than T, the choice of the workgroup that takes the remainder - is otherwise
compared with itself (another launch scheme, another S) at n >= 1e6.  ZF_TILES_PER_WG, set before the solver exists,
produces those geometries at n <= 103 430 (tests/diag_tile_cases.py; tests/test_diag_tile_cases.py proves on the CPU that
each geometry is what its row says and that no decision of a case depends on the order of a sum)."""
import numpy as np
import pytest

import diag_tile_cases as D

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _end(status):
    """(status, message) of the result the solver's final state becomes (proximal_gradient._solve_native)."""
    from zfista_amd import _lib, proximal_gradient as pg

    return {_lib.ZF_CONVERGED: (1, pg._MSG_OK), _lib.ZF_MAXITER: (0, pg._MSG_MAXITER),
            _lib.ZF_BACKTRACK_FAILED: (None, f"Error: {pg._MSG_BACKTRACK}")}[status]


def _solve(geom, scen, monkeypatch, sub=D.SUB, env=None, timing=False, acceptance=None, chunk=3, history=None):
    """One device-resident solve of a pair under ZF_TILES_PER_WG (and `env`), advanced `chunk` passes at a time."""
    from zfista_amd import _lib
    from zfista_amd.problems import DiagQuadL1
    from zfista_amd.proximal_gradient import NativeRun

    T, n, _ = D.GEOMETRIES[geom]
    d, c, lam, bounds, x0, o = D.inputs(geom, scen)
    for k in ("ZF_RUNAHEAD", "ZF_AHEAD_UNSHARDED", "ZF_AHEAD", "ZF_SUB_ITERS", "ZF_ACCEPT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ZF_TILES_PER_WG", str(T))
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    o = dict(o, sub_iters=sub)
    if acceptance:
        o["acceptance"] = acceptance
    if history is not None:
        o.update(return_all=True, history_slots=history[0])
    run = NativeRun(DiagQuadL1(d, c, lam, bounds=bounds), x0, o, timing=timing)
    assert run.solver.tiles_per_wg == min(T, D.MAX_T) and run.sub_iters == sub
    rows = [np.zeros((0, _lib.ZF_TRACE_COLS))]
    while run.status == _lib.ZF_RUNNING:
        rows.append(run.advance(chunk))
    ctl = run.solver.ctl
    out = dict(rows=np.concatenate(rows), x=run.solver.get_x(), xp=run.solver.get_x_prev(), nit=int(ctl.nit), status=int(ctl.status),
               lr=ctl.lr, F=ctl.F_old, trials=int(ctl.total_trials), x0=x0,
               passes=[(f, lag) for lag, f, _, _ in run.solver.pass_records()] if timing else None,
               report=run.solver.ahead_report(), launches=run.solver.launch_counts())
    if history is not None:
        H = run.history()
        out["hist"] = [H[k] for k in range(len(H))]
        out["hist_host"] = len(run._hist_host)
    run.solver.close()
    return out


def _against_oracle(got, exp, sub=D.SUB):
    """nit, status and message, the lr and trial-count columns, F and err at 1e-10, the iterate - and, where the last pass
    stored it, the one before - bit for bit."""
    from zfista_amd import _lib

    assert got["nit"] == exp.nit
    assert _end(got["status"]) == (exp.status, exp.message)
    rows = got["rows"]
    assert len(rows) == exp.nit
    assert np.array_equal(rows[:, _lib.TR_LR], exp.alllrs)
    assert np.array_equal(rows[:, _lib.TR_TRIALS].astype(np.int64), exp.alltrials)
    assert got["trials"] == len(exp.decisions)   # (rejected trials included; speculative ones are no trials)
    same = np.array_equal(got["x"], exp.x)
    assert same, (f"{np.count_nonzero(got['x'] != exp.x)} of {exp.x.size} elements differ, the first at "
                  f"{np.flatnonzero(got['x'] != exp.x)[:8].tolist()}")
    if exp.nit >= 1 and sum(exp.passes[sub][-1]) >= 2:   # (a chain of one trial stores x+ alone)
        bad = np.flatnonzero(got["xp"] != exp.x_prev)
        assert bad.size == 0, f"x_prev: {bad.size} of {exp.x.size} elements differ, the first at {bad[:8].tolist()}"
    # one element dropped from a sum or added twice moves F by ~1 / n >= 1e-5
    np.testing.assert_allclose(rows[:, _lib.TR_F], exp.allfuns[1:], rtol=TOL, atol=0)
    np.testing.assert_allclose(rows[:, _lib.TR_ERR], exp.allerrs, rtol=TOL, atol=0)
    if exp.nit >= 1:
        np.testing.assert_allclose(got["F"], exp.fun, rtol=TOL, atol=0)


_S16 = {}   # the default solve of a pair (chains of 16, run-ahead), shared by the axes that compare with it


def _default(geom, scen, monkeypatch):
    if (geom, scen) not in _S16:
        _S16[geom, scen] = _solve(geom, scen, monkeypatch, timing=True)
    return _S16[geom, scen]


def _same(a, b):
    assert (a["nit"], a["status"], a["lr"], a["F"], a["trials"]) == (b["nit"], b["status"], b["lr"], b["F"], b["trials"])
    assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["x"], b["x"])


@pytest.mark.parametrize("geom", D.GEOMETRY_IDS)
@pytest.mark.parametrize("scen", D.SCENARIO_IDS)
def test_tile_walk_against_the_oracle(scen, geom, monkeypatch):
    exp = D.oracle_run(geom, scen)
    got = _default(geom, scen, monkeypatch)
    # the passes the scenario is there for ran - with these shapes, not through another kernel
    assert D.shapes_ran(D.SCENARIOS[scen][2], got["passes"]), (D.SCENARIOS[scen][2], got["passes"])
    assert set(got["passes"]) <= set(exp.passes[D.SUB]), (got["passes"], exp.passes[D.SUB])
    _against_oracle(got, exp)


@pytest.mark.parametrize("sub", [1, 2, 4, 8])
@pytest.mark.parametrize("geom", D.AXIS_GEOMETRIES)
@pytest.mark.parametrize("scen", D.SUB_SCENARIOS)
def test_shorter_chains_walk_the_same_tiles(scen, geom, sub, monkeypatch):
    """sub_iters = 8 is the only way into the software-pipelined register path, whose prefetch crosses tiles; 1, 2 and 4 take
    the batch-per-tile loop.  Trace rows and iterates: those of the chains of 16, and the oracle's."""
    exp = D.oracle_run(geom, scen)
    got = _solve(geom, scen, monkeypatch, sub=sub, timing=True)
    if sub == 8:
        assert (8, 0) in got["passes"], got["passes"]
    assert set(got["passes"]) <= set(exp.passes[sub]), (got["passes"], exp.passes[sub])
    _against_oracle(got, exp, sub=sub)
    _same(got, _default(geom, scen, monkeypatch))


SCHEMES = {"runahead": {}, "per-pass": {"ZF_RUNAHEAD": "0"}, "ahead": {"ZF_RUNAHEAD": "0", "ZF_AHEAD_UNSHARDED": "1"}}


@pytest.mark.parametrize("scheme", list(SCHEMES))
@pytest.mark.parametrize("geom", D.AXIS_GEOMETRIES)
@pytest.mark.parametrize("scen", D.LAUNCH_SCENARIOS)
def test_launch_schemes_walk_the_same_tiles(scen, geom, scheme, monkeypatch):
    """Run-ahead passes (workgroup granularity, coherent loads and stores), one launch per pass, passes ahead at kernel
    granularity: the oracle's results from each, and the scheme in question did launch passes."""
    exp = D.oracle_run(geom, scen)
    got = _solve(geom, scen, monkeypatch, env=SCHEMES[scheme], chunk=64)
    _against_oracle(got, exp)
    _same(got, _default(geom, scen, monkeypatch))
    assert np.array_equal(got["xp"], _default(geom, scen, monkeypatch)["xp"])
    rep, (steps, kernels) = got["report"], got["launches"]
    assert steps >= len(exp.passes[D.SUB]) and kernels >= steps
    # two full chains in a row (or a full chain and the mid chains behind it): something to run ahead of
    full = sum(p == (16, 0) for p in exp.passes[D.SUB])
    if scheme == "runahead":
        assert rep["ahead"] == 0
        if full >= 2:
            assert rep["runahead"] >= 2 and rep["runahead_overlapped"] >= 1, rep
    elif scheme == "per-pass":
        assert rep["runahead"] == 0 and rep["ahead"] == 0, rep
    else:
        assert rep["runahead"] == 0
        if full >= 2:
            assert rep["ahead"] >= 2, rep
    assert rep["timeouts"] == 0 and not rep["runahead_off"]


@pytest.mark.parametrize("sub", [16, 1])
@pytest.mark.parametrize("geom", D.AXIS_GEOMETRIES)
@pytest.mark.parametrize("scen", D.RESOLVED_SCENARIOS)
def test_resolved_acceptance_walks_the_same_tiles(scen, geom, sub, monkeypatch):
    """acceptance="resolved" has kernels of its own (zf_trial_res_*): chains of 16 and single trials, against the oracle's
    f_diff form."""
    exp = D.oracle_run(geom, scen, "resolved")
    got = _solve(geom, scen, monkeypatch, sub=sub, acceptance="resolved", timing=True)
    assert set(got["passes"]) <= set(exp.passes[sub]), (got["passes"], exp.passes[sub])
    if sub == 16:
        assert D.shapes_ran(D.SCENARIOS[scen][2], got["passes"]), got["passes"]
    _against_oracle(got, exp, sub=sub)


@pytest.mark.parametrize("slots", [None, 19])
@pytest.mark.parametrize("sub", [1, 8])
@pytest.mark.parametrize("geom", D.HIST_GEOMETRIES)
@pytest.mark.parametrize("scen", D.HIST_SCENARIOS)
def test_streaming_return_all_walks_the_same_tiles(scen, geom, sub, slots, monkeypatch):
    """The history-recording bodies: every trial stores its iterate into a ring slot - 16-byte stores from the tiles, scalar
    stores from the remainder path.  Every recorded iterate is the oracle's, bit for bit (a roomy ring, and one of 19 slots
    that wraps: older iterates are moved to the host between chunks)."""
    exp = D.oracle_run(geom, scen, "reference", True)
    got = _solve(geom, scen, monkeypatch, sub=sub, history=(slots,))
    _against_oracle(got, exp, sub=sub)
    H = got["hist"]
    assert len(H) == exp.nit + 1 == len(exp.allvecs) and H[0] is got["x0"]
    for k in range(len(H)):
        assert np.array_equal(H[k], exp.allvecs[k]), (k, np.flatnonzero(H[k] != exp.allvecs[k])[:8].tolist())
    assert np.array_equal(H[-1], got["x"])
    if slots:
        assert got["hist_host"] >= exp.nit - slots   # the ring wrapped: older iterates live on the host
