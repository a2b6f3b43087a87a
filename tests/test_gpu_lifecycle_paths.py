"""GPU: the lifecycle calls of a live solve on every path that decides or records in a kernel of its own (the tables of
tests/lifecycle_cases.py; tests/test_lifecycle_cases.py proves them on the CPU).

  resume       snapshot -> .npz -> from_snapshot in a new solver (zf_solver_restore), on the fused small-matrix path, on the same
               shapes driven by the host-driven sequence and behind a one-rank communicator, and for the operator problem: the continuation equals the uninterrupted device solve BIT FOR BIT - x, the trace rows, nit,
               status, lr, total_trials - from snapshots at nit = 0 (between a rejected trial and its retry), 1, 2 and the middle
               of the run, through a resume of a resumed solve, and past the point where the reference's test stalls
  ring         a history ring smaller than the solve on every recording kernel outside the separable chains: the slot index, a
               rejected trial's iterate overwritten by its retry, the spill to the host in the middle of a run
  max_iter     set_max_iter on a live solve, a finished solve resumed with a larger max_iter, a converged solve left alone

Two references throughout: the uninterrupted device solve (np.array_equal) and the CPU oracle (the lr and trial sequences exactly,
iterates and traces to the project's 1e-10).  Every id clears the path switches, sets its case's and asserts through ls_plan() that
the path it is about ran."""
import numpy as np
import pytest

import lifecycle_cases as LC
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-10


@pytest.fixture
def switches(monkeypatch):
    """Set exactly the case's ZF_* switches (the others unset, whatever the environment holds)."""

    def apply(case):
        for k in LC.SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in case.env.items():
            monkeypatch.setenv(k, v)

    return apply


@pytest.fixture
def one_rank_group(tmp_path):
    """The host-driven sequence (ZF_FORCE_SPLIT=1) gathers its packs through torch.distributed: a default group of this one
    process (gloo over a file store), made on request and taken down after the test."""
    import torch.distributed as dist

    made = []

    def make():
        if not dist.is_initialized():
            dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "rendezvous"), 1), rank=0, world_size=1)
            made.append(True)

    yield make
    if made:
        dist.destroy_process_group()


def _opts(case, **over):
    return dict(LC.BASE, **case.opts) | over


def _drain(run, chunk=3):
    from zfista_amd import _lib

    rows = [np.zeros((0, _lib.ZF_TRACE_COLS))]
    while run.status == _lib.ZF_RUNNING:
        rows.append(run.advance(chunk))
    return np.concatenate(rows)


def _end(run):
    ctl = run.solver.ctl
    return int(ctl.nit), int(ctl.status), ctl.lr, int(ctl.total_trials), ctl.F_old


def _assert_path(case, run, recording=False):
    plan = run.solver.ls_plan()
    assert case.plan_ok(plan, run.solver.responses_plan()), (case.id, plan, run.solver.responses_plan())
    if case.family == "op":
        # the prox step rides in the adjoint kernel unless the switch or a history ring says otherwise
        assert plan[3] == (0 if recording else int(case.env.get("ZF_OP_FUSE_PROX", "1"))), plan
    return plan


def _against_oracle(case, rows, x, exp, status):
    """The lr and trial sequences exactly; the error and objective traces and the final iterate to 1e-10 (the error trace is a
    difference of two iterates, each within 1e-10 of the oracle's: tests/test_gpu_dense_ls_paths.py)."""
    from zfista_amd import _lib

    assert len(rows) == exp.nit and (status == _lib.ZF_CONVERGED) == bool(exp.success)
    assert np.array_equal(rows[:, _lib.TR_LR], np.asarray(exp.alllrs, float))
    assert np.array_equal(rows[:, _lib.TR_TRIALS], np.asarray(exp.alltrials, float))
    funs = np.asarray(exp.allfuns, float).reshape(-1)
    np.testing.assert_allclose(rows[:, _lib.TR_F], funs[1:], rtol=TOL, atol=0)
    xmax = max(float(np.max(np.abs(v))) for v in exp.allvecs)
    np.testing.assert_allclose(rows[:, _lib.TR_ERR], np.asarray(exp.allerrs, float).reshape(-1), rtol=1e-9, atol=2 * TOL * xmax)
    assert rel_err(x, exp.x) <= TOL


def _through_a_file(state, path):
    np.savez(path, **state)
    return dict(np.load(path))


# ---- B1 / B2: resume ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.RESUME_SMALL + LC.RESUME_OP, ids=lambda c: c.id)
def test_resume_continues_the_uninterrupted_solve_bit_for_bit(case, switches, tmp_path, one_rank_group):
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    switches(case)
    comm = None
    if case.tag == "split":
        one_rank_group()
    if case.tag == "comm":   # a one-rank communicator: the steps decide in a launch of their own, the margins are the row sweep's
        from zfista_amd.comm import LibComm

        comm = LibComm(0, 1, LibComm.new_unique_id())
    prob, x0, o = case.problem(group=comm), case.x0(), _opts(case)
    exp = case.oracle()
    whole = NativeRun(prob, x0, o)
    plan = _assert_path(case, whole)
    if case.family == "small":
        assert plan[0] == 1   # (tags split / comm: the shape is eligible - what their passes run is the general sequence)
        assert whole.solver.split == (case.tag == "split") and (whole.solver.comm is not None) == (case.tag == "comm")
    else:
        print(f"{case.id}: plan {plan} (plan[2] - walking workgroups - is recorded, not asserted)")
    whole_rows, whole_x, whole_end = _drain(whole), whole.solver.get_x(), _end(whole)
    whole.solver.close()
    _against_oracle(case, whole_rows, whole_x, exp, whole_end[1])

    run, rows, done = NativeRun(prob, x0, o), [], 0
    for visit, point in enumerate(case.snap):
        passes = case.passes_at(point)
        rows.append(run.advance(passes - done))
        done = passes
        state = run.snapshot()
        run.solver.close()
        ctl = _lib.Control.from_buffer_copy(np.asarray(state["control"], dtype=np.uint8).tobytes())
        nit, retry = case.nit_after(passes)
        assert int(ctl.nit) == nit and int(ctl.status) == _lib.ZF_RUNNING and int(ctl.total_trials) == passes, (point, int(ctl.nit))
        if retry:   # between a rejected trial and its retry
            assert ctl.trial > 0 and ctl.need_grad == 0
        else:
            assert ctl.trial == 0
        # the saved iterates are the oracle's x_k, x_{k-1} (x_{-1} = x_0)
        assert rel_err(state["x"], exp.allvecs[nit]) <= TOL and rel_err(state["x_prev"], exp.allvecs[max(nit - 1, 0)]) <= TOL
        state = _through_a_file(state, tmp_path / f"ckpt{visit}.npz")
        run = NativeRun.from_snapshot(prob, state, o)
        _assert_path(case, run)
        assert run.nit_seen == nit and run.status == _lib.ZF_RUNNING
    rows.append(_drain(run))
    rows = np.concatenate(rows)
    got_x, got_end = run.solver.get_x(), _end(run)
    run.solver.close()
    assert got_end == whole_end
    assert np.array_equal(rows, whole_rows)
    assert np.array_equal(got_x, whole_x)
    _against_oracle(case, rows, got_x, exp, got_end[1])
    if comm is not None:
        import torch

        torch.cuda.synchronize()
        comm.close()


# ---- B3: a ring that wraps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.RING, ids=lambda c: c.id)
def test_a_small_history_ring_wraps_and_spills(case, switches):
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    switches(case)
    prob, x0 = case.problem(), case.x0()
    exp = case.oracle()
    hist = {}
    for slots in LC.RING_SLOTS:
        run = NativeRun(prob, x0, _opts(case, return_all=True, history_slots=slots))
        _assert_path(case, run, recording=True)
        assert run.sub_iters == 1
        if slots:
            assert run._hist_cap == max(slots, 2 * run.sub_iters + 2) == (5 if slots == 5 else 4)   # (1 is raised to 2 S + 2)
        else:
            assert run._hist_cap > exp.nit + 1, "the roomy ring holds the whole solve"
        rows = _drain(run, chunk=3)
        nit, status = int(run.solver.ctl.nit), int(run.solver.ctl.status)
        H = run.history()
        assert len(H) == nit + 1 and H[0] is x0
        hist[slots] = [np.array(H[k]) for k in range(len(H))]
        assert np.array_equal(hist[slots][-1], run.solver.get_x())
        if slots:
            assert nit >= 2 * run._hist_cap and len(run._hist_host) >= nit - run._hist_cap
        else:
            _against_oracle(case, rows, run.solver.get_x(), exp, status)
            assert status == _lib.ZF_CONVERGED and len(H) == len(exp.allvecs)
            for k, (a, e) in enumerate(zip(hist[slots], exp.allvecs)):
                assert rel_err(a, e) <= TOL, k
        run.solver.close()
    for slots in LC.RING_SLOTS[1:]:
        assert len(hist[slots]) == len(hist[None]), slots
        for k, (a, e) in enumerate(zip(hist[slots], hist[None])):
            assert np.array_equal(a, e), (slots, k)


# ---- B4: set_max_iter and finished solves --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.MAXITER, ids=lambda c: c.id)
def test_a_solve_stopped_by_max_iter_continues(case, switches):
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    switches(case)
    prob, x0 = case.problem(), case.x0()
    first, then = LC.MAXITER_FIRST, LC.MAXITER_THEN
    full = NativeRun(prob, x0, _opts(case, max_iter=then))
    _assert_path(case, full)
    full_rows, full_x, full_end = _drain(full), full.solver.get_x(), _end(full)
    full.solver.close()
    assert full_end[:2] == (then, _lib.ZF_MAXITER)
    _against_oracle(case, full_rows, full_x, case.solve(case.ref(), max_iter=then), full_end[1])

    part = NativeRun(prob, x0, _opts(case, max_iter=first))
    _assert_path(case, part)
    head = _drain(part)
    assert part.status == _lib.ZF_MAXITER and part.nit_seen == first
    state = part.snapshot()
    # the live solve, told to go on
    part.set_max_iter(then)
    assert part.status == _lib.ZF_RUNNING
    rows = np.concatenate([head, _drain(part)])
    assert _end(part) == full_end and np.array_equal(rows, full_rows) and np.array_equal(part.solver.get_x(), full_x)
    part.solver.close()
    # the stopped solve's snapshot, resumed with the larger max_iter
    cont = NativeRun.from_snapshot(prob, state, _opts(case, max_iter=then))
    _assert_path(case, cont)
    assert cont.status == _lib.ZF_RUNNING and cont.nit_seen == first
    rows = np.concatenate([head, _drain(cont)])
    assert _end(cont) == full_end and np.array_equal(rows, full_rows) and np.array_equal(cont.solver.get_x(), full_x)
    cont.solver.close()


@pytest.mark.parametrize("case", LC.CONVERGED, ids=lambda c: c.id)
def test_a_converged_solve_stays_converged(case, switches):
    from zfista_amd import _lib
    from zfista_amd.proximal_gradient import NativeRun

    switches(case)
    prob, x0, o = case.problem(), case.x0(), _opts(case)
    exp = case.oracle()
    run = NativeRun(prob, x0, o)
    _assert_path(case, run)
    rows, x, end = _drain(run), run.solver.get_x(), _end(run)
    assert end[1] == _lib.ZF_CONVERGED and end[0] < o["max_iter"]
    _against_oracle(case, rows, x, exp, end[1])
    state = run.snapshot()
    run.set_max_iter(10 * o["max_iter"])
    assert run.status == _lib.ZF_CONVERGED and len(run.advance(3)) == 0
    assert _end(run) == end and np.array_equal(run.solver.get_x(), x)
    run.solver.close()
    cont = NativeRun.from_snapshot(prob, state, dict(o, max_iter=10 * o["max_iter"]))
    assert cont.status == _lib.ZF_CONVERGED and cont.nit_seen == end[0]
    assert len(cont.advance(3)) == 0
    assert _end(cont) == end and np.array_equal(cont.solver.get_x(), x)
    cont.solver.close()
