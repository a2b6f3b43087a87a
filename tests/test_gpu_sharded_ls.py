"""GPU: sharded dense least squares (LeastSquaresL1 over world > 1 ranks) in both layouts - column blocks (A_p, x_p per rank; the
m-vector A_p x_p is exchanged) and row blocks (A_p, b_p per rank, x replicated; the n-vector A_p^T r_p is exchanged) - at uneven
splits, with a box, from x0 != 0 and under the whole option set.  The tables and the driver are tests/sharded_ls_cases.py;
tests/test_sharded_ls_cases.py proves on the CPU that every solve compared here is decided alike under a second summation order.

  element checks   per shape case: each rank's exchanged part against a longdouble evaluation within an a-priori fp64 bound, and
                   F(x0), F(x+) against longdouble f + g - what sees a pack term that is doubled or dropped (contribute_f /
                   contribute_x / contribute_g, f_repl): every rank then still agrees with every other, bit for bit
  solves           per shape case 30 FISTA iterations, and 2 x 24 seeded option cases, against the oracle on the UNSHARDED
                   problem: decisions exactly, numbers to 1e-10
  thread ranks     the library's own sequence (zf_solver_enqueue_steps with a communicator attached) on three cases per layout
  refusals         zf_solver_restore on a sharded least-squares solver

The ranks of a case run in ONE thread, in lockstep (sharded_ls_cases.Lockstep): a wrong kernel yields a wrong number, never a
waiting rank.

ZF_SHARDED_LS_BOUNDS_RECORD=1 appends the worst error / bound ratio of every element check to profiles/sharded_ls_bounds.jsonl
(the mechanism of tests/test_gpu_logistic.py).  The ratios are records, not thresholds; the committed file was measured on an
MI355X when these tests were written."""
import json
import os
import warnings

import numpy as np
import pytest

import sharded_ls_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = C.U
SHAPE_IDS = [c.name for c in C.SHAPE_CASES]


def _record(**rec):
    where = os.environ.get("ZF_SHARDED_LS_BOUNDS_RECORD", "")
    if where in ("", "0"):
        return
    path = os.path.join(ROOT, "profiles", "sharded_ls_bounds.jsonl") if where == "1" else where
    with open(path, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


def _gamma(k):
    return k * U / (1 - k * U)


def _F_longdouble(A, b, lam, x, scale):
    """(F = f + g at x in longdouble, the bound of an fp64 evaluation: ls_longdouble's f bound plus n u g, f, g).  No box: the
    element checks run without one."""
    from oracle import problems_ref as P

    f, _, f_bound, _ = P.ls_longdouble(A, b, x, scale, grad=False)
    g = np.longdouble(lam) * np.sum(np.abs(np.asarray(x, np.float64).astype(np.longdouble)))
    return f + g, f_bound + x.size * U * float(g), float(f), float(g)


@pytest.mark.parametrize("case", C.SHAPE_CASES, ids=SHAPE_IDS)
def test_parts_and_pack_terms_element_by_element(case):
    """One accepted trial from a random x0 (lr <= 1 / (2 L)).  Every rank reports the plan the table claims.  Column blocks: after
    the first half of the initialisation each rank's part is A_p x0_p, every element within gamma_(n_p) (|A_p| |x0_p|)_i of the
    longdouble product.  Row blocks: after the first half of the first trial each rank's part is 2 scale A_p^T (A_p x0 - b_p),
    every element within ls_longdouble's gradient bound for that row block.  Both: F(x0) of the control block and F(x+) of the
    first trace row, at the device's own x+, within ls_longdouble's f bound + n u g of longdouble f + g - a g or f that one rank
    too many (or too few) contributed is off by the size of g or f itself."""
    from oracle import problems_ref as P
    from zfista_amd import _lib

    m, n = case.shape
    A, b, lam, _ = C.shape_data(case.shape)
    cut = C.bounds_of(case.parts)
    x0 = np.random.default_rng(m * 7919 + n).standard_normal(n)
    lr = C.accepted_lr(case.shape, case.scale)
    run = C.Lockstep(A, b, lam, case.parts, case.layout, x0, dict(lr=lr, tol=0.0, max_iter=1, nesterov=True), scale=case.scale)
    try:
        assert tuple(s.ls_plan() for s in run.solvers) == case.plans
        worst_part = 0.0
        if case.layout == "columns":
            for r, part in enumerate(run.s_parts()):
                Ap, xp = A[:, cut[r]:cut[r + 1]], x0[cut[r]:cut[r + 1]]
                exact = Ap.astype(np.longdouble) @ xp.astype(np.longdouble)
                bound = _gamma(xp.size) * (np.abs(Ap) @ np.abs(xp))
                assert part.shape == (m,)
                err = np.abs(part.astype(np.longdouble) - exact).astype(np.float64)
                bad = np.flatnonzero(err > bound)
                assert bad.size == 0, (f"rank {r}: {bad.size} of {m} elements of A_p x0_p outside the fp64 bound, first {bad[:8]}: "
                                       f"error / bound up to {np.max(err[bad] / bound[bad]):.3g}")
                worst_part = max(worst_part, float(np.max(err / np.maximum(bound, 1e-300))))
        ctls = run.finish_init()
        F0, F0_bound, f0, g0 = _F_longdouble(A, b, lam, x0, case.scale)
        # the bound means something: one rank's g too many, or the f of all but one rank missing, exceeds it by orders of magnitude
        assert g0 > 1e3 * F0_bound and f0 > 1e3 * F0_bound
        F0_err = abs(float(np.longdouble(ctls[0].F_old) - F0))
        assert F0_err <= F0_bound, (float(ctls[0].F_old), float(F0), F0_bound, "f", f0, "g", g0)
        if case.layout == "rows":
            run.trial()
            for r, part in enumerate(run.s_parts()):
                Ap, bp = A[cut[r]:cut[r + 1]], b[cut[r]:cut[r + 1]]
                _, g, _, g_bound = P.ls_longdouble(Ap, bp, x0, case.scale)
                assert part.shape == (n,)
                err = np.abs(part.astype(np.longdouble) - g).astype(np.float64)
                bad = np.flatnonzero(err > g_bound)
                assert bad.size == 0, (f"rank {r}: {bad.size} of {n} elements of 2 scale A_p^T r_p outside the fp64 bound, first "
                                       f"{bad[:8]}: error / bound up to {np.max(err[bad] / g_bound[bad]):.3g}")
                worst_part = max(worst_part, float(np.max(err / np.maximum(g_bound, 1e-300))))
            run.finish_trial()
        else:
            run.step()
        ctls = run.poll()
        assert int(ctls[0].nit) == 1 and int(ctls[0].status) == _lib.ZF_MAXITER
        row = run.rows_seen[0]
        assert int(row[_lib.TR_TRIALS]) == 1 and row[_lib.TR_LR] == lr, "lr <= 1 / (2 L): the first trial is accepted"
        x1 = run.x()
        assert x1.shape == (n,) and not np.array_equal(x1, x0)
        F1, F1_bound, f1, g1 = _F_longdouble(A, b, lam, x1, case.scale)
        assert g1 > 1e3 * F1_bound and f1 > 1e3 * F1_bound
        F1_err = abs(float(np.longdouble(row[_lib.TR_F]) - F1))
        assert F1_err <= F1_bound, (float(row[_lib.TR_F]), float(F1), F1_bound, "f", f1, "g", g1)
        assert ctls[0].F_old == row[_lib.TR_F]
        _record(case=case.name, layout=case.layout, shape=list(case.shape), parts=list(case.parts), scale=case.scale,
                part_worst_ratio=worst_part, F0_ratio=F0_err / F0_bound, F1_ratio=F1_err / F1_bound)
    finally:
        run.close()


@pytest.mark.parametrize("case", C.SHAPE_CASES, ids=SHAPE_IDS)
def test_shape_case_solve_vs_oracle(case):
    """30 iterations of FISTA from lr = 1 (the line search backtracks) against the oracle on the unsharded problem: nit, status,
    the lr and the trial sequence exactly; every iterate, F and err to 1e-10."""
    A, b, lam, _ = C.shape_data(case.shape)
    exp = C.shape_oracle(case.name)
    run = C.Lockstep(A, b, lam, case.parts, case.layout, C.solve_x0(case), C.SOLVE_OPTIONS, scale=case.scale)
    try:
        assert tuple(s.ls_plan() for s in run.solvers) == case.plans
        res = run.run(chunk=1)
    finally:
        run.close()
    assert res.nit == 30 and res.allvecs is not None
    C.compare_with_oracle(res, exp)


@pytest.mark.parametrize("name", ["C1", "R4"])
def test_polling_every_16_steps_gives_the_same_bits(name):
    """The steps of a chunk are enqueued without a host synchronisation between them; steps behind the end of the solve do
    nothing."""
    case = C.SHAPE_BY_NAME[name]
    A, b, lam, _ = C.shape_data(case.shape)
    out = []
    for chunk in (1, 16):
        run = C.Lockstep(A, b, lam, case.parts, case.layout, C.solve_x0(case), C.SOLVE_OPTIONS, scale=case.scale)
        try:
            out.append(run.run(chunk=chunk))
        finally:
            run.close()
    one, many = out
    assert many.steps >= one.steps and many.steps % 16 == 0
    assert one.nit == many.nit == 30 and one.status == many.status
    assert np.array_equal(one.x, many.x)
    assert one.allfuns == many.allfuns and one.allerrs == many.allerrs and one.alllrs == many.alllrs and one.alltrials == many.alltrials


@pytest.mark.parametrize("name", ["C1", "R4"])
def test_kernel_timing_in_lockstep_changes_no_bit(name):
    """zf_solver_set_timing on the two-halves sequence.  Row blocks: the first half of a trial returns before the prox step
    and gives the event pair it took back (zf_collect_timing would otherwise read events that were never recorded: an error,
    or garbage); column blocks: the pair brackets the trial kernels.  The timing calls succeed, and the solve is the untimed
    one bit for bit."""
    case = C.SHAPE_BY_NAME[name]
    A, b, lam, _ = C.shape_data(case.shape)
    out = []
    for timing in (False, True):
        run = C.Lockstep(A, b, lam, case.parts, case.layout, C.solve_x0(case), C.SOLVE_OPTIONS, scale=case.scale, timing=timing)
        try:
            res = run.run(chunk=3)
            if timing:
                for s in run.solvers:
                    ms, cnt = s.trial_kernel_ms()
                    assert ms >= 0.0 and 0 <= cnt <= res.steps
                    assert case.layout == "rows" or (cnt > 0 and ms > 0.0)
                    (fm, fn), (pm, pn) = s.pass_stats()
                    assert fm >= 0.0 and pm >= 0.0 and fn + pn <= res.steps
            out.append(res)
        finally:
            run.close()
    plain, timed = out
    assert plain.nit == timed.nit == 30 and plain.steps == timed.steps
    assert np.array_equal(plain.x, timed.x)
    assert plain.allfuns == timed.allfuns and plain.alllrs == timed.alllrs and plain.alltrials == timed.alltrials


@pytest.mark.parametrize("spec", C.SWEEP, ids=[C.spec_id(sp) for sp in C.SWEEP])
def test_option_sweep_vs_oracle(spec):
    """One seeded case of the sweep against the oracle on the unsharded problem: nit, success, status, message, the lr and the
    trial sequence exactly; every iterate, the F and err traces to 1e-10; all ranks bit-identical at every poll (the driver)."""
    A, b, lam, x0, o, exp = C.oracle(spec)
    run = C.Lockstep(A, b, lam, spec.parts, spec.layout, x0, o, scale=0.5, bounds=spec.bounds)
    try:
        blocks = C.block_shapes(spec.shape, spec.parts, spec.layout)
        assert [s.ls_plan() for s in run.solvers] == [C.dispatch(mp, np_, spec.world) for mp, np_ in blocks]
        res = run.run(chunk=1)
    finally:
        run.close()
    C.compare_with_oracle(res, exp)
    assert res.steps <= o["max_iter"] * o["max_backtrack_iter"]


@pytest.mark.parametrize("case", C.THREAD_CASES, ids=[f"{c.layout}-{c.name}" for c in C.THREAD_CASES])
def test_library_sequence_with_thread_ranks(case):
    """The library's OWN multi-rank sequence (zf_solver_enqueue_init_all / zf_solver_enqueue_steps with a communicator attached:
    the exchange of the s vectors and of the packs on the stream) through LibComm.local_group and the public
    LeastSquaresL1(..., group=, shard=): an uneven split, an active box with ISTA, and x0 != 0 with a run that tol ends.  Every
    rank's arrays and problem are built, and every argument is checked, before any thread starts."""
    import threading

    import torch

    from oracle import problems_ref as P
    from zfista_amd import minimize_proximal_gradient
    from zfista_amd.comm import LibComm
    from zfista_amd.problems import LeastSquaresL1

    A, b, lam, x0 = C.thread_inputs(case)
    kw = dict(case.options, return_all=True)
    exp = C.run_ref(P.LeastSquaresL1Ref(A, b, lam, scale=case.scale, bounds=case.bounds), x0, case.options)
    world, cut, rows = len(case.parts), C.bounds_of(case.parts), case.layout == "rows"
    comms = LibComm.local_group(world, cap_doubles=4096)
    threads = []
    try:
        probs, starts = [], []
        for r in range(world):
            lo, hi = cut[r], cut[r + 1]
            if rows:
                prob = LeastSquaresL1(np.ascontiguousarray(A[lo:hi]), b[lo:hi].copy(), lam, scale=case.scale, bounds=case.bounds,
                                      group=comms[r], shard="rows")
                xr = x0.copy()
            else:
                prob = LeastSquaresL1(np.ascontiguousarray(A[:, lo:hi]), b, lam, scale=case.scale, bounds=case.bounds, group=comms[r])
                xr = x0[lo:hi].copy()
            assert xr.size == prob.n_features and prob._descriptor()[0]["world"] == world and prob._descriptor()[0]["rank"] == r
            assert prob._descriptor()[0]["row_sharded"] == int(rows)
            probs.append(prob)
            starts.append(xr)
        torch.cuda.synchronize()
        out, errs = [None] * world, []

        def rank_main(r):
            try:
                with torch.cuda.stream(torch.cuda.Stream()):
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        out[r] = minimize_proximal_gradient(*probs[r].callbacks(), starts[r], **kw)
                    torch.cuda.current_stream().synchronize()
            except Exception as exc:   # pragma: no cover - reported below
                errs.append(exc)

        threads = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
        assert not errs, errs
        assert all(o is not None for o in out), "a rank thread did not finish"
    finally:
        if not any(t.is_alive() for t in threads):   # (a rank that still waits holds its communicator)
            for c_ in comms:
                c_.close()
    for res in out:
        assert res.nit == exp.nit == out[0].nit and res.fun == out[0].fun, "ranks must agree bit for bit"
        assert res.success == exp.success and res.message == exp.message and res.status == exp.status
        assert np.array_equal(np.asarray(res.allfuns), np.asarray(out[0].allfuns))
        assert np.array_equal(np.asarray(res.allerrs), np.asarray(out[0].allerrs))
    if rows:
        for k in range(exp.nit + 1):
            assert all(np.array_equal(o.allvecs[k], out[0].allvecs[k]) for o in out), "the replicated x must be identical on every rank"
        cat = lambda vs: vs[0]   # noqa: E731
    else:
        cat = np.concatenate
    assert np.linalg.norm(cat([o.x for o in out]) - exp.x) <= 1e-10 * np.linalg.norm(exp.x)
    for k in range(exp.nit + 1):
        xk = cat([o.allvecs[k] for o in out])
        assert np.linalg.norm(xk - exp.allvecs[k]) <= 1e-10 * max(np.linalg.norm(exp.allvecs[k]), 1e-300), k
    np.testing.assert_allclose(out[0].allfuns, exp.allfuns, rtol=1e-10)
    xmax = float(np.max(np.abs(np.stack(exp.allvecs))))
    np.testing.assert_allclose(out[0].allerrs, exp.allerrs, rtol=1e-10, atol=1e-10 * xmax)
    if case.bounds is not None:
        X = np.stack([cat([o.allvecs[k] for o in out]) for k in range(1, exp.nit + 1)])
        assert X.min() >= case.bounds[0] and X.max() <= case.bounds[1]
        assert np.count_nonzero((X == case.bounds[0]) | (X == case.bounds[1])) >= 30, "the box should be active"


@pytest.mark.parametrize("layout", ["columns", "rows"])
def test_restore_is_refused_and_leaves_the_solver_usable(layout):
    """zf_solver_restore on a sharded least-squares solver returns its error - before it has touched the solver: the solve that
    was under way goes on to the oracle's result."""
    import torch

    from zfista_amd import _lib

    spec = next(sp for sp in C.SWEEP if sp.layout == layout and sp.shape == (40, 64) and C.ending(C.oracle(sp)[5]) == "max_iter"
                and C.oracle(sp)[5].nit >= 5)
    A, b, lam, x0, o, exp = C.oracle(spec)
    run = C.Lockstep(A, b, lam, spec.parts, spec.layout, x0, o, scale=0.5, bounds=spec.bounds)
    try:
        ctls = run.finish_init()
        for _ in range(3):
            run.step()
        ctls = run.poll()
        assert int(ctls[0].status) == _lib.ZF_RUNNING
        for s in run.solvers:
            junk = torch.full((s.n,), 7.0, dtype=torch.float64, device="cuda")
            saved = _lib.Control.from_buffer_copy(bytes(s.ctl))
            with pytest.raises(_lib.ZfError, match="sharded least squares is not supported"):
                s.restore(junk.data_ptr(), junk.data_ptr(), saved)
        res = run.run(chunk=1)
    finally:
        run.close()
    C.compare_with_oracle(res, exp)


@pytest.mark.parametrize("shard", ["columns", "rows"])
def test_a_sharded_least_squares_problem_accepts_a_box(shard):
    from oracle import problems_ref as P
    from zfista_amd.comm import LibComm
    from zfista_amd.problems import LeastSquaresL1

    A, b, lam = P.make_plasso(6, 4, seed=0, n_informative=2)
    comms = LibComm.local_group(2, cap_doubles=64)
    try:
        prob = LeastSquaresL1(A, b, lam, bounds=(-0.05, 0.08), group=comms[1], shard=shard)
        fields, _ = prob._descriptor()
        assert (fields["box_lo"], fields["box_hi"]) == (-0.05, 0.08)
        assert (fields["world"], fields["rank"], fields["row_sharded"]) == (2, 1, int(shard == "rows"))
    finally:
        for c_ in comms:
            c_.close()
