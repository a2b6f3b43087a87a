#!/usr/bin/env python3
"""Rate of a dense LASSO solve on a matrix stored in fp32 (matrix_dtype="float32") beside its fp64 sibling on the SAME matrix,
one JSON line per process.

    python tools/bench_f32.py --m 16384 --n 65536 --warmup 48 --repeats 3      # BASELINE cfg3's shape
    python tools/bench_f32.py --m 16384 --n 65536 --dtype float32 --repeats 1  # one storage alone (a profiler run)

The protocol is tools/bench_logistic.py's (its builder is imported): the matrix is drawn in HBM, seeded, and ROUNDED TO FP32
FIRST - the fp64 sibling holds float64(float32(A)), so both solve the same problem - W untimed passes, a synchronise, K timed
passes of NativeRun.advance between two HIP events on the solver's stream, a synchronise; FISTA with lr = 0.9 / |A|_2^2 (20 power
iterations on the stored matrix, untimed: tools/bench_configs.py's cfg3), so every trial is accepted and runs both sweeps; one
trial per pass.  --dtype both (default) ALTERNATES the two storages `repeats` times in this one process - float64, float32, float64,
... - each run a fresh solver on the resident problem: the fp64 sibling's code is the yardstick, and alternation keeps
clocks and neighbours the same for both.

Reported per storage: accepted iterations per second and ms per trial (wall and HIP events) of every repeat with their
medians, the plan, and the fraction of 8 TB/s the two sweeps of a trial reach TOGETHER WITH everything else a trial launches:
2 m n B bytes (B = 4 or 8) over the event time of a trial - a lower bound of the sweeps' own fraction, which a kernel trace
of a --dtype float32 / --dtype float64 run gives per kernel.  speedup = the ratio of the median event times; it means what it
says only when every timed trial of both was accepted (a rejected trial is followed by one without the A^T sweep):
windows_all_accepted."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_logistic import build_dense  # noqa: E402
from tools.bench_sparse import PEAK_BYTES_PER_S  # noqa: E402

OPTS = dict(lr=1, tol=0.0, tol_internal=1e-12, max_iter=10 ** 9, max_iter_internal=100000, max_backtrack_iter=100, warm_start=False,
            decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False, deprecated=False)


def lipschitz(A32):
    """|A|_2^2 by 20 power iterations, in the matrix's own precision (input preparation; the step keeps a tenth of margin)."""
    import torch

    v = torch.ones(A32.shape[1], dtype=A32.dtype, device=A32.device)
    for _ in range(20):
        v = A32.T @ (A32 @ v)
        v /= torch.linalg.norm(v)
    return float(torch.linalg.norm(A32 @ v)) ** 2


def timed_run(prob, n, warmup, steps, lr):
    import torch

    from zfista_amd.proximal_gradient import NativeRun

    run = NativeRun(prob, np.zeros(n), dict(OPTS, lr=lr))
    plan = list(run.solver.ls_plan())
    warm = run.advance(warmup)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    e0.record()
    rows = run.advance(steps)
    e1.record()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t1
    run.solver.close()
    return dict(plan=plan, warmup_accepted=len(warm), accepted=len(rows), it_per_s=len(rows) / dt, ms_per_trial_wall=1e3 * dt / steps,
                ms_per_trial_events=e0.elapsed_time(e1) / steps, lr=float(rows[-1][2]) if len(rows) else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--dtype", choices=("both", "float32", "float64"), default="both")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=48)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import torch

    from zfista_amd.problems import LeastSquaresL1

    t0 = time.time()
    A, b, _, _, _ = build_dense(args)
    A32 = A.to(torch.float32)
    del A
    m, n = int(A32.shape[0]), int(A32.shape[1])
    probs = {}
    if args.dtype in ("both", "float32"):
        probs["float32"] = LeastSquaresL1(A32, b, 1.0, matrix_dtype="float32")
        assert probs["float32"].A.data_ptr() == A32.data_ptr()
    if args.dtype in ("both", "float64"):
        probs["float64"] = LeastSquaresL1(A32.to(torch.float64), b, 1.0)
    lam = 0.1 * float(next(iter(probs.values())).lam_max())   # (a tenth of the smallest lam that gives x = 0)
    lr = 0.9 / lipschitz(A32)
    probs = {k: p.with_lam(lam) for k, p in probs.items()}
    out = dict(tool="bench_f32", label=args.label, dtype=args.dtype, m=m, n=n, seed=args.seed, warmup=args.warmup, steps=args.steps,
               repeats=args.repeats, lam=lam, lr=lr, build_s=round(time.time() - t0, 2))
    print(f"built {m} x {n} in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    runs = {k: [] for k in probs}
    for _ in range(args.repeats):
        for k in sorted(probs, reverse=True):   # alternated: float64, float32, float64, ...
            runs[k].append(timed_run(probs[k], n, args.warmup, args.steps, lr))
    for k, rs in runs.items():
        ev, wall = [r["ms_per_trial_events"] for r in rs], [r["ms_per_trial_wall"] for r in rs]
        nbytes = 2 * m * n * (4 if k == "float32" else 8)
        out[k] = dict(plan=rs[0]["plan"], it_per_s=[r["it_per_s"] for r in rs], it_per_s_median=float(np.median([r["it_per_s"] for r in rs])),
                      ms_per_trial_wall=wall, ms_per_trial_wall_median=float(np.median(wall)), ms_per_trial_events=ev,
                      ms_per_trial_events_median=float(np.median(ev)), accepted=[r["accepted"] for r in rs],
                      warmup_accepted=[r["warmup_accepted"] for r in rs], lr=rs[-1]["lr"], sweep_bytes_per_trial=nbytes,
                      trial_fraction_of_8TBps=nbytes / (1e-3 * float(np.median(ev))) / PEAK_BYTES_PER_S)
    if len(runs) == 2:
        out["windows_all_accepted"] = all(a == args.steps for k in runs for a in out[k]["accepted"])
        out["speedup_events"] = out["float64"]["ms_per_trial_events_median"] / out["float32"]["ms_per_trial_events_median"]
        out["speedup_it_per_s"] = out["float32"]["it_per_s_median"] / out["float64"]["it_per_s_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
