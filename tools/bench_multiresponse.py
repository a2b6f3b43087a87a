#!/usr/bin/env python3
"""Rate of a K-response dense LASSO solve (MultiResponseLeastSquaresL1) beside the plain LeastSquaresL1 sibling on the SAME device
matrix, one JSON line per process.

    python tools/bench_multiresponse.py --m 16384 --n 65536 --ks 2,4,8,16 --repeats 3    # BASELINE cfg3's shape
    python tools/bench_multiresponse.py --m 16384 --n 65536 --ks 8 --repeats 1 --steps 16   # a short run for a kernel trace

The protocol is tools/bench_f32.py's (its builder, step rule and timed window are imported): the matrix is drawn in HBM, seeded;
W untimed passes, a synchronise, S timed passes of NativeRun.advance between two HIP events on the solver's stream, a synchronise;
FISTA with lr = 0.9 / |A|_2^2, so every trial is accepted and runs both sweeps; one trial per pass.  The K right-hand sides are the
builder's b plus independent noise, ``plain.with_responses(B)`` shares the matrix.  The runs are ALTERNATED `repeats` times in this
one process - plain, K = 2, 4, ..., plain, ... - each a fresh solver on the resident problems: the plain sibling's kernels are the
yardstick, and alternation keeps clocks and neighbours the same for all.

Reported per K (and for "plain"): ms per trial (wall and HIP events) of every repeat with median and spread (max - min), accepted
iterations per second, the plan, and the fraction of 8 TB/s the two sweeps of a trial reach on the bytes of A together with
everything else a trial launches (2 m n 8 bytes over the event time of a trial: a lower bound of the sweeps' own fraction).
Per K also t_K / t_1, K t_1 / t_K (how many plain trials one K-response trial replaces) and `beats_k_plain_trials`:
t_K + spread_K < K (t_1 - spread_1)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_f32 import lipschitz, timed_run  # noqa: E402
from tools.bench_logistic import build_dense  # noqa: E402
from tools.bench_sparse import PEAK_BYTES_PER_S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--ks", default="2,4,8,16")
    ap.add_argument("--plain", type=int, default=1, help="0: leave the plain sibling out (a profiler run of one K)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import torch

    from zfista_amd.problems import LeastSquaresL1

    t0 = time.time()
    A, b, _, _, _ = build_dense(args)
    m, n = int(A.shape[0]), int(A.shape[1])
    ks = [int(v) for v in args.ks.split(",") if v]
    plain = LeastSquaresL1(A, b, 1.0)
    lam = 0.1 * float(plain.lam_max())
    lr = 0.9 / lipschitz(A)
    plain = plain.with_lam(lam)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed + 1)
    probs = {}
    for K in ks:
        B = b.reshape(m, 1) + 0.01 * torch.randn(m, K, dtype=torch.float64, device="cuda", generator=gen)
        probs[K] = plain.with_responses(B.cpu().numpy())
        assert probs[K].A.data_ptr() == plain.A.data_ptr()
    out = dict(tool="bench_multiresponse", label=args.label, m=m, n=n, seed=args.seed, ks=ks, warmup=args.warmup, steps=args.steps,
               repeats=args.repeats, lam=lam, lr=lr, build_s=round(time.time() - t0, 2))
    print(f"built {m} x {n} in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    runs = {k: [] for k in (["plain"] if args.plain else []) + ks}
    for _ in range(args.repeats):
        for k in runs:   # alternated: plain, K = 2, 4, ..., plain, ...
            p = plain if k == "plain" else probs[k]
            runs[k].append(timed_run(p, p.n_features, args.warmup, args.steps, lr))
    nbytes = 2 * m * n * 8
    for k, rs in runs.items():
        ev, wall = [r["ms_per_trial_events"] for r in rs], [r["ms_per_trial_wall"] for r in rs]
        out[str(k)] = dict(plan=rs[0]["plan"], it_per_s=[r["it_per_s"] for r in rs], it_per_s_median=float(np.median([r["it_per_s"] for r in rs])),
                           ms_per_trial_wall=wall, ms_per_trial_events=ev, ms_per_trial_events_median=float(np.median(ev)),
                           ms_per_trial_events_spread=float(max(ev) - min(ev)), accepted=[r["accepted"] for r in rs],
                           warmup_accepted=[r["warmup_accepted"] for r in rs],
                           trial_fraction_of_8TBps=nbytes / (1e-3 * float(np.median(ev))) / PEAK_BYTES_PER_S)
    out["windows_all_accepted"] = all(a == args.steps for k in runs for a in out[str(k)]["accepted"])
    if args.plain:
        t1, s1 = out["plain"]["ms_per_trial_events_median"], out["plain"]["ms_per_trial_events_spread"]
        for K in ks:
            o = out[str(K)]
            o["t_over_t1"] = o["ms_per_trial_events_median"] / t1
            o["plain_trials_replaced"] = K * t1 / o["ms_per_trial_events_median"]
            o["beats_k_plain_trials"] = bool(o["ms_per_trial_events_median"] + o["ms_per_trial_events_spread"] < K * (t1 - s1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
