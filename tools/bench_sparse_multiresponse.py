#!/usr/bin/env python3
"""Rate of a K-response sparse LASSO solve (SparseMultiResponseLeastSquaresL1) beside the plain SparseLeastSquaresL1 sibling on
the SAME matrix handle and beside what a user could do before: the plain class on sp.kron(A, I_K).  One JSON line per process.

    python tools/bench_sparse_multiresponse.py --m 200000 --n 1000003 --per-col 8 --ks 2,4,8,16 --kron 4,16 --repeats 3
    python tools/bench_sparse_multiresponse.py --m 8192 --n 32768 --density 0.01 --ks 2,4,8,16 --kron 4,16 --repeats 3
    python tools/bench_sparse_multiresponse.py ... --ks 8 --kron "" --repeats 1 --warmup 4 --steps 12     # a short run for a kernel trace

The matrix is tools/bench_sparse.py's (its builder is imported), the timed window tools/bench_f32.py's: W untimed passes, a
synchronise, S timed passes of NativeRun.advance between two HIP events on the solver's stream, a synchronise; FISTA with
lr = 0.9 / |A|_2^2, so every trial is accepted and runs both sweeps; one trial per pass.  The K right-hand sides are b plus
independent noise; ``plain.with_responses(B)`` shares the handle.  The runs are ALTERNATED `repeats` times in this one process -
plain, K = 2, 4, ..., kron 4, ..., plain, ... - each a fresh solver on the resident problems.

Reported per run: ms per trial (wall and HIP events) of every repeat with median and spread (max - min), the plan, and the bytes
model of the two sweeps of a trial - 12 nnz + 8 K (rows out) per sweep, the gathered input not counted - with the fraction of
8 TB/s the whole trial reaches on them (a lower bound of the sweeps' own).  Per K: t_K / t_1, K t_1 / t_K (the plain trials one
K-response trial replaces) and `beats_k_plain_trials`: t_K + spread_K < K (t_1 - spread_1); where the Kronecker form ran,
t_kron / t_K and `beats_kron`: t_K + spread_K < t_kron - spread_kron."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_f32 import timed_run  # noqa: E402
from tools.bench_sparse import PEAK_BYTES_PER_S, build, lengths  # noqa: E402


def lipschitz(A):
    """|A|_2^2 by 20 power iterations on the host (input preparation; the step keeps a tenth of margin)."""
    AT = A.T.tocsr()
    v = np.ones(A.shape[1])
    for _ in range(20):
        v = AT @ (A @ v)
        v /= np.linalg.norm(v)
    return float(np.linalg.norm(A @ v)) ** 2


def sweep_bytes(m, n, nnz, K):
    return (12 * nnz + 8 * K * m) + (12 * nnz + 8 * K * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200_000)
    ap.add_argument("--n", type=int, default=1_000_003)
    ap.add_argument("--per-col", type=int, default=8)
    ap.add_argument("--density", type=float, default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--skew", action="store_true")
    ap.add_argument("--ks", default="2,4,8,16")
    ap.add_argument("--kron", default="4,16", help="K for which the plain class on sp.kron(A, I_K) runs beside the others")
    ap.add_argument("--plain", type=int, default=1, help="0: leave the plain sibling out (a profiler run of one K)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import scipy.sparse as sp

    from zfista_amd.problems import SparseLeastSquaresL1

    t0 = time.time()
    A, b, _ = build(args)
    m, n = A.shape
    ks = [int(v) for v in args.ks.split(",") if v]
    krons = [int(v) for v in args.kron.split(",") if v]
    lr = 0.9 / lipschitz(A)
    plain = SparseLeastSquaresL1(A, b, 1.0)
    rng = np.random.default_rng(args.seed + 1)
    Bs = {K: b.reshape(m, 1) + 0.01 * rng.standard_normal((m, K)) for K in sorted(set(ks + krons))}
    lam = 0.1 * float(np.max(np.abs(A.T @ b)))
    plain = plain.with_lam(lam)
    probs = {}
    for K in ks:
        probs[K] = plain.with_responses(Bs[K])
        assert probs[K]._spmat is plain._spmat
    for K in krons:
        t1 = time.time()
        probs[f"kron{K}"] = SparseLeastSquaresL1(sp.kron(A, sp.identity(K, format="csr"), format="csr"), Bs[K].reshape(-1), lam)
        print(f"kron K = {K} prepared in {time.time() - t1:.1f} s", file=sys.stderr, flush=True)
    out = dict(tool="bench_sparse_multiresponse", label=args.label, m=m, n=n, nnz=int(A.nnz), seed=args.seed, ks=ks, kron=krons,
               row_len_A=lengths(A.indptr), row_len_At=lengths(A.T.tocsr().indptr), warmup=args.warmup, steps=args.steps,
               repeats=args.repeats, lam=lam, lr=lr, build_s=round(time.time() - t0, 2))
    print(f"built {m} x {n}, nnz {A.nnz} in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    runs = {k: [] for k in (["plain"] if args.plain else []) + ks + [f"kron{K}" for K in krons]}
    for _ in range(args.repeats):
        for k in runs:   # alternated: plain, K = 2, 4, ..., kron 4, ..., plain, ...
            p = plain if k == "plain" else probs[k]
            runs[k].append(timed_run(p, p.n_features, args.warmup, args.steps, lr))
    for k, rs in runs.items():
        ev, wall = [r["ms_per_trial_events"] for r in rs], [r["ms_per_trial_wall"] for r in rs]
        K = 1 if k == "plain" else int(str(k).replace("kron", ""))
        nbytes = sweep_bytes(m * K, n * K, A.nnz * K, 1) if str(k).startswith("kron") else sweep_bytes(m, n, A.nnz, K)
        out[str(k)] = dict(plan=rs[0]["plan"], ms_per_trial_wall=wall, ms_per_trial_events=ev, ms_per_trial_events_median=float(np.median(ev)),
                           ms_per_trial_events_spread=float(max(ev) - min(ev)), accepted=[r["accepted"] for r in rs],
                           warmup_accepted=[r["warmup_accepted"] for r in rs], sweep_bytes_model=int(nbytes),
                           trial_fraction_of_8TBps=nbytes / (1e-3 * float(np.median(ev))) / PEAK_BYTES_PER_S)
    out["windows_all_accepted"] = all(a == args.steps for k in runs for a in out[str(k)]["accepted"])
    if args.plain:
        t1, s1 = out["plain"]["ms_per_trial_events_median"], out["plain"]["ms_per_trial_events_spread"]
        for K in ks:
            o = out[str(K)]
            o["t_over_t1"] = o["ms_per_trial_events_median"] / t1
            o["plain_trials_replaced"] = K * t1 / o["ms_per_trial_events_median"]
            o["beats_k_plain_trials"] = bool(o["ms_per_trial_events_median"] + o["ms_per_trial_events_spread"] < K * (t1 - s1))
    for K in krons:
        if K in ks:
            o, kr = out[str(K)], out[f"kron{K}"]
            o["kron_over_t"] = kr["ms_per_trial_events_median"] / o["ms_per_trial_events_median"]
            o["beats_kron"] = bool(o["ms_per_trial_events_median"] + o["ms_per_trial_events_spread"] <
                                   kr["ms_per_trial_events_median"] - kr["ms_per_trial_events_spread"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
