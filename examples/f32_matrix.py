#!/usr/bin/env python3
"""The same LASSO path on a dense matrix stored in fp64 and in fp32.

A design matrix is rarely known to more than seven digits; stored in fp32 it takes half the HBM and both sweeps of a trial
read half the bytes.  Everything else stays double - the iterates, the residuals, every sum - and float32 -> float64 is
exact, so the fp32 problem is, in fp64 arithmetic, exactly the fp64 problem on the rounded matrix: the two paths below are
run on ``A32`` and on ``A32.double()`` and agree to rounding wherever both stop at the same iteration (a gap check that lands on
``gap_tol`` within rounding may stop one of them a check earlier; both are then solved to the tolerance asked for).  The last
column shows what the rounding itself costs: the distance to the path on the matrix as generated.

    python examples/f32_matrix.py [--m 4096 --n 16384 --points 6]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zfista_amd.path import l1_path  # noqa: E402
from zfista_amd.problems import LeastSquaresL1  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--points", type=int, default=6)
    args = ap.parse_args()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    A = torch.randn(args.m, args.n, dtype=torch.float64, device="cuda", generator=gen)
    x_true = torch.zeros(args.n, dtype=torch.float64, device="cuda")
    x_true[:20] = torch.randn(20, dtype=torch.float64, device="cuda", generator=gen)
    b = A @ x_true + 0.01 * torch.randn(args.m, dtype=torch.float64, device="cuda", generator=gen)

    full = LeastSquaresL1(A, b, 1.0)                               # the matrix as generated, fp64
    p32 = LeastSquaresL1(A, b, 1.0, matrix_dtype="float32")        # rounded to nearest on the device; A32 = p32.A
    p64 = p32.with_matrix_dtype("float64")                         # float64(A32): the same problem, stored in fp64
    print(f"{args.m} x {args.n}: {p64.A.numel() * 8 / 2**20:.0f} MiB as float64, {p32.A.numel() * 4 / 2**20:.0f} MiB as float32")
    lam_max = float(p64.lam_max())
    assert abs(float(p32.lam_max()) - lam_max) <= 1e-10 * lam_max
    lams = lam_max * np.logspace(-0.3, -1.5, args.points)
    gap_tol = 1e-6 * float(p64.with_lam(lams[-1]).duality_gap(np.zeros(args.n)).primal)
    paths, secs = {}, {}
    for name, prob in (("float64", p64), ("float32", p32), ("unrounded", full)):
        t0 = time.time()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            paths[name] = l1_path(prob, lams, gap_tol=gap_tol, lr=1.0, nesterov=True, tol=0.0, max_iter=5000)
        secs[name] = time.time() - t0
    print(f"path of {args.points} points: float64 {secs['float64']:.2f} s, float32 {secs['float32']:.2f} s")
    print(f"{'lam / lam_max':>14} {'nit 64':>7} {'nit 32':>7} {'gap 32':>11} {'nonzeros':>9} {'|x32 - x64| / |x64|':>20} {'|x32 - x_unrounded| / |x|':>26}")
    for r64, r32, ru in zip(paths["float64"], paths["float32"], paths["unrounded"]):
        den = max(np.linalg.norm(r64.x), 1e-300)
        print(f"{r32.lam / lam_max:14.5f} {r64.nit:7d} {r32.nit:7d} {r32.dual_gap:11.3e} {np.count_nonzero(r32.x):9d} "
              f"{np.linalg.norm(r32.x - r64.x) / den:20.3e} {np.linalg.norm(r32.x - ru.x) / den:26.3e}")


if __name__ == "__main__":
    main()
