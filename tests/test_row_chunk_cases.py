"""CPU: the sizes of tests/row_chunk_cases.py sit on the edges of the chunk cap of the rows passes, the restated launch shape is
the one in zfista_amd/csrc/zf_spmv.hip, and the bound that tests/test_gpu_row_chunk_cap.py holds f to would notice a walk that
misses the last chunk, the last row or the fifth trip of the first chunk: each moves the long-double f of the test's own margins
by more than 100 times that bound."""
import os
import re

import numpy as np
import pytest

import row_chunk_cases as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "zfista_amd", "csrc")


def test_the_launch_shape_is_restated_from_the_source():
    """zf_spmv_resid_chunks and its cap, as they stand in the source: the kernels take `per` from their own grid, so a cap of
    another value computes the same f in another order - no value test can see it; this restatement can."""
    with open(os.path.join(CSRC, "zf_spmv.h")) as fh:
        assert int(re.search(r"constexpr int ZF_SPMV_RESID_MAX_CHUNKS = (\d+);", fh.read()).group(1)) == R.MAX_CHUNKS
    with open(os.path.join(CSRC, "zf_spmv.hip")) as fh:
        body = re.search(r"int zf_spmv_resid_chunks\(int64_t m\) \{(.*?)\n\}", fh.read(), re.S).group(1)
    lines = [" ".join(l.split()) for l in body.strip().splitlines()]
    assert lines == ["int64_t chunks = (m + 1023) / 1024;", "if (chunks < 1) chunks = 1;",
                     "if (chunks > ZF_SPMV_RESID_MAX_CHUNKS) chunks = ZF_SPMV_RESID_MAX_CHUNKS;", "return (int)chunks;"]
    with open(os.path.join(CSRC, "zf_kernels_loss.h")) as fh:   # the ONE rows kernel of the four losses, with or without weights
        text = fh.read()
    assert text.count("__global__") == 2 and "void zf_loss_rows_kernel(" in text and "void zf_rows_finish_kernel(" in text
    assert "const int64_t per = (m + gridDim.x - 1) / gridDim.x;" in text
    assert "const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < m ? lo + per : m;" in text
    assert "for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {" in text


def test_the_sizes_sit_on_the_edges_of_the_cap():
    assert (R.M0, R.M1, R.M2) == (2 ** 20, 2 ** 20 + 1, 2 ** 21 + 3)
    for m in (1, 1024, 1025, 40000, 200_000):   # the largest row counts the suite had: far below the cap
        assert R.chunks(m) == -(-m // 1024) < R.MAX_CHUNKS and R.per_chunk(m) <= 1024
    # M0: the last size below the cap branch - 1024 chunks of 1024 rows, four trips for every thread
    assert R.chunks(R.M0) == 1024 and R.per_chunk(R.M0) == 1024 and -(-R.M0 // 1024) == 1024
    assert all(R.chunk_range(R.M0, k) == (1024 * k, 1024 * (k + 1)) for k in (0, 1, 1023))
    assert {R.trips(R.M0, k, t) for k in (0, 511, 1023) for t in (0, 1, 255)} == {4} and R.fifth_trip_rows(R.M0).size == 0
    # M1: the first size the cap cuts - per = 1025, a fifth trip for thread 0 only, a last chunk of two rows
    assert -(-R.M1 // 1024) == 1025 and R.chunks(R.M1) == 1024 and R.per_chunk(R.M1) == 1025
    assert [R.trips(R.M1, 0, t) for t in (0, 1, 255)] == [5, 4, 4] and list(R.fifth_trip_rows(R.M1)) == [1024]
    assert R.chunk_range(R.M1, 1023) == (R.M1 - 2, R.M1) and R.trips(R.M1, 1023, 0) == R.trips(R.M1, 1023, 1) == 1 and R.trips(R.M1, 1023, 2) == 0
    # M2: per = 2049, nine trips, a last chunk of 1028 rows
    assert R.per_chunk(R.M2) == 2049 and [R.trips(R.M2, 0, t) for t in (0, 1, 255)] == [9, 8, 8]
    lo, hi = R.chunk_range(R.M2, 1023)
    assert hi == R.M2 and hi - lo == 1028 and [R.trips(R.M2, 1023, t) for t in (0, 3, 4, 255)] == [5, 5, 4, 4]
    for m in R.SIZES:   # the chunks tile [0, m) without a gap
        edges = [R.chunk_range(m, k) for k in range(R.chunks(m))]
        assert edges[0][0] == 0 and edges[-1][1] == m and all(a[1] == b[0] for a, b in zip(edges, edges[1:]))
        at = R.special_rows(m)
        assert len(set(at.values())) == 5 and at["last_lo"] == edges[-1][0] and at["last"] == m - 1
        assert edges[-1][0] <= at["last_lo"] < m
        if m > R.M0:
            assert at["fifth"] in R.fifth_trip_rows(m) and (at["fifth"] - 0) % R.BLOCK == 0


@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("m", [R.M1, R.M2])
def test_a_walk_that_misses_rows_moves_f_by_more_than_100_bounds(m, loss):
    z, b = R.margins(loss, m)
    at = R.special_rows(m)
    assert z[at["zero"]] == 0 and not np.signbit(z[at["zero"]]) and np.signbit(z[at["neg_zero"]]) and z[at["neg_zero"]] == 0
    assert abs(z[at["fifth"]]) == abs(z[at["last_lo"]]) == abs(z[at["last"]]) == R.BIG
    f, bound, _, _ = R.loss_reference(loss, z, b)
    assert np.isfinite(float(f)) and 0 < bound < 1e-6 * abs(float(f))
    lo_last = R.chunk_range(m, R.chunks(m) - 1)[0]
    drops = {"the last chunk": np.arange(lo_last, m), "the last row": np.array([m - 1]), "the fifth trip of the first chunk": R.fifth_trip_rows(m)}
    for what, rows in drops.items():
        keep = np.ones(m, bool)
        keep[rows] = False
        f_wrong = R.loss_reference(loss, z[keep], b[keep])[0]
        ratio = abs(float(f - f_wrong)) / bound
        print(f"m={m} {loss}: dropping {what} ({rows.size} rows) moves f by {ratio:.3g} bounds")
        assert ratio > 100, (what, ratio)
    # weighted: the last row is switched off (its part is the +0 the gradient test looks for); the two other walks still show
    w = R.weights(m)
    assert w[-1] == 0 and abs((w == 0).mean() - 0.1) < 0.01 and w[at["fifth"]] > 0 and w[at["last_lo"]] > 0
    f, bound, _, _ = R.loss_reference(loss, z, b, w)
    for what in ("the last chunk", "the fifth trip of the first chunk"):
        if loss == "poisson" and what == "the last chunk":
            continue   # (its rows there are exp(-700) and the row that is off: the gradient elements hold that chunk)
        keep = np.ones(m, bool)
        keep[drops[what]] = False
        ratio = abs(float(f - R.loss_reference(loss, z[keep], b[keep], w[keep])[0])) / bound
        print(f"m={m} {loss} weighted: dropping {what} moves f by {ratio:.3g} bounds")
        assert ratio > 100, (what, ratio)
