"""CPU: the table of tests/restrict_cases.py reaches what it claims - the plans, the wave contents, the model of the fill kernel
and its mutants, the two small references - so that a green run of tests/test_gpu_screen_kernels.py means something."""
import numpy as np
import pytest
import scipy.sparse as sp

import restrict_cases as R
from zfista_amd import sparse

T = R.T
MUTANTS = ("no-first", "no-mask", "wide-prefix")


def test_every_case_has_the_plan_it_claims_and_every_lane_width_is_on_both_sides():
    seen_a, seen_t = set(), set()
    for name in R.LANE_CASES + R.SEGMENT_CASES + ("wide",):
        c = R.case(name)
        indptr, _, _, shape = sparse.canonical_csr(c.A)
        t_indptr = sparse.canonical_csr(c.A.T.tocsr())[0]
        a, t = sparse.plan_rows(indptr), sparse.plan_rows(t_indptr)
        got = R.plan_of((a, t))
        print(f"{name}: {shape[0]} x {shape[1]}, nnz {c.A.nnz}, plan {got}")
        assert got == c.plan, name
        if name in R.LANE_CASES:
            seen_a.add(a["lanes"])
            seen_t.add(t["lanes"])
    assert seen_a == seen_t == set(R.LANES)
    assert R.case("segments").plan == (64, 4, 4, 0, 10, 0) and R.case("segments-T").plan == (4, 64, 0, 4, 0, 10)
    assert R.case("wide").A.shape == (64, 2 ** 21 + 3) and R.case("wide").plan[:2] == (64, 4)
    assert int(np.diff(R.case("wide").A.indptr).max()) > 2 * T


@pytest.mark.parametrize("L", R.LANES)
def test_lane_matrices_hold_the_lengths_and_the_waves_they_claim(L):
    c = R.case(f"lanes-{L}")
    lens = np.diff(c.A.indptr)
    assert np.array_equal(lens, c.lens) and lens.size == R.ROWS == 203
    named = [0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 1, 4 * L, 4 * L + 1, 7 * L + 3]
    assert all((lens == v).any() for v in named) and (lens == 0).sum() >= 2 and (lens == 1).sum() >= 2
    rest = np.sort(lens)[::-1][6:]   # (everything but 7L + 3, 4L + 1, 4L, 3L + 1, 2L + 1, 2L)
    assert rest.max() < 3 * L
    assert c.A.shape[1] == 7 * L + 6 and (np.diff(c.A.tocsc().indptr)[-3:] == 0).all() and (np.diff(c.A.tocsc().indptr)[:-3] > 0).all()
    # position inside the row = column number
    for i in (0, 64, 65, 202):
        assert np.array_equal(c.A.indices[c.A.indptr[i]:c.A.indptr[i + 1]], np.arange(lens[i]))
    per_wave = 64 // L
    if L < 64:
        good = False
        for w in range(0, lens.size, per_wave):
            wave = lens[w:w + per_wave]
            rounds = (wave + L - 1) // L
            good |= bool(np.unique(rounds).size > 1 and (wave == 0).any() and (wave == L).any())
        assert good, "no wave holds an empty row, a full group and rows of different rounds"
    if L <= 16:
        assert 64 % per_wave == 0 and list(lens[65:68]) == [L, L - 1, L + 1], "L - 1, L, L + 1 side by side in one wave"
    assert lens.size % (256 // L) != 0, "the last workgroup is partial"


@pytest.mark.parametrize("name", R.LANE_CASES[:5])
def test_the_fill_model_is_the_restriction_and_every_mutant_shows(name):
    c = R.case(name)
    L = c.L
    shows = {m: [] for m in MUTANTS}
    for pattern in c.pattern_names:
        mask, cols, want = R.restricted_case(name, pattern)
        if want is None:
            assert not mask.any()
            continue
        assert R.model_agrees(R.fill_model(c.A, mask, L), want), pattern
        for m in MUTANTS:
            if not R.model_agrees(R.fill_model(c.A, mask, L, m), want):
                shows[m].append(pattern)
    print(name, shows)
    for m in MUTANTS:
        if L < 64 or m == "wide-prefix":
            assert set(R.MUTANT_PATTERNS) <= set(shows[m]), (m, shows[m])
        else:
            assert shows[m] == [], "at L = 64 the group is the wave: no shift, no mask"


def test_the_fill_model_on_the_transposes():
    """Rows that are no prefixes (the A side of a transpose has 32 lanes)."""
    for name in R.LANE_CASES[5:]:
        c = R.case(name)
        for pattern in ("all", "last-lane", "bernoulli-0.5", "empty-columns"):
            mask, cols, want = R.restricted_case(name, pattern)
            assert R.model_agrees(R.fill_model(c.A, mask, 32), want), (name, pattern)


def test_patterns_are_what_they_say():
    c = R.case("lanes-8")
    n = c.A.shape[1]
    j = np.arange(n)
    assert np.array_equal(R.keep_mask(c, "last-lane"), j % 8 == 7) and np.array_equal(R.keep_mask(c, "first-round"), j < 8)
    assert np.array_equal(np.flatnonzero(R.keep_mask(c, "single")), [8])
    assert np.array_equal(np.flatnonzero(R.keep_mask(c, "empty-columns")), [n - 3, n - 2, n - 1])
    assert np.array_equal(R.keep_mask(c, "bernoulli-0.5"), R.keep_mask(c, "bernoulli-0.5"))
    for name in R.LANE_CASES + R.SEGMENT_CASES:
        mask, cols, want = R.restricted_case(name, "empty-columns")
        assert cols.size >= 1 and want["nnz"] == 0 and want["n"] == cols.size
        base = R.case(name[:-2]) if name.endswith("-T") else None   # a transpose: the columns of the empty rows
        c = R.case(name)
        assert cols.size == (c.A.shape[1] - int(c.lens.max()) if base is None else int((base.lens == 0).sum()))
        assert cols.size == (3 if name in R.LANE_CASES[:5] else 7 if name == "segments" else cols.size)
    s = R.case("segments")
    assert s.pattern_names[-2:] == ("segment-borders", "not-first-segment")
    assert np.array_equal(np.flatnonzero(R.keep_mask(s, "segment-borders")), [T - 1, T, 2 * T - 1, 2 * T])
    assert np.array_equal(R.keep_mask(s, "not-first-segment"), np.arange(2 * T + 70) >= T)
    # the split rows the restricted segment matrix must have, from the row lengths alone
    for pattern, split in (("all", 4), ("not-first-segment", 2), ("alternating", 2), ("segment-borders", 0), ("empty-columns", 0)):
        mask, cols, want = R.restricted_case("segments", pattern)
        kept = np.array([mask[:k].sum() for k in s.lens])
        assert (kept > T).sum() == split == want["plan"]["split_row"].size, pattern
    mask, cols, want = R.restricted_case("segments", "not-first-segment")
    assert sorted(np.diff(want["indptr"])[[1, 2, 3, 8]]) == [1, T, T + 1, T + 63]


def test_scan_ref_and_stats_ld_against_loops():
    rng = np.random.default_rng(0)
    for keep in (np.array([0], dtype=np.uint8), np.array([1], dtype=np.uint8), np.array([0, 2, 255, 0, 1, 1, 0], dtype=np.uint8),
                 rng.integers(0, 2, 37).astype(bool)):
        index, count = R.scan_ref(keep)
        run, want = 0, []
        for v in keep:
            want.append(run)
            run += 1 if v else 0
        assert index.dtype == np.int32 and list(index) == want and count == run
    for norms in (np.array([0.0]), np.array([3.0, 4.0]), np.abs(rng.standard_normal(29))):
        total, bound = R.stats_ld(norms)
        loop = np.longdouble(0)
        for v in norms:
            loop += np.longdouble(v) * np.longdouble(v)
        assert abs(total - loop) <= 64 * np.finfo(np.longdouble).eps * loop
        assert bound == 2.0 * norms.size * 2.0 ** -53 * float(total)
        lens = np.arange(norms.size)
        wider = R.stats_ld(norms, lens)[1]
        extra = sum(4.0 * (k / 2 + 2) * 2.0 ** -53 * float(v) ** 2 for k, v in zip(lens, norms))
        assert abs(wider - (bound + extra)) <= 1e-12 * wider + 0.0 and wider >= bound
    assert R.stats_ld(np.array([3.0, 4.0]))[0] == 25
    # a sum of squares in fp64, in two orders, is inside the bound; one that misses its last element is not
    a = np.abs(rng.standard_normal(5000))
    total, bound = R.stats_ld(a)
    for s in (float(np.sum(a * a)), float(sum(a[::-1] * a[::-1]))):
        assert abs(np.longdouble(s) - total) <= bound
    assert abs(np.longdouble(float(np.sum(a[:-1] ** 2))) - total) > bound


def test_prefix_matrix():
    A = R.prefix_matrix([0, 3, 1], 5, 1)
    assert sp.issparse(A) and A.shape == (3, 5) and list(A.indptr) == [0, 0, 3, 4] and list(A.indices) == [0, 1, 2, 0]
    assert np.array_equal(A.data, R.prefix_matrix([0, 3, 1], 5, 1).data) and not np.array_equal(A.data, R.prefix_matrix([0, 3, 1], 5, 2).data)
