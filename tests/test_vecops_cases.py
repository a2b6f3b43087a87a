"""CPU: the table of tests/vecops_cases.py reaches what it claims - the sizes sit on the edges of the launch geometry restated
from csrc/zf_common.h, the element-wise references are the oracle's, the model of the summation order and NumPy's own orders
stay inside the a-priori bounds, and the bounds are tight enough to show every mutant - so that a green run of
tests/test_gpu_vecops.py means something.

Mutants of the summation model and the sizes at which they can act (asserted below at every such size of the table):
  drop-last                the last element of the stride loop is not taken: every n
  drop-second-trip-first   element 256 g, the first of the second trip, is not taken: n >= 524289
  twice                    element n // 2 is taken twice: every n
  drop-block-256           k_reduce_partials does not read the partials of block 256, the first of its second trip: n >= 65537
  row-stride               row k of the partials is read k (g + 1) doubles in instead of k g: the kernels with more than one
                           quantity (k_model_terms, k_eval_diag), every n
Each must move a sum out of its bound or change the bits of max |x - y| (the maximum moves only where the element or block
that the mutant loses held it)."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import vecops_cases as V
from conftest import ROOT


def _outside(got, want, bound):
    return np.abs(np.asarray(got, dtype=float) - np.asarray(want, dtype=float)) > np.asarray(bound, dtype=float)


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_librarys():
    src = open(os.path.join(ROOT, "zfista_amd", "csrc", "zf_common.h")).read()
    assert int(re.search(r"constexpr int ZF_BLOCK = (\d+);", src).group(1)) == V.ZF_BLOCK
    assert int(re.search(r"constexpr int ZF_MAX_GRID = (\d+);", src).group(1)) == V.ZF_MAX_GRID
    assert "ZF_WAVES = ZF_BLOCK / 64" in src and V.ZF_WAVES * V.WAVE == V.ZF_BLOCK
    vec = open(os.path.join(ROOT, "zfista_amd", "csrc", "zf_vecops.hip")).read()
    assert "int64_t cap = (n + 1023) & ~int64_t(1023);" in vec and V.WS_UNIT == 1024
    assert "for (int b = threadIdx.x; b < nblocks; b += 256)" in vec and V.REDUCE_THREADS == 256
    assert "__launch_bounds__(256) void k_reduce_partials" in vec


def test_every_size_sits_on_its_edge():
    assert V.N_ALL == [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537, 524287, 524288, 524289, 1048833]
    assert all(reason for _, reason in V.SIZES) and max(V.N_ALL) == 2 * V.CAP + 257
    assert (63 < V.WAVE, 64 == V.WAVE, 65 == V.WAVE + 1) == (True, True, True)
    assert [V.grid_of(n) for n in (255, 256, 257)] == [1, 1, 2] and 256 == V.ZF_BLOCK
    assert [V.workspace_capacity(n) for n in (1023, 1024, 1025)] == [1024, 1024, 2048]
    # k_reduce_partials: thread t takes b = t, t + 256, ...: a second trip of ITS loop from 257 blocks
    assert [V.grid_of(n) for n in (65535, 65536, 65537)] == [256, 256, 257] and V.REDUCE_THREADS == 256
    assert [(V.grid_of(n), V.trips(n)) for n in (524287, 524288, 524289)] == [(2048, 1), (2048, 1), (2048, 2)]
    n = V.N_ALL[-1]
    assert (V.grid_of(n), V.trips(n), n - 2 * V.CAP) == (2048, 3, V.ZF_BLOCK + 1)
    assert all(V.trips(n) == 1 for n in V.N_SMALL) and V.N_LARGE == [524287, 524288, 524289, n]
    assert [V.size_class(n) for n in (1, 65, 255, 257, 1023, 1025, 65535, 65537, 524287, 524289, n)] == \
        ["wave", "wave", "block", "block", "workspace-unit", "workspace-unit", "reduce-wrap", "reduce-wrap", "second-trip",
         "second-trip", "third-trip"]


def test_partition_model_takes_every_element_once():
    for n in V.N_ALL + [5000, 600001]:
        count = V.thread_values(n, lambda acc, sl: acc + 1.0)
        assert count.sum() == n and count.shape == (V.grid_of(n), 256)
        assert count.max() == V.trips(n) and count.min() >= V.trips(n) - 1
        index_sum = V.thread_values(n, lambda acc, sl: acc + np.arange(sl.start, sl.stop, dtype=np.float64))
        assert index_sum.sum() == n * (n - 1) / 2
        # thread (b, t) holds elements b 256 + t + k 256 g
        b, t = V.grid_of(n) - 1, 255
        own = np.arange(b * 256 + t, n, V.grid_of(n) * 256)
        assert index_sum[b, t] == own.sum() and count[b, t] == own.size


# ---- the element-wise references are the oracle's ---------------------------------------------------------------------------
def test_special_values_reach_every_window():
    for n in (65, 1025, 524289, V.N_ALL[-1]):
        for a, vals in [(x, V.specials()) for x in V.elementwise_inputs(n)] + [(V.prox_input(n, tau), V.specials(tau)) for tau in V.TAUS]:
            for name, lo, hi in V.windows(n):
                if hi - lo < vals.size:
                    continue
                for v in vals:
                    assert V.differing(a[lo:hi], np.full(hi - lo, v)).size < hi - lo, (n, name, v)
    assert [name for name, _, _ in V.windows(V.N_ALL[-1])] == ["first", "last", "end of trip 1", "start of trip 2", "start of trip 3"]
    assert V.windows(524289)[3][1:] == (524288, 524289) and V.windows(V.N_ALL[-1])[4][1] == 2 * V.CAP
    a, b, c = V.elementwise_inputs(1025)
    # the pairs that make a new kind of result meet somewhere: inf - inf (NaN) and inf + inf, inf and NaN beside a number, 0 - 0
    fin = np.isfinite(a) & np.isfinite(b)
    for what, hit in (("inf, same sign", np.isinf(a) & (a == b)), ("inf, opposite signs", np.isinf(a) & (a == -b)),
                      ("inf beside a number", np.isinf(a) & np.isfinite(b)), ("a number beside inf", np.isfinite(a) & np.isinf(b)),
                      ("NaN beside a number", np.isnan(a) & np.isfinite(b)), ("a number beside NaN", np.isfinite(a) & np.isnan(b)),
                      ("zeros", fin & (a == 0) & (b == 0)), ("1e300 with 1e300", fin & (np.abs(a) == 1e300) & (np.abs(b) == 1e300))):
        assert hit.any(), what


def test_prox_references_reproduce_the_oracle_and_the_existing_models():
    from oracle.problems_ref import clip_box, soft_threshold
    from test_gpu_soft_threshold_bits import expected

    for n in (1, 65, 1025, 65537):
        for tau in V.TAUS:
            u = V.prox_input(n, tau)
            assert V.same_bits(V.prox_l1_box(u, tau, -np.inf, np.inf), expected(u, np.float64(tau)))
            ok = ~np.isnan(u)
            for lo, hi in V.BOXES:
                with np.errstate(invalid="ignore", over="ignore"):
                    l1 = clip_box(soft_threshold(u[ok], tau), lo, hi)
                    mine = V.prox_l1_box(u, tau, lo, hi)
                    assert np.array_equal(mine[ok], l1) and np.isnan(mine[~ok]).all()
                    # bit for bit but for the sign of a zero: the oracle's sign(u) * 0 is +0 at u = +-0 (the kernel copies the sign)
                    nz = l1 != 0.0
                    assert V.same_bits(mine[ok][nz], l1[nz])
                    for shrink in (1.0, 1.0 / (1.0 + 0.625 * 0.37)):
                        want = clip_box(soft_threshold(u, tau) * shrink, lo, hi)   # tests/test_gpu_enet.py
                        assert V.same_bits(V.prox_enet_box(u, tau, shrink, lo, hi), want)
            assert n < 64 or ((np.abs(u) < tau).any() or tau == 0.0) and (np.abs(u) > tau).any()


def test_elementwise_references_are_numpys_expressions():
    for n in (1, 257, 524289):
        a, b, c = V.elementwise_inputs(n)
        with np.errstate(invalid="ignore", over="ignore"):
            assert V.same_bits(V.grad_step(a, b, V.LR), a - V.LR * b.flatten())        # cpu_ref.trial_single
            for beta in V.BETAS:
                assert V.same_bits(V.momentum(a, b, beta), a + beta * (a - b))      # cpu_ref.minimize_proximal_gradient
            assert V.same_bits(V.diag_grad(a, b, c), b * (a - c))                       # DiagQuadL1Ref.jac_f
        assert np.isnan(V.grad_step(a, b, V.LR)).any() or n == 1


def test_fma_is_one_rounding():
    rng = np.random.default_rng(3)
    n = 3000
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    c = rng.standard_normal(n) * rng.choice([1.0, 1e-8, 1e8, 2.0 ** -53, 1e-17], n)
    c[:200] = -(a[:200] * b[:200])   # cancellation: the result is the product's own rounding error
    got = V.fma(a, b, c)
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())])
    assert V.same_bits(got, want)
    assert (a * b + c != want).sum() > 100, "the sample must tell one rounding from two"


# ---- the summation model and NumPy's orders stay inside the bounds -----------------------------------------------------
def _all(c, visit=None, **mutant):
    """Every sum the device test checks: values of the model (with a mutant), references, bounds; the index of the maximum."""
    one = {k: v for k, v in mutant.items() if k != "row_stride"}   # (kernels with one quantity have no second row)
    got = np.concatenate([V.emulate_model_terms(c.jac, c.x, c.y, visit, **mutant), V.emulate_eval_diag(c.x, c.d, c.c, V.LAM, visit, **mutant),
                          [V.emulate_asum(c.x, visit, **one), V.emulate_enet_g(c.x, V.LAM, V.L2, visit, **one)]])
    refs = [V.model_terms_ref(c.jac, c.x, c.y), V.eval_diag_ref(c.x, c.d, c.c, V.LAM), V.asum_ref(c.x), V.enet_g_ref(c.x, V.LAM, V.L2)]
    want = np.concatenate([np.atleast_1d(r[0]) for r in refs])
    bound = np.concatenate([np.atleast_1d(r[1]) for r in refs])
    return got, want, bound


MAX = 2   # index of max |x - y| in _all


@pytest.mark.parametrize("n", V.N_ALL)
def test_model_and_numpy_orders_stay_inside_the_bounds(n):
    c = V.reduction_case(n)
    got, want, bound = _all(c)
    assert not _outside(got, want, bound).any(), (n, got, want, bound)
    assert V.same_bits(got[MAX], want[MAX]) and bound[MAX] == 0.0
    assert (np.delete(bound, MAX) > 0).all() and (np.delete(bound, MAX) <= 1e-3).all()   # (<= 1 / 125 of the smallest term)
    dx, r = c.x - c.y, c.x - c.c
    terms = [c.jac * dx, dx * dx, None, c.d * (r * r), np.abs(c.x), np.abs(c.x), V.LAM * np.abs(c.x) + 0.5 * V.L2 * c.x * c.x]
    scale = [1.0, 1.0, None, 0.5, V.LAM, 1.0, 1.0]
    least = [0.25, 0.25, None, 0.125, 0.5, 0.5, 0.5 * V.LAM]   # (magnitudes in [1/2, 2])
    for k, t in enumerate(terms):
        if t is None:
            continue
        assert np.abs(t).min() >= least[k] * (1 - 1e-12) and np.abs(t).max() <= 8.0, "every term is of the size of the others"
        for total in (np.sum(t), np.cumsum(t)[-1]):   # pairwise, left to right
            assert not _outside(scale[k] * total, want[k], bound[k]), (n, k)


def test_the_bound_at_the_largest_size_is_what_the_text_says():
    c = V.reduction_case(V.N_ALL[-1])
    _, _, bound = _all(c)
    assert 1e-4 < bound[0] < 5e-4 and 1e-4 < bound[1] < 5e-4


# ---- every mutant shows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", V.N_ALL)
def test_every_mutant_leaves_a_bound_or_changes_the_maximum(n):
    c = V.reduction_case(n)
    base, want, bound = _all(c)
    mutants = [("drop-last", dict(visit=V.visits(n, "drop-last"))), ("twice", dict(visit=V.visits(n, "twice")))]
    if V.trips(n) >= 2:
        mutants.append(("drop-second-trip-first", dict(visit=V.visits(n, "drop-second-trip-first"))))
    if V.grid_of(n) > V.REDUCE_THREADS:
        mutants.append(("drop-block-256", dict(drop_block=256)))
    mutants.append(("row-stride", dict(row_stride=V.grid_of(n) + 1)))
    assert len(mutants) == 3 + (n >= 524289) + (n >= 65537)
    for name, kw in mutants:
        got, _, _ = _all(c, **kw)
        out = _outside(got, want, bound)
        out[MAX] = not V.same_bits(got[MAX], base[MAX])
        if name == "row-stride":    # row 1 of k_model_terms and of k_eval_diag move; row 0 and the single sums cannot;
            # row 2, the maximum, is read two blocks late: it changes if block 0 or 1 held it (always for g <= 2)
            assert out[[1, 4]].all() and not out[[0, 3, 5, 6]].any(), (n, name, out)
            holder = (int(np.argmax(np.abs(c.x - c.y))) % (V.grid_of(n) * V.ZF_BLOCK)) // V.ZF_BLOCK
            assert out[MAX] == (holder < 2), (n, name, holder)
        else:                      # every sum moves (the maximum only if the element or block held it)
            assert np.delete(out, MAX).all(), (n, name, out, got, want, bound)


def test_a_mutant_that_cannot_act_changes_nothing():
    for n in (65536, 524288):
        c = V.reduction_case(n)
        base, _, _ = _all(c)
        if n == 524288:
            with pytest.raises(AssertionError):
                V.visits(n, "drop-second-trip-first")
        else:
            assert V.same_bits(_all(c, drop_block=256)[0], base)   # (256 blocks: there is no block 256)


def test_fmax_drops_a_nan_and_the_sums_keep_it():
    for n in (257, 524289):
        c = V.reduction_case(n)
        for j in (0, n - 1, min(n - 1, V.CAP)):
            x = c.x.copy()
            x[j] = np.nan
            got = V.emulate_model_terms(c.jac, x, c.y)
            rest = np.abs(np.delete(c.x - c.y, j)).max()
            assert np.isnan(got[0]) and np.isnan(got[1]) and V.same_bits(got[2], rest)
            x[j] = np.inf
            got = V.emulate_model_terms(c.jac, x, c.y)
            assert np.isinf(got[0]) and got[1] == np.inf and got[2] == np.inf
