"""CPU: the table of tests/mo_cases.py reaches what it claims - the references are the oracle's, every branch of the staged prox
and of the clip is taken, the bounds hold for NumPy's own summation order and are tight enough to show every mutant - so that a
green run of tests/test_gpu_mo_kernels.py means something.

Mutants and the sizes at which they can act (asserted below at every such size of the table, G = 4 CUs for the persistent search):
  drop-last                the last element of a grid-stride loop is not taken: every n
  drop-second-trip-first   the first element of the second trip of the stride loop is not taken: n >= 262145
  skip-streamed-row        the streamed loop of k_dual_solve starts one row late: every size with a streamed row
  count-padded             the j >= n guard of the resident loop is dropped (a zero of the LDS padding is taken as an element):
                           every size with resident_rows * grid * 512 > n; modelled for scalar or no bounds only
  no-shift-back            + shift_i is not added back after stage i >= 1: every l1 case (every shift but one is non-zero);
                           n = 1: under at least one of the three weights
  no-tail                  tail_sum is ignored in stage 0: every l1 case with a tail (m = 2 with w_1 = 0 has none); n = 1 likewise
  J rows n_pad apart       row i of J read at i * n_pad: every n that is no multiple of 64, except n = 1 (J is one zero column)
  lo0                      lo_v[0] used for every j: every case with per-coordinate bounds and n >= 63
The first four change how often an element is counted and must move a sum out of its bound; the last four change elements and
must change at least one of x+ = prox(lr w, y - lr w @ J) (they move the sums out of their bounds too; asserted for the J rows)."""
import numpy as np
import pytest

import mo_cases as C

U = C.U
L1 = ("l1", "l1_boxv")


def _w(m):
    return C.weights(m)


def _outside(got, want, bound):
    return bool(np.any(np.abs(np.asarray(got) - np.asarray(want)) > np.asarray(bound)))


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
def test_sizes_and_capacity():
    assert [C.capmax(m) for m in C.MS] == [13, 9, 7, 6, 5, 4, 4]
    assert C.N_GRID == [1, 63, 64, 65, 255, 256, 257, 1000, 262143, 262144, 262145, 524289]
    assert C.grid_of(262144) == 1024 and C.grid_of(262145) == 1024 and C.grid_of(262143) == 1024 and C.grid_of(257) == 2
    for G in (4, 256, 304):
        for m in C.MS:
            sizes = C.n_solve(G, m)
            assert sizes == [1, 511, 512, 513, G * 512 - 1, G * 512, G * 512 + 1, 2 * G * 512 + 1]
            assert [C.rows_per_workgroup(n, G) for n in sizes] == [1, 1, 1, 1, 1, 1, 2, 3]
            for n in C.n_streamed(G, m):
                assert C.rows_per_workgroup(n, G) == C.capmax(m) + 1 > C.capmax(m)
    assert max(C.n_streamed(256, 2)) < 1.8e6 and max(C.n_streamed(256, 8)) < 6e5


def test_partition_models_take_every_element_once():
    for n in (1, 255, 256, 257, 1000, 262143, 262144, 262145, 524289):
        assert (C.grid_stride_visits(n) == 1).all()
    for G in (3, 4):
        for m in (2, 8):
            for n in C.n_solve(G, m) + C.n_streamed(G, m):
                for cap in (C.capmax(m), C.capmax(m) - 1, 1, 0):
                    v, padded = C.solve_visits(n, G, C.resident_rows(n, G, cap))
                    assert (v == 1).all() and padded == 0, (G, m, n, cap)
    assert C.grid_stride_visits(262145, "drop-second-trip-first")[262144] == 0
    assert C.grid_stride_visits(262145, "drop-second-trip-first").sum() == 262144
    assert C.grid_stride_visits(262144, "drop-second-trip-first").sum() == 262144   # (no second trip: cannot act)


# ---- the references are the oracle's ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("m", C.MS)
def test_prox_and_g_equal_the_oracle_bit_for_bit(m, variant):
    for n in C.N_SMALL:
        c = C.case(m, variant, n)
        ref = c.g.oracle(n)
        for name, w in _w(m).items():
            for x in (c.y, 2.0 * c.xk):
                coef, tail = C.coefs(c.g, c.lr, w)
                mine, theirs = C.prox(c.g, coef, tail, x), ref.prox_wsum_g(c.lr * w, x)
                assert np.array_equal(mine, theirs), (n, name)
                # bit for bit but for the sign of a zero: the oracle's sign(u) turns u = -0 into +0 (see mo_cases)
                differ = C.bits(mine) != C.bits(theirs)
                assert not differ[mine != 0.0].any() and differ.sum() <= 6, (n, name, int(differ.sum()))
        # g: the terms bit for bit, the value within the bound of any order of adding them
        p = C.prox(c.g, *C.coefs(c.g, c.lr, _w(m)["interior"]), c.y)
        terms, viol = C.g_terms(c.g, p)
        assert viol == 0 and C.same_bits(terms, np.abs(p - c.g.s().reshape(-1, 1)))
        val, bound = C.g_ref(c.g, p)
        assert not _outside(ref.g(p), val, bound), (n, ref.g(p), val, bound)
        if c.g.box and n >= 63:
            far = p.copy()
            far[n - 1] = 50.0
            assert np.isinf(C.g_ref(c.g, far)[0]).all() and np.isinf(ref.g(far)).all()


def _oracle_dual(c, w, f_y, F_old):
    from oracle import cpu_ref

    ref = c.g.oracle(c.n)
    return cpu_ref.dual_value_and_grad(w, ref.g, ref.prox_wsum_g, c.lr, c.y, c.J, f_y, F_old)


def _dual_agrees(c):
    f_y, F_old = C.solve_inputs(c)
    for name, w in _w(c.m).items():
        fun, fb, jac, jb = C.dual_ref(c, c.lr, w, f_y, F_old)
        val, grad = _oracle_dual(c, w, f_y, F_old)
        # the oracle forms w @ J, J @ (p - y) and the norms with BLAS (fused multiply-adds, blocked sums): its own result is one
        # of the orders the bound is for, plus one rounding per element of w @ J: (m + 2) u |terms|, inside N u sum |t| for N > m + 2
        slack = (c.m + 2) * U * (abs(fun) + np.abs(jac).max() + 1.0)
        assert abs(val - fun) <= fb + slack, (c.m, c.variant, c.n, name, val, fun, fb)
        assert np.all(np.abs(grad - jac) <= jb + slack), (c.m, c.variant, c.n, name)


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("m", C.MS)
def test_dual_value_and_gradient_equal_the_oracle_within_the_bound(m, variant):
    for n in C.N_SMALL:
        _dual_agrees(C.case(m, variant, n))


def test_dual_value_and_gradient_equal_the_oracle_at_a_large_size():
    _dual_agrees(C.case(5, "l1_boxv", 262145))


def test_the_interior_weight_is_the_minimiser_of_the_search_cases():
    for m in C.MS:
        for variant in L1:
            c = C.case(m, variant, 513)
            f_y, F_old = C.solve_inputs(c)
            _, _, jac, jb = C.dual_ref(c, c.lr, _w(m)["interior"], f_y, F_old)
            assert np.all(np.abs(jac - 1.0) <= jb + 8 * U * 513), (m, variant, jac)
            c1 = C.case(m, variant, 1)
            f_y, F_old = C.solve_inputs(c1)
            for w in _w(m).values():   # objective 0 dominates everywhere: the minimiser is e_0
                _, _, jac, _ = C.dual_ref(c1, c1.lr, w, f_y, F_old)
                assert jac[0] < jac[1:].min() - 50.0


# ---- every branch is taken -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("m", C.MS)
def test_every_branch_is_taken_three_times(m, variant):
    w = _w(m)["interior"]
    for n in [n for n in C.N_SMALL if n >= 64] + ([262145] if m in C.M_LARGE and variant == "l1_boxv" else []):
        c = C.case(m, variant, n)
        coef, tail = C.coefs(c.g, c.lr, w)
        counts = C.branch_counts(c.g, coef, tail, c.y)
        want = 2 + (3 * m if c.g.l1 else 0) + (5 if c.g.box else 0)
        assert len(counts) == want and min(counts.values()) >= 3, (n, {k: v for k, v in counts.items() if v < 3})
        # the designated elements take the same branch on the way through the dual: v = y there, bit for bit
        _, v, _, _ = C.trial_point(c, c.lr, w)
        assert C.same_bits(v[c.pos], c.y[c.pos]) and not c.J[:, c.pos].any()
        assert {0, n - 1} <= set(c.pos.tolist()) and (n <= 262144 or {262143, 262144} <= set(c.pos.tolist()))
    # the short cases: placed by hand
    c = C.case(m, variant, 1)
    counts = C.branch_counts(c.g, *C.coefs(c.g, c.lr, w), c.y)
    if c.g.l1:
        assert counts[("stage", 0, "on")] == 1
    elif c.g.box:
        assert counts[("clip", "on_lo")] == 1
    else:
        assert counts[("zero", "+0")] + counts[("zero", "-0")] == 1
    counts = C.branch_counts(c.g, *C.coefs(c.g, c.lr, w), C.case(m, variant, 63).y)
    assert sum(v > 0 for v in counts.values()) >= len(counts) // 2, counts   # (31 of the designated elements at most)


# ---- the bounds are not too tight --------------------------------------------------------------------------------------------------
def _pairwise_inside(c):
    m = c.m
    for name, w in _w(m).items():
        t = C.dual_terms(c, c.lr, w)
        S, B = C.dual_sums(c, c.lr, w, terms=t)
        got = t.sum(axis=1)
        got[:m] = c.g.ratios * got[:m] if c.g.l1 else 0.0
        assert not _outside(got, S, B), (m, c.variant, c.n, name)
        PS, PB = C.post_sums(c, c.lr, w, c.xk)
        wJ = C.w_dot_J(w, c.J)
        dy, dv = c.xk - c.y, c.xk - (c.y - c.lr * wJ)
        assert not _outside(np.append((c.J * dy).sum(axis=1), (dv * dv).sum()), PS, PB)
    if m <= 5:
        H, HB = C.hessian_ref(c, c.lr, _w(m)["uniform"])
        if not c.g.l1 and not c.g.box:   # the prox is the identity: H = lr J J^T
            assert not _outside(c.lr * (c.J @ c.J.T), H, HB + (m + 2) * U * np.abs(H))


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("m", C.MS)
def test_numpys_own_order_stays_inside_every_bound(m, variant):
    for n in C.N_SMALL:
        _pairwise_inside(C.case(m, variant, n))


def test_numpys_own_order_stays_inside_every_bound_at_a_large_size():
    _pairwise_inside(C.case(5, "l1_boxv", 262145))


@pytest.mark.parametrize("variant", ["l1", "l1_boxv", "box"])
def test_the_hessian_reference_is_the_derivative_of_the_gradient(variant):
    """Central differences of the composed gradient at a weight that puts no element on a kink (the uniform one)."""
    m, n = 3, 1000
    c = C.case(m, variant, n)
    w = _w(m)["uniform"]
    H, _ = C.hessian_ref(c, c.lr, w)
    f_y, F_old = C.solve_inputs(c)
    h = 1e-7
    fd = np.zeros((m, m))
    for k in range(m):
        e = np.zeros(m)
        e[k] = h
        fd[:, k] = (C.dual_ref(c, c.lr, w + e, f_y, F_old)[2] - C.dual_ref(c, c.lr, w - e, f_y, F_old)[2]) / (2 * h)
    # a kink crossed inside +-h moves a column by O(|J| |a|) ~ a few units of n * 1e-3
    assert np.abs(fd - H).max() <= 2e-3 * np.abs(H).max(), (fd, H)


# ---- the bounds and the inputs are not too loose: every mutant shows ---------------------------------------------------
def _all_sums(c, visits=None, padded=0, stride=None):
    """Every sum the device test checks, at the interior weight: dual_eval, post_terms at xk, the raw sums of g at xk."""
    w = _w(c.m)["interior"]
    terms = C.dual_terms(c, c.lr, w, stride=stride)
    S, B = C.dual_sums(c, c.lr, w, terms=terms, visits=visits, padded=padded)
    wJ = C.w_dot_J(w, C.jac_rows(c.J, stride))
    dy, dv = c.xk - c.y, c.xk - (c.y - c.lr * wJ)
    rows = np.concatenate([C.jac_rows(c.J, stride) * dy[None, :], (dv * dv)[None, :], C.g_terms(c.g, c.xk)[0]])
    if visits is not None:
        rows = rows * visits[None, :]
    more = [C.sum_ref(r) for r in rows]
    return np.concatenate([S, [o[0] for o in more]]), np.concatenate([B, [o[1] for o in more]])


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("m", C.M_LARGE)
def test_grid_stride_mutants_leave_a_sum_outside_its_bound(m, variant):
    for n in C.N_SMALL + ([262144, 262145, 524289] if variant == "l1_boxv" else []):
        c = C.case(m, variant, n)
        S, B = _all_sums(c)
        mutants = ["drop-last"] + (["drop-second-trip-first"] if n >= 262145 else [])
        for mutant in mutants:
            v = C.grid_stride_visits(n, mutant)
            assert v.sum() == n - 1
            S2, _ = _all_sums(c, visits=v)
            assert _outside(S2, S, B), (m, variant, n, mutant)
        if n == 262144:
            assert (C.grid_stride_visits(n, "drop-second-trip-first") == 1).all()


@pytest.mark.parametrize("m", C.MS)
def test_persistent_partition_mutants_leave_a_sum_outside_its_bound(m):
    G = 4
    for n in C.n_solve(G, m) + C.n_streamed(G, m):
        c = C.case(m, "l1", n)
        S, B = _all_sums(c)
        for cap in (C.capmax(m), 2):
            ER = C.resident_rows(n, G, cap)
            streams = C.rows_per_workgroup(n, G) > ER
            if n in C.n_streamed(G, m):
                assert streams
            if streams:
                v, _ = C.solve_visits(n, G, ER, "skip-streamed-row")
                assert v.sum() < n
                assert _outside(_all_sums(c, visits=v)[0], S, B), (m, n, cap)
            if ER * C.solve_grid(n, G) * 512 > n:
                v, padded = C.solve_visits(n, G, ER, "count-padded")
                assert padded == ER * C.solve_grid(n, G) * 512 - n and (v == 1).all()
                assert _outside(_all_sums(c, visits=v, padded=padded)[0][:2 * m + 2], S[:2 * m + 2], B[:2 * m + 2]), (m, n, cap)


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("m", C.MS)
def test_element_mutants_change_an_element(m, variant):
    for n in C.N_SMALL:
        c = C.case(m, variant, n)
        shown = {}
        for name, w in _w(m).items():
            _, _, p, _ = C.trial_point(c, c.lr, w)
            if c.g.l1:
                for mutant in ("no-shift-back", "no-tail"):
                    if mutant == "no-tail" and C.coefs(c.g, c.lr, w)[1] == 0.0:
                        continue   # (m = 2 with w_1 = 0: the tail is 0)
                    shown[mutant, name] = not C.same_bits(C.trial_point(c, c.lr, w, mutant)[2], p)
            if c.g.arrays and n >= 63:
                shown["lo0", name] = not C.same_bits(C.trial_point(c, c.lr, w, "lo0")[2], p)
            if n % 64 and n > 1 and name != "zero":   # (m = 2 with w_1 = 0 reads row 0 only, which stays where it is)
                shown["n_pad", name] = not C.same_bits(C.trial_point(c, c.lr, w, stride=(n + 63) & ~63)[2], p)
        if n == 1:   # one element on the threshold of stage 0 under the interior weight: any ONE weight must show the mutant
            assert all(any(v for (mu, _), v in shown.items() if mu == mutant) for mutant in {k[0] for k in shown}), (n, shown)
        else:
            assert all(shown.values()), (n, shown)
        if n % 64 and n > 1:
            S, B = _all_sums(c)
            assert _outside(_all_sums(c, stride=(n + 63) & ~63)[0], S, B), (m, variant, n)
