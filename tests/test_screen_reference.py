"""CPU: the extended-precision restatement of gap-safe screening (tests/screen_cases.py) proved on its own.  On SMALL cases
0, 1 and 3 of tests/sparse_cases.py, least squares and logistic, along the warm-started path lam = 0.5 / 0.2 / 0.05 lam_max
(18 runs): no column the exact rule discards - at the warm start, after 10, 100 and 1000 FISTA iterations - is in the support
of a 20 000-iteration solution; the guard E dominates the measured fp64 error of g_j; and the rule bites (the kept set
shrinks as the gap falls)."""
import numpy as np
import pytest

import logistic_cases as L
import screen_cases as SC
import sparse_cases as S

FRACTIONS = (0.5, 0.2, 0.05)
POINTS = (10, 100, 1000)
LONG = 20000


@pytest.mark.parametrize("logistic", [False, True], ids=["ls", "logistic"])
@pytest.mark.parametrize("case", [0, 1, 3])
def test_no_discarded_column_is_in_the_support_of_a_long_solution(case, logistic):
    if logistic:
        A, b, _ = L.make_logistic(*L.SMALL[case])
        scale = 1.0
    else:
        A, b, _ = S.make_sparse(*S.SMALL[case])
        scale = 0.5
    n = A.shape[1]
    lmax = SC.lam_max(A, b, scale, logistic)
    x = np.zeros(n)
    for frac in FRACTIONS:
        lam = frac * lmax
        x_long, at = SC.fista(A, b, lam, scale, logistic, x, LONG, record=POINTS)
        support = x_long != 0.0
        kept = []
        for name, xp in [("start", x)] + [(k, at[k]) for k in POINTS]:
            for dense in (False, True):
                s = SC.screen_longdouble(A, b, xp, lam, scale, logistic, dense=dense)
                assert s["E"] > 0 and np.isfinite(s["E"])
            assert not (s["discard"] & support).any(), (case, logistic, frac, name, np.flatnonzero(s["discard"] & support))
            # the guarded rule (the widest guard: dense storage) is the exact rule with a larger radius: it discards no more
            guarded = s["left"] + np.longdouble(s["E"]) * s["norms"] < np.longdouble(lam)
            assert not (guarded & ~s["discard"]).any()
            # E dominates what an fp64 evaluation of g loses: |g64_j - g_j| <= Eg |a_j| <= E |a_j| / 2
            err = np.abs(SC.grad_fp64(A, b, xp, scale, logistic).astype(np.longdouble) - s["grad"]).astype(float)
            s_sparse = SC.screen_longdouble(A, b, xp, lam, scale, logistic)
            bound = s_sparse["Eg"] * s["norms"].astype(float)
            assert (err <= bound).all(), (case, logistic, frac, name, float(np.max(err / np.maximum(bound, 1e-300))))
            assert 2.0 * s_sparse["Eg"] <= s_sparse["E"] <= s["E"]
            kept.append(int(n - guarded.sum()))
        print(f"case {case} {'logistic' if logistic else 'ls'} lam {frac} lam_max: kept {kept} of {n}; support {int(support.sum())}")
        assert kept[-1] >= support.sum() and kept[-1] <= kept[0]
        if frac == 0.5:
            assert kept[-1] < n // 2, "the rule must bite at the largest lam"
        x = x_long
