"""CPU: the exact reference of tests/operator_exact.py against the fp64 oracle (oracle/operator_ref.py: SciPy's
correlate2d) at the bounds tests/test_gpu_operator_kernels.py holds the device kernels to.  What this proves without
a GPU: a correct fp64 implementation - whatever its summation order - stays inside the element-wise bound, with room
(the worst ratio is printed; measured 0.0005 ... 0.04 for these cases), and the bound is not slack enough to let a
wrong tap, mirrored taps or a shifted mirror row through."""
import numpy as np
import pytest

import operator_exact as E
from oracle import operator_ref as O

CASES = [  # (K, shape, kind of taps)
    (3, (8, 8), "general"),
    (15, (8, 8), "general"),          # halo = image - 1: every row and column mirrored
    (3, (1000, 2), "general"),        # two pixels wide: the mirror is all there is beside a pixel
    (3, (2, 164), "separable"),
    (9, (100, 200), "separable"),     # u v^T with u != v: asymmetric
    (9, (100, 200), "general"),
    (15, (130, 96), "general"),
    (1, (16, 16), "general"),
]


def _setup(k, shape, kind, seed=5):
    rng = np.random.default_rng(seed + 17 * k + shape[0])
    taps = E.make_taps(rng, k, kind)
    observed = rng.standard_normal(shape)
    x = rng.standard_normal(shape[0] * shape[1])
    return taps, observed, x


@pytest.mark.parametrize("k,shape,kind", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_fp64_oracle_is_inside_the_bounds(k, shape, kind):
    taps, observed, x = _setup(k, shape, kind)
    ref, ex = O.BlurHaarL1Ref(taps, observed), E.Exact(taps, observed)
    g, bound = ex.grad_and_bound(x, separable=False)      # (SciPy adds all K^2 products whatever the rank)
    ratio, at = E.worst(ref.jac_f(x), g, bound)
    f = ex.f(x)
    f_rel = float(abs(ref.f(x)[0] - f) / f)
    print(f"K={k} {shape} {kind}: worst |jac_f - exact| / bound = {ratio:.3g} at {E.locate(at, shape, 8)}; f rel {f_rel:.2g}")
    assert ratio < 1.0
    assert f_rel <= E.F_RTOL


def test_two_pass_fp64_is_inside_the_separable_bound():
    """The separable kernels correlate rows with v, then columns with u, from factors refactored out of the taps
    (zf_op_factor_rank1): the same in NumPy fp64 must be inside the separable bound."""
    for k, shape in ((5, (100, 200)), (15, (8, 8)), (3, (2, 164))):
        rng = np.random.default_rng(k)
        u, v = rng.standard_normal(k), rng.standard_normal(k)
        taps = np.outer(u, v)
        taps /= np.abs(taps).sum()
        pi, pj = np.unravel_index(np.argmax(np.abs(taps)), taps.shape)
        uu, vv = taps[:, pj].copy(), taps[pi, :] / taps[pi, pj]
        observed, x = rng.standard_normal(shape), rng.standard_normal(shape[0] * shape[1])

        def blur2(img):
            p = np.pad(img, k // 2, mode="symmetric")
            t = sum(vv[j] * p[:, j:j + shape[1]] for j in range(k))
            return sum(uu[i] * t[i:i + shape[0]] for i in range(k))

        got = 2 * O.dwt(blur2(blur2(O.idwt(x, shape)) - observed))
        g, bound = E.Exact(taps, observed).grad_and_bound(x, separable=True)
        ratio, at = E.worst(got, g, bound)
        print(f"K={k} {shape} two-pass: worst ratio {ratio:.3g}")
        assert ratio < 1.0


@pytest.mark.parametrize("mutation", ["transposed_taps", "mirrored_columns", "largest_tap_1e-11", "mirror_off_by_one", "convolution"])
def test_the_bound_bites(mutation):
    """A wrong fp64 operator is outside the bound - the structural mistakes by twelve orders of magnitude, one tap off
    by 1e-11 relative still by a factor of 20 (general 9 x 9 taps on 100 x 200)."""
    k, shape = 9, (100, 200)
    taps, observed, x = _setup(k, shape, "general")
    wrong, mode = taps, "symmetric"
    if mutation == "transposed_taps":
        wrong = taps.T
    elif mutation == "mirrored_columns":
        wrong = taps[:, ::-1]
    elif mutation == "convolution":
        wrong = taps[::-1, ::-1]
    elif mutation == "largest_tap_1e-11":
        wrong = taps.copy()
        wrong[np.unravel_index(np.argmax(np.abs(taps)), taps.shape)] *= 1 + 1e-11
    else:
        mode = "reflect"      # the mirror without the edge sample

    def blur(img):
        p = np.pad(img, k // 2, mode=mode)
        return sum(wrong[i, j] * p[i:i + shape[0], j:j + shape[1]] for i in range(k) for j in range(k))

    got = 2 * O.dwt(blur(blur(O.idwt(x, shape)) - observed))
    g, bound = E.Exact(taps, observed).grad_and_bound(x, separable=False)
    ratio, _ = E.worst(got, g, bound)
    print(f"{mutation}: worst ratio {ratio:.3g}")
    assert ratio > 1.0      # detected
