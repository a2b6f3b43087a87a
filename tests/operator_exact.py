"""An exact reference of the operator-form least squares f(x) = scale |B W^-1 x - b|^2 (csrc/zf_kernels_op.h) and the
element-wise rounding bounds the kernel tests hold the device results to.  TEST INFRASTRUCTURE: plain NumPy in
np.longdouble (64-bit mantissa on x86: eps 1.08e-19, a thousand times finer than the fp64 under test), independent
of SciPy and of oracle/operator_ref.py - tests/test_operator_exact.py pins the one against the other on the CPU.

    s(x)    = B W^-1 x           B: K x K correlation, image mirrored about its edges (edge sample included);
    f(x)    = scale sum (s - b)^2                                    W: one orthonormal Haar level, [cA, cH, cV, cD]
    grad(x) = 2 scale W B (s - b)                                    (the notebook applies B itself as the adjoint)

The bounds (u = 2^-53; every count below is doubled: SAFETY = 2, and nothing else is added).  With a = (|cA| + |cH| +
|cV| + |cD|) / 2 the bound of a pixel of W^-1 x and N the roundings of one correlation sum (K^2 for the general
kernels; 2 K + 1 for the separable ones, which also may use factors u v^T that differ from the taps by 1e-14 max|tap|:
zf_op_factor_rank1):

    E_s  = (N + 3) u |B| a                         (+ 1e-14 max|tap| box(a), separable)       error of s
    E_r  = E_s + u |r|                                                                         error of r = s - b
    E_B  = |B| E_r + N u |B| |r|                   (+ 1e-14 max|tap| box(|r|), separable)     error of B r
    E_g  = 2 scale (W_abs E_B + 4 u W_abs(|B| |r| + E_B))     (three additions of the Haar level, the factor 2 scale)

|B| is the correlation with |taps|, box the K x K sum, W_abs(z) the sum of a 2 x 2 block / 2 (the same for all four
quadrants).  The majorants are computed in fp64: their own rounding (1e-16 relative) is far inside the factor 2."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SAFETY = 2.0
RANK1_SLACK = 1e-14      # zf_op_factor_rank1: |k[i][j] - u[i] v[j]| <= 1e-14 max|k|
# f: zf_resid_x_kernel is ONE workgroup whose threads each add n / 1024 squares one after the other before the shuffle
# tree - not a tree sum, so the tree bound 2 sum |r| E_r + (log2 n + 8) u sum r^2 does not describe it; f keeps the
# project's existing relative tolerance (tests/test_gpu_operator_lasso.py).  The sharp check is the gradient's.
F_RTOL = 1e-12


def make_taps(rng, k, kind):
    """Random taps without any symmetry, sum |taps| = 1: "general" K x K normal, or "separable" u v^T with u != v."""
    t = rng.standard_normal((k, k)) if kind == "general" else np.outer(rng.standard_normal(k), rng.standard_normal(k))
    return t / np.abs(t).sum()


def make_self_adjoint_taps(rng, k, kind):
    """The same, made equal to their own mirror image in each axis (separable: palindromic u and v, still u != v).  With
    the mirrored boundary B is then a symmetric matrix, so that W B (B W^-1 x - b) - the notebook applies B itself as the
    adjoint - IS the gradient of f and a line search accepts a step of 1 / L.  (Taps equal to their rotation by 180 degrees
    are not enough: next to an edge a tap mirrored in x meets one that is not mirrored in y.)  Still not symmetric under
    a transposition."""
    if kind == "general":
        t = rng.standard_normal((k, k))
        t = t + t[::-1]
        t = t + t[:, ::-1]
    else:
        u, v = rng.standard_normal(k), rng.standard_normal(k)
        t = np.outer(u + u[::-1], v + v[::-1])
    return t / np.abs(t).sum()


def idwt(vec, shape, dtype=LD):
    h, w = shape[0] // 2, shape[1] // 2
    cA, cH, cV, cD = np.asarray(vec, dtype).reshape(4, h, w)
    img = np.empty((2 * h, 2 * w), dtype)
    img[0::2, 0::2] = (cA + cH + cV + cD) / 2
    img[0::2, 1::2] = (cA + cH - cV - cD) / 2
    img[1::2, 0::2] = (cA - cH + cV - cD) / 2
    img[1::2, 1::2] = (cA - cH - cV + cD) / 2
    return img


def dwt(img):
    a, b, c, d = img[0::2, 0::2], img[0::2, 1::2], img[1::2, 0::2], img[1::2, 1::2]
    return np.array([(a + b + c + d) / 2, (a + b - c - d) / 2, (a - b + c - d) / 2, (a - b - c + d) / 2]).reshape(-1)


def blur(img, taps):
    """out[y, x] = sum_ij taps[i, j] img[y + i - K // 2, x + j - K // 2], the image mirrored about its edges."""
    taps = np.asarray(taps, img.dtype)
    k = taps.shape[0]
    h, w = img.shape
    p = np.pad(img, k // 2, mode="symmetric")
    out = np.zeros((h, w), img.dtype)
    for i in range(k):
        for j in range(k):
            if taps[i, j] != 0:
                out += taps[i, j] * p[i:i + h, j:j + w]
    return out


def _wabs(z):
    q = (z[0::2, 0::2] + z[0::2, 1::2] + z[1::2, 0::2] + z[1::2, 1::2]) / 2
    return np.tile(q.reshape(-1), 4)


class Exact:
    """f, grad of one (taps, observed, scale) in np.longdouble, and the bounds on an fp64 evaluation of them."""

    def __init__(self, taps, observed, scale=1.0):
        if np.finfo(LD).nmant < 63:
            raise RuntimeError("np.longdouble is no finer than fp64 on this host: no reference to hold fp64 to")
        self.taps = np.asarray(taps, np.float64)
        if self.taps.shape[0] < 3:     # as launched: a 1 x 1 kernel is zero-padded to 3 x 3
            self.taps = np.pad(self.taps, (3 - self.taps.shape[0]) // 2)
        self.b = np.asarray(observed, np.float64)
        self.scale = float(scale)
        self.shape = self.b.shape
        self.k = self.taps.shape[0]

    def s(self, x):
        return blur(idwt(x, self.shape), self.taps)

    def f(self, x):
        r = self.s(x) - self.b.astype(LD)
        return LD(self.scale) * np.sum(r * r)

    def grad_and_bound(self, x, separable):
        """(grad in longdouble, E_g in fp64, both flat [cA, cH, cV, cD]) - see the module docstring."""
        r = self.s(x) - self.b.astype(LD)
        g = 2 * LD(self.scale) * dwt(blur(r, self.taps))
        k, at = self.k, np.abs(self.taps)
        n_round = (2 * k + 1) if separable else k * k
        slack = RANK1_SLACK * at.max() * np.ones((k, k))
        a = np.abs(np.asarray(x, np.float64)).reshape(4, self.shape[0] // 2, self.shape[1] // 2).sum(0) / 2
        a = np.kron(a, np.ones((2, 2)))          # the four pixels of a block share its bound
        ra = np.abs(r).astype(np.float64)
        b_ra = blur(ra, at)
        e_s = (n_round + 3) * U * blur(a, at) + (blur(a, slack) if separable else 0.0)
        e_b = blur(e_s + U * ra, at) + n_round * U * b_ra + (blur(ra, slack) if separable else 0.0)
        e_g = 2 * self.scale * (_wabs(e_b) + 4 * U * _wabs(b_ra + e_b))
        return g, SAFETY * e_g


def worst(got, ref, bound):
    """(largest |got - ref| / bound, its flat index); a zero bound admits a zero error only."""
    err = np.abs(np.asarray(got, LD).reshape(-1) - ref).astype(np.float64)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    at = int(np.argmax(ratio))
    return float(ratio[at]), at


def locate(at, shape, ty):
    """'quadrant, row, column, tile' of coefficient `at` - the 64 x ty image tile its 2 x 2 block lies in."""
    h2, w2 = shape[0] // 2, shape[1] // 2
    q, rem = divmod(at, h2 * w2)
    row, col = divmod(rem, w2)
    tiles_x = (shape[1] + 63) // 64
    return f"c{'AHVD'[q]}[{row}, {col}] (image tile {(2 * row) // ty * tiles_x + (2 * col) // 64}: row {(2 * row) // ty}, column {(2 * col) // 64})"
