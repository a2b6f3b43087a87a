"""Native operator objects: callback providers the engine recognises.

The reference's solver takes four opaque callables (``f, g, jac_f,
prox_wsum_g``; zfista/proximal_gradient.py:311-316) and its problem library
supplies them as bound methods (zfista/problems.py:140-150).  The objects here
keep that contract - ``prob.f(x)`` etc. are ordinary callables on NumPy arrays,
evaluated on the GPU - and additionally carry a descriptor.  When
``zfista_amd.minimize_proximal_gradient`` is handed the four bound methods of
ONE such object it runs the device-resident fused path instead of calling them.

Problem data lives in HBM (torch CUDA tensors are accepted as-is; NumPy arrays
are uploaded once).  There is no host implementation of any of these methods.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def _to_device(a, name):
    """float64 contiguous CUDA tensor from a NumPy array or a torch tensor."""
    import torch

    _lib.require_gpu()
    if isinstance(a, torch.Tensor):
        t = a
        if not t.is_cuda:
            t = t.cuda()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()
    if t.dtype != torch.float64:
        raise TypeError(f"{name} must be float64 (the reference path is float64 throughout)")
    return t.contiguous()


def _as_host(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64))


def _matrix_dtype(v):
    """``matrix_dtype`` as the string "float64" (None: the default) or "float32".  ValueError for anything else - on the host,
    before anything touches the device."""
    if v is None:
        return "float64"
    name = v if isinstance(v, str) else str(v).rsplit(".", 1)[-1] if type(v).__module__.split(".")[0] == "torch" else None
    if name is None:
        try:
            name = np.dtype(v).name
        except TypeError:
            name = None
    if name not in ("float64", "float32"):
        raise ValueError(f"matrix_dtype must be None, 'float64' or 'float32' (or the NumPy / torch dtype of that name), got {v!r}")
    return name


def _to_device_f32(a, name):
    """float32 contiguous CUDA tensor from a NumPy array or a torch tensor: a float32 CUDA tensor is taken as it is (no copy when it
    is contiguous), anything else is rounded to nearest.  A value that is not finite after the rounding raises ValueError - found on
    the host for a host matrix, by one ``isfinite().all()`` on the device for a device one."""
    import torch

    _lib.require_gpu()
    bad = ValueError(f"{name} holds a value that is not finite as float32 (NaN, an infinity, or a magnitude beyond 3.4e38)")
    if isinstance(a, torch.Tensor):
        if a.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{name} must be float32 or float64")
        t = (a if a.is_cuda else a.cuda()).to(torch.float32).contiguous()
        if not bool(torch.isfinite(t).all()):
            raise bad
        return t
    with np.errstate(over="ignore"):
        host = np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))
    if not np.all(np.isfinite(host)):
        raise bad
    return torch.from_numpy(host).cuda()


class NativeProblem:
    """Marker base: a single-objective problem with a device descriptor."""

    n_features: int

    def callbacks(self):
        return self.f, self.g, self.jac_f, self.prox_wsum_g

    def minimize_proximal_gradient(self, x0, **kwargs):
        """Bound-method form, as zfista/problems.py:140-150."""
        from .proximal_gradient import minimize_proximal_gradient

        return minimize_proximal_gradient(self.f, self.g, self.jac_f, self.prox_wsum_g, x0, **kwargs)

    # -- shared g / prox: lam * |x|_1 (+ box) ------------------------------------------
    def g(self, x):
        x = _as_host(x)
        if self._has_box() and ((x < self.box[0]).any() or (x > self.box[1]).any()):
            return np.float64(np.inf)   # zfista/problems.py:104-106
        return self._eval_fg(x)[1]

    def prox_wsum_g(self, weight, x):
        x = _as_host(x)
        out = np.empty_like(x)
        lib = _lib.require_gpu()
        _lib.check(lib.zf_host_prox_l1_box(C.c_void_p(_lib.ptr(out)), C.c_void_p(_lib.ptr(x)),
                                           float(self.lam * weight), self.box[0], self.box[1], x.size),
                   "zf_host_prox_l1_box")
        return out

    def _has_box(self):
        return not (self.box[0] == -np.inf and self.box[1] == np.inf)


class DiagQuadL1(NativeProblem):
    r"""f(x) = 1/2 \sum_i d_i (x_i - c_i)^2,  g(x) = lam \|x\|_1 (+ optional box).

    The single-objective analogue of the diagonal-gradient problems of
    zfista/problems.py:193-205 (BASELINE cfg2 / the headline metric).  With
    ``group`` set, ``d`` and ``c`` are this rank's contiguous shard of a
    decision vector partitioned across the ranks of that process group.
    """

    kind = _lib.ZF_PROBLEM_DIAG_QUAD_L1
    separable = True   # f is a sum over elements: chains of trials per pass, and acceptance="resolved"

    def __init__(self, d, c, lam, bounds=None, group=None):
        self.d = _to_device(d, "d")
        self.c = _to_device(c, "c")
        if self.d.ndim != 1 or self.d.shape != self.c.shape:
            raise ValueError("d and c must be 1-D of equal length")
        self.lam = float(lam)
        self.box = (-np.inf, np.inf) if bounds is None else (float(bounds[0]), float(bounds[1]))
        self.n_features = int(self.d.numel())
        self.group = group

    def _eval_fg(self, x):
        import torch

        if x.size != self.n_features:
            raise ValueError(f"len(x) should be equal to n_features, got {x}.")
        lib = _lib.require_gpu()
        xd = torch.from_numpy(x).cuda()
        out = np.zeros(2)
        _lib.check(lib.zf_eval_diag_l1(C.c_void_p(xd.data_ptr()), C.c_void_p(self.d.data_ptr()),
                                       C.c_void_p(self.c.data_ptr()), self.lam, x.size,
                                       C.c_void_p(_lib.ptr(out)),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "zf_eval_diag_l1")
        return np.float64(out[0]), np.float64(out[1])

    def f(self, x):
        return self._eval_fg(_as_host(x))[0]

    def jac_f(self, x):
        x = _as_host(x)
        if x.size != self.n_features:
            raise ValueError(f"len(x) should be equal to n_features, got {x}.")
        out = np.empty_like(x)
        lib = _lib.require_gpu()
        _lib.check(lib.zf_host_diag_grad(C.c_void_p(_lib.ptr(out)), C.c_void_p(_lib.ptr(x)),
                                         C.c_void_p(self.d.data_ptr()), C.c_void_p(self.c.data_ptr()),
                                         x.size), "zf_host_diag_grad")
        return out

    def _descriptor(self):
        from .comm import rank_world

        rank, world = rank_world(self.group)
        fields = dict(kind=self.kind, world=world, rank=rank, n=self.n_features, m_rows=0,
                      d=self.d.data_ptr(), c=self.c.data_ptr(), A=None, b=None,
                      scale=0.5, lam=self.lam, box_lo=self.box[0], box_hi=self.box[1])
        return fields, (self.d, self.c)


class DualityGap:
    """What ``problem.duality_gap(x)`` / ``NativeRun.duality_gap()`` return: ``primal`` = P(x) = f(x) + lam |x|_1, ``dual`` =
    D(nu) at the dual point nu = alpha grad phi(A x), ``gap`` >= 0 - the sum of the two Fenchel-Young gaps, formed term by
    term (csrc/zf_kernels_gap.h), not ``primal - dual`` - ``alpha`` = min(1, lam / |grad f(x)|_inf) and ``grad_inf`` =
    |grad f(x)|_inf; also ``f``, ``g_l1`` = lam |x|_1 and ``rows_gap`` (the loss part of the gap; ``gap - rows_gap`` is the
    l1 part).  ``P(x) - min P <= gap``.

    Elastic net (``l2 > 0``): P also holds ``g_l2`` = (l2 / 2) |x|^2, the ridge term enters the dual as n more least-squares
    rows, ``grad_inf`` = |grad f(x) + l2 x|_inf, and ``ridge_gap`` = (l2 / 2) (1 - alpha)^2 |x|^2 is their part of the gap
    (``gap - rows_gap - ridge_gap`` is the l1 part).  Both are 0 for an l1 problem."""

    __slots__ = ("primal", "dual", "gap", "alpha", "grad_inf", "f", "g_l1", "rows_gap", "g_l2", "ridge_gap")

    def __init__(self, out):
        self.g_l2 = self.ridge_gap = np.float64(0.0)
        for k, v in zip(self.__slots__, out):
            setattr(self, k, np.float64(v))

    def __repr__(self):
        return "DualityGap(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"


class Screen(tuple):
    """What ``problem.screen(x)`` returns: the triple ``(gap, keep, count)`` - the ``DualityGap`` at x, the device mask of the
    columns the gap-safe rule cannot discard (a bool CUDA tensor of n_features) and their number - with, as attributes
    beside those three, ``index`` (int32 CUDA tensor: the exclusive scan of the mask, the new number of a kept column),
    ``radius`` = sqrt(2 L gap) and ``guard`` = E, the widening of the radius that covers the fp64 evaluation
    (csrc/zf_kernels_screen.h)."""

    def __new__(cls, gap, keep, count, index, radius, guard):
        self = tuple.__new__(cls, (gap, keep, count))
        self.gap, self.keep, self.count = gap, keep, count
        self.index, self.radius, self.guard = index, np.float64(radius), np.float64(guard)
        return self


class _ColumnNorms:
    """|a_j|_2 of one device matrix (a float64 CUDA tensor), [sum |a_j|^2, max |a_j|] beside it: computed by the first
    ``column_norms()`` and shared by every ``with_lam`` sibling of the problem."""

    __slots__ = ("norms", "stats")

    def __init__(self):
        self.norms = self.stats = None


def _dp(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)


def _check_l2(l2, group=None):
    """The ridge weight of an elastic-net penalty as a float: finite and >= 0, and 0 for a sharded problem."""
    l2 = float(l2)
    if not (np.isfinite(l2) and l2 >= 0):
        raise ValueError(f"l2 must be finite and >= 0 (the weight of (l2 / 2) |x|^2 in g), got {l2!r}")
    if l2 > 0 and group is not None:
        raise ValueError("l2 > 0 is not available with group=: the elastic-net step and its certificate are built for one GPU")
    return l2


def _check_weights(w, m, group=None):
    """Per-row sample weights as a host float64 vector: m of them, finite and >= 0, at least one > 0.  ValueError otherwise -
    on the host, before anything touches the device (a torch tensor is copied to the host for the check)."""
    if group is not None:
        raise ValueError("sample_weight is not available with group=: the weighted loss kernels, their certificate and "
                         "zf_solver_set_row_weights are built for one GPU (world = 1)")
    host = w.detach().cpu().numpy() if hasattr(w, "detach") else np.asarray(w)
    if np.dtype(host.dtype).kind not in "biuf":
        raise ValueError(f"sample_weight must be real numbers, got dtype {host.dtype}")
    host = np.array(host, dtype=np.float64, order="C", copy=True)   # (the problem's own copy: never the caller's array)
    if host.ndim != 1 or host.shape[0] != m:
        raise ValueError(f"sample_weight must be a vector of {m} weights (one per row of A), got shape {host.shape}")
    if not np.all(np.isfinite(host)) or np.any(host < 0):
        raise ValueError("sample_weight must be finite and >= 0")
    if not np.any(host > 0):
        raise ValueError("sample_weight must hold at least one weight > 0 (no row is left)")
    return host


def _check_penalty_factor(p, n, group=None, l2=0.0):
    """Per-column penalty factors as a host float64 vector: n of them, finite and >= 0.  ValueError otherwise - on the host,
    before anything touches the device (a torch tensor is copied to the host for the check)."""
    if group is not None:
        raise ValueError("penalty_factor is not available with group=: the penalty-factor step, its certificate and "
                         "zf_solver_set_penalty_factors are built for one GPU (world = 1)")
    if l2 > 0:
        raise ValueError("penalty_factor is not available with l2 > 0: the ridge term would need the factors too (glmnet scales "
                         "both), and that step is not built")
    host = p.detach().cpu().numpy() if hasattr(p, "detach") else np.asarray(p)
    if np.dtype(host.dtype).kind not in "biuf":
        raise ValueError(f"penalty_factor must be real numbers, got dtype {host.dtype}")
    host = np.array(host, dtype=np.float64, order="C", copy=True)   # (the problem's own copy: never the caller's array)
    if host.ndim != 1 or host.shape[0] != n:
        raise ValueError(f"penalty_factor must be a vector of {n} factors (one per column of A), got shape {host.shape}")
    if not np.all(np.isfinite(host)) or np.any(host < 0):
        raise ValueError("penalty_factor must be finite and >= 0")
    return host


def add_intercept(A):
    """``(A1, p)``: ``A`` with a leading column of ones - dense, or any ``scipy.sparse`` form (returned as CSR) - and the penalty
    factors ``[0, 1, ..., 1]`` that leave that column unpenalised: ``cls(A1, b, lam, penalty_factor=p)`` is the model with an
    intercept, x[0].  A host helper: no kernel."""
    if hasattr(A, "tocsr") and not isinstance(A, np.ndarray):
        import scipy.sparse as sp

        A = sp.csr_matrix(A, dtype=np.float64)
        A1 = sp.hstack([sp.csr_matrix(np.ones((A.shape[0], 1))), A], format="csr")
    else:
        A = A.detach().cpu().numpy() if hasattr(A, "detach") else np.asarray(A, dtype=np.float64)
        if A.ndim != 2:
            raise ValueError("A must be (m, n)")
        A1 = np.ascontiguousarray(np.hstack([np.ones((A.shape[0], 1)), A]))
    p = np.ones(A1.shape[1])
    p[0] = 0.0
    return A1, p


class _GapMixin:
    """What the eight margins classes (LeastSquaresL1, SparseLeastSquaresL1, LogisticL1, SparseLogisticL1, HuberL1, SparseHuberL1,
    PoissonL1, SparsePoissonL1) share: f / jac_f at a host vector, the duality-gap certificate, lam_max, same-matrix siblings, gap-safe screening and column
    restriction.  The three C entries (zf_margins_eval / _gap / _screen) take one descriptor, built HERE (``_eval_desc``) from the loss (``_loss``), the weights
    (``_w``), the penalty factors (``_pf``) and ``l2``; the storage class below supplies its matrix fields (``_matrix_fields``)."""

    has_duality_gap = True
    l2 = 0.0   # elastic net: g(x) = lam |x|_1 + (l2 / 2) |x|^2 (+ box)
    # per-row sample weights: f(x) = scale sum_i w_i loss_i - a weighted SUM, not a mean; the weights are used as given
    # (csrc/zf_kernels_loss.h).  _w: the device vector, shared by every sibling; None: the unweighted problem, every call as before
    _w = None
    _w_host = None
    # per-column penalty factors: g(x) = lam sum_j p_j |x_j|, p_j >= 0 (0: an unpenalised column).  _pf: the device vector, shared
    # by every sibling; None: the plain problem, every call as before
    _pf = None
    _pf_host = None
    _loss = _lib.ZF_LOSS_SQUARE   # the loss of the class: everything below that depends on it reads this one attribute
    _longest = (0, 0)       # (sparse classes: the longest row and column, which the screen reads for a handle)
    _f32 = False            # (dense classes: A is stored in fp32)

    @staticmethod
    def _flat(x):
        return x

    def _eval_desc(self):
        """The ``zf_eval_desc`` every evaluation entry takes.  The loss, the weights, the penalty factors, l2, delta, scale, lam and K
        are read HERE, once; the storage class supplies the matrix fields alone (``_matrix_fields``).  No site chooses an entry."""
        return _lib.EvalDesc(b=self.b.data_ptr(), w=None if self._w is None else self._w.data_ptr(),
                             p=None if self._pf is None else self._pf.data_ptr(), scale=self.scale, lam=self.lam, l2=self.l2,
                             delta=float(self.delta) if self._loss == _lib.ZF_LOSS_HUBER else 0.0, loss=self._loss,
                             K=getattr(self, "n_responses", 1), **self._matrix_fields())

    def _ls(self, x, want_grad):
        """(f, jac_f or None) at a host vector."""
        x = _as_host(self._flat(x))
        if x.size != self.n_features:
            raise ValueError(f"len(x) should be equal to n_features, got {x}.")
        lib = _lib.require_gpu()
        fval = C.c_double(0.0)
        grad = np.empty_like(x) if want_grad else None
        d = self._eval_desc()
        _lib.check(lib.zf_margins_eval(C.byref(d), C.sizeof(d), C.c_void_p(_lib.ptr(x)), C.byref(fval),
                                       C.c_void_p(_lib.ptr(grad)) if want_grad else None), "zf_margins_eval")
        return np.float64(fval.value), grad

    def f(self, x):
        return self._ls(x, False)[0]

    def jac_f(self, x):
        return self._ls(x, True)[1]

    def _gap_call(self, lib, x, out):
        d = self._eval_desc()
        _lib.check(lib.zf_margins_gap(C.byref(d), C.sizeof(d), C.c_void_p(_lib.ptr(x)), C.c_void_p(_lib.ptr(out)), out.size), "zf_margins_gap")

    def _screen_call(self, lib, x, out, h, keep, index):
        d = self._eval_desc()
        _lib.check(lib.zf_margins_screen(C.byref(d), C.sizeof(d), C.c_void_p(_lib.ptr(x)), C.c_void_p(_lib.ptr(out)), out.size, _dp(h.norms),
                                         _dp(h.stats), *self._longest, _dp(keep), _dp(index)), "zf_margins_screen")

    def _finish_descriptor(self, fields, keep):
        """The descriptor of a storage class with what has no field of zf_problem_desc: the engine calls zf_solver_set_l2 /
        zf_solver_set_row_weights / zf_solver_set_huber / zf_solver_set_poisson / zf_solver_set_penalty_factors for these."""
        if self.l2 > 0:
            fields["l2"] = self.l2
        if self._w is not None:
            fields["row_weights"] = self._w.data_ptr()
            keep = keep + (self._w,)
        if self._loss == _lib.ZF_LOSS_HUBER:
            fields["huber_delta"] = self.delta
        if self._loss == _lib.ZF_LOSS_POISSON:
            fields["poisson"] = True
        if self._loss == _lib.ZF_LOSS_MULTINOMIAL:   # (the engine calls the setter after the responses)
            fields["multinomial"] = True
        if self._f32:   # (zf_solver_create takes the same address as A; after zf_solver_set_matrix_f32 nothing reads it)
            fields["matrix_f32"] = self.A.data_ptr()
        if self._pf is not None:
            fields["penalty_factors"] = self._pf.data_ptr()
            keep = keep + (self._pf,)
        return fields, keep

    @property
    def penalty_factor(self):
        """The per-column penalty factors (a host copy), or None."""
        return None if self._pf_host is None else self._pf_host.copy()

    def with_penalty_factor(self, p):
        """A sibling problem with g(x) = lam sum_j p_j |x_j| (``p``: n_features values, finite and >= 0; 0 leaves a column
        unpenalised) that SHARES the device matrix, b, the matrix handle and the sample weights: only p is uploaded.  ``None``:
        the plain sibling.  Not with l2 > 0.  ``with_lam`` and ``with_sample_weight`` keep the factors, so ``l1_path`` and
        ``l1_cv`` work through the siblings.  With a zero in ``p`` there is no duality-gap certificate: solve with
        ``gap_tol=None``."""
        import copy

        sib = copy.copy(self)
        sib._set_penalty_factor(p)
        return sib

    def _set_penalty_factor(self, p):
        if p is None:
            self._pf = self._pf_host = None
            return
        host = _check_penalty_factor(p, self.n_features, getattr(self, "group", None), self.l2)
        self._pf_host = host
        self._pf = _to_device(host, "penalty_factor")

    def _pf_refusal(self, what):
        if self._pf is not None:
            raise ValueError(f"{what} is not available with penalty_factor: the gap-safe rule compares against lam p_j, and its "
                             "rounding guard has to be re-derived for g / p; neither is built yet")

    @property
    def sample_weight(self):
        """The per-row sample weights (a host copy), or None."""
        return None if self._w_host is None else self._w_host.copy()

    def with_sample_weight(self, w):
        """A sibling problem with the per-row weights ``w`` (m values, finite and >= 0, at least one > 0; used as given:
        f = scale sum_i w_i loss_i) that SHARES the device matrix, b and (sparse classes) the matrix handle: only w is
        uploaded.  A row with w_i = 0 is a row that is not there, whatever its b_i holds.  ``None``: the unweighted sibling."""
        import copy

        sib = copy.copy(self)
        sib._set_weights(w)
        return sib

    def _set_weights(self, w):
        if w is None:
            self._w = self._w_host = None
            self.__dict__.pop("taylor_remainder", None)
            return
        host = _check_weights(w, self.m_rows, getattr(self, "group", None))
        self._w_host = host
        self._w = _to_device(host, "sample_weight")
        self.taylor_remainder = False   # (the residual kernels that form scale |A (x+ - y)|^2 carry no weights)

    def _weights_refusal(self, what):
        if self._w is not None:
            raise ValueError(f"{what} is not available with sample_weight: the weighted screening rule needs sum_i w_i a_ij^2 for "
                             "|a_j|^2 and a re-derived rounding guard, which are not built yet")

    # -- g / prox with the ridge term (l2 = 0: the shared l1 forms, the same calls as before) --------------------
    def prox_wsum_g(self, weight, x):
        if self._pf is not None:
            x = _as_host(x)
            if x.size != self.n_features:
                raise ValueError(f"len(x) should be equal to n_features, got {x}.")
            out = np.empty_like(x)
            lib = _lib.require_gpu()
            _lib.check(lib.zf_host_prox_pf_box(C.c_void_p(_lib.ptr(out)), C.c_void_p(_lib.ptr(x)), C.c_void_p(_lib.ptr(self._pf_host)),
                                               float(self.lam * weight), self.box[0], self.box[1], x.size), "zf_host_prox_pf_box")
            return out
        if not self.l2 > 0:
            return NativeProblem.prox_wsum_g(self, weight, x)
        x = _as_host(x)
        out = np.empty_like(x)
        lib = _lib.require_gpu()
        shrink = 1.0 / (1.0 + self.l2 * weight)   # once, a scalar: the kernel multiplies
        _lib.check(lib.zf_host_prox_enet_box(C.c_void_p(_lib.ptr(out)), C.c_void_p(_lib.ptr(x)), float(self.lam * weight),
                                             float(shrink), self.box[0], self.box[1], x.size), "zf_host_prox_enet_box")
        return out

    def _eval_fg(self, x):
        lib = _lib.require_gpu()
        s = C.c_double(0.0)
        if self._pf is not None:
            if x.size != self.n_features:
                raise ValueError(f"len(x) should be equal to n_features, got {x}.")
            _lib.check(lib.zf_host_pf_g(C.c_void_p(_lib.ptr(x)), C.c_void_p(_lib.ptr(self._pf_host)), x.size, self.lam, C.byref(s)),
                       "zf_host_pf_g")
            return None, np.float64(s.value)
        if self.l2 > 0:
            _lib.check(lib.zf_host_enet_g(C.c_void_p(_lib.ptr(x)), x.size, self.lam, self.l2, C.byref(s)), "zf_host_enet_g")
            return None, np.float64(s.value)
        _lib.check(lib.zf_host_asum(C.c_void_p(_lib.ptr(x)), x.size, C.byref(s)), "zf_host_asum")
        return None, np.float64(self.lam * s.value)

    _F32_NO_SCREEN = ("the matrix is stored in fp32 (matrix_dtype='float32'): the column-norm and restriction kernels "
                      "(zf_dense_col_norms, zf_dense_restrict) and the screen's rounding guard read and assume an fp64 A")

    def _f32_refusal(self, what):
        if self._f32:
            raise ValueError(f"{what} is not available: {self._F32_NO_SCREEN}")

    def _screen_refusal(self):
        """Why this problem cannot be screened (None: it can)."""
        if self._f32:
            return self._F32_NO_SCREEN
        if self._pf is not None:
            return ("penalty_factor is set: the gap-safe rule compares against lam p_j, and its rounding guard has to be re-derived "
                    "for g / p; neither is built yet")
        if self._w is not None:
            return ("sample_weight is set: the weighted rule needs sum_i w_i a_ij^2 for |a_j|^2 and a re-derived rounding guard, "
                    "which are not built yet")
        if self.l2 > 0:
            return ("l2 > 0: the gap-safe rule of the elastic net (alpha |gt_j| against sqrt(2 gap) sqrt(L |a_j|^2 + l2)) and its "
                    "rounding guard are not built yet")
        return self._gap_refusal()

    def column_norms(self):
        """|a_j|_2 of every column of A: a float64 CUDA tensor of n_features, computed on the GPU once per matrix."""
        import torch

        self._f32_refusal("column_norms")
        self._pf_refusal("column_norms")
        self._weights_refusal("column_norms")
        h = self._norms
        if h.norms is None:
            lib = _lib.require_gpu()
            norms = torch.empty(self.n_features, dtype=torch.float64, device="cuda")
            stats = torch.empty(2, dtype=torch.float64, device="cuda")
            self._norms_call(lib, norms, stats)
            h.norms, h.stats = norms, stats
        return h.norms

    def screen(self, x):
        """The duality gap at ``x`` and, from the same evaluation, the gap-safe screen: ``Screen`` = (gap, keep, count).
        Column j is dropped (``keep[j]`` False) when alpha |g_j| + (r + E) |a_j|_2 < lam, r = sqrt(2 L gap): such a column is
        zero at every optimum.  ``gap`` is, bit for bit, ``duality_gap(x)``."""
        import torch

        why = self._screen_refusal()
        if why:
            raise ValueError(f"screen is not available: {why}")
        if type(x).__module__.split(".")[0] == "torch":
            x = x.detach().cpu().numpy()
        x = _as_host(x)
        if x.size != self.n_features:
            raise ValueError(f"len(x) should be equal to n_features, got {x}.")
        lib = _lib.require_gpu()
        self.column_norms()
        keep = torch.empty(self.n_features, dtype=torch.uint8, device="cuda")
        index = torch.empty(self.n_features, dtype=torch.int32, device="cuda")
        out = np.zeros(12)
        self._screen_call(lib, x, out, self._norms, keep, index)
        return Screen(DualityGap(out[:8]), keep.view(torch.bool), int(out[11]), index, out[8], out[9])

    def _keep_mask(self, keep):
        """``keep`` - a Screen, a device mask, a host boolean mask or a host array of column numbers - as a uint8 CUDA tensor."""
        import torch

        n = self.n_features
        if isinstance(keep, Screen):
            keep = keep.keep
        if isinstance(keep, torch.Tensor):
            if keep.dtype not in (torch.bool, torch.uint8) or keep.ndim != 1 or keep.numel() != n:
                raise ValueError(f"a device mask must be a bool or uint8 tensor of {n} values")
            return keep.cuda().contiguous().view(torch.uint8)
        a = np.asarray(keep)
        if a.dtype == np.bool_:
            if a.shape != (n,):
                raise ValueError(f"a boolean mask must hold {n} values, got shape {a.shape}")
            host = np.ascontiguousarray(a)
        elif a.dtype.kind in "iu" and a.ndim == 1:
            if a.size and (a.min() < 0 or a.max() >= n):
                raise ValueError(f"column numbers must lie in [0, {n})")
            host = np.zeros(n, dtype=np.bool_)
            host[a] = True
            if int(host.sum()) != a.size:
                raise ValueError("column numbers must not repeat")
        else:
            raise ValueError("keep must be a mask (device or host) or a 1-D array of column numbers")
        return torch.from_numpy(host.view(np.uint8)).cuda()

    def restrict(self, keep):
        """The problem over the columns ``keep`` alone - same class, same b (shared), ``n_features`` = the number kept - built
        on the device from the resident matrix: the CSR of A[:, keep] and of its transpose, or the dense A[:, keep].  ``keep``:
        the ``Screen`` of ``screen(x)``, a device mask, a host boolean mask, or a host array of column numbers (the columns
        keep their order).  With x_full[keep] = x and zeros elsewhere, f and jac_f of the restricted problem at x are the
        full problem's at x_full (jac_f: its kept entries).  Keeping no column is refused: that problem's solution is x = 0."""
        self._f32_refusal("restrict")
        self._pf_refusal("restrict")
        self._weights_refusal("restrict")
        why = self._gap_refusal()
        if why:
            raise ValueError(f"restrict is not available: {why}")
        import copy

        sub = copy.copy(self)
        sub._norms = _ColumnNorms()
        self._restrict_into(_lib.require_gpu(), self._keep_mask(keep), sub)
        return sub

    @staticmethod
    def _none_kept():
        return ValueError("no column is kept: the restricted problem has no variable (its solution is x = 0)")

    def _gap_refusal(self):
        """Why this problem has no duality gap (None: it has one)."""
        if self._has_box():
            return "bounds are set: the dual of the boxed problem is a different one"
        if getattr(self, "group", None) is not None:
            return "the problem is sharded over a process group (group=): the dual point needs the whole A^T grad phi"
        if self._pf_host is not None and not np.all(self._pf_host > 0):
            return ("penalty_factor holds a zero (an unpenalised column): the dual candidate cannot be made feasible by scaling - it "
                    "needs a_j^T theta = 0 exactly there; solve with gap_tol=None (the solver's own tol stops the solve)")
        return None

    def duality_gap(self, x):
        """``DualityGap`` at ``x`` (a NumPy array or a float64 CUDA tensor), evaluated on the GPU."""
        why = self._gap_refusal()
        if why:
            raise ValueError(f"duality_gap is not available: {why}")
        x = self._flat(x)
        if type(x).__module__.split(".")[0] == "torch":
            x = x.detach().cpu().numpy()
        x = _as_host(x)
        if x.size != self.n_features:
            raise ValueError(f"len(x) should be equal to n_features, got {x}.")
        out = np.zeros(10 if self.l2 > 0 else 8)
        self._gap_call(_lib.require_gpu(), x, out)
        return DualityGap(out)

    def lam_max(self, tol=1e-10, max_iter=5000, **solver_kwargs):
        """|grad f(0)|_inf: the smallest lam for which x = 0 is optimal.  With penalty factors p > 0: max_j |grad f(0)_j| / p_j.
        With unpenalised columns U (p_j = 0): max over p_j > 0 of |grad f(x_U)_j| / p_j, x_U the minimiser of f over the columns U
        alone - the smallest lam at which every penalised coordinate is zero.  x_U is the solution of ``with_lam(L)`` for an L
        large enough: L starts at twice the value at x = 0 and is accepted when every penalised entry of the solution is exactly
        0 and the resulting value is <= L; otherwise it is doubled, at most 8 times (RuntimeError).  ``tol``, ``max_iter`` and
        ``solver_kwargs`` go to those solves only."""
        g0 = np.abs(self.jac_f(np.zeros(self.n_features)))
        if self._pf_host is None:
            return np.float64(np.max(g0))
        p = self._pf_host
        pen = p > 0
        if not pen.any():
            return np.float64(0.0)
        if pen.all():
            return np.float64(np.max(g0 / p))
        L = 2.0 * float(np.max(g0[pen] / p[pen]))
        if not L > 0:
            L = 1.0
        x = np.zeros(self.n_features)
        for _ in range(8):
            res = self.with_lam(L).minimize_proximal_gradient(x, tol=tol, max_iter=max_iter, **solver_kwargs)
            x = np.asarray(res.x, dtype=np.float64)
            if not np.any(x[pen] != 0):
                val = float(np.max(np.abs(self.jac_f(x))[pen] / p[pen]))
                if val <= L:
                    return np.float64(val)
            x = np.where(pen, 0.0, x)
            L *= 2.0
        raise RuntimeError("lam_max: no lam was found in 8 doublings at which every penalised coordinate is zero (raise max_iter, "
                           "or loosen tol)")

    def with_lam(self, lam):
        """A sibling problem with another l1 weight that SHARES the device matrix, b and (sparse classes) the matrix
        handle: nothing is uploaded."""
        import copy

        sib = copy.copy(self)
        sib.lam = float(lam)
        return sib

    def with_penalty(self, lam, l2):
        """``with_lam`` for both weights of the elastic net: the sibling with g = lam |x|_1 + (l2 / 2) |x|^2 on the same device
        matrix, b and matrix handle; nothing is uploaded."""
        sib = self.with_lam(lam)
        sib.l2 = _check_l2(l2, getattr(self, "group", None))
        if sib.l2 > 0 and self._pf is not None:
            raise ValueError("l2 > 0 is not available with penalty_factor: the ridge term would need the factors too (glmnet scales "
                             "both), and that step is not built")
        return sib


class _DenseMarginsL1(_GapMixin, NativeProblem):
    """What the dense single-GPU problems f(x) = scale * sum_i loss_i((Ax)_i), g = lam |x|_1 (+ (l2 / 2) |x|^2) (+ box) share: A (m x n, dense
    row-major) and the m-vector b in HBM, the matrix fields of the evaluation descriptor, the descriptor of one GPU.  The
    loss is the subclass's: its ``kind``, its ``_loss``, what b means."""

    kind = None

    def _matrix_fields(self):
        """A (fp64 or fp32) and the MATRIX's sizes: with K responses m_rows and n_features are the flattened lengths."""
        K = getattr(self, "n_responses", 1)
        return {"A32" if self._f32 else "A": self.A.data_ptr(), "m_rows": self.m_rows // K, "n": self.n_features // K}

    @property
    def matrix_dtype(self):
        """How A is stored in HBM: "float64" or "float32"."""
        return "float32" if self._f32 else "float64"

    def with_matrix_dtype(self, dtype):
        """A sibling problem whose matrix is stored as ``dtype`` ("float32" or "float64") that SHARES b, the sample weights and the
        penalty factors.  Its matrix is a copy made on the device (``A.to(torch.float32)``: rounded to nearest; or widened, which
        is exact) and it holds no reference to this problem's; a problem that already stores ``dtype`` returns a plain sibling
        (nothing is copied).  An fp32 problem solves, in fp64 arithmetic, exactly the fp64 problem on ``A.to(torch.float64)``: both
        sweeps of a trial read half the bytes, everything else is unchanged (csrc/zf_kernels_gemv_f32.h).  No screening on it."""
        import copy

        import torch

        name = _matrix_dtype(dtype)
        sib = copy.copy(self)
        if name == self.matrix_dtype:
            return sib
        if name == "float32":
            if getattr(self, "group", None) is not None:
                raise ValueError("matrix_dtype='float32' is not available with group=: the fp32 sweeps are built for one GPU (world = 1)")
            A32 = self.A.to(torch.float32)
            if not bool(torch.isfinite(A32).all()):
                raise ValueError("A holds a value that is not finite as float32 (NaN, an infinity, or a magnitude beyond 3.4e38)")
            sib.A, sib._f32 = A32, True
        else:
            sib.A, sib._f32 = self.A.to(torch.float64), False
        sib._norms = _ColumnNorms()
        return sib

    def _set(self, A, b, lam, scale, bounds, l2=0.0, sample_weight=None, group=None, penalty_factor=None, matrix_dtype=None):
        self._f32 = _matrix_dtype(matrix_dtype) == "float32"   # (every ValueError before anything touches the device)
        if self._f32 and group is not None:
            raise ValueError("matrix_dtype='float32' is not available with group=: the fp32 sweeps are built for one GPU (world = 1)")
        self.l2 = _check_l2(l2)
        if sample_weight is not None:   # (every ValueError before anything touches the device)
            sample_weight = _check_weights(sample_weight, int(np.shape(b)[0]) if np.ndim(b) == 1 else -1, group)
        if penalty_factor is not None:
            shape = tuple(getattr(A, "shape", None) or np.shape(A))
            penalty_factor = _check_penalty_factor(penalty_factor, int(shape[1]) if len(shape) == 2 else -1, group, self.l2)
        self.A = _to_device_f32(A, "A") if self._f32 else _to_device(A, "A")
        self.b = _to_device(b, "b")
        if self.A.ndim != 2 or self.b.ndim != 1 or self.A.shape[0] != self.b.shape[0]:
            raise ValueError("A must be (m, n) and b (m,)")
        self.lam, self.scale = float(lam), float(scale)
        self.box = (-np.inf, np.inf) if bounds is None else (float(bounds[0]), float(bounds[1]))
        self.m_rows, self.n_features = int(self.A.shape[0]), int(self.A.shape[1])
        self.group = None
        self._norms = _ColumnNorms()
        self._set_weights(sample_weight)
        self._set_penalty_factor(penalty_factor)

    def _norms_call(self, lib, norms, stats):
        _lib.check(lib.zf_dense_col_norms(_dp(self.A), self.m_rows, self.n_features, _dp(norms), _dp(stats)), "zf_dense_col_norms")

    def _restrict_into(self, lib, mask, sub):
        import torch

        n = self.n_features
        index = torch.empty(n, dtype=torch.int32, device="cuda")
        k = C.c_int64(0)
        _lib.check(lib.zf_screen_scan(_dp(mask), n, _dp(index), C.byref(k)), "zf_screen_scan")
        if k.value == 0:
            raise self._none_kept()
        out = torch.empty((self.m_rows, k.value), dtype=torch.float64, device="cuda")
        _lib.check(lib.zf_dense_restrict(_dp(self.A), self.m_rows, n, _dp(mask), _dp(index), k.value, _dp(out)), "zf_dense_restrict")
        sub.A, sub.n_features = out, int(k.value)

    def _descriptor(self, rank=0, world=1, row_sharded=0):
        fields = dict(kind=self.kind, world=world, rank=rank, n=self.n_features, m_rows=self.m_rows, row_sharded=row_sharded,
                      d=None, c=None, A=self.A.data_ptr(), b=self.b.data_ptr(),
                      scale=self.scale, lam=self.lam, box_lo=self.box[0], box_hi=self.box[1])
        return self._finish_descriptor(fields, (self.A, self.b))


class LeastSquaresL1(_DenseMarginsL1):
    r"""f(x) = scale \|Ax - b\|^2,  g(x) = lam \|x\|_1 (+ optional box); A dense row-major.

    The LASSO closures of tests/test_proximal_gradient.py:49-61,81-97 are the
    ``scale = 1/6`` member; BASELINE cfg1 / cfg3 use ``scale = 1/2``.
    """

    kind = _lib.ZF_PROBLEM_LEAST_SQUARES_L1
    taylor_remainder = True   # acceptance="remainder": R = scale |A (x+ - y)|^2 from the residual kernels at x+

    def __init__(self, A, b, lam, scale=0.5, bounds=None, group=None, shard="columns", l2=0.0, *, sample_weight=None, penalty_factor=None,
                 matrix_dtype=None):
        """With ``group`` set and ``shard="columns"`` (default), ``A`` is this rank's column block A_p
        (m x n_p, row-major) of a matrix whose columns - and the decision vector - are partitioned
        over the ranks of that process group; ``b`` is replicated; the solve exchanges the m-vector
        A_p x_p once per trial.  ``shard="rows"``: ``A`` (m_p x n) and ``b`` (m_p) are this rank's ROW
        block, x is replicated on every rank (pass the whole x0) and the n-vector A_p^T r_p is
        exchanged instead - the layout for tall matrices.  ``f`` / ``jac_f`` as plain callables
        refer to the local block only.  ``matrix_dtype="float32"`` stores A in single precision (``with_matrix_dtype``): a float32
        CUDA tensor is adopted as it is, anything else is rounded to nearest; not with ``group``."""
        if shard not in ("columns", "rows"):
            raise ValueError("shard must be 'columns' or 'rows'")
        self.shard = shard
        _check_l2(l2, group)
        self._set(A, b, lam, scale, bounds, l2, sample_weight, group, penalty_factor, matrix_dtype)
        self.group = group

    def _descriptor(self):
        from .comm import rank_world

        rank, world = rank_world(self.group)
        return super()._descriptor(rank, world, int(self.shard == "rows" and world > 1))


class _SpmatHandle:
    """Owner of a ``zf_spmat`` handle and of the device arrays behind it."""

    def __init__(self, prep, dev=None):
        """``prep``: what ``sparse.prepare`` returns, uploaded here - or, with ``dev`` (the six arrays, already in HBM), only
        its sizes and the two plans."""
        import torch

        lib = _lib.require_gpu()
        self.lib = lib
        names = ("indptr", "indices", "data", "t_indptr", "t_indices", "t_data")
        self.dev = {k: torch.from_numpy(prep[k]).cuda() for k in names} if dev is None else {k: dev[k] for k in names}
        self.plans = []   # (the host arrays a zf_spmv_plan points to, for the duration of the call)
        for key in ("plan", "t_plan"):
            p = prep[key]
            c = _lib.SpmvPlan(lanes=p["lanes"], threshold=p["threshold"], nsplit=p["split_row"].size, nseg=p["seg_start"].size,
                              split_row=_lib.ptr(p["split_row"]) if p["split_row"].size else None,
                              split_first=_lib.ptr(p["split_first"]) if p["split_row"].size else None,
                              seg_start=_lib.ptr(p["seg_start"]) if p["seg_start"].size else None)
            self.plans.append((c, p))
        dp = lambda k: C.c_void_p(self.dev[k].data_ptr() if self.dev[k].numel() else None)
        h = C.c_void_p()
        _lib.check(lib.zf_spmat_create(C.byref(h), prep["m"], prep["n"], prep["nnz"], dp("indptr"), dp("indices"), dp("data"),
                                       C.byref(self.plans[0][0]), dp("t_indptr"), dp("t_indices"), dp("t_data"),
                                       C.byref(self.plans[1][0]), C.sizeof(_lib.SpmvPlan)), "zf_spmat_create")
        self.value = h

    def __del__(self):
        try:
            if getattr(self, "value", None):
                self.lib.zf_spmat_destroy(self.value)
                self.value = None
        except Exception:
            pass


class _SparseMarginsL1(_GapMixin, NativeProblem):
    """What the sparse single-GPU problems f(x) = scale * sum_i loss_i((Ax)_i), g = lam |x|_1 (+ box) share: the canonical
    CSR of A and of A^T behind one immutable handle, b in HBM, the matrix field of the evaluation descriptor, the
    descriptor.  The loss is the subclass's: its ``kind``, its ``_loss``, what b means."""

    kind = None

    def _matrix_fields(self):
        return {"spmat": self._spmat.value.value}

    def _set(self, A, b, lam, scale, bounds, l2=0.0, sample_weight=None, penalty_factor=None):
        import torch

        from . import sparse

        self.l2 = _check_l2(l2)
        if sample_weight is not None:   # (every ValueError before anything touches the device)
            sample_weight = _check_weights(sample_weight, int(A.shape[0]))
        if penalty_factor is not None:
            penalty_factor = _check_penalty_factor(penalty_factor, int(A.shape[1]), None, self.l2)

        b_host = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b
        prep = sparse.prepare(A, b_host)   # (every ValueError comes from here, before anything touches the device)
        self.b = _to_device(b, "b")
        self.lam, self.scale = float(lam), float(scale)
        self.box = (-np.inf, np.inf) if bounds is None else (float(bounds[0]), float(bounds[1]))
        self.m_rows, self.n_features, self.nnz = prep["m"], prep["n"], prep["nnz"]
        self.plan = (prep["plan"], prep["t_plan"])
        self.group = None
        self._spmat = _SpmatHandle(prep)
        self._norms = _ColumnNorms()
        self._longest = (int(np.diff(prep["indptr"]).max(initial=0)), int(np.diff(prep["t_indptr"]).max(initial=0)))
        self._set_weights(sample_weight)
        self._set_penalty_factor(penalty_factor)

    def _norms_call(self, lib, norms, stats):
        _lib.check(lib.zf_spmat_col_norms(self._spmat.value, _dp(norms), _dp(stats)), "zf_spmat_col_norms")

    def _restrict_into(self, lib, mask, sub):
        """Counts, the two scans of the lengths (torch.cumsum), the fill; the host reads the two new row pointer arrays for the
        plans (sparse.plan_rows) and creates the handle on the device arrays."""
        import torch

        from . import sparse

        m, n, h = self.m_rows, self.n_features, self._spmat
        i64 = dict(dtype=torch.int64, device="cuda")
        index = torch.empty(n, dtype=torch.int32, device="cuda")
        seg_off = torch.empty(self.plan[0]["seg_start"].size, dtype=torch.int32, device="cuda")
        lens, t_lens = torch.empty(m, **i64), torch.empty(n, **i64)
        k = C.c_int64(0)
        _lib.check(lib.zf_spmat_restrict_count(h.value, _dp(mask), _dp(index), _dp(lens), _dp(t_lens), _dp(seg_off), C.byref(k)),
                   "zf_spmat_restrict_count")
        k = int(k.value)
        if k == 0:
            raise self._none_kept()
        dev = dict(indptr=torch.zeros(m + 1, **i64), t_indptr=torch.zeros(k + 1, **i64))
        dev["indptr"][1:] = torch.cumsum(lens, 0)
        dev["t_indptr"][1:] = torch.cumsum(t_lens[:k], 0)
        indptr, t_indptr = dev["indptr"].cpu().numpy(), dev["t_indptr"].cpu().numpy()
        nnz = int(indptr[-1])
        for key in ("indices", "t_indices"):
            dev[key] = torch.empty(nnz, dtype=torch.int32, device="cuda")
        for key in ("data", "t_data"):
            dev[key] = torch.empty(nnz, dtype=torch.float64, device="cuda")
        _lib.check(lib.zf_spmat_restrict_fill(h.value, _dp(mask), _dp(index), _dp(seg_off), k, nnz, _dp(dev["indptr"]), _dp(dev["indices"]),
                                              _dp(dev["data"]), _dp(dev["t_indptr"]), _dp(dev["t_indices"]), _dp(dev["t_data"])),
                   "zf_spmat_restrict_fill")
        prep = dict(m=m, n=k, nnz=nnz, plan=sparse.plan_rows(indptr), t_plan=sparse.plan_rows(t_indptr))
        sub.n_features, sub.nnz, sub.plan = k, nnz, (prep["plan"], prep["t_plan"])
        sub._spmat = _SpmatHandle(prep, dev)
        sub._longest = (int(np.diff(indptr).max(initial=0)), int(np.diff(t_indptr).max(initial=0)))

    def _descriptor(self):
        fields = dict(kind=self.kind, world=1, rank=0, n=self.n_features, m_rows=self.m_rows, row_sharded=0,
                      d=None, c=None, A=None, b=self.b.data_ptr(), scale=self.scale, lam=self.lam,
                      box_lo=self.box[0], box_hi=self.box[1], spmat=self._spmat.value.value)
        return self._finish_descriptor(fields, (self._spmat, self.b))


class SparseLeastSquaresL1(_SparseMarginsL1):
    r"""f(x) = scale \|Ax - b\|^2,  g(x) = lam \|x\|_1 (+ optional box) with a SPARSE A: the problem of
    ``LeastSquaresL1`` - same keywords, same result fields - for matrices that have no dense form in HBM.

    ``A``: a scipy.sparse matrix / array of any format and real dtype (m x n; m, n < 2**31).  It is made canonical CSR on
    the host (duplicates summed, indices sorted; float64 values, int32 column indices, int64 row pointers), and so is
    ``A.T``: both sweeps of a trial - A x+ and A^T r - are row sums of a stored matrix against a gathered vector
    (csrc/zf_kernels_spmv.h), with no atomics and in an order fixed by the matrix alone.  Both copies go to HBM: 24 B per
    stored element in total.  A matrix with no stored element is legal.  Single GPU."""

    kind = _lib.ZF_PROBLEM_SPARSE_LS_L1
    taylor_remainder = True   # acceptance="remainder": R = scale |A (x+ - y)|^2 from the residual kernels at x+

    def __init__(self, A, b, lam, scale=0.5, bounds=None, l2=0.0, *, sample_weight=None, penalty_factor=None):
        self._set(A, b, lam, scale, bounds, l2, sample_weight, penalty_factor=penalty_factor)


def _check_labels(b, m=None):
    """The labels of a logistic problem as a host vector: exactly -1 or +1, one per row.  ValueError otherwise - on the
    host, before anything touches the device (a torch tensor is copied to the host for the check)."""
    host = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
    if host.ndim != 1 or (m is not None and host.shape[0] != m):
        raise ValueError(f"b must be a vector of {'m' if m is None else m} labels (the rows of A), got shape {host.shape}")
    if np.dtype(host.dtype).kind not in "biuf" or not np.all((host == 1) | (host == -1)):
        raise ValueError("the labels b must be exactly -1 or +1")
    return host


class LogisticL1(_DenseMarginsL1):
    r"""f(x) = scale \sum_i softplus(-b_i (Ax)_i) with labels b_i in {-1, +1},  g(x) = lam \|x\|_1 (+ optional box); A dense
    row-major: L1-regularised logistic regression on the device-resident trial of ``LeastSquaresL1`` - same keywords,
    same result fields.  grad f = scale A^T rho, rho_i = -b_i sigma(-b_i (Ax)_i) (csrc/zf_kernels_loss.h: one
    exp(-|t|) per row feeds both, finite for every finite margin).  Labels other than exactly -1 / +1 raise ValueError.
    Single GPU.  The elastic net: ``LogisticL1(A, b, lam).with_penalty(lam, l2)``; sample weights:
    ``LogisticL1(A, b, lam).with_sample_weight(w)`` (the constructor's parameter list is fixed)."""

    kind = _lib.ZF_PROBLEM_LOGISTIC_L1
    _loss = _lib.ZF_LOSS_LOGISTIC

    def __init__(self, A, b, lam, scale=1.0, bounds=None):
        shape = tuple(getattr(A, "shape", np.shape(A)))
        if len(shape) != 2:
            raise ValueError("A must be (m, n) and b (m,)")
        _check_labels(b, shape[0])
        self._set(A, b, lam, scale, bounds)


class SparseLogisticL1(_SparseMarginsL1):
    r"""``LogisticL1`` with a SPARSE A (any scipy.sparse matrix): the matrix is prepared, stored and swept exactly as for
    ``SparseLeastSquaresL1`` (canonical CSR of A and of A^T behind one immutable handle); the loss kernels are the dense
    class's.  Single GPU."""

    kind = _lib.ZF_PROBLEM_SPARSE_LOGISTIC_L1
    _loss = _lib.ZF_LOSS_LOGISTIC

    def __init__(self, A, b, lam, scale=1.0, bounds=None):
        _check_labels(b)
        self._set(A, b, lam, scale, bounds)


def _check_delta(delta):
    """The threshold of Huber's loss as a float: finite and > 0."""
    delta = float(delta)
    if not (np.isfinite(delta) and delta > 0):
        raise ValueError(f"delta must be finite and > 0 (the residual size beyond which Huber's loss is linear), got {delta!r}")
    return delta


class _HuberMixin:
    """Huber's loss on the trial of a least-squares class: f(x) = scale sum_i H(r_i), r = A x - b, H(r) = r^2 for
    |r| <= delta and delta (2 |r| - delta) beyond; grad f = 2 scale A^T clip(r, -delta, delta) (csrc/zf_kernels_loss.h).  The
    problem kind is the least-squares one; ``huber_delta`` in the descriptor fields makes the engine call
    ``zf_solver_set_huber``.  No ``taylor_remainder``: scale |A (x+ - y)|^2 is not this loss's remainder, so
    ``acceptance="remainder"`` is refused as for the logistic classes."""

    _loss = _lib.ZF_LOSS_HUBER

    @staticmethod
    def _refuse_group(group):
        if group is not None:
            raise ValueError("group= is not available: the Huber loss kernels, their certificate and zf_solver_set_huber are built "
                             "for one GPU (world = 1)")


class HuberL1(_HuberMixin, _DenseMarginsL1):
    r"""f(x) = scale \sum_i H_delta((Ax - b)_i),  g(x) = lam \|x\|_1 (+ (l2 / 2) \|x\|^2) (+ optional box); A dense row-major:
    robust L1 regression on the device-resident trial of ``LeastSquaresL1`` - same keywords, same result fields, with the
    duality-gap certificate, ``gap_tol``, ``l1_path``, screening (l2 = 0) and the elastic net.  ``scale = 0.5`` is the
    textbook Huber function (r^2 / 2 inside, delta |r| - delta^2 / 2 beyond).  Single GPU."""

    kind = _lib.ZF_PROBLEM_LEAST_SQUARES_L1

    def __init__(self, A, b, lam, delta, scale=0.5, bounds=None, l2=0.0, *, group=None, sample_weight=None, penalty_factor=None,
                 matrix_dtype=None):
        self._refuse_group(group)
        self.delta = _check_delta(delta)
        self._set(A, b, lam, scale, bounds, l2, sample_weight, penalty_factor=penalty_factor, matrix_dtype=matrix_dtype)


class SparseHuberL1(_HuberMixin, _SparseMarginsL1):
    r"""``HuberL1`` with a SPARSE A (any scipy.sparse matrix): the matrix is prepared, stored and swept exactly as for
    ``SparseLeastSquaresL1``; the loss kernels are the dense class's and sum the rows of the same m in the same order.
    Single GPU."""

    kind = _lib.ZF_PROBLEM_SPARSE_LS_L1

    def __init__(self, A, b, lam, delta, scale=0.5, bounds=None, l2=0.0, *, group=None, sample_weight=None, penalty_factor=None):
        self._refuse_group(group)
        self.delta = _check_delta(delta)
        self._set(A, b, lam, scale, bounds, l2, sample_weight, penalty_factor=penalty_factor)


def _check_counts(b, m=None):
    """The counts of a Poisson problem as a host vector: finite and >= 0, one per row (not necessarily integers).  ValueError
    otherwise - on the host, before anything touches the device (a torch tensor is copied to the host for the check)."""
    host = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
    if host.ndim != 1 or (m is not None and host.shape[0] != m):
        raise ValueError(f"b must be a vector of {'m' if m is None else m} counts (the rows of A), got shape {host.shape}")
    if np.dtype(host.dtype).kind not in "biuf" or not np.all(np.isfinite(host)) or np.any(host < 0):
        raise ValueError("the counts b must be finite and >= 0")
    return host


class _PoissonMixin:
    """The Poisson loss with a log link on the trial of a least-squares class: f(x) = scale sum_i w_i (exp(z_i) - b_i z_i),
    z = A x; grad f = scale A^T (w o (exp(z) - b)) (csrc/zf_kernels_loss.h: one exp per row).  The problem kind is the
    least-squares one; ``poisson`` in the descriptor fields makes the engine call ``zf_solver_set_poisson``.  No
    ``taylor_remainder`` and not separable: ``acceptance="remainder"`` / ``"resolved"`` are refused.  No screening: exp is not
    globally Lipschitz, so the gap-safe radius sqrt(2 L gap) does not apply."""

    _loss = _lib.ZF_LOSS_POISSON

    @staticmethod
    def _refuse_group(group):
        if group is not None:
            raise ValueError("group= is not available: the Poisson loss kernels, their certificate and zf_solver_set_poisson are "
                             "built for one GPU (world = 1)")

    def _screen_refusal(self):
        return ("the Poisson loss has no globally Lipschitz gradient, so the gap-safe radius sqrt(2 L gap) does not apply "
                "(a level-set bound is not built)")

    def _no_screening(self, what):
        raise ValueError(f"{what} is not available: {self._screen_refusal()}")

    def column_norms(self):
        self._no_screening("column_norms")

    def restrict(self, keep):
        self._no_screening("restrict")

    def lam_max(self, *args, **kwargs):
        """|grad f(0)|_inf = scale |A^T (w o (1 - b))|_inf: the smallest lam for which x = 0 is optimal (with penalty factors:
        as the other margins classes)."""
        return super().lam_max(*args, **kwargs)


class PoissonL1(_PoissonMixin, _DenseMarginsL1):
    r"""f(x) = scale \sum_i w_i (exp((Ax)_i) - b_i (Ax)_i),  g(x) = lam \|x\|_1 (+ (l2 / 2) \|x\|^2) (+ optional box); A dense
    row-major: L1-regularised Poisson regression with a log link on the device-resident trial of ``LeastSquaresL1`` - same
    keywords, same result fields, with the duality-gap certificate, ``gap_tol``, ``l1_path``, ``l1_cv``, the elastic net and
    sample weights.  The negative log-likelihood up to the constant log b!.

    ``b``: the counts, finite and >= 0.  They need not be integers: with an exposure t_i per row, pass the RATE
    ``b = count / t`` and ``sample_weight = t`` - w_i (exp(z_i) - (count_i / t_i) z_i) is the likelihood of
    count_i ~ Poisson(t_i exp(z_i)) up to a constant, so exposure is exactly a sample weight.  A trial whose margins leave
    the range of exp has f = +inf and is rejected: the line search backtracks.  No screening (``column_norms``, ``screen``,
    ``restrict``, ``solve_screened``, ``l1_path(screen=True)``): exp is not globally Lipschitz.  Single GPU."""

    kind = _lib.ZF_PROBLEM_LEAST_SQUARES_L1

    def __init__(self, A, b, lam, scale=1.0, bounds=None, l2=0.0, *, group=None, sample_weight=None, penalty_factor=None,
                 matrix_dtype=None):
        self._refuse_group(group)
        shape = tuple(getattr(A, "shape", np.shape(A)))
        if len(shape) != 2:
            raise ValueError("A must be (m, n) and b (m,)")
        _check_counts(b, shape[0])
        self._set(A, b, lam, scale, bounds, l2, sample_weight, penalty_factor=penalty_factor, matrix_dtype=matrix_dtype)


class SparsePoissonL1(_PoissonMixin, _SparseMarginsL1):
    r"""``PoissonL1`` with a SPARSE A (any scipy.sparse matrix): the matrix is prepared, stored and swept exactly as for
    ``SparseLeastSquaresL1``; the loss kernels are the dense class's and sum the rows of the same m in the same order.
    Single GPU."""

    kind = _lib.ZF_PROBLEM_SPARSE_LS_L1

    def __init__(self, A, b, lam, scale=1.0, bounds=None, l2=0.0, *, group=None, sample_weight=None, penalty_factor=None):
        self._refuse_group(group)
        _check_counts(b)
        self._set(A, b, lam, scale, bounds, l2, sample_weight, penalty_factor=penalty_factor)


# ---------------------------------------------------------------------------
# K responses on one dense matrix (csrc/zf_kernels_mr.h)
# ---------------------------------------------------------------------------
MAX_RESPONSES = 16


def _broadcast_columns(v, rows, K, what, per):
    """``v`` - (rows,) or (rows, K), host or torch - as a host (rows, K) array (a 1-D form is repeated for every response)."""
    host = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    if np.dtype(host.dtype).kind not in "biuf":
        raise ValueError(f"{what} must be real numbers, got dtype {host.dtype}")
    if host.shape == (rows,):
        host = np.repeat(host.reshape(rows, 1), K, axis=1)
    if host.shape != (rows, K):
        raise ValueError(f"{what} must have shape ({rows},) or ({rows}, {K}) (one value per {per}, or per {per} and response), "
                         f"got shape {host.shape}")
    return np.ascontiguousarray(host, dtype=np.float64)


class _MultiResponseMixin:
    r"""K right-hand sides on one resident matrix: X in R^{n x K}, B in R^{m x K},

        f(X) = scale sum_k sum_i W_ik phi((A x_k)_i ; B_ik),   g(X) = lam sum_jk P_jk |X_jk| (+ (l2 / 2) |X|^2) (+ box).

    This is the plain problem of the class on the matrix A (x) I_K (``np.kron(A, np.eye(K))``) with every array flattened in C
    order - ``x[j K + k] = X[j, k]`` - so everything the plain class offers carries over on vectors of n K and m K entries;
    only the two sweeps over A differ: they multiply A into K columns and read A once per sweep (csrc/zf_kernels_mr.h), so K
    solves cost one solve's HBM traffic.  One step size serves all responses (the Lipschitz constant of A (x) I_K is A's).
    ``n_features`` = n K, ``n_responses`` = K, ``coef(x)`` -> (n, K); ``x0`` may be (n, K) or flat, results are flat.
    The duality gap uses one alpha for all responses: the dual point is feasible for each of them, and the gap is the sum of
    the K per-response gaps at that point.  K = 1 is the plain class, bit for bit.  K <= 16.  No screening, no fp32 matrix,
    no process group, no acceptance="remainder" / "resolved"."""

    taylor_remainder = False
    n_responses = 1

    _MR_WHY = ("the problem has several responses: the column-norm, screening and restriction kernels see one column of x per "
               "column of A, and the K-response forms are not built")

    def _check_mr(self, shape, B, l2, sample_weight, penalty_factor):
        """Everything that can be refused is refused on the host, before anything touches the device: (B as a host array, m, n,
        K, the flat weights or None, the flat factors or None) for a matrix of ``shape``; sets ``l2``."""
        Bh = B.detach().cpu().numpy() if hasattr(B, "detach") else np.asarray(B)
        if len(shape) != 2 or Bh.ndim != 2 or Bh.shape[0] != shape[0] or Bh.shape[1] < 1:
            raise ValueError(f"A must be (m, n) and B (m, K) with K >= 1, got A {shape} and B {Bh.shape}")
        m, n, K = int(shape[0]), int(shape[1]), int(Bh.shape[1])
        if K > MAX_RESPONSES:
            raise ValueError(f"at most {MAX_RESPONSES} responses per problem (the register tiles of the K-response sweeps are built "
                             f"for K <= {MAX_RESPONSES}), got K = {K}: split B into groups of columns")
        if self._loss == _lib.ZF_LOSS_LOGISTIC:
            _check_labels(Bh.reshape(-1))
        self.l2 = _check_l2(l2)
        w = p = None
        if sample_weight is not None:
            w = _check_weights(_broadcast_columns(sample_weight, m, K, "sample_weight", "row").reshape(-1), m * K)
        if penalty_factor is not None:
            p = _check_penalty_factor(_broadcast_columns(penalty_factor, n, K, "penalty_factor", "column").reshape(-1), n * K, None, self.l2)
        return Bh, m, n, K, w, p

    def _finish_mr(self, Bh, lam, scale, bounds, m, n, K, w, p):
        """B, the scalars, the flattened lengths, the weights and the factors - whatever the storage of the matrix is."""
        self.b = _to_device(np.ascontiguousarray(Bh, dtype=np.float64).reshape(-1), "B")
        self.lam, self.scale = float(lam), float(scale)
        self.box = (-np.inf, np.inf) if bounds is None else (float(bounds[0]), float(bounds[1]))
        self.n_responses, self._m, self._n = K, m, n
        self.m_rows, self.n_features = m * K, n * K   # (the lengths of the flattened margins and decision vectors)
        self.group = None
        self._norms = _ColumnNorms()
        self._set_weights(w)
        self._set_penalty_factor(p)

    def _set_mr(self, A, B, lam, scale, bounds, l2, sample_weight, penalty_factor, share=None):
        """``share``: a plain problem whose device matrix is adopted (``with_responses``)."""
        shape = tuple(share.A.shape) if share is not None else tuple(getattr(A, "shape", None) or np.shape(A))
        checked = self._check_mr(shape, B, l2, sample_weight, penalty_factor)
        self._f32 = False
        self.A = share.A if share is not None else _to_device(A, "A")
        self._finish_mr(checked[0], lam, scale, bounds, *checked[1:])

    # -- shapes --------------------------------------------------------------------------------
    def coef(self, x):
        """The flat vector ``x`` as the (n, K) matrix of coefficients, one column per response."""
        return np.asarray(x, dtype=np.float64).reshape(self._n, self.n_responses)

    def _flat(self, x):
        if type(x).__module__.split(".")[0] == "torch":
            return x.reshape(-1) if x.ndim == 2 and tuple(x.shape) == (self._n, self.n_responses) else x
        a = np.asarray(x)
        return a.reshape(-1) if a.ndim == 2 and a.shape == (self._n, self.n_responses) else x

    def minimize_proximal_gradient(self, x0, **kwargs):
        return NativeProblem.minimize_proximal_gradient(self, self._flat(x0), **kwargs)

    def _descriptor(self):
        fields, keep = super()._descriptor()   # (m_rows and n_features are the flattened lengths already)
        if self.n_responses > 1:
            fields["responses"] = self.n_responses
        return fields, keep

    # -- siblings ------------------------------------------------------------------------------
    def with_sample_weight(self, w):
        """A sibling with the weights ``w`` - (m,), repeated for every response, or (m, K) - on the same device matrix and B."""
        if w is not None:
            w = _broadcast_columns(w, self._m, self.n_responses, "sample_weight", "row").reshape(-1)
        return super().with_sample_weight(w)

    def with_penalty_factor(self, p):
        """A sibling with the penalty factors ``p`` - (n,), repeated for every response, or (n, K) - on the same device matrix."""
        if p is not None:
            p = _broadcast_columns(p, self._n, self.n_responses, "penalty_factor", "column").reshape(-1)
        return super().with_penalty_factor(p)

    def with_matrix_dtype(self, dtype):
        if _matrix_dtype(dtype) == "float32":
            raise ValueError("matrix_dtype='float32' is not available with several responses: the K-response sweeps read an fp64 A")
        return super().with_matrix_dtype(dtype)

    # -- what has no K-response form ---------------------------------------------------------------
    def _mr_refusal(self, what):
        if self.n_responses > 1:
            raise ValueError(f"{what} is not available: {self._MR_WHY}")

    def _screen_refusal(self):
        return self._MR_WHY if self.n_responses > 1 else super()._screen_refusal()

    def column_norms(self):
        self._mr_refusal("column_norms")
        return super().column_norms()

    def screen(self, x):
        self._mr_refusal("screen")
        return super().screen(x)

    def restrict(self, keep):
        self._mr_refusal("restrict")
        return super().restrict(keep)


class MultiResponseLeastSquaresL1(_MultiResponseMixin, _DenseMarginsL1):
    r"""``LeastSquaresL1`` for K right-hand sides at once: f(X) = scale \|A X - B\|_F^2 (weighted: scale sum W o (A X - B)^2),
    B (m, K); sklearn's ``Lasso.fit(X, Y)`` with 2-D ``Y``.  See ``_MultiResponseMixin``."""

    kind = _lib.ZF_PROBLEM_LEAST_SQUARES_L1

    def __init__(self, A, B, lam, scale=0.5, bounds=None, l2=0.0, *, sample_weight=None, penalty_factor=None, _share=None):
        self._set_mr(A, B, lam, scale, bounds, l2, sample_weight, penalty_factor, _share)


class MultiResponseLogisticL1(_MultiResponseMixin, _DenseMarginsL1):
    r"""``LogisticL1`` for K label vectors at once (one-vs-rest classification): B (m, K) holds exactly -1 / +1.
    See ``_MultiResponseMixin``."""

    kind = _lib.ZF_PROBLEM_LOGISTIC_L1
    _loss = _lib.ZF_LOSS_LOGISTIC

    def __init__(self, A, B, lam, scale=1.0, bounds=None, l2=0.0, *, sample_weight=None, penalty_factor=None, _share=None):
        self._set_mr(A, B, lam, scale, bounds, l2, sample_weight, penalty_factor, _share)


def _with_responses(problem, cls, B, sample_weight):
    if problem._f32:
        raise ValueError("with_responses is not available with matrix_dtype='float32': the K-response sweeps read an fp64 A")
    if getattr(problem, "group", None) is not None:
        raise ValueError("with_responses is not available with group=: the K-response sweeps are built for one GPU (world = 1)")
    bounds = problem.box if problem._has_box() else None
    return cls(None, B, problem.lam, problem.scale, bounds, problem.l2, sample_weight=sample_weight,
               penalty_factor=problem.penalty_factor, _share=problem)


def _ls_with_responses(self, B, sample_weight=None):
    """A ``MultiResponseLeastSquaresL1`` on this problem's device matrix (shared, nothing but B is uploaded) with its lam, scale,
    bounds, l2 and penalty factors (repeated for every response).  ``B``: (m, K); ``sample_weight``: (m,) or (m, K) or None.
    Not for an fp32 matrix or a process group."""
    return _with_responses(self, MultiResponseLeastSquaresL1, B, sample_weight)


def _logistic_with_responses(self, B, sample_weight=None):
    """A ``MultiResponseLogisticL1`` on this problem's device matrix (shared, nothing but B is uploaded) with its lam, scale,
    bounds, l2 and penalty factors (repeated for every response).  ``B``: (m, K) of -1 / +1; ``sample_weight``: (m,) or (m, K) or
    None."""
    return _with_responses(self, MultiResponseLogisticL1, B, sample_weight)


LeastSquaresL1.with_responses = _ls_with_responses
LogisticL1.with_responses = _logistic_with_responses


# ---------------------------------------------------------------------------
# K responses on one CSR matrix (csrc/zf_kernels_spmm.h)
# ---------------------------------------------------------------------------
class _SparseMultiResponseMixin(_MultiResponseMixin):
    r"""``_MultiResponseMixin`` on the storage of ``_SparseMarginsL1``: the plain sparse problem on ``sp.kron(A, sp.identity(K))``
    with every array flattened in C order, solved on the handle of A as it is - same CSR arrays, same plans, nothing stored K
    times.  The two sweeps gather the K values of a stored element as K 8 contiguous bytes (csrc/zf_kernels_spmm.h): one index,
    one value and one gathered line serve K responses, and response k is summed exactly as the plain sweep sums a vector, so
    every output is bit-equal to the plain sparse class on the Kronecker matrix.  K = 1 is the plain sparse class, bit for bit
    (the plain creator; K = 1 in the evaluation descriptor).  K <= 16.  No screening, no acceptance="remainder" / "resolved"."""

    def _set_mr(self, A, B, lam, scale, bounds, l2, sample_weight, penalty_factor, share=None):
        """``share``: a plain sparse problem whose matrix handle - the object itself - is adopted (``with_responses``)."""
        from . import sparse

        shape = (share.m_rows, share.n_features) if share is not None else tuple(getattr(A, "shape", None) or ())
        checked = self._check_mr(shape, B, l2, sample_weight, penalty_factor)
        if self._loss != _lib.ZF_LOSS_MULTINOMIAL and not np.isfinite(checked[0]).all():   # (the multinomial classes check Y row by row)
            raise ValueError("B holds non-finite values")
        if share is not None:
            self._spmat, self.nnz, self.plan, self._longest = share._spmat, share.nnz, share.plan, share._longest
        else:
            prep = sparse.prepare(A)   # (every ValueError comes from here, before anything touches the device)
            self.nnz, self.plan = prep["nnz"], (prep["plan"], prep["t_plan"])
            self._longest = (int(np.diff(prep["indptr"]).max(initial=0)), int(np.diff(prep["t_indptr"]).max(initial=0)))
            self._spmat = _SpmatHandle(prep)
        self._finish_mr(checked[0], lam, scale, bounds, *checked[1:])

    def with_matrix_dtype(self, dtype):
        raise ValueError("with_matrix_dtype is not available: a sparse matrix is stored as fp64 values")


class SparseMultiResponseLeastSquaresL1(_SparseMultiResponseMixin, _SparseMarginsL1):
    r"""``SparseLeastSquaresL1`` for K right-hand sides at once: f(X) = scale \|A X - B\|_F^2 (weighted: scale sum W o (A X - B)^2),
    B (m, K), A any scipy.sparse matrix.  See ``_SparseMultiResponseMixin``."""

    kind = _lib.ZF_PROBLEM_SPARSE_LS_L1

    def __init__(self, A, B, lam, scale=0.5, bounds=None, l2=0.0, *, sample_weight=None, penalty_factor=None, _share=None):
        self._set_mr(A, B, lam, scale, bounds, l2, sample_weight, penalty_factor, _share)


class SparseMultiResponseLogisticL1(_SparseMultiResponseMixin, _SparseMarginsL1):
    r"""``SparseLogisticL1`` for K label vectors at once (one-vs-rest classification): B (m, K) holds exactly -1 / +1.
    See ``_SparseMultiResponseMixin``."""

    kind = _lib.ZF_PROBLEM_SPARSE_LOGISTIC_L1
    _loss = _lib.ZF_LOSS_LOGISTIC

    def __init__(self, A, B, lam, scale=1.0, bounds=None, l2=0.0, *, sample_weight=None, penalty_factor=None, _share=None):
        self._set_mr(A, B, lam, scale, bounds, l2, sample_weight, penalty_factor, _share)


def _sparse_with_responses(problem, cls, B, sample_weight):
    bounds = problem.box if problem._has_box() else None
    return cls(None, B, problem.lam, problem.scale, bounds, problem.l2, sample_weight=sample_weight,
               penalty_factor=problem.penalty_factor, _share=problem)


def _sparse_ls_with_responses(self, B, sample_weight=None):
    """A ``SparseMultiResponseLeastSquaresL1`` on this problem's matrix handle (the same object: no upload, no new plan; only B is
    uploaded) with its lam, scale, bounds, l2 and penalty factors (repeated for every response).  ``B``: (m, K);
    ``sample_weight``: (m,) or (m, K) or None."""
    return _sparse_with_responses(self, SparseMultiResponseLeastSquaresL1, B, sample_weight)


def _sparse_logistic_with_responses(self, B, sample_weight=None):
    """A ``SparseMultiResponseLogisticL1`` on this problem's matrix handle (the same object; only B is uploaded) with its lam,
    scale, bounds, l2 and penalty factors (repeated for every response).  ``B``: (m, K) of -1 / +1; ``sample_weight``: (m,) or
    (m, K) or None."""
    return _sparse_with_responses(self, SparseMultiResponseLogisticL1, B, sample_weight)


SparseLeastSquaresL1.with_responses = _sparse_ls_with_responses
SparseLogisticL1.with_responses = _sparse_logistic_with_responses


# ---------------------------------------------------------------------------
# multinomial (softmax) regression on the K-response sweeps (csrc/zf_kernels_softmax.h)
# ---------------------------------------------------------------------------
def _check_classes(y, m, n_classes=None, weights=None):
    """The targets of a multinomial problem as ``(Y, classes)``: Y a host (m, K) float64 array with rows on the probability simplex,
    ``classes`` the K labels 0 .. K-1.  ``y``: a 1-D integer vector of m labels in 0 .. K-1 (K = max + 1, or ``n_classes``), expanded to
    one-hot rows, or an (m, K) matrix of probabilities - finite, >= 0, every row summing to 1 within 1e-12.  A row whose weight is 0
    is a row that is not there: it is not checked.  ValueError otherwise - on the host, before anything touches the device."""
    host = y.detach().cpu().numpy() if hasattr(y, "detach") else np.asarray(y)
    if np.dtype(host.dtype).kind not in "biuf":
        raise ValueError(f"y must be integer class labels or a matrix of probabilities, got dtype {host.dtype}")
    if n_classes is not None and (int(n_classes) != n_classes or not 2 <= int(n_classes) <= MAX_RESPONSES):
        raise ValueError(f"n_classes must be an integer in 2 .. {MAX_RESPONSES}, got {n_classes!r}")
    there = np.ones(m, dtype=bool) if weights is None else np.asarray(weights) != 0
    if host.ndim == 1:
        if host.shape[0] != m:
            raise ValueError(f"y must hold {m} class labels (one per row of A), got shape {host.shape}")
        if np.dtype(host.dtype).kind not in "biu":
            raise ValueError(f"a 1-D y must be INTEGER class labels 0 .. K-1, got dtype {host.dtype} (probabilities are an (m, K) matrix)")
        lab = host.astype(np.int64)
        if lab.size == 0 or lab.min() < 0:
            raise ValueError("the class labels must be >= 0 (and there must be at least one row)")
        K = int(lab.max()) + 1 if n_classes is None else int(n_classes)
        if lab.max() >= K:
            raise ValueError(f"a class label {int(lab.max())} is outside 0 .. n_classes - 1 = {K - 1}")
        if not 2 <= K <= MAX_RESPONSES:
            raise ValueError(f"the number of classes must be 2 .. {MAX_RESPONSES} (the register tiles of the K-response sweeps), got K = {K}")
        Y = np.zeros((m, K))
        Y[np.arange(m), lab] = 1.0
        return Y, np.arange(K)
    if host.ndim != 2 or host.shape[0] != m:
        raise ValueError(f"y must be {m} class labels or an ({m}, K) matrix of probabilities, got shape {host.shape}")
    K = int(host.shape[1])
    if n_classes is not None and int(n_classes) != K:
        raise ValueError(f"n_classes = {n_classes} but y has {K} columns")
    if not 2 <= K <= MAX_RESPONSES:
        raise ValueError(f"the number of classes must be 2 .. {MAX_RESPONSES} (the register tiles of the K-response sweeps), got K = {K}")
    Y = np.array(host, dtype=np.float64, order="C", copy=True)
    rows = Y[there]
    if not np.all(np.isfinite(rows)) or np.any(rows < 0):
        raise ValueError("the probabilities y must be finite and >= 0")
    if np.any(np.abs(rows.sum(axis=1) - 1.0) > 1e-12):
        raise ValueError("every row of y must sum to 1 (within 1e-12): the loss is logsumexp(z) - <y, z> only on the simplex")
    return Y, np.arange(K)


class _MultinomialMixin:
    r"""Multinomial (softmax) regression on the K-response problem: Y (m, K) with rows on the probability simplex, X (n, K),

        f(X) = scale \sum_i w_i [ logsumexp(z_i) - <y_i, z_i> ],  z_i = (A X)_i,   grad f = scale A^T (w o (softmax(Z) - Y)),

    with the penalty, the flattening (``x[j K + k] = X[j, k]``), the two sweeps and everything element-wise of ``_MultiResponseMixin``;
    only the loss couples the K margins of a row (csrc/zf_kernels_softmax.h).  The problem kind is the least-squares one;
    ``multinomial`` in the descriptor fields makes the engine call ``zf_solver_set_multinomial`` after the responses.  A row has ONE
    weight: ``sample_weight`` is (m,), repeated K times for the library.  2 <= K <= 16.  No screening, no fp32 matrix, no process
    group, no acceptance="remainder" / "resolved", no ``l1_cv_lockstep`` (the responses are taken)."""

    _loss = _lib.ZF_LOSS_MULTINOMIAL
    # The problem kind is the instance's (``_set_multinomial`` copies ``_ls_kind``), the class keeps ``kind = None``: a class-level
    # kind enters a class into the descriptor table of the losses that are a function of ONE margin (tests/test_evaldesc_host.py);
    # the descriptor of these classes is checked in tests/test_multinomial_host.py.
    _ls_kind = None

    def _row_weights(self, w, m):
        """(m,) weights -> the (m, K)-shaped repeat the K-response layer takes; (m, K) and everything else: ValueError."""
        if w is None:
            return None
        return _check_weights(w, m)

    def _set_multinomial(self, A, y, lam, scale, bounds, l2, sample_weight, penalty_factor, n_classes, group, share):
        if group is not None:
            raise ValueError("group= is not available: the multinomial loss kernels, their certificate and zf_solver_set_multinomial "
                             "are built for one GPU (world = 1)")
        self.kind = self._ls_kind
        shape = self._share_shape(share) if share is not None else tuple(getattr(A, "shape", None) or np.shape(A))
        if len(shape) != 2:
            raise ValueError(f"A must be (m, n), got shape {shape}")
        m = int(shape[0])
        w = self._row_weights(sample_weight, m)
        Y, self.classes = _check_classes(y, m, n_classes, w)
        K = Y.shape[1]
        self._set_mr(A, Y, lam, scale, bounds, l2, None if w is None else np.repeat(w.reshape(m, 1), K, axis=1), penalty_factor, share)

    @staticmethod
    def _share_shape(share):
        return tuple(share.A.shape) if hasattr(share, "A") else (share.m_rows, share.n_features)

    @property
    def sample_weight(self):
        """The per-row sample weights, (m,) (a host copy), or None."""
        return None if self._w_host is None else self._w_host.reshape(self._m, self.n_responses)[:, 0].copy()

    def with_sample_weight(self, w):
        """A sibling with the per-row weights ``w`` - (m,) only: a row of this loss has one weight - on the same device matrix and Y.
        The rows of Y with a positive weight must lie on the simplex - with ``None`` every row: ValueError otherwise."""
        w = self._row_weights(w, self._m)   # (None: every row is there again, so every row of Y is checked)
        _check_classes(self.b.detach().cpu().numpy().reshape(self._m, self.n_responses), self._m, None, w)
        return super().with_sample_weight(None if w is None else np.repeat(w.reshape(self._m, 1), self.n_responses, axis=1))

    def predict_proba(self, x, A=None):
        """softmax(A X) -> (rows of A, K), on the host from ``coef(x)`` (a convenience, not a kernel).  ``A``: a host matrix (dense
        or scipy.sparse) with n columns; None: the problem's own matrix, copied from the device."""
        X = self.coef(_as_host(self._flat(x)))
        if A is None:
            A = self._host_matrix()
        Z = np.asarray(A @ X, dtype=np.float64)
        Z = Z - Z.max(axis=1, keepdims=True)
        E = np.exp(Z)
        return E / E.sum(axis=1, keepdims=True)


class MultinomialL1(_MultinomialMixin, _MultiResponseMixin, _DenseMarginsL1):
    r"""L1-regularised multinomial (softmax) regression, A dense row-major: glmnet's ``family="multinomial"``, sklearn's
    ``LogisticRegression(penalty="l1")`` with several classes.  ``y``: m integer class labels 0 .. K-1 (``n_classes=`` when the largest
    does not occur) or an (m, K) matrix of probabilities.  ``coef(x)`` -> (n, K), ``predict_proba(x)`` -> (m, K), ``classes`` the K
    labels; f, jac_f, duality_gap, gap_tol, lam_max, l1_path, snapshots and the siblings as for the K-response classes.
    See ``_MultinomialMixin``."""

    _ls_kind = _lib.ZF_PROBLEM_LEAST_SQUARES_L1

    def __init__(self, A, y, lam, scale=1.0, bounds=None, l2=0.0, *, sample_weight=None, penalty_factor=None, n_classes=None, group=None,
                 _share=None):
        self._set_multinomial(A, y, lam, scale, bounds, l2, sample_weight, penalty_factor, n_classes, group, _share)

    def _host_matrix(self):
        return self.A.detach().cpu().numpy()


class SparseMultinomialL1(_MultinomialMixin, _SparseMultiResponseMixin, _SparseMarginsL1):
    r"""``MultinomialL1`` with a SPARSE A (any scipy.sparse matrix): the handle, plans and sweeps of the sparse K-response classes,
    the loss kernels of the dense class - the rows of the same (m, K) are summed in the same order."""

    _ls_kind = _lib.ZF_PROBLEM_SPARSE_LS_L1

    def __init__(self, A, y, lam, scale=1.0, bounds=None, l2=0.0, *, sample_weight=None, penalty_factor=None, n_classes=None, group=None,
                 _share=None):
        self._set_multinomial(A, y, lam, scale, bounds, l2, sample_weight, penalty_factor, n_classes, group, _share)

    def _host_matrix(self):
        import scipy.sparse as sp

        d = self._spmat.dev
        return sp.csr_matrix((d["data"].cpu().numpy(), d["indices"].cpu().numpy(), d["indptr"].cpu().numpy()), shape=(self._m, self._n))


def _logistic_with_classes(self, y, sample_weight=None, n_classes=None):
    """A ``MultinomialL1`` on this problem's device matrix (shared, nothing but Y is uploaded) with its lam, scale, bounds, l2 and
    penalty factors (repeated for every class).  ``y``: m class labels or (m, K) probabilities; ``sample_weight``: (m,) or None."""
    return _with_responses(self, lambda A, B, *a, **kw: MultinomialL1(A, B, *a, n_classes=n_classes, **kw), y, sample_weight)


def _sparse_logistic_with_classes(self, y, sample_weight=None, n_classes=None):
    """A ``SparseMultinomialL1`` on this problem's matrix handle (the same object; only Y is uploaded) with its lam, scale, bounds,
    l2 and penalty factors (repeated for every class).  ``y``: m class labels or (m, K) probabilities; ``sample_weight``: (m,) or None."""
    return _sparse_with_responses(self, lambda A, B, *a, **kw: SparseMultinomialL1(A, B, *a, n_classes=n_classes, **kw), y, sample_weight)


LogisticL1.with_classes = _logistic_with_classes
SparseLogisticL1.with_classes = _sparse_logistic_with_classes


class BlurHaarL1(NativeProblem):
    r"""Operator-form LASSO: f(x) = scale \|B W^{-1} x - b\|^2,  g(x) = lam \|x\|_1 (+ optional box), with B the
    correlation with ``kernel`` (odd size <= 15, symmetric boundary - ``scipy.signal.correlate2d(..., mode="same",
    boundary="symm")``) and W one orthonormal Haar level (``pywt.dwt2(.., "haar")``, coefficients flattened as
    [cA, cH, cV, cD]): the image-deblurring problem of the reference's ``examples/cameraman.ipynb`` (cells 6-11,
    ``l1_ratio`` = lam, scale = 1).  ``jac_f`` applies B itself as its adjoint, as the notebook does.

    The callbacks keep the notebook's types - ``f`` and ``g`` return arrays of ONE value, ``jac_f`` a (1, n) array
    (m = 1 by zfista/proximal_gradient.py:143) - and so do ``fun`` / ``allfuns`` of a solve.  Handed to
    ``minimize_proximal_gradient`` as its four bound methods, the solve runs device-resident: the Haar levels are
    folded into the tile loads / epilogues of the two correlation kernels (csrc/zf_kernels_op.h), B W^-1 y comes by
    linearity from the cached B W^-1 x_k, B W^-1 x_{k-1}; no host synchronisation per iteration."""

    kind = _lib.ZF_PROBLEM_BLUR_HAAR_L1
    array_valued = True      # f, g -> (1,) arrays; jac_f -> (1, n)

    def __init__(self, kernel, observed, l1_ratio, scale=1.0, bounds=None):
        self.taps = _to_device(kernel, "kernel")
        self.b = _to_device(observed, "observed")
        if self.taps.ndim != 2 or self.taps.shape[0] != self.taps.shape[1] or self.taps.shape[0] % 2 != 1 or self.taps.shape[0] > 15:
            raise ValueError("kernel must be square with an odd size of at most 15")
        if self.b.ndim != 2 or self.b.shape[0] % 2 or self.b.shape[1] % 2:
            raise ValueError("the observed image must be 2-D with even sides")
        if self.taps.shape[0] // 2 >= min(self.b.shape):
            raise ValueError("the kernel is too large for the image")
        self.k = int(self.taps.shape[0])
        self.h, self.w = int(self.b.shape[0]), int(self.b.shape[1])
        self.lam, self.scale = float(l1_ratio), float(scale)
        self.box = (-np.inf, np.inf) if bounds is None else (float(bounds[0]), float(bounds[1]))
        self.n_features = self.h * self.w
        self.group = None

    def _op(self, x, want_grad):
        x = _as_host(x).reshape(-1)
        if x.size != self.n_features:
            raise ValueError(f"len(x) should be equal to n_features, got {x}.")
        lib = _lib.require_gpu()
        fval = C.c_double(0.0)
        grad = np.empty_like(x) if want_grad else None
        _lib.check(lib.zf_op_eval(C.c_void_p(self.taps.data_ptr()), self.k, C.c_void_p(self.b.data_ptr()), self.h, self.w,
                                  self.scale, C.c_void_p(_lib.ptr(x)), C.byref(fval),
                                  C.c_void_p(_lib.ptr(grad)) if want_grad else None), "zf_op_eval")
        return np.float64(fval.value), grad

    def f(self, x):
        return np.array([self._op(x, False)[0]])

    def jac_f(self, x):
        return self._op(x, True)[1].reshape(1, -1)

    def g(self, x):
        return np.array([NativeProblem.g(self, np.asarray(x).reshape(-1))])

    def prox_wsum_g(self, weight, x):
        # (weight is lr - a float - for m = 1, :148; tolerate the 1-element array a caller may pass)
        return NativeProblem.prox_wsum_g(self, float(np.asarray(weight).reshape(-1)[0]), np.asarray(x).reshape(-1))

    def _eval_fg(self, x):
        lib = _lib.require_gpu()
        s = C.c_double(0.0)
        _lib.check(lib.zf_host_asum(C.c_void_p(_lib.ptr(x)), x.size, C.byref(s)), "zf_host_asum")
        return None, np.float64(self.lam * s.value)

    def _descriptor(self):
        fields = dict(kind=self.kind, world=1, rank=0, n=self.n_features, m_rows=self.n_features, row_sharded=0,
                      d=None, c=None, A=None, b=self.b.data_ptr(), scale=self.scale, lam=self.lam,
                      box_lo=self.box[0], box_hi=self.box[1], op_h=self.h, op_w=self.w, op_taps=self.taps.data_ptr(),
                      op_k=self.k)
        return fields, (self.taps, self.b)


def match_native(f, g, jac_f, prox_wsum_g):
    """The NativeProblem whose four bound methods these are, else None."""
    owner = getattr(f, "__self__", None)
    if not isinstance(owner, NativeProblem):
        return None
    want = ("f", "g", "jac_f", "prox_wsum_g")
    for cb, name in zip((f, g, jac_f, prox_wsum_g), want):
        if getattr(cb, "__self__", None) is not owner:
            return None
        if getattr(cb, "__func__", None) is not getattr(type(owner), name):
            return None
    return owner


# ---------------------------------------------------------------------------
# multi-objective problem family of zfista/problems.py (shifted l1 + box)
# ---------------------------------------------------------------------------
class Problem:
    """Mirror of zfista.problems.Problem (problems.py:25-150): F_i = f_i + g_i with
    g_i(x) = l1_ratios[i] * |x - l1_shifts[i]|_1 plus an optional box.

    ``g`` and ``prox_wsum_g`` are NumPy-callable and evaluated on the GPU
    (``zf_mo_eval_F`` / ``zf_mo_prox_host``).  Subclasses with a built-in device
    ``f`` / ``jac_f`` (``JOS1``, ``FDS``) are run by ``minimize_proximal_gradient``
    with everything but SciPy's dual search on the GPU.
    """

    _kind = _lib.ZF_MO_GENERIC

    def __init__(self, n_features, n_objectives, l1_ratios=None, l1_shifts=None, bounds=None, group=None):
        # group (torch.distributed): the decision vector is split over its ranks in contiguous
        # blocks; n_features stays the length of the WHOLE vector, x0 / res.x are this rank's block
        self.group = group
        self.n_features = int(n_features)
        self.n_objectives = int(n_objectives)
        self.l1_ratios = None if l1_ratios is None else np.array(l1_ratios, dtype=np.float64)
        self.l1_shifts = np.zeros(n_objectives) if l1_shifts is None else np.array(l1_shifts, dtype=np.float64)
        self.bounds = bounds   # scalars or per-coordinate arrays of n_features (problems.py:69-70)
        self.name = self._generate_name()
        self._eng = None

    def _generate_name(self):   # problems.py:81-91
        parts = [type(self).__name__, f"n_{self.n_features}"]
        if self.l1_ratios is not None:
            parts.append("l1_ratios_" + "_".join(map(str, self.l1_ratios)))
            parts.append("l1_shifts_" + "_".join(map(str, self.l1_shifts)))
        if self.bounds is not None:
            parts.append("bounds_" + "_".join(map(str, [self.bounds[0], self.bounds[1]])))
        return "_".join(parts)

    def _engine(self):
        from .multiobjective import MoEngine

        if self._eng is None or self._eng.h is None:
            lo, hi = self.shard_bounds()
            arrays = self.bounds is not None and (np.ndim(self.bounds[0]) > 0 or np.ndim(self.bounds[1]) > 0)
            self._eng = MoEngine(self._kind, self.n_objectives, hi - lo, self.l1_ratios,
                                 self.l1_shifts, None if arrays else self.bounds, group=self.group,
                                 n_global=self.n_features, offset=lo)
            if arrays:   # per-coordinate box: this rank's block of each bound vector
                full = [np.broadcast_to(np.asarray(b, dtype=np.float64), (self.n_features,)) for b in self.bounds]
                self._eng.set_bounds(full[0][lo:hi], full[1][lo:hi])
        return self._eng

    def shard_bounds(self):
        """[lo, hi): this rank's block of the decision vector (the whole vector without a group)."""
        if self.group is None:
            return 0, self.n_features
        from .comm import rank_world

        rank, world = rank_world(self.group)
        return rank * self.n_features // world, (rank + 1) * self.n_features // world

    def _check_len(self, x):
        lo, hi = self.shard_bounds()
        if hi - lo != len(x):
            raise ValueError(f"len(x) should be equal to n_features, got {x}.")   # problems.py:102-103

    def g(self, x):
        self._check_len(x)
        eng = self._engine()
        eng.put(2, x)
        return eng.eval_F(2, builtin_f=False)[1]

    def prox_wsum_g(self, weight, x):
        self._check_len(x)
        return self._engine().prox_host(weight, x)

    def f(self, x):
        raise NotImplementedError

    def jac_f(self, x):
        raise NotImplementedError

    def callbacks(self):
        return self.f, self.g, self.jac_f, self.prox_wsum_g

    def minimize_proximal_gradient(self, x0, **kwargs):   # problems.py:140-150
        from .proximal_gradient import minimize_proximal_gradient

        return minimize_proximal_gradient(self.f, self.g, self.jac_f, self.prox_wsum_g, x0, **kwargs)


class _BuiltinProblem(Problem):
    _host_f = False

    def f(self, x):
        self._check_len(x)
        eng = self._engine()
        eng.put(2, x)
        return eng.eval_F(2)[0]

    def jac_f(self, x):
        self._check_len(x)
        eng = self._engine()
        saved = eng.get(1)
        eng.put(1, x)
        eng.prepare()
        J = eng.get_jac()
        eng.put(1, saved)
        return J


class JOS1(_BuiltinProblem):
    """f_1 = |x|^2 / n, f_2 = |x - 2|^2 / n   (zfista/problems.py:153-205)."""

    _kind = _lib.ZF_MO_JOS1

    def __init__(self, n_features=5, l1_ratios=None, l1_shifts=None, bounds=None, group=None):
        super().__init__(n_features, 2, l1_ratios, l1_shifts, bounds, group=group)


class FDS(_BuiltinProblem):
    """Fliege-Drummond-Svaiter test problem, m = 3   (zfista/problems.py:267-328)."""

    _kind = _lib.ZF_MO_FDS

    def __init__(self, n_features=10, l1_ratios=None, l1_shifts=None, bounds=None, group=None):
        super().__init__(n_features, 3, l1_ratios, l1_shifts, bounds, group=group)


# The remaining families of zfista/problems.py have n_features between 3 and 30: their f / jac_f
# are a handful of scalar operations, evaluated on the host (a kernel launch would cost more than
# the arithmetic); g, prox_wsum_g and the solver's own vector work run on the GPU like for every
# Problem.  Each follows the reference's CODE where it differs from its docstring.
class _HostProblem(Problem):
    # f / jac_f are host NumPy; g, prox and every O(n) expression of the dual run in the device
    # engine (multiobjective.solve_native), one host round trip per dual evaluation
    _host_f = True

    def _x(self, x):
        self._check_len(x)
        return np.asarray(x, dtype=np.float64)


class SD(_HostProblem):
    """Stadler-Dauer, n = 4, m = 2, box (1e-6, inf)   (zfista/problems.py:208-264)."""

    def __init__(self):
        super().__init__(4, 2, bounds=(1e-6, np.inf))

    def f(self, x):
        x = self._x(x)
        r2 = np.sqrt(2)
        return np.array([2 * x[0] + r2 * x[1] + r2 * x[2] + x[3],
                         2 / x[0] + 2 * r2 / x[1] + 2 * r2 / x[2] + 2 / x[3]])   # :251 (2 / x_4 as coded)

    def jac_f(self, x):
        x = np.asarray(x, dtype=np.float64)
        r2 = np.sqrt(2)
        return np.vstack((np.array([2, r2, r2, 1]),
                          np.array([-2 / x[0] ** 2, -2 * r2 / x[1] ** 2, -2 * r2 / x[2] ** 2, -2 / x[3] ** 2])))


class ZDT1(_HostProblem):
    """Zitzler-Deb-Thiele 1, m = 2, box (1e-6, inf)   (zfista/problems.py:331-386)."""

    def __init__(self, n_features=30):
        super().__init__(n_features, 2, bounds=(1e-6, np.inf))

    def f(self, x):
        x = self._x(x)
        h = 1 + 9 / (self.n_features - 1) * np.sum(x[1:])
        return np.array([x[0], h * (1 - np.sqrt(x[0] / h))])

    def jac_f(self, x):
        x = self._x(x)
        n = self.n_features
        h = 1 + 9 / (n - 1) * np.sum(x[1:])
        j1 = np.zeros(n)
        j1[0] = 1
        j2 = np.full(n, 9 * (2 - np.sqrt(x[0] / h)) / 2 / (n - 1))   # :381-383 as coded (the derivative)
        j2[0] = -np.sqrt(h / x[0]) / 2
        return np.vstack((j1, j2))


class TOI4(_HostProblem):
    """Toint 4, n = 4, m = 2   (zfista/problems.py:389-448)."""

    def __init__(self, l1_ratios=None, l1_shifts=None, bounds=None):
        super().__init__(4, 2, l1_ratios, l1_shifts, bounds)

    def f(self, x):
        x = self._x(x)
        return np.array([x[0] ** 2 + x[1] ** 2 + 1, 0.5 * ((x[0] - x[1]) ** 2 + (x[2] - x[3]) ** 2) + 1])

    def jac_f(self, x):
        x = self._x(x)
        a, b = x[0] - x[1], x[2] - x[3]
        return np.array([[2 * x[0], 2 * x[1], 0.0, 0.0], [a, -a, b, -b]])


class TRIDIA(_HostProblem):
    """Toint tridiagonal, n = 3, m = 3   (zfista/problems.py:451-514)."""

    def __init__(self, l1_ratios=None, l1_shifts=None, bounds=None):
        super().__init__(3, 3, l1_ratios, l1_shifts, bounds)

    def f(self, x):
        x = self._x(x)
        return np.array([(2 * x[0] - 1) ** 2, 2 * (2 * x[0] - x[1]) ** 2, 3 * (2 * x[1] - x[2]) ** 2])

    def jac_f(self, x):
        x = self._x(x)
        return np.array([[8 * x[0] - 4, 0, 0],
                         [16 * x[0] - 8 * x[1], 4 * x[1] - 8 * x[0], 0],
                         [0, 24 * x[1] - 12 * x[2], 6 * x[2] - 12 * x[1]]], dtype=np.float64)


class LinearFunctionRank1(_HostProblem):
    """f_i = (i <(1..n), x> - 1)^2, i = 1..m   (zfista/problems.py:517-575)."""

    def __init__(self, n_features=10, n_objectives=4, l1_ratios=None, l1_shifts=None, bounds=None):
        super().__init__(n_features, n_objectives, l1_ratios, l1_shifts, bounds)
        self.range_n_objectives = np.arange(1, self.n_objectives + 1)
        self.range_n_features = np.arange(1, self.n_features + 1)

    def f(self, x):
        x = self._x(x)
        return (self.range_n_objectives * np.inner(self.range_n_features, x) - 1) ** 2

    def jac_f(self, x):
        x = self._x(x)
        i = self.range_n_objectives[:, None]
        return 2 * i * self.range_n_features * (i * np.inner(self.range_n_features, x) - 1)


def match_native_multi(f, g, jac_f, prox_wsum_g):
    """The built-in multi-objective Problem whose four bound methods these are, else None."""
    owner = getattr(f, "__self__", None)
    if not isinstance(owner, (_BuiltinProblem, _HostProblem)):
        return None
    for cb, name in zip((f, g, jac_f, prox_wsum_g), ("f", "g", "jac_f", "prox_wsum_g")):
        if getattr(cb, "__self__", None) is not owner:
            return None
        if getattr(cb, "__func__", None) is not getattr(type(owner), name):
            return None
    return owner
