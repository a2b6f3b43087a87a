"""A ``zf_eval_desc`` from keyword fields, and the three evaluation entries called with it: what the host tests of the argument
checks share (no test in here).  A call reads as the old positional ones did: ``E.gap(E.dense(P, l2=bad), P, P, 10)``."""
import ctypes as C

from zfista_amd import _lib


def _raw(v):
    return v.value if isinstance(v, C.c_void_p) else v


def desc(**fields):
    """An EvalDesc with scale = 0.5, lam = 0.1, the squared loss and K = 1; every other field zero / NULL unless given."""
    d = _lib.EvalDesc(scale=0.5, lam=0.1, loss=_lib.ZF_LOSS_SQUARE, K=1)
    for name, v in fields.items():
        setattr(d, name, _raw(v))
    return d


def dense(P, **fields):
    """A 3 x 2 fp64 matrix at P with b at P (P: any 16-byte aligned host address - nothing may read through it)."""
    return desc(**{**dict(A=P, b=P, m_rows=3, n=2), **fields})


def dense32(P, **fields):
    return desc(**{**dict(A32=P, b=P, m_rows=3, n=2), **fields})


def sparse(P, **fields):
    """A handle at P with b at P (nothing may read through either)."""
    return desc(**{**dict(spmat=P, b=P), **fields})


def point(d, x, f, grad=None, desc_bytes=None):
    return _lib.load().zf_margins_eval(C.byref(d), C.sizeof(d) if desc_bytes is None else desc_bytes, x, f, grad)


def gap(d, x, out, count, desc_bytes=None):
    return _lib.load().zf_margins_gap(C.byref(d), C.sizeof(d) if desc_bytes is None else desc_bytes, x, out, count)


def screen(d, x, out, count, norms, stats, max_row, max_col, keep, index, desc_bytes=None):
    return _lib.load().zf_margins_screen(C.byref(d), C.sizeof(d) if desc_bytes is None else desc_bytes, x, out, count, norms, stats,
                                         max_row, max_col, keep, index)
