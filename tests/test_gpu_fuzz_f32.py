"""GPU: the option sweep of tests/f32_fuzz_cases.py on the four dense margins classes with the matrix stored in fp32
(``matrix_dtype="float32"``; LogisticL1 through ``with_matrix_dtype``, before or after its other siblings) - every loss at every
load width of csrc/zf_kernels_gemv_f32.h (V4, V2, V1), with per-row weights (real and 0 / 1 fold masks), per-column penalty
factors, the box, the elastic-net l2, starts outside the box, decay rates 0.3 / 0.5 / 0.9 / 1, ``deprecated``, runs of 1 or 2
iterations, runs ended by tol and by "Backtracking failed", and on 40000 rows - against the CPU oracle on the reference closures
over A64 = float64(float32(A)).

tests/test_f32_fuzz_cases.py has shown on the CPU that the oracle's decisions on every case of the fixed table do not depend on
the summation order, so a mismatch here is a finding about the product.  One test id is one case.  The checks are those of
tests/test_gpu_fuzz_margins.py (``_check_storage``, TOL = 1e-10, unchanged) and the three of
tests/test_gpu_fuzz_margins_ext.py (``_extra_checks``: another sub_iters bit for bit, the columns with p_j = 0, NaN in b on
zero-weight rows).  Each case also asserts the whole ls_plan it claims - the fp32 column and row forms, the slices and the rows per
slice - and that the problem's matrix is a float32 tensor: a path that silently kept the fp64 matrix fails there, not on a
tolerance.

ZF_FUZZ_SCALE=k appends k - 1 further blocks of seeds (a one-off soak), each case filtered by the CPU criteria while the ids are
collected."""
import os

import pytest

import f32_fuzz_cases as XF
from test_gpu_fuzz_margins import TOL, _check_resume, _check_storage, default_switches, solve   # noqa: F401 (fixtures)
from test_gpu_fuzz_margins_ext import _extra_checks

pytestmark = pytest.mark.gpu

assert TOL == 1e-10
SCALE = int(os.environ.get("ZF_FUZZ_SCALE", "1"))
TABLE = XF.TABLE + [c for k in range(1, SCALE) for c in XF.extra_block(k)]
SPECS = [XF.draw(loss, seed) for loss, seed in TABLE]


def _is_f32(prob, spec):
    import torch

    m, n = spec.shape[:2]
    assert prob.matrix_dtype == "float32" and prob.A.dtype == torch.float32 and tuple(prob.A.shape) == (m, n)
    assert prob._descriptor()[0]["matrix_f32"] == prob.A.data_ptr()


@pytest.mark.parametrize("spec", SPECS, ids=[XF.case_id(sp) for sp in SPECS])
def test_fuzz_f32(spec, solve):
    case, o, exp, _ = XF.oracle(spec)
    assert exp is not None
    kept = {}
    _check_storage(case, "dense", o, exp, solve, cases=XF, keep=kept)
    assert tuple(kept["plan"]) == XF.plan(spec), (kept["plan"], XF.plan(spec))
    _is_f32(kept["prob"], spec)
    _extra_checks(case, "dense", o, exp, solve, kept)


RESUME = XF.resume_cases()


@pytest.mark.parametrize("spec,kind", RESUME, ids=[f"{sp.loss}-{kind}-s{sp.seed:02d}" for sp, kind in RESUME])
def test_snapshot_resume_across_the_last_chunk(spec, kind, tmp_path):
    """The table's longest run of the loss that ends by tol, and its longest that ends in the error path: a snapshot taken one
    chunk before the end, and the run resumed from it, end with the status, x and trace of the uninterrupted run."""
    case, o, exp, _ = XF.oracle(spec)
    _is_f32(XF.make_problem(case), spec)
    _check_resume(case, o, exp, kind, tmp_path, cases=XF)
