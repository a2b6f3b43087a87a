"""GPU: the eight zf_solver_set_* entries against what the PARENT commit's library answered (tests/golden/solver_options_parent.jsonl,
recorded by tests/golden/make_solver_options_parent.py; tests/solver_options_cases.py lists the sequences).

Every entry is replayed against the built library: the plan at creation, then the return code and the six values of
zf_solver_ls_plan after every call - and a refused call leaves the plan as it was.  No solve is run; an id creates some hundred
solvers on zero-filled buffers and launches nothing beyond the memsets of zf_solver_create (after-init: the initial evaluation of
nine 64 x 64 solvers).  One id per base of the 81 ordered pairs of the nine option values, one for the ordered triples on the dense
least-squares base, one for calls after zf_solver_enqueue_init, one for the slab regrow and the refused arguments.

Time per id on an MI355X: 0.01 - 0.11 s (the triples: 0.11 s, 336 sequences; a base of pairs: 0.02 - 0.10 s, 81 sequences), and 1.8 s
once for the module's buffers and the four CSR handles.
"""
import pytest

import solver_options_cases as S

GROUPS = S.PAIR_BASES + ("triples", "after-init", "regrow-and-bad-arguments")


@pytest.fixture(scope="module")
def driver():
    return S.Driver()


@pytest.fixture(scope="module")
def golden():
    head, recorded = S.load_golden()
    assert [e[:4] for e in recorded] == [list(e) for e in S.entries()], "the golden file holds other sequences than solver_options_cases.entries()"
    return recorded


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_the_setters_answer_as_the_parent_did(group, driver, golden):
    mine = [e for e in golden if e[0] == group]
    assert mine
    for _, base, init, calls, want in mine:
        got = driver.run(base, init, calls)
        assert got == want, (base, init, calls, got, want)
        if base == "dense-ls":
            assert got[0][0] == 1, "the base of the fused small-matrix path must start on it"
        before = got[0]
        for call, (rc, plan) in zip(calls, got[1:]):
            if rc != 0:
                assert plan == before, (base, calls, call, "a refused call must leave the plan as it was")
            before = plan
