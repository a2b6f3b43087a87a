"""CPU: the rule table of a margins solver's options (zfista_amd/csrc/zf_solver_options.h - plain C++, compiled here with g++)
against the return codes the PARENT commit's library gave on an MI355X (tests/golden/solver_options_parent.jsonl; the sequences:
tests/solver_options_cases.py), and against the compatibility table in the comment of include/zfista_hip.h.  No device."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import solver_options_cases as S
from conftest import ROOT

PTR = {0: 0, 1: 0x1000, 2: 0x1008}   # NULL, aligned, offset by 8 bytes


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("optcpp") / "libsolver_options_host.so"
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "solver_options_host.cpp"),
                    "-o", str(out)], check=True)
    L = C.CDLL(str(out))
    L.solver_options_apply.restype = C.c_int
    L.solver_options_apply.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                       C.c_int, C.c_double, C.c_uint64, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    return L


@pytest.fixture(scope="module")
def golden():
    return S.load_golden()[1]


def replay_args(entry):
    """(the base's arguments of solver_options_apply, [(option, value, pointer, K, recorded code, small-matrix path open afterwards or -1)])"""
    _, base, init, calls, want = entry
    B = S.BASES[base]
    dense = B["kind"] in (2, 5)
    head = (B["kind"], B["world"], B["accept"], int(init), B["m_rows"], B["n"], 0x2000 + B["b_off"], int(dense and want[0][0] == 1), B["K0"])
    rows = []
    for call, (rc, plan) in zip(calls, want[1:]):
        opt, value, ptr, K = S.decode(call)
        rows.append((opt, value, PTR[ptr], K, rc, int(plan[0] == 1) if dense else -1))
    return head, rows


def present_after(base, calls, codes):
    """per call: the set of options present BEFORE it (K of the sparse creator; an accepted l2 = 0 sets nothing)"""
    have, out = ({"K"} if S.BASES[base]["K0"] else set()), []
    for call, rc in zip(calls, codes):
        out.append(set(have))
        if rc == 0 and call != "l2=0":
            have.add(S.option_of(call))
    return out


def test_the_golden_file_holds_the_sequences_of_the_cases_module(golden):
    assert [e[:4] for e in golden] == [list(e) for e in S.entries()]
    assert len(golden) == 12 * 81 + 8 * 7 * 6 + 9 + 2 + len(S.BAD) + 1


def test_the_rule_table_gives_the_parents_return_codes(lib, golden):
    record = C.create_string_buffer(256)
    msg = C.create_string_buffer(400)
    small = C.c_int(-1)
    for entry in golden:
        head, rows = replay_args(entry)
        small.value = head[7]
        for i, (opt, value, ptr, K, rc_want, small_want) in enumerate(rows):
            head = head[:7] + (small.value,) + head[8:]   # (the path is open for a call if it still was after the one before)
            rc = lib.solver_options_apply(*head, record, int(i == 0), opt, value, ptr, K, msg, 400, C.byref(small))
            assert rc == rc_want, (entry[:4], i, rc, msg.value)
            assert small_want < 0 or small.value == small_want, (entry[:4], i, "zf_options_small_open against zf_solver_ls_plan()[0] == 1")
            if rc != 0:
                assert S.ENTRY[S.OPTIONS[opt]].encode() in msg.value, "a refusal names its entry"


def header_table():
    """{(row, column): cell} of the options-by-options table in the comment of include/zfista_hip.h"""
    text = open(os.path.join(ROOT, "include", "zfista_hip.h")).read()
    block = text[text.index("options by options"):]
    lines = block.splitlines()[1:]
    cols = lines[0].lstrip(" *").split()
    names = dict(zip(("l2", "penalty_factors", "huber", "poisson", "multinomial", "row_weights", "matrix_f32", "responses"), S.OPTIONS))
    assert [names[c] for c in cols] == list(S.OPTIONS)
    cells = {}
    for line in lines[1:9]:
        row, *marks = line.lstrip(" *").split()
        assert len(marks) == 8, line
        cells.update({(names[row], names[c]): m for c, m in zip(cols, marks)})
    return cells


def test_the_table_is_no_vacuous_check_and_agrees_with_the_header(golden):
    codes, accepted_second, refused_second = set(), set(), set()
    refused_with, accepted_with = set(), set()   # (option present, option called)
    for _, base, init, calls, want in golden:
        rcs = [rc for rc, _ in want[1:]]
        codes.update(rcs)
        for i, (call, rc, have) in enumerate(zip(calls, rcs, present_after(base, calls, rcs))):
            name = S.option_of(call)
            if i >= 1:
                (accepted_second if rc == 0 else refused_second).add(name)
            if init or call == "l2=0":
                continue
            for other in have:
                (accepted_with if rc == 0 else refused_with).add((other, name))
    assert codes == {0, -2, -3}
    assert accepted_second == set(S.OPTIONS) and refused_second == set(S.OPTIONS)
    cells = header_table()
    for (a, b), mark in cells.items():
        assert mark in ("x", "+", "o", "2") and mark == cells[b, a], (a, b, mark)
        if a == b:   # a second call: refused, or replaces the value
            assert mark in ("x", "2") and ((a, a) in refused_with) == (mark == "x") and ((a, a) in accepted_with) == (mark == "2"), (a, mark)
        elif mark == "x":
            assert (a, b) in refused_with and (b, a) in refused_with and (a, b) not in accepted_with and (b, a) not in accepted_with, (a, b)
        elif mark == "+":
            assert (a, b) in accepted_with and (b, a) in accepted_with, (a, b)
    # the one ordering rule: the multinomial loss after the responses, never before
    assert cells["multinomial", "K"] == "o" and ("K", "multinomial") in accepted_with and ("multinomial", "K") not in accepted_with


def test_the_shared_predicates_give_the_verdict_of_the_evaluation_entries(lib):
    """zf_desc_args (zf_margins_eval / _gap / _screen) refuses: K > 1 with a loss other than square, logistic, multinomial; the
    multinomial loss with K < 2 or a matrix stored in fp32; K > 1 on a matrix stored in fp32."""
    lib.solver_options_verdict.restype = C.c_int
    for loss in range(5):
        for K in range(1, 17):
            for f32 in (0, 1):
                r1 = K > 1 and loss not in (0, 1, 4)
                r2 = loss == 4 and (K < 2 or f32)
                r3 = K > 1 and f32
                got = lib.solver_options_verdict(loss, K, f32)
                assert bool(got & 1) == (loss in (0, 1, 4)) and bool(got & 2) == (K >= 2 and not f32) and bool(got & 4) == (not r3)
                assert bool(got & 8) == (not (r1 or r2 or r3)), (loss, K, f32)
