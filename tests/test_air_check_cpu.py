"""CPU side of the generic trace-domain assertion (include/bfhip.h: bfhip_air_check / bfhip_format_air_check): the report has one layout in
the header, the ctypes mirror and the generated Rust; the report's text; and the numpy reference the GPU tests compare the kernel with
(tests/air_check_model.py) is anchored to the CPU oracle's AssertEvaluator on the 13 Brainfuck programs. Its one-pass form is pinned to the
per-constraint one, and the cases of tests/air_check_cases.py are shown, on the model alone, to contain what
tests/test_gpu_air_check_edges.py runs them for; the host evaluator agrees with the model on the identity programs."""
import ctypes
import os
import re

import numpy as np
import pytest

import air_check_cases as cases
import air_check_model
import air_model
import oracle_air_check
import pcs_replay
from air_model import C_BASE, C_EXT
from conftest import ROOT, P, splitmix_column

NO_CELL = (1 << 64) - 1
PROGRAM = ("+>,<[>+.<-]", b"\x01")            # memory/component.rs:163-209
ELEMS = [5, 1, 2, 3, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83]      # tests/test_trace_check_cpu.py
N_CONSTRAINTS = [12, 11, 5, 10, 9, 9, 7, 7, 8, 8, 8, 7, 2]
OFFSETS = {"log_size": 0, "n_constraints": 4, "n_bad_cells": 8, "first_bad_cell": 16, "first_bad_constraint": 24, "reserved0": 28, "first_bad_value": 32,
           "bad_per_constraint": 48, "first_cell_per_constraint": 560, "reserved": 1072}


def test_report_and_entry_points_are_declared_in_header_ctypes_and_rust(pkg):
    header = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    assert re.search(r"int32_t bfhip_air_check\(bfhip_ctx\* ctx, const bfhip_air\* air, uint32_t log_size,", header)
    assert re.search(r"int32_t bfhip_format_air_check\(const bfhip_air_check_report\* rep, char\* buf, size_t cap, size_t\* need\);", header)
    body = re.search(r"typedef struct bfhip_air_check_report \{(.*?)\} bfhip_air_check_report;", header, re.S).group(1)
    declared = [name for name in re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body))]
    R = pkg.AirCheckReport
    assert declared == [n for n, _ in R._fields_] == list(OFFSETS)
    assert ctypes.sizeof(R) == 1088 and {n: getattr(R, n).offset for n, _ in R._fields_} == OFFSETS
    assert "1088 bytes" in header and all("%s %d" % (n, o) in header for n, o in OFFSETS.items())      # the header states the layout
    rust = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    assert "pub fn bfhip_air_check(" in rust and "pub fn bfhip_format_air_check(" in rust and "pub struct BfhipAirCheckReport" in rust
    L = pkg.lib()
    assert L.bfhip_air_check and L.bfhip_format_air_check


def _report(pkg, log_size, n_constraints, failing=(), first=None):
    """failing: (constraint, cells, first cell); first: (cell, constraint, value) of the overall first violation"""
    r = pkg.AirCheckReport()
    r.log_size, r.n_constraints = log_size, n_constraints
    r.first_bad_cell, r.first_bad_constraint = NO_CELL, -1
    for j in range(64):
        r.first_cell_per_constraint[j] = NO_CELL
    for j, cells, cell in failing:
        r.bad_per_constraint[j], r.first_cell_per_constraint[j] = cells, cell
    if first is not None:
        r.first_bad_cell, r.first_bad_constraint = first[0], first[1]
        for w in range(4):
            r.first_bad_value[w] = first[2][w]
    return r


def test_format_air_check(pkg):
    clean = _report(pkg, 6, 5)
    assert pkg.format_air_check(clean) == "air check: ok"
    assert clean.as_dict()["ok"] and clean.as_dict()["first_bad_cell"] is None and clean.as_dict()["first_cell_per_constraint"] == [None] * 5
    one = _report(pkg, 7, 5, [(2, 3, 17)], (17, 2, [9, 0, 0, 0]))
    one.n_bad_cells = 3
    assert pkg.format_air_check(one) == "air check: 3 of 128 cells violate 1 of 5 constraints\nconstraint 2: 3 cells, first at cell 17, value (9, 0, 0, 0)"
    two = _report(pkg, 10, 64, [(4, 7, 900), (63, 2, 5)], (5, 63, [1, 2, 3, P - 1]))
    two.n_bad_cells = 9
    text = "air check: 9 of 1024 cells violate 2 of 64 constraints\nconstraint 4: 7 cells, first at cell 900\nconstraint 63: 2 cells, first at cell 5, value (1, 2, 3, %d)" % (P - 1)
    assert pkg.format_air_check(two) == text
    assert two.as_dict()["first_cell_per_constraint"][63] == 5 and two.as_dict()["bad_per_constraint"][4] == 7
    # the size query, and a short buffer: -2 with a NUL-terminated prefix
    L, need = pkg.lib(), ctypes.c_size_t()
    assert L.bfhip_format_air_check(ctypes.byref(two), None, ctypes.c_size_t(0), ctypes.byref(need)) == -2 and need.value == len(text) + 1
    assert L.bfhip_last_error().decode() == "capacity"
    buf = ctypes.create_string_buffer(b"\xff" * 32, 32)
    assert L.bfhip_format_air_check(ctypes.byref(two), buf, ctypes.c_size_t(20), ctypes.byref(need)) == -2 and need.value == len(text) + 1
    assert buf.raw[:20] == text[:19].encode() + b"\0" and buf.raw[20:] == b"\xff" * 12
    exact = ctypes.create_string_buffer(len(text) + 1)
    assert L.bfhip_format_air_check(ctypes.byref(two), exact, ctypes.c_size_t(len(text) + 1), None) == 0 and exact.value.decode() == text
    assert L.bfhip_format_air_check(None, exact, ctypes.c_size_t(8), None) == -1 and "null" in L.bfhip_last_error().decode()


@pytest.fixture(scope="module")
def oracle_check(tmp_path_factory):
    return oracle_air_check.build(tmp_path_factory.mktemp("oracle_air_check"))


def program_columns(rows, inter):
    """The columns of brainfuck_air_program in its order, full size: main (each row 16 times), logUp coordinates, IsFirst = [cell == 0]."""
    n = 16 * rows.shape[1]
    is_first = np.zeros((1, n), dtype=np.uint32); is_first[0, 0] = 1
    return np.concatenate([np.repeat(rows, 16, axis=1), inter, is_first])


@pytest.mark.parametrize("comp", range(13))
def test_numpy_model_reproduces_the_oracle_on_the_brainfuck_programs(pkg, _oracle, oracle_check, comp):
    """The anchor of the GPU tests' reference: for each of the 13 programs the model gives the per-constraint counts, the first bad cell and
    the first bad constraint and value of the oracle's AssertEvaluator looped over every cell — on a valid trace, with one main cell changed
    and with one interaction cell changed. (It passes without bfhip_air_check: nothing here calls it.)"""
    program, _, _ = pkg.brainfuck_air_program(comp)
    k = N_CONSTRAINTS[comp]
    assert program.shape["n_constraints"] == k == air_check_model.n_constraints_of(program.code)
    rows = np.ascontiguousarray(_oracle.table(*PROGRAM, comp).T)
    n_main, M = rows.shape
    log_size = int(np.log2(M)) + 4
    inter, claimed = _oracle.logup_generate(comp, rows, ELEMS)
    params = pkg.brainfuck_air_params(ELEMS, claimed)
    bad_rows = rows.copy()
    bad_rows[(3 * comp + 1) % n_main, (5 * comp + 2) % M] = (int(bad_rows[(3 * comp + 1) % n_main, (5 * comp + 2) % M]) + 1) % P
    bad_inter = inter.copy()
    cell = (37 * comp + 11) % (16 * M)
    bad_inter[inter.shape[0] - 4 + comp % 4, cell] = (int(bad_inter[inter.shape[0] - 4 + comp % 4, cell]) + 1) % P
    seen = []
    for tag, r, it in (("valid", rows, inter), ("main cell", bad_rows, inter), ("interaction cell", rows, bad_inter)):
        want = oracle_check.check(comp, r, ELEMS, inter=it, claimed=claimed)
        got = air_check_model.report(program.code, program_columns(r, it), params, log_size)
        print(comp, tag, {f: got[f] for f in air_check_model.FIELDS})
        assert air_check_model.report_one_pass(program.code, program_columns(r, it), params, log_size) == got      # the one-pass path: the same anchor
        assert got["bad_per_constraint"] == want["bad_per_constraint"][:k] and not any(want["bad_per_constraint"][k:])
        assert (got["n_bad_cells"], got["first_bad_cell"], got["first_bad_constraint"], got["first_bad_value"]) == (
            want["n_bad_cells"], want["first_bad_cell"], want["first_bad_constraint"], want["first_bad_value"])
        assert got["first_cell_per_constraint"][got["first_bad_constraint"]] == got["first_bad_cell"] if got["n_bad_cells"] else got["first_cell_per_constraint"] == [None] * k
        seen.append(got["n_bad_cells"])
    assert seen[0] == 0 and seen[2] == 2      # a last-column cell breaks the last logUp constraint at the cell and at its coset successor


# ---- the one-pass model, and what the cases of tests/test_gpu_air_check_edges.py contain (tests/air_check_cases.py) -----------------------------
@pytest.mark.parametrize("log_size", [1, 2, 5, 6, 7, 10])
@pytest.mark.parametrize("seed", [4, 34])
def test_one_pass_model_equals_the_model_run_per_constraint(seed, log_size):
    """air_check_model.one_pass against report() — a run per constraint under a one-hot coefficient — on the random programs and columns
    of tests/test_gpu_air_check.py's seeds (the same generator calls), every field; the bad matrix adds up to the report's counts."""
    code, n_cols, n_params, _ = air_model.random_program(seed, n_cols=14, n_ops=150, max_off=16, max_cons=64)
    n = 1 << log_size
    full = np.stack([splitmix_column((seed << 8) + 16 * log_size + k, n) for k in range(n_cols)])
    params = splitmix_column(seed + 1000, 4 * n_params).reshape(n_params, 4).tolist()
    for cols in (full, np.where(splitmix_column(seed, n) % np.uint32(3) == 0, full, np.uint32(0))):      # all bad; two cells in three zeroed
        want = air_check_model.report(code, cols, params, log_size)
        got, bad = air_check_model.one_pass(code, cols, params, log_size)
        assert got == want
        assert bad.shape == (want["n_constraints"], n) and bad.sum(axis=1).tolist() == want["bad_per_constraint"]
        assert int(bad.any(axis=0).sum()) == want["n_bad_cells"]
    assert want["n_constraints"] in (34, 29)


@pytest.mark.parametrize("log_size", [6, 7, 10])
def test_defect_cases_hold_the_ballots_they_were_built_for(log_size):
    """In the model alone: 64 interleaved constraints over both halves of the lane mask; within single waves a constraint fails at exactly
    1, 2, 33, 63 and 64 cells while another fails at none; lowest failing lanes that differ between constraints and from the wave's lowest
    bad lane; first cells in wave 0 and in the last wave; the cells 63, 64 and n - 1. And the closed form that needs no interpreter."""
    case = cases.defect_case(log_size)
    cases.assert_defect_conditions(case)
    counts, firsts = cases.defect_closed_form(case)
    print(log_size, {f: case.want[f] for f in air_check_model.FIELDS})
    assert case.want["bad_per_constraint"] == counts and case.want["first_cell_per_constraint"] == firsts
    if log_size < 10:
        assert air_check_model.report(case.code, case.full, case.params, log_size) == case.want


def test_defect_case_of_two_to_the_20_cells():
    case = cases.defect_case_big()
    want, n = case.want, 1 << cases.BIG_LOG
    print({f: want[f] for f in air_check_model.FIELDS})
    assert (want["bad_per_constraint"], want["first_cell_per_constraint"]) == cases.defect_closed_form(case)
    assert want["bad_per_constraint"] == [len(cells) for _, _, cells in cases.BIG_SPEC] == [1, 3, 2, 3, 0, 2]
    assert want["first_cell_per_constraint"] == [min(cells) if cells else None for _, _, cells in cases.BIG_SPEC]
    assert want["first_cell_per_constraint"][0] >= n - 64                                  # the only defect of constraint 0: in the last wave
    assert want["first_bad_cell"] == 65600 > 1 << 16 and want["first_bad_constraint"] == 2 and want["n_bad_cells"] == 10
    assert want["n_constraints"] == 6 <= 8 and set(case.kinds()) == {C_BASE, C_EXT}


@pytest.mark.parametrize("log_size", [1, 5, 6, 7])
def test_caps_case_is_at_the_caps_and_every_constraint_fails(pkg, log_size):
    case = cases.caps_case(log_size)
    shape = pkg.AirProgram(case.code, case.n_cols, case.n_params).shape
    assert (shape["m_regs"], shape["q_regs"], shape["n_instr"], shape["n_constraints"]) == (96, 24, 4096, 64), shape
    assert (shape["min_offset"], shape["max_offset"]) == (-16, 16) and 4 * 64 * (96 + 4 * 24) == 49152      # bytes of LDS per wave
    kinds = case.kinds()
    assert C_BASE in kinds and C_EXT in kinds and any(a != b for a, b in zip(kinds, kinds[1:]))
    assert min(case.want["bad_per_constraint"]) > 0      # every constraint fails somewhere: 2 * 64 + 2 atomics in a wave


@pytest.mark.parametrize("which", list(cases.ONE_FILE))
def test_one_file_cases_have_partial_ballots(pkg, which):
    for log_size in (6, 7):
        case = cases.one_file_case(which, log_size)
        shape = pkg.AirProgram(case.code, case.n_cols, case.n_params).shape
        assert (shape["m_regs"], shape["q_regs"]) == ((96, 0) if which == "no_q" else (0, 24))
        assert all(0 < b < 1 << log_size for b in case.want["bad_per_constraint"]) and case.want["n_bad_cells"] < sum(case.want["bad_per_constraint"])


@pytest.mark.parametrize("log_size", [4, 9])
def test_shift_cases_fail_inside_shift_groups(log_size):
    cases.assert_shift_conditions(cases.shift_case(log_size))


@pytest.mark.parametrize("family", cases.IDENTITY_FAMILIES)
def test_identities_are_ok_in_the_model_and_their_twins_fail_everywhere(family):
    case = cases.identity_case(family)
    kinds = case.notes["kinds"]
    assert len(kinds) == 20 and kinds.count(C_BASE) == 10 and case.kinds() == kinds
    assert case.want["n_bad_cells"] == 0 and case.want["first_bad_constraint"] == -1 and not case.bad.any()
    assert all(q == [P - 1] * 4 for q in case.params[:2])
    if family == "max":
        assert np.all(case.full == P - 1)
    for twin in (4, 17):
        assert kinds[twin] == (C_BASE if twin == 4 else C_EXT)
        t = cases.identity_case(family, twin)
        assert t.want == cases.twin_report(t) and t.want["n_bad_cells"] == 1 << t.log_size
        assert t.want["first_bad_value"] == ([1, 0, 0, 0] if twin == 4 else [0, 0, 0, 1])


def test_complement_columns_sum_to_exactly_p():
    case = cases.complement_case()
    full = case.full.astype(np.int64)
    for u, v in [(cases.A, cases.B)] + [(cases.X + k, cases.Y + k) for k in range(4)]:
        s = full[u] + full[v]
        assert set(np.unique(s).tolist()) <= {0, P} and np.count_nonzero(s == P) > full.shape[1] // 2
    assert case.want["n_bad_cells"] == 0
    assert cases.identity_case("complement").want["n_bad_cells"] == 0


def test_one_coordinate_and_first_constraint_cases_equal_their_closed_forms():
    for lowest in range(4):
        case = cases.one_coordinate_case(lowest)
        assert case.want == case.notes["report"] and sum(1 for w in case.want["first_bad_value"] if w) == 1 and case.want["first_bad_value"][lowest]
    for kind in (C_EXT, C_BASE):
        case = cases.first_constraint_case(kind)
        assert case.want == case.notes["report"] and case.kinds()[cases.FIRST_CONSTRAINT] == kind
        assert case.want["first_bad_constraint"] == 41 and case.want["bad_per_constraint"][0] == 1 and not case.bad[:41, cases.FIRST_CELL].any()
        assert case.bad[42:, cases.FIRST_CELL].all()      # later constraints fail at the first bad cell too


@pytest.mark.parametrize("family", ["max", "edge", "complement"])
def test_host_evaluator_agrees_with_the_model_on_the_identity_programs(pkg, family):
    """bfhip_air_eval_at_point (C++, shares no code with the model or the kernel) times the vanishing polynomial against air_model.run at
    n = 1, the mask values being a cell's own column values: zero for the identities under any coefficients, the coefficient of the twin
    times its one for the twins."""
    ch = pkg.Channel((0, 0, 0, 0))
    ch.mix_u64(41)
    point = ch.draw_point()
    van = air_model.coset_vanishing(cases.IDENTITY_LOG, point)
    for twin in (None, 4, 17):
        case = cases.identity_case(family, twin)
        prog = pkg.AirProgram(case.code, case.n_cols, case.n_params)
        coeffs = splitmix_column(900, 4 * 20).reshape(20, 4).tolist()
        for cell in (0, 1, 126, 127):
            mask = prog.mask()
            assert all(off == 0 for _, off in mask)
            values = [[int(case.full[col, cell]), 0, 0, 0] for col, _ in mask]
            got = pcs_replay.q_mul(prog.eval_at_point(case.log_size, point, values, case.params, coeffs), van)
            at = {m: air_model.q(v) for m, v in zip(mask, values)}
            model = [int(w) for w in air_model.run(case.code, lambda col, off: at[(col, off)], case.params, coeffs)[:, 0]]
            want = [0, 0, 0, 0] if twin is None else coeffs[twin] if twin == 4 else pcs_replay.q_mul(coeffs[twin], [0, 0, 0, 1])
            assert got == model == want, (family, twin, cell)
