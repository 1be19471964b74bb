"""CPU side of the generic trace-domain assertion (include/bfhip.h: bfhip_air_check / bfhip_format_air_check): the report has one layout in
the header, the ctypes mirror and the generated Rust; the report's text; and the numpy reference the GPU tests compare the kernel with
(tests/air_check_model.py) is anchored to the CPU oracle's AssertEvaluator on the 13 Brainfuck programs."""
import ctypes
import os
import re

import numpy as np
import pytest

import air_check_model
import oracle_air_check
from conftest import ROOT, P

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
        assert got["bad_per_constraint"] == want["bad_per_constraint"][:k] and not any(want["bad_per_constraint"][k:])
        assert (got["n_bad_cells"], got["first_bad_cell"], got["first_bad_constraint"], got["first_bad_value"]) == (
            want["n_bad_cells"], want["first_bad_cell"], want["first_bad_constraint"], want["first_bad_value"])
        assert got["first_cell_per_constraint"][got["first_bad_constraint"]] == got["first_bad_cell"] if got["n_bad_cells"] else got["first_cell_per_constraint"] == [None] * k
        seen.append(got["n_bad_cells"])
    assert seen[0] == 0 and seen[2] == 2      # a last-column cell breaks the last logUp constraint at the cell and at its coset successor
