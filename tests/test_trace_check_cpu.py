"""CPU side of the trace-domain constraint check (include/bfhip.h: bfhip_check_constraints / bfhip_trace_check): the shim that gives the
oracle's AssertEvaluator a FULL report (tests/native/oracle_air_check.cpp) is pinned against the reference's own negative cases and against
the oracle's first-failure entry point, and `bfhip_check_report` has one layout in the header, the ctypes mirror and the generated Rust."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_air_check
from conftest import ROOT
from oracle_air_check import table_from_registers

V = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")))
ELEMS = [5, 1, 2, 3, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83]      # drawn elements (dummy ones give a zero denominator)
PROGRAM = ("+>,<[>+.<-]", b"\x01")            # memory/component.rs:163-209


@pytest.fixture(scope="module")
def air_check(tmp_path_factory):
    return oracle_air_check.build(tmp_path_factory.mktemp("oracle_air_check"))


@pytest.mark.single_conv
@pytest.mark.parametrize("v", V["air_negative"], ids=lambda v: v["cite"].split("(")[1].split(":")[0].split(")")[0])
def test_shim_reproduces_the_negative_cases_of_the_reference(oracle, air_check, v):
    """memory/component.rs:211-609: table row, constraint and value of the reference's panic text — and the shim's counters are consistent."""
    rows = table_from_registers(oracle, v["trace"], [43], v["component"])
    for r, c, val in v["patch"]:
        rows[r, c] = val
    rep = air_check.check(v["component"], rows.T, ELEMS)
    assert rep["first_bad_cell"] >> 4 == v["table_row"] and rep["first_bad_constraint"] == v["constraint"] and rep["first_bad_value"] == [v["value"], 0, 0, 0], rep
    assert rep["bad_per_constraint"][v["constraint"]] >= 1 and max(rep["bad_per_constraint"]) <= rep["n_bad_cells"] <= sum(rep["bad_per_constraint"])
    rc, bad_cell, bad_c, value = oracle.assert_constraints_table(v["component"], rows, ELEMS)
    assert rc == 1 and (rep["first_bad_cell"], rep["first_bad_constraint"], rep["first_bad_value"]) == (bad_cell, bad_c, value)


@pytest.mark.single_conv
@pytest.mark.parametrize("component,col,row,val,constraint", [
    (0, 3, 1, 2, 4), (0, 0, 0, 1, 0), (1, 3, 0, 2, 1), (3, 8, 2, 9, 6), (10, 2, 0, 44, 0),      # the corruptions of tests/test_oracle_prove.py
])
def test_shim_agrees_with_the_oracle_on_the_first_failure(oracle, air_check, component, col, row, val, constraint):
    rows = oracle.table(*PROGRAM, component)
    rows[row, col] = val
    rc, bad_cell, bad_c, value = oracle.assert_constraints_table(component, rows, ELEMS)
    rep = air_check.check(component, rows.T, ELEMS)
    assert rc == 1 and bad_c == constraint
    assert (rep["first_bad_cell"], rep["first_bad_constraint"], rep["first_bad_value"]) == (bad_cell, bad_c, value)
    assert rep["n_bad_cells"] >= 1 and rep["bad_per_constraint"][bad_c] >= 1


@pytest.mark.single_conv
@pytest.mark.parametrize("component", range(13))
def test_shim_reports_no_violation_on_a_real_trace(oracle, air_check, component):
    rows = oracle.table(*PROGRAM, component)
    rep = air_check.check(component, rows.T, ELEMS)
    assert rep["n_bad_cells"] == 0 and rep["first_bad_cell"] is None and rep["first_bad_constraint"] == -1
    assert rep["first_bad_value"] == [0] * 4 and rep["bad_per_constraint"] == [0] * 16
    assert rep["claimed_sum"] == oracle.logup_generate(component, np.ascontiguousarray(rows.T), ELEMS)[1]


@pytest.mark.single_conv
def test_shim_counts_a_logup_side_corruption_in_two_cells(oracle, air_check):
    """Caller-supplied logUp columns: one patched cell of the last column breaks the logUp constraint at that cell and at its coset successor."""
    rows = np.ascontiguousarray(oracle.table(*PROGRAM, 0).T)
    inter, claimed = oracle.logup_generate(0, rows, ELEMS)
    inter[0, 37] = (int(inter[0, 37]) + 1) % ((1 << 31) - 1)
    rep = air_check.check(0, rows, ELEMS, inter=inter, claimed=claimed)
    assert rep["n_bad_cells"] == 2 and rep["bad_per_constraint"] == [0] * 11 + [2] + [0] * 4 and rep["first_bad_constraint"] == 11


def test_failure_line_format(pkg):
    rep = {"name": "memory", "n_bad_cells": 16, "first_bad_constraint": 6, "first_bad_row": 0, "first_bad_cell": 0, "first_bad_value": [2, 0, 0, 0],
           "bad_per_constraint": [0] * 6 + [16] + [0] * 9}
    assert pkg.format_check_failure(rep) == "memory: constraint 6 fails at table row 0 (cell 0), value (2, 0, 0, 0); 16 cells violate it"


C_LAYOUT = r"""
#include <stdio.h>
#include <stddef.h>
#include "bfhip.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(bfhip_check_report, f), sizeof(((bfhip_check_report*)0)->f));
int main(void) {
    printf("sizeof %zu %zu\n", sizeof(bfhip_check_report), sizeof(bfhip_check_report));
    F(component) F(log_size) F(n_bad_cells) F(first_bad_cell) F(first_bad_constraint) F(first_bad_value) F(bad_per_constraint) F(claimed_sum) F(reserved)
    return 0;
}
"""


def test_check_report_has_one_layout_in_header_ctypes_and_rust(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(C_LAYOUT)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = [l.split() for l in subprocess.check_output([str(exe)], text=True).strip().split("\n")]
    c_size = int(lines[0][1])
    c_fields = [(name, int(off), int(size)) for name, off, size in lines[1:]]
    R = pkg.CheckReport
    assert ctypes.sizeof(R) == c_size == 208
    assert [(n, getattr(R, n).offset, getattr(R, n).size) for n, _ in R._fields_] == c_fields
    # the generated Rust struct: #[repr(C)] lays the same field types out by the same rule — natural alignment, declaration order
    rust = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    body = re.search(r"pub struct BfhipCheckReport \{(.*?)\}", rust).group(1)
    assert "#[repr(C)]" in rust[rust.index("pub struct BfhipCheckReport") - 120: rust.index("pub struct BfhipCheckReport")]
    sizes = {"u32": 4, "i32": 4, "u64": 8}
    off, align, r_fields = 0, 1, []
    for name, ty in re.findall(r"pub (\w+): ([^,]+?)(?:,|$)", body.strip()):
        m = re.match(r"\[(\w+); (\d+)\]", ty.strip())
        base, count = (m.group(1), int(m.group(2))) if m else (ty.strip(), 1)
        a = sizes[base]
        off = (off + a - 1) // a * a
        r_fields.append((name, off, a * count))
        off += a * count
        align = max(align, a)
    assert r_fields == c_fields and (off + align - 1) // align * align == c_size
