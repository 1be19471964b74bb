"""CPU: bfhip_relation_program_multiplicities (include/bfhip.h "Lookup multiplicities") at what a host without a GPU can check — the report's
layout in header, ctypes and Rust, the entry's declarations, the null-context refusal, and the model of tests/relation_multiplicities_model.py
against cases worked out by hand."""
import ctypes
import os
import re
import subprocess

import numpy as np

import relation_multiplicities_model as model
from conftest import ROOT

P = (1 << 31) - 1
M_COL, WORD, ENTRY = 0, 17, 18
FIELDS = [("relation", 0, 4), ("n_words", 4, 4), ("target_table", 8, 4), ("target_entry", 12, 4), ("n_rows", 16, 8), ("n_row_tuples", 24, 8),
          ("n_entries", 32, 8), ("n_tuples", 40, 8), ("n_filled", 48, 8), ("n_missing", 56, 8), ("n_reported", 64, 8), ("reserved", 72, 8)]


def test_report_has_one_layout_in_header_ctypes_and_rust(pkg, tmp_path):
    c_name = "bfhip_multiplicity_report"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bfhip.h"\nint main(void) {\n    printf("sizeof %%zu\\n", sizeof(%s));\n' % c_name +
                   "".join('    printf("%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));\n' % (f, c_name, f, c_name, f) for f, _, _ in FIELDS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = [l.split() for l in subprocess.check_output([str(exe)], text=True).strip().split("\n")]
    c_fields = [(name, int(off), int(sz)) for name, off, sz in lines[1:]]
    R = pkg.MultiplicityReport
    assert ctypes.sizeof(R) == int(lines[0][1]) == 80
    assert [(n, getattr(R, n).offset, getattr(R, n).size) for n, _ in R._fields_] == c_fields == FIELDS
    hdr = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    stated = re.search(r"%s\s+(\d+) bytes: (.*?)\s*\*/" % c_name, hdr, flags=re.S)
    assert int(stated.group(1)) == 80 and [(n, int(o)) for n, o in re.findall(r"(\w+) (\d+)", stated.group(2))] == [(n, o) for n, o, _ in FIELDS]
    rust = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    decl = re.search(r"pub struct BfhipMultiplicityReport \{(.*?)\}", rust).group(1)
    assert re.findall(r"pub (\w+): ([^,]+?)(?:,| $)", decl) == [(n, {4: "u32", 8: "u64"}[s] if n != "reserved" else "[u32; 2]") for n, _, s in FIELDS]


def test_entry_is_declared_in_header_rust_and_library(pkg):
    hdr = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    assert re.search(r"int32_t bfhip_relation_program_multiplicities\(bfhip_ctx\* ctx, const bfhip_relation_program_table\* tables, uint32_t n_tables", hdr)
    assert "bfhip_relation_program_multiplicities," in hdr.split("While a session is open")[1].split("Everything else keeps working")[0]
    rust = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    assert ("pub fn bfhip_relation_program_multiplicities(ctx: *mut BfhipCtx, tables: *const BfhipRelationProgramTable, n_tables: u32, n_relations: u32, relation: u32, "
            "target_table: u32, target_entry: u32, out_d: *mut u32, report: *mut BfhipMultiplicityReport, missing_h: *mut BfhipRelationEntry, cap: u32) -> i32;") in rust
    assert "pub fn multiplicities(" in open(os.path.join(ROOT, "bindings", "rust", "lib.rs")).read()
    assert hasattr(pkg.lib(), "bfhip_relation_program_multiplicities") and hasattr(pkg.Context, "relation_program_multiplicities")


def test_null_context_is_refused(pkg):
    rep = pkg.MultiplicityReport()
    tables = (pkg.RelationProgramTable * 1)()
    assert pkg.lib().bfhip_relation_program_multiplicities(None, tables, 1, 1, 0, 0, 0, None, ctypes.byref(rep), None, 0) == -1
    assert pkg.lib().bfhip_last_error().decode() == "null context"


def test_result_lines(pkg):
    entry = {"relation": 0, "name": "lookup", "tuple": (9,), "net": 1, "n_yield": 1, "n_use": 0, "n_other": 0, "first_yield": (0, 5), "first_use": None}
    report = {"name": "lookup", "n_missing": 3, "n_reported": 1}
    res = pkg.MultiplicityResult(report, [entry], ["trace"], "trace")
    assert not res.ok
    assert res.lines() == ["lookup relation: (9) net +1: yielded 1x (first: trace row 5), used 0x; no row of trace holds it", "lookup relation: 2 more missing tuples not listed"]
    assert pkg.MultiplicityResult(dict(report, n_missing=0, n_reported=0), [], ["trace"], "trace").ok


# ---- the model against cases worked out by hand -------------------------------------------------------------------------------------------------
def entry(relation, cols, mult_col):
    """{WORD of each column, ENTRY}: registers = column indices"""
    code = []
    for c in cols + [mult_col]:
        code += [M_COL, c, c, 0]
    for c in cols:
        code += [WORD, 0, c, 0]
    return code + [ENTRY, relation, mult_col, 0]


U = lambda *v: np.array(v, dtype=np.uint32)


def test_model_duplicates_missing_net_zero_and_negative_net():
    """Consumer (table 0, 8 rows): values 5 5 5 7 7 9 3 3 with multiplicities 1 1 1 1 p-1 1 p-1 p-1. Table (table 1, 4 rows): 5 7 5 3 with a
    multiplicity column of garbage. 5 is used +3 (row 0 gets 3, its duplicate at row 2 gets 0), 7 cancels (net 0: row 1 gets 0, and it is not
    missing), 9 is used once and no row holds it (missing), 3 has net p - 2 (row 3)."""
    consumer = (entry(0, [0], 1), 3, 0, [U(5, 5, 5, 7, 7, 9, 3, 3), U(1, 1, 1, 1, P - 1, 1, P - 1, P - 1)], None)
    table = (entry(0, [0], 1), 2, 0, [U(5, 7, 5, 3), U(0xFFFFFFFF, 0, P, 77)], None)
    out, report, missing = model.multiplicities([consumer, table], 0, 1, 0)
    assert out.tolist() == [3, 0, 0, P - 2]
    assert report == {"n_rows": 4, "n_row_tuples": 3, "n_entries": 8, "n_tuples": 4, "n_filled": 2, "n_missing": 1}
    assert missing == [{"tuple": (9,), "net": 1, "n_yield": 1, "n_use": 0, "n_other": 0, "first_yield": (0, 5), "first_use": None}]


def test_model_second_entry_of_the_target_counts_and_other_relations_do_not():
    """One table, two ENTRYs of relation 1 (width 2) and one of relation 0 between them. Target = the second ENTRY of relation 1: the first one
    counts as an other entry (multiplicity 2, an "other" kind; row 2's is 0: no entry), relation 0 is ignored."""
    code = entry(1, [0, 1], 2) + entry(0, [0], 2) + entry(1, [3, 4], 5)
    cols = [U(1, 2, 3, 4), U(1, 1, 1, 1), U(2, 2, 0, 2), U(2, 1, 6, 6), U(1, 1, 6, 6), U(0, 0, 0, 0)]
    out, report, missing = model.multiplicities([(code, 2, 0, cols, None)], 1, 0, 1)
    assert out.tolist() == [2, 2, 0, 0]
    assert report == {"n_rows": 4, "n_row_tuples": 3, "n_entries": 3, "n_tuples": 3, "n_filled": 2, "n_missing": 1}
    assert missing == [{"tuple": (4, 1), "net": 2, "n_yield": 0, "n_use": 0, "n_other": 1, "first_yield": None, "first_use": None}]
    # with the first ENTRY as the target the second one counts, with its zero multiplicities: nothing to write, nothing missing
    out, report, missing = model.multiplicities([(code, 2, 0, cols, None)], 1, 0, 0)
    assert out.tolist() == [0, 0, 0, 0] and missing == []
    assert report == {"n_rows": 4, "n_row_tuples": 4, "n_entries": 0, "n_tuples": 0, "n_filled": 0, "n_missing": 0}


def test_model_row_granular_target():
    """The target at row_shift 2 with a full-size tuple column (read at r << 2) and a row-granular multiplicity column."""
    consumer = (entry(0, [0], 1), 3, 0, [U(10, 10, 14, 14, 14, 11, 11, 11), U(1, 1, 1, 1, 1, 1, 1, 1)], None)
    table = (entry(0, [0], 1), 3, 2, [U(10, 11, 12, 13, 14, 15, 16, 17), U(0, 0)], [0, 2])
    out, report, missing = model.multiplicities([consumer, table], 0, 1, 0)
    assert out.tolist() == [2, 3]
    assert report == {"n_rows": 2, "n_row_tuples": 2, "n_entries": 8, "n_tuples": 3, "n_filled": 2, "n_missing": 1}
    assert [m["tuple"] for m in missing] == [(11,)] and missing[0]["net"] == 3 and missing[0]["first_yield"] == (0, 5)
