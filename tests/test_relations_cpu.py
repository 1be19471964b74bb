"""CPU side of the relation summary (include/bfhip.h: bfhip_relation_summary / bfhip_trace_relations): the model the GPU results are compared
against (tests/relation_model.py) agrees with the oracle's logUp total on what "balanced" means, and the three structs have one layout in
the header, the ctypes mirror and the generated Rust."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import relation_model
from conftest import ROOT, P
from oracle_air_check import table_from_registers

ALL_OPS = ("+++>,<[>+.<-]", b"\x01")
UNKNOWN_TUPLE = (1, 1, 35, 43, 0, 1, 1)
ELEMS = [5, 1, 2, 3, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83]      # the drawn elements of tests/test_trace_check_cpu.py


def unknown_opcode_registers(oracle):
    """The second '+' (ip 1) becomes 35, which is no instruction — in the register rows and in the program: what a VM that steps over
    comment characters hands over. Every AIR holds row by row; the Processor relation keeps one tuple nobody consumes."""
    code, inp = ALL_OPS
    regs = oracle.run(code, inp)[1].copy()
    words = list(oracle.compile(code))
    assert regs[1, 2] == ord("+") and regs[0, 3] == ord("+") and words[1] == ord("+")
    regs[1, 2] = 35; regs[0, 3] = 35; words[1] = 35
    return regs, words


def altered_registers(oracle):
    """The case of tests/test_gpu_trace_check.py: a VM that adds 5."""
    code, inp = ALL_OPS
    regs = oracle.run(code, inp)[1].copy()
    regs[1, 5] = 5
    return regs, list(oracle.compile(code))


def oracle_tables(oracle, regs, words):
    return [(k, np.ascontiguousarray(table_from_registers(oracle, regs, words, k).T)) for k in range(13)]


def oracle_logup_total(oracle, tables, elems):
    total = np.zeros(4, dtype=object)
    for comp, cols in tables:
        total = (total + np.array(oracle.logup_generate(comp, cols, elems)[1], dtype=object)) % P
    return tuple(int(v) for v in total)


@pytest.mark.single_conv
@pytest.mark.parametrize("case", ["valid", "unknown_opcode", "altered_registers"])
def test_model_says_balanced_iff_the_oracles_logup_total_is_zero(oracle, case):
    if case == "valid":
        regs, words = oracle.run(*ALL_OPS)[1], oracle.compile(ALL_OPS[0])
    else:
        regs, words = unknown_opcode_registers(oracle) if case == "unknown_opcode" else altered_registers(oracle)
    tables = oracle_tables(oracle, regs, words)
    model = relation_model.relations(tables)
    total = oracle_logup_total(oracle, tables, ELEMS)
    print(case, total, [(m["n_entries"], m["n_tuples"], m["entries"]) for m in model])
    balanced = all(not m["entries"] for m in model)
    # altered_registers breaks row-local constraints only: every table is built from the same rows, so the tuples still pair up
    assert balanced == (total == (0, 0, 0, 0)) == (case != "unknown_opcode")
    assert all(m["n_entries"] > 0 and 0 < m["n_tuples"] <= m["n_entries"] for m in model)
    if case == "unknown_opcode":
        assert total == (1975556491, 1550389372, 741348851, 295949303)
        assert model[0]["entries"] == [] and model[1]["entries"] == []
        assert model[2]["entries"] == [{"tuple": UNKNOWN_TUPLE, "net": 1, "n_yield": 1, "n_use": 0, "n_other": 0, "first_yield": (3, 1), "first_use": None}]


def test_entry_line_format(pkg):
    e = {"name": "processor", "tuple": UNKNOWN_TUPLE, "net": 1, "n_yield": 1, "n_use": 0, "n_other": 0, "first_yield": (3, 1), "first_use": None}
    assert pkg.format_relation_entry(e) == "processor relation: (1, 1, 35, 43, 0, 1, 1) net +1: yielded 1x (first: processor row 1), used 0x"
    e = {"name": "memory", "tuple": (4, 0, 2), "net": P - 2, "n_yield": 0, "n_use": 2, "n_other": 0, "first_yield": None, "first_use": (0, 9)}
    assert pkg.format_relation_entry(e) == "memory relation: (4, 0, 2) net -2: yielded 0x, used 2x (first: memory row 9)"
    e = {"name": "memory", "tuple": (4, 0, 2), "net": 3, "n_yield": 1, "n_use": 0, "n_other": 1, "first_yield": (1, 0), "first_use": None}
    assert pkg.format_relation_entry(e, ["processor[0]", "memory[1]"]) == \
        "memory relation: (4, 0, 2) net +3: yielded 1x (first: memory[1] row 0), used 0x, 1 rows with another multiplicity"


STRUCTS = {"bfhip_relation_entry": ("RelationEntry", "BfhipRelationEntry", 96,
                                    "relation n_words tuple net n_yield n_use n_other first_yield_table first_use_table first_yield_row first_use_row reserved"),
           "bfhip_relation_report": ("RelationReport", "BfhipRelationReport", 48, "relation n_words n_entries n_tuples n_unbalanced n_reported reserved"),
           "bfhip_relation_table": ("RelationTable", "BfhipRelationTable", 16, "component log_size main_rows_h")}


@pytest.mark.parametrize("c_name", sorted(STRUCTS))
def test_structs_have_one_layout_in_header_ctypes_and_rust(pkg, tmp_path, c_name):
    py_name, rust_name, size, fields = STRUCTS[c_name]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bfhip.h"\nint main(void) {\n    printf("sizeof %%zu\\n", sizeof(%s));\n' % c_name +
                   "".join('    printf("%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));\n' % (f, c_name, f, c_name, f) for f in fields.split()) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = [l.split() for l in subprocess.check_output([str(exe)], text=True).strip().split("\n")]
    c_size = int(lines[0][1])
    c_fields = [(name, int(off), int(sz)) for name, off, sz in lines[1:]]
    R = getattr(pkg, py_name)
    assert ctypes.sizeof(R) == c_size == size
    assert [(n, getattr(R, n).offset, getattr(R, n).size) for n, _ in R._fields_] == c_fields
    # the offsets the header's comment states
    hdr = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    stated = re.search(r"%s\s+(\d+) bytes: (.*?)(?=\n \*   bfhip_|\s*\*/)" % c_name, hdr, flags=re.S)
    assert int(stated.group(1)) == c_size
    assert [(n, int(o)) for n, o in re.findall(r"(\w+) (\d+)", stated.group(2).replace("\n", " "))] == [(n, o) for n, o, _ in c_fields]
    # the generated Rust struct: #[repr(C)] lays the same field types out by the same rule — natural alignment, declaration order
    rust = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    at = rust.index("pub struct %s " % rust_name)
    assert "#[repr(C)]" in rust[rust.rindex("\n", 0, at): at]
    body = re.search(r"pub struct %s \{(.*?)\}" % rust_name, rust).group(1)
    sizes = {"u32": 4, "i32": 4, "u64": 8, "*const *const u32": 8}
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


def test_new_symbols_are_in_header_python_and_rust(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bfhip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    rust_lib = open(os.path.join(ROOT, "bindings", "rust", "lib.rs")).read()
    for sym in ("bfhip_relation_summary", "bfhip_trace_relations"):
        assert re.search(r"int32_t\s+%s\s*\(" % sym, hdr) and "pub fn %s(" % sym in rust and hasattr(pkg.lib(), sym)
    assert "sys::bfhip_trace_relations" in rust_lib and "pub fn relations(" in rust_lib
    for name in ("RelationEntry", "RelationReport", "RelationTable", "RelationResult", "format_relation_entry", "RELATION_NAMES"):
        assert hasattr(pkg, name)
    assert callable(pkg.Context.relation_summary) and callable(pkg.Trace.relations)
