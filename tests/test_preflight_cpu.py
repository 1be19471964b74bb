"""CPU side of a proof's preflight (include/bfhip.h: bfhip_ctx_set_preflight, bfhip_ctx_last_preflight, bfhip_format_preflight,
bfhip_pool_set_preflight): `bfhip_preflight_report` has one layout in the header comment, the compiled header, the ctypes mirror and the
generated Rust; bfhip_format_preflight (host only) writes the lines of the Python formatters on canned reports; the new symbols are exported
by both builds of the library. No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, TESTHOOKS_LIBRARY

P = (1 << 31) - 1
NEW_SYMBOLS = ("bfhip_ctx_set_preflight", "bfhip_ctx_get_preflight", "bfhip_ctx_last_preflight", "bfhip_format_preflight", "bfhip_pool_set_preflight")
FIELDS = ("ran", "rejected", "n_bad_components", "n_entries", "logup_total", "components", "relations", "entries", "seconds", "reserved")

C_LAYOUT = r"""
#include <stdio.h>
#include <stddef.h>
#include "bfhip.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(bfhip_preflight_report, f), sizeof(((bfhip_preflight_report*)0)->f));
int main(void) {
    printf("sizeof %zu %d\n", sizeof(bfhip_preflight_report), (int)BFHIP_TRACE_REJECTED);
    F(ran) F(rejected) F(n_bad_components) F(n_entries) F(logup_total) F(components) F(relations) F(entries) F(seconds) F(reserved)
    return 0;
}
"""


def test_preflight_report_has_one_layout_in_header_comment_ctypes_and_rust(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(C_LAYOUT)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = [l.split() for l in subprocess.check_output([str(exe)], text=True).strip().split("\n")]
    c_size, rejected_code = int(lines[0][1]), int(lines[0][2])
    c_fields = [(name, int(off), int(size)) for name, off, size in lines[1:]]
    R = pkg.PreflightReport
    assert rejected_code == pkg.TRACE_REJECTED == -3
    assert ctypes.sizeof(R) == c_size == 4064
    assert [n for n, _ in R._fields_] == list(FIELDS)
    assert [(n, getattr(R, n).offset, getattr(R, n).size) for n, _ in R._fields_] == c_fields
    # the header comment states the same numbers
    hdr = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    said = re.search(r"bfhip_preflight_report\s+(\d+) bytes:(.*?)\*/", hdr, flags=re.S)
    assert int(said.group(1)) == c_size
    offsets = {n: int(o) for n, o in re.findall(r"(\w+) (\d+)", said.group(2).replace("*", " "))}
    assert offsets == {n: o for n, o, _ in c_fields}
    # the generated Rust struct: #[repr(C)], same field order; nested structs have their own layout tests
    rust = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    at = rust.index("pub struct BfhipPreflightReport ")
    assert "#[repr(C)]" in rust[at - 120: at]
    body = re.search(r"pub struct BfhipPreflightReport \{(.*?)\}", rust).group(1)
    sizes = {"u32": (4, 4), "i32": (4, 4), "u64": (8, 8), "f64": (8, 8), "BfhipCheckReport": (208, 8), "BfhipRelationReport": (48, 8), "BfhipRelationEntry": (96, 8)}
    off, align, r_fields = 0, 1, []
    for name, ty in re.findall(r"pub (\w+): ([^,]+?)(?:,|$)", body.strip()):
        m = re.match(r"\[(\w+); (\d+)\]", ty.strip())
        base, count = (m.group(1), int(m.group(2))) if m else (ty.strip(), 1)
        size, a = sizes[base]
        off = (off + a - 1) // a * a
        r_fields.append((name, off, size * count))
        off += size * count
        align = max(align, a)
    assert r_fields == c_fields and (off + align - 1) // align * align == c_size
    assert "pub const BFHIP_TRACE_REJECTED: i32 = -3;" in rust


def test_generated_rust_block_is_current():
    path = os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")
    committed = open(path).read()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(path).read() == committed, "bfhip_sys.rs is stale: run tools/gen_rust_ffi.py"
    for s in NEW_SYMBOLS:
        assert "pub fn %s(" % s in committed
    assert "pub fn bfhip_ctx_last_preflight(ctx: *mut BfhipCtx, out: *mut BfhipPreflightReport) -> i32;" in committed
    assert "pub fn set_preflight(&self, on: bool)" in open(os.path.join(ROOT, "bindings", "rust", "lib.rs")).read()


def test_new_symbols_are_exported_by_both_builds(pkg):
    L, H = pkg.lib(), ctypes.CDLL(TESTHOOKS_LIBRARY)
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), f"libbfhip.so does not export {s}"
        assert hasattr(H, s), f"libbfhip_testhooks.so does not export {s}"
    # the column-overwrite hook of tests/test_gpu_preflight.py exists in the test-hooks build only
    assert hasattr(H, "bfhip_test_trace_set_column")
    assert b"bfhip_test_trace_set_column" not in open(os.path.join(ROOT, "stwo-brainfuck_amd", "libbfhip.so"), "rb").read()


# ---- bfhip_format_preflight against the Python formatters ------------------------------------------------------------------------------------
def bad_component(rep, k, constraint, cell, value, counts):
    c = rep.components[k]
    c.n_bad_cells, c.first_bad_cell, c.first_bad_constraint = max(counts.values()), cell, constraint
    for w, v in enumerate(value):
        c.first_bad_value[w] = v
    for j, n in counts.items():
        c.bad_per_constraint[j] = n


def entry(rep, slot, relation, tup, net, n_yield, n_use, n_other=0, first_yield=None, first_use=None):
    e = rep.entries[slot]
    e.relation, e.n_words, e.net, e.n_yield, e.n_use, e.n_other = relation, len(tup), net % P, n_yield, n_use, n_other
    for w, v in enumerate(tup):
        e.tuple[w] = v
    e.first_yield_table, e.first_yield_row = (-1, (1 << 64) - 1) if first_yield is None else first_yield
    e.first_use_table, e.first_use_row = (-1, (1 << 64) - 1) if first_use is None else first_use


def blank(pkg, ran=1, rejected=1):
    rep = pkg.PreflightReport()
    rep.ran, rep.rejected = ran, rejected
    for k in range(13):
        rep.components[k].component, rep.components[k].log_size = k, 4 + k
        rep.components[k].first_bad_cell, rep.components[k].first_bad_constraint = (1 << 64) - 1, -1
    for r in range(3):
        rep.relations[r].relation, rep.relations[r].n_words = r, (3, 3, 7)[r]
    return rep


def canned(pkg, which):
    if which == "did_not_run":
        return blank(pkg, 0, 0)
    if which == "passed":
        return blank(pkg, 1, 0)
    rep = blank(pkg)
    if which == "one_component":
        bad_component(rep, 0, 6, 0, (2, 0, 0, 0), {6: 16})
        rep.n_bad_components = 1
    elif which == "thirteen_components":
        for k in range(13):
            bad_component(rep, k, k % 2, 16 * k + 3, (k + 1, P - 1, 0, 7), {k % 2: 16 + k, 11: 1})
        rep.n_bad_components = 13
        rep.logup_total[1] = 5
    elif which == "total_only":
        rep.logup_total[0], rep.logup_total[3] = 16, P - 1
        rep.relations[2].n_entries, rep.relations[2].n_tuples, rep.relations[2].n_unbalanced, rep.relations[2].n_reported = 40, 20, 1, 1
        entry(rep, 8, 2, (1, 1, 35, 43, 0, 1, 1), 1, 1, 0, first_yield=(3, 1))
        rep.n_entries = 1
    elif which == "cut_and_other":
        bad_component(rep, 3, 9, 1 << 33, (0, 0, 0, 1), {9: 1 << 40})
        rep.n_bad_components = 1
        rep.logup_total[2] = 9
        rep.relations[0].n_unbalanced, rep.relations[0].n_reported = 7, 4
        for i in range(4):
            entry(rep, i, 0, (i, 2, 3), -1 - i, 0, 1 + i, n_other=3 * (i % 2), first_use=(0, 10 + i))
        rep.relations[1].n_unbalanced, rep.relations[1].n_reported = 2, 2
        entry(rep, 4, 1, (7, 8, 9), 2, 2, 0, first_yield=(2, 5))
        entry(rep, 5, 1, (7, 8, 10), P // 2 + 1, 1, 1, n_other=2, first_yield=(3, 0), first_use=(1, (1 << 40) + 1))
        rep.relations[2].n_unbalanced, rep.relations[2].n_reported = 1 << 35, 4
        for i in range(4):
            entry(rep, 8 + i, 2, (i, 1, 2, 3, 4, 5, P - 1), 1, 1, 0, first_yield=(3, i))
        rep.n_entries = 10
    return rep


CASES = ("did_not_run", "passed", "one_component", "thirteen_components", "total_only", "cut_and_other")


@pytest.mark.parametrize("which", CASES)
def test_format_preflight_equals_the_python_formatters(pkg, which):
    rep = canned(pkg, which)
    text = pkg.format_preflight(rep)
    check, relations = rep.results()
    lines = pkg.format_preflight_lines(check, relations)
    print(text)
    assert text == "\n".join(lines)
    if which == "did_not_run":
        assert lines == ["preflight: did not run"]
    elif which == "passed":
        assert lines == ["preflight: ok"]
    else:
        # the documented composition: headline, CheckResult.failures() (format_check_failure lines + the logUp line), RelationResult.lines()
        assert lines[1:] == check.failures() + relations.lines()
        assert lines[1:1 + check.n_bad_components] == [pkg.format_check_failure(r) for r in check if r["n_bad_cells"]]
        assert [l for l in lines if " relation: (" in l] == [pkg.format_relation_entry(e) for e in relations.entries]
    if which == "one_component":
        assert lines == ["TraceRejected: 1 of 13 components violate their constraints",
                         "memory: constraint 6 fails at table row 0 (cell 0), value (2, 0, 0, 0); 16 cells violate it"]
    if which == "total_only":
        assert lines == ["TraceRejected: the logUp total is not zero", "logUp: the 13 claimed sums add up to (16, 0, 0, %d), not zero" % (P - 1),
                         "processor relation: (1, 1, 35, 43, 0, 1, 1) net +1: yielded 1x (first: processor row 1), used 0x"]
    if which == "thirteen_components":
        assert lines[0] == "TraceRejected: 13 of 13 components violate their constraints and the logUp total is not zero" and len(lines) == 15
    if which == "cut_and_other":
        assert lines[-2:] == ["memory relation: 3 more unbalanced tuples not listed", "processor relation: %d more unbalanced tuples not listed" % ((1 << 35) - 4)]
        assert ", 3 rows with another multiplicity" in lines[4] and "net -2:" in lines[4] and len(lines) == 1 + 1 + 1 + 10 + 2


def test_format_preflight_buffer_too_small_and_bad_arguments(pkg):
    L = pkg.lib()
    rep = canned(pkg, "cut_and_other")
    full = pkg.format_preflight(rep).encode()
    need = ctypes.c_size_t()
    assert L.bfhip_format_preflight(ctypes.byref(rep), None, ctypes.c_size_t(0), ctypes.byref(need)) == -2 and need.value == len(full) + 1
    assert L.bfhip_last_error().decode() == "capacity"
    for cap in (1, 2, 14, len(full)):
        buf = ctypes.create_string_buffer(b"\xff" * (len(full) + 8), len(full) + 8)
        need = ctypes.c_size_t()
        assert L.bfhip_format_preflight(ctypes.byref(rep), buf, ctypes.c_size_t(cap), ctypes.byref(need)) == -2
        assert need.value == len(full) + 1 and buf.raw[:cap] == full[:cap - 1] + b"\0" and buf.raw[cap:] == b"\xff" * (len(full) + 8 - cap)
    buf = ctypes.create_string_buffer(len(full) + 1)
    assert L.bfhip_format_preflight(ctypes.byref(rep), buf, ctypes.c_size_t(len(full) + 1), None) == 0 and buf.value == full
    assert L.bfhip_format_preflight(None, buf, ctypes.c_size_t(8), None) == -1 and "null" in L.bfhip_last_error().decode()
    assert L.bfhip_format_preflight(ctypes.byref(rep), None, ctypes.c_size_t(8), None) == -1 and "null" in L.bfhip_last_error().decode()
    # the switch itself needs no GPU to refuse a null context
    on = ctypes.c_int32()
    assert L.bfhip_ctx_set_preflight(None, 1) == -1 and L.bfhip_ctx_get_preflight(None, ctypes.byref(on)) == -1
    assert L.bfhip_ctx_last_preflight(None, ctypes.byref(rep)) == -1 and L.bfhip_pool_set_preflight(None, 1) == -1
