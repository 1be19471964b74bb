"""CPU: the pool's queue (bfhip_pool_submit_* / bfhip_pool_wait / ...) and bfhip_prove_registers at the boundary a host without a GPU can
check — declared in include/bfhip.h, exported by both builds of the library, bound in the Python mirror and in the Rust wrapper; the
layout of bfhip_pool_result as a C compiler sees it; and every entry returning -1 on null arguments without blocking."""
import ctypes
import os
import re
import subprocess
import sys
import textwrap

from conftest import ROOT, TESTHOOKS_LIBRARY

NEW_ENTRIES = ["bfhip_prove_registers", "bfhip_pool_submit_trace", "bfhip_pool_submit_brainfuck", "bfhip_pool_submit_registers", "bfhip_pool_wait",
               "bfhip_pool_outstanding", "bfhip_pool_cancel"]
# bfhip_pool_result as include/bfhip.h documents it
OFFSETS = {"ticket": 0, "user_tag": 8, "status": 16, "worker": 20, "flags": 24, "log_max_rows": 28, "proof_json": 32, "proof_len": 40, "error": 48,
           "seconds_queued": 56, "seconds_proving": 64, "reserved": 72}


def _header():
    return open(os.path.join(ROOT, "include", "bfhip.h")).read()


def test_entries_are_declared_exported_and_bound(pkg):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    L, H = pkg.lib(), ctypes.CDLL(TESTHOOKS_LIBRARY)
    rust_sys = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, code), f"{name} is not declared in include/bfhip.h"
        assert hasattr(L, name) and hasattr(H, name), f"{name} is not exported"
        assert "pub fn %s(" % name in rust_sys, f"{name} is missing from bfhip_sys.rs"
    assert "BFHIP_JOB_CANCELLED = -2" in code and "BFHIP_POOL_MAX_OUTSTANDING = 4096" in code
    # the Python mirror
    assert callable(pkg.prove_registers)
    for method in ("submit_trace", "submit_program", "submit_registers", "wait", "outstanding", "cancel", "as_completed"):
        assert callable(getattr(pkg.Pool, method)), method
    assert pkg.JOB_CANCELLED == -2 and pkg.POOL_MAX_OUTSTANDING == 4096
    # the Rust side: the generated struct and the safe wrapper
    assert "pub struct BfhipPoolResult" in rust_sys and "pub const BFHIP_JOB_CANCELLED: i32 = -2;" in rust_sys
    wrapper = open(os.path.join(ROOT, "bindings", "rust", "lib.rs")).read()
    for needle in ("pub fn submit_machine(&self, machine: &'a Machine, tag: u64)", "pub fn wait(&self, timeout_ms: u32)", "pub fn prove_machine(",
                   "sys::bfhip_prove_registers(", "sys::bfhip_pool_submit_registers(", "sys::bfhip_pool_wait("):
        assert needle in wrapper, needle
    declared = set(re.findall(r"pub fn (bfhip_\w+)\(", rust_sys))
    assert set(re.findall(r"sys::(bfhip_\w+)", wrapper)) <= declared


def test_pool_result_layout(pkg, tmp_path):
    """88 bytes with the offsets the header states — as a C compiler lays the struct out, as the Python mirror declares it and as the
    generated Rust struct lists its fields."""
    src = tmp_path / "layout.c"
    fields = list(OFFSETS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bfhip.h"\nint main(void) {\n    printf("%zu", sizeof(bfhip_pool_result));\n' +
                   "".join('    printf(" %%zu", offsetof(bfhip_pool_result, %s));\n' % f for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 88 and dict(zip(fields, got[1:])) == OFFSETS
    assert ctypes.sizeof(pkg.PoolResult) == 88
    assert {n: getattr(pkg.PoolResult, n).offset for n, _ in pkg.PoolResult._fields_} == OFFSETS
    documented = re.search(r"bfhip_pool_result\s+88 bytes:(.*?)\*/", _header(), flags=re.S).group(1)
    assert {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+) (\d+)", documented.replace("*", " "))} == OFFSETS
    rust = re.search(r"pub struct BfhipPoolResult \{(.*?)\}", open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()).group(1)
    assert [f.strip().split(":")[0].replace("pub ", "") for f in rust.split(", pub ")] == fields


def test_new_entries_return_minus_one_on_null_arguments_without_blocking():
    """Each call in a child process with a time limit: a wait that blocked on a null pool would end as a timeout, a crash as a signal."""
    prog = textwrap.dedent("""
        import ctypes, sys
        sys.path.insert(0, %r)
        from conftest import load_package
        pkg = load_package()
        L = pkg.lib()
        z, t, r = ctypes.c_size_t(0), ctypes.c_uint64(), pkg.PoolResult()
        rows, words = (ctypes.c_uint32 * 7)(), (ctypes.c_uint32 * 1)(43)
        forever = ctypes.c_uint32(0xFFFFFFFF)
        calls = {
            "prove_registers_null_ctx": lambda: L.bfhip_prove_registers(None, rows, ctypes.c_size_t(1), words, ctypes.c_size_t(1), 12, None, None, None, None),
            "submit_trace_null": lambda: L.bfhip_pool_submit_trace(None, None, 12, ctypes.c_uint64(0), ctypes.byref(t)),
            "submit_brainfuck_null": lambda: L.bfhip_pool_submit_brainfuck(None, b"+", None, z, 12, ctypes.c_uint64(0), ctypes.byref(t)),
            "submit_registers_null": lambda: L.bfhip_pool_submit_registers(None, rows, ctypes.c_size_t(1), words, ctypes.c_size_t(1), 12, ctypes.c_uint64(0), ctypes.byref(t)),
            "wait_null_pool_forever": lambda: L.bfhip_pool_wait(None, forever, ctypes.byref(r)),
            "wait_all_null_forever": lambda: L.bfhip_pool_wait(None, forever, None),
            "outstanding_null": lambda: L.bfhip_pool_outstanding(None, None, None, None),
            "cancel_null": lambda: L.bfhip_pool_cancel(None, ctypes.c_uint64(1)),
        }
        for name, call in calls.items():
            print(name, call(), L.bfhip_last_error().decode(), flush=True)
        print("done", t.value)
    """) % os.path.join(ROOT, "tests")
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done 0"                        # no ticket was issued
    assert len(lines) == 9
    for line in lines[:-1]:
        name, rc, msg = line.split(" ", 2)
        assert rc == "-1", line
        assert msg == ("null context" if name == "prove_registers_null_ctx" else "null pool"), line
