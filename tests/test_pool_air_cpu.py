"""CPU: bfhip_pool_submit_air and the scratch reserve (include/bfhip.h "AIR statements as jobs of a pool's queue", "The scratch reserve") at
what a host without a GPU can check — the new entries declared, exported, generated into both bindings and mirrored; bfhip_pool_result still
88 bytes; null arguments refused without blocking; and the two host-only headers behind the feature (csrc/air_statement_copy.h,
csrc/scratch_reserve.h) under AddressSanitizer + UBSan in a stand-alone program (tests/native/pool_air_host_sanitize.cpp)."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT, TESTHOOKS_LIBRARY
from pool_air_cases import _lookup_statement, shapes_statement
from test_air_prove_cpu import _statement_text

ENTRIES = ["bfhip_pool_submit_air", "bfhip_pool_set_scratch_reserve", "bfhip_ctx_set_scratch_reserve", "bfhip_ctx_scratch_stats"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bfhip.h")).read(), flags=re.S)


def test_entries_are_declared_exported_generated_and_mirrored(pkg):
    code, gen = _code(), open(os.path.join(ROOT, "stwo-brainfuck_amd", "_abi_gen.py")).read()
    rust_sys = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    L, H = pkg.lib(), ctypes.CDLL(TESTHOOKS_LIBRARY)
    for name in ENTRIES:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, code), f"{name} is not declared in include/bfhip.h"
        assert hasattr(L, name) and hasattr(H, name), f"{name} is not exported"
        assert '"%s"' % name in gen, f"{name} is missing from _abi_gen.py"
        assert "pub fn %s(" % name in rust_sys, f"{name} is missing from bfhip_sys.rs"
    # the prototype as the issue states it, argument by argument
    proto = re.search(r"int32_t\s+bfhip_pool_submit_air\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert [re.sub(r"\s+", " ", a.strip()) for a in proto.split(",")] == [
        "bfhip_pool* pool", "const bfhip_air_statement* statement", "const uint32_t* const* const* tree_cols_h", "bfhip_air_kernel* const* kernels_h",
        "const bfhip_channel* ch", "uint32_t flags", "uint64_t user_tag", "uint64_t* ticket"]
    assert re.search(r"int32_t\s+bfhip_ctx_set_scratch_reserve\s*\(\s*bfhip_ctx\*\s+ctx,\s*uint64_t\s+bytes\s*\)", code)
    assert re.search(r"int32_t\s+bfhip_ctx_scratch_stats\s*\(\s*bfhip_ctx\*\s+ctx,\s*uint64_t\s+out\[4\]\s*\)", code)
    assert re.search(r"int32_t\s+bfhip_pool_set_scratch_reserve\s*\(\s*bfhip_pool\*\s+pool,\s*uint64_t\s+bytes_per_worker\s*\)", code)
    for method in ("submit_air", "air_compile", "prove_batch_air", "set_scratch_reserve"):
        assert callable(getattr(pkg.Pool, method)), method
    for method in ("set_scratch_reserve", "scratch_stats"):
        assert callable(getattr(pkg.Context, method)), method
    assert callable(pkg.PoolCompiledAir)
    wrapper = open(os.path.join(ROOT, "bindings", "rust", "lib.rs")).read()
    assert "pub fn submit_air(" in wrapper and "sys::bfhip_pool_submit_air(" in wrapper
    assert set(re.findall(r"sys::(bfhip_\w+)", wrapper)) <= set(re.findall(r"pub fn (bfhip_\w+)\(", rust_sys))


def test_pool_result_is_still_88_bytes(pkg, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "bfhip.h"\nint main(void) { printf("%zu %zu", sizeof(bfhip_pool_result), sizeof(bfhip_air_statement)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["88", "32"]
    assert ctypes.sizeof(pkg.PoolResult) == 88
    rust = re.search(r"pub struct BfhipPoolResult \{(.*?)\}", open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read(), flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", rust) == [n for n, _ in pkg.PoolResult._fields_]


def test_null_arguments_return_without_blocking(pkg):
    L = pkg.lib()
    t = ctypes.c_uint64(7)
    st = _lookup_statement(pkg, 6)
    with pkg.Channel((0, 0, 0, 0)) as ch:
        assert L.bfhip_pool_submit_air(None, ctypes.byref(st._c()), None, None, ch._h, 0, ctypes.c_uint64(0), ctypes.byref(t)) == -1
    assert L.bfhip_last_error().decode() == "bfhip_pool_submit_air: null argument" and t.value == 7
    assert L.bfhip_pool_set_scratch_reserve(None, ctypes.c_uint64(0)) == -1
    assert L.bfhip_ctx_set_scratch_reserve(None, ctypes.c_uint64(0)) == -1
    assert L.bfhip_ctx_scratch_stats(None, None) == -1


def test_host_headers_under_address_and_ub_sanitizers(pkg, tmp_path):
    """tests/native/pool_air_host_sanitize.cpp (its own main) with the four host-only translation units as plain C++ under g++
    -fsanitize=address,undefined, run directly. The deep copy: every source array overwritten and freed, then air_statement_plan on the
    copy gives the plan of the original — for the lookup statement and for the one of four components, under both blowups (the plan
    words are compared with the mirror's sample description too). The reserve's bookkeeping: nested marks, alignment, a request that
    does not fit, the high-water mark, a close out of order refused."""
    exe = str(tmp_path / "pool_air_host_sanitize")
    csrc = os.path.join(ROOT, "stwo-brainfuck_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "native", "pool_air_host_sanitize.cpp"),
                           "-x", "c++"] + [os.path.join(csrc, f) for f in ("air_prove_host.hip", "air_program_host.hip", "logup_program_host.hip", "pcs_host.hip")])
    statements = [_lookup_statement(pkg, 6), shapes_statement(pkg, 4), shapes_statement(pkg, 9)]
    paths = []
    for i, st in enumerate(statements):
        paths.append(str(tmp_path / ("statement_%d.txt" % i)))
        open(paths[-1], "w").write(_statement_text(st))
    for blowup in (1, 2):
        r = subprocess.run([exe, str(blowup), "14"] + paths, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-600:], r.stderr[-2000:])
        lines = r.stdout.strip().splitlines()
        assert len(lines) == len(statements) + 1 and lines[-1].startswith("reserve ok "), lines
        assert int(lines[-1].split()[2]) >= 20      # the checks the program made, each a condition that held
        for st, line in zip(statements, lines):
            words = line.split()
            assert words[:4] == ["copy", "ok", str(len(st.trees)), str(len(st.components))], line
            # the plan the program printed against the mirror's description of the same statement
            pts, samples = st.samples(pkg.PcsConfig(log_blowup_factor=blowup))
            assert [w for w in words if w.startswith("P")] == ["P%d,%d" % p for p in pts]
            got_counts = [int(w[1:]) for w in words if w.startswith("S")]
            assert got_counts == [len(c) for t in samples for c in t]
