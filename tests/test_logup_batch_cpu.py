"""CPU: what bfhip_logup_program_generate_batch (include/bfhip.h "Fraction programs, batched") shows without a GPU — the layout of
bfhip_logup_component as the header states it, the constant, the symbol in both libraries, the Rust wrapper's presence, and the host-only
planner (csrc/logup_batch_plan.h: launch groups, the three prefix tables, the scratch layout, the interval-overlap check) under
AddressSanitizer + UBSan in a stand-alone program (tests/native/logup_batch_plan_sanitize.cpp)."""
import ctypes
import os
import subprocess

from conftest import ROOT

OFFSETS = {"program": 0, "log_size": 8, "n_params": 12, "cols_h": 16, "col_shifts_h": 24, "params_h": 32, "out_cols_h": 40, "reserved": 48}


def test_the_struct_has_the_layout_the_header_states(pkg):
    cls = pkg.LogupComponent
    assert ctypes.sizeof(cls) == 56
    assert {name: getattr(cls, name).offset for name, _ in cls._fields_} == OFFSETS
    assert ctypes.sizeof(dict(cls._fields_)["reserved"]) == 8
    text = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    assert "bfhip_logup_component  56 bytes: program 0, log_size 8, n_params 12, cols_h 16, col_shifts_h 24, params_h 32, out_cols_h 40, reserved 48" in text
    assert "enum { BFHIP_LOGUP_BATCH_MAX_COMPONENTS = 64 };" in text
    assert pkg.LOGUP_BATCH_MAX_COMPONENTS == 64


def test_the_symbol_is_exported_by_both_libraries(pkg):
    assert hasattr(pkg.lib(), "bfhip_logup_program_generate_batch")
    hooks = ctypes.CDLL(os.path.join(os.path.dirname(pkg._LIB_PATH), pkg.TESTHOOKS_LIBRARY))
    assert hasattr(hooks, "bfhip_logup_program_generate_batch")
    assert callable(pkg.Context.logup_program_generate_batch)
    rust = open(os.path.join(ROOT, "bindings", "rust", "lib.rs")).read()
    assert "pub fn logup_program_generate_batch(ctx: &Context, comps: &[LogupComponent])" in rust


def test_planner_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/logup_batch_plan_sanitize.cpp (its own main) over csrc/logup_batch_plan.h, compiled as plain C++ under
    g++ -fsanitize=address,undefined and run once, directly: 10 component lists x 4 launch modes."""
    exe = str(tmp_path / "logup_batch_plan_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "logup_batch_plan_sanitize.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-800:], r.stderr[-2000:])
    assert "lists checked: 40; failures: 0" in r.stdout, r.stdout
