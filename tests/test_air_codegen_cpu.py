"""CPU: constraint programs compiled to HIP source (include/bfhip.h "Compiled constraint programs": bfhip_air_source) at everything a host
without a GPU can check. The generated text is deterministic and answers the size query; compiled as host C++ (-DBFHIP_AIR_GEN_HOST) with
tests/native/air_codegen_host.cpp it equals the numpy model of tests/air_model.py word for word; the same driver runs once under ASan + UBSan
as the stand-alone program it is; every source compiles for gfx950 through libhiprtc with no device present; and the default library does not
depend on libhiprtc at load time. Programs: the 13 Brainfuck programs, the synthetic AIR with offsets -2 .. +2 (its builder lives in
tests/test_gpu_air_program.py and is imported from there), and a seeded random program at the caps (tests/air_codegen_cases.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import air_codegen_cases as cases
import air_model
import test_gpu_air_program as synthetic
from conftest import ROOT, splitmix_column

P = (1 << 31) - 1
NAMES = synthetic.NAMES + ["synthetic_pm2", "caps"]
SIZES = [(log_size, log_expand) for log_size in (4, 6) for log_expand in (1, 2, 3)]
CELLS = ("random", "p_minus_1", "zero")


@pytest.fixture(scope="module")
def programs(pkg):
    """name -> AirProgram, built once"""
    progs = {name: pkg.brainfuck_air_program(k)[0] for k, name in enumerate(synthetic.NAMES)}
    progs["synthetic_pm2"] = synthetic._synthetic_program(pkg, 3)
    code, n_cols, n_params, n_cons = cases.caps_program(2024)
    progs["caps"] = pkg.AirProgram(code, n_cols, n_params)
    s = progs["caps"].shape
    assert (s["n_instr"], s["m_regs"], s["q_regs"], s["n_constraints"], s["min_offset"], s["max_offset"]) == (4096, 96, 24, 64, -16, 16)
    return progs


@pytest.fixture(scope="module")
def code_objects(programs):
    """name -> (gfx950 code object, compile seconds): each source goes through libhiprtc once per test session"""
    return {name: cases.rtc_compile(prog.source()) for name, prog in programs.items()}


@pytest.mark.parametrize("name", NAMES)
def test_source_is_deterministic_and_answers_the_size_query(pkg, programs, name):
    prog = programs[name]
    src = prog.source()
    assert src == prog.source() and src == pkg.AirProgram(prog.code, prog.shape["n_cols"], prog.shape["n_params"]).source()
    n = ctypes.c_size_t()
    assert pkg.lib().bfhip_air_source(prog._h, None, ctypes.c_size_t(0), ctypes.byref(n)) == 0 and n.value == len(src.encode())
    buf = ctypes.create_string_buffer(16)
    n = ctypes.c_size_t()
    assert pkg.lib().bfhip_air_source(prog._h, buf, ctypes.c_size_t(16), ctypes.byref(n)) == -2 and n.value == len(src.encode())
    assert b"capacity" in pkg.lib().bfhip_last_error() and buf.raw == b"\0" * 16
    # one statement per value, every value a const local; no register file, no run-time indexed array, no inline assembly
    body = src[src.index("BFA_FN void air_row"):]
    assert "asm" not in body and "__shared__" not in src and "m[" not in body and "q[" not in body
    assert body.count("    const ") >= prog.shape["n_instr"]
    # the field arithmetic is m31.h itself
    header = open(os.path.join(ROOT, "stwo-brainfuck_amd", "csrc", "m31.h")).read()
    assert header in src
    # an offset is computed once per distinct non-zero offset, not once per read
    offs = {w - (1 << 32) if w >> 31 else w for i, w in enumerate(prog.code) if i % 4 == 3 and prog.code[i - 3] in (air_model.M_COL, air_model.Q_COL)} - {0}
    assert body.count("offset_row(row, ") == len(offs)


def _inputs(prog, log_size, log_expand, cells, seed):
    s, n = prog.shape, 1 << (log_size + log_expand)
    rnd = lambda k, m: splitmix_column(seed + k, m)
    if cells == "random":
        cols = np.stack([rnd(k, n) for k in range(s["n_cols"])])
        params, coeffs = rnd(1000, 4 * s["n_params"]), rnd(1001, 4 * s["n_constraints"])
    else:      # saturated: every cell, parameter word and coefficient word p - 1; or every cell zero under random parameters and coefficients
        v = P - 1 if cells == "p_minus_1" else 0
        cols = np.full((s["n_cols"], n), v, dtype=np.uint32)
        params = np.full(4 * s["n_params"], v, dtype=np.uint32) if v else rnd(1000, 4 * s["n_params"])
        coeffs = np.full(4 * s["n_constraints"], v, dtype=np.uint32) if v else rnd(1001, 4 * s["n_constraints"])
    acc0 = np.stack([rnd(2000 + k, n) for k in range(4)])      # a non-zero start: the sweep accumulates
    return cols, params.reshape(-1, 4), coeffs.reshape(-1, 4), acc0


_DEN = {}


def _denominators(log_size, log_expand):
    if (log_size, log_expand) not in _DEN:
        _DEN[(log_size, log_expand)] = air_model.domain_denominators(log_size, log_expand)
    return _DEN[(log_size, log_expand)]


def _case_words(prog, log_size, log_expand, inputs):
    cols, params, coeffs, acc0 = inputs
    den = _denominators(log_size, log_expand)
    table = [int(den[i << log_size]) for i in range(1 << log_expand)] + [0] * (8 - (1 << log_expand))
    head = [log_size, log_expand, prog.shape["n_cols"], prog.shape["n_params"], prog.shape["n_constraints"]] + table
    return np.concatenate([np.array(head, dtype=np.uint32), cols.ravel(), params.ravel().astype(np.uint32), coeffs.ravel().astype(np.uint32), acc0.ravel()])


def _model(prog, log_size, log_expand, inputs):
    cols, params, coeffs, acc0 = inputs
    n = 1 << (log_size + log_expand)
    got = air_model.run(prog.code, air_model.domain_reader(cols, log_size, log_expand), params.tolist(), coeffs.tolist(), n)
    got = air_model.q_mul(got, air_model.from_m(_denominators(log_size, log_expand)))
    return ((got + acc0) % np.uint64(P)).astype(np.uint32)


def _build_driver(prog, tmp_path, name, flags):
    src, exe = tmp_path / (name + "_generated.hip"), str(tmp_path / (name + "_driver"))
    src.write_text(prog.source())
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-DBFHIP_AIR_GEN_HOST", '-DBFHIP_AIR_GEN_FILE="%s"' % src, "-o", exe,
                           os.path.join(ROOT, "tests", "native", "air_codegen_host.cpp")])
    return exe


def _run_driver(exe, tmp_path, prog, todo):
    """todo: [(log_size, log_expand, inputs)] -> the accumulators of each case"""
    words = np.concatenate([np.array([len(todo)], dtype=np.uint32)] + [_case_words(prog, ls, le, inp) for ls, le, inp in todo])
    path_in, path_out = str(tmp_path / "cases.bin"), str(tmp_path / "acc.bin")
    words.tofile(path_in)
    r = subprocess.run([exe, path_in, path_out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    assert r.stdout.strip() == "cases: %d" % len(todo)
    out, got, at = np.fromfile(path_out, dtype=np.uint32), [], 0
    for ls, le, _ in todo:
        n = 1 << (ls + le)
        got.append(out[at: at + 4 * n].reshape(4, n))
        at += 4 * n
    assert at == len(out)
    return got


@pytest.mark.parametrize("name", NAMES)
def test_generated_source_as_host_code_equals_the_model(programs, tmp_path, name):
    """The emitted file compiled by g++ with the driver: accumulators == tests/air_model.py times the model's own denominators, word for word,
    at log_size 4 and 6 for log_expand 1, 2 and 3, from a non-zero accumulator, with random cells, with every cell / parameter word /
    coefficient word p - 1, and with every cell zero."""
    prog = programs[name]
    exe = _build_driver(prog, tmp_path, name, ["-O1"])
    todo = [(ls, le, _inputs(prog, ls, le, cells, 31 * ls + 7 * le)) for ls, le in SIZES for cells in CELLS]
    got = _run_driver(exe, tmp_path, prog, todo)
    changed = 0
    for (ls, le, inputs), acc in zip(todo, got):
        want = _model(prog, ls, le, inputs)
        assert np.array_equal(acc, want), (name, ls, le)
        changed += not np.array_equal(acc, inputs[3])
    assert changed >= len(SIZES)      # not only sweeps that add zero: every random case at least (uniform cells satisfy the synthetic AIR)


def test_generated_source_under_address_and_ub_sanitizers(programs, tmp_path):
    """The same driver as a stand-alone program under g++ -fsanitize=address,undefined, run directly (nothing is loaded into Python): the
    synthetic AIR, whose reads at offsets -2 .. +2 wrap around both halves of the domain, on buffers of exactly the contract's sizes."""
    prog = programs["synthetic_pm2"]
    exe = _build_driver(prog, tmp_path, "sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"])
    todo = [(ls, le, _inputs(prog, ls, le, cells, 5)) for ls, le in ((4, 1), (4, 3), (6, 2)) for cells in ("random", "p_minus_1")]
    for (ls, le, inputs), acc in zip(todo, _run_driver(exe, tmp_path, prog, todo)):
        assert np.array_equal(acc, _model(prog, ls, le, inputs)), (ls, le)


@pytest.mark.parametrize("name", NAMES)
def test_source_compiles_for_gfx950_without_a_device(programs, code_objects, name):
    """libhiprtc, driven directly, compiles each generated source for gfx950 with the options of bfhip_air_compile; the code object holds the
    kernel. The 13 components (at most 17 m and 6 q values live) take no scratch; whatever the caps program takes is printed."""
    co, seconds = code_objects[name]
    res = cases.resources(co)
    print(name, "instructions", programs[name].shape["n_instr"], "source bytes", len(programs[name].source()), "code object bytes", len(co),
          "compile %.2f s" % seconds, res)
    assert co[:4] == b"\x7fELF" and b"bfhip_air_generated" in co
    assert res["vgpr_count"] is not None and res["private_segment_fixed_size"] is not None and res["group_segment_fixed_size"] == 0
    if name != "caps":
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_count"] <= 128, res


def test_default_library_does_not_need_hiprtc_to_load(pkg):
    """libhiprtc is opened with dlopen at the first compile: no NEEDED entry of the default library (or of the test-hooks build) names it, so a
    host without it loses bfhip_air_compile and nothing else."""
    for lib in ("libbfhip.so", "libbfhip_testhooks.so"):
        out = subprocess.run(["readelf", "-d", os.path.join(ROOT, "stwo-brainfuck_amd", lib)], capture_output=True, text=True, check=True).stdout
        needed = [line for line in out.splitlines() if "NEEDED" in line]
        assert needed and any("libamdhip64" in line for line in needed), out
        assert not any("hiprtc" in line for line in needed), needed
