"""Shared by tests/test_air_codegen_cpu.py and tests/test_gpu_air_compiled.py: the programs the compiled-kernel tests run (the 13 Brainfuck
programs, the synthetic AIRs with offsets, a seeded random program at the caps), libhiprtc driven directly through ctypes (so that the
generated sources can be compiled for gfx950 on a host without a GPU), and the resource figures of a code object's metadata note."""
import ctypes
import random
import time

import air_model
from air_model import (M_COL, M_CONST, M_ADD, M_SUB, M_MUL, M_NEG, Q_COL, Q_PARAM, Q_FROM_M, Q_ADD, Q_SUB, Q_MUL, Q_MULM, C_BASE, C_EXT)

P = (1 << 31) - 1
RTC_OPTIONS = ("-O3", "-std=c++17", "-Wno-pragma-once-outside-header")      # what bfhip_air_compile passes, behind --offload-arch


def caps_program(seed, n_instr=4096, n_cols=256, n_params=64):
    """A random program of exactly n_instr instructions in which all 96 m and all 24 q registers hold a value that is still read later — at
    the end of the random part every one of the 120 is live — with 64 constraints (base and extension interleaved) and column reads at offsets
    up to +-16. Layout: fill every register (120 instructions), random arithmetic over the whole files with constraints strewn in, then both
    files summed into m0 and q0 (95 + 23 instructions: every register is read) and the last constraints on the sums.
    Returns (code words, n_cols, n_params, n_constraints = 64)."""
    rng = random.Random(seed)
    code, n_cons = [], 0
    off = lambda: rng.choice([0, 0, 1, -1, 2, -2, 16, -16, rng.randrange(-16, 17)]) & 0xFFFFFFFF
    for r in range(96):
        code += [M_COL, r, rng.randrange(n_cols), off()] if r % 4 else [M_CONST, r, rng.choice([0, 1, P - 1, rng.randrange(P)]), 0]
    for r in range(24):
        code += [Q_COL, r, rng.randrange(n_cols - 3), off()] if r % 2 else [Q_PARAM, r, rng.randrange(n_params), 0]
    n_tail = 95 + 23 + 4
    n_random = n_instr - len(code) // 4 - n_tail
    assert n_random >= 60
    strewn = sorted(rng.sample(range(n_random), 60))      # where the first 60 constraints go
    for i in range(n_random):
        if strewn and strewn[0] == i:
            strewn.pop(0)
            code += [C_BASE, 0, rng.randrange(96), 0] if rng.random() < 0.7 else [C_EXT, 0, rng.randrange(24), 0]
            n_cons += 1
            continue
        op = rng.choice([M_COL, M_CONST, M_ADD, M_ADD, M_SUB, M_SUB, M_MUL, M_MUL, M_MUL, M_NEG, Q_COL, Q_PARAM, Q_FROM_M, Q_ADD, Q_SUB, Q_MUL, Q_MULM])
        md, qd, ma, mb, qa, qb = rng.randrange(96), rng.randrange(24), rng.randrange(96), rng.randrange(96), rng.randrange(24), rng.randrange(24)
        code += {M_COL: [op, md, rng.randrange(n_cols), off()], M_CONST: [op, md, rng.randrange(P), 0], M_ADD: [op, md, ma, mb], M_SUB: [op, md, ma, mb],
                 M_MUL: [op, md, ma, mb], M_NEG: [op, md, ma, 0], Q_COL: [op, qd, rng.randrange(n_cols - 3), off()], Q_PARAM: [op, qd, rng.randrange(n_params), 0],
                 Q_FROM_M: [op, qd, ma, 0], Q_ADD: [op, qd, qa, qb], Q_SUB: [op, qd, qa, qb], Q_MUL: [op, qd, qa, qb], Q_MULM: [op, qd, qa, mb]}[op]
    for r in range(1, 96):
        code += [M_ADD, 0, 0, r]
    for r in range(1, 24):
        code += [Q_ADD, 0, 0, r]
    code += [C_BASE, 0, 0, 0, C_EXT, 0, 0, 0, C_BASE, 0, 0, 0, C_EXT, 0, 0, 0]
    assert len(code) == 4 * n_instr
    return code, n_cols, n_params, n_cons + 4


def synthetic_wide_program(pkg):
    """The synthetic AIR's shape with the largest offsets the format has: nxt = a[+16], prv = a[-16], and a degree-2 product. Columns
    a, b, out, nxt, prv. On a trace of 2^4 rows offset 16 is a whole turn of the trace coset: both copies are the column itself."""
    b = pkg.AirBuilder()
    a = b.col(0)
    b.constraint(b.col(2) - a * b.col(1))
    b.constraint(b.col(3) - b.col(0, 16))
    b.constraint(b.col(4) - b.col(0, -16))
    return b.program()


def constraint_run_program(pkg, n_base, interleave_ext=False):
    """n_base base-field constraints in a row over three columns (the lazy reduction folds before every fifth product); with interleave_ext
    an extension constraint after every third base one (it must not reset the count). One parameter."""
    b = pkg.AirBuilder()
    x, y, z = b.col(0), b.col(1), b.col(2)
    for j in range(n_base):
        b.constraint(x * y + z * (j + 1) - (x if j % 2 else y))
        if interleave_ext and j % 3 == 2:
            b.constraint(b.param(0) * x - b.secure_col(3) * y)
    return b.program(n_cols=7, n_params=1)


# ---- libhiprtc through ctypes: compiling without a device ----------------------------------------------------------------------------------
_rtc = None


def hiprtc():
    global _rtc
    if _rtc is None:
        _rtc = ctypes.CDLL("libhiprtc.so.7")      # a missing library is an error with the loader's message, not a skip
        _rtc.hiprtcGetErrorString.restype = ctypes.c_char_p
    return _rtc


def rtc_compile(source, arch="gfx950"):
    """(code object bytes, seconds). Raises with the compiler's log."""
    rtc = hiprtc()
    prog = ctypes.c_void_p()
    r = rtc.hiprtcCreateProgram(ctypes.byref(prog), source.encode(), b"bfhip_air_generated.hip", 0, None, None)
    assert r == 0, rtc.hiprtcGetErrorString(r)
    try:
        opts = [("--offload-arch=" + arch).encode()] + [o.encode() for o in RTC_OPTIONS]
        t0 = time.perf_counter()
        r = rtc.hiprtcCompileProgram(prog, len(opts), (ctypes.c_char_p * len(opts))(*opts))
        seconds = time.perf_counter() - t0
        n = ctypes.c_size_t()
        rtc.hiprtcGetProgramLogSize(prog, ctypes.byref(n))
        log = ctypes.create_string_buffer(n.value + 1)
        rtc.hiprtcGetProgramLog(prog, log)
        assert r == 0, (rtc.hiprtcGetErrorString(r), log.value.decode()[:3000])
        assert rtc.hiprtcGetCodeSize(prog, ctypes.byref(n)) == 0 and n.value > 0
        code = ctypes.create_string_buffer(n.value)
        assert rtc.hiprtcGetCode(prog, code) == 0
        return code.raw, seconds
    finally:
        rtc.hiprtcDestroyProgram(ctypes.byref(prog))


def metadata_count(code_object, key):
    """An integer of the kernel's metadata note (msgpack: the key, then a fixint, uint8, uint16 or uint32); None if absent."""
    i = code_object.find(key.encode())
    if i < 0:
        return None
    v = code_object[i + len(key): i + len(key) + 5]
    if v[0] < 0x80:
        return v[0]
    return {0xCC: lambda: v[1], 0xCD: lambda: (v[1] << 8) | v[2], 0xCE: lambda: int.from_bytes(v[1:5], "big")}.get(v[0], lambda: None)()


def resources(code_object):
    return {k: metadata_count(code_object, "." + k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
