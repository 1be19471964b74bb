"""CPU: witness programs (include/bfhip.h "Witness programs") at everything a host without a GPU can check — bfhip_witness_program_eval_table
against the plain-Python model of tests/witness_model.py on random programs and tables (field edges, offsets that wrap a small domain several
times, INV0 over zeros and non-zeros), the Processor program of brainfuck_witness_program against bfhip_host_table column for column, every
refusal of bfhip_witness_program_create and of eval_table word for word, the older create calls still refusing the new opcodes, the prototypes
in the header and both generated bindings, the AirBuilder, and the host code under AddressSanitizer + UBSan in a stand-alone program
(tests/native/witness_host_sanitize.cpp)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import witness_model as model
from conftest import ROOT
from witness_model import AND, ARG, INV0, IS_ZERO, LT, M_ADD, M_COL, M_CONST, M_MUL, M_NEG, M_SUB, ROW, SHR, STORE, P

(Q_COL, Q_PARAM, Q_FROM_M, Q_ADD, Q_SUB, Q_MUL, Q_MULM, C_BASE, C_EXT, FRAC, END_COL, REL_WORD, REL_ENTRY) = range(6, 19)
HEAD = [M_CONST, 0, 1, 0]                                   # m[0] = 1
ST = [STORE, 0, 0, 0]                                       # output 0 = m[0]
OK = HEAD + ST
WHO = "bfhip_witness_program_create: instruction "
BASE_ONLY = ": a witness program is base field only (no q registers, no parameters)"
UNWRITTEN = "m register 5 is read before it is written"
HELLO1 = open(os.path.join(ROOT, "tests", "golden", "programs", "hello1.bf")).read()
COLLATZ = open(os.path.join(ROOT, "tests", "golden", "programs", "collatz.bf")).read()

# (what, code words, n_cols, n_out, n_args, the whole message behind "bfhip_witness_program_create: instruction "): one refused program per rule
REJECTED = [(name, HEAD + [op, 0, 0, 0] + ST, 4, 1, 1, "1: " + name + BASE_ONLY)
            for name, op in zip(("Q_COL", "Q_PARAM", "Q_FROM_M", "Q_ADD", "Q_SUB", "Q_MUL", "Q_MULM"), range(Q_COL, Q_MULM + 1))] + [
    ("C_BASE", HEAD + [C_BASE, 0, 0, 0] + ST, 4, 1, 1, "1: C_BASE: a witness program has no constraints"),
    ("C_EXT", HEAD + [C_EXT, 0, 0, 0] + ST, 4, 1, 1, "1: C_EXT: a witness program has no constraints"),
    ("FRAC", HEAD + [FRAC, 0, 0, 0] + ST, 4, 1, 1, "1: FRAC: a witness program has no fractions"),
    ("END_COL", OK + [END_COL, 0, 0, 0], 4, 1, 1, "2: END_COL: a witness program has no logUp columns"),
    ("REL_WORD", HEAD + [REL_WORD, 0, 0, 0] + ST, 4, 1, 1, "1: REL_WORD: a witness program has no relation entries"),
    ("REL_ENTRY", HEAD + [REL_ENTRY, 0, 0, 0] + ST, 4, 1, 1, "1: REL_ENTRY: a witness program has no relation entries"),
    ("opcode", OK + [27, 0, 0, 0], 4, 1, 1, "2: unknown opcode 27"),
    ("offset 17", [M_COL, 0, 0, 17] + ST, 4, 1, 1, "0: offset 17 out of range (|offset| <= 16)"),
    ("offset -17", [M_COL, 0, 0, (-17) & 0xFFFFFFFF] + ST, 4, 1, 1, "0: offset -17 out of range (|offset| <= 16)"),
    ("m register range", [M_CONST, 96, 1, 0] + OK, 4, 1, 1, "0: m register 96 out of range (BFHIP_AIR_MAX_M_REGS = 96)"),
    ("own destination range", HEAD + [ROW, 96, 0, 0] + ST, 4, 1, 1, "1: m register 96 out of range (BFHIP_AIR_MAX_M_REGS = 96)"),
    ("own source range", HEAD + [INV0, 0, 200, 0] + ST, 4, 1, 1, "1: m register 200 out of range (BFHIP_AIR_MAX_M_REGS = 96)"),
    ("M_ADD reads an unwritten register", HEAD + [M_ADD, 1, 0, 5] + ST, 4, 1, 1, "1: " + UNWRITTEN),
    ("INV0 reads an unwritten register", HEAD + [INV0, 1, 5, 0] + ST, 4, 1, 1, "1: " + UNWRITTEN),
    ("IS_ZERO reads an unwritten register", HEAD + [IS_ZERO, 1, 5, 0] + ST, 4, 1, 1, "1: " + UNWRITTEN),
    ("LT reads an unwritten register", HEAD + [LT, 1, 0, 5] + ST, 4, 1, 1, "1: " + UNWRITTEN),
    ("AND reads an unwritten register", HEAD + [AND, 1, 5, 1] + ST, 4, 1, 1, "1: " + UNWRITTEN),
    ("SHR reads an unwritten register", HEAD + [SHR, 1, 5, 1] + ST, 4, 1, 1, "1: " + UNWRITTEN),
    ("STORE reads an unwritten register", HEAD + [STORE, 0, 5, 0], 4, 1, 1, "1: " + UNWRITTEN),
    ("col within n_cols", [M_COL, 1, 4, 0] + OK, 4, 1, 1, "0: column 4 out of range (the program has 4 columns)"),
    ("col without columns", [M_COL, 1, 0, 0] + OK, 0, 1, 1, "0: column 0 out of range (the program has 0 columns)"),
    ("v < p", [M_CONST, 0, P, 0] + ST, 4, 1, 1, "0: constant 2147483647 is not a canonical M31 (v < 2^31 - 1)"),
    ("arg index", HEAD + [ARG, 1, 1, 0] + ST, 4, 1, 1, "1: ARG: arg 1 out of range (the program has 1 args)"),
    ("arg without args", HEAD + [ARG, 1, 0, 0] + ST, 4, 1, 0, "1: ARG: arg 0 out of range (the program has 0 args)"),
    ("cap: args", OK, 4, 1, 65, "0: more than BFHIP_AIR_MAX_PARAMS (64) args"),
    ("AND immediate", HEAD + [AND, 1, 0, 1 << 31] + ST, 4, 1, 1, "1: AND: immediate 2147483648 out of range (imm < 2^31)"),
    ("SHR immediate", HEAD + [SHR, 1, 0, 31] + ST, 4, 1, 1, "1: SHR: immediate 31 out of range (imm <= 30)"),
    ("no outputs", OK, 4, 0, 1, "0: 0 outputs, not 1 to BFHIP_AIR_MAX_COLUMNS (256)"),
    ("cap: outputs", OK, 4, 257, 1, "0: 257 outputs, not 1 to BFHIP_AIR_MAX_COLUMNS (256)"),
    ("store index", HEAD + [STORE, 1, 0, 0], 4, 1, 1, "1: STORE: output 1 out of range (the program has 1 outputs)"),
    ("second store", OK + ST, 4, 1, 1, "2: STORE: output 0 is stored a second time"),
    ("output never stored", OK, 4, 2, 1, "2: the program ends with output 1 never stored"),
    ("nothing stored", HEAD, 4, 1, 1, "1: the program ends with output 0 never stored"),
    ("cap: instructions", HEAD * 4096 + ST, 4, 1, 1, "4096: more than BFHIP_AIR_MAX_INSTRUCTIONS (4096) instructions"),
    ("cap: columns", OK, 257, 1, 1, "0: more than BFHIP_AIR_MAX_COLUMNS (256) columns"),
    ("length", OK + [M_NEG, 1, 0], 4, 1, 1, "2: the program is 11 words, not a positive multiple of 4"),
    ("empty", [], 4, 1, 1, "0: the program is 0 words, not a positive multiple of 4"),
]


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_validator_refuses_one_program_per_rule(pkg, case):
    _, code, n_cols, n_out, n_args, rule = case
    with pytest.raises(pkg.BfhipError) as e:
        pkg.WitnessProgram(code, n_cols, n_out, n_args)
    assert str(e.value) == WHO + rule


def test_validator_accepts_what_the_rules_allow(pkg):
    # the caps themselves: 4096 instructions, 256 columns, 256 outputs, 64 args, the last register, both extreme offsets and immediates
    body = [M_COL, 95, 255, 16, M_COL, 0, 0, (-16) & 0xFFFFFFFF, ARG, 1, 63, 0, AND, 2, 95, 0x7FFFFFFF, SHR, 3, 95, 30]
    stores = [w for k in range(256) for w in (STORE, k, 95, 0)]
    code = [M_CONST, 94, P - 1, 0] * (4096 - 5 - 256) + body + stores
    prog = pkg.WitnessProgram(code, 256, 256, 64)
    assert prog.shape() == {"n_cols": 256, "n_out": 256, "n_args": 64, "n_instr": 4096, "m_regs": 96, "min_offset": -16, "max_offset": 16}
    assert pkg.WitnessProgram(OK, 0, 1, 0).shape() == {"n_cols": 0, "n_out": 1, "n_args": 0, "n_instr": 2, "m_regs": 1, "min_offset": 0, "max_offset": 0}
    assert pkg.WitnessProgram(OK, 0, 1, 0).eval_table(np.zeros((2, 0), dtype=np.uint32)).tolist() == [[1], [1]]


def test_older_create_calls_refuse_the_new_opcodes(pkg):
    for op in range(ARG, STORE + 2):
        with pytest.raises(pkg.BfhipError, match=r"^bfhip_air_create: instruction 2: unknown opcode %d$" % op):
            pkg.AirProgram([M_CONST, 0, 1, 0, C_BASE, 0, 0, 0, op, 0, 0, 0], 4, 1)
        with pytest.raises(pkg.BfhipError, match=r"^bfhip_logup_create: instruction 3: unknown opcode %d$" % op):
            pkg.LogupProgram([Q_PARAM, 0, 0, 0, FRAC, 0, 0, 0, END_COL, 0, 0, 0, op, 0, 0, 0], 4, 1)
        with pytest.raises(pkg.BfhipError, match=r"^bfhip_relation_program_create: instruction 3: unknown opcode %d$" % op):
            pkg.RelationProgram(HEAD + [REL_WORD, 0, 0, 0, REL_ENTRY, 0, 0, 0, op, 0, 0, 0], 4, [1])


def _check_against_model(pkg, code, table, args, n_cols, n_out, inv0_seen=None):
    prog = pkg.WitnessProgram(code, n_cols, n_out, len(args))
    got = prog.eval_table(np.array(table, dtype=np.uint32).reshape(len(table), n_cols), args)
    want = model.eval_table(code, table, args, n_out, inv0_seen)
    assert got.tolist() == want
    assert int(got.max()) < P


@pytest.mark.parametrize("log_size", [1, 2, 5, 6])
def test_eval_table_equals_the_model_on_random_programs(pkg, log_size):
    inv0_seen = []
    for seed in range(12):
        rng = model.random.Random(1000 * log_size + seed)
        n_cols, n_out, n_args = 1 + rng.randrange(5), 1 + rng.randrange(4), rng.randrange(3)
        offsets = (0,) if seed % 2 else (0, 0, 1, -1, 2, -2, 16, -16)
        code = model.random_program(rng, n_cols, n_out, n_args, 40, offsets)
        args = [rng.choice([0, 1, P - 1, rng.randrange(P)]) for _ in range(n_args)]
        for fill in (None, P - 1, 0):
            _check_against_model(pkg, code, model.random_table(rng, log_size, n_cols, fill), args, n_cols, n_out, inv0_seen)
    assert 0 in inv0_seen and any(v > 1 for v in inv0_seen) and P - 1 in inv0_seen, "the INV0 inputs must hold zeros and non-zeros"


@pytest.mark.parametrize("log_size", [1, 2, 3])
@pytest.mark.parametrize("off", [1, -1, 2, -2, 16, -16])
def test_offsets_that_wrap_a_small_domain(pkg, log_size, off):
    """One column read at the offset and stored: out[r] = table[(r + off) mod n]; +-16 wraps a 2-row domain eight times."""
    n = 1 << log_size
    table = [[100 + r] for r in range(n)]
    code = [M_COL, 0, 0, off & 0xFFFFFFFF, ROW, 1, 0, 0, M_ADD, 2, 0, 1, STORE, 0, 0, 0, STORE, 1, 2, 0]
    got = pkg.WitnessProgram(code, 1, 2, 0).eval_table(np.array(table, dtype=np.uint32))
    assert got.tolist() == [[100 + (r + off) % n, 100 + (r + off) % n + r] for r in range(n)] == model.eval_table(code, table, [], 2)


def _processor(pkg, regs7, code_words):
    """(the witness program's 9 columns from the six register columns, bfhip_host_table's Processor table) for one register trace."""
    L = pkg.lib()
    regs7 = np.ascontiguousarray(regs7, dtype=np.uint32)
    words = np.ascontiguousarray(code_words, dtype=np.uint32)
    nr, nc = ctypes.c_size_t(), ctypes.c_size_t()
    args = (regs7.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(regs7.shape[0]), words.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(words.size), 3)
    assert L.bfhip_host_table(*args, None, ctypes.c_size_t(0), ctypes.byref(nr), ctypes.byref(nc)) == 0
    want = np.zeros((nr.value, nc.value), dtype=np.uint32)
    assert L.bfhip_host_table(*args, want.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(want.size), ctypes.byref(nr), ctypes.byref(nc)) == 0
    n_real, n = regs7.shape[0], want.shape[0]
    padded = np.concatenate([regs7[:, :6], np.repeat(regs7[-1:, :6], n - n_real, axis=0)])      # what repeat_last ingests
    prog, names = pkg.brainfuck_witness_program("processor")
    assert names == ("clk", "ip", "ci", "ni", "mp", "mv", "mvi", "d", "next_clk")
    return prog.eval_table(padded, [n_real]), want


@pytest.mark.parametrize("name,code,inp,n_prefix", [("hello1", HELLO1, b"", None), ("collatz", COLLATZ, bytes([55, 10]), None),
                                                    ("prefix of 64: no padding", COLLATZ, bytes([55, 10]), 64), ("prefix of 65: almost all padding", COLLATZ, bytes([55, 10]), 65)])
def test_processor_program_equals_the_host_table_column_for_column(pkg, name, code, inp, n_prefix):
    regs = pkg.host_run(code, inp)[1]
    assert regs.shape[0] > 65
    regs = regs if n_prefix is None else regs[:n_prefix]
    got, want = _processor(pkg, regs, pkg.host_compile(code))
    assert want.shape == (64 if n_prefix == 64 else 128 if n_prefix == 65 else want.shape[0], 9)
    for k in range(9):
        assert got[:, k].tolist() == want[:, k].tolist(), (name, k)
    assert (want[:, 7].sum() == 0) == (n_prefix == 64) and int(want[-1, 8]) == int(want[-1, 0]) + 1
    assert (want[: regs.shape[0], 5] == 0).any() and (want[: regs.shape[0], 5] != 0).any()      # mvi inverts zeros and non-zeros


def test_processor_program_uses_every_own_opcode_but_and_and_shr(pkg):
    prog = pkg.brainfuck_witness_program("processor")[0]
    assert set(prog.code[0::4]) == {M_COL, M_CONST, M_ADD, M_SUB, M_MUL, ARG, ROW, INV0, IS_ZERO, LT, STORE}
    assert prog.shape()["n_cols"] == 6 and prog.shape()["n_out"] == 9 and prog.shape()["n_args"] == 1 and (prog.shape()["min_offset"], prog.shape()["max_offset"]) == (0, 1)
    regs = model.processor_registers(model.random.Random(5), 37)
    table = regs + [regs[-1]] * (64 - 37)
    assert prog.eval_table(np.array(table, dtype=np.uint32), [37]).tolist() == model.processor_table(regs) == model.eval_table(prog.code, table, [37], 9)
    with pytest.raises(ValueError, match="processor"):
        pkg.brainfuck_witness_program("memory")


def test_eval_table_refusals(pkg):
    prog = pkg.WitnessProgram([ARG, 0, 0, 0, M_COL, 1, 0, 0] + ST, 1, 1, 1)
    L, who = pkg.lib(), "bfhip_witness_program_eval_table: "
    table, out, args = (ctypes.c_uint32 * 4)(1, 2, 3, P), (ctypes.c_uint32 * 4)(*[7] * 4), (ctypes.c_uint32 * 1)(5)
    f = L.bfhip_witness_program_eval_table
    cases = [((None, 1, table, args, 1, out), "null argument"), ((prog._h, 1, None, args, 1, out), "null argument"), ((prog._h, 1, table, None, 1, out), "null argument"),
             ((prog._h, 1, table, args, 1, None), "null argument"), ((prog._h, 0, table, args, 1, out), "log_size 0 is outside 1..30"),
             ((prog._h, 31, table, args, 1, out), "log_size 31 is outside 1..30"), ((prog._h, 1, table, args, 0, out), "0 args, the program has 1"),
             ((prog._h, 2, table, args, 1, out), "row 3, column 0: 2147483647 is not a canonical M31 value")]
    for call, rule in cases:
        assert f(*call) == -1 and L.bfhip_last_error().decode() == who + rule
    args[0] = P
    assert f(prog._h, 1, table, args, 1, out) == -1 and L.bfhip_last_error().decode() == who + "arg 0: 2147483647 is not a canonical M31 value"
    assert list(out) == [7] * 4      # nothing was written
    args[0] = 5
    assert f(prog._h, 1, table, args, 1, out) == 0 and list(out) == [5, 5, 7, 7]


def test_builder_round_trip(pkg):
    b = pkg.AirBuilder()
    x, nxt = b.col(0), b.col(0, 1)
    byte = b.bit_and(x, 0xFF)
    b.store(0, b.inv0(x))
    b.store(1, b.is_zero(x - nxt))
    b.store(2, b.lt(b.row(), b.arg(1)) * byte + b.shr(x, 8))
    prog = b.witness_program(3)
    assert prog.shape()["n_cols"] == 1 and prog.shape()["n_args"] == 2 and prog.shape()["n_out"] == 3 and prog.shape()["max_offset"] == 1
    table = [[0], [0x1234], [P - 1], [0x1234]]
    want = [[pow(v, P - 2, P), int(v == table[(r + 1) % 4][0]), (int(r < 2) * (v & 0xFF) + (v >> 8)) % P] for r, (v,) in enumerate(table)]
    assert prog.eval_table(np.array(table, dtype=np.uint32), [9, 2]).tolist() == want == model.eval_table(prog.code, table, [9, 2], 3)
    with pytest.raises(ValueError, match="base-field"):
        b.store(0, b.param(0))
    with pytest.raises(ValueError, match="base-field"):
        b.inv0(b.secure_col(0))
    c = pkg.AirBuilder()
    c.constraint(c.col(0))
    c.store(0, c.col(0))
    with pytest.raises(pkg.BfhipError, match="a witness program has no constraints"):
        c.witness_program(1)


def test_prototypes_in_header_and_both_generated_bindings(pkg):
    hdr = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    rust_lib = open(os.path.join(ROOT, "bindings", "rust", "lib.rs")).read()
    gen = open(os.path.join(ROOT, "stwo-brainfuck_amd", "_abi_gen.py")).read()
    for sym in ("create", "destroy", "shape", "eval_table", "generate"):
        name = "bfhip_witness_program_" + sym
        assert re.search(r"^int32_t %s\(" % name, hdr, flags=re.M) and "pub fn %s(" % name in rust and "sys::" + name in rust_lib and '"%s"' % name in gen, name
        assert getattr(pkg.lib(), name)
    assert "pub struct BfhipWitnessProgram" in rust and "pub struct WitnessProgram" in rust_lib
    consts = {"BFHIP_WIT_ARG": 19, "BFHIP_WIT_ROW": 20, "BFHIP_WIT_INV0": 21, "BFHIP_WIT_IS_ZERO": 22, "BFHIP_WIT_LT": 23, "BFHIP_WIT_AND": 24, "BFHIP_WIT_SHR": 25,
              "BFHIP_WIT_STORE": 26}
    for name, v in consts.items():
        assert re.search(r"\b%s = %d\b" % (name, v), hdr) and "pub const %s: u32 = %d;" % (name, v) in rust and getattr(pkg, name[len("BFHIP_"):]) == v
    assert (ARG, ROW, INV0, IS_ZERO, LT, AND, SHR, STORE) == tuple(consts.values())
    assert hasattr(pkg, "WitnessProgram") and hasattr(pkg.Context, "witness_program_generate") and hasattr(pkg.AirBuilder, "witness_program")


def test_host_code_under_address_and_ub_sanitizers(pkg, tmp_path):
    """tests/native/witness_host_sanitize.cpp (its own main) compiled together with csrc/witness_program_host.hip as plain C++ under g++
    -fsanitize=address,undefined and run directly: the Processor program, the caps program, every refused program above and 10 000 seeded
    random word arrays go through bfhip_witness_program_create, and whatever is accepted through _shape and _eval_table with exactly fitting
    buffers."""
    exe = str(tmp_path / "witness_host_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "witness_host_sanitize.cpp"),
                           "-x", "c++", os.path.join(ROOT, "stwo-brainfuck_amd", "csrc", "witness_program_host.hip")])
    processor = pkg.brainfuck_witness_program("processor")[0]
    caps = [M_COL, 95, 255, 16, ARG, 1, 63, 0] + [w for k in range(256) for w in (STORE, k, 95, 0)]
    lines = ["1 6 9 1 " + " ".join(str(w) for w in processor.code), "1 256 256 64 " + " ".join(str(w) for w in caps)]
    for _, code, n_cols, n_out, n_args, _ in REJECTED:
        lines.append("0 %d %d %d %s" % (n_cols, n_out, n_args, " ".join(str(w) for w in code)))
    path = tmp_path / "programs.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    out = r.stdout.strip().splitlines()
    assert out[0] == "listed: 2 accepted, %d refused, 0 unexpected" % len(REJECTED), out
    m = re.fullmatch(r"random: (\d+) accepted, (\d+) refused of 10000", out[1])
    assert m and int(m.group(1)) + int(m.group(2)) == 10000 and int(m.group(2)) > 3000 and int(m.group(1)) > 100, out
    assert re.fullmatch(r"edges refused (\d+) of \1", out[2]), out
