"""CPU: fraction programs (include/bfhip.h "Fraction programs") at everything a host without a GPU can check — the validator behind
bfhip_logup_create (one refused program per rule, every Brainfuck fraction program accepted, bfhip_air_create still refusing the two new
opcodes), the numpy model of tests/logup_model.py anchored word for word on the oracle's gen_interaction_trace for the 13 components, and
the new host code under AddressSanitizer + UBSan in a stand-alone program (tests/native/logup_host_sanitize.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import logup_model
from conftest import ROOT, splitmix_column

P = (1 << 31) - 1
ALL_OPS = ("+++>,<[>+.<-]", b"\x01")       # tests/test_gpu_air_program.py
HELLO = ("++++++++++[>+++++++>++++++++++>+++>+<<<<-]>++.>+.+++++++..+++.>++.<<+++++++++++++++.>.+++.------.--------.>+.>.", b"")
(M_COL, M_CONST, M_ADD, M_SUB, M_MUL, M_NEG, Q_COL, Q_PARAM, Q_FROM_M, Q_ADD, Q_SUB, Q_MUL, Q_MULM, C_BASE, C_EXT, FRAC, END_COL) = range(17)
NEG1 = 0xFFFFFFFF
HEAD = [Q_PARAM, 0, 0, 0]                      # q[0] = params[0]
OK = HEAD + [FRAC, 0, 0, 0, END_COL, 0, 0, 0]  # one column of one fraction: params[0] / params[0]
ONE_COL = [FRAC, 0, 0, 0, END_COL, 0, 0, 0]
ONE_COL_23 = [END_COL, 0, 0, 0, FRAC, 0, 23, 22]      # closes a column and opens the next with q[23] / q[22]

# (what, code words, n_cols, n_params, instruction index the message names, a word of the rule): one refused program per rule
REJECTED = [
    ("opcode", [17, 0, 0, 0] + OK, 4, 1, 0, "unknown opcode 17"),
    ("C_BASE", [M_CONST, 0, 1, 0, C_BASE, 0, 0, 0] + OK, 4, 1, 1, "C_BASE: a fraction program has no constraints"),
    ("C_EXT", HEAD + [C_EXT, 0, 0, 0] + ONE_COL, 4, 1, 1, "C_EXT: a fraction program has no constraints"),
    ("M_COL at an offset", [M_COL, 0, 0, 1] + OK, 4, 1, 0, "offset 1"),
    ("Q_COL at an offset", [Q_COL, 0, 0, NEG1] + OK, 4, 1, 0, "offset -1"),
    ("m register range", [M_CONST, 96, 1, 0] + OK, 4, 1, 0, "m register 96 out of range"),
    ("m source register range", [M_CONST, 0, 1, 0, M_ADD, 0, 0, 200] + OK, 4, 1, 1, "m register 200 out of range"),
    ("q register range", [Q_PARAM, 24, 0, 0] + OK, 4, 1, 0, "q register 24 out of range"),
    ("m read before write", [M_CONST, 0, 1, 0, M_ADD, 1, 0, 5] + OK, 4, 1, 1, "m register 5 is read before it is written"),
    ("q read before write", HEAD + [Q_MUL, 1, 0, 3] + ONE_COL, 4, 1, 1, "q register 3 is read before it is written"),
    ("fraction reads an unwritten numerator", HEAD + [FRAC, 0, 1, 0, END_COL, 0, 0, 0], 4, 1, 1, "q register 1 is read before it is written"),
    ("fraction reads an unwritten denominator", HEAD + [FRAC, 0, 0, 2, END_COL, 0, 0, 0], 4, 1, 1, "q register 2 is read before it is written"),
    ("fraction register range", HEAD + [FRAC, 0, 0, 24, END_COL, 0, 0, 0], 4, 1, 1, "q register 24 out of range"),
    ("col within n_cols", [M_COL, 1, 4, 0] + OK, 4, 1, 0, "column 4 out of range"),
    ("col + 3 within n_cols", [Q_COL, 0, 2, 0] + OK, 5, 1, 0, "column 2..5 out of range"),
    ("col + 3 without wrap-around", [Q_COL, 0, 0xFFFFFFFE, 0] + OK, 5, 1, 0, "out of range"),
    ("parameter index", [Q_PARAM, 0, 1, 0] + OK, 4, 1, 0, "parameter 1 out of range"),
    ("v < p", [M_CONST, 0, P, 0] + OK, 4, 1, 0, "not a canonical M31"),
    ("FRAC without END_COL", OK + [FRAC, 0, 0, 0], 4, 1, 4, "a FRAC that no END_COL follows"),
    ("END_COL without FRAC", OK + [END_COL, 0, 0, 0], 4, 1, 3, "no fraction since the previous END_COL"),
    ("END_COL first", HEAD + [END_COL, 0, 0, 0] + ONE_COL, 4, 1, 1, "no fraction since the previous END_COL"),
    ("no column", HEAD + [M_CONST, 0, 1, 0], 4, 1, 2, "without a logUp column"),
    ("cap: logUp columns", HEAD + ONE_COL * 9, 4, 1, 17, "BFHIP_LOGUP_MAX_COLUMNS"),
    ("cap: fractions", HEAD + [FRAC, 0, 0, 0] * 33 + [END_COL, 0, 0, 0], 4, 1, 33, "BFHIP_LOGUP_MAX_FRACTIONS"),
    ("cap: instructions", [M_CONST, 0, 1, 0] * 4094 + OK, 4, 1, 4096, "BFHIP_AIR_MAX_INSTRUCTIONS"),
    ("cap: columns", OK, 257, 1, 0, "BFHIP_AIR_MAX_COLUMNS"),
    ("cap: parameters", OK, 4, 65, 0, "BFHIP_AIR_MAX_PARAMS"),
    ("length", OK + [M_NEG, 1, 0], 4, 1, 3, "multiple of 4"),
]


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_validator_refuses_one_program_per_rule(pkg, case):
    _, code, n_cols, n_params, at, rule = case
    with pytest.raises(pkg.BfhipError) as e:
        pkg.LogupProgram(code, n_cols, n_params)
    msg = str(e.value)
    print(msg)
    assert re.match(r"bfhip_logup_create: instruction %d: " % at, msg) and rule in msg, msg


def test_validator_accepts_what_the_rules_allow(pkg):
    # the caps themselves: 4096 instructions, 8 columns, 32 fractions, 256 columns, 64 parameters, the last register of each file
    code = [M_CONST, 95, P - 1, 0] * (4096 - 3 - 40) + [M_COL, 0, 255, 0, Q_COL, 23, 252, 0, Q_PARAM, 22, 63, 0] + [FRAC, 9, 23, 22] * 25 + ONE_COL_23 * 7 + [END_COL, 7, 7, 7]
    prog = pkg.LogupProgram(code, 256, 64)
    assert prog.shape == {"n_cols": 256, "n_params": 64, "n_logup_cols": 8, "n_fractions": 32, "n_instr": 4096, "m_regs": 96, "q_regs": 24}
    assert pkg.LogupProgram(OK, 0, 1).shape["n_logup_cols"] == 1      # an empty column list
    # bfhip_air_create keeps treating the two opcodes as unknown, in its own words
    for op in (FRAC, END_COL):
        with pytest.raises(pkg.BfhipError, match=r"^bfhip_air_create: instruction 2: unknown opcode %d$" % op):
            pkg.AirProgram([M_CONST, 0, 1, 0, C_BASE, 0, 0, 0, op, 0, 0, 0], 4, 1)


def test_builder_writes_fractions_and_columns(pkg):
    b = pkg.AirBuilder()
    a, t = b.col(0), b.col(1)
    b.frac(1, b.param(1) * a - b.param(0))          # a base-field numerator is lifted
    b.end_column()
    b.frac(-b.col(2), b.param(1) * t - b.param(0))
    b.frac(b.param(2), t)                           # a base-field denominator too
    b.end_column()
    prog = b.logup_program()
    assert (prog.shape["n_cols"], prog.shape["n_params"], prog.shape["n_logup_cols"], prog.shape["n_fractions"]) == (3, 3, 2, 3)
    ops = [prog.code[i] for i in range(0, len(prog.code), 4)]
    assert ops.count(FRAC) == 3 and ops.count(END_COL) == 2 and ops[-1] == END_COL and Q_FROM_M in ops and C_BASE not in ops and C_EXT not in ops
    with pytest.raises(pkg.BfhipError, match="a fraction program has no constraints"):
        b.constraint(a)
        b.logup_program()


def test_brainfuck_programs_are_accepted_and_shaped_like_the_components(pkg):
    import ctypes
    for k in range(13):
        a, nl, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        assert pkg.lib().bfhip_component_shape(k, ctypes.byref(a), ctypes.byref(nl), ctypes.byref(c)) == 0
        prog, names = pkg.brainfuck_logup_program(k)
        s = prog.shape
        assert s["n_cols"] == a.value and s["n_logup_cols"] == s["n_fractions"] == nl.value == (3 if k == 3 else 1), (k, s)
        assert s["n_params"] == len(names) == 24 == pkg.BRAINFUCK_LOGUP_N_PARAMS and s["m_regs"] <= 16 and s["q_regs"] <= 4


def _elems(seed):
    e = splitmix_column(seed, 24)
    e[e == 0] = 1
    return e.tolist()


@pytest.mark.parametrize("name,prog", [("all_ops", ALL_OPS), ("hello", HELLO)])
def test_model_equals_the_oracle_on_the_13_brainfuck_programs(pkg, _oracle, name, prog):
    """The anchor of tests/logup_model.py: for the 13 brainfuck_logup_programs on the tables of two Brainfuck programs, the model on the
    row-granular main columns at shift 4 equals orc_logup_generate (gen_interaction_trace) word for word, claimed sums included — earlier
    columns, the coset-order prefix sum of the last one, and its last element."""
    elems = _elems(77)
    logs = set()
    for comp in range(13):
        rows = np.ascontiguousarray(_oracle.table(prog[0], prog[1], comp).T)
        want, claimed = _oracle.logup_generate(comp, rows, elems)
        program, _ = pkg.brainfuck_logup_program(comp)
        log_size = int(np.log2(rows.shape[1])) + 4
        params = pkg.brainfuck_air_params(elems, [0, 0, 0, 0])[:24]
        got, got_claimed, zeros = logup_model.generate(program.code, rows, [4] * len(rows), params, log_size)
        assert zeros == [] and got_claimed == claimed and np.array_equal(got, want), comp
        logs.add(log_size)
    assert min(logs) == 4 and max(logs) >= 9


def test_model_inverse_and_coset_order():
    x = np.stack([splitmix_column(5 + k, 64).astype(np.uint64) for k in range(4)])
    x[:, 0] = (P - 1, P - 1, P - 1, P - 1); x[:, 1] = (0, 0, 0, 1); x[:, 2] = (1, 0, 0, 0)
    one = logup_model.q_mul(x, logup_model.q_inv(x))
    assert np.array_equal(one, logup_model.q((1, 0, 0, 0), 64))
    # conftest.logup_expected_dummy_elements walks the same order by its own formula
    for log in (1, 2, 5):
        n = 1 << log
        pos = logup_model.coset_position(log)
        for i in range(n):
            idx = i // 2 if i % 2 == 0 else n - (i + 1) // 2
            s = int(format(idx, "0%db" % log)[::-1], 2)
            assert pos[s] == i


def test_host_code_under_address_and_ub_sanitizers(pkg, tmp_path):
    """tests/native/logup_host_sanitize.cpp (its own main) compiled together with csrc/logup_program_host.hip as plain C++ under
    g++ -fsanitize=address,undefined and run directly: the 13 programs, every refused program above and 10 000 seeded random word arrays go
    through bfhip_logup_create, and whatever is accepted through bfhip_logup_shape."""
    exe = str(tmp_path / "logup_host_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "native", "logup_host_sanitize.cpp"),
                           "-x", "c++", os.path.join(ROOT, "stwo-brainfuck_amd", "csrc", "logup_program_host.hip")])
    lines = []
    for k in range(13):
        prog = pkg.brainfuck_logup_program(k)[0]
        lines.append("1 %d %d %s" % (prog.shape["n_cols"], prog.shape["n_params"], " ".join(str(w) for w in prog.code)))
    for _, code, n_cols, n_params, _, _ in REJECTED:
        lines.append("0 %d %d %s" % (n_cols, n_params, " ".join(str(w) for w in code)))
    path = tmp_path / "programs.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    out = r.stdout.strip().splitlines()
    assert out[0] == "listed: 13 accepted, %d refused, 0 unexpected" % len(REJECTED), out
    m = re.fullmatch(r"random: (\d+) accepted, (\d+) refused of 10000", out[1])
    assert m and int(m.group(1)) + int(m.group(2)) == 10000 and int(m.group(2)) > 5000 and int(m.group(1)) > 0, out
    assert re.fullmatch(r"edges refused (\d+) of \1", out[2]), out
