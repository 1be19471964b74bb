"""CPU: constraint programs (include/bfhip.h "Constraint programs") at everything a host without a GPU can check — the validator behind
bfhip_air_create (one refused program per rule, every Brainfuck program accepted), the mask against tests/pcs_replay.py, the out-of-domain
evaluator against the project's own bfhip_brainfuck_composition_at_point on real proofs' sampled values, a numpy model of the bytecode
(tests/air_model.py) against it on random programs, and the new host code under AddressSanitizer + UBSan in a stand-alone program
(tests/native/air_host_sanitize.cpp). All comparisons are between integers."""
import ctypes
import json
import os
import random
import re
import subprocess
import zlib

import numpy as np
import pytest

import air_model
import field_inputs
import pcs_replay
from conftest import ROOT

P = (1 << 31) - 1
ALL_OPS = ("+++>,<[>+.<-]", b"\x01")       # tests/test_gpu_components.py
HELLO = ("++++++++++[>+++++++>++++++++++>+++>+<<<<-]>++.>+.+++++++..+++.>++.<<+++++++++++++++.>.+++.------.--------.>+.>.", b"")
LMR = 17
(M_COL, M_CONST, M_ADD, M_SUB, M_MUL, M_NEG, Q_COL, Q_PARAM, Q_FROM_M, Q_ADD, Q_SUB, Q_MUL, Q_MULM, C_BASE, C_EXT) = range(15)
NEG1 = 0xFFFFFFFF
OK_TAIL = [M_CONST, 0, 1, 0, C_BASE, 0, 0, 0]

# (what, code words, n_cols, n_params, instruction index the message names, a word of the rule): one refused program per rule
REJECTED = [
    ("opcode", [15, 0, 0, 0] + OK_TAIL, 4, 1, 0, "unknown opcode 15"),
    ("m register range", [M_CONST, 96, 1, 0] + OK_TAIL, 4, 1, 0, "m register 96 out of range"),
    ("m source register range", OK_TAIL + [M_ADD, 0, 0, 200], 4, 1, 2, "m register 200 out of range"),
    ("q register range", OK_TAIL + [Q_PARAM, 24, 0, 0], 4, 1, 2, "q register 24 out of range"),
    ("m read before write", OK_TAIL + [M_ADD, 1, 0, 5], 4, 1, 2, "m register 5 is read before it is written"),
    ("q read before write", OK_TAIL + [Q_PARAM, 0, 0, 0, Q_MUL, 1, 0, 3], 4, 1, 3, "q register 3 is read before it is written"),
    ("constraint reads an unwritten register", [C_EXT, 0, 0, 0], 4, 1, 0, "q register 0 is read before it is written"),
    ("col within n_cols", OK_TAIL + [M_COL, 1, 4, 0], 4, 1, 2, "column 4 out of range"),
    ("col + 3 within n_cols", OK_TAIL + [Q_COL, 0, 2, 0], 5, 1, 2, "column 2..5 out of range"),
    ("col + 3 without wrap-around", OK_TAIL + [Q_COL, 0, 0xFFFFFFFE, 0], 5, 1, 2, "out of range"),
    ("parameter index", OK_TAIL + [Q_PARAM, 0, 1, 0], 4, 1, 2, "parameter 1 out of range"),
    ("offset above 16", OK_TAIL + [M_COL, 1, 0, 17], 4, 1, 2, "offset 17 out of range"),
    ("offset below -16", OK_TAIL + [Q_COL, 1, 0, (-17) & NEG1], 4, 1, 2, "offset -17 out of range"),
    ("v < p", [M_CONST, 0, P, 0] + OK_TAIL, 4, 1, 0, "not a canonical M31"),
    ("at least one constraint", [M_CONST, 0, 1, 0, M_NEG, 1, 0, 0], 4, 1, 2, "without a constraint"),
    ("cap: instructions", [M_CONST, 0, 1, 0] * 4096 + [C_BASE, 0, 0, 0], 4, 1, 4096, "BFHIP_AIR_MAX_INSTRUCTIONS"),
    ("cap: constraints", [M_CONST, 0, 1, 0] + [C_BASE, 0, 0, 0] * 65, 4, 1, 65, "BFHIP_AIR_MAX_CONSTRAINTS"),
    ("cap: columns", OK_TAIL, 257, 1, 0, "BFHIP_AIR_MAX_COLUMNS"),
    ("cap: parameters", OK_TAIL, 4, 65, 0, "BFHIP_AIR_MAX_PARAMS"),
    ("length", OK_TAIL + [M_NEG, 1, 0], 4, 1, 2, "multiple of 4"),
]


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_validator_refuses_one_program_per_rule(pkg, case):
    _, code, n_cols, n_params, at, rule = case
    with pytest.raises(pkg.BfhipError) as e:
        pkg.AirProgram(code, n_cols, n_params)
    msg = str(e.value)
    print(msg)
    assert re.match(r"bfhip_air_create: instruction %d: " % at, msg) and rule in msg, msg


def test_validator_accepts_what_the_rules_allow(pkg):
    # the caps themselves, the extreme offsets, the last register of each file, an empty column list
    prog = pkg.AirProgram([M_CONST, 95, P - 1, 0] * 4031 + [C_BASE, 0, 95, 0] * 64 + [Q_PARAM, 23, 63, 0], 256, 64)
    assert prog.shape == {"n_cols": 256, "n_params": 64, "n_constraints": 64, "n_instr": 4096, "m_regs": 96, "q_regs": 24, "min_offset": 0, "max_offset": 0}
    prog = pkg.AirProgram([M_COL, 0, 255, 16, Q_COL, 0, 252, (-16) & NEG1, C_BASE, 7, 0, 9, C_EXT, 0, 0, 0], 256, 0)
    assert (prog.shape["min_offset"], prog.shape["max_offset"], prog.shape["n_constraints"]) == (-16, 16, 2)
    assert prog.mask() == [(252, -16), (253, -16), (254, -16), (255, 16), (255, -16)]
    assert pkg.AirProgram(OK_TAIL, 0, 0).mask() == []
    # the size query and a capacity that is too small
    n = ctypes.c_uint32()
    cols, offs = (ctypes.c_uint32 * 4)(), (ctypes.c_int32 * 4)()
    assert pkg.lib().bfhip_air_mask(prog._h, cols, offs, 4, ctypes.byref(n)) == -2 and n.value == 5
    assert b"capacity" in pkg.lib().bfhip_last_error()


def test_brainfuck_programs_are_accepted_and_shaped_like_the_components(pkg):
    for k in range(13):
        a, b, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        assert pkg.lib().bfhip_component_shape(k, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
        for order in (0, 1):
            prog, params, columns = pkg.brainfuck_air_program(k, order)
            s = prog.shape
            assert s["n_constraints"] == c.value and s["n_cols"] == a.value + 4 * b.value + 1 == len(columns), (k, s)
            assert s["n_params"] == len(params) == 25 and (s["min_offset"], s["max_offset"]) == (-1, 0)
            assert s["m_regs"] <= 64 and s["q_regs"] <= 24 and s["n_instr"] == len(prog.code) // 4


@pytest.mark.parametrize("order", [0, 1], ids=["cur_prev", "prev_cur"])
def test_brainfuck_masks_are_the_replay_masks(pkg, order):
    """bfhip_air_mask of component k against pcs_replay.mask_of: point 0 reads offset 0, point 1 + k offset -1; the only offset is -1, on the
    four coordinates of the last logUp column, in the order the convention gives."""
    log_sizes = [5 + (k % 4) for k in range(13)]
    oods = pkg.Channel((0, 0, 0, 0)).draw_point()
    _, samples = pcs_replay.mask_of(pkg, log_sizes, LMR, oods, order)
    shapes = pcs_replay.component_shapes(pkg)
    m0 = i0 = 0
    for k, (n_main, n_logup) in enumerate(shapes):
        prog, _, columns = pkg.brainfuck_air_program(k, order)
        want = []
        per_col = samples[1][m0: m0 + n_main] + samples[2][i0: i0 + 4 * n_logup] + [samples[0][LMR - log_sizes[k]]]
        for col, pts in enumerate(per_col):
            assert pts, columns[col]
            want += [(col, 0 if p == 0 else -1) for p in pts]
            assert all(p in (0, 1 + k) for p in pts)
        assert prog.mask() == want, k
        minus = [c for c, off in prog.mask() if off == -1]
        assert minus == list(range(n_main + 4 * (n_logup - 1), n_main + 4 * n_logup))
        m0, i0 = m0 + n_main, i0 + 4 * n_logup


def _q_pow_table(r, n):
    out, cur = [], [1, 0, 0, 0]
    for _ in range(n):
        out.append(cur)
        cur = pcs_replay.q_mul(cur, r)
    return out


@pytest.mark.parametrize("order", [0, 1], ids=["cur_prev", "prev_cur"])
@pytest.mark.parametrize("prog", [ALL_OPS, HELLO], ids=["all_ops", "hello"])
def test_point_evaluator_sums_to_the_projects_composition(pkg, _oracle, prog, order):
    """A real proof's sampled values, obtained as pcs_replay.verify_replay obtains them: the 13 programs' bfhip_air_eval_at_point, with
    the powers of random_coeff in stwo's accumulator order (constraint j of N = 103 gets r^(N - 1 - j)), add up to
    bfhip_brainfuck_composition_at_point word for word — and to the sampled composition value."""
    conv = (0, 0, order, 0)
    _oracle.set_conventions(*conv)
    try:
        raw = _oracle.prove(prog[0], prog[1], log_max_rows=LMR)[0]
    finally:
        _oracle.set_conventions(0, 0, 0, 0)
    full = json.loads(raw)
    pf = full["proof"]
    log_sizes = [full["claim"][n]["log_size"] for n in pcs_replay.NAMES]
    claimed = [pcs_replay.flat_q(full["interaction_claim"][n]["claimed_sum"]) for n in pcs_replay.NAMES]
    logs = pcs_replay.tree_log_sizes(pkg, log_sizes, LMR)
    ch, v = pkg.Channel(conv), pkg.PcsVerifier(conv)
    roots = [pcs_replay.root_bytes(h) for h in pf["commitments"]]
    v.commit(ch, roots[0], logs[0])
    for l in log_sizes:
        ch.mix_u64(l)
    v.commit(ch, roots[1], logs[1])
    lookup = [w for _ in range(3) for q in ch.draw_felts(2) for w in q]
    for c in claimed:
        ch.mix_felts([c])
    v.commit(ch, roots[2], logs[2])
    random_coeff = ch.draw_felt()
    v.commit(ch, roots[3], logs[3])
    oods = ch.draw_point()
    _, samples = pcs_replay.mask_of(pkg, log_sizes, LMR, oods, order)
    sv = [[[pcs_replay.flat_q(q) for q in col] for col in tree] for tree in pf["sampled_values"]]
    want = pkg.brainfuck_composition_at_point(log_sizes, claimed, LMR, lookup, oods, sv, random_coeff, conv)
    assert pcs_replay.from_partial_evals([sv[3][k][0] for k in range(4)]) == want

    shapes = pcs_replay.component_shapes(pkg)
    n_total = sum(pkg.brainfuck_air_program(k, order)[0].shape["n_constraints"] for k in range(13))
    assert n_total == 103
    powers = _q_pow_table(random_coeff, n_total)
    total, j0, m0, i0 = [0, 0, 0, 0], 0, 0, 0
    for k, (n_main, n_logup) in enumerate(shapes):
        program, _, _ = pkg.brainfuck_air_program(k, order)
        col_values = sv[1][m0: m0 + n_main] + sv[2][i0: i0 + 4 * n_logup] + [sv[0][LMR - log_sizes[k]]]
        col_points = samples[1][m0: m0 + n_main] + samples[2][i0: i0 + 4 * n_logup] + [samples[0][LMR - log_sizes[k]]]
        mask_values = [col_values[col][col_points[col].index(0 if off == 0 else 1 + k)] for col, off in program.mask()]
        n_cons = program.shape["n_constraints"]
        coeffs = [powers[n_total - 1 - (j0 + j)] for j in range(n_cons)]
        got = program.eval_at_point(log_sizes[k], oods, mask_values, pkg.brainfuck_air_params(lookup, claimed[k]), coeffs)
        total = pcs_replay.q_add(total, got)
        j0, m0, i0 = j0 + n_cons, m0 + n_main, i0 + 4 * n_logup
    assert total == want


def test_point_evaluator_refuses_what_does_not_fit(pkg):
    prog = pkg.AirProgram([M_COL, 0, 0, 0, Q_PARAM, 0, 0, 0, Q_MULM, 0, 0, 0, C_EXT, 0, 0, 0], 1, 1)
    pt = pkg.Channel((0, 0, 0, 0)).draw_point()
    one = [1, 0, 0, 0]
    assert prog.eval_at_point(5, pt, [one], [one], [one]) == pcs_replay.q_mul(one, _q_inv(air_model.coset_vanishing(5, pt)))
    for args, what in (((5, pt, [], [one], [one]), "mask has 1 entries"), ((5, pt, [one], [], [one]), "takes 1 parameters"), ((5, pt, [one], [one], [one, one]), "has 1 constraints"),
                       ((0, pt, [one], [one], [one]), "log_size"), ((31, pt, [one], [one], [one]), "log_size"), ((5, pt, [[P, 0, 0, 0]], [one], [one]), "canonical"),
                       ((5, [P] + pt[1:], [one], [one], [one]), "canonical")):
        with pytest.raises(pkg.BfhipError, match=what):
            prog.eval_at_point(*args)


def _q_inv(x):
    """x^(p^4 - 2) by square and multiply"""
    r, e, b = [1, 0, 0, 0], P ** 4 - 2, list(x)
    while e:
        if e & 1:
            r = pcs_replay.q_mul(r, b)
        b = pcs_replay.q_mul(b, b)
        e >>= 1
    return r


@pytest.mark.parametrize("seed", range(12))
def test_numpy_model_agrees_with_the_point_evaluator_on_random_programs(pkg, seed):
    """tests/air_model.py (no denominator) against bfhip_air_eval_at_point times the vanishing polynomial at the point: random programs that
    use every opcode over small register pools, random canonical mask values, parameters and coefficients."""
    rng = random.Random(9000 + seed)
    code, n_cols, n_params, n_cons = air_model.random_program(seed)
    assert {code[i] for i in range(0, len(code), 4)} == set(range(15))
    prog = pkg.AirProgram(code, n_cols, n_params)
    assert prog.shape["n_constraints"] == n_cons and prog.shape["m_regs"] <= 6 and prog.shape["q_regs"] <= 4
    writes = [code[i + 1] for i in range(0, len(code), 4) if code[i] < C_BASE]
    assert len(writes) > len(set(writes))              # registers are reused
    rq = lambda: [rng.choice([0, 1, P - 1, rng.randrange(P)]) for _ in range(4)]
    mask = prog.mask()
    mask_values, params, coeffs = [rq() for _ in mask], [rq() for _ in range(n_params)], [rq() for _ in range(n_cons)]
    log_size = 4 + seed % 5
    ch = pkg.Channel((0, 0, 0, 0))
    ch.mix_u64(seed)
    point = ch.draw_point()
    got = prog.eval_at_point(log_size, point, mask_values, params, coeffs)
    at = {m: air_model.q(v) for m, v in zip(mask, mask_values)}
    model = air_model.run(code, lambda col, off: at[(col, off)], params, coeffs)
    assert pcs_replay.q_mul(got, air_model.coset_vanishing(log_size, point)) == [int(w) for w in model[:, 0]]


# ---- the model where tests/test_gpu_program_edges.py leans on it ---------------------------------------------------------------------------
SIZES = [(log_size, log_expand) for log_size in range(1, 6) for log_expand in range(1, 4)]


def test_random_program_max_cons_leaves_earlier_seeds_alone_and_reaches_the_cap(pkg):
    """The default (60) generates what it always did — the programs of seeds 0 .. 11 are pinned by the CRC-32 of their words, taken before
    the parameter existed — and max_cons = 64 ends on exactly BFHIP_AIR_MAX_CONSTRAINTS constraints, which the validator accepts."""
    crcs = [3787532931, 2369096354, 1312251463, 2189620099, 3319918802, 4017957922, 3676917133, 2603008569, 2523549129, 882003699, 864611483, 3809035066]
    for seed in range(12):
        code = air_model.random_program(seed)[0]
        assert zlib.crc32(b"".join(w.to_bytes(4, "little") for w in code)) == crcs[seed], seed
        assert air_model.random_program(seed) == air_model.random_program(seed, max_cons=60)
    code, n_cols, n_params, n_cons = air_model.random_program(7, n_cols=256, n_params=64, n_ops=3900, m_pool=96, q_pool=24, max_off=16, max_cons=64)
    assert n_cons == 64 and pkg.AirProgram(code, n_cols, n_params).shape["n_constraints"] == 64
    assert max(air_model.random_program(s, n_ops=2000)[3] for s in range(3)) == 60


@pytest.mark.parametrize("log_size,log_expand", SIZES)
def test_domain_denominators_invert_the_vanishing_polynomial_at_the_domains_points(log_size, log_expand):
    """domain_denominators (Python integers on the x of G^index) times coset_vanishing (the model's QM31 arithmetic) at the same point is 1
    at every row; the group indices are those of a circle domain: the second half holds the conjugates of the first, every index is odd
    times 2^(30 - el), and no point lies on the trace domain."""
    el = log_size + log_expand
    n = 1 << el
    g = air_model.domain_group_indices(log_size, log_expand)
    den = air_model.domain_denominators(log_size, log_expand)
    assert den.shape == (n,) and len(set(g.tolist())) == n
    assert all(v % (1 << (30 - el)) == 0 and (v >> (30 - el)) & 1 for v in g.tolist())
    d = air_model.bit_reverse(range(n), el)
    natural = g[np.argsort(d)]                                      # indices in circle-domain order
    assert np.array_equal(natural[n // 2:], (-natural[: n // 2]) % (1 << 31))
    for row in range(n):
        van = air_model.coset_vanishing(log_size, [air_model.circle_x(int(g[row])), 0, 0, 0, 0, 0, 0, 0])
        assert van[1:] == [0, 0, 0] and van[0] * int(den[row]) % P == 1, (row, van)
    # the kernel's table has one entry per row >> log_size: the model, which assumes nothing of the kind, agrees that this is enough
    assert np.array_equal(den, np.repeat(den[:: 1 << log_size], 1 << log_size)) and len(set(den.tolist())) == 1 << log_expand


def test_circle_generator_has_order_two_to_the_31():
    assert air_model.circle_x(1 << 31) == 1 and air_model.circle_x(1 << 30) == P - 1 and air_model.circle_x(1 << 29) == 0
    x, y = air_model.CIRCLE_GEN
    assert (x * x + y * y) % P == 1


@pytest.mark.parametrize("log_size,log_expand", SIZES)
def test_offset_rows_is_the_offset_one_map_composed(log_size, log_expand):
    """Offsets 1 .. 16 on domains of 4 to 256 rows (on the small ones the offset wraps the half coset several times): a permutation, the
    offset-1 map applied `off` times, and the map of -off its inverse."""
    n = 1 << (log_size + log_expand)
    one, walk = air_model.offset_rows(log_size, log_expand, 1), np.arange(n)
    for off in range(1, 17):
        walk = one[walk]
        fwd, back = air_model.offset_rows(log_size, log_expand, off), air_model.offset_rows(log_size, log_expand, -off)
        assert sorted(fwd.tolist()) == list(range(n)), off
        assert np.array_equal(fwd, walk), off
        assert np.array_equal(back[fwd], np.arange(n)) and np.array_equal(fwd[back], np.arange(n)), off
    assert np.array_equal(air_model.offset_rows(log_size, log_expand, 1 << log_size), np.arange(n))      # a full turn of the trace coset


@pytest.mark.parametrize("cols,consts", field_inputs.CROSS, ids=["%s-%s" % c for c in field_inputs.CROSS])
def test_model_q_mul_is_exact_at_saturated_values(cols, consts):
    n = 96
    x = np.stack(field_inputs.columns(cols, 3, 4, n)).astype(np.uint64)
    y = field_inputs.const(consts, 5, 4 * n).reshape(n, 4).T.astype(np.uint64)
    got = air_model.q_mul(x, y)
    for j in range(n):
        assert [int(v) for v in got[:, j]] == field_inputs.qm31_mul_int(x[:, j], y[:, j]), (j, x[:, j], y[:, j])


def _quads_of(family, seed, n):
    if family == "zero":
        return [[0, 0, 0, 0] for _ in range(n)]
    return field_inputs.const(family, seed, 4 * n).reshape(n, 4).tolist() if n else []


SATURATED = ("max", "edge", "heavy", "zero")


@pytest.mark.parametrize("seed", range(6))
def test_numpy_model_agrees_with_the_point_evaluator_at_saturated_values(pkg, seed):
    """Random programs with offsets up to +-16 on mask values, parameters and coefficients from the families max, edge, heavy and all-zero,
    every crossing of the three: model.run(n = 1) == bfhip_air_eval_at_point times the vanishing polynomial. The host evaluator is C++ and
    shares no code with the model or with the kernel."""
    code, n_cols, n_params, n_cons = air_model.random_program(100 + seed, max_off=16)
    prog = pkg.AirProgram(code, n_cols, n_params)
    mask = prog.mask()
    assert max(abs(off) for _, off in mask) > 2
    log_size = 1 + seed % 5
    ch = pkg.Channel((0, 0, 0, 0))
    ch.mix_u64(700 + seed)
    point = ch.draw_point()
    van = air_model.coset_vanishing(log_size, point)
    non_zero = 0
    for fm in SATURATED:
        for fp in SATURATED:
            for fc in SATURATED:
                mask_values, params, coeffs = _quads_of(fm, seed, len(mask)), _quads_of(fp, seed + 1, n_params), _quads_of(fc, seed + 2, n_cons)
                got = prog.eval_at_point(log_size, point, mask_values, params, coeffs)
                at = {m: air_model.q(v) for m, v in zip(mask, mask_values)}
                model = [int(w) for w in air_model.run(code, lambda col, off: at[(col, off)], params, coeffs)[:, 0]]
                assert pcs_replay.q_mul(got, van) == model, (fm, fp, fc)
                non_zero += any(model)
    print("seed", seed, "non-zero results:", non_zero, "of 64 (16 have all-zero coefficients)")
    assert non_zero      # not only comparisons of zeros


def test_builder_reuses_registers_and_keeps_the_order_of_first_use(pkg):
    b = pkg.AirBuilder()
    x = b.col(0)
    for _ in range(200):          # a chain: each value dies at its one use
        x = x * x + b.col(1) - 3
    dead = b.col(2, 5) * 7        # no constraint depends on it: the product is dropped, the column read stays in the mask
    b.constraint(x)
    b.constraint(b.secure_col(3, -2) * b.param(1) - x + b.secure_col(3) * b.col(1, 1))
    prog = b.program()
    assert prog.shape["m_regs"] <= 4 and prog.shape["q_regs"] <= 3 and prog.shape["n_cols"] == 7 and prog.shape["n_params"] == 2
    assert prog.mask() == [(0, 0), (1, 0), (1, 1), (2, 5)] + [(c, o) for c in (3, 4, 5, 6) for o in (-2, 0)]
    assert dead.kind == "m" and M_MUL not in [prog.code[i] for i in range(4 * 602, len(prog.code), 4)]
    # without reuse the 13 components would not fit the caps; with it they stay far below
    big = pkg.AirBuilder()
    acc = big.col(0)
    for i in range(300):
        acc = acc + big.col(i % 8) * big.const(i)
    big.constraint(acc)
    assert big.program().shape["m_regs"] <= 12          # 8 columns stay live, everything else dies at its use
    with pytest.raises(ValueError, match="more than 96 m registers"):
        wide = pkg.AirBuilder()
        vals = [wide.col(0) + i for i in range(120)]
        s = vals[0]
        for v in vals[1:]:
            s = s * v
        wide.constraint(s)
        wide.program()


def test_host_code_under_address_and_ub_sanitizers(pkg, tmp_path):
    """tests/native/air_host_sanitize.cpp (its own main) compiled together with csrc/air_program_host.hip as plain C++ under
    g++ -fsanitize=address,undefined and run directly: the 13 programs (both mask orders), every refused program above and 10 000 seeded
    random word arrays go through bfhip_air_create, and whatever is accepted through shape, mask and the point evaluator."""
    exe = str(tmp_path / "air_host_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "native", "air_host_sanitize.cpp"),
                           "-x", "c++", os.path.join(ROOT, "stwo-brainfuck_amd", "csrc", "air_program_host.hip")])
    lines = []
    for k in range(13):
        for order in (0, 1):
            prog = pkg.brainfuck_air_program(k, order)[0]
            lines.append("1 %d %d %s" % (prog.shape["n_cols"], prog.shape["n_params"], " ".join(str(w) for w in prog.code)))
    for _, code, n_cols, n_params, _, _ in REJECTED:
        lines.append("0 %d %d %s" % (n_cols, n_params, " ".join(str(w) for w in code)))
    path = tmp_path / "programs.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    out = r.stdout.strip().splitlines()
    assert out[0] == "listed: 26 accepted, %d refused, 0 unexpected" % len(REJECTED), out
    m = re.fullmatch(r"random: (\d+) accepted, (\d+) refused of 10000", out[1])
    assert m and int(m.group(1)) + int(m.group(2)) == 10000 and int(m.group(2)) > 5000 and int(m.group(1)) > 0, out
    assert re.fullmatch(r"edges refused (\d+) of \1", out[2]), out
