"""-m gpu: k_relation_program (csrc/relation_program.hip) at its caps and edges — 32 entries per row over 16 relations, register 95 (24 KiB of
LDS), 4096 instructions, 2 rows and 1 row, a register named by several WORDs, arithmetic at the field's edge, several tables in one call — and
bfhip_relation_program_summary's use of the staging ring at the caps. Programs are written as bytecode where the builder would choose the
registers. Every case is compared with tests/relation_program_model.py, which copies a value at WORD (the kernel keeps the register index
and reads it at the ENTRY); every comparison is exact. The mutants these tests were run against are in tests/test_gpu_relation_scale.py
(MUTATIONS)."""
import numpy as np
import pytest

import field_inputs
import relation_program_model as model
from conftest import P
from test_gpu_relation_program import Dev, assert_same, drawn, run_both

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

COL, CONST, ADD, SUB, MUL, NEG, WORD, ENTRY = model.M_COL, model.M_CONST, model.M_ADD, model.M_SUB, model.M_MUL, model.M_NEG, model.WORD, model.ENTRY
SMALL = np.array([0, 1, P - 1, 5], dtype=np.uint32)
MULTS = np.array([0, 1, P - 1, 2, P - 2, 1, P - 1], dtype=np.uint32)


def program(pkg, instructions, n_cols, widths):
    return pkg.RelationProgram([w for ins in instructions for w in (list(ins) + [0, 0, 0])[:4]], n_cols, widths)


def entry(relation, mult_reg, word_regs):
    return [(WORD, 0, r) for r in word_regs] + [(ENTRY, relation, mult_reg)]


# ---- caps ------------------------------------------------------------------------------------------------------------------------------------------
CAP_WIDTHS = [1 + r % 7 for r in range(16)]


def caps_program(pkg, high_register=False, pad_to=None):
    """32 ENTRYs over 16 relations of widths 1..7, 1..7, 1, 2: entry e adds to relation 5 e mod 16, so the two entries of a relation are 16
    entries apart and every tuple is followed by another relation's. Columns 0..6 are words, column 7 the multiplicity; entry e takes the
    words rotated by e and the multiplicity (e < 16) or its negation. high_register: the multiplicity lives in register 95 (n_m = 96).
    pad_to: M_CONSTs into register 20 in front, in the middle and at the end, up to that many instructions."""
    mreg, nreg = (95, 94) if high_register else (7, 8)
    head = [(COL, k, k) for k in range(7)] + [(COL, mreg, 7), (NEG, nreg, mreg)]
    halves = [[ins for e in range(16 * h, 16 * h + 16) for ins in entry(5 * e % 16, nreg if h else mreg, [(e + k) % 7 for k in range(CAP_WIDTHS[5 * e % 16])])] for h in (0, 1)]
    n_pad = 0 if pad_to is None else pad_to - len(head) - len(halves[0]) - len(halves[1])
    pad = [(CONST, 20, (P - 1 - k) % P) for k in range(n_pad)]
    code = pad[: n_pad // 3] + head + halves[0] + pad[n_pad // 3: 2 * (n_pad // 3)] + halves[1] + pad[2 * (n_pad // 3):]
    prog = program(pkg, code, 8, CAP_WIDTHS)
    assert prog.shape["n_entries"] == 32 and prog.shape["m_regs"] == (96 if high_register else 21 if pad_to else 9) and (pad_to is None or prog.shape["n_instr"] == pad_to)
    return prog


@pytest.fixture(scope="module")
def caps_programs(pkg):
    return {"entries32": caps_program(pkg), "register95": caps_program(pkg, high_register=True), "instr4096": caps_program(pkg, high_register=True, pad_to=4096)}


@pytest.mark.parametrize("log_size,row_shift", [(6, 0), (7, 0), (1, 0), (1, 1), (7, 7), (9, 2)], ids=["64rows", "128rows", "2rows", "1row_of_2", "1row_of_128", "128rows_shift2"])
@pytest.mark.parametrize("which", ["entries32", "register95", "instr4096"])
def test_caps(ctx, caps_programs, which, log_size, row_shift):
    """Every relation gets two entries per row; words from {0, 1, p - 1, 5} so that rotations of a row meet other rows' tuples, multiplicities
    from {0, 1, p - 1, 2, p - 2}. One lane, two lanes, one wave, two waves."""
    rows = 1 << (log_size - row_shift)
    cols = [drawn(300 + k + 16 * log_size, rows, SMALL[: 2 + k % 3]) for k in range(7)] + [drawn(9 + log_size, rows, MULTS)]
    res, want = run_both(ctx, [(caps_programs[which], log_size, row_shift, cols, None)], CAP_WIDTHS)
    per_row = 2 * int(np.count_nonzero(cols[7]))
    assert [r["n_entries"] for r in res.reports] == [per_row] * 16 and [r["n_words"] for r in res.reports] == CAP_WIDTHS
    if rows >= 64:
        assert sum(r["n_unbalanced"] for r in res.reports) > 16


# ---- one register under several WORDs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_size", [1, 6, 7])
def test_repeated_and_rewritten_registers(ctx, pkg, log_size):
    """Relation 0 (2 words) names register 0 twice, relation 1 (7 words) names it seven times after it was rewritten (the ENTRY before has
    consumed the old value), relation 0 then takes it rewritten again beside register 1, and relation 2 (3 words) names 2, 0, 2."""
    code = [(COL, 0, 0), (COL, 1, 1), (COL, 2, 2)] + entry(0, 2, [0, 0]) + [(ADD, 0, 0, 1)] + entry(1, 2, [0] * 7) + [(MUL, 0, 0, 0), (NEG, 3, 2)] + entry(0, 3, [0, 1]) \
        + [(SUB, 2, 1, 0)] + entry(2, 3, [2, 0, 2])
    prog = program(pkg, code, 3, [2, 7, 3])
    n = 1 << log_size
    cols = [drawn(61, n, SMALL), drawn(62, n, SMALL), drawn(63, n, MULTS)]
    res, want = run_both(ctx, [(prog, log_size, 0, cols, None)], [2, 7, 3])
    assert [r["n_entries"] for r in res.reports] == [2 * int(np.count_nonzero(cols[2])), int(np.count_nonzero(cols[2])), int(np.count_nonzero(cols[2]))]
    seven = [e["tuple"] for e in res.entries if e["relation"] == 1]
    assert all(len(set(t)) == 1 for t in seven) and (log_size == 1 or len(seven) > 1)


# ---- arithmetic at the field's edge ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_size", [6, 7])
@pytest.mark.parametrize("family", ["edge", "max", "zero"])
def test_arithmetic_at_the_field_edge(ctx, pkg, family, log_size):
    """Column 0 is p - 1 everywhere, column 2 zero, column 1 the family. (p - 1)(p - 1) = 1, (p - 1) + 1 = 0, 0 - 1 = p - 1, -0 = 0,
    -(p - 1) = 1, the constant p - 1, 1 (p - 1) = p - 1 as words and as multiplicities: the entry whose multiplicity is (p - 1) + 1 does
    not exist, the one with 1 (p - 1) is a use, the one with -(p - 1) a yield."""
    code = [(COL, 0, 0), (COL, 1, 1), (COL, 2, 2), (CONST, 3, 1), (CONST, 4, P - 1),
            (MUL, 5, 0, 0), (ADD, 6, 0, 3), (SUB, 7, 2, 3), (NEG, 8, 2), (NEG, 9, 0), (MUL, 10, 3, 4),
            (MUL, 11, 1, 1), (ADD, 12, 1, 0), (SUB, 13, 1, 0), (NEG, 14, 1), (SUB, 15, 0, 1)]
    code += entry(0, 10, [5, 6, 7, 8, 9, 4, 11])          # a use of (1, 0, p - 1, 0, 1, p - 1, c1^2)
    code += entry(1, 6, [12, 13, 14])                     # multiplicity (p - 1) + 1 = 0: no entry
    code += entry(1, 9, [12, 13, 15])                     # a yield of (c1 - 1, c1 + 1, -1 - c1)
    code += entry(2, 7, [14]) + entry(2, 5, [14])         # -c1 used and yielded: balanced
    code += entry(0, 1, [5, 6, 7, 8, 9, 4, 11])           # the first tuple again with multiplicity c1
    prog = program(pkg, code, 3, [7, 3, 1])
    n = 1 << log_size
    c1 = np.zeros(n, dtype=np.uint32) if family == "zero" else field_inputs.column(family, 5, n)
    cols = [field_inputs.column("max", 0, n), c1, np.zeros(n, dtype=np.uint32)]
    res, want = run_both(ctx, [(prog, log_size, 0, cols, None)], [7, 3, 1])
    assert [r["n_entries"] for r in res.reports] == [n + int(np.count_nonzero(c1)), n, 2 * n] and res.reports[2]["n_unbalanced"] == 0
    assert all(e["tuple"][:6] == (1, 0, P - 1, 0, 1, P - 1) for e in res.entries if e["relation"] == 0)
    if family == "max":      # c1 = p - 1: relation 0 is (.., 1) used 2 n times, relation 1 is (p - 2, 0, 0) yielded n times
        assert [(e["tuple"][-1], e["net"], e["n_use"], e["n_yield"]) for e in res.entries] == [(1, P - 2 * n, 2 * n, 0), (0, n, 0, n)] and res.entries[1]["tuple"] == (P - 2, 0, 0)


# ---- several tables in one call --------------------------------------------------------------------------------------------------------------------------
def test_shared_handles_a_table_without_the_relation_and_mixed_shifts(ctx, pkg):
    """Tables 0 and 2 share one program handle (the code is staged once), table 4 has a second handle of the same code, tables 1 and 3 run a
    program that only adds to relation 1: relation 0 is launched over tables 0, 2, 4 and its first_yield / first_use must say 2 and 4, not 1
    and 2. Table 2 is read at row_shift 2 with a full-size column (shift 0: read at r << 2), a column of shift 4 (read at r >> 2) and one of
    shift 2."""
    widths = [2, 1]
    a_code = [(COL, 0, 0), (COL, 1, 1), (COL, 2, 2)] + entry(0, 2, [0, 1])
    a, a2 = program(pkg, a_code, 3, widths), program(pkg, a_code, 3, widths)
    b = program(pkg, [(COL, 0, 0), (COL, 1, 1)] + entry(1, 1, [0]), 2, widths)
    uses, yields = np.full(64, P - 1, dtype=np.uint32), np.ones(16, dtype=np.uint32)
    specs = [(a, 6, 0, [drawn(1, 64, SMALL[:2]), np.full(64, 9, dtype=np.uint32), uses], None),
             (b, 5, 0, [drawn(2, 32, SMALL[:3]), drawn(3, 32, MULTS)], None),
             (a, 8, 2, [drawn(4, 256, SMALL[:3]), np.full(16, 9, dtype=np.uint32), drawn(5, 64, MULTS[2:])], [0, 4, 2]),
             (b, 4, 0, [np.full(16, 5, dtype=np.uint32), yields], None),
             (a2, 4, 0, [drawn(8, 16, SMALL), np.full(16, 9, dtype=np.uint32), yields], None)]
    res, want = run_both(ctx, specs, widths)
    zero = [e for e in res.entries if e["tuple"] == (0, 9)][0]
    assert zero["first_use"] == (0, int(np.flatnonzero(specs[0][3][0] == 0)[0])) and zero["first_yield"][0] in (2, 4)
    five = [e for e in res.entries if e["tuple"] == (5, 9)][0]          # 5 is not among table 0's and table 2's words
    assert five["first_yield"] == (4, int(np.flatnonzero(specs[4][3][0] == 5)[0])) and five["first_use"] is None
    where = lambda r: {at[0] for e in res.entries if e["relation"] == r for at in (e["first_yield"], e["first_use"]) if at}
    assert where(0) == {0, 2, 4} and where(1) == {1, 3}
    assert model.table_rows(8, 2, specs[2][3], [0, 4, 2])[0].tolist() == specs[2][3][0][::4].tolist()


# ---- the staging ring at the caps ------------------------------------------------------------------------------------------------------------------------
def ring_program(pkg, h):
    """4096 instructions, one entry: the word is column 0 plus h, so each of the 64 programs adds its own tuples and a code block read from the
    wrong place shows."""
    code = [(COL, 0, 0), (COL, 1, 1), (CONST, 2, h), (ADD, 3, 0, 2)] + [(CONST, 4, k) for k in range(4096 - 6)] + entry(0, 1, [3])
    return program(pkg, code, 2, [1])


def test_the_staging_ring_holds_a_call_at_the_caps(pkg):
    """64 tables with 64 distinct programs of 4096 instructions stage, in one call,
        64 x (65 536 code + 256 for the 2 column descriptors, 32 bytes rounded up to stage()'s 256) + 2 x 8192 (two blocks of 64 RelProgLaunch,
        128 bytes each: four addresses, nine RelEntries addresses, six words) = 4 227 072 bytes,
    more than half of the 8 388 608-byte ring, and stage_checkpoint() recycles the ring only when it is MORE than half full. A call with 63 of the
    tables stages 63 x 65 792 + 2 x 8192 = 4 161 280 bytes <= 4 194 304 (with 64 it would be past the half and the next call would recycle): behind
    a one-table call (4 x 256 bytes) the ring holds 4 162 304 bytes, is not recycled, and the 64-table call ends at 8 389 376 > 8 388 608. (From an
    empty ring it would end at 8 388 352 and fit by 256 bytes.) The library refused that call with "staging buffer exhausted"; it now counts what
    it is going to stage and recycles the ring first. Also: the 64-table call twice in a row, and right after a small proof."""
    own = pkg.Context(0, max_log_domain=22)
    try:
        progs = [ring_program(pkg, h) for h in range(64)]
        small = program(pkg, [(COL, 0, 0), (COL, 1, 1)] + entry(0, 1, [0]), 2, [1])
        cols = [np.array([7, P - 1], dtype=np.uint32), np.array([1, P - 2], dtype=np.uint32)]
        want = {k: model.summary([(p.code, 1, 0, cols, None) for p in progs[:k]], [1]) for k in (63, 64)}
        assert want[64][0]["n_entries"] == 128 and want[64][0]["n_tuples"] > 64
        with Dev(own) as dev:
            ptrs = [dev.up(c) for c in cols]
            call = lambda k: own.relation_program_summary([(p, 1, 0, ptrs) for p in progs[:k]], max_entries=200)
            assert own.relation_program_summary([(small, 1, 0, ptrs)]).reports[0]["n_entries"] == 2
            assert_same(call(63), want[63], 200)
            assert_same(call(64), want[64], 200)
            assert_same(call(64), want[64], 200)
            assert_same(call(64), want[64], 200)
            assert pkg.prove_brainfuck("+++>,<[>+.<-]", b"\x01", ctx=own, log_max_rows=20)
            assert_same(call(64), want[64], 200)
    finally:
        own.close()
