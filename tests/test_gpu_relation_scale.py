"""-m gpu: relation_aggregate (csrc/relations.hip) above 2^19 entries, where its three second-level loops are entered for the first time — the
chunk loop of k_rel_stats_totals (the four-channel carry), the chunk loop of k_scan_u32_totals (rows, heads, unbalanced flags) and the
segment differences of rel_segment_stats across a chunk seam —, through both front ends, against the numpy reference of
tests/relation_model_np.py; and the same seams at small sizes against the Counter model. Every comparison is exact.

One plan of 1 076 875 entries (odd; 526 scan tiles: three chunks) in 526 153 tuples (two chunks of the unbalanced-flag scan) serves both
front ends. In sorted order, by word 0:
    0          the first tuple, a single yield                                       (unbalanced, rank 0)
    1          bulk A: 260 091 tuples yielded once and used once
    2          five unbalanced tuples of 1 to 3 entries                              (ranks below 2^19)
    3          long segment L1, 8193 entries: contains sorted position 2^19
    2^16       bulk B: 258 047 balanced tuples
    2^30       long segment L2, 8193 entries: contains sorted position 2^20; its first 3000 entries in (table, row) order are uses and
               others, the first yield comes after them (on the compiled path in a later table)
    2^30 + 1   bulk C: 8000 balanced tuples
    p - 3      five unbalanced tuples                                                (ranks above 2^19)
    p - 2      long segment L3, 8193 entries: contains an ordinary tile seam
    p - 1      the last tuple (p - 1, .., p - 1), a single entry of multiplicity p - 2 (guards start[n_tuples] = n)
The long segments draw their multiplicities from {1, p - 1, 2, p - 2}: the running M31 sum wraps thousands of times and all four channels
are non-zero on both sides of the seam. A wrong carry cancels inside a chunk and shows only in a segment that straddles the seam, so the
tests assert with the reference's [start, end) that each straddle happens before anything is uploaded.

MUTATIONS: each mutant of the library changes a computed value only (no index, count, size or address), was built on its own, run against
this module, tests/test_gpu_relation_program_edges.py and the three older relation modules (test_gpu_relations, test_gpu_relation_program,
test_gpu_preflight), and is not committed.
Each failure below is a failed comparison with the reference (wrong net, counts or unbalanced count), none a fault.
    mutant                                                   fails in the new modules                                 the three older modules
    1 k_rel_stats_totals: totals[i] = excl (carry dropped)   test_program_path_above_2p19, test_program_path_all_     all 56 pass: no case has more
                                                             balanced, test_compiled_path_above_2p19                  than 256 tiles
    2 k_rel_stats_totals: carry = total (not accumulated)    the same three (it needs the third chunk)                all 56 pass
    3 k_relation_program: M_SUB with its operands swapped    edges: test_arithmetic_at_the_field_edge (6 cases),      4 fail (the Brainfuck programs,
                                                             test_repeated_and_rewritten_registers (3)                the three-table case)
    4 k_relation_program: M_NEG returns its operand          edges: test_arithmetic_at_the_field_edge (6), test_caps  1 fails (the lookup example of
                                                             (18), test_repeated_and_rewritten_registers (3)          INTEGRATION.md)
"""
import numpy as np
import pytest

import relation_model_np
import test_gpu_relation_program as program_tests
import test_gpu_relations as compiled_tests
from conftest import P, splitmix_column

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

TILE, CHUNK = 2048, 1 << 19              # the scan tile; 256 tiles, one pass of the second-level loops
LONG = 4 * TILE + 1
N_A, N_B, N_C = 260091, 258047, 8000
GROUPS = [0, 1, 2, 3, 1 << 16, 1 << 30, (1 << 30) + 1, P - 3, P - 2, P - 1]
FILL = np.array([0, 1, 1 << 16, 1 << 30, P - 2, P - 1], dtype=np.uint32)
MULTS = np.array([1, P - 1, 2, P - 2], dtype=np.uint64)
SINGLES = [(P - 1,), (2,), (1, 1), (1, P - 2), (P - 2, P - 2, 1)]          # nets p - 1, 2, 2, p - 1, p - 3
LATE = 3000                               # L2: entries in front of the first yield
MEMORY, PROCESSOR = 0, 1                  # the class of an entry: which table holds it (compiled path)


def long_mults(seed, balanced):
    if not balanced:
        return MULTS[splitmix_column(seed, LONG) % np.uint32(4)]
    half = MULTS[splitmix_column(seed, LONG // 2 - 1) % np.uint32(4)]
    m = np.concatenate([half, np.uint64(P) - half, np.array([2, 2, P - 4], dtype=np.uint64)])
    return m[np.argsort(splitmix_column(seed + 1, LONG), kind="stable")]


def plan(n_words, balanced=False):
    """(words (n_words, n_tuples) with the tuples numbered in group order, and per entry: tuple, multiplicity, class, the L2 flag)."""
    tid, mult, cls = [], [], []
    group_of = []

    def add(ids, m, c):
        ids = np.asarray(ids, dtype=np.int64)
        tid.append(ids); mult.append(np.asarray(m, dtype=np.uint64)); cls.append(np.broadcast_to(np.asarray(c, dtype=np.int64), ids.shape))

    next_id = [0]

    def new(group, count):
        ids = np.arange(next_id[0], next_id[0] + count)
        next_id[0] += count
        group_of.append(np.full(count, GROUPS[group], dtype=np.uint32))
        return ids

    def bulk(group, count):
        ids = new(group, count)
        home = np.where(ids % 3 == 0, MEMORY, PROCESSOR)
        add(ids, np.ones(count), np.where(ids % 521 == 1, PROCESSOR, home))          # a few tuples are yielded and used in different tables
        add(ids, np.full(count, P - 1), np.where(ids % 521 == 1, MEMORY, home))

    def singles(group):
        for k, pattern in enumerate(SINGLES):
            m = list(pattern) + ([P - sum(pattern) % P] if balanced else [])
            add(np.repeat(new(group, 1), len(m)), m, [(k + j) % 2 for j in range(len(m))])

    def long(group, seed, c):
        add(np.repeat(new(group, 1), LONG), long_mults(seed, balanced), c)

    add(np.repeat(new(0, 1), 2 if balanced else 1), [1, P - 1] if balanced else [1], PROCESSOR)
    bulk(1, N_A)
    singles(2)
    long(3, 300, np.arange(LONG) % 3 == 0)                  # True = PROCESSOR
    bulk(4, N_B)
    l2 = next_id[0]
    long(5, 500, np.arange(LONG) >= LATE)
    bulk(6, N_C)
    singles(7)
    long(8, 800, np.arange(LONG) % 3 != 0)
    add(np.repeat(new(9, 1), 2 if balanced else 1), [P - 2, 2] if balanced else [P - 2], MEMORY)
    tid, mult, cls = np.concatenate(tid), np.concatenate(mult), np.concatenate(cls)
    n_tuples = next_id[0]
    words = np.zeros((n_words, n_tuples), dtype=np.uint32)
    words[0] = np.concatenate(group_of)
    for k in range(1, n_words - 1):
        words[k] = FILL[splitmix_column((7 + k) << 32, n_tuples) % np.uint32(len(FILL))]
    words[-1] = np.arange(n_tuples)
    words[1:, 0], words[:, -1] = 0, P - 1
    return words, tid, mult, cls, tid == l2


def late_first_yield(mult, is_l2, origin):
    """L2's multiplicities dealt again: the LATE entries lowest in (table, row) order get uses and others only, the rest keep the order drawn."""
    idx = np.flatnonzero(is_l2)
    m = mult[idx]
    front = np.flatnonzero(m != 1)[:LATE]
    assert len(front) == LATE
    rest = np.setdiff1d(np.arange(len(m)), front)
    mult = mult.copy()
    mult[idx[np.argsort(origin[idx], kind="stable")]] = np.concatenate([m[front], m[rest]])
    return mult


def check_plan(ref, balanced=False):
    """The conditions on the input, from the reference's segments: n odd and three chunks, more than 2^19 tuples, three long segments that
    straddle 2^19, 2^20 and an ordinary tile seam with all four channels non-zero on both sides, unbalanced ranks on both sides of 2^19 and at
    both ends."""
    n, start, end, mult = ref["n_entries"], ref["start"], ref["end"], ref["mult"]
    assert n % 2 == 1 and n > 2 * CHUNK + TILE and ref["n_tuples"] > CHUNK
    longs = np.flatnonzero(end - start >= 3 * TILE)
    assert len(longs) == 3
    seams = [CHUNK, 2 * CHUNK, (int(start[longs[2]]) // TILE + 2) * TILE]
    assert seams[2] % CHUNK != 0
    for s, seam in zip(longs, seams):
        assert start[s] < seam - TILE and seam + TILE < end[s]
        for side in (mult[start[s]: seam], mult[seam: end[s]]):
            kinds = [np.count_nonzero(side == 1), np.count_nonzero(side == P - 1), np.count_nonzero((side != 1) & (side != P - 1))]
            assert min(kinds) > 100 and int(side.sum()) > 1000 * P and int(side.sum()) % P != 0
    unb = ref["unbalanced"]
    if balanced:
        assert len(unb) == 0
        return
    assert unb[0] == 0 and unb[-1] == ref["n_tuples"] - 1 and set(longs) <= set(unb) and len(unb) <= 4096
    assert np.count_nonzero(unb < CHUNK) >= 6 and np.count_nonzero(unb >= CHUNK) >= 6
    late = ref["entries"][list(unb).index(longs[1])]
    assert late["n_use"] > 1000 and late["n_other"] > 1000 and late["n_yield"] > 1000


# ---- program path: one table of 2^20 rows, two 7-word entries per row ------------------------------------------------------------------------------
def program_columns(balanced=False):
    """The 16 columns of one_entry_program([7], 0, n_entries=2) at log_size 20: the plan's entries dealt to the 2^21 (row, entry) slots by a
    fixed pseudo-random permutation, every other slot with multiplicity zero."""
    words, tid, mult, _, is_l2 = plan(7, balanced)
    slot = np.argsort(splitmix_column(99, 1 << 21), kind="stable")[: len(tid)]
    if not balanced:
        mult = late_first_yield(mult, is_l2, slot)
    flat = np.zeros((8, 1 << 21), dtype=np.uint32)
    flat[:7, slot] = words[:, tid]
    flat[7, slot] = mult
    return [np.ascontiguousarray(flat[k, e::2]) for e in range(2) for k in range(8)]


def program_reference(prog, cols):
    ref = relation_model_np.summary([(prog.code, 20, 0, cols, None)], [7])
    # the slots a row leaves empty are not entries
    assert ref[0]["n_entries"] == int(np.count_nonzero(cols[7]) + np.count_nonzero(cols[15]))
    return ref


def test_program_path_above_2p19(ctx, pkg):
    """2^20 rows are 512 row tiles (two chunks of the counting scan); 1 076 875 entries are 526 tiles (three chunks of k_rel_stats_totals and of
    the head scan). All 15 unbalanced tuples are compared; then the same input with the report cut at 5."""
    prog = program_tests.one_entry_program(pkg, [7], 0, n_entries=2)
    cols = program_columns()
    ref = program_reference(prog, cols)
    check_plan(ref[0])
    assert len(ref[0]["entries"]) == 15
    late = [e for e in ref[0]["entries"] if e["tuple"][0] == 1 << 30][0]
    assert late["first_use"][1] < late["first_yield"][1]
    with program_tests.Dev(ctx) as dev:
        tables = [(prog, 20, 0, [dev.up(c) for c in cols])]
        program_tests.assert_same(ctx.relation_program_summary(tables, max_entries=64), ref, 64)
        cut = ctx.relation_program_summary(tables, max_entries=5)
        program_tests.assert_same(cut, ref, 5)
        assert cut.reports[0]["n_unbalanced"] == 15 and cut.reports[0]["n_reported"] == 5


def test_program_path_all_balanced(ctx, pkg):
    """The same plan with every tuple balanced (the long segments too, by multiplicities that sum to a multiple of p): a carry that is wrong
    reports the segments on the chunk seams."""
    prog = program_tests.one_entry_program(pkg, [7], 0, n_entries=2)
    cols = program_columns(balanced=True)
    ref = program_reference(prog, cols)
    check_plan(ref[0], balanced=True)
    res = program_tests.run_tables(ctx, [(prog, 20, 0, cols, None)])
    program_tests.assert_same(res, ref)
    assert res.balanced and res.entries == [] and res.reports[0]["n_reported"] == 0 and res.reports[0]["n_entries"] == ref[0]["n_entries"] > 2 * CHUNK


# ---- compiled path: Memory 2^19 rows, Instruction 2^19 rows, Processor 2^20 rows ---------------------------------------------------------------------
def compiled_tables():
    """The plan with 3-word tuples as the Memory relation: an entry of class MEMORY is a Memory row (multiplicity d - 1), one of class
    PROCESSOR a Processor row (1 - d) with the tuple in columns (0, 4, 5), rows dealt by a fixed permutation per table, every other row a dummy
    (d = 1). Columns (1, 2, 3) of the Processor repeat (0, 4, 5) and the Instruction table repeats the Memory table, so the Instruction relation
    sees the same entries from tables 1 and 2; the Processor relation is the Processor's rows alone."""
    words, tid, mult, cls, is_l2 = plan(3)
    rows = np.zeros(len(tid), dtype=np.int64)
    for c, log_rows, seed in ((MEMORY, 19, 41), (PROCESSOR, 20, 43)):
        mine = np.flatnonzero(cls == c)
        assert len(mine) <= 1 << log_rows
        rows[mine] = np.argsort(splitmix_column(seed, 1 << log_rows), kind="stable")[: len(mine)]
    mult = late_first_yield(mult, is_l2, (cls.astype(np.int64) << 32) | rows)
    mem, proc = np.zeros((8, 1 << 19), dtype=np.uint32), np.zeros((9, 1 << 20), dtype=np.uint32)
    mem[3], proc[7] = 1, 1
    m, p = cls == MEMORY, cls == PROCESSOR
    mem[:3, rows[m]] = words[:, tid[m]]
    mem[3, rows[m]] = (mult[m] + np.uint64(1)) % np.uint64(P)
    w = words[:, tid[p]]
    proc[0, rows[p]] = proc[1, rows[p]] = w[0]
    proc[4, rows[p]] = proc[2, rows[p]] = w[1]
    proc[5, rows[p]] = proc[3, rows[p]] = w[2]
    proc[7, rows[p]] = (np.uint64(P + 1) - mult[p]) % np.uint64(P)
    return [(0, mem), (1, mem.copy()), (3, proc)]


def test_compiled_path_above_2p19(ctx):
    """Relations 0 and 1 have 1.5 * 2^20 source rows (three chunks of the row scan) from two tables each and the plan's 1 076 875 entries;
    relation 2 is the Processor's 700 000 rows alone, in four sort passes. Every unbalanced tuple of every relation is compared."""
    tables = compiled_tables()
    ref = relation_model_np.relations(tables)
    for r in (0, 1):
        check_plan(ref[r])
        late = [e for e in ref[r]["entries"] if e["tuple"][0] == 1 << 30][0]
        assert late["first_use"][0] == r and late["first_yield"] == (2, late["first_yield"][1])          # the first yield in a later table
    assert ref[2]["n_entries"] > CHUNK + TILE and 15 < len(ref[2]["entries"]) <= 4096
    d = compiled_tests.DeviceTables(ctx, tables)
    try:
        res = d.summary(4096)
    finally:
        d.close()
    compiled_tests.assert_same(res, ref, 4096)


# ---- the seams at small sizes ------------------------------------------------------------------------------------------------------------------------
SEAMS = [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097]


def small_case(ctx, pkg, n, words, mult, cap=64):
    """n entries of a 2-word relation in the first n rows of the smallest table that holds them; the other rows have multiplicity zero."""
    log_size = max(1, int(n - 1).bit_length())
    cols = [np.zeros(1 << log_size, dtype=np.uint32) for _ in range(3)]
    cols[0][:n], cols[1][:n], cols[2][:n] = words[0], words[1], mult
    assert log_size <= 13 and np.count_nonzero(cols[2]) == n
    prog = program_tests.one_entry_program(pkg, [2], 0)
    return program_tests.run_both(ctx, [(prog, log_size, 0, cols, None)], [2], cap)


@pytest.mark.parametrize("n", SEAMS)
def test_seams_all_tuples_distinct(ctx, pkg, n):
    """n_tuples == n: the head scan and k_rel_starts write start[n_tuples] = n at the seam; every tuple is unbalanced and the report is cut."""
    i = np.arange(n, dtype=np.uint32)
    order = np.argsort(splitmix_column(n, n), kind="stable").astype(np.uint32)
    res, want = small_case(ctx, pkg, n, [order % np.uint32(7), order], MULTS[i % 4])
    assert res.reports[0]["n_tuples"] == res.reports[0]["n_unbalanced"] == n and res.reports[0]["n_reported"] == min(n, 64)


@pytest.mark.parametrize("n", SEAMS)
def test_seams_one_tuple(ctx, pkg, n):
    """n_tuples == 1: one segment over every tile, net 1 + (n - 1) (p - 2)."""
    mult = np.full(n, P - 2, dtype=np.uint64)
    mult[n // 2] = 1
    res, want = small_case(ctx, pkg, n, [np.full(n, P - 1), np.full(n, 5)], mult)
    assert res.reports[0]["n_tuples"] == 1 and res.entries[0]["net"] == (1 + (n - 1) * (P - 2)) % P and res.entries[0]["first_yield"] == (0, n // 2)


@pytest.mark.parametrize("n,n_unb", [(n, u) for n in SEAMS for u in (63, 64, 65) if n == u or n >= u + 2])
def test_seams_unbalanced_count_at_the_cap(ctx, pkg, n, n_unb):
    """cap - 1, cap and cap + 1 unbalanced tuples for cap = 64, spread among the entries of one balanced tuple that fills the rest."""
    rest = n - n_unb
    words0, words1, mult = np.full(n, 3, dtype=np.uint32), np.full(n, 1 << 30, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
    at = (np.arange(n_unb) * n) // n_unb                     # the rows of the unbalanced tuples
    words0[at], words1[at], mult[at] = np.arange(n_unb) % 5, np.arange(n_unb), MULTS[np.arange(n_unb) % 4]
    fill = np.setdiff1d(np.arange(n), at)
    pairs = np.tile(np.array([1, P - 1], dtype=np.uint64), rest // 2 + 1)
    mult[fill] = pairs[:rest] if rest % 2 == 0 else np.concatenate([np.array([2, P - 1, P - 1], dtype=np.uint64), pairs[: rest - 3]])
    res, want = small_case(ctx, pkg, n, [words0, words1], mult)
    assert res.reports[0]["n_unbalanced"] == n_unb and res.reports[0]["n_reported"] == min(64, n_unb) and res.reports[0]["n_tuples"] == n_unb + (rest > 0)
