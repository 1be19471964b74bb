"""-m gpu: bfhip_relation_program_multiplicities (Context.relation_program_multiplicities) — the multiplicity column of a looked-up table
filled on the device by the TARGET mode of the interpreter in csrc/relation_program.hip and relations.hip's relation_multiplicities. Every
comparison is exact against the Counter model of tests/relation_multiplicities_model.py: every word of the column, every count, every field
of every missing tuple. Every case also checks the post-condition: bfhip_relation_program_summary over the same tables, with the filled column
as the multiplicity column of the table side (written -mult), reports exactly the missing tuples as the relation's unbalanced ones, field for
field, and balanced iff there is none."""
import ctypes
import os

import numpy as np
import pytest

import relation_multiplicities_model as model
from conftest import ROOT, P, splitmix_column
from test_gpu_relation_program import ENTRY_FIELDS, MULTS, WORDS, Dev, c_tables, drawn

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

COUNTS = ("n_rows", "n_row_tuples", "n_entries", "n_tuples", "n_filled", "n_missing")
GARBAGE = np.array([0xFFFFFFFF, P, P + 5, 0, 1, 0x80000000, 12345, P - 1], dtype=np.uint32)


def program(pkg, widths, entries):
    """entries: [(relation, [word column], multiplicity column, negated)] in program order. A table side is written -mult."""
    b = pkg.AirBuilder()
    for rel, word_cols, mult_col, negated in entries:
        mult = b.col(mult_col)
        b.relation_entry(rel, -mult if negated else mult, [b.col(k) for k in word_cols])
    return b.relation_program(widths)


def consumer_program(pkg, width, relation=0, widths=None):
    """columns: the tuple's words, then the multiplicity"""
    return program(pkg, [width] if widths is None else widths, [(relation, list(range(width)), width, False)])


def table_program(pkg, width, relation=0, widths=None):
    """columns: the tuple's words, then mult; the entry is (relation, -mult, words)"""
    return program(pkg, [width] if widths is None else widths, [(relation, list(range(width)), width, True)])


def run_case(ctx, specs, relation, target_table, target_entry, mult_col, cap=64, alias=False):
    """specs: [(program, log_size, row_shift, [host column], shifts or None)]; mult_col = the column of the target table that the target
    ENTRY's multiplicity reads (one word per evaluated row). Runs the call (out = a buffer of its own, or that column itself with alias),
    compares with the model and checks the post-condition. Returns (result, out, model report)."""
    want_out, want_rep, want_missing = model.multiplicities([(p.code, log, rs, cols, shifts) for p, log, rs, cols, shifts in specs], relation, target_table, target_entry)
    n_rows = want_rep["n_rows"]
    with Dev(ctx) as dev:
        ptrs = [[dev.up(c) for c in cols] for _, _, _, cols, _ in specs]
        tables = lambda: [(p, log, rs, ptrs[t]) + (() if shifts is None else (shifts,)) for t, (p, log, rs, _, shifts) in enumerate(specs)]
        assert len(specs[target_table][3][mult_col]) == n_rows
        out = ptrs[target_table][mult_col] if alias else dev.up(np.full(n_rows, 0xDEADBEEF, dtype=np.uint32))
        res = ctx.relation_program_multiplicities(tables(), relation, target_table, target_entry, out, max_missing=cap)
        got_out = ctx.download(out, n_rows)
        # the post-condition: the filled column as the table side's multiplicities
        ptrs[target_table][mult_col] = out
        after = ctx.relation_program_summary(tables(), max_entries=max(1, len(want_missing)))
    print(res.report, res.missing[:4], "model", want_rep, want_missing[:4])
    assert np.array_equal(np.asarray(got_out, dtype=np.uint32), want_out), (np.asarray(got_out)[:16], want_out[:16])
    assert {k: res.report[k] for k in COUNTS} == want_rep
    assert (res.report["relation"], res.report["target_table"], res.report["target_entry"]) == (relation, target_table, target_entry)
    assert res.report["n_words"] == specs[0][0].relation_words[relation] and res.report["n_reported"] == min(cap, len(want_missing)) == len(res.missing)
    assert [{f: e[f] for f in ENTRY_FIELDS} for e in res.missing] == want_missing[:cap] and all(e["relation"] == relation for e in res.missing)
    assert res.ok == (not want_missing)
    unbalanced = [{f: e[f] for f in ENTRY_FIELDS} for e in after.entries if e["relation"] == relation]
    assert unbalanced == want_missing and after.reports[relation]["n_unbalanced"] == len(want_missing)
    assert (after.reports[relation]["n_unbalanced"] == 0) == res.ok
    return res, np.asarray(got_out, dtype=np.uint32), want_rep


def lookup_specs(pkg, table_log, consumer_log, width, seed=0, nonzero=False):
    """A consumer (table 0) looking up a table (table 1): words from WORDS, so tuples repeat among the consumers and among the table's rows;
    multiplicities from MULTS (0 is no entry, p - 1 and p - 2 go "negative", 1 and p - 1 cancel)."""
    n, m = 1 << consumer_log, 1 << table_log
    consumer = [drawn(seed + 10 + k, n, WORDS[: 2 + k % 4]) for k in range(width)] + [drawn(seed + 7, n, MULTS[1:] if nonzero else MULTS)]
    table = [drawn(seed + 50 + k, m, WORDS[: 2 + k % 4]) for k in range(width)] + [GARBAGE[np.arange(m) % len(GARBAGE)]]
    return [(consumer_program(pkg, width), consumer_log, 0, consumer, None), (table_program(pkg, width), table_log, 0, table, None)]


# ---- 1, 2. sizes and widths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table_log,consumer_log,width", [(1, 5, 1), (4, 7, 2), (6, 9, 3), (12, 13, 7), (6, 10, 1), (6, 10, 2), (6, 10, 7), (12, 10, 3)])
def test_sizes_and_widths_against_the_model(ctx, pkg, table_log, consumer_log, width):
    """Target tables of 2 rows, less than a wave, one wave and 64 workgroups; widths 1, 3 and 7 take a 32-bit key pass, 2, 3 and 7 a 64-bit one."""
    res, out, rep = run_case(ctx, lookup_specs(pkg, table_log, consumer_log, width, seed=100 * table_log + width), 0, 1, 0, width)
    assert rep["n_entries"] > 0 and rep["n_row_tuples"] <= rep["n_rows"] == 1 << table_log
    if table_log >= 4:
        assert rep["n_filled"] > 0


@pytest.mark.parametrize("total", [2047, 2048, 2049])
def test_entry_total_at_the_scan_tile(ctx, pkg, total):
    """A 2^11-row consumer beside a 16-row table: the entries the sort and the scans see (the consumer's non-zero ones plus the 16 table rows)
    number 2047, 2048 and 2049 — one tile of 2048 less one, full, and one entry into the second."""
    specs = lookup_specs(pkg, 4, 11, 2, seed=3, nonzero=True)
    zeros = 2048 + 16 - total
    specs[0][3][2][(np.arange(zeros) * 61 + 5) % 2048] = 0
    res, out, rep = run_case(ctx, specs, 0, 1, 0, 2)
    assert rep["n_entries"] + rep["n_rows"] == total


def test_above_2_to_19_entries(ctx, pkg):
    """A 2^19-row consumer whose every row is an entry, plus a 2^10-row table of distinct values, width 1: 2^19 + 2^10 entries, more than 256
    tiles, so the second round of the totals scan runs. About 7% of the consumer's rows hold one of 76 values that are in no table row
    (a missing tuple unless its multiplicities happen to cancel)."""
    n, m = 1 << 19, 1 << 10
    consumer = [(splitmix_column(77, n) % np.uint32(1100)) * np.uint32(3) + np.uint32(1), drawn(78, n, MULTS[1:])]
    table = [np.arange(m, dtype=np.uint32) * np.uint32(3) + np.uint32(1), np.zeros(m, dtype=np.uint32)]
    specs = [(consumer_program(pkg, 1), 19, 0, consumer, None), (table_program(pkg, 1), 10, 0, table, None)]
    res, out, rep = run_case(ctx, specs, 0, 1, 0, 1, cap=8)
    assert rep["n_entries"] == n and rep["n_row_tuples"] == m and 8 < rep["n_missing"] <= 1100 - m and res.report["n_reported"] == 8


# ---- 3. a segment spanning several tiles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [0, 63])
def test_one_table_row_used_by_every_consumer_row(ctx, pkg, row):
    n, m = 1 << 13, 1 << 6
    ids = np.arange(m, dtype=np.uint32)
    table = [ids + np.uint32(1000), ids * np.uint32(7), np.full(m, P, dtype=np.uint32)]
    consumer = [np.full(n, 1000 + row, dtype=np.uint32), np.full(n, 7 * row, dtype=np.uint32), np.ones(n, dtype=np.uint32)]
    specs = [(consumer_program(pkg, 2), 13, 0, consumer, None), (table_program(pkg, 2), 6, 0, table, None)]
    res, out, rep = run_case(ctx, specs, 0, 1, 0, 2)
    assert out[row] == n and np.count_nonzero(out) == 1 and res.ok
    assert rep == {"n_rows": m, "n_row_tuples": m, "n_entries": n, "n_tuples": 1, "n_filled": 1, "n_missing": 0}


# ---- 4. duplicate table rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distinct", [40, 1])
def test_duplicate_table_rows_get_zero(ctx, pkg, distinct):
    """A 64-row table whose rows from `distinct` - 1 on all hold one tuple (padding with the last tuple; with 1: all rows equal): the lowest of
    them gets everything, the copies exactly 0."""
    n, m = 1 << 9, 1 << 6
    ids = np.minimum(np.arange(m, dtype=np.uint32), np.uint32(distinct - 1))
    table = [ids + np.uint32(5), np.full(m, 0xFFFFFFFF, dtype=np.uint32)]
    consumer = [(splitmix_column(9, n) % np.uint32(distinct)) + np.uint32(5), np.ones(n, dtype=np.uint32)]
    specs = [(consumer_program(pkg, 1), 9, 0, consumer, None), (table_program(pkg, 1), 6, 0, table, None)]
    res, out, rep = run_case(ctx, specs, 0, 1, 0, 1)
    assert rep["n_row_tuples"] == distinct and res.ok and not out[distinct:].any() and out[distinct - 1] > 0 and int(out.sum()) == n
    if distinct == 1:
        assert out[0] == n


# ---- 5. three tables, the target in the middle, two ENTRYs of the relation and one of another -----------------------------------------------------
@pytest.mark.parametrize("target_entry", [0, 1])
def test_three_tables_target_in_the_middle(ctx, pkg, target_entry):
    """Relation 0 is two words wide, relation 1 one. Table 1's program: ENTRY of relation 0 over columns (0, 1) with -column 4, ENTRY of
    relation 1 (ignored), ENTRY of relation 0 over columns (2, 3) with -column 5. Whichever of the two is not the target counts as an other
    entry, with the multiplicities its column holds."""
    widths = [2, 1]
    middle = program(pkg, widths, [(0, [0, 1], 4, True), (1, [0], 6, False), (0, [2, 3], 5, True)])
    n0, n1, n2 = 1 << 8, 1 << 5, 1 << 7
    specs = [(consumer_program(pkg, 2, widths=widths), 8, 0, [drawn(1, n0, WORDS[:3]), drawn(2, n0, WORDS[:2]), drawn(3, n0, MULTS)], None),
             (middle, 5, 0, [drawn(4, n1, WORDS[:3]), drawn(5, n1, WORDS[:2]), drawn(6, n1, WORDS[:3]), drawn(7, n1, WORDS[:2]), drawn(8, n1, MULTS), drawn(9, n1, MULTS),
                             drawn(10, n1, MULTS)], None),
             (program(pkg, widths, [(1, [0], 2, False), (0, [1, 0], 2, False)]), 7, 0, [drawn(11, n2, WORDS[:2]), drawn(12, n2, WORDS[:3]), drawn(13, n2, MULTS)], None)]
    res, out, rep = run_case(ctx, specs, 0, 1, target_entry, 4 + target_entry)
    assert rep["n_rows"] == n1 and rep["n_entries"] > np.count_nonzero(specs[0][3][2]) and rep["n_filled"] > 0


# ---- 6. a row-granular target beside full-size consumers -----------------------------------------------------------------------------------------
def test_row_granular_target(ctx, pkg):
    """The target at row_shift 4 (16 evaluated rows of a 2^8 trace): its first word column is full size (shift 0, read at r << 4), its second
    word and its mult column hold one word per row (shift 4). The consumer is full size at row_shift 0."""
    n = 1 << 9
    full = drawn(21, 256, WORDS)
    table = [full, drawn(22, 16, WORDS[:2]), GARBAGE[np.arange(16) % 8]]
    consumer = [drawn(23, n, WORDS), drawn(24, n, WORDS[:2]), drawn(25, n, MULTS)]
    specs = [(consumer_program(pkg, 2), 9, 0, consumer, None), (table_program(pkg, 2), 8, 4, table, [0, 4, 4])]
    res, out, rep = run_case(ctx, specs, 0, 1, 0, 2)
    assert rep["n_rows"] == 16 and rep["n_filled"] > 0
    held = set(zip(full[::16].tolist(), table[1].tolist()))
    assert rep["n_row_tuples"] == len(held)


# ---- 7. out_d is the column the target's multiplicity reads ---------------------------------------------------------------------------------------
def test_out_may_be_the_multiplicity_column_itself(ctx, pkg):
    specs = lookup_specs(pkg, 6, 10, 2, seed=31)
    assert (specs[1][3][2] >= P).any()
    apart = run_case(ctx, specs, 0, 1, 0, 2)
    alias = run_case(ctx, specs, 0, 1, 0, 2, alias=True)
    assert np.array_equal(apart[1], alias[1]) and apart[0].report == alias[0].report and apart[0].missing == alias[0].missing


# ---- 8. missing tuples ----------------------------------------------------------------------------------------------------------------------------
def missing_specs(pkg, extra):
    """A 16-row table of 100 .. 115; 64 consumer rows of table values, then `extra` values 1, 2, ... that no row holds, then 50 used once with
    +1 and once with p - 1 (it cancels: not missing)."""
    table = [np.arange(16, dtype=np.uint32) + np.uint32(100), np.zeros(16, dtype=np.uint32)]
    values = np.concatenate([(splitmix_column(5, 128 - extra - 2) % np.uint32(16)) + np.uint32(100), np.arange(extra, 0, -1, dtype=np.uint32), np.array([50, 50], dtype=np.uint32)])
    mults = np.concatenate([np.ones(126, dtype=np.uint32), np.array([1, P - 1], dtype=np.uint32)])
    return [(consumer_program(pkg, 1), 7, 0, [values, mults], None), (table_program(pkg, 1), 4, 0, table, None)]


@pytest.mark.parametrize("extra,cap", [(0, 64), (1, 64), (9, 4), (9, 0)])
def test_missing_tuples(ctx, pkg, extra, cap):
    res, out, rep = run_case(ctx, missing_specs(pkg, extra), 0, 1, 0, 1, cap=cap)
    assert (res.report["n_missing"], res.report["n_reported"]) == (extra, min(extra, cap)) and res.ok == (extra == 0)
    assert [e["tuple"] for e in res.missing] == [(v,) for v in range(1, min(extra, cap) + 1)]
    assert rep["n_tuples"] == 16 + extra + 1 and int(out.sum()) == 126 - extra
    if cap:
        assert all(e["net"] == 1 and e["first_yield"] == (0, 126 - e["tuple"][0]) and e["first_use"] is None for e in res.missing)
    if extra > cap:
        assert res.lines()[-1] == "relation 0 relation: %d more missing tuples not listed" % (extra - cap)


# ---- 9. determinism and the arena ----------------------------------------------------------------------------------------------------------------
def raw_call(ctx, pkg, tables, n_rel, relation, target_table, target_entry, out, cap):
    rep, miss = pkg.MultiplicityReport(), (pkg.RelationEntry * max(cap, 1))()
    ctypes.memset(ctypes.byref(rep), 0xCD, ctypes.sizeof(rep))
    ctypes.memset(miss, 0xAB, ctypes.sizeof(miss))
    rc = pkg.lib().bfhip_relation_program_multiplicities(ctx._h, tables, len(tables), n_rel, relation, target_table, target_entry, ctypes.c_void_p(out), ctypes.byref(rep),
                                                         miss if cap else None, cap)
    return rc, rep, miss


def test_two_runs_give_identical_bytes_and_the_arena_is_put_back(pkg):
    ctx = pkg.Context(0, max_log_domain=16)
    try:
        specs = lookup_specs(pkg, 3, 12, 3, seed=41)
        keep = []
        with Dev(ctx) as dev:
            tables = c_tables(ctx, pkg, [(p, log, rs, [dev.up(c) for c in cols], shifts) for p, log, rs, cols, shifts in specs], keep)
            out1, out2 = dev.up(np.full(8, 7, dtype=np.uint32)), dev.up(np.full(8, 9, dtype=np.uint32))
            before = ctx.memory()["arena_in_use"]
            rc1, rep1, miss1 = raw_call(ctx, pkg, tables, 1, 0, 1, 0, out1, 200)
            assert ctx.memory()["arena_in_use"] == before
            rc2, rep2, miss2 = raw_call(ctx, pkg, tables, 1, 0, 1, 0, out2, 200)
            words1, words2 = ctx.download(out1, 8), ctx.download(out2, 8)
        assert rc1 == rc2 == 0 and bytes(rep1) == bytes(rep2) and bytes(miss1) == bytes(miss2) and np.array_equal(words1, words2)
        assert 0 < rep1.n_reported == rep1.n_missing < 200 and rep1.n_filled > 0 and ctx.memory()["arena_in_use"] == before
        assert (rep1.reserved[0], rep1.reserved[1]) == (0, 0)
        # slots beyond n_reported are not written
        assert bytes(miss1)[96 * rep1.n_reported:] == b"\xab" * (96 * (200 - rep1.n_reported))
    finally:
        ctx.close()


# ---- 10. the lookup example of INTEGRATION.md section 2e -----------------------------------------------------------------------------------------
def test_integration_lookup_example(_ctx, pkg):
    """The `a` / `t` / `mult` trace of tests/test_gpu_air_check.py with mult computed by the call, as the document prints it: it equals the
    hand-made column, the claimed sum is zero and air_check says ok. With one cell of `a` changed to a value not in `t`, lines() is the one
    line naming that tuple and its row."""
    log_size, ctx = 6, _ctx
    n = 1 << log_size
    f = pkg.AirBuilder()
    a, t, mult, z, alpha = f.col(0), f.col(1), f.col(2), f.param(0), f.param(1)
    f.frac(1, alpha * a - z); f.end_column()
    f.frac(-mult, alpha * t - z); f.end_column()
    fractions = f.logup_program()
    b = pkg.AirBuilder()
    a, t, mult, is_first = b.col(0), b.col(1), b.col(2), b.col(3)
    z, alpha, total = b.param(0), b.param(1), b.param(2)
    cur0, cur1, prev1 = b.secure_col(4), b.secure_col(8), b.secure_col(8, -1)
    b.constraint(cur0 * (alpha * a - z) - b._to_q(b.const(1)))
    b.constraint((cur1 - (prev1 - total * is_first) - cur0) * (alpha * t - z) - b._to_q(-mult))
    prog = b.program()
    r = pkg.AirBuilder()
    a, t, mult = r.col(0), r.col(1), r.col(2)
    r.relation_entry(0, 1, [a])
    r.relation_entry(0, -mult, [t])
    relation = r.relation_program([1])
    table = splitmix_column(51, n)
    assert len(set(table.tolist())) == n
    pick = splitmix_column(52 << 32, n) % np.uint32(n // 4)
    first = np.zeros(n, dtype=np.uint32); first[0] = 1
    by_hand = np.bincount(pick, minlength=n).astype(np.uint32)
    quads = splitmix_column(61, 8).reshape(2, 4).tolist()
    names = dict(relation_names=["lookup"], table_names=["trace"])
    with Dev(ctx) as dev:
        trace_cols = [dev.up(table[pick]), dev.up(table), dev.empty(n), dev.up(first)]
        inter_cols = [dev.empty(n) for _ in range(8)]
        res = ctx.relation_program_multiplicities([(relation, log_size, 0, trace_cols[:3])], 0, 0, 1, trace_cols[2], **names)
        assert res.ok, "\n".join(res.lines())
        assert np.array_equal(ctx.download(trace_cols[2], n), by_hand)
        assert res.report["n_filled"] == np.count_nonzero(by_hand) and res.report["n_entries"] == n and res.lines() == []
        assert ctx.relation_program_summary([(relation, log_size, 0, trace_cols[:3])], **names).balanced
        claimed = ctx.logup_program_generate(fractions, log_size, trace_cols[:3], quads, inter_cols)
        assert claimed == [0, 0, 0, 0]
        assert ctx.air_check(prog, log_size, trace_cols + inter_cols, quads + [claimed]).as_dict()["ok"]
        bad = table[pick].copy()
        bad[5] = 12345
        assert 12345 not in table.tolist()
        res = ctx.relation_program_multiplicities([(relation, log_size, 0, [dev.up(bad)] + trace_cols[1:3])], 0, 0, 1, trace_cols[2], **names)
        filled = ctx.download(trace_cols[2], n)
    want = by_hand.copy()
    want[pick[5]] -= 1
    assert np.array_equal(filled, want) and not res.ok and res.report["n_missing"] == 1
    assert res.lines() == ["lookup relation: (12345) net +1: yielded 1x (first: trace row 5), used 0x; no row of trace holds it"]
    assert res.lines()[0] in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_rule_and_leave_the_context_usable(ctx, pkg):
    L = pkg.lib()
    err = lambda: L.bfhip_last_error().decode()
    me = "bfhip_relation_program_multiplicities: "
    widths = [1, 2]
    prog = program(pkg, widths, [(0, [0], 1, False), (0, [0], 2, True), (1, [0, 0], 1, False)])
    other_n, other_w = consumer_program(pkg, 1), consumer_program(pkg, 1, widths=[1, 3])
    keep = []
    with Dev(ctx) as dev:
        ptrs = [dev.up(np.array([5, 5, 6, 7] * 16, dtype=np.uint32)), dev.up(np.array([1, P - 1, 1, 0] * 16, dtype=np.uint32)), dev.up(GARBAGE[np.arange(64) % 8])]
        out = dev.up(np.full(64, 0xDEADBEEF, dtype=np.uint32))
        good = (prog, 6, 0, ptrs, None)
        tables = c_tables(ctx, pkg, [good], keep)
        rep, miss = pkg.MultiplicityReport(), (pkg.RelationEntry * 2)()
        call = lambda tabs, n_tab, n_rel, rel, tt, te, o=out, r=rep, m=miss, cap=2: L.bfhip_relation_program_multiplicities(
            ctx._h, tabs, n_tab, n_rel, rel, tt, te, None if o is None else ctypes.c_void_p(o), None if r is None else ctypes.byref(r), m, cap)
        in_use = ctx.memory()["arena_in_use"]
        cases = [((tables, 1, 2, 2, 0, 0), "relation 2 out of range (the call names 2 relations)"),
                 ((tables, 1, 2, 0, 1, 0), "target table 1 out of range (the call names 1 tables)"),
                 ((tables, 1, 2, 0, 0, 2), "target entry 2: the program of table 0 has 2 ENTRY instructions of relation 0"),
                 ((tables, 1, 2, 1, 0, 1), "target entry 1: the program of table 0 has 1 ENTRY instructions of relation 1"),
                 ((tables, 1, 3, 0, 0, 0), "table 0: its program was created with 2 relations, the call names 3"),
                 ((c_tables(ctx, pkg, [good, (other_n, 6, 0, ptrs, None)], keep), 2, 2, 0, 0, 0), "table 1: its program was created with 1 relations, the call names 2"),
                 ((c_tables(ctx, pkg, [good, (other_w, 6, 0, ptrs, None)], keep), 2, 2, 0, 0, 0), "table 1: its program gives relation 1 3 words, table 0's 2"),
                 ((c_tables(ctx, pkg, [(prog, 6, 7, ptrs, None)], keep), 1, 2, 0, 0, 0), "table 0: row_shift 7 above log_size 6"),
                 ((tables, 0, 2, 0, 0, 0), "1 to 64 tables, got 0")]
        for args, what in cases:
            assert call(*args) == -1 and err() == me + what, err()
        assert call(tables, 1, 2, 0, 0, 0, o=None) == -1 and err() == me + "null argument"
        assert call(tables, 1, 2, 0, 0, 0, r=None) == -1 and err() == me + "null argument"
        assert call(tables, 1, 2, 0, 0, 0, m=None) == -1 and err() == me + "null argument"
        assert call(None, 1, 2, 0, 0, 0) == -1 and err() == me + "null argument"
        # nothing was written by a refused call, and the arena's bookkeeping is where it was
        assert ctx.memory()["arena_in_use"] == in_use and set(ctx.download(out, 64).tolist()) == {0xDEADBEEF}
        # an open commitment-scheme session
        ctx.set_pcs_config(pkg.PcsConfig())
        with pkg.PcsSession(ctx):
            held = ctx.memory()["arena_in_use"]
            with pytest.raises(pkg.BfhipError, match=r"^bfhip_relation_program_multiplicities: a commitment-scheme session is open on this context \(bfhip_pcs_destroy first\)$"):
                ctx.relation_program_multiplicities([good[:4]], 0, 0, 1, out)
            assert ctx.memory()["arena_in_use"] == held
        # a member of a shard group
        group = pkg.LocalGroup(2)
        member = pkg.Context(0, max_log_domain=12)
        try:
            member.join_local_group(group, 0)
            with pytest.raises(pkg.BfhipError, match="bfhip_relation_program_multiplicities: a context in a shard group"):
                member.relation_program_multiplicities([good[:4]], 0, 0, 1, out)
            member.leave_group()
        finally:
            member.close(); group.close()
        # missing tuples are not an error: status 0, the error text is left as it was, and the result after every refusal is the model's.
        # Target = the second ENTRY of relation 0; the first counts: 5 has +1 and p - 1 sixteen times each (net 0), 6 has +16, 7 has none.
        text = err()
        assert call(tables, 1, 2, 0, 0, 1, cap=0, m=None) == 0 and err() == text
        assert ctx.memory()["arena_in_use"] == in_use
        assert (rep.n_rows, rep.n_row_tuples, rep.n_entries, rep.n_tuples, rep.n_filled, rep.n_missing, rep.n_reported) == (64, 3, 48, 2, 1, 0, 0)
        got = ctx.download(out, 64)
        want = np.zeros(64, dtype=np.uint32); want[2] = 16
        assert np.array_equal(got, want)
    res, _, _ = run_case(ctx, [(prog, 6, 0, [np.array([5, 5, 6, 7] * 16, dtype=np.uint32), np.array([1, P - 1, 1, 0] * 16, dtype=np.uint32), GARBAGE[np.arange(64) % 8]], None)], 0, 0, 1, 2)
    assert res.ok
