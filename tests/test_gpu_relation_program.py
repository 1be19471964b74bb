"""-m gpu: the lookup tuples of ANY AIR that do not cancel — relation programs run by the gfx950 interpreter of csrc/relation_program.hip
(bfhip_relation_program_summary; Context.relation_program_summary) and reduced by relations.hip. Compared with the compiled path
(Trace.relations) on the 13 Brainfuck tables and with the Counter model of tests/relation_program_model.py on synthetic AIRs. Every comparison
is exact: integer counts, M31 sums, table indices and rows."""
import ctypes
import os

import numpy as np
import pytest

import relation_program_model as model
from conftest import ROOT, P, splitmix_column
from test_relations_cpu import UNKNOWN_TUPLE, unknown_opcode_registers

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

HELLO1 = (open(os.path.join(ROOT, "tests", "golden", "programs", "hello1.bf")).read(), b"")
N_MAIN = [8, 8, 4, 9, 13, 13, 11, 11, 11, 11, 11, 11, 7]
ENTRY_FIELDS = ("tuple", "net", "n_yield", "n_use", "n_other", "first_yield", "first_use")
MULTS = np.array([0, 1, P - 1, 2, P - 2], dtype=np.uint32)
WORDS = np.array([0, P - 1, 1, 7, 1 << 30], dtype=np.uint32)


class Dev:
    """device buffers freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, arr):
        self.ptrs.append(self.ctx.upload(np.ascontiguousarray(arr, dtype=np.uint32)))
        return self.ptrs[-1]

    def empty(self, n):
        self.ptrs.append(self.ctx.malloc(4 * n))
        return self.ptrs[-1]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.free(p)


def run_tables(ctx, specs, cap=64, **names):
    """specs: [(program, log_size, row_shift, [host column], shifts or None)]. Uploads, runs the summary, frees."""
    with Dev(ctx) as dev:
        tables = [(prog, log, rs, [dev.up(c) for c in cols]) + (() if shifts is None else (shifts,)) for prog, log, rs, cols, shifts in specs]
        return ctx.relation_program_summary(tables, max_entries=cap, **names)


def assert_same(res, want, cap=64):
    """Every count and every reported entry field against the model; the model's list cut at the cap."""
    assert len(res.reports) == len(want)
    for r, w in enumerate(want):
        rep = res.reports[r]
        got = [e for e in res.entries if e["relation"] == r]
        print(rep, got[:6], "model", w["n_entries"], w["n_tuples"], len(w["entries"]), w["entries"][:6])
        assert (rep["relation"], rep["name"], rep["n_words"]) == (r, "relation %d" % r, w["n_words"])
        assert (rep["n_entries"], rep["n_tuples"], rep["n_unbalanced"]) == (w["n_entries"], w["n_tuples"], len(w["entries"]))
        assert rep["n_reported"] == min(cap, len(w["entries"])) == len(got)
        assert [{f: e[f] for f in ENTRY_FIELDS} for e in got] == w["entries"][:cap]
    assert res.balanced == all(not w["entries"] for w in want)


def run_both(ctx, specs, relation_words, cap=64):
    res = run_tables(ctx, specs, cap)
    want = model.summary([(prog.code, log, rs, cols, shifts) for prog, log, rs, cols, shifts in specs], relation_words)
    assert_same(res, want, cap)
    return res, want


def one_entry_program(pkg, widths, relation, n_entries=1):
    """Columns: per entry the relation's words, then the multiplicity. `n_entries` entries of ONE relation per row."""
    b = pkg.AirBuilder()
    w = widths[relation]
    for e in range(n_entries):
        base = e * (w + 1)
        b.relation_entry(relation, b.col(base + w), [b.col(base + k) for k in range(w)])
    return b.relation_program(widths)


def drawn(seed, n, values):
    return values[splitmix_column(seed, n) % np.uint32(len(values))]


# ---- 1. parity with the compiled path -----------------------------------------------------------------------------------------------------------
def trace_specs(pkg, tr):
    """The 13 row-granular tables of a resident trace as relation-program tables: row_shift 4, one word per row in every column."""
    return [(pkg.brainfuck_relation_program(k)[0], tr.log_sizes[k], 4, [tr.column(k, j) for j in range(N_MAIN[k])], None) for k in range(13)]


@pytest.mark.parametrize("case", ["hello1", "unknown_opcode"])
def test_brainfuck_programs_equal_the_compiled_relations(ctx, pkg, oracle, case):
    if case == "hello1":
        tr = pkg.Trace(ctx, *HELLO1)
    else:
        tr = pkg.Trace.from_registers(ctx, *unknown_opcode_registers(oracle))
    try:
        specs = trace_specs(pkg, tr)
        for cap in (4, 64):
            want = tr.relations(cap)
            got = run_tables(ctx, specs, cap, relation_names=pkg.RELATION_NAMES, table_names=pkg.COMPONENT_NAMES)
            print(case, cap, got.reports, got.entries)
            assert got.reports == want.reports and got.entries == want.entries and got.lines() == want.lines() and got.balanced == want.balanced
            assert all(r["n_entries"] > 0 for r in got.reports)
        if case == "hello1":
            assert got.balanced and got.entries == []
        else:
            assert [r["n_unbalanced"] for r in got.reports] == [0, 0, 1] and got.entries[0]["tuple"] == UNKNOWN_TUPLE
            assert got.lines() == ["processor relation: (1, 1, 35, 43, 0, 1, 1) net +1: yielded 1x (first: processor row 1), used 0x"]
    finally:
        tr.close()


# ---- 2. the same tables as full-size columns -----------------------------------------------------------------------------------------------------
def test_full_size_columns_count_every_cell(ctx, pkg, oracle):
    """The unknown-opcode tables expanded 16-fold on the device (bfhip_broadcast16) and read at row_shift 0: the same tuples, every count and
    first row x 16, net x 16 mod p."""
    tr = pkg.Trace.from_registers(ctx, *unknown_opcode_registers(oracle))
    try:
        specs = trace_specs(pkg, tr)
        rows = run_tables(ctx, specs)
        with Dev(ctx) as dev:
            tables = []
            for prog, log, _, cols, _ in specs:
                ptrs = []
                for c in cols:
                    full = dev.empty(16 * len(c))
                    ctx.broadcast16(dev.up(c), full, len(c))
                    ptrs.append(full)
                tables.append((prog, log, 0, ptrs))
            cells = ctx.relation_program_summary(tables)
        print(cells.reports, cells.entries)
        for a, b in zip(rows.reports, cells.reports):
            assert b == dict(a, n_entries=16 * a["n_entries"])
        scale = lambda at: None if at is None else (at[0], 16 * at[1])
        assert len(rows.entries) == 1 and cells.entries == [dict(e, net=16 * e["net"] % P, n_yield=16 * e["n_yield"], n_use=16 * e["n_use"], n_other=16 * e["n_other"],
                                                                 first_yield=scale(e["first_yield"]), first_use=scale(e["first_use"])) for e in rows.entries]
    finally:
        tr.close()


# ---- 3. synthetic AIRs against the model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_size,width", [(4, 1), (5, 2), (6, 7), (12, 7), (12, 2)])
def test_one_table_against_the_model(ctx, pkg, log_size, width):
    """Less than one wave (log 4, 5), one wave (6), 64 workgroups (12); widths 1 and 7 take the 32-bit key pass. Words from {0, p - 1, 1, 7,
    2^30}, multiplicities from {0, 1, p - 1, 2, p - 2}: most tuples repeat, some cancel."""
    n = 1 << log_size
    prog = one_entry_program(pkg, [width], 0)
    cols = [drawn(100 * log_size + k, n, WORDS[: 2 + k % 4]) for k in range(width)] + [drawn(7 + log_size, n, MULTS)]
    res, want = run_both(ctx, [(prog, log_size, 0, cols, None)], [width])
    assert res.reports[0]["n_entries"] == int(np.count_nonzero(cols[-1])) < n and res.reports[0]["n_tuples"] > 1
    if (log_size, width) == (12, 2):
        assert any(e["n_other"] and e["n_yield"] and e["n_use"] for e in res.entries)


def test_two_entries_per_row_long_segment_and_truncation(ctx, pkg):
    """2^13 rows with two entries of one relation each: 16 384 entries, eight 2048-entry scan tiles. The second entry is one tuple on every
    row (a segment that spans 128 workgroups of the extraction and four scan tiles); the first is its own tuple per row, so the report is cut."""
    n = 1 << 13
    prog = one_entry_program(pkg, [2], 0, n_entries=2)
    row = np.arange(n, dtype=np.uint32)
    cols = [row, (row * 3) % 11, np.ones(n, dtype=np.uint32), np.full(n, P - 1, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.full(n, P - 1, dtype=np.uint32)]
    res, want = run_both(ctx, [(prog, 13, 0, cols, None)], [2], cap=5)
    assert res.reports[0] == {"relation": 0, "name": "relation 0", "n_words": 2, "n_entries": 2 * n, "n_tuples": n + 1, "n_unbalanced": n + 1, "n_reported": 5}
    assert res.entries[-1]["tuple"] == (4, 1) and res.lines()[-1] == "relation 0 relation: %d more unbalanced tuples not listed" % (n + 1 - 5)
    full = run_tables(ctx, [(prog, 13, 0, cols, None)], cap=n + 1)
    last = full.entries[-1]
    assert {f: last[f] for f in ENTRY_FIELDS} == {"tuple": (P - 1, 0), "net": P - n, "n_yield": 0, "n_use": n, "n_other": 0, "first_yield": None, "first_use": (0, 0)}


def three_table_specs(pkg):
    """(widths, specs) of test_three_tables_two_relations_shifts_and_an_unused_relation (tests/test_relation_model_np_cpu.py runs the numpy
    reference on them too)."""
    widths = [1, 3, 7, 2]
    b = pkg.AirBuilder()
    b.relation_entry(0, b.col(1), [b.col(0)])
    t0 = b.relation_program(widths)
    b = pkg.AirBuilder()
    c = [b.col(k) for k in range(9)]
    b.relation_entry(0, c[7], [c[0]])
    b.relation_entry(2, c[8], c[:7])
    b.relation_entry(0, c[7] * c[8] - 1, [c[1] + c[0]])
    t1 = b.relation_program(widths)
    t2 = one_entry_program(pkg, widths, 0)
    specs = [(t0, 6, 0, [drawn(1, 16, WORDS), np.array([P - 1], dtype=np.uint32)], [2, 6]),
             (t1, 9, 0, [drawn(10 + k, 512, WORDS[: 2 + k % 3]) for k in range(7)] + [drawn(20, 512, MULTS), drawn(21, 512, MULTS)], None),
             (t2, 8, 4, [drawn(30, 256, WORDS), drawn(31, 16, MULTS)], [0, 4])]
    return widths, specs


def test_three_tables_two_relations_shifts_and_an_unused_relation(ctx, pkg):
    """Three tables of 2^6, 2^9 and 2^4 evaluated rows in one call. Table 1 adds to relations 0 and 2 (and to 0 twice), table 0 and 2 to
    relation 0 only; nobody adds to relation 1 and 3. Table 0 is read at row_shift 0 with one column of shift 2 and one of shift 6 (a single
    word); table 2 at row_shift 4 with a full-size column (read at r << 4) beside row-granular ones."""
    widths, specs = three_table_specs(pkg)
    res, want = run_both(ctx, specs, widths)
    assert [r["n_words"] for r in res.reports] == widths and [r["n_entries"] for r in res.reports][1::2] == [0, 0]
    assert res.reports[0]["n_entries"] > 64 + 512 and res.reports[2]["n_entries"] > 0
    # the full-size column of table 2 is read at r << 4, not at r
    assert model.table_rows(8, 4, specs[2][3], [0, 4])[0].tolist() == specs[2][3][0][::16].tolist()
    # cap below the unbalanced count, and the counts alone
    cut, _ = run_both(ctx, specs, widths, cap=2)
    assert [r["n_reported"] for r in cut.reports] == [min(2, r["n_unbalanced"]) for r in res.reports] and res.reports[0]["n_unbalanced"] > 2
    counts = run_tables(ctx, specs, cap=0)
    assert counts.entries == [] and counts.reports == [dict(r, n_reported=0) for r in res.reports]


def test_all_multiplicities_zero(ctx, pkg):
    prog = one_entry_program(pkg, [2, 1], 0)
    res, want = run_both(ctx, [(prog, 7, 0, [drawn(1, 128, WORDS), drawn(2, 128, WORDS), np.zeros(128, dtype=np.uint32)], None)], [2, 1])
    assert res.balanced and res.entries == [] and all(r["n_entries"] == r["n_tuples"] == r["n_unbalanced"] == r["n_reported"] == 0 for r in res.reports)


# ---- 4. determinism and hygiene ------------------------------------------------------------------------------------------------------------------
def raw_summary(ctx, pkg, tables, n_rel, cap):
    """The C call on prepared ctypes tables: (status, reports, entries) with the entries as raw bytes."""
    reps, ents = (pkg.RelationReport * n_rel)(), (pkg.RelationEntry * (n_rel * cap))()
    ctypes.memset(ents, 0xAB, ctypes.sizeof(ents))
    rc = pkg.lib().bfhip_relation_program_summary(ctx._h, tables, len(tables), n_rel, reps, ents, cap)
    return rc, reps, ents


def c_tables(ctx, pkg, specs, keep):
    arr = (pkg.RelationProgramTable * len(specs))()
    for t, (prog, log, rs, ptrs, shifts) in enumerate(specs):
        pa = ctx._ptr_array(ptrs) if ptrs is not None else None
        sa = ctx._u32s(shifts) if shifts is not None else None
        keep += [pa, sa]
        arr[t] = pkg.RelationProgramTable(prog._h if prog is not None else None, log, rs, None if pa is None else ctypes.cast(pa, ctypes.POINTER(ctypes.c_void_p)),
                                          None if sa is None else ctypes.cast(sa, ctypes.POINTER(ctypes.c_uint32)))
    return arr


def test_two_runs_give_identical_bytes_and_the_arena_is_put_back(pkg):
    ctx = pkg.Context(0, max_log_domain=16)
    try:
        n = 1 << 12
        prog = one_entry_program(pkg, [3], 0)
        cols = [drawn(40 + k, n, WORDS) for k in range(3)] + [drawn(44, n, MULTS)]
        keep = []
        with Dev(ctx) as dev:
            tables = c_tables(ctx, pkg, [(prog, 12, 0, [dev.up(c) for c in cols], None)], keep)
            before = ctx.memory()["arena_in_use"]
            rc1, reps1, ents1 = raw_summary(ctx, pkg, tables, 1, 200)
            assert ctx.memory()["arena_in_use"] == before
            rc2, reps2, ents2 = raw_summary(ctx, pkg, tables, 1, 200)
        assert rc1 == rc2 == 0 and bytes(reps1) == bytes(reps2) and bytes(ents1) == bytes(ents2)
        assert 0 < reps1[0].n_reported == reps1[0].n_unbalanced < 200 and ctx.memory()["arena_in_use"] == before
        # slots beyond n_reported are not written
        assert bytes(ents1)[96 * reps1[0].n_reported:] == b"\xab" * (96 * (200 - reps1[0].n_reported))
    finally:
        ctx.close()


def test_an_open_session_refuses_the_call(ctx, pkg):
    prog = one_entry_program(pkg, [1], 0)
    ctx.set_pcs_config(pkg.PcsConfig())
    with Dev(ctx) as dev:
        cols = [dev.up(drawn(1, 64, WORDS)), dev.up(drawn(2, 64, MULTS))]
        with pkg.PcsSession(ctx):
            in_use = ctx.memory()["arena_in_use"]
            with pytest.raises(pkg.BfhipError, match=r"^bfhip_relation_program_summary: a commitment-scheme session is open on this context \(bfhip_pcs_destroy first\)$"):
                ctx.relation_program_summary([(prog, 6, 0, cols)])
            assert ctx.memory()["arena_in_use"] == in_use
        assert ctx.relation_program_summary([(prog, 6, 0, cols)]).reports[0]["n_entries"] > 0


def test_bad_arguments_are_refused_with_a_message(ctx, pkg):
    L = pkg.lib()
    err = lambda: L.bfhip_last_error().decode()
    prog, other_n, other_w = one_entry_program(pkg, [1, 2], 0), one_entry_program(pkg, [1], 0), one_entry_program(pkg, [1, 3], 0)
    keep = []
    with Dev(ctx) as dev:
        ptrs = [dev.up(np.array([5, 5, 6, 7] * 16, dtype=np.uint32)), dev.up(np.array([1, P - 1, 1, 0] * 16, dtype=np.uint32))]
        good = (prog, 6, 0, ptrs, None)
        cases = [([(None, 6, 0, ptrs, None)], 2, "table 0: null program"),
                 ([good, (other_n, 6, 0, ptrs, None)], 2, "table 1: its program was created with 1 relations, the call names 2"),
                 ([good, (other_w, 6, 0, ptrs, None)], 2, "table 1: its program gives relation 1 3 words, table 0's 2"),
                 ([good], 3, "table 0: its program was created with 2 relations, the call names 3"),
                 ([good], 0, "1 to 16 relations, got 0"),
                 ([(prog, 0, 0, ptrs, None)], 2, r"table 0: log_size must be in [1, max_log_domain = %d], got 0" % ctx.max_log_domain),
                 ([(prog, ctx.max_log_domain + 1, 0, ptrs, None)], 2, "table 0: log_size must be in"),
                 ([(prog, 6, 7, ptrs, None)], 2, "table 0: row_shift 7 above log_size 6"),
                 ([good, (prog, 6, 0, ptrs, [0, 7])], 2, "table 1: column 1 has shift 7 above log_size 6"),
                 ([(prog, 6, 0, None, None)], 2, "table 0: null column array"),
                 ([(prog, 6, 0, [ptrs[0], None], None)], 2, "table 0: null column pointer (column 1)")]
        reps, ents = (pkg.RelationReport * 3)(), (pkg.RelationEntry * 6)()
        for specs, n_rel, what in cases:
            assert L.bfhip_relation_program_summary(ctx._h, c_tables(ctx, pkg, specs, keep), len(specs), n_rel, reps, ents, 2) == -1
            assert err().startswith("bfhip_relation_program_summary: ") and what in err(), err()
        tables = c_tables(ctx, pkg, [good], keep)
        assert L.bfhip_relation_program_summary(ctx._h, None, 1, 2, reps, ents, 2) == -1 and err() == "bfhip_relation_program_summary: null argument"
        assert L.bfhip_relation_program_summary(ctx._h, tables, 1, 2, None, ents, 2) == -1 and err() == "bfhip_relation_program_summary: null argument"
        assert L.bfhip_relation_program_summary(ctx._h, tables, 1, 2, reps, None, 2) == -1 and err() == "bfhip_relation_program_summary: null argument"
        assert L.bfhip_relation_program_summary(ctx._h, tables, 0, 2, reps, ents, 2) == -1 and "1 to 64 tables, got 0" in err()
        assert L.bfhip_relation_program_summary(ctx._h, tables, 65, 2, reps, ents, 2) == -1 and "1 to 64 tables, got 65" in err()
        assert L.bfhip_relation_program_summary(None, tables, 1, 2, reps, ents, 2) == -1 and err() == "null context"
        # more than 2^31 (rows x ENTRY instructions) of one relation: 32 entries per row over 2^24 rows of 3 tables — refused before anything is read
        b = pkg.AirBuilder()
        for _ in range(32):
            b.relation_entry(0, b.col(1), [b.col(0)])
        many = b.relation_program([1, 2])
        if ctx.max_log_domain >= 24:
            big = [(many, 24, 0, ptrs, None)] * 5
            assert L.bfhip_relation_program_summary(ctx._h, c_tables(ctx, pkg, big, keep), 5, 2, reps, ents, 2) == -1 and "more than 2^31 entries" in err() and "relation 0" in err()
        # an imbalance is not an error: status 0, the error text is left as it was, and the context still computes after every refusal
        text = err()
        assert L.bfhip_relation_program_summary(ctx._h, tables, 1, 2, reps, ents, 2) == 0 and err() == text
        assert (reps[0].n_entries, reps[0].n_tuples, reps[0].n_unbalanced, reps[0].n_reported) == (48, 2, 1, 1) and reps[1].n_words == 2 and reps[1].n_entries == 0
        assert (ents[0].tuple[0], ents[0].net, ents[0].n_yield, ents[0].n_use, ents[0].first_yield_row, ents[0].first_use_table) == (6, 16, 16, 0, 2, -1)
        # a member of a shard group is refused
        group = pkg.LocalGroup(2)
        member = pkg.Context(0, max_log_domain=12)
        try:
            member.join_local_group(group, 0)
            with pytest.raises(pkg.BfhipError, match="bfhip_relation_program_summary: a context in a shard group"):
                member.relation_program_summary([(prog, 6, 0, ptrs)])
            member.leave_group()
        finally:
            member.close(); group.close()


def test_a_context_that_ran_a_summary_proves_the_same_bytes(ctx, pkg, oracle):
    code, inp = "+++>,<[>+.<-]", b"\x01"
    want = oracle.prove(code, inp, log_max_rows=20)[0]
    fresh = pkg.Context(0, max_log_domain=22)
    prog = one_entry_program(pkg, [2], 0)
    try:
        untouched = pkg.prove_brainfuck(code, inp, ctx=fresh, log_max_rows=20)
        before = pkg.prove_brainfuck(code, inp, ctx=ctx, log_max_rows=20)
        cols = [drawn(1, 1 << 10, WORDS), drawn(2, 1 << 10, WORDS), drawn(3, 1 << 10, MULTS)]
        assert not run_tables(ctx, [(prog, 10, 0, cols, None)]).balanced
        after = pkg.prove_brainfuck(code, inp, ctx=ctx, log_max_rows=20)
        assert after == before == untouched == want
    finally:
        fresh.close()


# ---- 5. the lookup example of INTEGRATION.md section 2e ------------------------------------------------------------------------------------------
def test_integration_lookup_example(ctx, pkg):
    """`a` looked up in `t` with `mult`, the trace of tests/test_gpu_air_check.py: balanced as it stands; with mult[3] changed exactly one tuple
    is reported, (t[3]), with the net the model gives, and the line is the one the document shows."""
    log_size = 6
    n = 1 << log_size
    r = pkg.AirBuilder()
    a, t, mult = r.col(0), r.col(1), r.col(2)
    r.relation_entry(0, 1, [a])
    r.relation_entry(0, -mult, [t])
    relation = r.relation_program([1])
    table = splitmix_column(51, n)
    assert len(set(table.tolist())) == n
    pick = splitmix_column(52 << 32, n) % np.uint32(n // 4)
    trace = [table[pick], table, np.bincount(pick, minlength=n).astype(np.uint32)]
    names = dict(relation_names=["lookup"], table_names=["trace"])
    res = run_tables(ctx, [(relation, log_size, 0, trace, None)], **names)
    assert res.balanced and res.lines() == [] and res.reports[0]["n_entries"] == n + int(np.count_nonzero(trace[2]))
    bad = trace[2].copy()
    bad[3] = (int(bad[3]) + 1) % P
    res = run_tables(ctx, [(relation, log_size, 0, trace[:2] + [bad], None)], **names)
    want = model.summary([(relation.code, log_size, 0, trace[:2] + [bad], None)], [1])
    print(res.reports, res.entries, want)
    assert len(want[0]["entries"]) == 1 and want[0]["entries"][0]["tuple"] == (int(table[3]),) and want[0]["entries"][0]["net"] == P - 1
    assert [{f: e[f] for f in ENTRY_FIELDS} for e in res.entries] == want[0]["entries"] and res.reports[0]["n_unbalanced"] == 1
    assert res.lines() == ["lookup relation: (729498903) net -1: yielded 6x (first: trace row 13), used 0x, 1 rows with another multiplicity"]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert res.lines()[0] in doc
