"""-m gpu: the lookup tuples that do not cancel, by the gfx950 kernels of csrc/relations.hip (bfhip_relation_summary, bfhip_trace_relations;
Context.relation_summary, Trace.relations, tools/bfprove.py relations) against the Counter model of tests/relation_model.py. Every comparison
is exact: integer counts, M31 sums, table indices and rows."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import relation_model
from conftest import ROOT, P, splitmix_column
from test_relations_cpu import ALL_OPS, UNKNOWN_TUPLE, unknown_opcode_registers

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

HELLO = ("++++++++++[>+++++++>++++++++++>+++>+<<<<-]>++.>+.+++++++..+++.>++.<<+++++++++++++++.>.+++.------.--------.>+.>.", b"")
COLLATZ = (open(os.path.join(ROOT, "tests", "golden", "programs", "collatz.bf")).read(), bytes([55, 10]))
N_MAIN = [8, 8, 4, 9, 13, 13, 11, 11, 11, 11, 11, 11, 7]
ENTRY_FIELDS = ("tuple", "net", "n_yield", "n_use", "n_other", "first_yield", "first_use")


class DeviceTables:
    """Tables [(component, (n_main, n_rows) array)] in HBM, as Context.relation_summary takes them."""

    def __init__(self, ctx, tables):
        self.ctx, self.ptrs, self.args = ctx, [], []
        for comp, cols in tables:
            cols = np.ascontiguousarray(cols, dtype=np.uint32)
            assert cols.shape[0] == N_MAIN[comp] and cols.shape[1] & (cols.shape[1] - 1) == 0
            p = [ctx.upload(c) for c in cols]
            self.ptrs += p
            self.args.append((comp, int(np.log2(cols.shape[1])) + 4, p))

    def summary(self, max_entries=64):
        return self.ctx.relation_summary(self.args, max_entries)

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)


def assert_same(res, model, cap=64):
    """Every count and every reported entry field against the model; the model's list cut at the cap."""
    for r in range(3):
        rep, want = res.reports[r], model[r]
        got = [e for e in res.entries if e["relation"] == r]
        print(rep, got[:8], "model", want["n_entries"], want["n_tuples"], len(want["entries"]), want["entries"][:8])
        assert (rep["relation"], rep["n_words"]) == (r, 7 if r == 2 else 3)
        assert (rep["n_entries"], rep["n_tuples"], rep["n_unbalanced"]) == (want["n_entries"], want["n_tuples"], len(want["entries"]))
        assert rep["n_reported"] == min(cap, len(want["entries"])) == len(got)
        assert [{f: e[f] for f in ENTRY_FIELDS} for e in got] == want["entries"][:cap]
    assert res.balanced == all(not m["entries"] for m in model)


def run_both(ctx, tables, cap=64):
    d = DeviceTables(ctx, tables)
    try:
        res = d.summary(cap)
    finally:
        d.close()
    model = relation_model.relations(tables)
    assert_same(res, model, cap)
    return res, model


def trace_tables(tr):
    return [(k, np.stack([tr.column(k, j) for j in range(N_MAIN[k])])) for k in range(13)]


# ---- resident traces ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog", [ALL_OPS, HELLO, COLLATZ], ids=["all_ops", "hello", "collatz"])
def test_real_executions_are_balanced(ctx, pkg, prog):
    tr = pkg.Trace(ctx, *prog)
    try:
        res = tr.relations()
        model = relation_model.relations(trace_tables(tr))
        assert_same(res, model)
        assert res.balanced and res.entries == [] and res.lines() == [] and all(r["n_unbalanced"] == 0 and r["n_entries"] > 0 for r in res.reports)
        assert tr.check().logup_total == (0, 0, 0, 0)
    finally:
        tr.close()


def test_unknown_opcode_is_invisible_to_the_check_and_named_by_the_relations(ctx, pkg, oracle):
    regs, words = unknown_opcode_registers(oracle)
    tr = pkg.Trace.from_registers(ctx, regs, words)
    try:
        chk = tr.check()
        print(chk.failures())
        assert chk.n_bad_components == 0 and any(chk.logup_total) and not chk.ok
        res = tr.relations()
        print(res.lines())
        assert_same(res, relation_model.relations(trace_tables(tr)))
        assert not res.balanced and [r["n_unbalanced"] for r in res.reports] == [0, 0, 1]
        assert res.entries == [{"relation": 2, "name": "processor", "tuple": UNKNOWN_TUPLE, "net": 1, "n_yield": 1, "n_use": 0, "n_other": 0,
                                "first_yield": (3, 1), "first_use": None}]
        assert res.lines() == ["processor relation: (1, 1, 35, 43, 0, 1, 1) net +1: yielded 1x (first: processor row 1), used 0x"]
        # counts only
        counts = tr.relations(max_entries=0)
        assert counts.reports == [dict(r, n_reported=0) for r in res.reports] and counts.entries == [] and not counts.balanced
    finally:
        tr.close()


# ---- caller-supplied tables -----------------------------------------------------------------------------------------------------------------
def processor_table(tuples, rows=None):
    """Processor rows yielding `tuples` (7 words each), padded with dummy rows to `rows` (a power of two)."""
    n = len(tuples)
    rows = rows or max(1, 1 << (n - 1).bit_length())
    cols = np.zeros((9, rows), dtype=np.uint32)
    cols[7, n:] = 1
    if n:
        cols[:7, :n] = np.array(tuples, dtype=np.uint32).T
    return cols


def opcode_table(comp, tuples, rows=None):
    """Rows of an opcode table (input .. right: d = column 7; jnz, jz: d = column 11) using `tuples`, padded with dummy rows."""
    n = len(tuples)
    rows = rows or max(1, 1 << (n - 1).bit_length())
    cols = np.zeros((N_MAIN[comp], rows), dtype=np.uint32)
    cols[11 if comp in (4, 5) else 7, n:] = 1
    if n:
        cols[:7, :n] = np.array(tuples, dtype=np.uint32).T
    return cols


def test_long_segment_and_truncation(ctx):
    """2^13 Processor rows with one (ip, ci, ni): one Instruction tuple whose segment spans four 2048-entry scan tiles and 32 workgroups; every
    row is its own Memory and Processor tuple, so those two relations have 8192 unbalanced tuples each and the report is cut at 5."""
    n = 1 << 13
    clk = np.arange(n)
    tuples = np.stack([clk, np.full(n, 5), np.full(n, 43), np.full(n, 62), clk % 7, (clk * 3) % 11, np.zeros(n, dtype=np.int64)], axis=1)
    res, model = run_both(ctx, [(3, processor_table(tuples))], cap=5)
    assert [r["n_unbalanced"] for r in res.reports] == [n, 1, n] and [r["n_reported"] for r in res.reports] == [5, 1, 5]
    ins = [e for e in res.entries if e["relation"] == 1]
    assert ins == [{"relation": 1, "name": "instruction", "tuple": (5, 43, 62), "net": n, "n_yield": n, "n_use": 0, "n_other": 0, "first_yield": (0, 0), "first_use": None}]
    assert [e["tuple"][0] for e in res.entries if e["relation"] == 2] == [0, 1, 2, 3, 4]
    assert len(res.lines()) == 11 + 2 and res.lines()[-1] == "processor relation: 8187 more unbalanced tuples not listed"


WORDS = [0, 1, 1 << 16, 1 << 30, P - 2, P - 1]


def sort_order_tables(seed):
    """The tables of test_sort_order_and_key_packing (tests/test_relation_model_np_cpu.py runs the numpy reference on them too)."""
    r = splitmix_column(1000 * seed, 7 + 60)
    t = [WORDS[int(v) % 6] for v in r[:7]]
    tuples = [tuple(t)]
    for i in range(47):
        t[i % 7] = WORDS[(WORDS.index(t[i % 7]) + 1 + int(r[7 + i]) % 5) % 6]       # another value of the set
        tuples.append(tuple(t))
    yields, uses = [], []
    for i, tup in enumerate(tuples):
        yields += [tup] * (3 if i % 3 < 2 else 0)
        uses += [tup] * (3 if i % 3 == 0 else 2 if i % 3 == 1 else 1)
    order = np.argsort(splitmix_column(seed, len(yields)), kind="stable")
    yields = [yields[k] for k in order]
    order = np.argsort(splitmix_column(seed + 50, len(uses)), kind="stable")
    uses = [uses[k] for k in order]
    proc = processor_table(yields)
    assert 64 <= proc.shape[1] <= 512
    return [(10, opcode_table(10, uses[: len(uses) // 3])), (3, proc), (10, opcode_table(10, uses[len(uses) // 3:]))]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sort_order_and_key_packing(ctx, seed):
    """Tuples over {0, 1, 2^16, 2^30, p - 2, p - 1}, each differing from its neighbour in ONE word, every word position in turn: a sort pass
    that drops or swaps a word of its key, or is not stable, orders or merges them differently from the model. Pattern by tuple: yielded 3x
    and used 3x (balanced: absent), yielded 3x and used 2x (net 1), used only (net p - 1). Uses are split over two plus tables."""
    res, model = run_both(ctx, sort_order_tables(seed))
    nets = [e["net"] for e in res.entries if e["relation"] == 2]
    assert 1 in nets and P - 1 in nets and res.reports[2]["n_tuples"] > res.reports[2]["n_unbalanced"] > 0
    assert res.reports[0]["n_unbalanced"] > 1 and res.reports[1]["n_unbalanced"] > 1        # the 3-word relations see the Processor rows only


def test_multiplicities_that_are_not_boolean(ctx):
    """A Memory row with d = 2 has numerator 1 (counted as a yield), d = 3 has numerator 2 (counted as other); net is the field sum."""
    mem = np.zeros((8, 16), dtype=np.uint32)
    mem[3] = 1                                             # dummy rows
    rows = [((7, 1, 2), 0), ((7, 1, 2), 2), ((7, 1, 2), 3), ((7, 1, 2), 3), ((9, 1, 2), 2), ((9, 1, 2), 0), ((8, 0, 0), 3), ((6, 0, 0), P - 1)]
    for i, (tup, d) in enumerate(rows):
        mem[0:3, i] = tup
        mem[3, i] = d
    res, model = run_both(ctx, [(0, mem)])
    by_tuple = {e["tuple"]: e for e in res.entries}
    assert res.reports[0]["n_entries"] == 8 and res.reports[0]["n_tuples"] == 4 and res.reports[0]["n_unbalanced"] == 3      # (9, 1, 2) cancels
    e = by_tuple[(7, 1, 2)]
    assert (e["net"], e["n_yield"], e["n_use"], e["n_other"], e["first_yield"], e["first_use"]) == (4, 1, 1, 2, (0, 1), (0, 0))
    assert (by_tuple[(8, 0, 0)]["net"], by_tuple[(8, 0, 0)]["n_other"], by_tuple[(8, 0, 0)]["first_yield"]) == (2, 1, None)
    assert (by_tuple[(6, 0, 0)]["net"], by_tuple[(6, 0, 0)]["n_other"]) == (P - 2, 1)


def test_edges(ctx):
    tup = (3, 9, 0, 0, 2, 5, 4)
    # one-row tables: the Processor row is consumed by end_of_execution; its Memory and Instruction tuples have no user
    res, _ = run_both(ctx, [(3, processor_table([tup])), (12, np.array(tup, dtype=np.uint32).reshape(7, 1))])
    assert [r["n_unbalanced"] for r in res.reports] == [1, 1, 0] and res.reports[2]["n_entries"] == 2
    # every row a dummy: no entry anywhere, nothing launched on an empty list; the Program-less, Instruction-less list leaves relation 1 to the Processor
    dummy = [(3, processor_table([], 4)), (10, opcode_table(10, [], 2)), (4, opcode_table(4, [], 1)), (0, np.tile(np.array([[0], [0], [0], [1], [1], [0], [0], [1]], dtype=np.uint32), (1, 8)))]
    res, _ = run_both(ctx, dummy)
    assert res.balanced and res.entries == [] and all(r["n_entries"] == r["n_tuples"] == r["n_unbalanced"] == r["n_reported"] == 0 for r in res.reports)
    # no table touches relations 0 and 1
    res, _ = run_both(ctx, [(12, np.array(tup, dtype=np.uint32).reshape(7, 1))])
    assert [r["n_entries"] for r in res.reports] == [0, 0, 1]
    assert res.entries == [{"relation": 2, "name": "processor", "tuple": tup, "net": P - 1, "n_yield": 0, "n_use": 1, "n_other": 0, "first_yield": None, "first_use": (0, 0)}]
    assert res.lines() == ["processor relation: (3, 9, 0, 0, 2, 5, 4) net -1: yielded 0x, used 1x (first: end_of_execution[0] row 0)"]


def test_a_context_that_ran_relations_proves_the_same_bytes(ctx, pkg, oracle):
    code, inp = HELLO
    want = oracle.prove(code, inp, log_max_rows=20)[0]
    fresh = pkg.Context(0, max_log_domain=22)
    tr_fresh = pkg.Trace(fresh, code, inp)
    tr = pkg.Trace(ctx, code, inp)
    try:
        untouched = tr_fresh.prove(20)[0]
        before = tr.prove(20)[0]
        assert tr.relations().balanced
        after = tr.prove(20)[0]
        assert tr.relations(max_entries=3).balanced
        assert tr.prove(20)[0] == after == before == untouched == want
    finally:
        tr.close(); tr_fresh.close(); fresh.close()


# ---- bad arguments --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_a_message(ctx, pkg):
    L = pkg.lib()
    err = lambda: L.bfhip_last_error().decode()
    tup = (3, 9, 0, 0, 2, 5, 4)
    d = DeviceTables(ctx, [(3, processor_table([tup, tup]))])
    tr = pkg.Trace(ctx, *ALL_OPS)
    reps, ents = (pkg.RelationReport * 3)(), (pkg.RelationEntry * 6)()
    table = lambda comp, log, ptrs: (pkg.RelationTable * 1)(pkg.RelationTable(comp, log, None if ptrs is None else ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))))
    ptrs = ctx._ptr_array(d.args[0][2])
    try:
        good = table(3, 5, ptrs)
        for comp in (13, -1):
            assert L.bfhip_relation_summary(ctx._h, table(comp, 5, ptrs), 1, reps, ents, 2) == -1 and "unknown component" in err()
        assert L.bfhip_relation_summary(ctx._h, table(3, 3, ptrs), 1, reps, ents, 2) == -1 and "LOG_N_LANES" in err()
        assert L.bfhip_relation_summary(ctx._h, table(3, 30, ptrs), 1, reps, ents, 2) == -1 and "2^29" in err()
        assert L.bfhip_relation_summary(ctx._h, table(3, 5, None), 1, reps, ents, 2) == -1 and "null main column array" in err()
        holes = ctx._ptr_array(d.args[0][2][:4] + [None] + d.args[0][2][5:])
        assert L.bfhip_relation_summary(ctx._h, table(3, 5, holes), 1, reps, ents, 2) == -1 and "null main column pointer" in err()
        assert L.bfhip_relation_summary(ctx._h, None, 1, reps, ents, 2) == -1 and "null" in err()
        assert L.bfhip_relation_summary(ctx._h, good, 1, None, ents, 2) == -1 and "null" in err()
        assert L.bfhip_relation_summary(ctx._h, good, 1, reps, None, 2) == -1 and "null" in err()
        assert L.bfhip_relation_summary(ctx._h, good, 0, reps, ents, 2) == -1 and "1 to 64 tables" in err()
        assert L.bfhip_relation_summary(ctx._h, good, 65, reps, ents, 2) == -1 and "1 to 64 tables" in err()
        assert L.bfhip_relation_summary(None, good, 1, reps, ents, 2) == -1 and "null context" in err()
        assert L.bfhip_trace_relations(ctx._h, None, reps, ents, 2) == -1 and "null" in err()
        assert L.bfhip_trace_relations(ctx._h, tr._h, None, ents, 2) == -1 and "null" in err()
        assert L.bfhip_trace_relations(ctx._h, tr._h, reps, None, 2) == -1 and "null" in err()
        assert L.bfhip_trace_relations(None, tr._h, reps, ents, 2) == -1 and "null context" in err()
        with pytest.raises(pkg.BfhipError, match="takes 9 main columns"):
            ctx.relation_summary([(3, 5, d.args[0][2][:8])])
        with pytest.raises(pkg.BfhipError, match="unknown component"):
            ctx.relation_summary([(13, 5, d.args[0][2])])
        # an imbalance is not an error: status 0, and the error text is left as it was
        assert L.bfhip_relation_summary(ctx._h, good, 1, reps, ents, 2) == 0 and reps[2].n_unbalanced == 1 and ents[4].net == 2 and err() == "unknown component"
        assert L.bfhip_relation_summary(ctx._h, good, 1, reps, None, 0) == 0 and reps[2].n_unbalanced == 1 and reps[2].n_reported == 0
        assert L.bfhip_trace_relations(ctx._h, tr._h, reps, None, 0) == 0 and reps[2].n_unbalanced == 0
        # a member of a shard group is refused
        group = pkg.LocalGroup(2)
        member = pkg.Context(0, max_log_domain=12)
        try:
            member.join_local_group(group, 0)
            with pytest.raises(pkg.BfhipError, match="shard group"):
                member.relation_summary(d.args)
            assert L.bfhip_trace_relations(member._h, tr._h, reps, ents, 2) == -1 and "shard group" in err()
            member.leave_group()
        finally:
            member.close(); group.close()
    finally:
        tr.close(); d.close()


# ---- tools/bfprove.py relations -------------------------------------------------------------------------------------------------------------
def test_bfprove_relations():
    code, inp = ALL_OPS
    tool = [sys.executable, os.path.join(ROOT, "tools", "bfprove.py"), "relations", "--code", code]
    good = subprocess.run(tool, input=inp, capture_output=True, timeout=300)
    print(good.stdout.decode(), good.stderr.decode())
    assert good.returncode == 0 and good.stdout.decode().strip() == "balanced"
    bad = subprocess.run(tool + ["--set-register", "1:ci=35", "--set-register", "0:ni=35", "--set-word", "1=35"], input=inp, capture_output=True, timeout=300)
    print(bad.stdout.decode(), bad.stderr.decode())
    assert bad.returncode == 1
    assert bad.stdout.decode().strip().split("\n") == ["processor relation: (1, 1, 35, 43, 0, 1, 1) net +1: yielded 1x (first: processor row 1), used 0x"]
