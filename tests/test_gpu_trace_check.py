"""-m gpu: the 13 AIRs asserted on the trace domain by the gfx950 kernels of csrc/check.hip (bfhip_check_constraints, bfhip_trace_check;
Context.check_constraints, Trace.check, tools/bfprove.py check) against the CPU oracle's AssertEvaluator looped over every cell
(tests/native/oracle_air_check.cpp). Every assertion is exact: integer field arithmetic, integer counters, no tolerance."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_air_check
from oracle_air_check import same_report, table_from_registers
from conftest import ROOT, P, splitmix_column

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

N_COMPONENTS = 13
NAMES = ["memory", "instruction", "program", "processor", "jnz", "jz", "input", "left", "minus", "output", "plus", "right", "end_of_execution"]
N_CONSTRAINTS = [12, 11, 5, 10, 9, 9, 7, 7, 8, 8, 8, 7, 2]
ALL_OPS = ("+++>,<[>+.<-]", b"\x01")       # brainfuck_air/mod.rs:807 — touches all 8 instructions
HELLO = ("++++++++++[>+++++++>++++++++++>+++>+<<<<-]>++.>+.+++++++..+++.>++.<<+++++++++++++++.>.+++.------.--------.>+.>.", b"")
COLLATZ = (open(os.path.join(ROOT, "tests", "golden", "programs", "collatz.bf")).read(), bytes([55, 10]))
V = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")))
ELEMS = [5, 1, 2, 3, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83]


@pytest.fixture(scope="module")
def air_check(tmp_path_factory):
    return oracle_air_check.build(tmp_path_factory.mktemp("oracle_air_check"))


def _elems(seed):
    e = splitmix_column(seed, 24)
    e[e == 0] = 1
    return e.tolist()


def n_logup(comp):
    return 3 if comp == 3 else 1


class DeviceComponent:
    """One component's columns in HBM: row-granular main columns (n_main, M) and the logUp columns bfhip_logup_generate wrote from them."""

    def __init__(self, ctx, comp, rows, elems):
        self.ctx, self.comp, self.elems = ctx, comp, elems
        self.rows = np.ascontiguousarray(rows, dtype=np.uint32)
        n_main, self.M = self.rows.shape
        self.log = int(np.log2(self.M)) + 4
        self.main = [ctx.upload(self.rows[j]) for j in range(n_main)]
        self.sizes = [self.M] * (4 * (n_logup(comp) - 1)) + [16 * self.M] * 4
        self.logup = [ctx.malloc(4 * n) for n in self.sizes]
        self.claimed = ctx.logup_generate(comp, self.log, self.main, elems, self.logup)

    def set_main(self, j, column):
        """Replaces main column j AFTER the logUp columns were generated (they keep the values of the original table)."""
        self.rows[j] = column
        self.ctx.free(self.main[j])
        self.main[j] = self.ctx.upload(self.rows[j])

    def logup_host(self):
        return [self.ctx.download(p, n) for p, n in zip(self.logup, self.sizes)]

    def set_logup(self, k, column):
        self.ctx.free(self.logup[k])
        self.logup[k] = self.ctx.upload(np.ascontiguousarray(column, dtype=np.uint32))

    def full_size(self, cols):
        """The logUp columns as the oracle lays them out: every column of 16 M cells."""
        return np.stack([c if c.size == 16 * self.M else np.repeat(c, 16) for c in cols])

    def check(self, claimed=None):
        return self.ctx.check_constraints(self.comp, self.log, self.main, self.logup, self.elems, self.claimed if claimed is None else claimed)

    def close(self):
        for p in self.main + self.logup:
            self.ctx.free(p)


def show(tag, got, want=None):
    """Every figure is printed before it is asserted on (visible with -s / in a captured failure)."""
    print(tag, {k: got[k] for k in oracle_air_check.FIELDS}, "" if want is None else {"shim": want})


def assert_clean(rep, comp, log, claimed):
    assert rep["component"] == comp and rep["log_size"] == log and rep["name"] == NAMES[comp]
    assert rep["ok"] and rep["n_bad_cells"] == 0 and rep["first_bad_cell"] is None and rep["first_bad_row"] is None and rep["first_bad_constraint"] == -1
    assert rep["first_bad_value"] == [0] * 4 and rep["bad_per_constraint"] == [0] * 16 and rep["claimed_sum"] == list(claimed)


# ---- valid programs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog", [ALL_OPS, HELLO, COLLATZ], ids=["all_ops", "hello", "collatz"])
def test_valid_tables_report_no_violation(ctx, oracle, prog):
    code, inp = prog
    elems = _elems(31)
    total = np.zeros(4, dtype=object)
    for comp in range(N_COMPONENTS):
        d = DeviceComponent(ctx, comp, oracle.table(code, inp, comp).T, elems)
        rep = d.check()
        show(NAMES[comp], rep)
        d.close()
        assert_clean(rep, comp, d.log, d.claimed)                     # claimed_sum is bfhip_logup_generate's
        assert d.claimed == oracle.logup_generate(comp, d.rows, elems)[1]
        total = (total + np.array(d.claimed, dtype=object)) % P
    assert not total.any()


# ---- the reference's ten negative cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", V["air_negative"], ids=lambda v: v["cite"].split("(")[1].split(":")[0].split(")")[0])
def test_negative_cases_of_the_reference(ctx, oracle, air_check, v):
    """memory/component.rs:211-609: table built from the registers, cells patched, logUp generated on the GPU from the patched rows."""
    rows = table_from_registers(oracle, v["trace"], [43], v["component"])
    for r, c, val in v["patch"]:
        rows[r, c] = val
    d = DeviceComponent(ctx, v["component"], rows.T, ELEMS)
    rep = d.check()
    want = air_check.check(v["component"], d.rows, ELEMS)
    show(v["cite"], rep, want)
    d.close()
    assert rep["first_bad_cell"] >> 4 == rep["first_bad_row"] == v["table_row"]
    assert rep["first_bad_constraint"] == v["constraint"] and rep["first_bad_value"] == [v["value"], 0, 0, 0]
    assert same_report(rep, want) and not rep["ok"]


# ---- randomised corruption of the main columns -------------------------------------------------------------------------------------------
N_SEEDS = 8


def corruption(comp, rows, seed):
    """1 to 8 cells of the (n_main, M) table replaced: positions and values from splitmix_column."""
    n_main, M = rows.shape
    k = 1 + seed % 8
    r = splitmix_column(7000 + 100 * comp + seed, 3 * k)
    out = rows.copy()
    for i in range(k):
        out[int(r[3 * i]) % n_main, int(r[3 * i + 1]) % M] = r[3 * i + 2]
    return out


@pytest.mark.parametrize("comp", range(N_COMPONENTS), ids=NAMES)
def test_random_corruption_matches_the_oracle(ctx, oracle, air_check, comp):
    """The logUp columns are those of the real table; the main cells are patched afterwards, so the logUp constraints see the change too."""
    code, inp = ALL_OPS
    elems = _elems(77)
    base = np.ascontiguousarray(oracle.table(code, inp, comp).T)
    d = DeviceComponent(ctx, comp, base, elems)
    inter = d.full_size(d.logup_host())
    several = 0
    try:
        for seed in range(N_SEEDS):
            bad = corruption(comp, base, seed)
            for j in range(base.shape[0]):
                if not np.array_equal(bad[j], d.rows[j]):
                    d.set_main(j, bad[j])
            rep = d.check()
            want = air_check.check(comp, bad, elems, inter=inter, claimed=d.claimed)
            show(f"{NAMES[comp]} seed {seed}", rep, want)
            assert same_report(rep, want), (seed, rep, want)
            several += sum(1 for c in rep["bad_per_constraint"] if c) > 1
    finally:
        d.close()
    assert several >= 1, "no seed with more than one failing constraint"


# ---- corruption on the logUp side, main columns intact -----------------------------------------------------------------------------------
def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def coset_successor(cell, log):
    """Storage index of the point at coset offset +1 on CanonicCoset(log): storage -> circle-domain index -> coset index, + 1, and back
    (stwo's circle_domain_index_to_coset_index / coset_index_to_circle_domain_index, restated)."""
    n = 1 << log
    d = bitrev(cell, log)
    c = 2 * d if d < n // 2 else 2 * (n - 1 - d) + 1
    c = (c + 1) % n
    return bitrev(c // 2 if c % 2 == 0 else n - (c + 1) // 2, log)


# a program of k '+' has k Plus rows, k + 1 Processor rows (one per step and the final row) and one EndOfExecution row
LAST_LOGUP_CASES = [(10, 1, 4), (10, 2, 5), (10, 20, 9), (10, 3000, 16), (12, 1, 4), (3, 1, 5), (3, 19, 9), (3, 2999, 16)]


@pytest.mark.parametrize("comp,n_plus,log", LAST_LOGUP_CASES, ids=[f"{NAMES[c]}-log{l}" for c, _, l in LAST_LOGUP_CASES])
def test_patched_last_logup_cell_fails_at_the_cell_and_its_coset_successor(ctx, oracle, air_check, comp, n_plus, log):
    """Pins the previous-row map of the TRACE domain: one patched cell i of the last logUp column breaks exactly the last logUp constraint, at
    exactly two cells — i and the cell whose predecessor i is."""
    code = "+" * n_plus
    elems = _elems(5)
    d = DeviceComponent(ctx, comp, oracle.table(code, b"", comp).T, elems)
    assert d.log == log
    n = 1 << log
    last = 4 * (n_logup(comp) - 1)
    logup_c = N_CONSTRAINTS[comp] - 1
    cols = d.logup_host()
    try:
        for i in sorted({0, 1, n - 1, n // 2, int(splitmix_column(log, 1)[0]) % n, int(splitmix_column(log + 40, 1)[0]) % n}):
            w = i % 4                                   # one coordinate of the QM31 cell
            col = cols[last + w].copy()
            col[i] = (int(col[i]) + 1) % P
            d.set_logup(last + w, col)
            rep = d.check()
            succ = coset_successor(i, log)
            patched = [c.copy() for c in cols]; patched[last + w] = col
            want = air_check.check(comp, d.rows, elems, inter=d.full_size(patched), claimed=d.claimed)
            show(f"{NAMES[comp]} log {log} cell {i} successor {succ}", rep, want)
            d.set_logup(last + w, cols[last + w])
            assert succ != i and rep["n_bad_cells"] == 2
            assert rep["bad_per_constraint"] == [2 if j == logup_c else 0 for j in range(16)]
            assert rep["first_bad_cell"] == min(i, succ) and rep["first_bad_constraint"] == logup_c
            assert same_report(rep, want)
    finally:
        d.close()


@pytest.mark.parametrize("comp", [0, 3, 12], ids=["memory", "processor", "end_of_execution"])
def test_patched_claimed_sum_fails_at_cell_zero_only(ctx, oracle, air_check, comp):
    code, inp = ALL_OPS
    elems = _elems(6)
    d = DeviceComponent(ctx, comp, oracle.table(code, inp, comp).T, elems)
    claimed = list(d.claimed); claimed[2] = (claimed[2] + 1) % P
    rep = d.check(claimed=claimed)
    want = air_check.check(comp, d.rows, elems, inter=d.full_size(d.logup_host()), claimed=claimed)
    show(NAMES[comp], rep, want)
    d.close()
    assert rep["n_bad_cells"] == 1 and rep["first_bad_cell"] == 0 and rep["first_bad_constraint"] == N_CONSTRAINTS[comp] - 1
    assert rep["bad_per_constraint"] == [1 if j == N_CONSTRAINTS[comp] - 1 else 0 for j in range(16)] and rep["claimed_sum"] == claimed
    assert same_report(rep, want)


@pytest.mark.parametrize("which,failing", [(0, (7, 8)), (1, (8, 9))], ids=["first_column", "second_column"])
def test_patched_non_final_processor_logup_cell_fails_in_the_16_cells_of_its_row(ctx, oracle, air_check, which, failing):
    """processor/component.rs:79-153: logUp column k holds the running sum of the row's first k + 1 fractions. Constraint 7 + k reads column k and
    column k - 1, so a patched cell of column k breaks its own constraint and the NEXT one (which subtracts it) — in the 16 cells the row stands
    for, since both columns are 16-lane broadcasts. Derived from the oracle's evaluation (the shim) and pinned here."""
    code, inp = ALL_OPS
    elems = _elems(8)
    d = DeviceComponent(ctx, 3, oracle.table(code, inp, 3).T, elems)
    cols = d.logup_host()
    row = 5 % d.M
    k = 4 * which + 1                                   # one coordinate of the row-granular column
    col = cols[k].copy(); col[row] = (int(col[row]) + 1) % P
    d.set_logup(k, col)
    rep = d.check()
    patched = [c.copy() for c in cols]; patched[k] = col
    want = air_check.check(3, d.rows, elems, inter=d.full_size(patched), claimed=d.claimed)
    show(f"processor logUp column {which} row {row}", rep, want)
    d.close()
    assert rep["n_bad_cells"] == 16 and rep["first_bad_cell"] == 16 * row and rep["first_bad_constraint"] == failing[0]
    assert rep["bad_per_constraint"] == [16 if j in failing else 0 for j in range(16)]
    assert same_report(rep, want)


# ---- large components --------------------------------------------------------------------------------------------------------------------
def test_large_components(ctx, pkg, oracle, air_check):
    """A 2^20-cell component (the Plus table of 40000 '+'): valid, then one patch in the last table row and one in row 0 together. And a
    2^24-cell one (600000 '+'), valid, when 4 GiB of device memory are free."""
    elems = _elems(9)
    comp = 10
    rows = np.ascontiguousarray(oracle.table("+" * 40000, b"", comp).T)
    d = DeviceComponent(ctx, comp, rows, elems)
    try:
        assert d.log == 20
        rep = d.check()
        show("plus 2^20 valid", rep)
        assert_clean(rep, comp, 20, d.claimed)
        inter = d.full_size(d.logup_host())
        M = d.M
        mv = rows[5].copy(); mv[M - 1] = 77               # a padding row with mv != 0: d * mv
        d.set_main(5, mv)
        last_only = d.check()
        nmv = rows[10].copy(); nmv[0] = 9                 # row 0: next_mv - mv - 1 != 0
        d.set_main(10, nmv)
        both = d.check()
        want = air_check.check(comp, d.rows, elems, inter=inter, claimed=d.claimed)
        show("plus 2^20 last row", last_only)
        show("plus 2^20 last row and row 0", both, want)
        assert last_only["first_bad_row"] == M - 1 and last_only["n_bad_cells"] == 16
        assert both["first_bad_row"] == 0 and both["first_bad_cell"] == want["first_bad_cell"] and both["n_bad_cells"] == 32
        assert same_report(both, want)
    finally:
        d.close()
    free, _ = pkg.device_memory(0)
    print("free device memory", free)
    if free >= 4 << 30:
        d = DeviceComponent(ctx, comp, oracle.table("+" * 600000, b"", comp).T, elems)
        try:
            assert d.log == 24
            rep = d.check()
            show("plus 2^24 valid", rep)
            assert_clean(rep, comp, 24, d.claimed)
        finally:
            d.close()


# ---- Trace.check ---------------------------------------------------------------------------------------------------------------------------
def shim_reports_of_trace(pkg, air_check, tr, elems):
    """The oracle's report of every component on the tables of a resident trace (read back with Trace.column), and the logUp total."""
    reports, total = [], np.zeros(4, dtype=object)
    for comp in range(N_COMPONENTS):
        n_main = [8, 8, 4, 9, 13, 13, 11, 11, 11, 11, 11, 11, 7][comp]
        rows = np.stack([tr.column(comp, j) for j in range(n_main)])
        reports.append(air_check.check(comp, rows, elems))
        total = (total + np.array(reports[-1]["claimed_sum"], dtype=object)) % P
    return reports, tuple(int(v) for v in total)


@pytest.mark.parametrize("prog", [ALL_OPS, HELLO], ids=["all_ops", "hello"])
def test_trace_check_accepts_a_real_execution(ctx, pkg, oracle, air_check, prog):
    code, inp = prog
    tr = pkg.Trace(ctx, code, inp)
    try:
        res = tr.check()
        print([pkg.format_check_failure(r) for r in res], res.logup_total)
        assert res.ok and res.n_bad_components == 0 and res.logup_total == (0, 0, 0, 0) and res.failures() == []
        assert len(res) == 13 and [r["log_size"] for r in res] == tr.log_sizes == oracle.log_sizes(code, inp)[0]
        # the documented default elements reproduce the report, and it is the oracle's
        again = tr.check(pkg.default_check_lookup())
        assert list(again) == list(res) and again.logup_total == res.logup_total
        want, total = shim_reports_of_trace(pkg, air_check, tr, pkg.default_check_lookup())
        assert total == (0, 0, 0, 0) and all(same_report(g, w) for g, w in zip(res, want))
        other = tr.check(_elems(3))
        assert other.ok and [r["claimed_sum"] for r in other] != [r["claimed_sum"] for r in res]
    finally:
        tr.close()


def altered_registers(oracle):
    code, inp = ALL_OPS
    _, regs = oracle.run(code, inp)
    regs = regs.copy()
    assert regs[1, 2] == ord("+") and regs[1, 5] == 1      # row 1: after the first '+', mv = 1
    regs[1, 5] = 5                                         # a VM that adds 5
    return code, inp, regs


def test_trace_check_names_what_a_failing_proof_does_not(ctx, pkg, oracle, air_check):
    """One register of one row altered: the proof says ConstraintsNotSatisfied, the check says where — and both agree on valid / invalid."""
    code, inp, regs = altered_registers(oracle)
    words = oracle.compile(code)
    good = pkg.Trace.from_registers(ctx, oracle.run(code, inp)[1], words)
    bad = pkg.Trace.from_registers(ctx, regs, words)
    try:
        res = bad.check()
        for line in res.failures():
            print(line)
        want, total = shim_reports_of_trace(pkg, air_check, bad, pkg.default_check_lookup())
        assert not res.ok and res.n_bad_components >= 1
        assert {r["name"] for r in res if not r["ok"]} == {NAMES[k] for k in range(13) if want[k]["n_bad_cells"]}
        assert all(same_report(g, w) for g, w in zip(res, want)), [(g, w) for g, w in zip(res, want) if not same_report(g, w)]
        assert res.logup_total == total
        assert res.failures()[0] == pkg.format_check_failure(next(r for r in res if not r["ok"]))
        with pytest.raises(pkg.BfhipError, match="ConstraintsNotSatisfied"):
            bad.prove(20)
        assert good.check().ok
        proof, _ = good.prove(20)
        assert proof == oracle.prove(code, inp, log_max_rows=20)[0]
    finally:
        good.close(); bad.close()


def test_a_context_that_ran_a_check_proves_the_same_bytes(ctx, pkg, oracle):
    code, inp = HELLO
    want = oracle.prove(code, inp, log_max_rows=20)[0]
    fresh = pkg.Context(0, max_log_domain=22)
    tr_fresh = pkg.Trace(fresh, code, inp)
    tr = pkg.Trace(ctx, code, inp)
    try:
        untouched = tr_fresh.prove(20)[0]
        before = tr.prove(20)[0]
        assert tr.check().ok
        after = tr.prove(20)[0]
        assert tr.check(_elems(4)).ok
        assert tr.prove(20)[0] == after == before == untouched == want
    finally:
        tr.close(); tr_fresh.close(); fresh.close()


def test_the_reference_failure_line_end_to_end(ctx, oracle, pkg):
    """memory/component.rs:368-403 (mp jumps by 2) through the public formatter: the line a user reads."""
    v = next(x for x in V["air_negative"] if "mp jumps by 2" in x["cite"])
    d = DeviceComponent(ctx, 0, table_from_registers(oracle, v["trace"], [43], 0).T, ELEMS)
    rep = d.check()
    d.close()
    assert pkg.format_check_failure(rep) == "memory: constraint 6 fails at table row 0 (cell 0), value (2, 0, 0, 0); 16 cells violate it"


# ---- bad arguments -------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_a_message(ctx, pkg, oracle):
    L = pkg.lib()
    code, inp = ALL_OPS
    d = DeviceComponent(ctx, 0, oracle.table(code, inp, 0).T, ELEMS)
    rep = pkg.CheckReport()
    main, logup = ctx._ptr_array(d.main), ctx._ptr_array(d.logup)
    lk, cl = ctx._u32s(ELEMS), ctx._u32s(d.claimed)
    err = lambda: L.bfhip_last_error().decode()
    try:
        assert L.bfhip_check_constraints(ctx._h, 13, d.log, main, logup, lk, cl, ctypes.byref(rep)) == -1 and "unknown component" in err()
        assert L.bfhip_check_constraints(ctx._h, -1, d.log, main, logup, lk, cl, ctypes.byref(rep)) == -1 and "unknown component" in err()
        assert L.bfhip_check_constraints(ctx._h, 0, 3, main, logup, lk, cl, ctypes.byref(rep)) == -1 and "LOG_N_LANES" in err()
        assert L.bfhip_check_constraints(ctx._h, 0, 30, main, logup, lk, cl, ctypes.byref(rep)) == -1 and "2^29" in err()
        for args in [(None, logup, lk, cl, ctypes.byref(rep)), (main, None, lk, cl, ctypes.byref(rep)), (main, logup, None, cl, ctypes.byref(rep)),
                     (main, logup, lk, None, ctypes.byref(rep)), (main, logup, lk, cl, None)]:
            assert L.bfhip_check_constraints(ctx._h, 0, d.log, *args) == -1 and "null" in err()
        holes = ctx._ptr_array(d.main[:3] + [None] + d.main[4:])
        assert L.bfhip_check_constraints(ctx._h, 0, d.log, holes, logup, lk, cl, ctypes.byref(rep)) == -1 and "null main column" in err()
        assert L.bfhip_check_constraints(None, 0, d.log, main, logup, lk, cl, ctypes.byref(rep)) == -1 and "null context" in err()
        tr = pkg.Trace(ctx, code, inp)
        reps, total = (pkg.CheckReport * 13)(), (ctypes.c_uint32 * 4)()
        assert L.bfhip_trace_check(ctx._h, None, None, reps, total, None) == -1 and "null" in err()
        assert L.bfhip_trace_check(ctx._h, tr._h, None, None, total, None) == -1 and "null" in err()
        assert L.bfhip_trace_check(ctx._h, tr._h, None, reps, None, None) == -1 and "null" in err()
        assert L.bfhip_trace_check(None, tr._h, None, reps, total, None) == -1 and "null context" in err()
        assert L.bfhip_trace_check(ctx._h, tr._h, None, reps, total, None) == 0          # n_bad_components is optional
        # a check that finds violations is not an error: status 0, and the error text is left as it was
        with pytest.raises(pkg.BfhipError, match="unknown component"):
            ctx.check_constraints(13, d.log, d.main, d.logup, ELEMS, d.claimed)
        bad = d.rows[3].copy(); bad[1] = 2
        d.set_main(3, bad)
        main = ctx._ptr_array(d.main)
        assert L.bfhip_check_constraints(ctx._h, 0, d.log, main, logup, lk, cl, ctypes.byref(rep)) == 0
        assert rep.n_bad_cells > 0 and err() == "unknown component"
        # a member of a shard group is refused
        group = pkg.LocalGroup(2)
        member = pkg.Context(0, max_log_domain=12)
        try:
            member.join_local_group(group, 0)
            with pytest.raises(pkg.BfhipError, match="shard group"):
                member.check_constraints(0, d.log, d.main, d.logup, ELEMS, d.claimed)
            assert L.bfhip_trace_check(member._h, tr._h, None, reps, total, None) == -1 and "shard group" in err()
            member.leave_group()
        finally:
            member.close(); group.close()
        tr.close()
    finally:
        d.close()


# ---- tools/bfprove.py check ----------------------------------------------------------------------------------------------------------------
def test_bfprove_check(ctx, pkg, oracle):
    code, inp, regs = altered_registers(oracle)
    tool = [sys.executable, os.path.join(ROOT, "tools", "bfprove.py"), "check", "--code", code]
    good = subprocess.run(tool, input=inp, capture_output=True, timeout=300)
    print(good.stdout.decode(), good.stderr.decode())
    assert good.returncode == 0 and good.stdout.decode().strip() == "ok"
    bad = subprocess.run(tool + ["--set-register", "1:mv=5"], input=inp, capture_output=True, timeout=300)
    print(bad.stdout.decode(), bad.stderr.decode())
    tr = pkg.Trace.from_registers(ctx, regs, oracle.compile(code))
    want = tr.check().failures()
    tr.close()
    assert bad.returncode == 1 and bad.stdout.decode().strip().split("\n") == want and len(want) >= 1
    assert "ok" not in bad.stdout.decode().split()
