"""-m gpu: a proof's preflight (include/bfhip.h bfhip_ctx_set_preflight / bfhip_pool_set_preflight; csrc/prover_preflight.hip, the batched
kernels k_check_batch / k_check_first_batch of csrc/check.hip). With the switch on, every proving entry point first asserts the 13 AIRs and
the logUp total on its tables: a valid trace is proved to the same bytes, an invalid one is refused with BFHIP_TRACE_REJECTED and the lines
of Trace.check() / Trace.relations(). Every report is compared with the unbatched bfhip_trace_check on the same tables, with the CPU oracle's
AssertEvaluator (tests/oracle_air_check.py) and, for the tuples, with the Counter model of tests/relation_model.py: exact, no tolerance.
Tables that no register trace produces (one component corrupted alone) are written into a resident trace with the test-hooks build's
bfhip_test_trace_set_column."""
import ctypes

import numpy as np
import pytest

import oracle_air_check
import relation_model
from oracle_air_check import same_report
from test_gpu_relations import assert_same, trace_tables
from test_gpu_trace_check import V, shim_reports_of_trace
from test_relations_cpu import UNKNOWN_TUPLE

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

PROG = ("++>,<[>+.<-]", b"\x01")      # its input and output components are single-row, 16-cell tables: less than one wave
LMR = 14
BIG = ("+" * 3000, b"")               # Plus, Memory, Program and Processor tables of 2^16 cells (256 workgroups), Instruction 2^17
BIG_LMR = 17
N_MAIN = [8, 8, 4, 9, 13, 13, 11, 11, 11, 11, 11, 11, 7]
# a main column of each component whose change in one table row breaks a constraint in the 16 cells of that row (checked against the
# oracle below): the dummy column d where the AIR asserts d (d - 1) = 0, mv_inv for the processor, ci for end_of_execution
BREAKS = {0: 3, 1: 3, 2: 3, 3: 8, 4: 11, 5: 11, 6: 7, 7: 7, 8: 7, 9: 7, 10: 7, 11: 7, 12: 2}


@pytest.fixture(scope="module")
def air_check(tmp_path_factory):
    return oracle_air_check.build(tmp_path_factory.mktemp("oracle_air_check"))


@pytest.fixture(scope="module")
def wanted():
    return {}


def want_proof(oracle, wanted, prog=PROG, lmr=LMR):
    if (prog, lmr) not in wanted:
        wanted[(prog, lmr)] = oracle.prove(*prog, log_max_rows=lmr)[0]
    return wanted[(prog, lmr)]


@pytest.fixture(scope="module")
def pctx(pkg):
    c = pkg.Context(0, max_log_domain=LMR + 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hctx(hooks_pkg):
    """A context of the test-hooks build (its traces can be overwritten column by column)."""
    c = hooks_pkg.Context(0, max_log_domain=BIG_LMR + 2)
    yield c
    c.close()


def machine(pkg, prog=PROG):
    return pkg.host_run(*prog)[1], pkg.host_compile(prog[0])


def set_column(hooks_pkg, tr, comp, col, values):
    v = np.ascontiguousarray(values, dtype=np.uint32)
    rc = hooks_pkg.lib().bfhip_test_trace_set_column(tr.ctx._h, tr._h, comp, col, v.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(v.size))
    assert rc == 0, hooks_pkg.lib().bfhip_last_error().decode()


def break_row(hooks_pkg, tr, comp, row):
    """Adds 2 to the BREAKS column of one table row of a resident trace; row < 0 counts from the end. Returns the row."""
    col = tr.column(comp, BREAKS[comp])
    row %= col.size
    col[row] = (int(col[row]) + 2) % relation_model.P
    set_column(hooks_pkg, tr, comp, BREAKS[comp], col)
    return row


def rejection_of(p, tr, lmr=LMR):
    """The TraceRejected a proof of `tr` raises under the preflight (the context's switch is restored)."""
    tr.ctx.set_preflight(True)
    try:
        with pytest.raises(p.TraceRejected) as ei:
            tr.prove(lmr)
    finally:
        tr.ctx.set_preflight(False)
    return ei.value


def assert_rejection(p, air_check, tr, err):
    """err (a TraceRejected of a proof over tr's tables) against bfhip_trace_check and bfhip_trace_relations on the same tables, the CPU oracle,
    the Counter model, and the Python formatters. Returns (CheckResult, RelationResult) of the unbatched calls."""
    chk = tr.check()
    got = err.check
    for line in str(err).split("\n"):
        print(line)
    print("preflight", [(r["name"], r["n_bad_cells"], r["first_bad_cell"], r["first_bad_constraint"]) for r in got if r["n_bad_cells"]], got.logup_total)
    print("unbatched", [(r["name"], r["n_bad_cells"], r["first_bad_cell"], r["first_bad_constraint"]) for r in chk if r["n_bad_cells"]], chk.logup_total)
    assert got.ran and got.rejected and not got.ok
    assert list(got) == list(chk) and got.logup_total == chk.logup_total and got.n_bad_components == chk.n_bad_components      # field by field
    want, total = shim_reports_of_trace(p, air_check, tr, p.default_check_lookup())
    assert all(same_report(g, w) for g, w in zip(got, want)), [(g, w) for g, w in zip(got, want) if not same_report(g, w)]
    assert got.logup_total == total and got.n_bad_components == sum(1 for w in want if w["n_bad_cells"])
    rel = None
    if any(total):
        rel = tr.relations(max_entries=4)
        assert err.relations.reports == rel.reports and err.relations.entries == rel.entries
        assert_same(err.relations, relation_model.relations(trace_tables(tr)), cap=4)
        assert not rel.balanced, "a non-zero logUp total without an unbalanced tuple"
    else:
        assert err.relations.entries == [] and all(r["n_entries"] == 0 and r["n_reported"] == 0 for r in err.relations.reports)
    lines = str(err).split("\n")
    assert lines == p.format_preflight_lines(got, err.relations)
    assert lines[1:] == chk.failures() + (rel.lines() if rel else [])
    head = []
    if chk.n_bad_components:
        head.append("%d of 13 components violate their constraints" % chk.n_bad_components)
    if any(total):
        head.append("the logUp total is not zero")
    assert lines[0] == "TraceRejected: " + " and ".join(head)
    assert p.format_preflight(tr.ctx.last_preflight_report()) == str(err)
    return chk, rel


# ---- a valid trace ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["prove_brainfuck", "prove_registers", "trace_prove"])
def test_valid_trace_is_proved_to_the_same_bytes(pkg, oracle, pctx, air_check, wanted, entry):
    rows, words = machine(pkg)
    tr = pkg.Trace(pctx, *PROG)
    run = {"prove_brainfuck": lambda: pkg.prove_brainfuck(*PROG, ctx=pctx, log_max_rows=LMR),
           "prove_registers": lambda: pkg.prove_registers(rows, words, ctx=pctx, log_max_rows=LMR),
           "trace_prove": lambda: tr.prove(LMR)[0]}[entry]
    try:
        assert not pctx.preflight()
        off = run()
        assert not pctx.last_proof_flags()["preflight"]
        mem_off = pctx.memory()
        pctx.set_preflight(True)
        assert pctx.preflight()
        on = run()
        flags = pctx.last_proof_flags()
        mem_on = pctx.memory()
        print(entry, "arena peak off/on", mem_off["arena_peak"], mem_on["arena_peak"], flags)
        assert on == off == want_proof(oracle, wanted)
        assert flags["preflight"]
        got, rel = pctx.last_preflight()
        print("preflight seconds", got.seconds)
        assert got.ran and not got.rejected and got.ok and got.n_bad_components == 0 and got.logup_total == (0, 0, 0, 0) and got.seconds > 0
        assert rel.entries == [] and rel.balanced
        assert pkg.format_preflight(pctx.last_preflight_report()) == "preflight: ok"
        pctx.set_preflight(False)
        chk = tr.check()
        assert list(got) == list(chk) and got.logup_total == chk.logup_total and chk.ok      # the 13 reports, field by field
        want, total = shim_reports_of_trace(pkg, air_check, tr, pkg.default_check_lookup())
        assert total == (0, 0, 0, 0) and all(same_report(g, w) for g, w in zip(got, want))
        assert run() == off and not pctx.last_proof_flags()["preflight"]
    finally:
        pctx.set_preflight(False)
        tr.close()


# ---- row-local corruption ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("register,entry", [(5, "prove_registers"), (4, "trace_prove"), (5, "prove_brainfuck_then_registers")], ids=["mv", "mp", "mv_after_program"])
def test_one_altered_register_is_rejected_with_row_and_constraint(pkg, oracle, pctx, air_check, wanted, register, entry):
    rows, words = machine(pkg)
    bad = rows.copy()
    bad[1, register] = (int(bad[1, register]) + 4) % relation_model.P
    tr = pkg.Trace.from_registers(pctx, bad, words)
    pctx.set_preflight(True)
    try:
        if entry == "prove_brainfuck_then_registers":
            assert pkg.prove_brainfuck(*PROG, ctx=pctx, log_max_rows=LMR) == want_proof(oracle, wanted)
        with pytest.raises(pkg.TraceRejected) as ei:
            if entry == "trace_prove":
                tr.prove(LMR)
            else:
                pkg.prove_registers(bad, words, ctx=pctx, log_max_rows=LMR)
        err = ei.value
        assert isinstance(err, pkg.BfhipError) and pkg.lib().bfhip_last_error().decode() == str(err)
        pctx.set_preflight(False)
        chk, _ = assert_rejection(pkg, air_check, tr, err)
        assert chk.n_bad_components >= 1
        # the same context then proves a valid trace to the expected bytes, with the preflight on
        pctx.set_preflight(True)
        assert pkg.prove_registers(rows, words, ctx=pctx, log_max_rows=LMR) == want_proof(oracle, wanted)
        assert pctx.last_proof_flags()["preflight"] and pctx.last_preflight()[0].ok
    finally:
        pctx.set_preflight(False)
        tr.close()


@pytest.mark.parametrize("v", V["air_negative"], ids=lambda v: v["cite"].split("(")[1].split(":")[0].split(")")[0])
def test_negative_cases_of_the_reference(hooks_pkg, oracle, hctx, air_check, wanted, v):
    """memory/component.rs:211-609 as tests/test_gpu_trace_check.py builds them — the Memory table of the case's registers with its cells
    patched — as the Memory component of a resident trace. A one-row case is a trace of its own; the two-row cases carry ci = 0 in both
    rows (no trace: InvalidEndOfExecution), so their table replaces the two-row Memory table of the program "+"."""
    want_rows = oracle_air_check.table_from_registers(oracle, v["trace"], [43], 0)
    for r, c, val in v["patch"]:
        want_rows[r, c] = val
    tr = hooks_pkg.Trace.from_registers(hctx, v["trace"], [43]) if len(v["trace"]) == 1 else hooks_pkg.Trace(hctx, "+")
    try:
        assert tr.log_sizes[0] == 4 + int(np.log2(want_rows.shape[0]))
        for c in range(N_MAIN[0]):
            set_column(hooks_pkg, tr, 0, c, want_rows[:, c])
        assert np.array_equal(np.stack([tr.column(0, j) for j in range(N_MAIN[0])]), want_rows.T)
        err = rejection_of(hooks_pkg, tr)
        chk, _ = assert_rejection(hooks_pkg, air_check, tr, err)
        memory = chk[0]
        assert memory["first_bad_row"] == v["table_row"] and memory["first_bad_constraint"] == v["constraint"] and memory["first_bad_value"] == [v["value"], 0, 0, 0]
        good = hooks_pkg.Trace(hctx, *PROG)
        try:
            hctx.set_preflight(True)
            assert good.prove(LMR)[0] == want_proof(oracle, wanted)
        finally:
            hctx.set_preflight(False)
            good.close()
    finally:
        tr.close()


# ---- batch-kernel edges ------------------------------------------------------------------------------------------------------------------------
def test_last_cell_of_one_component_and_first_cell_of_the_next(hooks_pkg, hctx, air_check):
    """Batch order = component order: the last table row of Memory (its last cell ends Memory's last workgroup) and row 0 of Instruction
    (cell 0 of the next workgroup of the same launch)."""
    tr = hooks_pkg.Trace(hctx, *PROG)
    try:
        last = break_row(hooks_pkg, tr, 0, -1)
        break_row(hooks_pkg, tr, 1, 0)
        chk, _ = assert_rejection(hooks_pkg, air_check, tr, rejection_of(hooks_pkg, tr))
        n = 1 << tr.log_sizes[0]
        assert last == n // 16 - 1 and chk[0]["first_bad_cell"] == n - 16 and chk[0]["n_bad_cells"] == 16      # cells n - 16 .. n - 1
        assert chk[1]["first_bad_cell"] == 0 and chk[1]["n_bad_cells"] == 16
        assert [r["n_bad_cells"] != 0 for r in chk] == [True, True] + [False] * 11
    finally:
        tr.close()


def test_violations_in_a_16_cell_component_only(hooks_pkg, hctx, air_check):
    tr = hooks_pkg.Trace(hctx, *PROG)
    try:
        assert tr.log_sizes[6] == 4 and tr.log_sizes[9] == 5
        break_row(hooks_pkg, tr, 6, 0)
        chk, _ = assert_rejection(hooks_pkg, air_check, tr, rejection_of(hooks_pkg, tr))
        assert [k for k in range(13) if chk[k]["n_bad_cells"]] == [6] and chk[6]["n_bad_cells"] == 16 and chk[6]["first_bad_cell"] == 0
    finally:
        tr.close()


def test_violations_in_all_13_components_at_once(hooks_pkg, hctx, air_check):
    tr = hooks_pkg.Trace(hctx, *PROG)
    try:
        rows = [break_row(hooks_pkg, tr, k, -1 if k % 2 else 0) for k in range(13)]
        err = rejection_of(hooks_pkg, tr)
        chk, _ = assert_rejection(hooks_pkg, air_check, tr, err)
        assert chk.n_bad_components == 13 and [r["first_bad_row"] for r in chk] == rows
        assert str(err).startswith("TraceRejected: 13 of 13 components violate their constraints")
    finally:
        tr.close()


def test_first_bad_cell_in_the_last_workgroup_of_a_2_16_cell_component(hooks_pkg, hctx, air_check):
    tr = hooks_pkg.Trace(hctx, *BIG)
    try:
        assert tr.log_sizes[10] == 16
        row = break_row(hooks_pkg, tr, 10, -1)
        chk, _ = assert_rejection(hooks_pkg, air_check, tr, rejection_of(hooks_pkg, tr, BIG_LMR))
        assert row == 4095 and chk[10]["first_bad_cell"] == 65520 and chk[10]["first_bad_cell"] // 256 == 255 and chk[10]["n_bad_cells"] == 16
        assert [k for k in range(13) if chk[k]["n_bad_cells"]] == [10]
    finally:
        tr.close()


# ---- lookups that do not balance ---------------------------------------------------------------------------------------------------------------
def test_unknown_opcode_is_rejected_on_the_total(pkg, oracle, pctx, air_check, wanted):
    """opcode 35 in the register rows and the program. All 13 AIRs hold; the Processor relation keeps one tuple."""
    from test_relations_cpu import unknown_opcode_registers
    regs, words = unknown_opcode_registers(oracle)
    tr = pkg.Trace.from_registers(pctx, regs, words)
    pctx.set_preflight(True)
    try:
        with pytest.raises(pkg.TraceRejected) as ei:
            pkg.prove_registers(regs, words, ctx=pctx, log_max_rows=LMR)
        pctx.set_preflight(False)
        err = ei.value
        chk, rel = assert_rejection(pkg, air_check, tr, err)
        assert chk.n_bad_components == 0 and any(chk.logup_total)
        full = tr.relations(max_entries=4)
        assert err.relations.entries == full.entries == [{"relation": 2, "name": "processor", "tuple": UNKNOWN_TUPLE, "net": 1, "n_yield": 1, "n_use": 0,
                                                          "n_other": 0, "first_yield": (3, 1), "first_use": None}]
        lines = str(err).split("\n")
        assert lines[0] == "TraceRejected: the logUp total is not zero" and len(lines) == 3
        assert lines[-1] == "processor relation: (1, 1, 35, 43, 0, 1, 1) net +1: yielded 1x (first: processor row 1), used 0x"
        pctx.set_preflight(True)
        assert pkg.prove_brainfuck(*PROG, ctx=pctx, log_max_rows=LMR) == want_proof(oracle, wanted)
    finally:
        pctx.set_preflight(False)
        tr.close()


# ---- the pool ----------------------------------------------------------------------------------------------------------------------------------
def expected_text(pkg, ctx, rows, words):
    tr = pkg.Trace.from_registers(ctx, rows, words)
    try:
        chk = tr.check()
        chk.ran, chk.rejected = True, True
        rel = tr.relations(max_entries=4) if any(chk.logup_total) else None
        return "\n".join(pkg.format_preflight_lines(chk, rel))
    finally:
        tr.close()


@pytest.mark.parametrize("k", [1, 2, 3])
def test_pool_queue_and_batch_mix_valid_and_rejected_jobs(pkg, oracle, pctx, wanted, k):
    from test_relations_cpu import unknown_opcode_registers
    rows, words = machine(pkg)
    bad_mv = rows.copy(); bad_mv[1, 5] = 5
    bad_op, bad_op_words = unknown_opcode_registers(oracle)
    jobs = [(rows, words), (bad_mv, words), (rows, words), (bad_op, bad_op_words), (bad_mv, words), (rows, words)]
    texts = [None, expected_text(pkg, pctx, bad_mv, words), None, expected_text(pkg, pctx, bad_op, bad_op_words)]
    texts += [texts[1], None]
    want = want_proof(oracle, wanted)
    pool = pkg.Pool(0, n_in_flight=k, max_log_domain=LMR + 2)
    traces = []
    try:
        # preflight off: the pool behaves as before (status -1, the proof's own text)
        t = pool.submit_registers(bad_mv, words, log_max_rows=LMR, tag=7)
        r = pool.wait(120.0)
        assert r.ticket == t == 1 and r.status == -1 and not r.rejected and r.error == "job 1: ConstraintsNotSatisfied" and r.flags == 0
        pool.set_preflight(True)
        tickets = [pool.submit_registers(a, b, log_max_rows=LMR, tag=i) for i, (a, b) in enumerate(jobs)]
        assert tickets == list(range(2, 2 + len(jobs)))
        with pytest.raises(pkg.BfhipError, match="jobs outstanding"):
            pool.set_preflight(False)                                   # refused while anything is queued, running or not yet taken
        results = [pool.wait(120.0) for _ in jobs]
        assert pool.wait(0) is None and sorted(r.ticket for r in results) == tickets
        for r in results:
            i = r.tag
            assert r.ticket == tickets[i] and r.worker < k
            if texts[i] is None:
                assert r.ok and not r.rejected and r.proof == want and r.error is None and r.preflight and r.flags & 64
            else:
                print(r.error)
                assert r.status == pkg.TRACE_REJECTED == -3 and r.rejected and not r.ok and r.proof is None and r.flags == 0
                assert r.error == "job %d: %s" % (r.ticket, texts[i])
        # batch calls: statuses likewise
        own = pool.ctx(0)
        traces = [pkg.Trace.from_registers(own, a, b) for a, b in jobs[:4]]
        with pytest.raises(pkg.BfhipError) as ei:
            pool.prove_batch(traces, log_max_rows=LMR)
        assert ei.value.info["statuses"] == [0, -3, 0, -3] and ei.value.proofs == [want, None, want, None]
        assert str(ei.value) == "proof 1 of the batch: " + texts[1]
        proofs, info = pool.prove_batch([traces[0], traces[2]], log_max_rows=LMR)
        assert proofs == [want, want] and info["statuses"] == [0, 0]
        pool.set_preflight(False)
        with pytest.raises(pkg.BfhipError, match="ConstraintsNotSatisfied") as ei:
            pool.prove_batch(traces[:2], log_max_rows=LMR)
        assert ei.value.info["statuses"] == [0, -1]
    finally:
        for t in traces:
            t.close()
        pool.close()


# ---- shard groups ------------------------------------------------------------------------------------------------------------------------------
def test_shard_group_members_are_refused(pkg):
    group = pkg.LocalGroup(2)
    member, other = pkg.Context(0, max_log_domain=12), pkg.Context(0, max_log_domain=12)
    try:
        member.join_local_group(group, 0)
        with pytest.raises(pkg.BfhipError, match=r"shard group.*bfhip_ctx_leave_group first"):
            member.set_preflight(True)
        assert not member.preflight()
        member.set_preflight(False)                                     # switching it off is always allowed
        member.leave_group()
        other.set_preflight(True)
        with pytest.raises(pkg.BfhipError, match=r"preflight on cannot join a shard group \(bfhip_ctx_set_preflight\(ctx, 0\) first\)"):
            other.join_local_group(group, 1)
        assert other.group_info()[1] == 1
        other.set_preflight(False)
    finally:
        member.close(); other.close(); group.close()


# ---- preflight off -----------------------------------------------------------------------------------------------------------------------------
def test_preflight_off_invalid_traces_end_as_before(pkg, oracle, pctx):
    """Observed on the parent commit and unchanged with the switch off (the default): the altered-register trace costs a whole proof and fails
    with BfhipError("ConstraintsNotSatisfied") — status -1, not TraceRejected —; the opcode-35 trace is PROVED (the prover has no
    lookup_sum_valid check) and the verifier rejects that proof with "InvalidLookup: Invalid LogUp sum"."""
    from test_relations_cpu import unknown_opcode_registers
    rows, words = machine(pkg)
    bad = rows.copy(); bad[1, 5] = 5
    assert not pctx.preflight()
    before = pctx.last_preflight()[0].seconds
    with pytest.raises(pkg.BfhipError, match="^ConstraintsNotSatisfied$") as ei:
        pkg.prove_registers(bad, words, ctx=pctx, log_max_rows=LMR)
    assert not isinstance(ei.value, pkg.TraceRejected)
    regs, op_words = unknown_opcode_registers(oracle)
    proof = pkg.prove_registers(regs, op_words, ctx=pctx, log_max_rows=LMR)
    verdict = pkg.verify_brainfuck(proof, LMR)
    print(verdict)
    assert verdict == (False, "InvalidLookup: Invalid LogUp sum")
    assert not pctx.last_proof_flags()["preflight"] and pctx.last_preflight()[0].seconds == before      # the preflight did not run


# ---- tools/bfprove.py prove --preflight --------------------------------------------------------------------------------------------------------
def test_bfprove_prove_preflight(pkg, oracle, pctx, wanted, tmp_path):
    import os
    import subprocess
    import sys
    from conftest import ROOT
    rows, words = machine(pkg)
    bad = rows.copy(); bad[1, 5] = 5
    out = tmp_path / "proof.json"
    tool = [sys.executable, os.path.join(ROOT, "tools", "bfprove.py"), "prove", "--preflight", "--code", PROG[0], "--log-max-rows", str(LMR), "--output", str(out)]
    good = subprocess.run(tool, input=PROG[1], capture_output=True, timeout=300)
    print(good.stdout.decode(), good.stderr.decode())
    assert good.returncode == 0 and out.read_bytes() == want_proof(oracle, wanted)
    out.unlink()
    rejected = subprocess.run(tool + ["--set-register", "1:mv=5"], input=PROG[1], capture_output=True, timeout=300)
    print(rejected.stdout.decode(), rejected.stderr.decode())
    assert rejected.returncode == 1 and not out.exists()
    assert rejected.stdout.decode().strip() == expected_text(pkg, pctx, bad, words)
