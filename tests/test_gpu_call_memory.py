"""-m gpu: device memory that lives for one call (csrc/ctx.h: DeviceScratch, ArenaBorrow). Every entry point that borrows the arena gives it
back — after a good call and after a refused one — a proof's preflight does so on the accepted and on the rejected path, and the entry
points that take hipMalloc scratch return the same words call after call without moving the context's memory figures. Context.memory() is
exact bookkeeping of the context; the device's free bytes are not looked at (other processes move them).
The paths between an allocation and its release that only a failing HIP call reaches are not provoked here: they are the two destructors."""
import numpy as np
import pytest

from conftest import P, splitmix_column
from test_gpu_air_compose import Comp, _compose
from test_gpu_logup_batch import Dev, Item
from test_gpu_preflight import LMR, PROG, set_column
from test_gpu_relation_multiplicities import lookup_specs
from test_gpu_relation_program import MULTS, WORDS, drawn, one_entry_program
from test_gpu_relations import DeviceTables, processor_table

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

N_CALLS = 64


def in_use(ctx):
    m = ctx.memory()
    print(m)
    return m["arena_in_use"], m["arena_reserved"]


# ---- the arena borrowers ---------------------------------------------------------------------------------------------------------------------
def test_arena_borrowers_leave_the_arena_as_they_found_it(pkg):
    """A proof leaves its allocations in the arena. Behind it each borrower runs once and is refused once: "in use" stays at the byte,
    "reserved" does not shrink."""
    ctx = pkg.Context(0, max_log_domain=LMR + 2)
    try:
        proof = pkg.prove_brainfuck(*PROG, ctx=ctx, log_max_rows=LMR)
        used, reserved = in_use(ctx)
        after_proof = used
        assert used > 0

        def unchanged(what):
            now_used, now_reserved = in_use(ctx)
            assert now_used == used, what
            assert now_reserved >= reserved, what

        with Dev(ctx) as dev:
            # bfhip_relation_program_summary: two tables of 2^5 and 2^4 rows, one relation of one word
            prog = one_entry_program(pkg, [1], 0)
            tables = [(prog, 5, 0, [dev.up(drawn(1, 32, WORDS)), dev.up(drawn(2, 32, MULTS))]), (prog, 4, 0, [dev.up(drawn(3, 16, WORDS)), dev.up(drawn(4, 16, MULTS))])]
            assert ctx.relation_program_summary(tables).reports[0]["n_entries"] > 0
            unchanged("bfhip_relation_program_summary")
            with pytest.raises(pkg.BfhipError, match="row_shift 7 above log_size 5"):
                ctx.relation_program_summary([(prog, 5, 7, tables[0][3])])
            unchanged("bfhip_relation_program_summary, refused")

            # bfhip_relation_program_multiplicities: a consumer of 2^5 rows looking up a table of 2^4
            specs = lookup_specs(pkg, 4, 5, 1)
            lookup = [(p, log, rs, [dev.up(c) for c in cols]) for p, log, rs, cols, _ in specs]
            out = dev.empty(16)
            assert ctx.relation_program_multiplicities(lookup, 0, 1, 0, out).report["n_rows"] == 16
            unchanged("bfhip_relation_program_multiplicities")
            with pytest.raises(pkg.BfhipError, match="target entry 1"):
                ctx.relation_program_multiplicities(lookup, 0, 1, 1, out)
            unchanged("bfhip_relation_program_multiplicities, refused")

        # bfhip_relation_summary: two Processor tables of 2^4 and 2^5 cells. The built-in summary borrows only inside a proof (the next test);
        # called by itself it starts from an empty arena like a proof and leaves its last relation's scratch there, as it always has
        # (7424 bytes here, after the proof's 8955648): a refusal changes nothing, a second call leaves the same bytes in use.
        built_in = DeviceTables(ctx, [(3, processor_table([(1, 1, 35, 43, 0, 1, 1)])), (3, processor_table([(2, 1, 43, 0, 0, 1, 1)], rows=2))])
        try:
            with pytest.raises(pkg.BfhipError, match="unknown component"):
                ctx.relation_summary([(13, 4, built_in.args[0][2])])
            unchanged("bfhip_relation_summary, refused")
            assert all(r["n_entries"] > 0 for r in built_in.summary().reports)
            used, reserved = in_use(ctx)[0], max(reserved, in_use(ctx)[1])
            assert all(r["n_entries"] > 0 for r in built_in.summary().reports)
            unchanged("bfhip_relation_summary")
            with pytest.raises(pkg.BfhipError, match="unknown component"):
                ctx.relation_summary([(13, 4, built_in.args[0][2])])
            unchanged("bfhip_relation_summary, refused")
        finally:
            built_in.close()
        assert pkg.prove_brainfuck(*PROG, ctx=ctx, log_max_rows=LMR) == proof
        assert in_use(ctx)[0] == after_proof
    finally:
        ctx.close()


# ---- a proof's preflight -----------------------------------------------------------------------------------------------------------------------
def test_preflight_gives_the_arena_back_when_it_accepts_and_when_it_rejects(hooks_pkg):
    """The same program three times as resident traces. `bad` has a Memory value changed: its tuple is used and never yielded, so the logUp
    total is not zero and the relation pass (relations_in_proof) runs inside the rejected proof. `bad_air` has the Processor's mv_inv
    changed, a column of no lookup tuple: rejected on a constraint with a zero total, without the relation pass.
    An accepted proof goes on to allocate its columns and trees, a rejected one stops at the preflight, so "in use" behind the two cannot
    be one number (8908032 and 2359808 bytes here, on the parent commit as well). What the borrow guarantees is compared instead: both
    rejections leave exactly what the proof held when its preflight began, whichever scratch they took, and an accepted proof behind them
    leaves what the first one left, and the same bytes."""
    p = hooks_pkg
    ctx = p.Context(0, max_log_domain=LMR + 2)
    good, bad, bad_air = p.Trace(ctx, *PROG), p.Trace(ctx, *PROG), p.Trace(ctx, *PROG)
    try:
        for tr, comp, column in ((bad, 0, 2), (bad_air, 3, 8)):
            col = tr.column(comp, column)
            col[0] = (int(col[0]) + 2) % P
            set_column(p, tr, comp, column, col)
        assert good.log_sizes == bad.log_sizes == bad_air.log_sizes
        ctx.set_preflight(True)
        first = good.prove(LMR)[0]
        accepted = in_use(ctx)
        with pytest.raises(p.TraceRejected) as ei:
            bad.prove(LMR)
        rejected = in_use(ctx)
        print(str(ei.value))
        assert any(ei.value.check.logup_total) and ei.value.relations.entries      # the relation pass ran
        with pytest.raises(p.TraceRejected) as ei:
            bad_air.prove(LMR)
        rejected_air = in_use(ctx)
        print(str(ei.value))
        assert ei.value.check.n_bad_components == 1 and not any(ei.value.check.logup_total) and ei.value.relations.entries == []
        assert 0 < rejected[0] == rejected_air[0] < accepted[0] and accepted[1] <= rejected[1] <= rejected_air[1]
        assert good.prove(LMR)[0] == first
        assert in_use(ctx)[0] == accepted[0]
    finally:
        ctx.set_preflight(False)
        good.close(); bad.close(); bad_air.close(); ctx.close()


# ---- the users of hipMalloc scratch ------------------------------------------------------------------------------------------------------------
def _logup_generate(pkg, ctx, dev):
    rows = np.stack([splitmix_column(70 + j, 4) for j in range(8)])      # a Memory table of 4 rows: 2^6 cells
    src, dst = [dev.up(r) for r in rows], [dev.empty(64) for _ in range(4)]
    elems = splitmix_column(31, 24)
    elems[elems == 0] = 1
    return lambda: (ctx.logup_generate(0, 6, src, elems.tolist(), dst), [ctx.download(q, 64).tobytes() for q in dst])


def _logup_program_generate(pkg, ctx, dev):
    it = Item(pkg, 6)
    src, dst = [dev.up(c) for c in it.cols], [dev.empty(64) for _ in range(it.n_out)]
    return lambda: (ctx.logup_program_generate(it.program, 6, src, it.params, dst), [ctx.download(q, 64).tobytes() for q in dst])


def _logup_program_generate_batch(pkg, ctx, dev):
    items = [Item(pkg, 5, seed=1), Item(pkg, 6, seed=2)]
    entries = [(it.program, it.log_size, [dev.up(c) for c in it.cols], it.params, [dev.empty(1 << it.log_size) for _ in range(it.n_out)]) for it in items]
    return lambda: (ctx.logup_program_generate_batch(entries), [ctx.download(q, 1 << e[1]).tobytes() for e in entries for q in e[4]])


def _air_compose(pkg, ctx, dev):
    comps = [Comp(pkg, dev, "small", 5, 1, 11), Comp(pkg, dev, "base", 4, 1, 12)]      # buckets of 2^6 and 2^5 rows: the smaller one is scratch
    return lambda: _compose(ctx, dev, [c.entry() for c in comps], [0x1234567, P - 1, 0, 0x7654321], 6).tobytes()


def _eval_at_point(pkg, ctx, dev):
    coeffs, point = dev.up(splitmix_column(5, 64) % np.uint32(P)), (splitmix_column(6, 8) % np.uint32(P)).tolist()
    return lambda: ctx.eval_at_point(coeffs, 6, point)


def _gather(pkg, ctx, dev):
    col = dev.up(splitmix_column(7, 64))
    return lambda: ctx.gather(col, [63, 0, 17, 17, 32]).tobytes()


@pytest.mark.parametrize("user", [_logup_generate, _logup_program_generate, _logup_program_generate_batch, _air_compose, _eval_at_point, _gather],
                         ids=lambda f: f.__name__[1:])
def test_scratch_users_repeat_their_result_and_do_not_move_the_context(_ctx, pkg, user):
    ctx = _ctx
    with Dev(ctx) as dev:
        call = user(pkg, ctx, dev)
        first, memory = call(), ctx.memory()
        print(memory)
        for k in range(1, N_CALLS):
            assert call() == first, k
        assert ctx.memory() == memory
