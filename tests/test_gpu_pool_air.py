"""-m gpu: AIR statements as jobs of the pool's queue (include/bfhip.h bfhip_pool_submit_air; csrc/pool.hip) and the scratch reserve
(bfhip_ctx_set_scratch_reserve; csrc/ctx.h DeviceScratch, csrc/scratch_reserve.h). The reference for a job's bytes is always
Context.air_prove on a stand-alone context under the same conventions and PcsConfig, never another pool job; every comparison is between
bytes and integers. Every wait has a finite timeout, so a lost wake-up fails a test instead of hanging it."""
import ctypes

import numpy as np
import pytest

from conftest import P, splitmix_column
from test_gpu_air_prove import B2, STWO, _failure_statement, _is_first, _lookup_statement, _lookup_trace, _mul_program, _shapes
from test_gpu_pcs_session import Dev

pytestmark = pytest.mark.gpu

WAIT_S = 120
MIB = 1 << 20
PREFIXES = (77, (1 << 40) + 5, 3)
CODE, INP, LMR = "+++>,<[>+.<-]", b"\x01", 17


@pytest.fixture(scope="module")
def pool(pkg):
    p = pkg.Pool(0, n_in_flight=3, max_log_domain=14)
    yield p
    p.close()


@pytest.fixture
def plain(_ctx):
    yield _ctx
    _ctx.set_conventions(*STWO)
    _ctx.set_pcs_config(None)


def _channel(pkg, prefix, conv=STWO):
    ch = pkg.Channel(conv)
    ch.mix_u64(prefix)
    return ch


def _reference(pkg, ctx, st, cols, prefix, kernels=None, check=False):
    with _channel(pkg, prefix) as ch:
        return ctx.air_prove(st, cols, ch, kernels=kernels, check=check)


def _drain(pool, n):
    got = [pool.wait(WAIT_S) for _ in range(n)]
    assert all(r is not None for r in got) and pool.wait(0) is None and pool.outstanding() == {"queued": 0, "running": 0, "finished": 0}
    assert len({r.ticket for r in got}) == n, "a result was delivered twice"
    return {r.ticket: r for r in got}


class Lookup6:
    """Nine lookup-AIR traces at log_size 6 on the device, and per PcsConfig the stand-alone proof of each under its channel prefix."""

    def __init__(self, pkg, ctx):
        self.pkg, self.ctx, self.dev = pkg, ctx, Dev(ctx)
        self.st = _lookup_statement(pkg, 6)
        self.cols = [[[self.dev.up(c) for c in np.concatenate([_lookup_trace(6, 500 + 10 * i), _is_first(6)[None]])]] for i in range(9)]
        self.prefix = [PREFIXES[i % 3] for i in range(9)]
        self._refs = {}

    def refs(self, name):
        if name not in self._refs:
            cfg = None if name == "default" else self.pkg.PcsConfig(**B2)
            self.ctx.set_pcs_config(cfg)
            try:
                self._refs[name] = [_reference(self.pkg, self.ctx, self.st, self.cols[i], self.prefix[i]) for i in range(9)]
            finally:
                self.ctx.set_pcs_config(None)
            assert len(set(self._refs[name])) == 9, "nine traces under three prefixes give nine different proofs"
        return self._refs[name]

    def submit(self, pool, i, kernels=None, check=False, tag=None):
        with _channel(self.pkg, self.prefix[i]) as ch:
            return pool.submit_air(self.st, self.cols[i], ch, kernels=kernels, check=check, tag=i if tag is None else tag)


@pytest.fixture(scope="module")
def lookup6(pkg, _ctx):
    data = Lookup6(pkg, _ctx)
    yield data
    data.dev.__exit__(None, None, None)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compiled", [False, True], ids=["interpreted", "compiled"])
@pytest.mark.parametrize("name", ["default", "b2"])
def test_nine_jobs_at_once_equal_the_stand_alone_proofs(pkg, pool, plain, lookup6, name, compiled):
    """Nine jobs with nine traces and three channel prefixes submitted at once: each result is the stand-alone proof of its own trace and
    prefix, the verifier accepts it, results arrive exactly once with their tags. Under the default config and under B2 (the constraint
    domain is evaluated from coefficients), interpreted and with Pool.air_compile kernels: the same bytes."""
    cfg = None if name == "default" else pkg.PcsConfig(**B2)
    want = lookup6.refs(name)
    kernel = pool.air_compile(lookup6.st.components[0][0]) if compiled else None
    pool.set_pcs_config(cfg)
    try:
        tickets = [lookup6.submit(pool, i, kernels=[kernel] if compiled else None) for i in range(9)]
        assert tickets == list(range(tickets[0], tickets[0] + 9))
        results = _drain(pool, 9)
        for i, t in enumerate(tickets):
            r = results[t]
            assert r.ok and r.error is None and r.tag == i and r.worker < 3 and r.log_max_rows == 0 and r.flags == 0, r
            assert len(r.proof) == len(want[i]) and r.proof == want[i], (name, compiled, i)
            with _channel(pkg, lookup6.prefix[i]) as ch:
                assert pkg.air_verify(lookup6.st, r.proof, ch, STWO, cfg) == (True, "")
        # the same through prove_batch_air: results in submit order
        chans = [_channel(pkg, lookup6.prefix[i]) for i in range(9)]
        batch = pool.prove_batch_air([(lookup6.st, lookup6.cols[i], chans[i], [kernel] if compiled else None) for i in range(9)], timeout_s=WAIT_S)
        assert [r.proof for r in batch] == want and [r.tag for r in batch] == list(range(9))
        for ch in chans:
            ch.close()
    finally:
        pool.set_pcs_config(None)
        if kernel:
            kernel.close()


# ---- 2. shape coverage ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blowup", [1, 2])
def test_four_component_statements_over_three_workers(pkg, pool, plain, blowup):
    """The four-component statement of test_shapes_equal_the_hand_made_sequence — log sizes 4 and 9, log_expand 2, an unbound column, a form-1
    tree, two relations — as six jobs (both sizes under three prefixes, interleaved) over three workers."""
    cfg = pkg.PcsConfig(log_blowup_factor=blowup)
    plain.set_pcs_config(cfg)
    pool.set_pcs_config(cfg)
    try:
        with Dev(plain) as dev:
            shapes = {L: _shapes(pkg, plain, dev, L) for L in (4, 9)}
            jobs = [(L, p) for p in PREFIXES for L in (4, 9)]
            want = [_reference(pkg, plain, *shapes[L], p) for L, p in jobs]
            assert len(set(want)) == 6
            tickets = []
            for i, (L, p) in enumerate(jobs):
                with _channel(pkg, p) as ch:
                    tickets.append(pool.submit_air(*shapes[L], ch, tag=100 + i))
            results = _drain(pool, 6)
            for i, t in enumerate(tickets):
                assert results[t].ok and results[t].tag == 100 + i and results[t].proof == want[i], (jobs[i], results[t])
                with _channel(pkg, jobs[i][1]) as ch:
                    assert pkg.air_verify(shapes[jobs[i][0]][0], results[t].proof, ch, STWO, cfg) == (True, "")
    finally:
        pool.set_pcs_config(None)


# ---- 3. mixed kinds ------------------------------------------------------------------------------------------------------------------------
def test_air_jobs_interleaved_with_brainfuck_jobs(pkg, plain, lookup6):
    """submit_program jobs at log_max_rows 17 need a twiddle tree of 2^19, more than the module's pool has: a pool of its own. Every job,
    of either kind, returns its own bytes; an air job's result carries log_max_rows 0 and flags 0."""
    programs = [(CODE, INP), ("++[-]+.", b""), ("+++[>++<-]>.", b"")]
    want_bf = [pkg.prove_brainfuck(code, inp, ctx=plain, log_max_rows=LMR) for code, inp in programs]
    want_air = lookup6.refs("default")
    mixed = pkg.Pool(0, n_in_flight=3, max_log_domain=LMR + 2)
    try:
        tickets = []
        for i in range(6):
            tickets.append(("air", i, lookup6.submit(mixed, i)))
            if i < 3:
                tickets.append(("bf", i, mixed.submit_program(*programs[i], log_max_rows=LMR, tag=50 + i)))
        results = _drain(mixed, 9)
        for kind, i, t in tickets:
            r = results[t]
            assert r.ok, r
            if kind == "air":
                assert r.proof == want_air[i] and r.tag == i and r.log_max_rows == 0 and r.flags == 0
            else:
                assert r.proof == want_bf[i] and r.tag == 50 + i and r.log_max_rows == LMR
    finally:
        mixed.close()


# ---- 4. copied, not borrowed ---------------------------------------------------------------------------------------------------------------
def test_the_statement_and_the_channel_are_copied_at_submit(pkg, pool, plain, lookup6):
    """Behind jobs that keep the workers busy: a job whose statement arrays are overwritten and dropped and whose channel is advanced
    right after the submit, and one whose channel is closed at once. Both return the stand-alone bytes; the caller's channel holds what
    the caller left in it."""
    want = lookup6.refs("default")
    blockers = [lookup6.submit(pool, i) for i in range(6)]
    st = _lookup_statement(pkg, 6)
    ch = _channel(pkg, lookup6.prefix[6])
    victim = pool.submit_air(st, lookup6.cols[6], ch, tag=6)
    raw, keep = st._built
    for obj in keep:
        if isinstance(obj, (ctypes.Array, ctypes.Structure)):
            ctypes.memset(ctypes.addressof(obj), 0xA5, ctypes.sizeof(obj))
    ctypes.memset(ctypes.addressof(raw), 0xA5, ctypes.sizeof(raw))
    st._built = None
    st.trees, st.components = [], []
    del raw, keep
    ch.mix_u64(123456789)
    left = ch.state()
    gone = _channel(pkg, lookup6.prefix[7])
    closed = pool.submit_air(lookup6.st, lookup6.cols[7], gone, tag=7)
    gone.close()
    results = _drain(pool, 8)
    assert results[victim].ok and results[victim].proof == want[6], results[victim]
    assert results[closed].ok and results[closed].proof == want[7], results[closed]
    for i, t in enumerate(blockers):
        assert results[t].proof == want[i]
    assert ch.state() == left
    with _channel(pkg, lookup6.prefix[6]) as fresh:
        fresh.mix_u64(123456789)
        assert fresh.state() == left      # the job did not advance the caller's channel
    ch.close()


# ---- 5. failures by name -------------------------------------------------------------------------------------------------------------------
class _WrongRows:
    """Pool.air_compile's kernels, each row moved to the next worker: whichever worker runs the job finds another context's kernel"""

    def __init__(self, compiled):
        self.kernels = compiled.kernels[1:] + compiled.kernels[:1]


def test_failing_jobs_are_named_and_the_others_return_their_bytes(pkg, pool, plain):
    log_size, n = 6, 64
    st = _failure_statement(pkg, log_size)
    x, y = splitmix_column(5 << 32, n).astype(np.uint64), splitmix_column(6 << 32, n).astype(np.uint64)
    trace = np.concatenate([_lookup_trace(log_size, 51), _is_first(log_size)[None], np.stack([x, y, x * y % np.uint64(P)]).astype(np.uint32)])
    bad = trace.copy()
    bad[6, 3] = (int(bad[6, 3]) + 1) % P
    # a zero denominator: a - a[37] does not depend on the drawn elements (tests/test_gpu_air_prove.py)
    S = pkg.AirStatement
    v = int(trace[0, 37])
    f = pkg.AirBuilder()
    f.frac(1, f.col(0) - f.const(v)); f.end_column()
    b = pkg.AirBuilder()
    cur, prev = b.secure_col(2), b.secure_col(2, -1)
    b.constraint((cur - (prev - b.param(0) * b.col(1))) * b._to_q(b.col(0) - b.const(v)) - b._to_q(b.const(1)))
    zero = S()
    zero.tree([log_size] * 7)
    zero.component(b.program(), log_size, 1, [(0, 0), (0, 3)] + [(S.INTERACTION, j) for j in range(4)], [S.claimed_sum()], fractions=f.logup_program(), fraction_columns=[(0, 0)])
    cell = min(i for i in range(n) if int(trace[0, i]) == v)
    compiled = pool.air_compile(st.components[1][0])
    try:
        with Dev(plain) as dev:
            good_cols, bad_cols = [[dev.up(c) for c in trace]], [[dev.up(c) for c in bad]]
            want = _reference(pkg, plain, st, good_cols, 77)
            report = plain.air_check(_mul_program(pkg), log_size, bad_cols[0][4:7], [])
            line = pkg.format_air_check(report).splitlines()[1]
            assert line.startswith("constraint 0: 1 cells, first at cell 3, value (1, 0, 0, 0)")

            def submit(statement, cols, **kw):
                with _channel(pkg, 77) as ch:
                    return pool.submit_air(statement, cols, ch, **kw)

            order = [("good", submit(st, good_cols)), ("unsatisfied", submit(st, bad_cols)), ("good", submit(st, good_cols)), ("checked", submit(st, bad_cols, check=True)),
                     ("zero", submit(zero, good_cols)), ("good", submit(st, good_cols, kernels=[None, compiled])), ("kernel", submit(st, good_cols, kernels=[None, _WrongRows(compiled)])),
                     ("good", submit(st, good_cols, check=True))]
            results = _drain(pool, len(order))
            messages = {"unsatisfied": "bfhip_air_prove: ConstraintsNotSatisfied", "checked": "bfhip_air_prove: component 1: " + line,
                        "zero": "bfhip_air_prove: bfhip_logup_program_generate_batch: component 0: fraction 0 has a zero denominator at cell %d" % cell,
                        "kernel": "bfhip_air_prove: component 1: the kernel was compiled by another context (a module belongs to the context that loaded it)"}
            for what, t in order:
                r = results[t]
                if what == "good":
                    assert r.ok and r.proof == want, (what, r)
                else:
                    assert r.status == -1 and r.proof is None and r.error == "job %d: %s" % (t, messages[what]), (what, r)
            # the pool proves the good case again, on every worker
            again = [submit(st, good_cols) for _ in range(6)]
            results = _drain(pool, 6)
            assert all(results[t].ok and results[t].proof == want for t in again) and {results[t].worker for t in again} <= {0, 1, 2}

            # ---- submit refusals: no ticket, nothing queued ---------------------------------------------------------------------------------
            last = again[-1]
            st.components[1] = st.components[1][:2] + (4,) + st.components[1][3:]
            st._built = None
            with pytest.raises(pkg.BfhipError) as e:
                submit(st, good_cols)
            assert str(e.value) == "bfhip_pool_submit_air: component 1: log_expand must be 1, 2 or 3, got 4"
            st.components[1] = st.components[1][:2] + (1,) + st.components[1][3:]
            st._built = None
            # log sizes the pool's twiddle tree does not hold: the validator's rule under the POOL's max_log_domain (14) and PcsConfig
            big = _lookup_statement(pkg, 14)
            with pytest.raises(pkg.BfhipError) as e:
                submit(big, [[1, 1, 1, 1]])
            assert str(e.value) == "bfhip_pool_submit_air: tree 0 column 0: log_size 14 outside [4, max_log_domain - log_blowup_factor] = [4, 13]"
            with pkg.Channel((0, 1, 0, 0)) as other:      # another mix_u64 form than the pool's
                with pytest.raises(pkg.BfhipError) as e:
                    pool.submit_air(st, good_cols, other)
            assert str(e.value) == "bfhip_pool_submit_air: the channel was created under other conventions (merkle_channel, mix_u64) than the pool's"
            L, tk = pkg.lib(), ctypes.c_uint64(0)
            with _channel(pkg, 77) as ch:
                assert L.bfhip_pool_submit_air(pool._h, None, None, None, ch._h, 0, ctypes.c_uint64(0), ctypes.byref(tk)) == -1
                assert L.bfhip_last_error().decode() == "bfhip_pool_submit_air: null argument" and tk.value == 0
                assert L.bfhip_pool_submit_air(pool._h, ctypes.byref(st._c()), None, None, ch._h, 0, ctypes.c_uint64(0), None) == -1
            assert pool.outstanding() == {"queued": 0, "running": 0, "finished": 0}
            assert submit(st, good_cols) == last + 1      # no refusal took a ticket
            assert _drain(pool, 1)[last + 1].proof == want

            # ---- while air jobs are outstanding ----------------------------------------------------------------------------------------------
            held = [submit(st, good_cols) for _ in range(3)]
            for call in (lambda: pool.prove_batch([], log_max_rows=10), lambda: pool.set_pcs_config(None), lambda: pool.set_conventions(*STWO), lambda: pool.set_preflight(False),
                         lambda: pool.set_preprocessed(1), lambda: pool.set_scratch_reserve(0)):
                with pytest.raises(pkg.BfhipError, match="jobs outstanding"):
                    call()
            with _channel(pkg, 77) as ch:
                with pytest.raises(pkg.BfhipError) as e:
                    pool.ctx(0).air_prove(st, good_cols, ch)
            assert str(e.value) == "bfhip_air_prove: bfhip_pcs_create: not supported on a pool's sub-context while jobs are outstanding on the pool"
            results = _drain(pool, 3)
            assert all(results[t].proof == want for t in held)
            assert _reference(pkg, pool.ctx(0), st, good_cols, 77) == want      # idle again: the caller may use a sub-context

            # ---- a queued air job can be cancelled: five jobs in front of it on three workers, three attempts ---------------------------------
            cancelled = 0
            for attempt in range(3):
                front = [submit(st, good_cols) for _ in range(8)]
                ninth = submit(st, good_cols, tag=9)
                was_queued = pool.cancel(ninth)
                results = _drain(pool, 9)
                r = results[ninth]
                if was_queued:
                    cancelled += 1
                    assert r.status == pkg.JOB_CANCELLED and r.cancelled and r.proof is None and r.error == "job %d: cancelled" % ninth and r.tag == 9, r
                else:
                    assert r.ok and r.proof == want
                assert all(results[t].proof == want for t in front)
            assert cancelled >= 1, "three cancels right behind their submits all found the job running already"
    finally:
        compiled.close()


# ---- 6. the reserve on a plain context -----------------------------------------------------------------------------------------------------
def test_reserve_on_a_plain_context(pkg):
    log_size = 10
    st = _lookup_statement(pkg, log_size)
    trace = np.concatenate([_lookup_trace(log_size, 51), _is_first(log_size)[None]])
    ctx = pkg.Context(0, max_log_domain=14)
    try:
        with Dev(ctx) as dev:
            cols = [[dev.up(c) for c in trace]]
            assert ctx.scratch_stats() == {"reserve": 0, "high_water": 0, "device_allocations": 0, "served": 0}
            want = _reference(pkg, ctx, st, cols, 77)
            without = ctx.scratch_stats()
            assert without["device_allocations"] >= 1 and without["served"] == 0 and without["reserve"] == 0      # today's behaviour: every request goes to the device
            in_use = ctx.memory()["arena_in_use"]

            ctx.set_scratch_reserve(64 * MIB)
            before = ctx.scratch_stats()
            assert before == {"reserve": 64 * MIB, "high_water": 0, "device_allocations": without["device_allocations"], "served": 0}
            served = 0
            for _ in range(3):
                assert _reference(pkg, ctx, st, cols, 77) == want
                now = ctx.scratch_stats()
                assert now["device_allocations"] == before["device_allocations"], "a proof of a seen shape allocated on the device"
                assert now["served"] > served and 0 < now["high_water"] <= 64 * MIB
                served = now["served"]
            assert served == 3 * without["device_allocations"], "every request the device answered before is now served from the reserve"
            assert ctx.memory()["arena_in_use"] == in_use
            high_water = ctx.scratch_stats()["high_water"]
            print("lookup AIR log_size 10: scratch high-water mark %d bytes, %d requests per proof" % (high_water, without["device_allocations"]))

            # the mark sizes the reserve: exactly that much is enough, one alignment step less is not
            ctx.set_scratch_reserve(high_water)
            assert _reference(pkg, ctx, st, cols, 77) == want
            assert ctx.scratch_stats()["device_allocations"] == before["device_allocations"] and ctx.scratch_stats()["high_water"] == high_water

            # too small: the same bytes through the fallback
            ctx.set_scratch_reserve(4096)
            small = ctx.scratch_stats()
            assert small["reserve"] == 4096 and small["high_water"] == 0
            assert _reference(pkg, ctx, st, cols, 77) == want
            assert ctx.scratch_stats()["device_allocations"] > small["device_allocations"]
            assert ctx.memory()["arena_in_use"] == in_use

            # refused while a session is open; the reserve stays what it was
            with pkg.PcsSession(ctx):
                with pytest.raises(pkg.BfhipError) as e:
                    ctx.set_scratch_reserve(MIB)
                assert str(e.value) == "bfhip_ctx_set_scratch_reserve: a commitment-scheme session is open on this context (bfhip_pcs_destroy first)"
            assert ctx.scratch_stats()["reserve"] == 4096
            ctx.set_scratch_reserve(0)
            assert ctx.scratch_stats()["reserve"] == 0
            assert _reference(pkg, ctx, st, cols, 77) == want
    finally:
        ctx.close()


# ---- 7. the reserve in the pool ------------------------------------------------------------------------------------------------------------
def test_reserve_in_the_pool(pkg, pool, plain, lookup6):
    """With a reserve on every sub-context: warm-up jobs, then nine more of the same shape during which no sub-context's call-scoped
    memory goes to the device."""
    want = lookup6.refs("default")
    pool.set_scratch_reserve(64 * MIB)
    try:
        assert all(pool.ctx(w).scratch_stats()["reserve"] == 64 * MIB for w in range(3))
        warm = [lookup6.submit(pool, i) for i in range(3)]
        results = _drain(pool, 3)
        assert all(results[t].proof == want[i] for i, t in enumerate(warm))
        before = [pool.ctx(w).scratch_stats() for w in range(3)]
        tickets = [lookup6.submit(pool, i) for i in range(9)]
        results = _drain(pool, 9)
        assert all(results[t].ok and results[t].proof == want[i] for i, t in enumerate(tickets))
        after = [pool.ctx(w).scratch_stats() for w in range(3)]
        for w in range(3):
            assert after[w]["device_allocations"] == before[w]["device_allocations"], (w, before[w], after[w])
            assert after[w]["high_water"] <= 64 * MIB
        assert sum(a["served"] - b["served"] for a, b in zip(after, before)) > 0
        ran = {results[t].worker for t in tickets}
        assert all(after[w]["served"] > before[w]["served"] for w in ran)
    finally:
        pool.set_scratch_reserve(0)
    assert all(pool.ctx(w).scratch_stats()["reserve"] == 0 for w in range(3))
