"""-m gpu: the pool as a queue (include/bfhip.h bfhip_pool_submit_* / bfhip_pool_wait / bfhip_pool_cancel; csrc/pool.hip). Jobs of all three
kinds — resident traces, program texts, register rows of executed machines — start in ticket order on whichever worker is free and come
back in completion order, each exactly once and each the bytes the CPU oracle produces for that program; a failing job is its own result
and nothing else's; cancel, destroy and the exclusion between batch calls and the queue behave as the header says.
Every wait has a finite timeout, so a lost wake-up fails a test instead of hanging it."""
import ctypes
import threading
import time

import numpy as np
import pytest

from test_gpu_pool import MIXED

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

LO, HI = 14, 17                    # two values of LOG_MAX_ROWS interleaved in one stream
SMALL = [0, 1, 3, 5, 6, 7]         # MIXED programs whose largest component fits 2^14 domain rows; 2 and 4 need 2^15
WAIT_S = 120.0


@pytest.fixture(scope="module")
def wanted():
    return {}


def want_proof(oracle, wanted, which, lmr):
    if (which, lmr) not in wanted:
        wanted[(which, lmr)] = oracle.prove(*MIXED[which], log_max_rows=lmr)[0]
    return wanted[(which, lmr)]


@pytest.fixture(scope="module")
def machines(pkg):
    """MIXED as executed machines: (register rows, program words) per program, what prove_brainfuck(&Machine) reads."""
    return [(pkg.host_run(code, inp)[1], pkg.host_compile(code)) for code, inp in MIXED]


def tag_of(which, lmr):
    return which * 100 + lmr


def drain(pool, n):
    """Takes n results; every ticket exactly once."""
    got = [pool.wait(WAIT_S) for _ in range(n)]
    assert all(r is not None for r in got)
    assert len({r.ticket for r in got}) == n
    return got


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_mixed_stream_of_all_job_kinds(pkg, oracle, conv, wanted, machines, k, mode):
    # runs of equal LOG_MAX_ROWS, the two values interleaved; every program of MIXED appears, the three job kinds take turns
    stream = [(0, LO), (1, LO), (2, HI), (4, HI), (3, LO), (7, HI), (5, LO), (6, LO), (0, HI), (2, HI), (7, LO), (1, HI), (4, HI), (3, HI)]
    pool = pkg.Pool(0, n_in_flight=k, max_log_domain=HI + 2, preprocessed=mode)
    own = pkg.Context(0, max_log_domain=HI + 2)
    traces = {}
    try:
        for which in {w for i, (w, _) in enumerate(stream) if i % 3 == 0}:
            traces[which] = pkg.Trace(own, *MIXED[which])
        tickets = []
        for i, (which, lmr) in enumerate(stream):
            if i % 3 == 0:
                tickets.append(pool.submit_trace(traces[which], lmr, tag=tag_of(which, lmr)))
            elif i % 3 == 1:
                tickets.append(pool.submit_program(*MIXED[which], log_max_rows=lmr, tag=tag_of(which, lmr)))
            else:
                tickets.append(pool.submit_registers(*machines[which], log_max_rows=lmr, tag=tag_of(which, lmr)))
        assert tickets == list(range(1, len(stream) + 1))
        results = drain(pool, len(stream))
        assert pool.wait(0) is None and pool.outstanding() == {"queued": 0, "running": 0, "finished": 0}
        assert sorted(r.ticket for r in results) == tickets
        if k == 1:
            assert [r.ticket for r in results] == tickets
        for r in results:
            which, lmr = stream[r.ticket - 1]
            assert r.tag == tag_of(which, lmr) and r.log_max_rows == lmr and r.worker < k
            assert r.status == 0 and r.error is None, r
            assert r.proof == want_proof(oracle, wanted, which, lmr), f"ticket {r.ticket} (program {which}, LOG_MAX_ROWS {lmr}) differs from the oracle (k={k}, mode {mode})"
            assert r.seconds_queued >= 0 and r.seconds_proving > 0
            first_of_run = r.ticket == 1 or stream[r.ticket - 2][1] != lmr
            if mode == 0:
                assert not r.shared_preprocessed, r
            elif not first_of_run:
                assert r.shared_preprocessed, f"ticket {r.ticket} (k={k}, mode {mode}) committed its own preprocessed tree"
        assert pkg.verify_brainfuck(results[0].proof, results[0].log_max_rows) == (True, "")
    finally:
        pool.close()
        for t in traces.values():
            t.close()
        own.close()


def test_producer_thread_and_consumer_thread(pkg, oracle, conv, wanted, machines):
    n_jobs, k = 24, 3
    pool = pkg.Pool(0, n_in_flight=k, max_log_domain=LO + 2)
    submitted, errors = [0], []

    def producer():
        try:
            for i in range(n_jobs):
                assert pool.submit_registers(*machines[SMALL[i % len(SMALL)]], log_max_rows=LO, tag=i) == i + 1
                submitted[0] = i + 1
        except Exception as e:          # noqa: BLE001 — reported by the main thread
            errors.append(e)

    th = threading.Thread(target=producer)
    try:
        th.start()
        taken, deadline = [], time.monotonic() + WAIT_S
        while len(taken) < n_jobs and not errors:
            assert time.monotonic() < deadline, f"only {len(taken)} of {n_jobs} results arrived"
            seen = submitted[0]
            try:
                r = pool.wait(WAIT_S) if seen > len(taken) else pool.wait(0)      # a job is known to be outstanding: wait for it; else poll
            except TimeoutError:
                assert seen <= len(taken)           # the poll found jobs outstanding and none finished
                continue
            if r is None:
                # nothing outstanding: every ticket issued before the call had been taken (this thread is the only consumer)
                assert len(taken) >= seen, (len(taken), seen)
                continue
            taken.append(r)
            o = pool.outstanding()
            assert o["running"] <= k and sum(o.values()) <= n_jobs - len(taken), (o, len(taken))
        th.join(WAIT_S)
        assert not th.is_alive() and not errors, errors
        assert sorted(r.ticket for r in taken) == list(range(1, n_jobs + 1))
        for r in taken:
            assert r.tag == r.ticket - 1 and r.proof == want_proof(oracle, wanted, SMALL[r.tag % len(SMALL)], LO), r
        assert pool.wait(0) is None and sum(pool.outstanding().values()) == 0
    finally:
        th.join(WAIT_S)
        pool.close()


def test_failing_jobs_in_the_middle_of_a_stream(pkg, oracle, conv, wanted, machines):
    rows0, words0 = machines[0]
    no_end = np.ascontiguousarray(rows0[:-1])                   # the executed machine without its final ci = 0 row
    bad = rows0.copy(); bad[3, 5] = (1 << 31) - 1               # a register that is not a canonical M31
    pool = pkg.Pool(0, n_in_flight=2, max_log_domain=HI + 2)
    try:
        t = [pool.submit_registers(*machines[1], log_max_rows=LO, tag=1),
             pool.submit_program(*MIXED[2], log_max_rows=LO, tag=2),            # 2^15 rows under LOG_MAX_ROWS 14
             pool.submit_program(*MIXED[3], log_max_rows=LO, tag=3),
             pool.submit_registers(no_end, words0, log_max_rows=LO, tag=4),
             pool.submit_registers(*machines[5], log_max_rows=LO, tag=5),
             pool.submit_registers(bad, words0, log_max_rows=LO, tag=6),
             pool.submit_program(",", b"", log_max_rows=LO, tag=7),             # reads input it was not given (machine.rs:163-169)
             pool.submit_registers(*machines[7], log_max_rows=LO, tag=8)]
        by_tag = {r.tag: r for r in drain(pool, len(t))}
        for tag, text in ((2, "LOG_MAX_ROWS"), (4, "InvalidEndOfExecution"), (6, r"register value is not a canonical M31 (row 3, register 5)"), (7, "input exhausted")):
            r = by_tag[tag]
            assert r.status == -1 and r.proof is None and r.error.startswith("job %d: " % r.ticket) and text in r.error, r
        for tag, which in ((1, 1), (3, 3), (5, 5), (8, 7)):
            assert by_tag[tag].status == 0 and by_tag[tag].proof == want_proof(oracle, wanted, which, LO), by_tag[tag]
        # the pool proves a further stream as if nothing had happened
        for which in SMALL:
            pool.submit_registers(*machines[which], log_max_rows=LO, tag=which)
        for r in drain(pool, len(SMALL)):
            assert r.status == 0 and r.proof == want_proof(oracle, wanted, r.tag, LO), r
        # what needs no GPU fails the submit itself and issues no ticket
        before = pool.submit_registers(*machines[7], log_max_rows=LO)
        with pytest.raises(pkg.BfhipError, match="EmptyTrace"):
            pool.submit_registers(rows0[:0], words0, log_max_rows=LO)
        L, tk = pkg.lib(), ctypes.c_uint64(0)
        assert L.bfhip_pool_submit_registers(pool._h, None, ctypes.c_size_t(5), None, ctypes.c_size_t(1), LO, ctypes.c_uint64(0), ctypes.byref(tk)) == -1
        assert L.bfhip_pool_submit_registers(pool._h, rows0.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(1 << 31), words0.ctypes.data_as(ctypes.c_void_p),
                                             ctypes.c_size_t(words0.size), LO, ctypes.c_uint64(0), ctypes.byref(tk)) == -1
        assert "2^31" in L.bfhip_last_error().decode() and tk.value == 0
        assert L.bfhip_pool_submit_trace(pool._h, None, LO, ctypes.c_uint64(0), ctypes.byref(tk)) == -1
        assert L.bfhip_pool_submit_brainfuck(pool._h, None, None, ctypes.c_size_t(0), LO, ctypes.c_uint64(0), ctypes.byref(tk)) == -1
        assert pool.submit_registers(*machines[7], log_max_rows=LO) == before + 1
        assert [r.status for r in drain(pool, 2)] == [0, 0]
        # a null result pointer returns at once, whatever the timeout
        assert L.bfhip_pool_wait(pool._h, ctypes.c_uint32(0xFFFFFFFF), None) == -1
        with pytest.raises(pkg.BfhipError, match="no such ticket"):
            pool.cancel(before + 2)
        assert pool.cancel(before) is False                   # issued, finished and taken long ago
    finally:
        pool.close()


def test_cancel_a_queued_job(pkg, oracle, conv, wanted, machines):
    """k = 1, five jobs queued, the sixth cancelled right behind its submit. The worker needs five whole proofs to get there, so at least one of
    three attempts must find the job still queued."""
    pool = pkg.Pool(0, n_in_flight=1, max_log_domain=HI + 2)
    cancelled = 0
    try:
        for attempt in range(3):
            for i in range(5):
                pool.submit_registers(*machines[2], log_max_rows=HI, tag=2)
            sixth = pool.submit_registers(*machines[0], log_max_rows=HI, tag=0)
            was_queued = pool.cancel(sixth)
            results = {r.ticket: r for r in drain(pool, 6)}
            r = results[sixth]
            if was_queued:
                cancelled += 1
                assert r.status == pkg.JOB_CANCELLED and r.cancelled and r.proof is None and r.error == "job %d: cancelled" % sixth, r
            else:
                assert r.status == 0 and r.proof == want_proof(oracle, wanted, 0, HI), r
            assert pool.cancel(sixth) is False                # delivered: nothing left to cancel
            for ticket, other in results.items():
                if ticket != sixth:
                    assert other.status == 0 and other.proof == want_proof(oracle, wanted, 2, HI), other
        assert cancelled >= 1, "three cancels right behind their submits all found the job running already"
    finally:
        pool.close()


def test_batch_calls_and_setters_are_refused_while_jobs_are_outstanding(pkg, oracle, conv, wanted, machines):
    pool = pkg.Pool(0, n_in_flight=2, max_log_domain=HI + 2)
    own = pkg.Context(0, max_log_domain=HI + 2)
    trace = pkg.Trace(own, *MIXED[0])
    try:
        for _ in range(4):
            pool.submit_registers(*machines[2], log_max_rows=HI, tag=2)
        for call in (lambda: pool.prove_batch([trace], log_max_rows=LO), lambda: pool.prove_batch_brainfuck([MIXED[0]], log_max_rows=LO),
                     lambda: pool.set_preprocessed(0), lambda: pool.set_conventions(0, 0, 0, 0), lambda: pool.set_pcs_config(None)):
            with pytest.raises(pkg.BfhipError, match="jobs outstanding"):
                call()
        results = drain(pool, 3)
        # finished or not, a result that has not been taken is outstanding
        with pytest.raises(pkg.BfhipError, match="jobs outstanding"):
            pool.set_preprocessed(0)
        results += drain(pool, 1)
        assert all(r.proof == want_proof(oracle, wanted, 2, HI) for r in results)
        # ... and work again afterwards
        pool.set_pcs_config(None); pool.set_conventions(*conv); pool.set_preprocessed(2)
        assert pool.prove_batch([trace], log_max_rows=LO)[0] == [want_proof(oracle, wanted, 0, LO)]
        assert pool.prove_batch_brainfuck([MIXED[1]], log_max_rows=LO)[0] == [want_proof(oracle, wanted, 1, LO)]
        pool.submit_trace(trace, LO, tag=0)
        assert drain(pool, 1)[0].proof == want_proof(oracle, wanted, 0, LO)
    finally:
        pool.close()
        trace.close()
        own.close()


def test_destroy_with_jobs_queued_and_running_frees_everything(pkg, conv, machines):
    # what the runtime allocates once per process at the first launch of a kernel is not the pool's: one proof first
    warm = pkg.Pool(0, n_in_flight=2, max_log_domain=HI + 2)
    warm.submit_registers(*machines[2], log_max_rows=HI)
    assert warm.wait(WAIT_S).status == 0
    warm.close()
    idle = pkg.Pool(0, n_in_flight=2, max_log_domain=HI + 2)
    idle.close()
    free_idle, _ = pkg.device_memory(0)
    pool = pkg.Pool(0, n_in_flight=2, max_log_domain=HI + 2)
    for i in range(10):
        pool.submit_registers(*machines[2 if i % 2 else 4], log_max_rows=HI, tag=i)
    first = pool.wait(WAIT_S)              # something has finished and been taken, something is running, the rest is queued or untaken
    assert first is not None and first.status == 0
    assert sum(pool.outstanding().values()) == 9
    pool.close()                           # queued jobs dropped, running ones finish, untaken results freed
    free_after, _ = pkg.device_memory(0)
    assert free_after >= free_idle, f"destroy with jobs outstanding left {(free_idle - free_after) >> 20} MiB of device memory behind"


def test_a_trace_of_a_caller_owned_context(pkg, oracle, conv, wanted):
    """Traces for submit_trace may come from any context on the pool's device: a trace is plain device memory."""
    own = pkg.Context(0, max_log_domain=HI + 2)
    pool = pkg.Pool(0, n_in_flight=2, max_log_domain=HI + 2)
    traces = []
    try:
        traces = [pkg.Trace(own, *MIXED[w]) for w in (2, 0)] + [pkg.Trace(pool.ctx(1), *MIXED[3])]
        for which, t in zip((2, 0, 3), traces):
            pool.submit_trace(t, HI, tag=which)
        for r in drain(pool, 3):
            assert r.status == 0 and r.proof == want_proof(oracle, wanted, r.tag, HI), r
        # the caller's context is its own: it proves the same trace itself while the pool works on another
        pool.submit_trace(traces[0], HI, tag=2)
        assert traces[1].prove(HI)[0] == want_proof(oracle, wanted, 0, HI)
        assert drain(pool, 1)[0].proof == want_proof(oracle, wanted, 2, HI)
    finally:
        pool.close()
        for t in traces:
            t.close()
        own.close()


def test_more_than_4096_jobs_outstanding_are_refused(pkg, conv, machines):
    pool = pkg.Pool(0, n_in_flight=1, max_log_domain=14)
    try:
        rows, words = machines[7]
        tickets = [pool.submit_registers(rows, words, log_max_rows=12, tag=i) for i in range(pkg.POOL_MAX_OUTSTANDING)]
        with pytest.raises(pkg.BfhipError, match="4096"):
            pool.submit_registers(rows, words, log_max_rows=12)
        for ticket in reversed(tickets):                      # cancelled or proved, a result stays outstanding until it is taken
            pool.cancel(ticket)
        with pytest.raises(pkg.BfhipError, match="4096"):
            pool.submit_registers(rows, words, log_max_rows=12)
        results = drain(pool, len(tickets))
        assert all(r.status in (0, pkg.JOB_CANCELLED) for r in results) and sum(r.cancelled for r in results) > 4000
        assert pool.submit_registers(rows, words, log_max_rows=12) == tickets[-1] + 1
        assert drain(pool, 1)[0].status == 0
    finally:
        pool.close()
