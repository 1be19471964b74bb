"""Several proofs in flight on one GPU behind one caller thread: Pool (batches and the submit / wait queue) and the results of its jobs."""
import ctypes

import numpy as np

from ._abi import TRACE_REJECTED, BfhipError, Owned, _check, _last_error, _ptr_array, _take_host_string, abi, struct_fields
from ._abi_gen import BFHIP_JOB_CANCELLED as JOB_CANCELLED, BFHIP_POOL_MAX_OUTSTANDING as POOL_MAX_OUTSTANDING
from .context import Context, Conventions, _default_conventions, _pcs_ref
from .programs import AIR_PROVE_CHECK, CompiledAir


class PoolResult(ctypes.Structure):
    """include/bfhip.h `bfhip_pool_result`: one finished job of a pool's queue (88 bytes)."""
    _fields_ = struct_fields("bfhip_pool_result")


class JobResult:
    """What Pool.wait() returns: ticket, tag, status (0 ok, -1 failed, JOB_CANCELLED, TRACE_REJECTED), worker, flags (Context.last_proof_flags bits of that
    proof), log_max_rows, proof (bytes, None unless ok), error (str, None when ok), seconds_queued, seconds_proving."""

    def __init__(self, r):
        self.ticket, self.tag, self.status, self.worker, self.flags = int(r.ticket), int(r.user_tag), int(r.status), int(r.worker), int(r.flags)
        self.log_max_rows, self.seconds_queued, self.seconds_proving = int(r.log_max_rows), float(r.seconds_queued), float(r.seconds_proving)
        self.proof = _take_host_string(r.proof_json, r.proof_len) if r.proof_json else None
        self.error = _take_host_string(r.error).decode() if r.error else None

    ok = property(lambda self: self.status == 0)
    cancelled = property(lambda self: self.status == JOB_CANCELLED)
    rejected = property(lambda self: self.status == TRACE_REJECTED)      # Pool.set_preflight: bad input, not an internal failure
    preflight = property(lambda self: bool(self.flags & 64))
    shared_preprocessed = property(lambda self: bool(self.flags & 4))

    def __repr__(self):
        return "JobResult(ticket=%d, tag=%d, status=%d, worker=%d, %s)" % (self.ticket, self.tag, self.status, self.worker,
                                                                             "%d proof bytes" % len(self.proof) if self.ok else self.error)


class PoolCompiledAir:
    """Pool.air_compile: one AirProgram compiled on every sub-context of a pool — .kernels[w] is the CompiledAir of sub-context w, the
    one a job that runs on worker w uses. close() closes them all; .shape is the program's."""

    def __init__(self, pool, program):
        self.shape, self.kernels = dict(program.shape), []
        try:
            for w in range(pool.n_in_flight):
                self.kernels.append(CompiledAir(pool.ctx(w), program))
        except Exception:
            self.close()
            raise

    def close(self):
        for k in self.kernels:
            k.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Pool(Owned):
    """bfhip_pool_create: `n_in_flight` sub-contexts on one GPU behind ONE caller thread — prove_batch() hands the library a batch of resident
    traces and returns when all are proved, n_in_flight at a time on the library's own worker threads; submit_trace / submit_program /
    submit_registers / submit_air + wait() / as_completed() use the same workers as a queue (results as they complete; not while a batch runs). The sub-contexts share one twiddle
    tree and (preprocessed=1, default) one preprocessed commitment per batch; 0 = every proof recommits it like the reference
    (mod.rs:495-500), 2 = kept across batches."""
    _destroy = "bfhip_pool_destroy"

    def __init__(self, device_id=0, n_in_flight=2, max_log_domain=24, preprocessed=1):
        self._h = ctypes.c_void_p()
        _check(abi().bfhip_pool_create(device_id, n_in_flight, max_log_domain, ctypes.byref(self._h)))
        self.n_in_flight, self.max_log_domain = n_in_flight, max_log_domain
        self._subs = {}
        self._borrowed = {}                       # ticket -> the arrays / trace the library borrows until that result is taken
        if preprocessed != 1:
            self.set_preprocessed(preprocessed)
        if any(_default_conventions):
            self.set_conventions(*_default_conventions)

    def close(self):
        if self._h:
            for c in self._subs.values():
                c._h = ctypes.c_void_p()          # borrowed handles die with the pool
            super().close()                       # running jobs finish before this returns: the borrowed arrays outlive them
            self._borrowed.clear()

    # -- the queue: submit returns a ticket at once, wait() hands out results in completion order -------------------------------------
    def _submitted(self, rc, ticket, keep):
        _check(rc)
        self._borrowed[ticket.value] = keep
        return ticket.value

    def submit_trace(self, trace, log_max_rows=24, tag=0):
        """bfhip_pool_submit_trace: a resident trace of ANY context on the pool's device. The pool keeps a reference to it until its result is taken."""
        t = ctypes.c_uint64()
        return self._submitted(abi().bfhip_pool_submit_trace(self._h, trace._h, log_max_rows, tag, ctypes.byref(t)), t, trace)

    def submit_program(self, code, input_bytes=b"", log_max_rows=24, tag=0):
        """bfhip_pool_submit_brainfuck: program text and input are copied; VM run, table build and upload happen inside the worker."""
        t = ctypes.c_uint64()
        return self._submitted(abi().bfhip_pool_submit_brainfuck(self._h, code.encode(), bytes(input_bytes), len(input_bytes), log_max_rows, tag, ctypes.byref(t)), t, None)

    def submit_registers(self, rows, code_words, log_max_rows=24, tag=0):
        """bfhip_pool_submit_registers: an executed machine's register rows (n x 7 u32) and program words — what prove_registers takes, as a job.
        The rows are borrowed by the library: the pool holds the array until the result is taken."""
        tr = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 7)
        code = np.ascontiguousarray(code_words, dtype=np.uint32)
        t = ctypes.c_uint64()
        return self._submitted(abi().bfhip_pool_submit_registers(self._h, tr.ctypes.data, tr.shape[0], code.ctypes.data, code.size, log_max_rows, tag, ctypes.byref(t)), t, tr)

    def submit_air(self, statement, tree_cols, channel, kernels=None, check=False, tag=0):
        """bfhip_pool_submit_air: what Context.air_prove takes, as a job; the result's proof is air_prove's bytes. The statement, the table
        of column pointers and the channel's state are copied by the library at submit: `channel` is not advanced and may be reused or
        closed at once. kernels: per component None or the PoolCompiledAir of its program (Pool.air_compile, while nothing is
        outstanding). The pool holds the programs, the kernels and tree_cols until the result is taken; the device columns behind
        tree_cols stay the caller's to keep alive until then."""
        st = statement._c()
        if len(tree_cols) != len(statement.trees) or any(len(cols) != len(tree[0]) for cols, tree in zip(tree_cols, statement.trees)):
            raise ValueError("one device column per column of every caller tree")
        if kernels is not None and len(kernels) != len(statement.components):
            raise ValueError("one kernel (or None) per component")
        per_tree = [_ptr_array(cols) for cols in tree_cols]
        trees = (ctypes.c_void_p * max(1, len(per_tree)))(*[ctypes.cast(a, ctypes.c_void_p) for a in per_tree])
        ks = None
        if kernels is not None:
            ks = (ctypes.c_void_p * (self.n_in_flight * len(kernels)))(*[None if k is None else k.kernels[w]._h for w in range(self.n_in_flight) for k in kernels])
        t = ctypes.c_uint64()
        rc = abi().bfhip_pool_submit_air(self._h, ctypes.byref(st), trees, ks, channel._h, AIR_PROVE_CHECK if check else 0, tag, ctypes.byref(t))
        keep = ([c[0] for c in statement.components], [c[5] for c in statement.components], list(kernels or ()), tree_cols)
        return self._submitted(rc, t, keep)

    def air_compile(self, program):
        """bfhip_air_compile on every sub-context: a PoolCompiledAir for submit_air's `kernels`. Call it while nothing is outstanding."""
        return PoolCompiledAir(self, program)

    def prove_batch_air(self, jobs, timeout_s=None):
        """Submits every job — (statement, tree_cols, channel) or (statement, tree_cols, channel, kernels[, check]) — and returns the
        JobResults in SUBMIT order once all are done. Needs an empty queue (results of other jobs would be taken with these)."""
        if any(self.outstanding().values()):
            raise BfhipError("prove_batch_air: jobs outstanding")
        tickets = [self.submit_air(*job[:3], kernels=job[3] if len(job) > 3 else None, check=bool(job[4]) if len(job) > 4 else False, tag=i) for i, job in enumerate(jobs)]
        by_ticket = {r.ticket: r for r in self.as_completed(timeout_s)}
        return [by_ticket[t] for t in tickets]

    def set_scratch_reserve(self, bytes_per_worker):
        """bfhip_pool_set_scratch_reserve: Context.set_scratch_reserve on every sub-context; refused while jobs are outstanding."""
        _check(abi().bfhip_pool_set_scratch_reserve(self._h, int(bytes_per_worker)))

    def wait(self, timeout_s=None):
        """bfhip_pool_wait: the next finished job as a JobResult; None when nothing is outstanding; TimeoutError when timeout_s (None = no limit,
        0 = poll) ran out with jobs outstanding."""
        ms = 0xFFFFFFFF if timeout_s is None else min(0xFFFFFFFE, max(0, int(round(timeout_s * 1000))))
        r = PoolResult()
        rc = abi().bfhip_pool_wait(self._h, ms, ctypes.byref(r))
        if rc == 0:
            self._borrowed.pop(int(r.ticket), None)
            return JobResult(r)
        if rc == 1:
            raise TimeoutError("no job of the pool finished within %s s" % timeout_s)
        if rc == 2:
            return None
        raise _last_error()

    def as_completed(self, timeout_s=None):
        """Yields JobResults in completion order until nothing is outstanding (jobs submitted meanwhile included); timeout_s is per result."""
        while True:
            r = self.wait(timeout_s)
            if r is None:
                return
            yield r

    def outstanding(self):
        """bfhip_pool_outstanding: {queued, running, finished} — finished = done and not yet taken by wait()."""
        q, r, f = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(abi().bfhip_pool_outstanding(self._h, ctypes.byref(q), ctypes.byref(r), ctypes.byref(f)))
        return {"queued": q.value, "running": r.value, "finished": f.value}

    def cancel(self, ticket):
        """bfhip_pool_cancel: True = the job was still queued (its result arrives with status JOB_CANCELLED), False = already running or finished."""
        rc = abi().bfhip_pool_cancel(self._h, ticket)
        if rc < 0:
            raise _last_error()
        return rc == 0

    def ctx(self, i=0):
        """Sub-context i as a (borrowed) Context: for Trace(...) on the pool's device between batches, per-context settings, memory()."""
        if i not in self._subs:
            h = ctypes.c_void_p()
            _check(abi().bfhip_pool_ctx(self._h, i, ctypes.byref(h)))
            c = Context.__new__(Context)
            c._h, c.max_log_domain = h, self.max_log_domain
            c.close = lambda: None                # owned by the pool
            self._subs[i] = c
        return self._subs[i]

    def set_conventions(self, merkle_node_hash=0, mix_u64=0, logup_mask_order=0, merkle_channel=0):
        cv = Conventions(merkle_node_hash, mix_u64, logup_mask_order, merkle_channel)
        _check(abi().bfhip_pool_set_conventions(self._h, ctypes.byref(cv)))

    def set_preprocessed(self, mode):
        _check(abi().bfhip_pool_set_preprocessed(self._h, int(mode)))

    def set_preflight(self, on=True):
        """bfhip_pool_set_preflight: Context.set_preflight on every sub-context. A job whose trace is rejected comes back with
        status TRACE_REJECTED (JobResult.rejected) and the rejection lines as its error; refused while jobs are outstanding."""
        _check(abi().bfhip_pool_set_preflight(self._h, 1 if on else 0))

    def set_pcs_config(self, pcs_config=None):
        """bfhip_pool_set_pcs_config: the PcsConfig of every sub-context and of the shared preprocessed tree's builder (None = the default)."""
        _check(abi().bfhip_pool_set_pcs_config(self._h, _pcs_ref(pcs_config)))

    def _outputs(self, n, want_json):
        js = (ctypes.c_void_p * n)() if want_json else None
        return js, (ctypes.c_size_t * n)(), (ctypes.c_int32 * n)(), (ctypes.c_double * (n + 1))()

    def _collect(self, rc, n, js, lens, st, sec, want_json):
        proofs = [_take_host_string(js[i], lens[i]) if want_json and js[i] else None for i in range(n)]
        info = {"statuses": [int(v) for v in st], "seconds": [float(v) for v in sec[:n]], "batch_seconds": float(sec[n])}
        if rc != 0:
            err = _last_error()
            err.proofs, err.info = proofs, info
            raise err
        return proofs, info

    def prove_batch(self, traces, log_max_rows=24, want_json=True):
        """bfhip_prove_batch: returns (proofs, info) — proofs[i] = JSON bytes of traces[i]'s proof; info = per-proof seconds + batch_seconds.
        Raises BfhipError when a proof failed (its .proofs / .info hold what the rest of the batch produced)."""
        n = len(traces)
        arr = (ctypes.c_void_p * max(n, 1))(*[t._h for t in traces])
        js, lens, st, sec = self._outputs(n, want_json)
        rc = abi().bfhip_prove_batch(self._h, arr, n, log_max_rows, js, lens, st, sec)
        return self._collect(rc, n, js, lens, st, sec, want_json)

    def prove_batch_brainfuck(self, programs, log_max_rows=24, want_json=True):
        """bfhip_prove_batch_brainfuck: programs = [(code, input_bytes), ...]; VM, table build and upload run inside the workers."""
        n = len(programs)
        codes = (ctypes.c_char_p * max(n, 1))(*[c.encode() for c, _ in programs])
        bufs = [ctypes.create_string_buffer(bytes(i), max(len(i), 1)) for _, i in programs]
        inputs = (ctypes.c_void_p * max(n, 1))(*[ctypes.addressof(b) for b in bufs])
        nin = (ctypes.c_size_t * max(n, 1))(*[len(i) for _, i in programs])
        js, lens, st, sec = self._outputs(n, want_json)
        rc = abi().bfhip_prove_batch_brainfuck(self._h, codes, inputs, nin, n, log_max_rows, js, lens, st, sec)
        return self._collect(rc, n, js, lens, st, sec, want_json)
