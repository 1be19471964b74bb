"""Proving and verifying a Brainfuck execution: the one-call entries (program text or register rows in, proof JSON out), the host-only
verifier, compiler and VM, Trace — the prover input resident in HBM — and the composition polynomial a hand-assembled verifier needs."""
import ctypes

import numpy as np

from ._abi import Owned, _check, _check_proof, _last_error, _take_host_string, _u32s, abi
from .context import Context, _conv_ref, _pcs_ref
from .reports import CheckReport, CheckResult, _relation_result

PHASES = ("preprocessed", "tables_host", "main_trace", "interaction", "composition", "oods", "quotients", "fri", "decommit", "total")


def _prove(ctx, own, call, with_transcript, with_timings):
    """What the one-call provers share: call(proof*, length*, transcript* or None, times) on the context, then the proof bytes alone or
    (proof, [transcript dict], [phase seconds]); a context made for the call is closed."""
    try:
        js, n, tr = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_void_p()
        times = (ctypes.c_double * 10)()
        _check_proof(call(ctypes.byref(js), ctypes.byref(n), ctypes.byref(tr) if with_transcript else None, times), ctx)
        out = [_take_host_string(js, n.value)]
        if with_transcript:
            out.append(dict(line.split(":") for line in _take_host_string(tr).decode().strip().split("\n")))
        if with_timings:
            out.append(dict(zip(PHASES, list(times))))
        return out[0] if len(out) == 1 else tuple(out)
    finally:
        if own:
            ctx.close()


def prove_brainfuck(code, input_bytes=b"", ctx=None, log_max_rows=24, with_transcript=False, with_timings=False, pcs_config=None):
    """prove_brainfuck (mod.rs:471): returns the proof as serde_json bytes of BrainfuckProof. GPU only. With ctx.set_preflight() a trace
    that cannot be proved raises TraceRejected (so do prove_registers and Trace.prove).
    pcs_config: a PcsConfig for this proof (None: the context's own, PcsConfig::default() for a new context). A context passed in keeps it
    afterwards."""
    own = ctx is None
    if own:
        blowup = 1 if pcs_config is None else pcs_config.log_blowup_factor
        ctx = Context(0, max_log_domain=log_max_rows + blowup + 1)

    def call(*outputs):
        if pcs_config is not None:
            ctx.set_pcs_config(pcs_config)
        return abi().bfhip_prove_brainfuck(ctx._h, code.encode(), input_bytes, len(input_bytes), log_max_rows, *outputs)
    return _prove(ctx, own, call, with_transcript, with_timings)


def prove_registers(rows, code_words, ctx=None, log_max_rows=24, with_transcript=False, with_timings=False):
    """bfhip_prove_registers — prove_brainfuck(&Machine) (mod.rs:471-473) in one call: an executed machine's register rows (n x 7 u32: clk, ip,
    ci, ni, mp, mv, mvi) and program words in, the proof's serde_json bytes out. Same bytes as Trace.from_registers(...).prove(...); no
    resident trace. A non-canonical register raises with its (row, register)."""
    own = ctx is None
    if own:
        ctx = Context(0, max_log_domain=log_max_rows + 2)

    def call(*outputs):
        tr = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 7)
        code = np.ascontiguousarray(code_words, dtype=np.uint32)
        return abi().bfhip_prove_registers(ctx._h, tr.ctypes.data, tr.shape[0], code.ctypes.data, code.size, log_max_rows, *outputs)
    return _prove(ctx, own, call, with_transcript, with_timings)


def verify_brainfuck(proof_json: bytes, log_max_rows=24, conventions=None, pcs_config=None):
    """verify_brainfuck (mod.rs:738): returns (ok, reason). Host only — no GPU needed, like the reference's verifier.
    conventions: (merkle_node_hash, mix_u64, logup_mask_order) the proof was produced under; None = the defaults.
    pcs_config: the PcsConfig the proof was made with; None = PcsConfig::default(). An invalid config raises BfhipError."""
    err = ctypes.create_string_buffer(512)
    rc = abi().bfhip_verify_brainfuck_pcs(proof_json, len(proof_json), log_max_rows, _conv_ref(conventions), _pcs_ref(pcs_config), err, 512)
    if rc < 0:
        raise _last_error()
    return rc == 0, err.value.decode()


def host_compile(code):
    """bfhip_host_compile (compiler.rs:17-37): the program words, jump targets included. Host only."""
    out = np.zeros(2 * len(code) + 4, dtype=np.uint32)
    n = ctypes.c_size_t()
    _check(abi().bfhip_host_compile(code.encode(), out.ctypes.data, out.size, ctypes.byref(n)))
    return out[: n.value].copy()


def host_run(code, input_bytes=b"", ram_size=0):
    """bfhip_host_run_ram (machine.rs:141-238): (output bytes, register trace as an (n, 7) u32 array: clk, ip, ci, ni, mp, mv, mvi). Host only."""
    n_out, n_rows = ctypes.c_size_t(), ctypes.c_size_t()
    args = (code.encode(), input_bytes, len(input_bytes), ram_size)
    _check(abi().bfhip_host_run_ram(*args, None, 0, ctypes.byref(n_out), None, 0, ctypes.byref(n_rows)))
    out = (ctypes.c_ubyte * max(1, n_out.value))()
    rows = np.zeros((n_rows.value, 7), dtype=np.uint32)
    _check(abi().bfhip_host_run_ram(*args, out, n_out.value, ctypes.byref(n_out), rows.ctypes.data, rows.shape[0], ctypes.byref(n_rows)))
    return bytes(out[: n_out.value]), rows


class Trace(Owned):
    """Prover input resident in HBM (bfhip_trace_create): VM trace -> 13 component tables -> row-granular device columns. close() needs
    the context the trace lives on, so it is the caller's to call: a trace does not close itself when collected."""
    _close_on_del = False

    def __init__(self, ctx, code, input_bytes=b"", ram_size=0):
        """ram_size: Machine RAM cells (MachineBuilder::with_ram_size, machine.rs:56-60); 0 = the default 30000."""
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        ls = (ctypes.c_uint32 * 13)()
        steps, mc, ic = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(abi().bfhip_trace_create_ram(ctx._h, code.encode(), input_bytes, len(input_bytes), ram_size,
                                            ctypes.byref(self._h), ls, ctypes.byref(steps), ctypes.byref(mc), ctypes.byref(ic)))
        self.log_sizes = list(ls)
        self.n_steps, self.main_cells, self.interaction_cells = steps.value, mc.value, ic.value

    @classmethod
    def from_registers(cls, ctx, trace7, code_words):
        """What prove_brainfuck(&Machine) receives (mod.rs:471-473,508): the executed machine's register trace (n x 7 u32: clk, ip, ci,
        ni, mp, mv, mvi) and its compiled program words. No re-execution."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        tr = np.ascontiguousarray(trace7, dtype=np.uint32).reshape(-1, 7)
        code = np.ascontiguousarray(code_words, dtype=np.uint32)
        ls = (ctypes.c_uint32 * 13)()
        mc, ic = ctypes.c_uint64(), ctypes.c_uint64()
        _check(abi().bfhip_trace_create_from_registers(ctx._h, tr.ctypes.data, tr.shape[0], code.ctypes.data, code.size,
                                                       ctypes.byref(self._h), ls, ctypes.byref(mc), ctypes.byref(ic)))
        self.log_sizes = list(ls)
        self.n_steps, self.main_cells, self.interaction_cells = tr.shape[0], mc.value, ic.value
        return self

    @property
    def cells(self):
        return self.main_cells + self.interaction_cells

    def prove(self, log_max_rows=24, want_json=True):
        js, n = ctypes.c_void_p(), ctypes.c_size_t()
        times = (ctypes.c_double * 10)()
        _check_proof(abi().bfhip_prove_trace(self.ctx._h, self._h, log_max_rows, ctypes.byref(js) if want_json else None, ctypes.byref(n), None, times), self.ctx)
        return _take_host_string(js, n.value) if want_json else None, dict(zip(PHASES, list(times)))

    def check(self, lookup24=None):
        """bfhip_trace_check: the 13 AIRs asserted on this trace (logUp columns generated on the GPU), as a CheckResult. lookup24: (z, alpha)
        of Memory, Instruction, Processor; None = default_check_lookup(). A trace that is not a valid execution gives ok = False and the
        failing component, constraint and row — where a proof would only say ConstraintsNotSatisfied."""
        reps = (CheckReport * 13)()
        total = (ctypes.c_uint32 * 4)()
        n_bad = ctypes.c_int32()
        _check(abi().bfhip_trace_check(self.ctx._h, self._h, None if lookup24 is None else _u32s(lookup24), reps, total, ctypes.byref(n_bad)))
        res = CheckResult(r.as_dict() for r in reps)
        res.logup_total, res.n_bad_components = tuple(int(v) for v in total), n_bad.value
        return res

    def relations(self, max_entries=64):
        """bfhip_trace_relations: the lookup tuples of this trace's 13 tables that do not cancel (stwo's relation tracker), as a
        RelationResult: .balanced, .reports (3 dicts), .entries (at most max_entries per relation), .lines(). Names what a non-zero
        check().logup_total cannot: which tuple is yielded and never used, or used and never yielded, and by which table row."""
        return _relation_result(lambda reps, ents, cap: abi().bfhip_trace_relations(self.ctx._h, self._h, reps, ents, cap), max_entries)

    def column(self, component, column):
        n = ctypes.c_size_t()
        _check(abi().bfhip_trace_column(self.ctx._h, self._h, component, column, None, 0, ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.uint32)
        _check(abi().bfhip_trace_column(self.ctx._h, self._h, component, column, out.ctypes.data, out.size, ctypes.byref(n)))
        return out

    def close(self):
        if self._h:
            abi().bfhip_trace_destroy(self.ctx._h, self._h)
            self._h = ctypes.c_void_p()


def brainfuck_composition_at_point(log_sizes, claimed_sums, log_max_rows, lookup24, point8, sampled, random_coeff4, conventions=None):
    """bfhip_brainfuck_composition_at_point: the snapshot AIR's composition polynomial at a point from the sampled mask values — what a
    verifier assembled from PcsVerifier compares with the composition polynomial's own sampled value. sampled[tree][column] = list of
    QM31 (4 words each) for the preprocessed, main-trace and interaction trees. Host only."""
    n_cols = _u32s([len(t) for t in sampled[:3]])
    counts = _u32s([len(c) for t in sampled[:3] for c in t])
    flat = _u32s([w for t in sampled[:3] for c in t for q in c for w in q])
    out = (ctypes.c_uint32 * 4)()
    _check(abi().bfhip_brainfuck_composition_at_point(_u32s(log_sizes), _u32s([w for q in claimed_sums for w in q]), int(log_max_rows),
                                                      _u32s(lookup24), _u32s(point8), n_cols, counts, flat, _u32s(random_coeff4),
                                                      _conv_ref(conventions), out))
    return [int(v) for v in out]
