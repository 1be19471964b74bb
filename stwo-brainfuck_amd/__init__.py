"""MI355X-native Circle-STARK prover backend for the Brainfuck zkVM — Python host mirror over the C ABI (include/bfhip.h).

The product path is libbfhip.so (hand-written gfx950 kernels). There is no CPU fallback: if the library or a GPU is missing,
every entry point raises.  Reference interface mirrored: crates/brainfuck_prover/src/brainfuck_air/mod.rs:471 (prove_brainfuck),
:738 (verify_brainfuck) and stwo's PolyOps/MerkleOps/FriOps/QuotientOps trait surface (SURVEY.md §8 b).
"""
import ctypes
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BFHIP_LIBRARY: another build of the library (A/B runs; tests of the late-host and RCCL-double paths name libbfhip_testhooks.so, the
# -DBFHIP_TEST_HOOKS build — the default library has no test hooks)
_LIB_PATH = os.environ.get("BFHIP_LIBRARY") or os.path.join(_HERE, "libbfhip.so")
TESTHOOKS_LIBRARY = os.path.join(_HERE, "libbfhip_testhooks.so")
_lib = None

P = (1 << 31) - 1


class BfhipError(RuntimeError):
    pass


def lib():
    """Load libbfhip.so (built in-tree by `make -C stwo-brainfuck_amd/csrc`). Fails loudly when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise BfhipError(f"{_LIB_PATH} is missing: build it with __graft_entry__.build(); there is no CPU fallback")
        _lib = ctypes.CDLL(_LIB_PATH)
        _lib.bfhip_last_error.restype = ctypes.c_char_p
    return _lib


TRACE_REJECTED = -3


class TraceRejected(BfhipError):
    """BFHIP_TRACE_REJECTED: a proof's preflight (Context.set_preflight) refused the trace before proving it. str() = the rejection lines
    (bfhip_format_preflight); .check = the CheckResult of the 13 components, .relations = the RelationResult of the tuples that do not
    cancel (empty unless the logUp total is not zero)."""

    def __init__(self, text, check=None, relations=None):
        super().__init__(text)
        self.check, self.relations = check, relations


def _check(rc):
    if rc != 0:
        raise BfhipError(lib().bfhip_last_error().decode())


def _check_proof(rc, ctx):
    """_check for the proving entry points: BFHIP_TRACE_REJECTED raises TraceRejected with the context's preflight report."""
    if rc == TRACE_REJECTED:
        text = lib().bfhip_last_error().decode()
        raise TraceRejected(text, *ctx.last_preflight())
    _check(rc)


def device_count():
    return lib().bfhip_device_count()


def device_memory(device_id=0):
    """bfhip_device_memory: (free, total) bytes of one GPU right now."""
    f, t = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().bfhip_device_memory(device_id, ctypes.byref(f), ctypes.byref(t)))
    return f.value, t.value


def rccl_unique_id() -> bytes:
    """bfhip_rccl_unique_id: the 128-byte id rank 0 creates for a multi-process shard group (loads librccl on first use)."""
    buf = (ctypes.c_uint8 * 128)()
    _check(lib().bfhip_rccl_unique_id(buf))
    return bytes(buf)


class LocalGroup:
    """Rendezvous object of an in-process shard group (bfhip_local_group_create): `count` contexts of this process, one thread each."""

    def __init__(self, count):
        self._h = ctypes.c_void_p()
        _check(lib().bfhip_local_group_create(count, ctypes.byref(self._h)))
        self.count = count

    def close(self):
        if self._h:
            lib().bfhip_local_group_destroy(self._h)
            self._h = ctypes.c_void_p()


class Conventions(ctypes.Structure):
    """include/bfhip.h `bfhip_conventions`: the byte-level stwo conventions that cannot be confirmed offline, one switch each.
    All zero = the defaults (zero-state raw-compress Merkle nodes, raw-compress mix_u64, logUp mask order [0, -1])."""
    _fields_ = [("merkle_node_hash", ctypes.c_uint32), ("mix_u64", ctypes.c_uint32), ("logup_mask_order", ctypes.c_uint32), ("merkle_channel", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 4)]


_default_conventions = (0, 0, 0, 0)
_live_contexts = weakref.WeakSet()


def set_default_conventions(merkle_node_hash=0, mix_u64=0, logup_mask_order=0, merkle_channel=0):
    """Process-wide default of the Python mirror: adopted by every Context created afterwards, applied to the live ones, and used by
    verify_brainfuck(conventions=None). The C ABI itself has no global state: conventions are per context / per verify call."""
    global _default_conventions
    _default_conventions = (int(merkle_node_hash), int(mix_u64), int(logup_mask_order), int(merkle_channel))
    for c in list(_live_contexts):
        if c._h:
            c.set_conventions(*_default_conventions)


class PcsConfig(ctypes.Structure):
    """include/bfhip.h `bfhip_pcs_config`: stwo's PcsConfig (pow_bits, FriConfig { log_last_layer_degree_bound, log_blowup_factor, n_queries }).
    PcsConfig() = PcsConfig::default() = pow_bits 5, log_blowup_factor 1, log_last_layer_degree_bound 0, n_queries 3. The proof JSON does not
    carry it: verify a proof under the config it was made with."""
    _fields_ = [("pow_bits", ctypes.c_uint32), ("log_blowup_factor", ctypes.c_uint32), ("log_last_layer_degree_bound", ctypes.c_uint32),
                ("n_queries", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 4)]

    def __init__(self, pow_bits=5, log_blowup_factor=1, n_queries=3, log_last_layer_degree_bound=0):
        super().__init__(pow_bits, log_blowup_factor, log_last_layer_degree_bound, n_queries)

    def security_bits(self):
        return security_bits(self)

    def as_dict(self):
        return {"pow_bits": self.pow_bits, "log_blowup_factor": self.log_blowup_factor, "log_last_layer_degree_bound": self.log_last_layer_degree_bound,
                "n_queries": self.n_queries}

    def __eq__(self, other):
        return isinstance(other, PcsConfig) and self.as_dict() == other.as_dict() and list(self.reserved) == list(other.reserved)

    def __repr__(self):
        return "PcsConfig(pow_bits=%d, log_blowup_factor=%d, n_queries=%d, log_last_layer_degree_bound=%d)" % (
            self.pow_bits, self.log_blowup_factor, self.n_queries, self.log_last_layer_degree_bound)


def security_bits(pcs_config=None):
    """stwo's conjectured security of a PcsConfig: pow_bits + log_blowup_factor x n_queries (the default: 5 + 1 x 3 = 8)."""
    c = PcsConfig() if pcs_config is None else pcs_config
    return c.pow_bits + c.log_blowup_factor * c.n_queries


def _pcs_ref(pcs_config):
    return None if pcs_config is None else ctypes.byref(pcs_config)


CHANNEL_BLAKE2S, CHANNEL_POSEIDON252 = 0, 1
MERKLE_STWO_COMPRESS, MERKLE_RFC7693 = 0, 1
MIX_U64_COMPRESS, MIX_U64_HASH = 0, 1
LOGUP_MASK_CUR_PREV, LOGUP_MASK_PREV_CUR = 0, 1


COMPONENT_NAMES = ("memory", "instruction", "program", "processor", "jnz", "jz", "input", "left", "minus", "output", "plus", "right", "end_of_execution")
NO_CELL = (1 << 64) - 1


class CheckReport(ctypes.Structure):
    """include/bfhip.h `bfhip_check_report`: one component's AIR asserted on its trace domain (stwo's assert_constraints)."""
    _fields_ = [("component", ctypes.c_uint32), ("log_size", ctypes.c_uint32), ("n_bad_cells", ctypes.c_uint64), ("first_bad_cell", ctypes.c_uint64),
                ("first_bad_constraint", ctypes.c_int32), ("first_bad_value", ctypes.c_uint32 * 4), ("bad_per_constraint", ctypes.c_uint64 * 16),
                ("claimed_sum", ctypes.c_uint32 * 4), ("reserved", ctypes.c_uint32 * 3)]

    def as_dict(self):
        """Named fields; first_bad_cell / first_bad_row are None for a component without violations (first_bad_constraint is -1 then)."""
        none = self.first_bad_cell == NO_CELL
        return {"component": int(self.component), "name": COMPONENT_NAMES[self.component], "log_size": int(self.log_size), "ok": self.n_bad_cells == 0,
                "n_bad_cells": int(self.n_bad_cells), "first_bad_cell": None if none else int(self.first_bad_cell),
                "first_bad_row": None if none else int(self.first_bad_cell) >> 4, "first_bad_constraint": int(self.first_bad_constraint),
                "first_bad_value": [int(v) for v in self.first_bad_value], "bad_per_constraint": [int(v) for v in self.bad_per_constraint],
                "claimed_sum": [int(v) for v in self.claimed_sum]}


def format_check_failure(report):
    """One line for a component's report (a dict of CheckReport.as_dict()), e.g.
    "memory: constraint 6 fails at table row 0 (cell 0), value (2, 0, 0, 0); 16 cells violate it"; "<name>: ok" without violations."""
    if report["n_bad_cells"] == 0:
        return "%s: ok" % report["name"]
    j = report["first_bad_constraint"]
    return "%s: constraint %d fails at table row %d (cell %d), value (%s); %d cells violate it" % (
        report["name"], j, report["first_bad_row"], report["first_bad_cell"], ", ".join(str(v) for v in report["first_bad_value"]), report["bad_per_constraint"][j])


def default_check_lookup():
    """The lookup elements bfhip_trace_check uses when none are given (include/bfhip.h): (z, alpha) of Memory, Instruction, Processor as
    the three `draw_felts(2)` of mod.rs:589-597 on Blake2sChannel::default() — 24 u32. Fixed, so a report can be reproduced."""
    import hashlib
    import struct
    out = []
    for k in range(3):
        words = struct.unpack("<8I", hashlib.blake2s(bytes(32) + struct.pack("<I", k) + bytes(28)).digest())
        assert all(w < 2 * P for w in words)      # none of the three draws is redrawn
        out += [w % P for w in words]
    return out


class CheckResult(list):
    """Trace.check(): the 13 component reports (dicts, claim order) + logup_total (the sum of the 13 claimed sums, 4 u32),
    n_bad_components and ok = no violation and a zero logUp total."""
    logup_total = (0, 0, 0, 0)
    n_bad_components = 0

    @property
    def ok(self):
        return self.n_bad_components == 0 and not any(self.logup_total)

    def failures(self):
        """One format_check_failure line per failing component, then the logUp total if it is not zero."""
        lines = [format_check_failure(r) for r in self if r["n_bad_cells"]]
        if any(self.logup_total):
            lines.append("logUp: the 13 claimed sums add up to (%s), not zero" % ", ".join(str(v) for v in self.logup_total))
        return lines


RELATION_NAMES = ("memory", "instruction", "processor")
NO_ROW = (1 << 64) - 1


class RelationEntry(ctypes.Structure):
    """include/bfhip.h `bfhip_relation_entry`: one unbalanced tuple of a lookup relation (stwo's relation tracker)."""
    _fields_ = [("relation", ctypes.c_uint32), ("n_words", ctypes.c_uint32), ("tuple", ctypes.c_uint32 * 7), ("net", ctypes.c_uint32),
                ("n_yield", ctypes.c_uint64), ("n_use", ctypes.c_uint64), ("n_other", ctypes.c_uint64),
                ("first_yield_table", ctypes.c_int32), ("first_use_table", ctypes.c_int32), ("first_yield_row", ctypes.c_uint64), ("first_use_row", ctypes.c_uint64),
                ("reserved", ctypes.c_uint32 * 2)]

    def as_dict(self, names=None):
        """Named fields; tuple cut to n_words; first_yield / first_use = (table index, row) or None. names: the relations' names (None =
        RELATION_NAMES, the three Brainfuck relations)."""
        return {"relation": int(self.relation), "name": (RELATION_NAMES if names is None else names)[self.relation], "tuple": tuple(int(v) for v in self.tuple[: self.n_words]), "net": int(self.net),
                "n_yield": int(self.n_yield), "n_use": int(self.n_use), "n_other": int(self.n_other),
                "first_yield": None if self.first_yield_table < 0 else (int(self.first_yield_table), int(self.first_yield_row)),
                "first_use": None if self.first_use_table < 0 else (int(self.first_use_table), int(self.first_use_row))}


class RelationReport(ctypes.Structure):
    """include/bfhip.h `bfhip_relation_report`: the counts of one relation."""
    _fields_ = [("relation", ctypes.c_uint32), ("n_words", ctypes.c_uint32), ("n_entries", ctypes.c_uint64), ("n_tuples", ctypes.c_uint64),
                ("n_unbalanced", ctypes.c_uint64), ("n_reported", ctypes.c_uint64), ("reserved", ctypes.c_uint32 * 2)]

    def as_dict(self, names=None):
        return {"relation": int(self.relation), "name": (RELATION_NAMES if names is None else names)[self.relation], "n_words": int(self.n_words), "n_entries": int(self.n_entries),
                "n_tuples": int(self.n_tuples), "n_unbalanced": int(self.n_unbalanced), "n_reported": int(self.n_reported)}


class RelationTable(ctypes.Structure):
    """include/bfhip.h `bfhip_relation_table`."""
    _fields_ = [("component", ctypes.c_int32), ("log_size", ctypes.c_uint32), ("main_rows_h", ctypes.POINTER(ctypes.c_void_p))]


class RelationProgramTable(ctypes.Structure):
    """include/bfhip.h `bfhip_relation_program_table` (32 bytes): one table of Context.relation_program_summary."""
    _fields_ = [("program", ctypes.c_void_p), ("log_size", ctypes.c_uint32), ("row_shift", ctypes.c_uint32), ("cols_h", ctypes.POINTER(ctypes.c_void_p)),
                ("col_shifts_h", ctypes.POINTER(ctypes.c_uint32))]


def format_relation_entry(entry, table_names=None):
    """One line for an unbalanced tuple (a dict of RelationEntry.as_dict()), e.g.
    "processor relation: (1, 1, 35, 43, 0, 1, 1) net +1: yielded 1x (first: processor row 1), used 0x". net is printed signed (values above
    p / 2 read as negative). table_names[i] names table i of the list the summary ran over; None = COMPONENT_NAMES (a resident trace)."""
    names = COMPONENT_NAMES if table_names is None else table_names
    net = entry["net"] - P if entry["net"] > P // 2 else entry["net"]
    where = lambda at: "" if at is None else " (first: %s row %d)" % (names[at[0]], at[1])
    line = "%s relation: (%s) net %+d: yielded %dx%s, used %dx%s" % (entry["name"], ", ".join(str(v) for v in entry["tuple"]), net, entry["n_yield"],
                                                                      where(entry["first_yield"]), entry["n_use"], where(entry["first_use"]))
    return line + (", %d rows with another multiplicity" % entry["n_other"] if entry["n_other"] else "")


class RelationResult:
    """Context.relation_summary() / Trace.relations(): reports = the 3 relations' counts (dicts), entries = the reported unbalanced tuples
    (dicts, relation by relation, each in lexicographic order of the tuple), balanced = no relation has an unbalanced tuple."""

    def __init__(self, reports, entries, table_names=None):
        self.reports, self.entries, self.table_names = reports, entries, table_names

    @property
    def balanced(self):
        return all(r["n_unbalanced"] == 0 for r in self.reports)

    def lines(self):
        """One format_relation_entry line per reported tuple, then one line per relation whose report was cut at max_entries."""
        out = [format_relation_entry(e, self.table_names) for e in self.entries]
        out += ["%s relation: %d more unbalanced tuples not listed" % (r["name"], r["n_unbalanced"] - r["n_reported"]) for r in self.reports if r["n_unbalanced"] > r["n_reported"]]
        return out


class MultiplicityReport(ctypes.Structure):
    """include/bfhip.h `bfhip_multiplicity_report` (80 bytes): the counts of Context.relation_program_multiplicities."""
    _fields_ = [("relation", ctypes.c_uint32), ("n_words", ctypes.c_uint32), ("target_table", ctypes.c_uint32), ("target_entry", ctypes.c_uint32),
                ("n_rows", ctypes.c_uint64), ("n_row_tuples", ctypes.c_uint64), ("n_entries", ctypes.c_uint64), ("n_tuples", ctypes.c_uint64),
                ("n_filled", ctypes.c_uint64), ("n_missing", ctypes.c_uint64), ("n_reported", ctypes.c_uint64), ("reserved", ctypes.c_uint32 * 2)]

    def as_dict(self, names=None):
        d = {f: int(getattr(self, f)) for f, _ in self._fields_[:-1]}
        d["name"] = ("relation %d" % self.relation) if names is None else names[self.relation]
        return d


class MultiplicityResult:
    """Context.relation_program_multiplicities(): report = the counts (a dict), missing = the reported tuples with a non-zero net that no
    row of the target table holds (dicts shaped like RelationResult.entries, in lexicographic order), ok = there is none."""

    def __init__(self, report, missing, table_names, target_name):
        self.report, self.missing, self.table_names, self.target_name = report, missing, table_names, target_name

    @property
    def ok(self):
        return self.report["n_missing"] == 0

    def lines(self):
        """One format_relation_entry line per reported missing tuple, each followed by "; no row of <table name> holds it", then one line if
        the list was cut at max_missing."""
        out = ["%s; no row of %s holds it" % (format_relation_entry(e, self.table_names), self.target_name) for e in self.missing]
        if self.report["n_missing"] > self.report["n_reported"]:
            out.append("%s relation: %d more missing tuples not listed" % (self.report["name"], self.report["n_missing"] - self.report["n_reported"]))
        return out


class PreflightReport(ctypes.Structure):
    """include/bfhip.h `bfhip_preflight_report` (4064 bytes): what the last proof of a context that reached the preflight found."""
    _fields_ = [("ran", ctypes.c_uint32), ("rejected", ctypes.c_uint32), ("n_bad_components", ctypes.c_int32), ("n_entries", ctypes.c_uint32),
                ("logup_total", ctypes.c_uint32 * 4), ("components", CheckReport * 13), ("relations", RelationReport * 3), ("entries", RelationEntry * 12),
                ("seconds", ctypes.c_double), ("reserved", ctypes.c_uint64 * 3)]

    def results(self):
        """(CheckResult, RelationResult): the CheckResult also carries ran, rejected and seconds."""
        check = CheckResult(r.as_dict() for r in self.components)
        check.logup_total, check.n_bad_components = tuple(int(v) for v in self.logup_total), int(self.n_bad_components)
        check.ran, check.rejected, check.seconds = bool(self.ran), bool(self.rejected), float(self.seconds)
        ents = [self.entries[4 * k + i].as_dict() for k in range(3) for i in range(min(4, self.relations[k].n_reported))]
        reps = [self.relations[k].as_dict() if self.relations[k].n_words else dict(RelationReport(k, (3, 3, 7)[k]).as_dict()) for k in range(3)]
        return check, RelationResult(reps, ents)


def format_preflight_lines(check, relations):
    """The lines of a rejection (what bfhip_format_preflight joins by "\\n"): the headline, CheckResult.failures(), RelationResult.lines().
    check: a CheckResult with .ran / .rejected (PreflightReport.results())."""
    if not getattr(check, "ran", True):
        return ["preflight: did not run"]
    if not getattr(check, "rejected", not check.ok):
        return ["preflight: ok"]
    what = []
    if check.n_bad_components:
        what.append("%d of 13 components violate their constraints" % check.n_bad_components)
    if any(check.logup_total):
        what.append("the logUp total is not zero")
    return ["TraceRejected: " + " and ".join(what)] + check.failures() + (relations.lines() if relations is not None else [])


def format_preflight(report):
    """bfhip_format_preflight of a PreflightReport (host only, no GPU): the text a rejection carries."""
    need = ctypes.c_size_t()
    rc = lib().bfhip_format_preflight(ctypes.byref(report), None, ctypes.c_size_t(0), ctypes.byref(need))
    if rc not in (0, -2):
        raise BfhipError(lib().bfhip_last_error().decode())
    buf = ctypes.create_string_buffer(need.value)
    _check(lib().bfhip_format_preflight(ctypes.byref(report), buf, ctypes.c_size_t(need.value), None))
    return buf.value.decode()


def _relation_result(call, max_entries, table_names=None):
    reps = (RelationReport * 3)()
    ents = (RelationEntry * (3 * max_entries))() if max_entries else None
    _check(call(reps, ents, max_entries))
    return RelationResult([r.as_dict() for r in reps], [ents[k * max_entries + i].as_dict() for k in range(3) for i in range(reps[k].n_reported)], table_names)


class Context:
    """One GPU + one HIP stream + the twiddle tree (mod.rs:480-487: twiddles, channel and commitment scheme setup)."""

    def __init__(self, device_id=0, max_log_domain=22):
        self._h = ctypes.c_void_p()
        _check(lib().bfhip_ctx_create(device_id, max_log_domain, ctypes.byref(self._h)))
        self.max_log_domain = max_log_domain
        _live_contexts.add(self)
        if _default_conventions != (0, 0, 0, 0):
            self.set_conventions(*_default_conventions)

    def close(self):
        if self._h:
            lib().bfhip_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(lib().bfhip_ctx_sync(self._h))

    def set_conventions(self, merkle_node_hash=0, mix_u64=0, logup_mask_order=0, merkle_channel=0):
        cv = Conventions(merkle_node_hash, mix_u64, logup_mask_order, merkle_channel)
        _check(lib().bfhip_ctx_set_conventions(self._h, ctypes.byref(cv)))

    def get_conventions(self):
        cv = Conventions()
        _check(lib().bfhip_ctx_get_conventions(self._h, ctypes.byref(cv)))
        return cv.merkle_node_hash, cv.mix_u64, cv.logup_mask_order, cv.merkle_channel

    def set_pcs_config(self, pcs_config=None):
        """bfhip_ctx_set_pcs_config: the PcsConfig of every later proof of this context (None = the default). Needs
        max_log_domain >= log_max_rows + log_blowup_factor + 1."""
        _check(lib().bfhip_ctx_set_pcs_config(self._h, _pcs_ref(pcs_config)))

    def pcs_config(self):
        out = PcsConfig()
        _check(lib().bfhip_ctx_get_pcs_config(self._h, ctypes.byref(out)))
        return out

    def set_overlap(self, mask=1):
        """bit 0: tree commitment (Merkle beside the transforms of the smaller columns), bit 1: quotients / FRI first-layer tree, bit 2 (shard
        groups): the send-receive of a tree's largest size class on the partner stream beside the transforms of the smaller columns."""
        _check(lib().bfhip_ctx_set_overlap(self._h, int(mask)))

    def set_sync_policy(self, blocking):
        """bfhip_ctx_set_sync_policy: True = the host sleeps in its waits (more waiting contexts than cores), False (default) = polls first."""
        _check(lib().bfhip_ctx_set_sync_policy(self._h, 1 if blocking else 0))

    def set_mailbox(self, mode=-2, timeout_ms=0, test_delay_ms=-1):
        """bfhip_ctx_set_mailbox: mode -2 keeps the mode / -1 automatic / 0 off / 1 on; timeout_ms 0 keeps the timeout; test_delay_ms < 0 keeps
        the (test) delay — a positive delay needs the test-hooks build of the library."""
        _check(lib().bfhip_ctx_set_mailbox(self._h, int(mode), int(timeout_ms), int(test_delay_ms)))

    def last_proof_flags(self):
        """bfhip_ctx_last_proof_flags: {mailbox_order, kept_preprocessed, shared_preprocessed, replicated_transforms, split_gather, fri_fold_leaf, preflight}
        of the last completed proof."""
        f = ctypes.c_uint32()
        _check(lib().bfhip_ctx_last_proof_flags(self._h, ctypes.byref(f)))
        return {"mailbox_order": bool(f.value & 1), "kept_preprocessed": bool(f.value & 2), "shared_preprocessed": bool(f.value & 4), "replicated_transforms": bool(f.value & 8),
                "split_gather": bool(f.value & 16), "fri_fold_leaf": bool(f.value & 32), "preflight": bool(f.value & 64)}

    def set_preflight(self, on=True):
        """bfhip_ctx_set_preflight: every later proof of this context first asserts the 13 AIRs and the logUp total on its tables (one batched
        launch pair, one read-back) and raises TraceRejected — naming component, constraint, row and unbalanced tuple — instead of proving a
        trace that cannot be proved. A filter, not a soundness gate: the lookup elements are the fixed public ones of Trace.check()."""
        _check(lib().bfhip_ctx_set_preflight(self._h, 1 if on else 0))

    def preflight(self):
        on = ctypes.c_int32()
        _check(lib().bfhip_ctx_get_preflight(self._h, ctypes.byref(on)))
        return bool(on.value)

    def last_preflight_report(self):
        """bfhip_ctx_last_preflight as the raw PreflightReport."""
        rep = PreflightReport()
        _check(lib().bfhip_ctx_last_preflight(self._h, ctypes.byref(rep)))
        return rep

    def last_preflight(self):
        """bfhip_ctx_last_preflight: (CheckResult, RelationResult) of the last proof of this context that reached the preflight. The
        CheckResult also has .ran, .rejected and .seconds (host wall time of the preflight)."""
        return self.last_preflight_report().results()

    def clock_probe(self, seconds=0.6):
        """bfhip_clock_probe: {ghz (median over workgroups), ghz_min, ghz_max, G_compressions_per_s, launches, ms_per_launch} of a register-only
        Blake2s loop run back to back for `seconds` — the clock this device sustains under the dominant kernel's instruction mix."""
        out = (ctypes.c_double * 6)()
        _check(lib().bfhip_clock_probe(self._h, ctypes.c_double(seconds), out))
        return dict(zip(("ghz", "ghz_min", "ghz_max", "G_compressions_per_s", "launches", "ms_per_launch"), [float(v) for v in out]))

    def clock_probe_mix(self, seconds=0.5, log_nodes=22):
        """bfhip_clock_probe_mix: {ghz, G_compressions_per_s, launches, us_per_launch, sampler_spanned_the_window, sampler_seconds} — the clock held under the REAL
        Merkle kernel (sidecar sampler) and that kernel's rate on an inner layer of 2^log_nodes nodes."""
        out = (ctypes.c_double * 6)()
        _check(lib().bfhip_clock_probe_mix(self._h, ctypes.c_double(seconds), int(log_nodes), out))
        d = dict(zip(("ghz", "G_compressions_per_s", "launches", "us_per_launch", "sampler_spanned_the_window", "sampler_seconds"), [float(v) for v in out]))
        d["sampler_spanned_the_window"] = bool(d["sampler_spanned_the_window"])
        return d

    def memory(self):
        """bfhip_ctx_memory: {arena_reserved, arena_peak, twiddles, arena_in_use} in bytes."""
        out = (ctypes.c_uint64 * 4)()
        _check(lib().bfhip_ctx_memory(self._h, out))
        return dict(zip(("arena_reserved", "arena_peak", "twiddles", "arena_in_use"), [int(v) for v in out]))

    def set_table_builder(self, on_gpu=True):
        """Where this context builds the 13 component tables: GPU kernels (default) or the host builders. Identical results."""
        _check(lib().bfhip_ctx_set_table_builder(self._h, int(on_gpu)))

    # -- one proof over several GPUs (shard group: bfhip_ctx_join_*_group) -----------------------------------------------------------------
    def join_local_group(self, group, rank):
        """Makes this context rank `rank` of a LocalGroup: N contexts of this process, one host thread each, prove ONE trace together."""
        _check(lib().bfhip_ctx_join_local_group(self._h, group._h, rank))
        self._group = group          # keep the rendezvous object alive as long as the context uses it

    def join_rccl_group(self, unique_id: bytes, rank, count):
        """One process per GPU: `unique_id` is rccl_unique_id() of rank 0, handed over by the host program (replicas.share_unique_id)."""
        if len(unique_id) != 128:
            raise BfhipError("an RCCL unique id has 128 bytes")
        _check(lib().bfhip_ctx_join_rccl_group(self._h, unique_id, rank, count))

    def set_shard_policy(self, policy=-1):
        """bfhip_ctx_set_shard_policy: -1 automatic, 0 exchange columns -> rows, 1 replicate the transforms (every rank of a group the same)."""
        _check(lib().bfhip_ctx_set_shard_policy(self._h, int(policy)))

    def leave_group(self):
        _check(lib().bfhip_ctx_leave_group(self._h))
        self._group = None

    def group_stats(self):
        """{all_gathers, max_reduces, exchanges, bytes_sent} of this rank since it joined its shard group."""
        out = (ctypes.c_uint64 * 4)()
        _check(lib().bfhip_ctx_group_stats(self._h, out))
        return dict(zip(("all_gathers", "max_reduces", "exchanges", "bytes_sent"), [int(v) for v in out]))

    def group_times(self):
        """{all_gather_ms, max_reduce_ms, exchange_ms}: GPU-side time of this rank's collectives since it joined its shard group."""
        out = (ctypes.c_double * 3)()
        _check(lib().bfhip_ctx_group_times(self._h, out))
        return dict(zip(("all_gather_ms", "max_reduce_ms", "exchange_ms"), [float(v) for v in out]))

    def group_latency(self, reset=False):
        """bfhip_ctx_group_latency: per kind of collective {count, gpu_us: {p50, p90, max}, host_us: {p50, p90, max}} since the join / the last reset."""
        out = (ctypes.c_double * 21)()
        _check(lib().bfhip_ctx_group_latency(self._h, 1 if reset else 0, out))
        res = {}
        for k, name in enumerate(("all_gather", "max_reduce", "exchange")):
            v = [float(x) for x in out[7 * k:7 * k + 7]]
            res[name] = {"count": int(v[0]), "gpu_us": {"p50": round(v[1], 1), "p90": round(v[2], 1), "max": round(v[3], 1)},
                         "host_us": {"p50": round(v[4], 1), "p90": round(v[5], 1), "max": round(v[6], 1)}}
        return res

    def group_info(self):
        r, n, t = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_char_p()
        _check(lib().bfhip_ctx_group_info(self._h, ctypes.byref(r), ctypes.byref(n), ctypes.byref(t)))
        return r.value, n.value, (t.value or b"").decode()

    # -- buffers ---------------------------------------------------------------------------------------------------
    def malloc(self, nbytes):
        p = ctypes.c_void_p()
        _check(lib().bfhip_malloc(self._h, ctypes.c_size_t(nbytes), ctypes.byref(p)))
        return p.value

    def free(self, ptr):
        _check(lib().bfhip_free(self._h, ctypes.c_void_p(ptr)))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        ptr = self.malloc(arr.nbytes)
        _check(lib().bfhip_upload(self._h, ctypes.c_void_p(ptr), arr.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(arr.nbytes)))
        return ptr

    def download(self, ptr, n, dtype=np.uint32):
        out = np.empty(n, dtype=dtype)
        _check(lib().bfhip_download(self._h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), ctypes.c_size_t(out.nbytes)))
        return out

    @staticmethod
    def _ptr_array(ptrs):
        return (ctypes.c_void_p * len(ptrs))(*ptrs)

    # -- PolyOps ---------------------------------------------------------------------------------------------------
    def interpolate(self, src_ptrs, dst_ptrs, log_size, replicated=False):
        _check(lib().bfhip_interpolate(self._h, self._ptr_array(src_ptrs), self._ptr_array(dst_ptrs), len(src_ptrs), log_size, int(replicated)))

    def evaluate(self, coeff_ptrs, dst_ptrs, log_size, log_eval, replicated=False):
        _check(lib().bfhip_evaluate(self._h, self._ptr_array(coeff_ptrs), self._ptr_array(dst_ptrs), len(coeff_ptrs), log_size, log_eval, int(replicated)))

    def is_first_coeffs(self, log_min, log_max, dst_ptrs):
        """interpolate(gen_is_first(n)) for n = log_min..log_max in closed form (mod.rs:497); dst_ptrs[n - log_min] may be None."""
        arr = (ctypes.c_void_p * len(dst_ptrs))(*[p or None for p in dst_ptrs])
        _check(lib().bfhip_is_first_coeffs(self._h, log_min, log_max, arr))

    def is_first_lde(self, log_min, log_max, log_blowup, dst_ptrs):
        """evaluate(interpolate(gen_is_first(n))) on 2^(n + log_blowup) cells for n = log_min..log_max in closed form; dst_ptrs[n - log_min] may be None."""
        arr = (ctypes.c_void_p * len(dst_ptrs))(*[p or None for p in dst_ptrs])
        _check(lib().bfhip_is_first_lde(self._h, log_min, log_max, log_blowup, arr))

    def is_first_eval_at_point(self, log_size, point8):
        """eval_at_point of IsFirst(log_size) in closed form (no coefficient column)."""
        pt = (ctypes.c_uint32 * 8)(*[int(v) for v in point8])
        out = (ctypes.c_uint32 * 4)()
        _check(lib().bfhip_is_first_eval_at_point(self._h, log_size, pt, out))
        return list(out)

    def eval_at_point(self, coeff_ptr, log_size, point8, replicated=False):
        pt = (ctypes.c_uint32 * 8)(*[int(v) for v in point8])
        out = (ctypes.c_uint32 * 4)()
        _check(lib().bfhip_eval_at_point(self._h, ctypes.c_void_p(coeff_ptr), log_size, int(replicated), pt, out))
        return list(out)

    # -- ColumnOps / FieldOps / AccumulationOps ---------------------------------------------------------------------------------
    def broadcast16(self, rows_ptr, dst_ptr, n_rows):
        _check(lib().bfhip_broadcast16(self._h, ctypes.c_void_p(rows_ptr), ctypes.c_void_p(dst_ptr), ctypes.c_size_t(n_rows)))

    def bit_reverse(self, src_ptr, dst_ptr, log_size):
        _check(lib().bfhip_bit_reverse(self._h, ctypes.c_void_p(src_ptr), ctypes.c_void_p(dst_ptr), log_size))

    def batch_inverse_m31(self, src_ptr, dst_ptr, n):
        _check(lib().bfhip_batch_inverse_m31(self._h, ctypes.c_void_p(src_ptr), ctypes.c_void_p(dst_ptr), ctypes.c_size_t(n)))

    def batch_inverse_qm31(self, src_ptrs, dst_ptrs, n):
        _check(lib().bfhip_batch_inverse_qm31(self._h, self._ptr_array(src_ptrs), self._ptr_array(dst_ptrs), ctypes.c_size_t(n)))

    def accumulate(self, dst_ptr, src_ptr, n):
        _check(lib().bfhip_accumulate(self._h, ctypes.c_void_p(dst_ptr), ctypes.c_void_p(src_ptr), ctypes.c_size_t(n)))

    # -- MerkleOps / FriOps / GrindOps -------------------------------------------------------------------------------------------------
    def merkle_commit_layer(self, log_size, prev_ptr, col_ptrs, out_ptr, col_shifts=None):
        sh = None if col_shifts is None else (ctypes.c_uint32 * len(col_shifts))(*col_shifts)
        _check(lib().bfhip_merkle_commit_layer(self._h, log_size, ctypes.c_void_p(prev_ptr) if prev_ptr else None, self._ptr_array(col_ptrs), sh, len(col_ptrs), ctypes.c_void_p(out_ptr)))

    def merkle_commit_layer_poseidon252(self, log_size, prev_ptr, col_ptrs, out_ptr, col_shifts=None):
        sh = None if col_shifts is None else (ctypes.c_uint32 * len(col_shifts))(*col_shifts)
        _check(lib().bfhip_merkle_commit_layer_poseidon252(self._h, log_size, ctypes.c_void_p(prev_ptr) if prev_ptr else None, self._ptr_array(col_ptrs), sh, len(col_ptrs), ctypes.c_void_p(out_ptr)))

    def hades_permutation(self, state3):
        """state3: three Python ints < p. Returns three ints."""
        words = []
        for x in state3:
            words += [(int(x) >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
        out = (ctypes.c_uint32 * 24)()
        _check(lib().bfhip_hades_permutation(self._h, (ctypes.c_uint32 * 24)(*words), out))
        return [sum(int(out[8 * k + i]) << (32 * i) for i in range(8)) for k in range(3)]

    def fold_line(self, src_ptrs, dst_ptrs, log_size, alpha4):
        _check(lib().bfhip_fold_line(self._h, self._ptr_array(src_ptrs), self._ptr_array(dst_ptrs), log_size, (ctypes.c_uint32 * 4)(*[int(v) for v in alpha4])))

    def fri_fold_leaf(self, src_ptrs, quot_ptrs, dst_ptrs, log_size, alpha4, out_ptr):
        """bfhip_fri_fold_leaf: fold into a layer of 2^log_size rows and hash its rows in one launch. src_ptrs None: the first line layer
        (circle fold of quot_ptrs alone); quot_ptrs None: a plain line fold. Whole layers only."""
        _check(lib().bfhip_fri_fold_leaf(self._h, self._ptr_array(src_ptrs) if src_ptrs is not None else None, self._ptr_array(quot_ptrs) if quot_ptrs is not None else None,
                                         self._ptr_array(dst_ptrs), log_size, (ctypes.c_uint32 * 4)(*[int(v) for v in alpha4]), ctypes.c_void_p(out_ptr)))

    def fold_circle_into_line(self, dst_ptrs, src_ptrs, log_size, alpha4):
        _check(lib().bfhip_fold_circle_into_line(self._h, self._ptr_array(dst_ptrs), self._ptr_array(src_ptrs), log_size, (ctypes.c_uint32 * 4)(*[int(v) for v in alpha4])))

    def grind(self, digest32, pow_bits):
        nonce = ctypes.c_uint64()
        _check(lib().bfhip_grind(self._h, bytes(digest32), pow_bits, ctypes.byref(nonce)))
        return nonce.value

    def grind_poseidon252(self, digest32, pow_bits, start_nonce=0, with_tried=False):
        """GrindOps::grind for Poseidon252Channel: the smallest nonce >= start_nonce whose poseidon_hash(digest, nonce) has >= pow_bits
        trailing zeros in that channel's sense. digest32: the felt252 digest as 32 canonical little-endian bytes.
        with_tried: also return the number of nonces scanned (launches x span)."""
        digest32 = bytes(digest32)
        if len(digest32) != 32:
            raise ValueError("grind_poseidon252: the digest is 32 bytes")
        nonce, tried = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().bfhip_grind_poseidon252(self._h, digest32, ctypes.c_uint32(pow_bits), ctypes.c_uint64(start_nonce), ctypes.byref(nonce), ctypes.byref(tried)))
        return (nonce.value, tried.value) if with_tried else nonce.value

    def gather(self, col_ptr, indices):
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        out = np.empty(idx.size, dtype=np.uint32)
        _check(lib().bfhip_gather(self._h, ctypes.c_void_p(col_ptr), idx.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(idx.size), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    # -- per-component AIR operations (LogupTraceGenerator / ComponentProver / QuotientOps) --------------------------------------------
    @staticmethod
    def _u32s(values):
        values = [int(v) for v in values]
        return (ctypes.c_uint32 * len(values))(*values)

    def logup_generate(self, component, log_size, main_row_ptrs, lookup24, out_col_ptrs):
        """interaction_trace_evaluation of one component; returns its claimed sum (4 u32)."""
        claimed = (ctypes.c_uint32 * 4)()
        _check(lib().bfhip_logup_generate(self._h, component, log_size, self._ptr_array(main_row_ptrs), self._u32s(lookup24), self._ptr_array(out_col_ptrs), claimed))
        return list(claimed)

    def eval_constraints(self, component, log_size, is_first_ptr, main_lde_ptrs, inter_lde_ptrs, lookup24, claimed4, coeffs, acc_ptrs, main_shifts=None, inter_shifts=None):
        """evaluate_constraint_quotients_on_domain of one component, accumulated into the 4 coordinate columns acc_ptrs."""
        _check(lib().bfhip_eval_constraints(self._h, component, log_size, ctypes.c_void_p(is_first_ptr), self._ptr_array(main_lde_ptrs),
                                            None if main_shifts is None else self._u32s(main_shifts), self._ptr_array(inter_lde_ptrs),
                                            None if inter_shifts is None else self._u32s(inter_shifts), self._u32s(lookup24), self._u32s(claimed4),
                                            self._u32s(coeffs), self._ptr_array(acc_ptrs)))

    def air_eval_domain(self, program, log_size, log_expand, col_ptrs, params, coeffs, acc_ptrs, col_shifts=None):
        """bfhip_air_eval_domain: the constraints of an AirProgram on CanonicCoset(log_size + log_expand).circle_domain(), each times its
        coefficient, the sum times 1 / vanishing, added into the 4 coordinate columns acc_ptrs. col_ptrs: one device column per program column
        (2^(log_size + log_expand - shift) cells); params / coeffs: QM31 values (4 words each), one per parameter / constraint.
        program: an AirProgram (interpreted), or the CompiledAir that this context's air_compile made of one (its own kernel; same result)."""
        params, coeffs = [list(q) for q in params], [list(q) for q in coeffs]
        if any(len(q) != 4 for q in params + coeffs):
            raise ValueError("a parameter or coefficient is 4 words")
        if len(col_ptrs) != program.shape["n_cols"] or (col_shifts is not None and len(col_shifts) != len(col_ptrs)):
            raise ValueError("one column pointer (and shift) per program column")
        if len(acc_ptrs) != 4:
            raise ValueError("the accumulator is 4 coordinate columns")
        # a CompiledAir (Context.air_compile) runs its own kernel behind the same checks: bfhip_air_kernel_eval_domain
        entry = lib().bfhip_air_kernel_eval_domain if isinstance(program, CompiledAir) else lib().bfhip_air_eval_domain
        _check(entry(self._h, program._h, int(log_size), int(log_expand), self._ptr_array(col_ptrs) if col_ptrs else None,
                     None if col_shifts is None or not col_ptrs else self._u32s(col_shifts),
                     self._u32s([w for q in params for w in q]) if params else None, len(params),
                     self._u32s([w for q in coeffs for w in q]) if coeffs else None, len(coeffs), self._ptr_array(acc_ptrs)))

    def air_compile(self, program):
        """bfhip_air_compile: the AirProgram as its own gfx950 kernel, generated (AirProgram.source) and compiled in-process for this
        context's device. Returns a CompiledAir, which air_eval_domain accepts in place of the program; the program may be closed."""
        return CompiledAir(self, program)

    def air_check(self, program, log_size, col_ptrs, params, col_shifts=None):
        """bfhip_air_check: the constraints of an AirProgram asserted on the trace domain CanonicCoset(log_size) itself (stwo's
        assert_constraints for any AIR). col_ptrs: one device column per program column (2^(log_size - shift) cells); params: QM31 values (4
        words each). Returns the AirCheckReport (as_dict() for named fields, format_air_check for the text); violations are a result, not
        an error."""
        params = [list(q) for q in params]
        if any(len(q) != 4 for q in params):
            raise ValueError("a parameter is 4 words")
        if len(col_ptrs) != program.shape["n_cols"] or (col_shifts is not None and len(col_shifts) != len(col_ptrs)):
            raise ValueError("one column pointer (and shift) per program column")
        rep = AirCheckReport()
        _check(lib().bfhip_air_check(self._h, program._h, int(log_size), self._ptr_array(col_ptrs) if col_ptrs else None,
                                     None if col_shifts is None or not col_ptrs else self._u32s(col_shifts),
                                     self._u32s([w for q in params for w in q]) if params else None, len(params), ctypes.byref(rep)))
        return rep

    def logup_program_generate(self, program, log_size, col_ptrs, params, out_col_ptrs, col_shifts=None):
        """bfhip_logup_program_generate: the logUp interaction trace of a LogupProgram on CanonicCoset(log_size).circle_domain(). col_ptrs: one
        device column per program column (2^(log_size - shift) cells); params: QM31 values (4 words each); out_col_ptrs: 4 full-size
        coordinate columns per logUp column. Returns the claimed sum (4 u32). A zero denominator raises BfhipError naming fraction and cell."""
        params = [list(q) for q in params]
        if any(len(q) != 4 for q in params):
            raise ValueError("a parameter is 4 words")
        if len(col_ptrs) != program.shape["n_cols"] or (col_shifts is not None and len(col_shifts) != len(col_ptrs)):
            raise ValueError("one column pointer (and shift) per program column")
        if len(out_col_ptrs) != 4 * program.shape["n_logup_cols"]:
            raise ValueError("4 coordinate columns per logUp column")
        claimed = (ctypes.c_uint32 * 4)()
        _check(lib().bfhip_logup_program_generate(self._h, program._h, int(log_size), self._ptr_array(col_ptrs) if col_ptrs else None,
                                                  None if col_shifts is None or not col_ptrs else self._u32s(col_shifts),
                                                  self._u32s([w for q in params for w in q]) if params else None, len(params),
                                                  self._ptr_array(out_col_ptrs), claimed))
        return list(claimed)

    def check_constraints(self, component, log_size, main_row_ptrs, logup_col_ptrs, lookup24, claimed4):
        """bfhip_check_constraints: one component's AIR asserted on its trace domain (stwo's assert_constraints). main_row_ptrs: row-granular
        main columns; logup_col_ptrs: what logup_generate wrote (the last four full size). Returns CheckReport.as_dict(); violations are
        a result, not an error."""
        rep = CheckReport()
        _check(lib().bfhip_check_constraints(self._h, component, log_size, self._ptr_array(main_row_ptrs), self._ptr_array(logup_col_ptrs),
                                             self._u32s(lookup24), self._u32s(claimed4), ctypes.byref(rep)))
        return rep.as_dict()

    def relation_summary(self, tables, max_entries=64):
        """bfhip_relation_summary: the lookup tuples that do not cancel over any list of 1..64 tables. tables: (component, log_size,
        main_row_ptrs) each — the row-granular device columns check_constraints takes; a component may be absent or repeated. Returns a
        RelationResult whose lines name table i as "<component name>[i]"; imbalances are a result, not an error."""
        n_main = (8, 8, 4, 9, 13, 13, 11, 11, 11, 11, 11, 11, 7)      # csrc/air.h: n_main_cols; the library reads that many pointers
        for comp, _, ptrs in tables:
            if ptrs is not None and 0 <= comp < 13 and len(ptrs) < n_main[comp]:
                raise BfhipError("relation summary: %s takes %d main columns, got %d" % (COMPONENT_NAMES[comp], n_main[comp], len(ptrs)))
        keep = [None if ptrs is None else self._ptr_array(ptrs) for _, _, ptrs in tables]
        arr = (RelationTable * max(1, len(tables)))()
        for t, ((comp, log_size, _), ptrs) in enumerate(zip(tables, keep)):
            arr[t] = RelationTable(comp, log_size, None if ptrs is None else ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p)))
        names = ["%s[%d]" % (COMPONENT_NAMES[c] if 0 <= c < 13 else "?", t) for t, (c, _, _) in enumerate(tables)]
        return _relation_result(lambda reps, ents, cap: lib().bfhip_relation_summary(self._h, arr, len(tables), reps, ents, cap), max_entries, names)

    def _relation_program_tables(self, tables):
        """(RelationProgramTable array, the ctypes arrays it points into) of a list of (program, log_size, row_shift, col_ptrs[, col_shifts])."""
        keep, arr = [], (RelationProgramTable * len(tables))()
        for t, tab in enumerate(tables):
            program, log_size, row_shift, ptrs = tab[:4]
            shifts = tab[4] if len(tab) > 4 else None
            if len(ptrs) != program.shape["n_cols"] or (shifts is not None and len(shifts) != len(ptrs)):
                raise ValueError("table %d: one column pointer (and shift) per program column" % t)
            pa = self._ptr_array(ptrs) if ptrs else None
            sa = None if shifts is None or not ptrs else self._u32s(shifts)
            keep.append((pa, sa))
            arr[t] = RelationProgramTable(program._h, int(log_size), int(row_shift), None if pa is None else ctypes.cast(pa, ctypes.POINTER(ctypes.c_void_p)),
                                          None if sa is None else ctypes.cast(sa, ctypes.POINTER(ctypes.c_uint32)))
        return arr, keep

    def relation_program_summary(self, tables, max_entries=64, relation_names=None, table_names=None):
        """bfhip_relation_program_summary: the lookup tuples of ANY AIR that do not cancel — relation_summary for RelationPrograms. tables:
        (program, log_size, row_shift, col_ptrs) or (program, log_size, row_shift, col_ptrs, col_shifts) each: one device column per program
        column, the program evaluated once per 2^row_shift cells (row-granular Brainfuck tables: row_shift 4; full-size session columns: 0);
        col_shifts None = every column holds one word per evaluated row. All programs share one list of relations. Returns a RelationResult
        (reports and entries for every relation of the programs); relation_names default to "relation <r>", table_names to "table <t>";
        imbalances are a result, not an error. Refused while a PcsSession is open on the context: run it in front of the session."""
        if not tables:
            raise BfhipError("bfhip_relation_program_summary: 1 to 64 tables, got 0")
        n_rel = tables[0][0].shape["n_relations"]
        arr, keep = self._relation_program_tables(tables)
        rel_names = ["relation %d" % r for r in range(n_rel)] if relation_names is None else list(relation_names)
        if len(rel_names) != n_rel:
            raise ValueError("one name per relation")
        reps = (RelationReport * n_rel)()
        ents = (RelationEntry * (n_rel * max_entries))() if max_entries else None
        _check(lib().bfhip_relation_program_summary(self._h, arr, len(tables), n_rel, reps, ents, max_entries))
        return RelationResult([r.as_dict(rel_names) for r in reps], [ents[k * max_entries + i].as_dict(rel_names) for k in range(n_rel) for i in range(reps[k].n_reported)],
                              ["table %d" % t for t in range(len(tables))] if table_names is None else list(table_names))

    def relation_program_multiplicities(self, tables, relation, target_table, target_entry, out_ptr, max_missing=64, relation_names=None, table_names=None):
        """bfhip_relation_program_multiplicities: fills the multiplicity column of a looked-up table on the device. tables: as for
        relation_program_summary. The target — the table side of the lookup — is the target_entry-th ENTRY of `relation` (program order, from 0)
        in the program of tables[target_table]; its multiplicity operand is ignored. out_ptr: one word per evaluated row of that table (it may
        be the column that operand reads): the lowest row holding a tuple receives the net of every OTHER entry of the relation with that
        tuple, every other row 0. Returns a MultiplicityResult: the counts, and up to max_missing tuples with a non-zero net that no row of
        the target holds (a result, not an error). Refused while a PcsSession is open on the context: run it in front of the session."""
        if not tables:
            raise BfhipError("bfhip_relation_program_multiplicities: 1 to 64 tables, got 0")
        n_rel = tables[0][0].shape["n_relations"]
        arr, keep = self._relation_program_tables(tables)
        rel_names = ["relation %d" % r for r in range(n_rel)] if relation_names is None else list(relation_names)
        if len(rel_names) != n_rel:
            raise ValueError("one name per relation")
        tab_names = ["table %d" % t for t in range(len(tables))] if table_names is None else list(table_names)
        rep = MultiplicityReport()
        miss = (RelationEntry * max_missing)() if max_missing else None
        _check(lib().bfhip_relation_program_multiplicities(self._h, arr, len(tables), n_rel, int(relation), int(target_table), int(target_entry), ctypes.c_void_p(out_ptr),
                                                           ctypes.byref(rep), miss, max_missing))
        return MultiplicityResult(rep.as_dict(rel_names), [miss[i].as_dict(rel_names) for i in range(rep.n_reported)], tab_names, tab_names[rep.target_table])

    def accumulate_quotients(self, log_size, col_ptrs, n_samples, sample_points, sample_values, random_coeff4, out_ptrs, col_shifts=None):
        """QuotientOps::accumulate_quotients for the columns of one LDE size."""
        _check(lib().bfhip_accumulate_quotients(self._h, log_size, self._ptr_array(col_ptrs), None if col_shifts is None else self._u32s(col_shifts), len(col_ptrs),
                                                self._u32s(n_samples), self._u32s(sample_points), self._u32s(sample_values), self._u32s(random_coeff4),
                                                self._ptr_array(out_ptrs)))

    def twiddles(self):
        tw, itw, rl = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32()
        _check(lib().bfhip_twiddles(self._h, ctypes.byref(tw), ctypes.byref(itw), ctypes.byref(rl)))
        return tw.value, itw.value, rl.value


JOB_CANCELLED = -2
POOL_MAX_OUTSTANDING = 4096


class PoolResult(ctypes.Structure):
    """include/bfhip.h `bfhip_pool_result`: one finished job of a pool's queue (88 bytes)."""
    _fields_ = [("ticket", ctypes.c_uint64), ("user_tag", ctypes.c_uint64), ("status", ctypes.c_int32), ("worker", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("log_max_rows", ctypes.c_uint32), ("proof_json", ctypes.c_void_p), ("proof_len", ctypes.c_size_t), ("error", ctypes.c_void_p),
                ("seconds_queued", ctypes.c_double), ("seconds_proving", ctypes.c_double), ("reserved", ctypes.c_uint64 * 2)]


class JobResult:
    """What Pool.wait() returns: ticket, tag, status (0 ok, -1 failed, JOB_CANCELLED, TRACE_REJECTED), worker, flags (Context.last_proof_flags bits of that
    proof), log_max_rows, proof (bytes, None unless ok), error (str, None when ok), seconds_queued, seconds_proving."""

    def __init__(self, r):
        self.ticket, self.tag, self.status, self.worker, self.flags = int(r.ticket), int(r.user_tag), int(r.status), int(r.worker), int(r.flags)
        self.log_max_rows, self.seconds_queued, self.seconds_proving = int(r.log_max_rows), float(r.seconds_queued), float(r.seconds_proving)
        self.proof = ctypes.string_at(r.proof_json, r.proof_len) if r.proof_json else None
        self.error = ctypes.string_at(r.error).decode() if r.error else None
        if r.proof_json:
            lib().bfhip_free_host(ctypes.c_void_p(r.proof_json))
        if r.error:
            lib().bfhip_free_host(ctypes.c_void_p(r.error))

    ok = property(lambda self: self.status == 0)
    cancelled = property(lambda self: self.status == JOB_CANCELLED)
    rejected = property(lambda self: self.status == TRACE_REJECTED)      # Pool.set_preflight: bad input, not an internal failure
    preflight = property(lambda self: bool(self.flags & 64))
    shared_preprocessed = property(lambda self: bool(self.flags & 4))

    def __repr__(self):
        return "JobResult(ticket=%d, tag=%d, status=%d, worker=%d, %s)" % (self.ticket, self.tag, self.status, self.worker,
                                                                             "%d proof bytes" % len(self.proof) if self.ok else self.error)


class Pool:
    """bfhip_pool_create: `n_in_flight` sub-contexts on one GPU behind ONE caller thread — prove_batch() hands the library a batch of resident
    traces and returns when all are proved, n_in_flight at a time on the library's own worker threads; submit_trace / submit_program /
    submit_registers + wait() / as_completed() use the same workers as a queue (results as they complete; not while a batch runs). The sub-contexts share one twiddle
    tree and (preprocessed=1, default) one preprocessed commitment per batch; 0 = every proof recommits it like the reference
    (mod.rs:495-500), 2 = kept across batches."""

    def __init__(self, device_id=0, n_in_flight=2, max_log_domain=24, preprocessed=1):
        self._h = ctypes.c_void_p()
        _check(lib().bfhip_pool_create(device_id, n_in_flight, max_log_domain, ctypes.byref(self._h)))
        self.n_in_flight, self.max_log_domain = n_in_flight, max_log_domain
        self._subs = {}
        self._borrowed = {}                       # ticket -> the arrays / trace the library borrows until that result is taken
        if preprocessed != 1:
            self.set_preprocessed(preprocessed)
        if _default_conventions != (0, 0, 0, 0):
            self.set_conventions(*_default_conventions)

    def close(self):
        if self._h:
            for c in self._subs.values():
                c._h = ctypes.c_void_p()          # borrowed handles die with the pool
            lib().bfhip_pool_destroy(self._h)             # running jobs finish before this returns: the borrowed arrays outlive them
            self._h = ctypes.c_void_p()
            self._borrowed.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the queue: submit returns a ticket at once, wait() hands out results in completion order -------------------------------------
    def _submitted(self, rc, ticket, keep):
        _check(rc)
        self._borrowed[ticket.value] = keep
        return ticket.value

    def submit_trace(self, trace, log_max_rows=24, tag=0):
        """bfhip_pool_submit_trace: a resident trace of ANY context on the pool's device. The pool keeps a reference to it until its result is taken."""
        t = ctypes.c_uint64()
        return self._submitted(lib().bfhip_pool_submit_trace(self._h, trace._h, log_max_rows, ctypes.c_uint64(tag), ctypes.byref(t)), t, trace)

    def submit_program(self, code, input_bytes=b"", log_max_rows=24, tag=0):
        """bfhip_pool_submit_brainfuck: program text and input are copied; VM run, table build and upload happen inside the worker."""
        t = ctypes.c_uint64()
        return self._submitted(lib().bfhip_pool_submit_brainfuck(self._h, code.encode(), bytes(input_bytes), ctypes.c_size_t(len(input_bytes)), log_max_rows,
                                                                 ctypes.c_uint64(tag), ctypes.byref(t)), t, None)

    def submit_registers(self, rows, code_words, log_max_rows=24, tag=0):
        """bfhip_pool_submit_registers: an executed machine's register rows (n x 7 u32) and program words — what prove_registers takes, as a job.
        The rows are borrowed by the library: the pool holds the array until the result is taken."""
        tr = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 7)
        code = np.ascontiguousarray(code_words, dtype=np.uint32)
        t = ctypes.c_uint64()
        return self._submitted(lib().bfhip_pool_submit_registers(self._h, tr.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(tr.shape[0]), code.ctypes.data_as(ctypes.c_void_p),
                                                                 ctypes.c_size_t(code.size), log_max_rows, ctypes.c_uint64(tag), ctypes.byref(t)), t, tr)

    def wait(self, timeout_s=None):
        """bfhip_pool_wait: the next finished job as a JobResult; None when nothing is outstanding; TimeoutError when timeout_s (None = no limit,
        0 = poll) ran out with jobs outstanding."""
        ms = 0xFFFFFFFF if timeout_s is None else min(0xFFFFFFFE, max(0, int(round(timeout_s * 1000))))
        r = PoolResult()
        rc = lib().bfhip_pool_wait(self._h, ctypes.c_uint32(ms), ctypes.byref(r))
        if rc == 0:
            self._borrowed.pop(int(r.ticket), None)
            return JobResult(r)
        if rc == 1:
            raise TimeoutError("no job of the pool finished within %s s" % timeout_s)
        if rc == 2:
            return None
        raise BfhipError(lib().bfhip_last_error().decode())

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
        _check(lib().bfhip_pool_outstanding(self._h, ctypes.byref(q), ctypes.byref(r), ctypes.byref(f)))
        return {"queued": q.value, "running": r.value, "finished": f.value}

    def cancel(self, ticket):
        """bfhip_pool_cancel: True = the job was still queued (its result arrives with status JOB_CANCELLED), False = already running or finished."""
        rc = lib().bfhip_pool_cancel(self._h, ctypes.c_uint64(ticket))
        if rc < 0:
            raise BfhipError(lib().bfhip_last_error().decode())
        return rc == 0

    def ctx(self, i=0):
        """Sub-context i as a (borrowed) Context: for Trace(...) on the pool's device between batches, per-context settings, memory()."""
        if i not in self._subs:
            h = ctypes.c_void_p()
            _check(lib().bfhip_pool_ctx(self._h, i, ctypes.byref(h)))
            c = Context.__new__(Context)
            c._h, c.max_log_domain = h, self.max_log_domain
            c.close = lambda: None                # owned by the pool
            self._subs[i] = c
        return self._subs[i]

    def set_conventions(self, merkle_node_hash=0, mix_u64=0, logup_mask_order=0, merkle_channel=0):
        cv = Conventions(merkle_node_hash, mix_u64, logup_mask_order, merkle_channel)
        _check(lib().bfhip_pool_set_conventions(self._h, ctypes.byref(cv)))

    def set_preprocessed(self, mode):
        _check(lib().bfhip_pool_set_preprocessed(self._h, int(mode)))

    def set_preflight(self, on=True):
        """bfhip_pool_set_preflight: Context.set_preflight on every sub-context. A job whose trace is rejected comes back with
        status TRACE_REJECTED (JobResult.rejected) and the rejection lines as its error; refused while jobs are outstanding."""
        _check(lib().bfhip_pool_set_preflight(self._h, 1 if on else 0))

    def set_pcs_config(self, pcs_config=None):
        """bfhip_pool_set_pcs_config: the PcsConfig of every sub-context and of the shared preprocessed tree's builder (None = the default)."""
        _check(lib().bfhip_pool_set_pcs_config(self._h, _pcs_ref(pcs_config)))

    def _outputs(self, n, want_json):
        js = (ctypes.c_void_p * n)() if want_json else None
        return js, (ctypes.c_size_t * n)(), (ctypes.c_int32 * n)(), (ctypes.c_double * (n + 1))()

    def _collect(self, rc, n, js, lens, st, sec, want_json):
        proofs = []
        for i in range(n):
            if want_json and js[i]:
                proofs.append(ctypes.string_at(js[i], lens[i]))
                lib().bfhip_free_host(ctypes.c_void_p(js[i]))
            else:
                proofs.append(None)
        info = {"statuses": [int(v) for v in st], "seconds": [float(v) for v in sec[:n]], "batch_seconds": float(sec[n])}
        if rc != 0:
            err = BfhipError(lib().bfhip_last_error().decode())
            err.proofs, err.info = proofs, info
            raise err
        return proofs, info

    def prove_batch(self, traces, log_max_rows=24, want_json=True):
        """bfhip_prove_batch: returns (proofs, info) — proofs[i] = JSON bytes of traces[i]'s proof; info = per-proof seconds + batch_seconds.
        Raises BfhipError when a proof failed (its .proofs / .info hold what the rest of the batch produced)."""
        n = len(traces)
        arr = (ctypes.c_void_p * max(n, 1))(*[t._h for t in traces])
        js, lens, st, sec = self._outputs(n, want_json)
        rc = lib().bfhip_prove_batch(self._h, arr, n, log_max_rows, js, lens, st, sec)
        return self._collect(rc, n, js, lens, st, sec, want_json)

    def prove_batch_brainfuck(self, programs, log_max_rows=24, want_json=True):
        """bfhip_prove_batch_brainfuck: programs = [(code, input_bytes), ...]; VM, table build and upload run inside the workers."""
        n = len(programs)
        codes = (ctypes.c_char_p * max(n, 1))(*[c.encode() for c, _ in programs])
        bufs = [ctypes.create_string_buffer(bytes(i), max(len(i), 1)) for _, i in programs]
        inputs = (ctypes.c_void_p * max(n, 1))(*[ctypes.addressof(b) for b in bufs])
        nin = (ctypes.c_size_t * max(n, 1))(*[len(i) for _, i in programs])
        js, lens, st, sec = self._outputs(n, want_json)
        rc = lib().bfhip_prove_batch_brainfuck(self._h, codes, inputs, nin, n, log_max_rows, js, lens, st, sec)
        return self._collect(rc, n, js, lens, st, sec, want_json)


PHASES = ("preprocessed", "tables_host", "main_trace", "interaction", "composition", "oods", "quotients", "fri", "decommit", "total")


def prove_brainfuck(code, input_bytes=b"", ctx=None, log_max_rows=24, with_transcript=False, with_timings=False, pcs_config=None):
    """prove_brainfuck (mod.rs:471): returns the proof as serde_json bytes of BrainfuckProof. GPU only. With ctx.set_preflight() a trace
    that cannot be proved raises TraceRejected (so do prove_registers and Trace.prove).
    pcs_config: a PcsConfig for this proof (None: the context's own, PcsConfig::default() for a new context). A context passed in keeps it
    afterwards."""
    own = ctx is None
    if own:
        blowup = 1 if pcs_config is None else pcs_config.log_blowup_factor
        ctx = Context(0, max_log_domain=log_max_rows + blowup + 1)
    try:
        if pcs_config is not None:
            ctx.set_pcs_config(pcs_config)
        js, n, tr = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_void_p()
        times = (ctypes.c_double * 10)()
        _check_proof(lib().bfhip_prove_brainfuck(ctx._h, code.encode(), input_bytes, ctypes.c_size_t(len(input_bytes)), log_max_rows,
                                                 ctypes.byref(js), ctypes.byref(n), ctypes.byref(tr) if with_transcript else None, times), ctx)
        proof = ctypes.string_at(js, n.value)
        lib().bfhip_free_host(js)
        out = [proof]
        if with_transcript:
            t = ctypes.string_at(tr).decode()
            lib().bfhip_free_host(tr)
            out.append(dict(line.split(":") for line in t.strip().split("\n")))
        if with_timings:
            out.append(dict(zip(PHASES, list(times))))
        return out[0] if len(out) == 1 else tuple(out)
    finally:
        if own:
            ctx.close()


def prove_registers(rows, code_words, ctx=None, log_max_rows=24, with_transcript=False, with_timings=False):
    """bfhip_prove_registers — prove_brainfuck(&Machine) (mod.rs:471-473) in one call: an executed machine's register rows (n x 7 u32: clk, ip,
    ci, ni, mp, mv, mvi) and program words in, the proof's serde_json bytes out. Same bytes as Trace.from_registers(...).prove(...); no
    resident trace. A non-canonical register raises with its (row, register)."""
    own = ctx is None
    if own:
        ctx = Context(0, max_log_domain=log_max_rows + 2)
    try:
        tr = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 7)
        code = np.ascontiguousarray(code_words, dtype=np.uint32)
        js, n, t = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_void_p()
        times = (ctypes.c_double * 10)()
        _check_proof(lib().bfhip_prove_registers(ctx._h, tr.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(tr.shape[0]), code.ctypes.data_as(ctypes.c_void_p),
                                                 ctypes.c_size_t(code.size), log_max_rows, ctypes.byref(js), ctypes.byref(n),
                                                 ctypes.byref(t) if with_transcript else None, times), ctx)
        proof = ctypes.string_at(js, n.value)
        lib().bfhip_free_host(js)
        out = [proof]
        if with_transcript:
            text = ctypes.string_at(t).decode()
            lib().bfhip_free_host(t)
            out.append(dict(line.split(":") for line in text.strip().split("\n")))
        if with_timings:
            out.append(dict(zip(PHASES, list(times))))
        return out[0] if len(out) == 1 else tuple(out)
    finally:
        if own:
            ctx.close()


def verify_brainfuck(proof_json: bytes, log_max_rows=24, conventions=None, pcs_config=None):
    """verify_brainfuck (mod.rs:738): returns (ok, reason). Host only — no GPU needed, like the reference's verifier.
    conventions: (merkle_node_hash, mix_u64, logup_mask_order) the proof was produced under; None = the defaults.
    pcs_config: the PcsConfig the proof was made with; None = PcsConfig::default(). An invalid config raises BfhipError."""
    err = ctypes.create_string_buffer(512)
    cv = ctypes.byref(Conventions(*(_default_conventions if conventions is None else conventions)))
    rc = lib().bfhip_verify_brainfuck_pcs(proof_json, ctypes.c_size_t(len(proof_json)), log_max_rows, cv, _pcs_ref(pcs_config), err,
                                          ctypes.c_size_t(512))
    if rc < 0:
        raise BfhipError(lib().bfhip_last_error().decode())
    return rc == 0, err.value.decode()


def host_compile(code):
    """bfhip_host_compile (compiler.rs:17-37): the program words, jump targets included. Host only."""
    out = np.zeros(2 * len(code) + 4, dtype=np.uint32)
    n = ctypes.c_size_t()
    _check(lib().bfhip_host_compile(code.encode(), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.size), ctypes.byref(n)))
    return out[: n.value].copy()


def host_run(code, input_bytes=b"", ram_size=0):
    """bfhip_host_run_ram (machine.rs:141-238): (output bytes, register trace as an (n, 7) u32 array: clk, ip, ci, ni, mp, mv, mvi). Host only."""
    n_out, n_rows = ctypes.c_size_t(), ctypes.c_size_t()
    args = (code.encode(), input_bytes, ctypes.c_size_t(len(input_bytes)), ctypes.c_size_t(ram_size))
    _check(lib().bfhip_host_run_ram(*args, None, ctypes.c_size_t(0), ctypes.byref(n_out), None, ctypes.c_size_t(0), ctypes.byref(n_rows)))
    out = (ctypes.c_ubyte * max(1, n_out.value))()
    rows = np.zeros((n_rows.value, 7), dtype=np.uint32)
    _check(lib().bfhip_host_run_ram(*args, out, ctypes.c_size_t(n_out.value), ctypes.byref(n_out), rows.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.c_size_t(rows.shape[0]), ctypes.byref(n_rows)))
    return bytes(out[: n_out.value]), rows


class Trace:
    """Prover input resident in HBM (bfhip_trace_create): VM trace -> 13 component tables -> row-granular device columns."""

    def __init__(self, ctx, code, input_bytes=b"", ram_size=0):
        """ram_size: Machine RAM cells (MachineBuilder::with_ram_size, machine.rs:56-60); 0 = the default 30000."""
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        ls = (ctypes.c_uint32 * 13)()
        steps, mc, ic = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().bfhip_trace_create_ram(ctx._h, code.encode(), input_bytes, ctypes.c_size_t(len(input_bytes)), ctypes.c_size_t(ram_size),
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
        _check(lib().bfhip_trace_create_from_registers(ctx._h, tr.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(tr.shape[0]), code.ctypes.data_as(ctypes.c_void_p),
                                                       ctypes.c_size_t(code.size), ctypes.byref(self._h), ls, ctypes.byref(mc), ctypes.byref(ic)))
        self.log_sizes = list(ls)
        self.n_steps, self.main_cells, self.interaction_cells = tr.shape[0], mc.value, ic.value
        return self

    @property
    def cells(self):
        return self.main_cells + self.interaction_cells

    def prove(self, log_max_rows=24, want_json=True):
        js, n = ctypes.c_void_p(), ctypes.c_size_t()
        times = (ctypes.c_double * 10)()
        _check_proof(lib().bfhip_prove_trace(self.ctx._h, self._h, log_max_rows, ctypes.byref(js) if want_json else None, ctypes.byref(n), None, times), self.ctx)
        proof = None
        if want_json:
            proof = ctypes.string_at(js, n.value)
            lib().bfhip_free_host(js)
        return proof, dict(zip(PHASES, list(times)))

    def check(self, lookup24=None):
        """bfhip_trace_check: the 13 AIRs asserted on this trace (logUp columns generated on the GPU), as a CheckResult. lookup24: (z, alpha)
        of Memory, Instruction, Processor; None = default_check_lookup(). A trace that is not a valid execution gives ok = False and the
        failing component, constraint and row — where a proof would only say ConstraintsNotSatisfied."""
        reps = (CheckReport * 13)()
        total = (ctypes.c_uint32 * 4)()
        n_bad = ctypes.c_int32()
        _check(lib().bfhip_trace_check(self.ctx._h, self._h, None if lookup24 is None else Context._u32s(lookup24), reps, total, ctypes.byref(n_bad)))
        res = CheckResult(r.as_dict() for r in reps)
        res.logup_total, res.n_bad_components = tuple(int(v) for v in total), n_bad.value
        return res

    def relations(self, max_entries=64):
        """bfhip_trace_relations: the lookup tuples of this trace's 13 tables that do not cancel (stwo's relation tracker), as a
        RelationResult: .balanced, .reports (3 dicts), .entries (at most max_entries per relation), .lines(). Names what a non-zero
        check().logup_total cannot: which tuple is yielded and never used, or used and never yielded, and by which table row."""
        return _relation_result(lambda reps, ents, cap: lib().bfhip_trace_relations(self.ctx._h, self._h, reps, ents, cap), max_entries)

    def column(self, component, column):
        n = ctypes.c_size_t()
        _check(lib().bfhip_trace_column(self.ctx._h, self._h, component, column, None, ctypes.c_size_t(0), ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.uint32)
        _check(lib().bfhip_trace_column(self.ctx._h, self._h, component, column, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.size), ctypes.byref(n)))
        return out

    def close(self):
        if self._h:
            lib().bfhip_trace_destroy(self.ctx._h, self._h)
            self._h = ctypes.c_void_p()


# ---- commitment-scheme session (include/bfhip.h "Commitment-scheme session"): commit and open any AIR's columns -----------------------
PCS_MAX_SAMPLES_PER_COLUMN, PCS_MAX_POINTS, PCS_MAX_COLUMNS, PCS_MAX_TREES = 2, 64, 4096, 64


def _conv_ref(conventions):
    return ctypes.byref(Conventions(*(_default_conventions if conventions is None else conventions)))


def _flat_samples(samples):
    """samples[tree][column] = list of point indices -> (n_samples per column, the indices flat), both as u32 arrays."""
    counts = [len(col) for tree in samples for col in tree]
    idx = [int(i) for tree in samples for col in tree for i in col]
    return Context._u32s(counts), Context._u32s(idx) if idx else None


def _flat_points(points):
    flat = [int(w) for p in points for w in p]
    if len(flat) != 8 * len(points):
        raise ValueError("a point is 8 words: x (4) then y (4)")
    return Context._u32s(flat) if flat else None


def circle_point_offset(point8, log_size, offset):
    """bfhip_circle_point_offset: point + offset * CanonicCoset(log_size).step() — the mask point of a column of 2^log_size rows at a row
    offset (offset -1: the previous row). Host only."""
    out = (ctypes.c_uint32 * 8)()
    _check(lib().bfhip_circle_point_offset(Context._u32s(point8), int(log_size), int(offset), out))
    return [int(v) for v in out]


def brainfuck_composition_at_point(log_sizes, claimed_sums, log_max_rows, lookup24, point8, sampled, random_coeff4, conventions=None):
    """bfhip_brainfuck_composition_at_point: the snapshot AIR's composition polynomial at a point from the sampled mask values — what a
    verifier assembled from PcsVerifier compares with the composition polynomial's own sampled value. sampled[tree][column] = list of
    QM31 (4 words each) for the preprocessed, main-trace and interaction trees. Host only."""
    n_cols = Context._u32s([len(t) for t in sampled[:3]])
    counts = Context._u32s([len(c) for t in sampled[:3] for c in t])
    flat = Context._u32s([w for t in sampled[:3] for c in t for q in c for w in q])
    out = (ctypes.c_uint32 * 4)()
    _check(lib().bfhip_brainfuck_composition_at_point(Context._u32s(log_sizes), Context._u32s([w for q in claimed_sums for w in q]), int(log_max_rows),
                                                      Context._u32s(lookup24), Context._u32s(point8), n_cols, counts, flat, Context._u32s(random_coeff4),
                                                      _conv_ref(conventions), out))
    return [int(v) for v in out]


class Channel:
    """bfhip_channel: Blake2sChannel::default() / Poseidon252Channel::default() (by conventions[3]) — what stwo passes as `channel` to
    commit, prove_values and verify_values. Host only. conventions: (merkle_node_hash, mix_u64, logup_mask_order, merkle_channel); None =
    the mirror's defaults."""

    def __init__(self, conventions=None):
        self._h = ctypes.c_void_p()
        self.conventions = tuple(_default_conventions if conventions is None else conventions)
        _check(lib().bfhip_channel_create(_conv_ref(self.conventions), ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib().bfhip_channel_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def mix_root(self, hash32):
        hash32 = bytes(hash32)
        if len(hash32) != 32:
            raise ValueError("a root is 32 bytes")
        _check(lib().bfhip_channel_mix_root(self._h, hash32))

    def mix_u64(self, value):
        _check(lib().bfhip_channel_mix_u64(self._h, ctypes.c_uint64(int(value))))

    def mix_felts(self, felts):
        """felts: QM31 values, 4 canonical words each."""
        flat = [int(w) for q in felts for w in q]
        if len(flat) != 4 * len(felts):
            raise ValueError("a secure felt is 4 words")
        _check(lib().bfhip_channel_mix_felts(self._h, Context._u32s(flat) if flat else None, ctypes.c_size_t(len(felts))))

    def draw_felts(self, n=1):
        """stwo's draw_felts(n): n QM31 values (lists of 4 words). n = 1 is draw_felt, n = 2 a lookup element's (z, alpha)."""
        out = (ctypes.c_uint32 * (4 * max(1, n)))()
        _check(lib().bfhip_channel_draw_felts(self._h, ctypes.c_size_t(n), out))
        return [[int(out[4 * i + k]) for k in range(4)] for i in range(n)]

    def draw_felt(self):
        return self.draw_felts(1)[0]

    def draw_point(self):
        """CirclePoint::get_random_point: 8 words, x then y."""
        out = (ctypes.c_uint32 * 8)()
        _check(lib().bfhip_channel_draw_point(self._h, out))
        return [int(v) for v in out]

    def state(self):
        """(digest bytes, n_sent)"""
        d, n = (ctypes.c_uint8 * 32)(), ctypes.c_uint32()
        _check(lib().bfhip_channel_state(self._h, d, ctypes.byref(n)))
        return bytes(d), n.value

    def trailing_zeros(self):
        out = ctypes.c_uint32()
        _check(lib().bfhip_channel_trailing_zeros(self._h, ctypes.byref(out)))
        return out.value


class PcsSession:
    """bfhip_pcs: stwo's CommitmentSchemeProver on one Context — commit trees of arbitrary device columns, then open them at arbitrary
    points through the fused path of a Brainfuck proof. One open session per context; while it is open the context refuses its proving,
    checking and trace-building entries (include/bfhip.h lists them). close() (or the context manager) ends it."""

    def __init__(self, ctx):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        _check(lib().bfhip_pcs_create(ctx._h, ctypes.byref(self._h)))
        self.roots, self.log_sizes = [], []

    def close(self):
        if self._h:
            lib().bfhip_pcs_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def commit(self, channel, col_ptrs, log_sizes, form=0):
        """bfhip_pcs_commit: col_ptrs = device pointers, column k of 2^log_sizes[k] words. form 0 = evaluations (bit-reversed circle domain),
        1 = coefficients. Mixes the root into `channel` and returns it (32 bytes)."""
        if len(col_ptrs) != len(log_sizes):
            raise ValueError("one log size per column")
        root = (ctypes.c_uint8 * 32)()
        _check(lib().bfhip_pcs_commit(self._h, channel._h, Context._ptr_array(col_ptrs), Context._u32s(log_sizes), len(col_ptrs), int(form), root))
        self.roots.append(bytes(root))
        self.log_sizes.append([int(v) for v in log_sizes])
        return bytes(root)

    def tree_columns(self, tree):
        """bfhip_pcs_tree_columns: (coefficient pointers, LDE pointers) of a committed tree's columns, valid until close()."""
        n = ctypes.c_uint32()
        _check(lib().bfhip_pcs_tree_columns(self._h, int(tree), None, None, 0, ctypes.byref(n)))
        co, ev = (ctypes.c_void_p * max(1, n.value))(), (ctypes.c_void_p * max(1, n.value))()
        _check(lib().bfhip_pcs_tree_columns(self._h, int(tree), co, ev, n.value, ctypes.byref(n)))
        return [co[k] for k in range(n.value)], [ev[k] for k in range(n.value)]

    def prove_values(self, channel, points, samples, with_sampled=False):
        """bfhip_pcs_prove_values: points = list of 8-word points; samples[tree][column] = indices into points, in the order the sampled
        values are to appear. Returns the CommitmentSchemeProof JSON bytes (and, with_sampled, the sampled values flat as 4-word lists)."""
        counts, idx = _flat_samples(samples)
        n_samples = sum(len(col) for tree in samples for col in tree)
        if [len(t) for t in samples] != [len(t) for t in self.log_sizes]:
            raise ValueError("samples must list every column of every committed tree")
        out = (ctypes.c_uint32 * (4 * max(1, n_samples)))() if with_sampled else None
        js, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().bfhip_pcs_prove_values(self._h, channel._h, _flat_points(points), len(points), counts, idx, out, ctypes.byref(js), ctypes.byref(n)))
        proof = ctypes.string_at(js, n.value)
        lib().bfhip_free_host(js)
        if with_sampled:
            return proof, [[int(out[4 * i + k]) for k in range(4)] for i in range(n_samples)]
        return proof


class PcsVerifier:
    """bfhip_pcs_verifier: stwo's CommitmentSchemeVerifier. Host only. conventions / pcs_config: what the proof was made under."""

    def __init__(self, conventions=None, pcs_config=None):
        self._h = ctypes.c_void_p()
        _check(lib().bfhip_pcs_verifier_create(_conv_ref(conventions), _pcs_ref(pcs_config), ctypes.byref(self._h)))
        self.n_cols = []

    def close(self):
        if self._h:
            lib().bfhip_pcs_verifier_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def commit(self, channel, root, log_sizes):
        """CommitmentSchemeVerifier::commit: the trace-domain log sizes of the tree's columns; mixes the root into `channel`."""
        root = bytes(root)
        if len(root) != 32:
            raise ValueError("a root is 32 bytes")
        _check(lib().bfhip_pcs_verifier_commit(self._h, channel._h, root, Context._u32s(log_sizes), len(log_sizes)))
        self.n_cols.append(len(log_sizes))

    def verify_values(self, channel, points, samples, proof_json):
        """(ok, reason): the description of PcsSession.prove_values; reason = the VerificationError name of a rejection."""
        if [len(t) for t in samples] != self.n_cols:
            raise ValueError("samples must list every column of every committed tree")
        counts, idx = _flat_samples(samples)
        err = ctypes.create_string_buffer(512)
        rc = lib().bfhip_pcs_verifier_verify_values(self._h, channel._h, _flat_points(points), len(points), counts, idx, proof_json,
                                                    ctypes.c_size_t(len(proof_json)), err, ctypes.c_size_t(512))
        if rc < 0:
            raise BfhipError(lib().bfhip_last_error().decode())
        return rc == 0, err.value.decode()


# ---- constraint programs (include/bfhip.h "Constraint programs") ------------------------------------------------------------------------
AIR_OPS = ("M_COL", "M_CONST", "M_ADD", "M_SUB", "M_MUL", "M_NEG", "Q_COL", "Q_PARAM", "Q_FROM_M", "Q_ADD", "Q_SUB", "Q_MUL", "Q_MULM", "C_BASE", "C_EXT")
(AIR_M_COL, AIR_M_CONST, AIR_M_ADD, AIR_M_SUB, AIR_M_MUL, AIR_M_NEG, AIR_Q_COL, AIR_Q_PARAM, AIR_Q_FROM_M, AIR_Q_ADD, AIR_Q_SUB, AIR_Q_MUL, AIR_Q_MULM,
 AIR_C_BASE, AIR_C_EXT) = range(15)
AIR_MAX_M_REGS, AIR_MAX_Q_REGS, AIR_MAX_INSTRUCTIONS, AIR_MAX_COLUMNS, AIR_MAX_PARAMS, AIR_MAX_CONSTRAINTS, AIR_MAX_OFFSET = 96, 24, 4096, 256, 64, 64, 16


class AirProgram:
    """bfhip_air: a validated constraint program. code = the bytecode, four u32 words {op, dst, a, b} per instruction (what bindings pass;
    AirBuilder writes it from expressions). Host only: creating, shape, mask and eval_at_point need no GPU; Context.air_eval_domain runs it
    on the constraint domain. A refused program raises BfhipError naming the instruction index and the rule."""

    def __init__(self, code, n_cols, n_params):
        self.code = [int(w) & 0xFFFFFFFF for w in code]
        self._h = ctypes.c_void_p()
        arr = (ctypes.c_uint32 * max(1, len(self.code)))(*self.code)
        _check(lib().bfhip_air_create(arr, ctypes.c_size_t(len(self.code)), int(n_cols), int(n_params), ctypes.byref(self._h)))
        out = (ctypes.c_uint32 * 8)()
        _check(lib().bfhip_air_shape(self._h, out))
        signed = lambda v: v - (1 << 32) if v >= 1 << 31 else v
        self.shape = {"n_cols": out[0], "n_params": out[1], "n_constraints": out[2], "n_instr": out[3], "m_regs": out[4], "q_regs": out[5],
                      "min_offset": signed(out[6]), "max_offset": signed(out[7])}

    def close(self):
        if self._h:
            lib().bfhip_air_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def mask(self):
        """bfhip_air_mask: [(column, offset)] — by column, within a column by first use. The order of a column's samples for
        PcsSession.prove_values and of eval_at_point's mask values."""
        n = ctypes.c_uint32()
        _check(lib().bfhip_air_mask(self._h, None, None, 0, ctypes.byref(n)))
        cols, offs = (ctypes.c_uint32 * max(1, n.value))(), (ctypes.c_int32 * max(1, n.value))()
        _check(lib().bfhip_air_mask(self._h, cols, offs, n.value, ctypes.byref(n)))
        return [(int(cols[i]), int(offs[i])) for i in range(n.value)]

    def source(self):
        """bfhip_air_source: the HIP source of the kernel Context.air_compile builds from this program (host only; the same program gives
        the same text). With -DBFHIP_AIR_GEN_HOST it compiles as plain C++."""
        n = ctypes.c_size_t()
        _check(lib().bfhip_air_source(self._h, None, ctypes.c_size_t(0), ctypes.byref(n)))
        buf = ctypes.create_string_buffer(max(1, n.value))
        _check(lib().bfhip_air_source(self._h, buf, ctypes.c_size_t(n.value), ctypes.byref(n)))
        return buf.raw[: n.value].decode()

    def eval_at_point(self, log_size, point8, mask_values, params, coeffs):
        """bfhip_air_eval_at_point: (sum_j coeffs[j] C_j) / coset_vanishing at a point, from the sampled mask values (QM31 each, mask order)."""
        flat = lambda qs: Context._u32s([w for q in qs for w in q]) if len(qs) else None
        for qs in (mask_values, params, coeffs):
            if any(len(q) != 4 for q in qs):
                raise ValueError("a QM31 value is 4 words")
        out = (ctypes.c_uint32 * 4)()
        _check(lib().bfhip_air_eval_at_point(self._h, int(log_size), Context._u32s(point8), flat(mask_values), len(mask_values), flat(params), len(params),
                                             flat(coeffs), len(coeffs), out))
        return [int(v) for v in out]


class CompiledAir:
    """bfhip_air_kernel: an AirProgram compiled to its own kernel by Context.air_compile. Pass it to Context.air_eval_domain of the context
    that compiled it. .shape is the program's; info() the kernel's resources. A context that is closed first unloads the kernel: the object can then
    only be closed."""

    INFO = ("vgprs", "sgprs", "scratch_bytes", "lds_bytes", "code_object_bytes", "source_bytes", "compile_us", "from_cache")

    def __init__(self, ctx, program):
        self._h = ctypes.c_void_p()
        self.shape = dict(program.shape)
        _check(lib().bfhip_air_compile(ctx._h, program._h, ctypes.byref(self._h)))

    def info(self):
        """bfhip_air_kernel_info as a dict; sgprs is None when the code object does not state it."""
        out = (ctypes.c_uint32 * 8)()
        _check(lib().bfhip_air_kernel_info(self._h, out))
        d = dict(zip(self.INFO, (int(v) for v in out)))
        d["sgprs"] = None if d["sgprs"] == 0xFFFFFFFF else d["sgprs"]
        d["from_cache"] = bool(d["from_cache"])
        return d

    def close(self):
        if self._h:
            lib().bfhip_air_kernel_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AirCheckReport(ctypes.Structure):
    """include/bfhip.h `bfhip_air_check_report` (1088 bytes): an AirProgram asserted on its trace domain (Context.air_check)."""
    _fields_ = [("log_size", ctypes.c_uint32), ("n_constraints", ctypes.c_uint32), ("n_bad_cells", ctypes.c_uint64), ("first_bad_cell", ctypes.c_uint64),
                ("first_bad_constraint", ctypes.c_int32), ("reserved0", ctypes.c_uint32), ("first_bad_value", ctypes.c_uint32 * 4),
                ("bad_per_constraint", ctypes.c_uint64 * 64), ("first_cell_per_constraint", ctypes.c_uint64 * 64), ("reserved", ctypes.c_uint64 * 2)]

    def as_dict(self):
        """Named fields; the per-constraint lists have n_constraints entries. first_bad_cell and first_cell_per_constraint[j] are None where
        nothing fails (first_bad_constraint is -1 then)."""
        cell = lambda v: None if v == NO_CELL else int(v)
        k = min(int(self.n_constraints), 64)
        return {"log_size": int(self.log_size), "n_constraints": int(self.n_constraints), "ok": self.n_bad_cells == 0, "n_bad_cells": int(self.n_bad_cells),
                "first_bad_cell": cell(self.first_bad_cell), "first_bad_constraint": int(self.first_bad_constraint),
                "first_bad_value": [int(v) for v in self.first_bad_value], "bad_per_constraint": [int(v) for v in self.bad_per_constraint[:k]],
                "first_cell_per_constraint": [cell(v) for v in self.first_cell_per_constraint[:k]]}


def format_air_check(report):
    """bfhip_format_air_check of an AirCheckReport (host only, no GPU): "air check: ok", or the headline and one line per failing constraint."""
    need = ctypes.c_size_t()
    rc = lib().bfhip_format_air_check(ctypes.byref(report), None, ctypes.c_size_t(0), ctypes.byref(need))
    if rc not in (0, -2):
        raise BfhipError(lib().bfhip_last_error().decode())
    buf = ctypes.create_string_buffer(need.value)
    _check(lib().bfhip_format_air_check(ctypes.byref(report), buf, ctypes.c_size_t(need.value), None))
    return buf.value.decode()


LOGUP_FRAC, LOGUP_END_COL, LOGUP_MAX_COLUMNS, LOGUP_MAX_FRACTIONS = 15, 16, 8, 32


class LogupProgram:
    """bfhip_logup: a validated fraction program (include/bfhip.h "Fraction programs") — a constraint program's bytecode without constraints,
    with FRAC (add q[a] / q[b] to the open logUp column) and END_COL. Host only to create; Context.logup_program_generate runs it on the
    trace domain. A refused program raises BfhipError naming the instruction index and the rule."""

    def __init__(self, code, n_cols, n_params):
        self.code = [int(w) & 0xFFFFFFFF for w in code]
        self._h = ctypes.c_void_p()
        arr = (ctypes.c_uint32 * max(1, len(self.code)))(*self.code)
        _check(lib().bfhip_logup_create(arr, ctypes.c_size_t(len(self.code)), int(n_cols), int(n_params), ctypes.byref(self._h)))
        out = (ctypes.c_uint32 * 8)()
        _check(lib().bfhip_logup_shape(self._h, out))
        self.shape = {"n_cols": out[0], "n_params": out[1], "n_logup_cols": out[2], "n_fractions": out[3], "n_instr": out[4], "m_regs": out[5], "q_regs": out[6]}

    def close(self):
        if self._h:
            lib().bfhip_logup_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


REL_WORD, REL_ENTRY, RELATION_PROGRAM_MAX_RELATIONS, RELATION_PROGRAM_MAX_WORDS, RELATION_PROGRAM_MAX_ENTRIES = 17, 18, 16, 7, 32


class RelationProgram:
    """bfhip_relation_program: a validated relation program (include/bfhip.h "Relation programs") — the base-field opcodes of a constraint
    program with WORD (append m[a] to the pending tuple) and ENTRY (add_to_relation(relation, multiplicity m[a], the pending tuple)).
    relation_words[r] = the width of relation r, 1 to 7. Host only to create and for eval_row; Context.relation_program_summary runs it over
    a component's cells. A refused program raises BfhipError naming the instruction index and the rule."""

    def __init__(self, code, n_cols, relation_words):
        self.code = [int(w) & 0xFFFFFFFF for w in code]
        self.relation_words = [int(w) for w in relation_words]
        self._h = ctypes.c_void_p()
        arr = (ctypes.c_uint32 * max(1, len(self.code)))(*self.code)
        widths = (ctypes.c_uint32 * max(1, len(self.relation_words)))(*self.relation_words)
        _check(lib().bfhip_relation_program_create(arr, ctypes.c_size_t(len(self.code)), int(n_cols), widths, len(self.relation_words), ctypes.byref(self._h)))
        out = (ctypes.c_uint32 * 8)()
        _check(lib().bfhip_relation_program_shape(self._h, out))
        self.shape = {"n_cols": out[0], "n_relations": out[1], "n_entries": out[2], "n_instr": out[3], "m_regs": out[4]}

    def close(self):
        if self._h:
            lib().bfhip_relation_program_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def eval_row(self, col_values):
        """bfhip_relation_program_eval_row (host only): the entries of ONE row, in program order, zero multiplicities included, as
        [(relation, multiplicity, tuple)] with the tuple cut to the relation's width. col_values: n_cols canonical words."""
        if len(col_values) != self.shape["n_cols"]:
            raise ValueError("one value per program column")
        n = ctypes.c_uint32()
        cap = self.shape["n_entries"]
        rels, mults, tups = (ctypes.c_uint32 * cap)(), (ctypes.c_uint32 * cap)(), (ctypes.c_uint32 * (7 * cap))()
        _check(lib().bfhip_relation_program_eval_row(self._h, Context._u32s(col_values) if len(col_values) else None, rels, mults, tups, cap, ctypes.byref(n)))
        return [(int(rels[e]), int(mults[e]), tuple(int(v) for v in tups[7 * e: 7 * e + self.relation_words[rels[e]]])) for e in range(n.value)]


class AirExpr:
    """A value of an AirBuilder: kind 'm' (M31, a base-field column expression) or 'q' (QM31). Operators + - * and unary -; a Python int
    stands for const(int). m op q promotes the m side (Q_FROM_M), except a product, which is Q_MULM."""
    __slots__ = ("builder", "id", "kind")

    def __init__(self, builder, vid, kind):
        self.builder, self.id, self.kind = builder, vid, kind

    def __add__(self, other): return self.builder._binary("add", self, other)
    def __radd__(self, other): return self.builder._binary("add", other, self)
    def __sub__(self, other): return self.builder._binary("sub", self, other)
    def __rsub__(self, other): return self.builder._binary("sub", other, self)
    def __mul__(self, other): return self.builder._binary("mul", self, other)
    def __rmul__(self, other): return self.builder._binary("mul", other, self)
    def __neg__(self): return self.builder._negate(self)


class AirBuilder:
    """Writes a constraint program from expressions — what a user writes; the bytecode is what bindings pass.
        b = AirBuilder(); a, x = b.col(0), b.col(1); b.constraint(a * a - x); prog = b.program()
    col(i, off) / secure_col(i, off) (coordinates in columns i..i+3) / param(i) / const(v) give values; every value is computed once, in
    the order it was created (so the order of first use of a column's offsets — the mask order — is the order of the col() calls that are
    used); other values no constraint depends on are dropped, but a column read stays (like stwo's next_trace_mask, it is part of the mask
    whether or not a constraint uses it); a register is reused after its value's last use."""

    def __init__(self):
        self._ops = []        # [op, kind of the result or None, sources (value ids), immediates]
        self._memo = {}

    def _emit(self, op, kind, srcs=(), imm=(), key=None):
        if key is not None and key in self._memo:
            return self._memo[key]
        self._ops.append((op, kind, tuple(srcs), tuple(imm)))
        e = AirExpr(self, len(self._ops) - 1, kind) if kind else None
        if key is not None:
            self._memo[key] = e
        return e

    def col(self, i, off=0):
        return self._emit(AIR_M_COL, "m", imm=(int(i), int(off)), key=("col", int(i), int(off)))

    def secure_col(self, i, off=0):
        return self._emit(AIR_Q_COL, "q", imm=(int(i), int(off)), key=("qcol", int(i), int(off)))

    def param(self, i):
        return self._emit(AIR_Q_PARAM, "q", imm=(int(i),), key=("param", int(i)))

    def const(self, v):
        return self._emit(AIR_M_CONST, "m", imm=(int(v) % P,), key=("const", int(v) % P))

    def _value(self, x):
        if isinstance(x, AirExpr):
            if x.builder is not self:
                raise ValueError("a value of another AirBuilder")
            return x
        if isinstance(x, (int, np.integer)):
            return self.const(int(x))
        raise TypeError("an AirBuilder value or an int, got %r" % (x,))

    def _to_q(self, x):
        return x if x.kind == "q" else self._emit(AIR_Q_FROM_M, "q", (x.id,), key=("from_m", x.id))

    def _binary(self, what, x, y):
        x, y = self._value(x), self._value(y)
        if x.kind == "m" and y.kind == "m":
            return self._emit({"add": AIR_M_ADD, "sub": AIR_M_SUB, "mul": AIR_M_MUL}[what], "m", (x.id, y.id))
        if what == "mul" and x.kind != y.kind:
            qv, mv = (x, y) if x.kind == "q" else (y, x)
            return self._emit(AIR_Q_MULM, "q", (qv.id, mv.id))
        return self._emit({"add": AIR_Q_ADD, "sub": AIR_Q_SUB, "mul": AIR_Q_MUL}[what], "q", (self._to_q(x).id, self._to_q(y).id))

    def _negate(self, x):
        if x.kind == "m":
            return self._emit(AIR_M_NEG, "m", (x.id,))
        return self._emit(AIR_Q_MULM, "q", (x.id, self.const(P - 1).id))

    def constraint(self, expr):
        expr = self._value(expr)
        self._emit(AIR_C_BASE if expr.kind == "m" else AIR_C_EXT, None, (expr.id,))

    def frac(self, num, den):
        """BFHIP_LOGUP_FRAC: add num / den to the open logUp column (LogupTraceGenerator::write_frac). A base-field numerator or
        denominator is lifted (Q_FROM_M). Fraction programs only: see logup_program()."""
        num, den = self._to_q(self._value(num)), self._to_q(self._value(den))
        self._emit(LOGUP_FRAC, None, (num.id, den.id))

    def end_column(self):
        """BFHIP_LOGUP_END_COL: close the open logUp column (finalize_col); the next frac() opens the next one."""
        self._emit(LOGUP_END_COL, None)

    def relation_entry(self, relation, multiplicity, values):
        """BFHIP_REL_WORD per value, then BFHIP_REL_ENTRY: one add_to_relation(relation, multiplicity, values). Base-field values only.
        Relation programs only: see relation_program()."""
        mult, values = self._value(multiplicity), [self._value(v) for v in values]
        if mult.kind != "m" or any(v.kind != "m" for v in values):
            raise ValueError("a relation entry takes base-field values (kind 'm')")
        for v in values:
            self._emit(REL_WORD, None, (v.id,))
        # the words are sources of the ENTRY too: the interpreters read them there, so their registers live until then
        self._emit(REL_ENTRY, None, (mult.id,) + tuple(v.id for v in values), imm=(int(relation),))

    def code(self):
        """The bytecode (a flat list of u32 words). Raises ValueError if the program needs more registers than the caps."""
        import heapq
        ops = self._ops
        live = [kind is None or op in (AIR_M_COL, AIR_Q_COL) for op, kind, _, _ in ops]
        for i in range(len(ops) - 1, -1, -1):
            if live[i]:
                for s in ops[i][2]:
                    live[s] = True
        last_use = {}
        for i, (_, _, srcs, _) in enumerate(ops):
            if live[i]:
                for s in srcs:
                    last_use[s] = i
        free = {"m": list(range(AIR_MAX_M_REGS + 1)), "q": list(range(AIR_MAX_Q_REGS + 1))}
        reg, words = {}, []
        for i, (op, kind, srcs, imm) in enumerate(ops):
            if not live[i]:
                continue
            regs = [reg[s] for s in srcs]
            for s in set(srcs):
                if last_use[s] == i:
                    heapq.heappush(free[ops[s][1]], reg[s])
            dst = 0
            if kind:
                dst = reg[i] = heapq.heappop(free[kind])
                if dst >= (AIR_MAX_M_REGS if kind == "m" else AIR_MAX_Q_REGS):
                    raise ValueError("the program needs more than %d %s registers" % ((AIR_MAX_M_REGS, "m") if kind == "m" else (AIR_MAX_Q_REGS, "q")))
                if i not in last_use:         # a column read no constraint uses: it stays for the mask, its register is free at once
                    heapq.heappush(free[kind], dst)
            if op in (AIR_M_COL, AIR_Q_COL):
                words += [op, dst, imm[0], imm[1] & 0xFFFFFFFF]
            elif op in (AIR_M_CONST, AIR_Q_PARAM):
                words += [op, dst, imm[0], 0]
            elif op in (AIR_C_BASE, AIR_C_EXT):
                words += [op, 0, regs[0], 0]
            elif op == LOGUP_END_COL:
                words += [op, 0, 0, 0]
            elif op == REL_WORD:
                words += [op, 0, regs[0], 0]
            elif op == REL_ENTRY:
                words += [op, imm[0] & 0xFFFFFFFF, regs[0], 0]
            else:
                words += [op, dst, regs[0], regs[1] if len(regs) > 1 else 0]
        return words

    def program(self, n_cols=None, n_params=None):
        """AirProgram of the bytecode; n_cols / n_params default to one more than the highest column / parameter any col() / param() named."""
        cols = [imm[0] + (4 if op == AIR_Q_COL else 1) for op, _, _, imm in self._ops if op in (AIR_M_COL, AIR_Q_COL)]
        pars = [imm[0] + 1 for op, _, _, imm in self._ops if op == AIR_Q_PARAM]
        return AirProgram(self.code(), max(cols, default=0) if n_cols is None else n_cols, max(pars, default=0) if n_params is None else n_params)

    def logup_program(self, n_cols=None, n_params=None):
        """LogupProgram of the bytecode (frac() / end_column() instead of constraint()); n_cols / n_params default as for program()."""
        cols = [imm[0] + (4 if op == AIR_Q_COL else 1) for op, _, _, imm in self._ops if op in (AIR_M_COL, AIR_Q_COL)]
        pars = [imm[0] + 1 for op, _, _, imm in self._ops if op == AIR_Q_PARAM]
        return LogupProgram(self.code(), max(cols, default=0) if n_cols is None else n_cols, max(pars, default=0) if n_params is None else n_params)


    def relation_program(self, relation_words, n_cols=None):
        """RelationProgram of the bytecode (relation_entry() instead of constraint()); relation_words[r] = the width of relation r; n_cols
        defaults as for program()."""
        cols = [imm[0] + (4 if op == AIR_Q_COL else 1) for op, _, _, imm in self._ops if op in (AIR_M_COL, AIR_Q_COL)]
        return RelationProgram(self.code(), max(cols, default=0) if n_cols is None else n_cols, relation_words)


def _q_mul(x, y):
    """QM31 product of two 4-word values: (a + b u)(c + d u), u^2 = 2 + i, over CM31 = M31[i]."""
    cm = lambda p, q: ((p[0] * q[0] - p[1] * q[1]) % P, (p[0] * q[1] + p[1] * q[0]) % P)
    a, b, c, d = (x[0], x[1]), (x[2], x[3]), (y[0], y[1]), (y[2], y[3])
    bd, ac, ad, bc = cm(b, d), cm(a, c), cm(a, d), cm(b, c)
    e = cm(bd, (2, 1))
    return [(ac[0] + e[0]) % P, (ac[1] + e[1]) % P, (ad[0] + bc[0]) % P, (ad[1] + bc[1]) % P]


BRAINFUCK_AIR_N_PARAMS = 25
_BF_N_MAIN = (8, 8, 4, 9, 13, 13, 11, 11, 11, 11, 11, 11, 7)


def brainfuck_air_params(lookup24, claimed4):
    """The 25 parameters of a brainfuck_air_program: for each of the Memory, Instruction and Processor relations z, alpha^0 .. alpha^6
    (8 values), then the component's claimed sum. lookup24: (z, alpha) of the three relations, as for logup_generate."""
    out = []
    for r in range(3):
        z, alpha = [int(v) for v in lookup24[8 * r: 8 * r + 4]], [int(v) for v in lookup24[8 * r + 4: 8 * r + 8]]
        out.append(z)
        cur = [1, 0, 0, 0]
        for _ in range(7):
            out.append(cur)
            cur = _q_mul(cur, alpha)
    return out + [[int(v) for v in claimed4]]


def brainfuck_air_program(component, logup_mask_order=0):
    """The constraints of component 0..12 of the Brainfuck AIR as a program — restated from csrc/air.h (the `FrameworkEval::evaluate` bodies
    of components/**/component.rs), logUp constraints included; the worked example of INTEGRATION.md section 2e.
    Returns (AirProgram, parameter names, column names). Columns: the n_main main-trace columns, then 4 coordinate columns per logUp column,
    then IsFirst — n_main + 4 n_logup + 1. Parameters: brainfuck_air_params. Constraints in bfhip_eval_constraints' order. The last logUp
    column is read at offsets [0, -1], or [-1, 0] under logup_mask_order = LOGUP_MASK_PREV_CUR."""
    if not 0 <= component < 13:
        raise ValueError("component 0..12")
    b = AirBuilder()
    n_main, n_logup = _BF_N_MAIN[component], 3 if component == 3 else 1
    t = [b.col(j) for j in range(n_main)]
    first_col = n_main + 4 * n_logup
    is_first, one = b.col(first_col), b.const(1)
    REL = {"memory": 0, "instruction": 1, "processor": 2}
    total = b.param(24)

    def combine(rel, values):
        base = 8 * REL[rel]
        acc = None
        for i, v in enumerate(values):
            term = b.param(base + 1 + i) * v
            acc = term if acc is None else acc + term
        return acc - b.param(base)

    state = {"col": 0, "prev": None}

    def logup_mid(num, den):
        cur = b.secure_col(n_main + 4 * state["col"])
        diff = cur if state["prev"] is None else cur - state["prev"]
        state["col"], state["prev"] = state["col"] + 1, cur
        b.constraint(diff * den - b._to_q(num))

    def logup_last(num, den):
        at = n_main + 4 * state["col"]
        if logup_mask_order == LOGUP_MASK_PREV_CUR:
            prev_row, cur = b.secure_col(at, -1), b.secure_col(at)
        else:
            cur, prev_row = b.secure_col(at), b.secure_col(at, -1)
        diff = cur - (prev_row - total * is_first)
        if state["prev"] is not None:
            diff = diff - state["prev"]
        b.constraint(diff * den - b._to_q(num))

    c = b.constraint
    if component == 0:        # memory/component.rs:62-137
        clk, mp, mv, d, n_clk, n_mp, n_mv, n_d = t
        c(is_first * clk); c(is_first * mp); c(is_first * mv); c(is_first * d)
        c(d * (d - one)); c(n_d * (n_d - one))
        c((n_mp - mp) * (n_mp - mp - one)); c((n_mp - mp - one) * (n_clk - clk - one)); c((n_mp - mp) * n_mv)
        c(d * (n_mp - mp)); c(d * (n_mv - mv))
        logup_last(d - one, combine("memory", (clk, mp, mv)))
    elif component == 1:      # instruction/component.rs:65-142
        ip, ci, ni, d, n_ip, n_ci, n_ni, n_d = t
        c(is_first * ip); c(d * (d - one)); c(n_d * (n_d - one)); c(d * ci); c(d * ni); c(n_d * n_ci); c(n_d * n_ni)
        c((n_ip - ip) * (n_ip - ip - one)); c((n_ip - ip - one) * (n_ci - ci)); c((n_ip - ip - one) * (n_ni - ni))
        logup_last(d - one, combine("instruction", (ip, ci, ni)))
    elif component == 2:      # program/component.rs:60-104
        ip, ci, ni, d = t
        c(is_first * ip); c(d * (d - one)); c(d * ci); c(d * ni)
        logup_last(one - d, combine("instruction", (ip, ci, ni)))
    elif component == 3:      # processor/component.rs:79-153 — three relation entries: Processor, Instruction, Memory
        clk, ip, ci, ni, mp, mv, mvi, d, n_clk = t
        c(is_first * clk); c(is_first * ip); c(is_first * mp); c(is_first * mv)
        c(mv * (mv * mvi - one)); c(mvi * (mv * mvi - one)); c(n_clk - clk - one)
        num = one - d
        den_p, den_i, den_m = combine("processor", (clk, ip, ci, ni, mp, mv, mvi)), combine("instruction", (ip, ci, ni)), combine("memory", (clk, mp, mv))
        logup_mid(num, den_p); logup_mid(num, den_i); logup_last(num, den_m)
    elif component in (4, 5):   # jump/jump_if_not_zero_component.rs:61-130, jump/jump_if_zero_component.rs:61-130
        clk, ip, ci, ni, mp, mv, mvi, n_clk, n_ip, n_mp, n_mv, d, is_mv_zero = t
        two = b.const(2)
        c(ci * (ci - b.const(ord("[") if component == 5 else ord("]"))))
        c(n_clk - clk - one); c(d * (d - one)); c(d * mv); c(d * ci)
        if component == 5:
            c((d - one) * (mv * (n_ip - ip - two) + is_mv_zero * (n_ip - (ni + one))))
        else:
            c((d - one) * (is_mv_zero * (n_ip - ip - two) + mv * (n_ip - ni)))
        c(n_mp - mp); c(n_mv - mv)
        logup_last(d - one, combine("processor", (clk, ip, ci, ni, mp, mv, mvi)))
    elif component == 12:     # end_of_execution/component.rs:61-90
        clk, ip, ci, ni, mp, mv, mvi = t
        c(ci)
        logup_last(b.const(P - 1), combine("processor", (clk, ip, ci, ni, mp, mv, mvi)))
    else:                     # processor/instructions/{input,left,minus,output,plus,right}_component.rs:62-122
        clk, ip, ci, ni, mp, mv, mvi, d, n_ip, n_mp, n_mv = t
        opcode = {6: ",", 7: "<", 8: "-", 9: ".", 10: "+", 11: ">"}[component]
        c(ci * (ci - b.const(ord(opcode)))); c(d * (d - one)); c(d * mv); c(d * ci); c((one - d) * (n_ip - ip - one))
        if opcode == "+":
            c(n_mp - mp); c((one - d) * (n_mv - mv - one))
        elif opcode == "-":
            c(n_mp - mp); c((one - d) * (n_mv - mv + one))
        elif opcode == "<":
            c((one - d) * (n_mp - mp + one))
        elif opcode == ">":
            c((one - d) * (n_mp - mp - one))
        elif opcode == ",":
            c(n_mp - mp)
        else:
            c(n_mp - mp); c(n_mv - mv)
        logup_last(d - one, combine("processor", (clk, ip, ci, ni, mp, mv, mvi)))
    names = ["%s.%s" % (r, p) for r in ("memory", "instruction", "processor") for p in ["z"] + ["alpha^%d" % i for i in range(7)]] + ["claimed_sum"]
    columns = ["main%d" % j for j in range(n_main)] + ["logup%d.%d" % (k, w) for k in range(n_logup) for w in range(4)] + ["is_first"]
    return b.program(n_cols=n_main + 4 * n_logup + 1, n_params=BRAINFUCK_AIR_N_PARAMS), names, columns


BRAINFUCK_LOGUP_N_PARAMS = 24


def brainfuck_logup_program(component):
    """`interaction_trace_evaluation` of component 0..12 of the Brainfuck AIR as a fraction program — restated from the branches of
    k_logup_rows (csrc/air.hip; memory/table.rs:485-518, instruction/table.rs:456-490, program/table.rs:233-265, processor/table.rs:456-529,
    jump/table.rs:436-475, instructions/table.rs:466-505, end_of_execution/table.rs:220-255). Returns (LogupProgram, parameter names).
    Columns: the n_main main-trace columns. Parameters: the first 24 of brainfuck_air_params. The Processor has three logUp columns of one
    fraction each (Processor, Instruction, Memory relations), the others one; numerators d - 1, 1 - d or -1."""
    if not 0 <= component < 13:
        raise ValueError("component 0..12")
    b = AirBuilder()
    n_main = _BF_N_MAIN[component]
    t = lambda *js: [b.col(j) for j in js]      # only the columns a fraction reads: a column read is never dropped
    one = b.const(1)
    REL = {"memory": 0, "instruction": 1, "processor": 2}

    def combine(rel, values):
        base = 8 * REL[rel]
        acc = None
        for i, v in enumerate(values):
            term = b.param(base + 1 + i) * v
            acc = term if acc is None else acc + term
        return acc - b.param(base)

    def column(num, den):
        b.frac(num, den)
        b.end_column()

    if component == 0:
        column(t(3)[0] - one, combine("memory", t(0, 1, 2)))
    elif component == 1:
        column(t(3)[0] - one, combine("instruction", t(0, 1, 2)))
    elif component == 2:
        column(one - t(3)[0], combine("instruction", t(0, 1, 2)))
    elif component == 3:
        num = one - t(7)[0]
        column(num, combine("processor", t(0, 1, 2, 3, 4, 5, 6)))
        column(num, combine("instruction", t(1, 2, 3)))
        column(num, combine("memory", t(0, 4, 5)))
    elif component in (4, 5):
        column(t(11)[0] - one, combine("processor", t(0, 1, 2, 3, 4, 5, 6)))
    elif component == 12:
        column(b.const(P - 1), combine("processor", t(0, 1, 2, 3, 4, 5, 6)))
    else:
        column(t(7)[0] - one, combine("processor", t(0, 1, 2, 3, 4, 5, 6)))
    names = ["%s.%s" % (r, p) for r in ("memory", "instruction", "processor") for p in ["z"] + ["alpha^%d" % i for i in range(7)]]
    return b.logup_program(n_cols=n_main, n_params=BRAINFUCK_LOGUP_N_PARAMS), names


BRAINFUCK_RELATION_WORDS = (3, 3, 7)


def brainfuck_relation_program(component):
    """The `add_to_relation` calls of component 0..12 of the Brainfuck AIR as a relation program — restated from the table of
    include/bfhip.h "the lookup tuples that do not cancel" (components/**/component.rs). Returns (RelationProgram, relation names).
    Columns: the n_main main-trace columns. Relations: 0 Memory (clk, mp, mv), 1 Instruction (ip, ci, ni), 2 Processor (clk, ip, ci, ni, mp,
    mv, mvi). Multiplicities d - 1 (a use), 1 - d (a yield) or -1; the Processor adds one entry to each relation."""
    if not 0 <= component < 13:
        raise ValueError("component 0..12")
    b = AirBuilder()
    n_main = _BF_N_MAIN[component]
    t = lambda *js: [b.col(j) for j in js]
    one = b.const(1)
    if component == 0:
        b.relation_entry(0, t(3)[0] - one, t(0, 1, 2))
    elif component == 1:
        b.relation_entry(1, t(3)[0] - one, t(0, 1, 2))
    elif component == 2:
        b.relation_entry(1, one - t(3)[0], t(0, 1, 2))
    elif component == 3:
        num = one - t(7)[0]
        b.relation_entry(0, num, t(0, 4, 5))
        b.relation_entry(1, num, t(1, 2, 3))
        b.relation_entry(2, num, t(0, 1, 2, 3, 4, 5, 6))
    elif component in (4, 5):
        b.relation_entry(2, t(11)[0] - one, t(0, 1, 2, 3, 4, 5, 6))
    elif component == 12:
        b.relation_entry(2, b.const(P - 1), t(0, 1, 2, 3, 4, 5, 6))
    else:
        b.relation_entry(2, t(7)[0] - one, t(0, 1, 2, 3, 4, 5, 6))
    return b.relation_program(BRAINFUCK_RELATION_WORDS, n_cols=n_main), RELATION_NAMES
