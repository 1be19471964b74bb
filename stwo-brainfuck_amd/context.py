"""One GPU as the library sees it: the device functions, the byte-level conventions and the PcsConfig (both by-value structs), shard
groups, and Context — the stream, the twiddles and every per-operation entry point (stwo's backend trait surface)."""
import contextlib
import ctypes
import json
import weakref

import numpy as np

from ._abi import BfhipError, Owned, _check, _ptr_array, _qm31s, _take_host_string, _u32s, abi, struct_fields
from ._abi_gen import (BFHIP_CHANNEL_BLAKE2S as CHANNEL_BLAKE2S, BFHIP_CHANNEL_POSEIDON252 as CHANNEL_POSEIDON252, BFHIP_LOGUP_MASK_CUR_PREV as LOGUP_MASK_CUR_PREV,
                       BFHIP_LOGUP_MASK_PREV_CUR as LOGUP_MASK_PREV_CUR, BFHIP_MERKLE_RFC7693 as MERKLE_RFC7693, BFHIP_MERKLE_STWO_COMPRESS as MERKLE_STWO_COMPRESS,
                       BFHIP_MIX_U64_COMPRESS as MIX_U64_COMPRESS, BFHIP_MIX_U64_HASH as MIX_U64_HASH)
from . import columns as _columns
from .programs import AIR_PROVE_CHECK, AirComponent, CompiledAir, LogupComponent
from .reports import (COMPONENT_NAMES, AirCheckReport, CheckReport, MultiplicityReport, MultiplicityResult, PreflightReport, RelationEntry, RelationProgramTable,
                      RelationTable, _relation_result)


def device_count():
    return abi().bfhip_device_count()


def device_memory(device_id=0):
    """bfhip_device_memory: (free, total) bytes of one GPU right now."""
    f, t = ctypes.c_uint64(), ctypes.c_uint64()
    _check(abi().bfhip_device_memory(device_id, ctypes.byref(f), ctypes.byref(t)))
    return f.value, t.value


def rccl_unique_id() -> bytes:
    """bfhip_rccl_unique_id: the 128-byte id rank 0 creates for a multi-process shard group (loads librccl on first use)."""
    buf = (ctypes.c_uint8 * 128)()
    _check(abi().bfhip_rccl_unique_id(buf))
    return bytes(buf)


class LocalGroup(Owned):
    """Rendezvous object of an in-process shard group (bfhip_local_group_create): `count` contexts of this process, one thread each."""
    _destroy = "bfhip_local_group_destroy"
    _close_on_del = False       # the contexts that joined it use it until they leave

    def __init__(self, count):
        self._h = ctypes.c_void_p()
        _check(abi().bfhip_local_group_create(count, ctypes.byref(self._h)))
        self.count = count


class Conventions(ctypes.Structure):
    """include/bfhip.h `bfhip_conventions`: the byte-level stwo conventions that cannot be confirmed offline, one switch each.
    All zero = the defaults (zero-state raw-compress Merkle nodes, raw-compress mix_u64, logUp mask order [0, -1])."""
    _fields_ = struct_fields("bfhip_conventions")


# One list, changed in place, so that every module that imported it sees the current default
_default_conventions = [0, 0, 0, 0]
_live_contexts = weakref.WeakSet()


def set_default_conventions(merkle_node_hash=0, mix_u64=0, logup_mask_order=0, merkle_channel=0):
    """Process-wide default of the Python mirror: adopted by every Context created afterwards, applied to the live ones, and used by
    verify_brainfuck(conventions=None). The C ABI itself has no global state: conventions are per context / per verify call."""
    _default_conventions[:] = int(merkle_node_hash), int(mix_u64), int(logup_mask_order), int(merkle_channel)
    for c in list(_live_contexts):
        if c._h:
            c.set_conventions(*_default_conventions)


def _conv_ref(conventions):
    return ctypes.byref(Conventions(*(_default_conventions if conventions is None else conventions)))


class PcsConfig(ctypes.Structure):
    """include/bfhip.h `bfhip_pcs_config`: stwo's PcsConfig (pow_bits, FriConfig { log_last_layer_degree_bound, log_blowup_factor, n_queries }).
    PcsConfig() = PcsConfig::default() = pow_bits 5, log_blowup_factor 1, log_last_layer_degree_bound 0, n_queries 3. The proof JSON does not
    carry it: verify a proof under the config it was made with."""
    _fields_ = struct_fields("bfhip_pcs_config")

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


def _program_columns(program, col_ptrs, col_shifts, where=""):
    """(column pointers, column shifts) of a program's run as host arrays, either None where there is nothing to pass."""
    if len(col_ptrs) != program.shape["n_cols"] or (col_shifts is not None and len(col_shifts) != len(col_ptrs)):
        raise ValueError(where + "one column pointer (and shift) per program column")
    return _ptr_array(col_ptrs) if col_ptrs else None, None if col_shifts is None or not col_ptrs else _u32s(col_shifts)


class Context(Owned):
    """One GPU + one HIP stream + the twiddle tree (mod.rs:480-487: twiddles, channel and commitment scheme setup)."""
    _destroy = "bfhip_ctx_destroy"
    _ptr_array, _u32s = staticmethod(_ptr_array), staticmethod(_u32s)

    def __init__(self, device_id=0, max_log_domain=22):
        self._h = ctypes.c_void_p()
        _check(abi().bfhip_ctx_create(device_id, max_log_domain, ctypes.byref(self._h)))
        self.max_log_domain = max_log_domain
        _live_contexts.add(self)
        if any(_default_conventions):
            self.set_conventions(*_default_conventions)

    def sync(self):
        _check(abi().bfhip_ctx_sync(self._h))

    def set_conventions(self, merkle_node_hash=0, mix_u64=0, logup_mask_order=0, merkle_channel=0):
        cv = Conventions(merkle_node_hash, mix_u64, logup_mask_order, merkle_channel)
        _check(abi().bfhip_ctx_set_conventions(self._h, ctypes.byref(cv)))

    def get_conventions(self):
        cv = Conventions()
        _check(abi().bfhip_ctx_get_conventions(self._h, ctypes.byref(cv)))
        return cv.merkle_node_hash, cv.mix_u64, cv.logup_mask_order, cv.merkle_channel

    def set_pcs_config(self, pcs_config=None):
        """bfhip_ctx_set_pcs_config: the PcsConfig of every later proof of this context (None = the default). Needs
        max_log_domain >= log_max_rows + log_blowup_factor + 1."""
        _check(abi().bfhip_ctx_set_pcs_config(self._h, _pcs_ref(pcs_config)))

    def pcs_config(self):
        out = PcsConfig()
        _check(abi().bfhip_ctx_get_pcs_config(self._h, ctypes.byref(out)))
        return out

    def set_overlap(self, mask=1):
        """bit 0: tree commitment (Merkle beside the transforms of the smaller columns), bit 1: quotients / FRI first-layer tree, bit 2 (shard
        groups): the send-receive of a tree's largest size class on the partner stream beside the transforms of the smaller columns."""
        _check(abi().bfhip_ctx_set_overlap(self._h, int(mask)))

    def set_sync_policy(self, blocking):
        """bfhip_ctx_set_sync_policy: True = the host sleeps in its waits (more waiting contexts than cores), False (default) = polls first."""
        _check(abi().bfhip_ctx_set_sync_policy(self._h, 1 if blocking else 0))

    def set_mailbox(self, mode=-2, timeout_ms=0, test_delay_ms=-1):
        """bfhip_ctx_set_mailbox: mode -2 keeps the mode / -1 automatic / 0 off / 1 on; timeout_ms 0 keeps the timeout; test_delay_ms < 0 keeps
        the (test) delay — a positive delay needs the test-hooks build of the library."""
        _check(abi().bfhip_ctx_set_mailbox(self._h, int(mode), int(timeout_ms), int(test_delay_ms)))

    def last_proof_flags(self):
        """bfhip_ctx_last_proof_flags: {mailbox_order, kept_preprocessed, shared_preprocessed, replicated_transforms, split_gather, fri_fold_leaf, preflight}
        of the last completed proof."""
        f = ctypes.c_uint32()
        _check(abi().bfhip_ctx_last_proof_flags(self._h, ctypes.byref(f)))
        return {"mailbox_order": bool(f.value & 1), "kept_preprocessed": bool(f.value & 2), "shared_preprocessed": bool(f.value & 4), "replicated_transforms": bool(f.value & 8),
                "split_gather": bool(f.value & 16), "fri_fold_leaf": bool(f.value & 32), "preflight": bool(f.value & 64)}

    def set_preflight(self, on=True):
        """bfhip_ctx_set_preflight: every later proof of this context first asserts the 13 AIRs and the logUp total on its tables (one batched
        launch pair, one read-back) and raises TraceRejected — naming component, constraint, row and unbalanced tuple — instead of proving a
        trace that cannot be proved. A filter, not a soundness gate: the lookup elements are the fixed public ones of Trace.check()."""
        _check(abi().bfhip_ctx_set_preflight(self._h, 1 if on else 0))

    def preflight(self):
        on = ctypes.c_int32()
        _check(abi().bfhip_ctx_get_preflight(self._h, ctypes.byref(on)))
        return bool(on.value)

    def last_preflight_report(self):
        """bfhip_ctx_last_preflight as the raw PreflightReport."""
        rep = PreflightReport()
        _check(abi().bfhip_ctx_last_preflight(self._h, ctypes.byref(rep)))
        return rep

    def last_preflight(self):
        """bfhip_ctx_last_preflight: (CheckResult, RelationResult) of the last proof of this context that reached the preflight. The
        CheckResult also has .ran, .rejected and .seconds (host wall time of the preflight)."""
        return self.last_preflight_report().results()

    def clock_probe(self, seconds=0.6):
        """bfhip_clock_probe: {ghz (median over workgroups), ghz_min, ghz_max, G_compressions_per_s, launches, ms_per_launch} of a register-only
        Blake2s loop run back to back for `seconds` — the clock this device sustains under the dominant kernel's instruction mix."""
        out = (ctypes.c_double * 6)()
        _check(abi().bfhip_clock_probe(self._h, seconds, out))
        return dict(zip(("ghz", "ghz_min", "ghz_max", "G_compressions_per_s", "launches", "ms_per_launch"), [float(v) for v in out]))

    def clock_probe_mix(self, seconds=0.5, log_nodes=22):
        """bfhip_clock_probe_mix: {ghz, G_compressions_per_s, launches, us_per_launch, sampler_spanned_the_window, sampler_seconds} — the clock held under the REAL
        Merkle kernel (sidecar sampler) and that kernel's rate on an inner layer of 2^log_nodes nodes."""
        out = (ctypes.c_double * 6)()
        _check(abi().bfhip_clock_probe_mix(self._h, seconds, int(log_nodes), out))
        d = dict(zip(("ghz", "G_compressions_per_s", "launches", "us_per_launch", "sampler_spanned_the_window", "sampler_seconds"), [float(v) for v in out]))
        d["sampler_spanned_the_window"] = bool(d["sampler_spanned_the_window"])
        return d

    def memory(self):
        """bfhip_ctx_memory: {arena_reserved, arena_peak, twiddles, arena_in_use} in bytes."""
        out = (ctypes.c_uint64 * 4)()
        _check(abi().bfhip_ctx_memory(self._h, out))
        return dict(zip(("arena_reserved", "arena_peak", "twiddles", "arena_in_use"), [int(v) for v in out]))

    def set_scratch_reserve(self, nbytes):
        """bfhip_ctx_set_scratch_reserve: ONE device block of nbytes that the call-scoped memory of air_prove, logup_program_generate_batch,
        air_compose and the other generic calls is served from where it fits, instead of one device allocation and release per call (a
        release waits for the whole device). 0 = none, the default. Same results either way. Size it from scratch_stats()["high_water"].
        Refused while a PcsSession is open."""
        _check(abi().bfhip_ctx_set_scratch_reserve(self._h, int(nbytes)))

    def scratch_stats(self):
        """bfhip_ctx_scratch_stats: {reserve (bytes), high_water (of its use since it was set), device_allocations (made by call-scoped
        memory since the context was created), served (requests placed in a reserve since then)}."""
        out = (ctypes.c_uint64 * 4)()
        _check(abi().bfhip_ctx_scratch_stats(self._h, out))
        return dict(zip(("reserve", "high_water", "device_allocations", "served"), [int(v) for v in out]))

    # -- the per-kernel profiler (HIP events around every instrumented launch) ----------------------------------------------------------
    def profile_enable(self, mode=1):
        """bfhip_profile_enable: 0 off, 1 every instrumented kernel, 2 only k_merkle_layer (the dominant kernel; lowest overhead)."""
        _check(abi().bfhip_profile_enable(self._h, int(mode)))

    def profile_reset(self):
        """bfhip_profile_reset: forgets the records so far; the mode stays."""
        _check(abi().bfhip_profile_reset(self._h))

    def profile_report(self):
        """bfhip_profile_report as a dict: {scope: {"calls": n, "total_ms": t, "bytes": b, ...}, ...} since the last reset."""
        js = ctypes.c_void_p()
        _check(abi().bfhip_profile_report(self._h, ctypes.byref(js)))
        return json.loads(_take_host_string(js))

    @contextlib.contextmanager
    def profiling(self, mode=1):
        """with ctx.profiling(): the profiler on and reset for the block, off again behind it (also when the block raises). Read
        profile_report() inside the block."""
        self.profile_enable(mode)
        try:
            self.profile_reset()
            yield self
        finally:
            self.profile_enable(0)

    def set_table_builder(self, on_gpu=True):
        """Where this context builds the 13 component tables: GPU kernels (default) or the host builders. Identical results."""
        _check(abi().bfhip_ctx_set_table_builder(self._h, int(on_gpu)))

    # -- one proof over several GPUs (shard group: bfhip_ctx_join_*_group) -----------------------------------------------------------------
    def join_local_group(self, group, rank):
        """Makes this context rank `rank` of a LocalGroup: N contexts of this process, one host thread each, prove ONE trace together."""
        _check(abi().bfhip_ctx_join_local_group(self._h, group._h, rank))
        self._group = group          # keep the rendezvous object alive as long as the context uses it

    def join_rccl_group(self, unique_id: bytes, rank, count):
        """One process per GPU: `unique_id` is rccl_unique_id() of rank 0, handed over by the host program (replicas.share_unique_id)."""
        if len(unique_id) != 128:
            raise BfhipError("an RCCL unique id has 128 bytes")
        _check(abi().bfhip_ctx_join_rccl_group(self._h, unique_id, rank, count))

    def set_shard_policy(self, policy=-1):
        """bfhip_ctx_set_shard_policy: -1 automatic, 0 exchange columns -> rows, 1 replicate the transforms (every rank of a group the same)."""
        _check(abi().bfhip_ctx_set_shard_policy(self._h, int(policy)))

    def leave_group(self):
        _check(abi().bfhip_ctx_leave_group(self._h))
        self._group = None

    def group_stats(self):
        """{all_gathers, max_reduces, exchanges, bytes_sent} of this rank since it joined its shard group."""
        out = (ctypes.c_uint64 * 4)()
        _check(abi().bfhip_ctx_group_stats(self._h, out))
        return dict(zip(("all_gathers", "max_reduces", "exchanges", "bytes_sent"), [int(v) for v in out]))

    def group_times(self):
        """{all_gather_ms, max_reduce_ms, exchange_ms}: GPU-side time of this rank's collectives since it joined its shard group."""
        out = (ctypes.c_double * 3)()
        _check(abi().bfhip_ctx_group_times(self._h, out))
        return dict(zip(("all_gather_ms", "max_reduce_ms", "exchange_ms"), [float(v) for v in out]))

    def group_latency(self, reset=False):
        """bfhip_ctx_group_latency: per kind of collective {count, gpu_us: {p50, p90, max}, host_us: {p50, p90, max}} since the join / the last reset."""
        out = (ctypes.c_double * 21)()
        _check(abi().bfhip_ctx_group_latency(self._h, 1 if reset else 0, out))
        res = {}
        for k, name in enumerate(("all_gather", "max_reduce", "exchange")):
            v = [float(x) for x in out[7 * k:7 * k + 7]]
            res[name] = {"count": int(v[0]), "gpu_us": {"p50": round(v[1], 1), "p90": round(v[2], 1), "max": round(v[3], 1)},
                         "host_us": {"p50": round(v[4], 1), "p90": round(v[5], 1), "max": round(v[6], 1)}}
        return res

    def group_info(self):
        r, n, t = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_char_p()
        _check(abi().bfhip_ctx_group_info(self._h, ctypes.byref(r), ctypes.byref(n), ctypes.byref(t)))
        return r.value, n.value, (t.value or b"").decode()

    # -- buffers ---------------------------------------------------------------------------------------------------
    def malloc(self, nbytes):
        p = ctypes.c_void_p()
        _check(abi().bfhip_malloc(self._h, nbytes, ctypes.byref(p)))
        return p.value

    def free(self, ptr):
        _check(abi().bfhip_free(self._h, ptr))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        ptr = self.malloc(arr.nbytes)
        _check(abi().bfhip_upload(self._h, ptr, arr.ctypes.data, arr.nbytes))
        return ptr

    def download(self, ptr, n, dtype=np.uint32):
        out = np.empty(n, dtype=dtype)
        _check(abi().bfhip_download(self._h, out.ctypes.data, ptr, out.nbytes))
        return out

    # -- row order <-> storage order ----------------------------------------------------------------------------------------------------
    def columns_from_rows(self, table, log_size, columns=None, pad=None, repeat_last=False, out=None):
        """bfhip_columns_from_rows: a trace in ROW order (row r + 1 = the row at offset +1) to storage-order device columns of 2^log_size
        words, in one launch; every word read is checked to be a canonical M31 value (BfhipError naming the lowest row, then column).
        table: a (n_rows, n_src) uint32 array (uploaded into a temporary device buffer, freed before return), a DeviceRows(ptr, n_rows,
        n_cols, row_stride) or a DeviceRowColumns(ptrs, n_rows). columns: the source column of every output column (None = all, in
        order; subsets, permutations and repeats are fine). Rows n_rows .. 2^log_size - 1 hold pad[k] (None = 0), or with repeat_last a
        copy of the last row. out: device pointers to write instead of new columns. Returns a Columns handle (closable, a context
        manager) whose pointers go wherever column pointers are taken."""
        return _columns.columns_from_rows(self, table, log_size, columns, pad, repeat_last, out)

    def rows_select(self, table, log_size=None, where=(), order_by=(), columns=None, rows=None, pad=None, repeat_last=False, out=None, want_order=False):
        """bfhip_rows_select: columns_from_rows of a SELECTION of the table's rows — filtered, sorted, read at row offsets — without a trip
        through the host. table: as columns_from_rows. where: (col, "==" | "!=" | "<" | "<=" | ">" | ">=", value) terms, all of which a
        selected row satisfies (integer comparison). order_by: col or (col, "desc") keys, most significant first; the sort is stable and
        without keys the order is the source's. columns: col or (col, offset) per output column (None = every source column): output row i
        is the source row of selected row i plus the offset. rows: (begin, end) = the candidate rows, None = all; the offsets must stay
        inside the table from every candidate. Rows past the selected ones hold pad[k] (None = 0), or with repeat_last the last selected
        row. log_size None: a count-only call first, then the smallest domain that holds the selection (at least 1). Returns a Columns
        handle that also carries .n_selected and, with want_order, .order — the source row of every selected row (else None)."""
        return _columns.rows_select(self, table, log_size, where, order_by, columns, rows, pad, repeat_last, out, want_order)

    def rows_fill(self, table, log_size=None, group=(), step=None, gaps=False, columns=None, order=None, n_order=None, rows=None, out=None):
        """bfhip_rows_fill: the entries of the table — rows `rows` = (begin, end) in source order, or the source rows `order` (a device
        pointer to n_order words as rows_select's order_d, or a uint32 array) — with the missing rows inserted: with gaps=True a row for
        every value of column `step` skipped between two consecutive entries that agree in the `group` columns, and behind the last entry
        rows without end. columns: ("keep", col[, offset]) | ("set", col, value[, offset]) | ("mark", value[, offset]); offset 0..16 reads
        the successor rows. Returns Columns with .n_filled = the rows before the tail; log_size None takes the smallest domain that holds
        them."""
        return _columns.rows_fill(self, table, log_size, group, step, gaps, columns, order, n_order, rows, out)

    def rows_fill_count(self, table, group=(), step=None, gaps=False, order=None, n_order=None, rows=None):
        """The count-only form of bfhip_rows_fill: the number of rows before the tail, the inserted ones included."""
        return _columns.rows_fill_count(self, table, group, step, gaps, order, n_order, rows)

    def rows_select_count(self, table, where=(), order_by=(), rows=None, want_order=False, order_out=None):
        """The count-only form of bfhip_rows_select: (the number of selected rows, their source rows in order if want_order else None).
        order_out: a device pointer to one word per candidate row that receives the order instead (nothing is downloaded; the second
        value is None) — what rows_fill takes as `order`."""
        return _columns.rows_select_count(self, table, where, order_by, rows, want_order, order_out)

    def rows_from_columns(self, col_ptrs, log_size, n_rows=None):
        """bfhip_rows_from_columns: storage-order device columns (pointers, or a Columns handle) back in row order, as a (n_rows,
        n_cols) uint32 array; n_rows None = all 2^log_size. What reads a generated column — multiplicities, a logUp column — by row."""
        return _columns.rows_from_columns(self, col_ptrs, log_size, n_rows)

    def witness_program_generate(self, program, log_size, col_ptrs, args=(), out=None):
        """bfhip_witness_program_generate: a WitnessProgram at every row of CanonicCoset(log_size), in one launch and without a read-back.
        col_ptrs: one full-size storage-order device column per program column (pointers, or a Columns handle); args: the program's
        per-call canonical words; out: device pointers to write instead of new columns. Returns a Columns handle of the n_out output
        columns that owns what it allocated. Nothing comes from the arena: it works inside an open PcsSession."""
        return _columns.witness_program_generate(self, program, log_size, col_ptrs, args, out)

    # -- PolyOps ---------------------------------------------------------------------------------------------------
    def interpolate(self, src_ptrs, dst_ptrs, log_size, replicated=False):
        _check(abi().bfhip_interpolate(self._h, _ptr_array(src_ptrs), _ptr_array(dst_ptrs), len(src_ptrs), log_size, int(replicated)))

    def evaluate(self, coeff_ptrs, dst_ptrs, log_size, log_eval, replicated=False):
        _check(abi().bfhip_evaluate(self._h, _ptr_array(coeff_ptrs), _ptr_array(dst_ptrs), len(coeff_ptrs), log_size, log_eval, int(replicated)))

    def is_first_coeffs(self, log_min, log_max, dst_ptrs):
        """interpolate(gen_is_first(n)) for n = log_min..log_max in closed form (mod.rs:497); dst_ptrs[n - log_min] may be None."""
        _check(abi().bfhip_is_first_coeffs(self._h, log_min, log_max, _ptr_array(dst_ptrs)))

    def is_first_lde(self, log_min, log_max, log_blowup, dst_ptrs):
        """evaluate(interpolate(gen_is_first(n))) on 2^(n + log_blowup) cells for n = log_min..log_max in closed form; dst_ptrs[n - log_min] may be None."""
        _check(abi().bfhip_is_first_lde(self._h, log_min, log_max, log_blowup, _ptr_array(dst_ptrs)))

    def is_first_eval_at_point(self, log_size, point8):
        """eval_at_point of IsFirst(log_size) in closed form (no coefficient column)."""
        out = (ctypes.c_uint32 * 4)()
        _check(abi().bfhip_is_first_eval_at_point(self._h, log_size, _u32s(point8), out))
        return list(out)

    def eval_at_point(self, coeff_ptr, log_size, point8, replicated=False):
        out = (ctypes.c_uint32 * 4)()
        _check(abi().bfhip_eval_at_point(self._h, coeff_ptr, log_size, int(replicated), _u32s(point8), out))
        return list(out)

    # -- ColumnOps / FieldOps / AccumulationOps ---------------------------------------------------------------------------------
    def broadcast16(self, rows_ptr, dst_ptr, n_rows):
        _check(abi().bfhip_broadcast16(self._h, rows_ptr, dst_ptr, n_rows))

    def bit_reverse(self, src_ptr, dst_ptr, log_size):
        _check(abi().bfhip_bit_reverse(self._h, src_ptr, dst_ptr, log_size))

    def batch_inverse_m31(self, src_ptr, dst_ptr, n):
        _check(abi().bfhip_batch_inverse_m31(self._h, src_ptr, dst_ptr, n))

    def batch_inverse_qm31(self, src_ptrs, dst_ptrs, n):
        _check(abi().bfhip_batch_inverse_qm31(self._h, _ptr_array(src_ptrs), _ptr_array(dst_ptrs), n))

    def accumulate(self, dst_ptr, src_ptr, n):
        _check(abi().bfhip_accumulate(self._h, dst_ptr, src_ptr, n))

    # -- MerkleOps / FriOps / GrindOps -------------------------------------------------------------------------------------------------
    def merkle_commit_layer(self, log_size, prev_ptr, col_ptrs, out_ptr, col_shifts=None):
        sh = None if col_shifts is None else _u32s(col_shifts)
        _check(abi().bfhip_merkle_commit_layer(self._h, log_size, prev_ptr or None, _ptr_array(col_ptrs), sh, len(col_ptrs), out_ptr))

    def merkle_commit_layer_poseidon252(self, log_size, prev_ptr, col_ptrs, out_ptr, col_shifts=None):
        sh = None if col_shifts is None else _u32s(col_shifts)
        _check(abi().bfhip_merkle_commit_layer_poseidon252(self._h, log_size, prev_ptr or None, _ptr_array(col_ptrs), sh, len(col_ptrs), out_ptr))

    def hades_permutation(self, state3):
        """state3: three Python ints < p. Returns three ints."""
        words = []
        for x in state3:
            words += [(int(x) >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
        out = (ctypes.c_uint32 * 24)()
        _check(abi().bfhip_hades_permutation(self._h, _u32s(words), out))
        return [sum(int(out[8 * k + i]) << (32 * i) for i in range(8)) for k in range(3)]

    def fold_line(self, src_ptrs, dst_ptrs, log_size, alpha4):
        _check(abi().bfhip_fold_line(self._h, _ptr_array(src_ptrs), _ptr_array(dst_ptrs), log_size, _u32s(alpha4)))

    def fri_fold_leaf(self, src_ptrs, quot_ptrs, dst_ptrs, log_size, alpha4, out_ptr):
        """bfhip_fri_fold_leaf: fold into a layer of 2^log_size rows and hash its rows in one launch. src_ptrs None: the first line layer
        (circle fold of quot_ptrs alone); quot_ptrs None: a plain line fold. Whole layers only."""
        _check(abi().bfhip_fri_fold_leaf(self._h, _ptr_array(src_ptrs) if src_ptrs is not None else None, _ptr_array(quot_ptrs) if quot_ptrs is not None else None,
                                         _ptr_array(dst_ptrs), log_size, _u32s(alpha4), out_ptr))

    def fold_circle_into_line(self, dst_ptrs, src_ptrs, log_size, alpha4):
        _check(abi().bfhip_fold_circle_into_line(self._h, _ptr_array(dst_ptrs), _ptr_array(src_ptrs), log_size, _u32s(alpha4)))

    def grind(self, digest32, pow_bits):
        nonce = ctypes.c_uint64()
        _check(abi().bfhip_grind(self._h, bytes(digest32), pow_bits, ctypes.byref(nonce)))
        return nonce.value

    def grind_poseidon252(self, digest32, pow_bits, start_nonce=0, with_tried=False):
        """GrindOps::grind for Poseidon252Channel: the smallest nonce >= start_nonce whose poseidon_hash(digest, nonce) has >= pow_bits
        trailing zeros in that channel's sense. digest32: the felt252 digest as 32 canonical little-endian bytes.
        with_tried: also return the number of nonces scanned (launches x span)."""
        digest32 = bytes(digest32)
        if len(digest32) != 32:
            raise ValueError("grind_poseidon252: the digest is 32 bytes")
        nonce, tried = ctypes.c_uint64(), ctypes.c_uint64()
        _check(abi().bfhip_grind_poseidon252(self._h, digest32, pow_bits, start_nonce, ctypes.byref(nonce), ctypes.byref(tried)))
        return (nonce.value, tried.value) if with_tried else nonce.value

    def gather(self, col_ptr, indices):
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        out = np.empty(idx.size, dtype=np.uint32)
        _check(abi().bfhip_gather(self._h, col_ptr, idx.ctypes.data, idx.size, out.ctypes.data))
        return out

    # -- per-component AIR operations (LogupTraceGenerator / ComponentProver / QuotientOps) --------------------------------------------
    def logup_generate(self, component, log_size, main_row_ptrs, lookup24, out_col_ptrs):
        """interaction_trace_evaluation of one component; returns its claimed sum (4 u32)."""
        claimed = (ctypes.c_uint32 * 4)()
        _check(abi().bfhip_logup_generate(self._h, component, log_size, _ptr_array(main_row_ptrs), _u32s(lookup24), _ptr_array(out_col_ptrs), claimed))
        return list(claimed)

    def eval_constraints(self, component, log_size, is_first_ptr, main_lde_ptrs, inter_lde_ptrs, lookup24, claimed4, coeffs, acc_ptrs, main_shifts=None, inter_shifts=None):
        """evaluate_constraint_quotients_on_domain of one component, accumulated into the 4 coordinate columns acc_ptrs."""
        _check(abi().bfhip_eval_constraints(self._h, component, log_size, is_first_ptr, _ptr_array(main_lde_ptrs),
                                            None if main_shifts is None else _u32s(main_shifts), _ptr_array(inter_lde_ptrs),
                                            None if inter_shifts is None else _u32s(inter_shifts), _u32s(lookup24), _u32s(claimed4),
                                            _u32s(coeffs), _ptr_array(acc_ptrs)))

    def air_eval_domain(self, program, log_size, log_expand, col_ptrs, params, coeffs, acc_ptrs, col_shifts=None):
        """bfhip_air_eval_domain: the constraints of an AirProgram on CanonicCoset(log_size + log_expand).circle_domain(), each times its
        coefficient, the sum times 1 / vanishing, added into the 4 coordinate columns acc_ptrs. col_ptrs: one device column per program column
        (2^(log_size + log_expand - shift) cells); params / coeffs: QM31 values (4 words each), one per parameter / constraint.
        program: an AirProgram (interpreted), or the CompiledAir that this context's air_compile made of one (its own kernel; same result)."""
        pars, coes = _qm31s(params, "a parameter or coefficient"), _qm31s(coeffs, "a parameter or coefficient")
        cols, shifts = _program_columns(program, col_ptrs, col_shifts)
        if len(acc_ptrs) != 4:
            raise ValueError("the accumulator is 4 coordinate columns")
        # a CompiledAir (Context.air_compile) runs its own kernel behind the same checks: bfhip_air_kernel_eval_domain
        entry = abi().bfhip_air_kernel_eval_domain if isinstance(program, CompiledAir) else abi().bfhip_air_eval_domain
        _check(entry(self._h, program._h, int(log_size), int(log_expand), cols, shifts, *pars, *coes, _ptr_array(acc_ptrs)))

    def air_compose(self, components, random_coeff, dst_ptrs, dst_log):
        """bfhip_air_compose: the composition polynomial of ALL components of an AIR — its 4 coefficient columns of 2^dst_log words written
        to dst_ptrs (overwritten), ready for PcsSession.commit(form 1). A component is (program_or_CompiledAir, log_size, log_expand,
        col_ptrs, params[, col_shifts]) with the columns on CanonicCoset(log_size + log_expand).circle_domain(); constraint g of all T gets
        random_coeff^(T - 1 - g) (air_compose_coeffs). dst_log = the largest log_size + log_expand of the list. AirPrograms run in one
        launch, CompiledAirs in one launch each behind it."""
        if len(dst_ptrs) != 4:
            raise ValueError("the destination is 4 coordinate columns")
        r = [int(w) for w in random_coeff]
        if len(r) != 4:
            raise ValueError("random_coeff is 4 words")
        comps, keep = (AirComponent * max(1, len(components)))(), []
        for k, comp in enumerate(components):
            program, log_size, log_expand, col_ptrs, params = comp[:5]
            cols, shifts = _program_columns(program, col_ptrs, comp[5] if len(comp) > 5 else None, "component %d: " % k)
            pars, n_params = _qm31s(params, "a parameter")
            keep += [cols, shifts, pars, program]
            compiled = isinstance(program, CompiledAir)
            comps[k] = AirComponent(None if compiled else program._h.value, program._h.value if compiled else None, int(log_size), int(log_expand),
                                    None if cols is None else ctypes.cast(cols, ctypes.POINTER(ctypes.c_void_p)), shifts, pars, n_params, 0)
        _check(abi().bfhip_air_compose(self._h, comps, len(components), _u32s(r), int(dst_log), _ptr_array(dst_ptrs)))

    def air_prove(self, statement, tree_cols, channel, kernels=None, check=False):
        """bfhip_air_prove: the whole proof of an AIR given as an AirStatement — the session, the mixes and draws, the batched interaction
        trace, air_compose, the mask, prove_values and the sanity check, in the order include/bfhip.h states. tree_cols[t][c]: device
        column c of caller tree t (full size). kernels: per component None or the CompiledAir of its program. check: air_check on every
        component behind the interaction trace; a violation raises BfhipError naming component, constraint and cell. Returns the bytes
        {"claimed_sums": [...], "proof": <CommitmentSchemeProof>} that air_verify takes."""
        st = statement._c()
        if len(tree_cols) != len(statement.trees) or any(len(cols) != len(tree[0]) for cols, tree in zip(tree_cols, statement.trees)):
            raise ValueError("one device column per column of every caller tree")
        if kernels is not None and len(kernels) != len(statement.components):
            raise ValueError("one kernel (or None) per component")
        per_tree = [_ptr_array(cols) for cols in tree_cols]
        trees = (ctypes.c_void_p * max(1, len(per_tree)))(*[ctypes.cast(a, ctypes.c_void_p) for a in per_tree])
        ks = None if kernels is None else (ctypes.c_void_p * len(kernels))(*[None if k is None else k._h for k in kernels])
        js, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(abi().bfhip_air_prove(self._h, ctypes.byref(st), trees, ks, channel._h, AIR_PROVE_CHECK if check else 0, ctypes.byref(js), ctypes.byref(n)))
        return _take_host_string(js, n.value)

    def air_compile(self, program):
        """bfhip_air_compile: the AirProgram as its own gfx950 kernel, generated (AirProgram.source) and compiled in-process for this
        context's device. Returns a CompiledAir, which air_eval_domain accepts in place of the program; the program may be closed."""
        return CompiledAir(self, program)

    def air_check(self, program, log_size, col_ptrs, params, col_shifts=None):
        """bfhip_air_check: the constraints of an AirProgram asserted on the trace domain CanonicCoset(log_size) itself (stwo's
        assert_constraints for any AIR). col_ptrs: one device column per program column (2^(log_size - shift) cells); params: QM31 values (4
        words each). Returns the AirCheckReport (as_dict() for named fields, format_air_check for the text); violations are a result, not
        an error."""
        pars = _qm31s(params, "a parameter")
        cols, shifts = _program_columns(program, col_ptrs, col_shifts)
        rep = AirCheckReport()
        _check(abi().bfhip_air_check(self._h, program._h, int(log_size), cols, shifts, *pars, ctypes.byref(rep)))
        return rep

    def logup_program_generate(self, program, log_size, col_ptrs, params, out_col_ptrs, col_shifts=None):
        """bfhip_logup_program_generate: the logUp interaction trace of a LogupProgram on CanonicCoset(log_size).circle_domain(). col_ptrs: one
        device column per program column (2^(log_size - shift) cells); params: QM31 values (4 words each); out_col_ptrs: 4 full-size
        coordinate columns per logUp column. Returns the claimed sum (4 u32). A zero denominator raises BfhipError naming fraction and cell."""
        pars = _qm31s(params, "a parameter")
        cols, shifts = _program_columns(program, col_ptrs, col_shifts)
        if len(out_col_ptrs) != 4 * program.shape["n_logup_cols"]:
            raise ValueError("4 coordinate columns per logUp column")
        claimed = (ctypes.c_uint32 * 4)()
        _check(abi().bfhip_logup_program_generate(self._h, program._h, int(log_size), cols, shifts, *pars, _ptr_array(out_col_ptrs), claimed))
        return list(claimed)

    def logup_program_generate_batch(self, components):
        """bfhip_logup_program_generate_batch: the logUp interaction trace of ALL components of an AIR in one call — one allocation, one
        row-stage launch for the components below 2^16 cells and one per larger one, three scan launches, one read-back. A component is
        (LogupProgram, log_size, col_ptrs, params, out_col_ptrs[, col_shifts]), each as for logup_program_generate; no output column may
        overlap another column of the list. Returns (claimed_sums, total): one claimed sum (4 u32) per component, word for word
        logup_program_generate's, and their QM31 sum. A zero denominator raises BfhipError naming the lowest such component, fraction, cell."""
        comps, keep = (LogupComponent * max(1, len(components)))(), []
        for k, comp in enumerate(components):
            program, log_size, col_ptrs, params, out_col_ptrs = comp[:5]
            cols, shifts = _program_columns(program, col_ptrs, comp[5] if len(comp) > 5 else None, "component %d: " % k)
            pars, n_params = _qm31s(params, "a parameter")
            if len(out_col_ptrs) != 4 * program.shape["n_logup_cols"]:
                raise ValueError("component %d: 4 coordinate columns per logUp column" % k)
            outs = _ptr_array(out_col_ptrs)
            keep += [cols, shifts, pars, outs, program]
            comps[k] = LogupComponent(program._h.value, int(log_size), n_params, None if cols is None else ctypes.cast(cols, ctypes.POINTER(ctypes.c_void_p)),
                                      shifts, pars, ctypes.cast(outs, ctypes.POINTER(ctypes.c_void_p)), 0)
        claimed, total = (ctypes.c_uint32 * (4 * max(1, len(components))))(), (ctypes.c_uint32 * 4)()
        _check(abi().bfhip_logup_program_generate_batch(self._h, comps, len(components), claimed, total))
        return [[int(claimed[4 * k + w]) for w in range(4)] for k in range(len(components))], list(total)

    def check_constraints(self, component, log_size, main_row_ptrs, logup_col_ptrs, lookup24, claimed4):
        """bfhip_check_constraints: one component's AIR asserted on its trace domain (stwo's assert_constraints). main_row_ptrs: row-granular
        main columns; logup_col_ptrs: what logup_generate wrote (the last four full size). Returns CheckReport.as_dict(); violations are
        a result, not an error."""
        rep = CheckReport()
        _check(abi().bfhip_check_constraints(self._h, component, log_size, _ptr_array(main_row_ptrs), _ptr_array(logup_col_ptrs),
                                             _u32s(lookup24), _u32s(claimed4), ctypes.byref(rep)))
        return rep.as_dict()

    def relation_summary(self, tables, max_entries=64):
        """bfhip_relation_summary: the lookup tuples that do not cancel over any list of 1..64 tables. tables: (component, log_size,
        main_row_ptrs) each — the row-granular device columns check_constraints takes; a component may be absent or repeated. Returns a
        RelationResult whose lines name table i as "<component name>[i]"; imbalances are a result, not an error."""
        n_main = (8, 8, 4, 9, 13, 13, 11, 11, 11, 11, 11, 11, 7)      # csrc/air.h: n_main_cols; the library reads that many pointers
        for comp, _, ptrs in tables:
            if ptrs is not None and 0 <= comp < 13 and len(ptrs) < n_main[comp]:
                raise BfhipError("relation summary: %s takes %d main columns, got %d" % (COMPONENT_NAMES[comp], n_main[comp], len(ptrs)))
        keep = [None if ptrs is None else _ptr_array(ptrs) for _, _, ptrs in tables]
        arr = (RelationTable * max(1, len(tables)))()
        for t, ((comp, log_size, _), ptrs) in enumerate(zip(tables, keep)):
            arr[t] = RelationTable(comp, log_size, None if ptrs is None else ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p)))
        names = ["%s[%d]" % (COMPONENT_NAMES[c] if 0 <= c < 13 else "?", t) for t, (c, _, _) in enumerate(tables)]
        return _relation_result(lambda reps, ents, cap: abi().bfhip_relation_summary(self._h, arr, len(tables), reps, ents, cap), max_entries, names)

    def _relation_program_tables(self, tables, relation_names, table_names, entry):
        """What the relation-program entries share. tables: (program, log_size, row_shift, col_ptrs[, col_shifts]) each. Returns (the
        RelationProgramTable array, the ctypes arrays it points into, n_relations, relation names, table names)."""
        if not tables:
            raise BfhipError("%s: 1 to 64 tables, got 0" % entry)
        n_rel = tables[0][0].shape["n_relations"]
        keep, arr = [], (RelationProgramTable * len(tables))()
        for t, tab in enumerate(tables):
            program, log_size, row_shift, ptrs = tab[:4]
            pa, sa = _program_columns(program, ptrs, tab[4] if len(tab) > 4 else None, "table %d: " % t)
            keep.append((pa, sa))
            arr[t] = RelationProgramTable(program._h, int(log_size), int(row_shift), None if pa is None else ctypes.cast(pa, ctypes.POINTER(ctypes.c_void_p)),
                                          None if sa is None else ctypes.cast(sa, ctypes.POINTER(ctypes.c_uint32)))
        rel_names = ["relation %d" % r for r in range(n_rel)] if relation_names is None else list(relation_names)
        if len(rel_names) != n_rel:
            raise ValueError("one name per relation")
        return arr, keep, n_rel, rel_names, ["table %d" % t for t in range(len(tables))] if table_names is None else list(table_names)

    def relation_program_summary(self, tables, max_entries=64, relation_names=None, table_names=None):
        """bfhip_relation_program_summary: the lookup tuples of ANY AIR that do not cancel — relation_summary for RelationPrograms. tables:
        (program, log_size, row_shift, col_ptrs) or (program, log_size, row_shift, col_ptrs, col_shifts) each: one device column per program
        column, the program evaluated once per 2^row_shift cells (row-granular Brainfuck tables: row_shift 4; full-size session columns: 0);
        col_shifts None = every column holds one word per evaluated row. All programs share one list of relations. Returns a RelationResult
        (reports and entries for every relation of the programs); relation_names default to "relation <r>", table_names to "table <t>";
        imbalances are a result, not an error. Refused while a PcsSession is open on the context: run it in front of the session."""
        arr, keep, n_rel, rel_names, tab_names = self._relation_program_tables(tables, relation_names, table_names, "bfhip_relation_program_summary")
        return _relation_result(lambda reps, ents, cap: abi().bfhip_relation_program_summary(self._h, arr, len(tables), n_rel, reps, ents, cap),
                                max_entries, tab_names, rel_names, n_rel)

    def relation_program_multiplicities(self, tables, relation, target_table, target_entry, out_ptr, max_missing=64, relation_names=None, table_names=None):
        """bfhip_relation_program_multiplicities: fills the multiplicity column of a looked-up table on the device. tables: as for
        relation_program_summary. The target — the table side of the lookup — is the target_entry-th ENTRY of `relation` (program order, from 0)
        in the program of tables[target_table]; its multiplicity operand is ignored. out_ptr: one word per evaluated row of that table (it may
        be the column that operand reads): the lowest row holding a tuple receives the net of every OTHER entry of the relation with that
        tuple, every other row 0. Returns a MultiplicityResult: the counts, and up to max_missing tuples with a non-zero net that no row of
        the target holds (a result, not an error). Refused while a PcsSession is open on the context: run it in front of the session."""
        arr, keep, n_rel, rel_names, tab_names = self._relation_program_tables(tables, relation_names, table_names, "bfhip_relation_program_multiplicities")
        rep = MultiplicityReport()
        miss = (RelationEntry * max_missing)() if max_missing else None
        _check(abi().bfhip_relation_program_multiplicities(self._h, arr, len(tables), n_rel, int(relation), int(target_table), int(target_entry), out_ptr,
                                                           ctypes.byref(rep), miss, max_missing))
        return MultiplicityResult(rep.as_dict(rel_names), [miss[i].as_dict(rel_names) for i in range(rep.n_reported)], tab_names, tab_names[rep.target_table])

    def accumulate_quotients(self, log_size, col_ptrs, n_samples, sample_points, sample_values, random_coeff4, out_ptrs, col_shifts=None):
        """QuotientOps::accumulate_quotients for the columns of one LDE size."""
        _check(abi().bfhip_accumulate_quotients(self._h, log_size, _ptr_array(col_ptrs), None if col_shifts is None else _u32s(col_shifts), len(col_ptrs),
                                                _u32s(n_samples), _u32s(sample_points), _u32s(sample_values), _u32s(random_coeff4),
                                                _ptr_array(out_ptrs)))

    def twiddles(self):
        tw, itw, rl = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32()
        _check(abi().bfhip_twiddles(self._h, ctypes.byref(tw), ctypes.byref(itw), ctypes.byref(rl)))
        return tw.value, itw.value, rl.value
