"""Commitment-scheme session (include/bfhip.h "Commitment-scheme session"): commit and open any AIR's columns — the channel, the prover
session of a context and the host-only verifier session."""
import ctypes

from ._abi import Owned, _check, _last_error, _ptr_array, _take_host_string, _u32s, abi
from ._abi_gen import (BFHIP_PCS_MAX_COLUMNS as PCS_MAX_COLUMNS, BFHIP_PCS_MAX_POINTS as PCS_MAX_POINTS,
                       BFHIP_PCS_MAX_SAMPLES_PER_COLUMN as PCS_MAX_SAMPLES_PER_COLUMN, BFHIP_PCS_MAX_TREES as PCS_MAX_TREES)
from .context import _conv_ref, _default_conventions, _pcs_ref


def _flat_samples(samples):
    """samples[tree][column] = list of point indices -> (n_samples per column, the indices flat), both as u32 arrays."""
    counts = [len(col) for tree in samples for col in tree]
    idx = [int(i) for tree in samples for col in tree for i in col]
    return _u32s(counts), _u32s(idx) if idx else None


def _flat_points(points):
    flat = [int(w) for p in points for w in p]
    if len(flat) != 8 * len(points):
        raise ValueError("a point is 8 words: x (4) then y (4)")
    return _u32s(flat) if flat else None


def circle_point_offset(point8, log_size, offset):
    """bfhip_circle_point_offset: point + offset * CanonicCoset(log_size).step() — the mask point of a column of 2^log_size rows at a row
    offset (offset -1: the previous row). Host only."""
    out = (ctypes.c_uint32 * 8)()
    _check(abi().bfhip_circle_point_offset(_u32s(point8), int(log_size), int(offset), out))
    return [int(v) for v in out]


class Channel(Owned):
    """bfhip_channel: Blake2sChannel::default() / Poseidon252Channel::default() (by conventions[3]) — what stwo passes as `channel` to
    commit, prove_values and verify_values. Host only. conventions: (merkle_node_hash, mix_u64, logup_mask_order, merkle_channel); None =
    the mirror's defaults."""
    _destroy = "bfhip_channel_destroy"

    def __init__(self, conventions=None):
        self._h = ctypes.c_void_p()
        self.conventions = tuple(_default_conventions if conventions is None else conventions)
        _check(abi().bfhip_channel_create(_conv_ref(self.conventions), ctypes.byref(self._h)))

    def mix_root(self, hash32):
        hash32 = bytes(hash32)
        if len(hash32) != 32:
            raise ValueError("a root is 32 bytes")
        _check(abi().bfhip_channel_mix_root(self._h, hash32))

    def mix_u64(self, value):
        _check(abi().bfhip_channel_mix_u64(self._h, int(value)))

    def mix_felts(self, felts):
        """felts: QM31 values, 4 canonical words each."""
        flat = [int(w) for q in felts for w in q]
        if len(flat) != 4 * len(felts):
            raise ValueError("a secure felt is 4 words")
        _check(abi().bfhip_channel_mix_felts(self._h, _u32s(flat) if flat else None, len(felts)))

    def draw_felts(self, n=1):
        """stwo's draw_felts(n): n QM31 values (lists of 4 words). n = 1 is draw_felt, n = 2 a lookup element's (z, alpha)."""
        out = (ctypes.c_uint32 * (4 * max(1, n)))()
        _check(abi().bfhip_channel_draw_felts(self._h, n, out))
        return [[int(out[4 * i + k]) for k in range(4)] for i in range(n)]

    def draw_felt(self):
        return self.draw_felts(1)[0]

    def draw_point(self):
        """CirclePoint::get_random_point: 8 words, x then y."""
        out = (ctypes.c_uint32 * 8)()
        _check(abi().bfhip_channel_draw_point(self._h, out))
        return [int(v) for v in out]

    def state(self):
        """(digest bytes, n_sent)"""
        d, n = (ctypes.c_uint8 * 32)(), ctypes.c_uint32()
        _check(abi().bfhip_channel_state(self._h, d, ctypes.byref(n)))
        return bytes(d), n.value

    def trailing_zeros(self):
        out = ctypes.c_uint32()
        _check(abi().bfhip_channel_trailing_zeros(self._h, ctypes.byref(out)))
        return out.value


class PcsSession(Owned):
    """bfhip_pcs: stwo's CommitmentSchemeProver on one Context — commit trees of arbitrary device columns, then open them at arbitrary
    points through the fused path of a Brainfuck proof. One open session per context; while it is open the context refuses its proving,
    checking and trace-building entries (include/bfhip.h lists them). close() (or the context manager) ends it."""
    _destroy = "bfhip_pcs_destroy"

    def __init__(self, ctx):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        _check(abi().bfhip_pcs_create(ctx._h, ctypes.byref(self._h)))
        self.roots, self.log_sizes = [], []

    def commit(self, channel, col_ptrs, log_sizes, form=0):
        """bfhip_pcs_commit: col_ptrs = device pointers, column k of 2^log_sizes[k] words. form 0 = evaluations (bit-reversed circle domain),
        1 = coefficients. Mixes the root into `channel` and returns it (32 bytes)."""
        if len(col_ptrs) != len(log_sizes):
            raise ValueError("one log size per column")
        root = (ctypes.c_uint8 * 32)()
        _check(abi().bfhip_pcs_commit(self._h, channel._h, _ptr_array(col_ptrs), _u32s(log_sizes), len(col_ptrs), int(form), root))
        self.roots.append(bytes(root))
        self.log_sizes.append([int(v) for v in log_sizes])
        return bytes(root)

    def tree_columns(self, tree):
        """bfhip_pcs_tree_columns: (coefficient pointers, LDE pointers) of a committed tree's columns, valid until close()."""
        n = ctypes.c_uint32()
        _check(abi().bfhip_pcs_tree_columns(self._h, int(tree), None, None, 0, ctypes.byref(n)))
        co, ev = (ctypes.c_void_p * max(1, n.value))(), (ctypes.c_void_p * max(1, n.value))()
        _check(abi().bfhip_pcs_tree_columns(self._h, int(tree), co, ev, n.value, ctypes.byref(n)))
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
        _check(abi().bfhip_pcs_prove_values(self._h, channel._h, _flat_points(points), len(points), counts, idx, out, ctypes.byref(js), ctypes.byref(n)))
        proof = _take_host_string(js, n.value)
        if with_sampled:
            return proof, [[int(out[4 * i + k]) for k in range(4)] for i in range(n_samples)]
        return proof


class PcsVerifier(Owned):
    """bfhip_pcs_verifier: stwo's CommitmentSchemeVerifier. Host only. conventions / pcs_config: what the proof was made under."""
    _destroy = "bfhip_pcs_verifier_destroy"

    def __init__(self, conventions=None, pcs_config=None):
        self._h = ctypes.c_void_p()
        _check(abi().bfhip_pcs_verifier_create(_conv_ref(conventions), _pcs_ref(pcs_config), ctypes.byref(self._h)))
        self.n_cols = []

    def commit(self, channel, root, log_sizes):
        """CommitmentSchemeVerifier::commit: the trace-domain log sizes of the tree's columns; mixes the root into `channel`."""
        root = bytes(root)
        if len(root) != 32:
            raise ValueError("a root is 32 bytes")
        _check(abi().bfhip_pcs_verifier_commit(self._h, channel._h, root, _u32s(log_sizes), len(log_sizes)))
        self.n_cols.append(len(log_sizes))

    def verify_values(self, channel, points, samples, proof_json):
        """(ok, reason): the description of PcsSession.prove_values; reason = the VerificationError name of a rejection."""
        if [len(t) for t in samples] != self.n_cols:
            raise ValueError("samples must list every column of every committed tree")
        counts, idx = _flat_samples(samples)
        err = ctypes.create_string_buffer(512)
        rc = abi().bfhip_pcs_verifier_verify_values(self._h, channel._h, _flat_points(points), len(points), counts, idx, proof_json, len(proof_json), err, 512)
        if rc < 0:
            raise _last_error()
        return rc == 0, err.value.decode()
