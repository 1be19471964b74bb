"""The FRI commit phase over numpy columns: the model bfhip_test_fri_commit (libbfhip_testhooks.so) is compared against. Restates
FriProver::commit as the oracle's prover runs it (oracle/prover.h, "FriProver::commit" down to the last layer) from pieces that have pins of
their own: the folds are orc_fold_circle_into_line / orc_fold_line, the trees orc_merkle_commit with every level kept, and the Blake2s channel
is hashlib — mix_root = blake2s(digest || root), draw = blake2s(digest || LE32(n_sent) || 28 zero bytes), redrawn while a word is >= 2P, words
mod P. It starts from any digest, takes any columns (nothing here asks for a low degree: the last layer is returned as it is, no polynomial is
made of it) and never runs a proof. Under the Poseidon252 channel the oracle's own channel primitives step it, from the zero digest."""
import ctypes
import hashlib
import struct

import numpy as np

P = (1 << 31) - 1


def mix_root(digest, root):
    return hashlib.blake2s(digest + root).digest()


def draw_words(digest, n_sent):
    """One draw: the 8 words of blake2s(digest || LE32(n_sent) || zero padding to 64 bytes)."""
    return struct.unpack("<8I", hashlib.blake2s(digest + struct.pack("<I", n_sent) + bytes(28)).digest())


def draw_felt(digest):
    """Blake2sChannel::draw_felt right behind a mix: (the first 4 words mod P, n_sent afterwards = the number of draws it took)."""
    n_sent = 0
    while True:
        w = draw_words(digest, n_sent)
        n_sent += 1
        if all(x < 2 * P for x in w):
            return [x % P for x in w[:4]], n_sent


def qm31_mul(x, y):
    """(a0 + a1 i + (a2 + a3 i) u)(b0 + b1 i + (b2 + b3 i) u), i^2 = -1, u^2 = 2 + i, over Python integers."""
    a0, a1, a2, a3 = [int(v) for v in x]
    b0, b1, b2, b3 = [int(v) for v in y]
    cm = lambda p, q, r, s: (p * r - q * s, p * s + q * r)
    aa, bb, ab, ba = cm(a0, a1, b0, b1), cm(a2, a3, b2, b3), cm(a0, a1, b2, b3), cm(a2, a3, b0, b1)
    return [(aa[0] + 2 * bb[0] - bb[1]) % P, (aa[1] + bb[0] + 2 * bb[1]) % P, (ab[0] + ba[0]) % P, (ab[1] + ba[1]) % P]


def pattern_sizes(pattern, line_log, log_blowup):
    """log sizes of the quotient columns, descending. "every": line_log + 1 down to log_blowup + 4, as in a proof (IsFirst has every size);
    "largest": the first only, every later layer is folded without a quotient; "every_other": every second size."""
    every = list(range(line_log + 1, log_blowup + 3, -1)) or [line_log + 1]
    return {"every": every, "largest": every[:1], "every_other": every[::2]}[pattern]


def quotient_columns(family, sizes, seed=0):
    """[(log_size, 4 coordinate columns)] of the family f(seed, n) -> uint32[n]; seeds differ per size and coordinate."""
    return [(lg, [family(seed + 64 * lg + 8 * j, 1 << lg) for j in range(4)]) for lg in sizes]


def _ptrs(cols):
    return (ctypes.c_void_p * len(cols))(*[c.ctypes.data for c in cols])


def merkle_commit(L, cols, logs):
    """(root, every level of the tree deepest first as one (n_nodes, 8) word array): orc_merkle_commit with layers_out."""
    max_log = max(logs)
    out = np.zeros(((2 << max_log) - 1, 8), dtype=np.uint32)
    root = (ctypes.c_ubyte * 32)()
    rc = L.orc_merkle_commit(_ptrs(cols), (ctypes.c_uint32 * len(logs))(*logs), ctypes.c_size_t(len(logs)), root, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, L.orc_last_error()
    return bytes(root), out


class _Blake2sChannel:
    def __init__(self, digest):
        self.digest, self.n_sent = bytes(digest), 0

    def step(self, root):
        """mix_root(root), draw_felt(): the drawn alpha."""
        self.digest = mix_root(self.digest, root)
        alpha, self.n_sent = draw_felt(self.digest)
        return alpha


class _OracleChannel:
    """The oracle's channel under its current conventions (Poseidon252Channel when merkle_channel is 1); n_sent is not exposed."""

    def __init__(self, L):
        L.orc_channel_new.restype = ctypes.c_void_p
        self.L, self.h, self.n_sent = L, ctypes.c_void_p(L.orc_channel_new()), None

    def step(self, root):
        out = (ctypes.c_uint32 * 4)()
        self.L.orc_channel_mix_root(self.h, root)
        self.L.orc_channel_draw_felt(self.h, out)
        return list(out)

    @property
    def digest(self):
        d = (ctypes.c_ubyte * 32)()
        self.L.orc_channel_digest(self.h, d)
        return bytes(d)

    def close(self):
        self.L.orc_channel_free(self.h)


def commit(L, quotients, log_blowup, digest=bytes(32), oracle_channel=False):
    """quotients: [(log_size, [4 coordinate columns])], sizes distinct and descending; the last layer has 2^log_blowup rows.
    Returns {"layers": the line layers 0 .. last as (4, n) arrays (the last one = the 2^log_blowup evaluations left over),
    "trees": [first-layer tree, inner layer 0's, ..] each (n_nodes, 8) deepest level first, "roots": their roots,
    "alphas": (n_steps, 8) alpha || alpha^2 per channel step, "digest": the channel's digest at the end, "n_sent": its counter (None under
    the oracle's channel), "draws": per step how many draws its draw_felt took (Blake2s channel)}."""
    ch = _OracleChannel(L) if oracle_channel else _Blake2sChannel(digest)
    if oracle_channel:
        assert digest == bytes(32)
    quotients = [(lg, [np.ascontiguousarray(c, dtype=np.uint32) for c in cols]) for lg, cols in quotients]
    u4 = lambda a: (ctypes.c_uint32 * 4)(*[int(v) for v in a])
    trees, roots, alphas, draws, layers = [], [], [], [], []

    def step(root, tree):
        roots.append(root); trees.append(tree)
        a = ch.step(root)
        alphas.append(a + qm31_mul(a, a)); draws.append(ch.n_sent)
        return a

    root, tree = merkle_commit(L, [c for _, cols in quotients for c in cols], [lg for lg, cols in quotients for _ in cols])
    alpha = step(root, tree)
    line_log = quotients[0][0] - 1
    layer = [np.zeros(1 << line_log, dtype=np.uint32) for _ in range(4)]
    qi = 0
    while line_log > log_blowup:
        if qi < len(quotients) and quotients[qi][0] - 1 == line_log:
            assert L.orc_fold_circle_into_line(_ptrs(layer), _ptrs(quotients[qi][1]), line_log + 1, u4(alpha)) == 0
            qi += 1
        layers.append(np.stack(layer))
        root, tree = merkle_commit(L, layer, [line_log] * 4)
        alpha = step(root, tree)
        nxt = [np.zeros(1 << (line_log - 1), dtype=np.uint32) for _ in range(4)]
        assert L.orc_fold_line(_ptrs(layer), line_log, u4(alpha), _ptrs(nxt)) == 0
        layer = nxt
        line_log -= 1
    assert qi == len(quotients), "not all columns consumed"
    layers.append(np.stack(layer))
    out = {"layers": layers, "trees": trees, "roots": roots, "alphas": np.array(alphas, dtype=np.uint32), "digest": ch.digest, "n_sent": ch.n_sent, "draws": draws}
    if oracle_channel:
        ch.close()
    return out
