"""Fixed inputs of the Poseidon252 proof-of-work tests (test_grind_poseidon_cpu.py, test_gpu_grind_poseidon.py): the digests, the table of
smallest nonces from 0 (first computed with oracle/poseidon252.py; None = no hit below 30 000), the CPU oracle's grind under the Poseidon252
channel, and a restatement of Poseidon252Channel::trailing_zeros written here, over oracle/poseidon252.py's hades."""
import ctypes
import functools
import hashlib
import importlib.util
import os

from conftest import ROOT

spec = importlib.util.spec_from_file_location("poseidon252_oracle", os.path.join(ROOT, "oracle", "poseidon252.py"))
poseidon252 = importlib.util.module_from_spec(spec)
spec.loader.exec_module(poseidon252)
P252 = poseidon252.P

N_DIGESTS = 8
POW_BITS = (0, 1, 2, 3, 5, 8, 9, 12, 14, 16, 18, 20)


def digest_int(k):
    return int.from_bytes(hashlib.sha256(b"bfhip grind %d" % k).digest(), "big") % P252


def le32(v):
    return int(v).to_bytes(32, "little")


def digest(k):
    return le32(digest_int(k))


#      pow_bits:  3..8   9     12    14    16    18     20
_ROWS = {0: (6, 6, 149, 222, 512, 546, None),
         1: (19, 19, 364, 364, 2182, 7417, 20364),
         2: (5, 5, 37, 672, 4427, 4427, 13702),
         3: (4, 5, 91, 365, 5169, 14392, None),
         4: (1, 1, 93, 1285, 2240, 3039, None),
         5: (3, 5, 95, 272, 2967, 5926, 16880),
         6: (3, 3, 80, 498, 7619, 14513, 14513),
         7: (10, 24, 246, 435, 853, 853, 15596)}
_COLS = ((3, 4, 5, 6, 7, 8), (9,), (12,), (14,), (16,), (18,), (20,))
TABLE = {(k, pw): row[i] for k, row in _ROWS.items() for i, pws in enumerate(_COLS) for pw in pws if row[i] is not None}


def first_span(pow_bits):
    """Nonces per launch of bfhip_grind_poseidon252: 2^clamp(pow_bits - 4, 12, 20)."""
    return 1 << min(max(pow_bits - 4, 12), 20)


@functools.lru_cache(maxsize=None)
def _oracle_grind_cached(oracle, digest32, pow_bits):
    oracle.L.orc_grind_digest.restype = ctypes.c_uint64
    oracle.set_conventions(0, 0, 0, 1)        # Poseidon252 channel for this call only
    try:
        return oracle.L.orc_grind_digest(digest32, ctypes.c_uint32(pow_bits))
    finally:
        oracle.set_conventions(0, 0, 0, 0)


def oracle_grind(oracle, digest32, pow_bits):
    """orc_grind_digest under the Poseidon252 channel; the oracle's conventions are back at their defaults afterwards. Computed once per input."""
    return _oracle_grind_cached(oracle, bytes(digest32), pow_bits)


@functools.lru_cache(maxsize=None)
def trailing_zeros(d, nonce):
    """Poseidon252Channel::trailing_zeros of the digest after mix_u64(nonce): poseidon_hash(d, nonce) = hades([d, nonce, 2])[0], written big-endian;
    its first 16 bytes read as a little-endian u128; the trailing zeros of that (128 for 0)."""
    be = poseidon252.hades([d, nonce, 2])[0].to_bytes(32, "big")
    v = int.from_bytes(be[:16], "little")
    return 128 if v == 0 else (v & -v).bit_length() - 1


def assert_smallest(d, pow_bits, start_nonce, nonce):
    assert nonce >= start_nonce
    assert trailing_zeros(d, nonce) >= pow_bits, (hex(d), pow_bits, nonce)
    for n in range(start_nonce, nonce):
        assert trailing_zeros(d, n) < pow_bits, (hex(d), pow_bits, start_nonce, nonce, n)
