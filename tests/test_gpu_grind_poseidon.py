"""-m gpu: bfhip_grind_poseidon252 (GrindOps::grind for Poseidon252Channel) against the CPU oracle's grind under the Poseidon252 channel, the
table of tests/grind_poseidon_cases.py, and a restatement of the channel's trailing_zeros over oracle/poseidon252.py's hades."""
import ctypes
import hashlib

import pytest

from grind_poseidon_cases import N_DIGESTS, P252, POW_BITS, TABLE, assert_smallest, digest, digest_int, first_span, le32, oracle_grind

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

# nonces beyond the first launch's span (4096 at pow_bits 16): 4427, 5169, 7619
MULTI_LAUNCH = [(2, 16), (3, 16), (6, 16)]


@pytest.mark.parametrize("pow_bits", POW_BITS)
def test_nonce_equals_the_oracles_and_the_table(ctx, oracle, pow_bits):
    for k in range(N_DIGESTS):
        want = oracle_grind(oracle, digest(k), pow_bits)
        got, tried = ctx.grind_poseidon252(digest(k), pow_bits, with_tried=True)
        print(f"d{k} pow_bits {pow_bits}: nonce {got} (oracle {want}, table {TABLE.get((k, pow_bits))}), tried {tried}")
        assert got == want, (k, pow_bits)
        if (k, pow_bits) in TABLE:
            assert got == TABLE[(k, pow_bits)], (k, pow_bits)
        span = first_span(pow_bits)
        assert tried % span == 0 and tried == (got // span + 1) * span, (k, pow_bits, got, tried)
        if pow_bits <= 12:
            assert_smallest(digest_int(k), pow_bits, 0, got)


def test_at_least_three_cases_need_more_than_one_launch(ctx):
    assert len(MULTI_LAUNCH) >= 3
    for k, pow_bits in MULTI_LAUNCH:
        assert TABLE[(k, pow_bits)] >= first_span(pow_bits)
        got, tried = ctx.grind_poseidon252(digest(k), pow_bits, with_tried=True)
        assert got == TABLE[(k, pow_bits)]
        assert tried > first_span(pow_bits), (k, pow_bits, tried)


def test_pow_bits_3_to_8_agree_and_pow_bits_0_returns_the_start(ctx):
    """The channel reads the big-endian top bytes, so three zero bits imply eight: one nonce for pow_bits 3..8. A launch holds many hits at
    these pow_bits (every lane at pow_bits 0) and keeps the minimum."""
    for k in range(N_DIGESTS):
        got = [ctx.grind_poseidon252(digest(k), pw) for pw in (3, 4, 5, 6, 7, 8)]
        assert got == [TABLE[(k, 8)]] * 6, (k, got)
        for start in (0, 1, 4095, 4097, (1 << 32) - 1, (1 << 63) + 5):
            assert ctx.grind_poseidon252(digest(k), 0, start_nonce=start) == start


@pytest.mark.parametrize("start,pow_bits", [((1 << 32) - 100, 12), ((1 << 40) + 12345, 9)])
def test_64_bit_nonces_and_unaligned_starts(ctx, start, pow_bits):
    for k in range(4):
        got = ctx.grind_poseidon252(digest(k), pow_bits, start_nonce=start)
        print(f"d{k} pow_bits {pow_bits} from {start}: {got}")
        assert_smallest(digest_int(k), pow_bits, start, got)


def test_start_at_the_known_nonce_and_just_after_it(ctx):
    for k in range(4):
        for pow_bits in (9, 12):
            known = TABLE[(k, pow_bits)]
            assert ctx.grind_poseidon252(digest(k), pow_bits, start_nonce=known) == known
            nxt = ctx.grind_poseidon252(digest(k), pow_bits, start_nonce=known + 1)
            assert nxt > known
            assert_smallest(digest_int(k), pow_bits, known + 1, nxt)


def test_edge_digests(ctx, oracle):
    for d in (0, P252 - 1):
        got = ctx.grind_poseidon252(le32(d), 9)
        assert got == oracle_grind(oracle, le32(d), 9), hex(d)
        assert_smallest(d, 9, 0, got)


def test_refusals_leave_the_context_usable(pkg, ctx):
    for bad in (P252, (1 << 256) - 1):
        with pytest.raises(pkg.BfhipError, match="not a canonical felt252"):
            ctx.grind_poseidon252(le32(bad), 9)
    with pytest.raises(pkg.BfhipError, match="pow_bits"):
        ctx.grind_poseidon252(digest(0), 33)
    with pytest.raises(pkg.BfhipError, match="wrap past 2\\^64"):
        ctx.grind_poseidon252(digest(0), 12, start_nonce=(1 << 64) - 10)
    L = pkg.lib()
    nonce, tried = ctypes.c_uint64(), ctypes.c_uint64()
    args = lambda h, d, n: (h, d, ctypes.c_uint32(9), ctypes.c_uint64(0), n, ctypes.byref(tried))
    for call in (args(None, digest(0), ctypes.byref(nonce)), args(ctx._h, None, ctypes.byref(nonce)), args(ctx._h, digest(0), None)):
        assert L.bfhip_grind_poseidon252(*call) == -1
        assert b"null" in L.bfhip_last_error()
    assert L.bfhip_grind_poseidon252(ctx._h, digest(0), ctypes.c_uint32(9), ctypes.c_uint64(0), ctypes.byref(nonce), None) == 0     # tried may be NULL
    assert nonce.value == TABLE[(0, 9)]
    assert ctx.grind_poseidon252(digest(1), 12) == TABLE[(1, 12)]


def test_the_contexts_conventions_do_not_matter(ctx):
    cases = [(k, pw) for k in range(4) for pw in (9, 14)]
    try:
        ctx.set_conventions(0, 0, 0, 1)
        as_poseidon = [ctx.grind_poseidon252(digest(k), pw) for k, pw in cases]
        ctx.set_conventions(1, 1, 1, 0)
        as_blake = [ctx.grind_poseidon252(digest(k), pw) for k, pw in cases]
    finally:
        ctx.set_conventions(0, 0, 0, 0)
    assert as_poseidon == as_blake == [TABLE[c] for c in cases]


def test_the_blake2s_grind_is_untouched(ctx):
    digests = [hashlib.blake2s(b"bfhip grind poseidon independence %d" % i).digest() for i in range(2)]
    before = [ctx.grind(d, 14) for d in digests]
    assert ctx.grind_poseidon252(digest(5), 16) == TABLE[(5, 16)]
    assert [ctx.grind(d, 14) for d in digests] == before
