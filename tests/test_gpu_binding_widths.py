"""-m gpu: the Python mirror passes 64-bit scalars and device pointers at their full width through the typed handle — the smallest
cases in which a by-value argument narrowed to a C int would show."""
import ctypes

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

LOG_MAX_ROWS = 14      # the smallest the pool tests use (tests/test_gpu_pool_queue.py: LO)


def test_pool_tag_above_2_to_the_32_comes_back_whole(pkg, conv):
    tag = (1 << 40) + 5
    pool = pkg.Pool(0, n_in_flight=1, max_log_domain=LOG_MAX_ROWS + 2)
    try:
        ticket = pool.submit_program("+", log_max_rows=LOG_MAX_ROWS, tag=tag)
        r = pool.wait(timeout_s=120)
        assert r is not None and r.ticket == ticket and r.tag == tag and r.status == 0 and r.ok, r
        assert pkg.verify_brainfuck(r.proof, LOG_MAX_ROWS) == (True, "")
        assert pool.wait(timeout_s=0) is None
    finally:
        pool.close()


def test_grind_start_nonce_above_2_to_the_32(pkg, ctx):
    start = (1 << 33) + 1
    nonce, tried = ctx.grind_poseidon252(bytes(32), pow_bits=4, start_nonce=start, with_tried=True)
    assert nonce >= start
    raw_nonce, raw_tried = ctypes.c_uint64(), ctypes.c_uint64()
    assert pkg.lib().bfhip_grind_poseidon252(ctx._h, bytes(32), ctypes.c_uint32(4), ctypes.c_uint64(start), ctypes.byref(raw_nonce), ctypes.byref(raw_tried)) == 0
    assert (nonce, tried) == (raw_nonce.value, raw_tried.value)


def test_buffer_and_gather_round_trip(ctx):
    """Device pointers (above 2^32 on this GPU's address map) and size_t lengths through upload, gather, download and free."""
    rng = np.random.default_rng(20250)
    words = rng.integers(0, 1 << 31, size=1 << 10, dtype=np.uint32)
    idx = rng.integers(0, words.size, size=16)
    ptr = ctx.upload(words)
    try:
        assert ptr > 1 << 32, hex(ptr)
        assert np.array_equal(ctx.gather(ptr, idx), words[idx])
        assert np.array_equal(ctx.download(ptr, words.size), words)
    finally:
        ctx.free(ptr)
