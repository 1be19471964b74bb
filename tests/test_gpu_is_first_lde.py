"""-m gpu parity: the preprocessed IsFirst columns in closed form — bfhip_is_first_lde (one launch writes the LDE of every size, no coefficients,
no transforms) word for word against bfhip_is_first_coeffs followed by bfhip_evaluate on the same context, and bfhip_is_first_eval_at_point against
bfhip_eval_at_point on the coefficient columns. Exact field arithmetic on canonical words: equality, no tolerance."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

LOG_MIN = 4
# where the closed-form kernel's paths change: one lane and no prefix layers (4), the first prefix layer (5), around one 4096-cell tile (11, 12), 13, 16,
# and 20 = where the reference path's two-pass transform plan starts
LOG_MAXES = (4, 5, 11, 12, 13, 16, 20)
BLOWUPS = (1, 2, 4)

_reference = {}      # (n, log_blowup) -> evaluate(is_first_coeffs(n)) on 2^(n + log_blowup) cells, computed once and shared by every case


def reference_lde(ctx, n, log_blowup):
    key = (n, log_blowup)
    if key not in _reference:
        coeffs, dst = ctx.malloc(4 << n), ctx.malloc(4 << (n + log_blowup))
        try:
            ctx.is_first_coeffs(n, n, [coeffs])
            ctx.evaluate([coeffs], [dst], n, n + log_blowup)
            ref = ctx.download(dst, 1 << (n + log_blowup))
        finally:
            ctx.free(coeffs); ctx.free(dst)
        ref.setflags(write=False)
        _reference[key] = ref
    return _reference[key]


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return "equal" if bad.size == 0 else "first difference at cell %d: got %d, want %d (%d cells differ)" % (bad[0], got[bad[0]], want[bad[0]], bad.size)


@pytest.mark.parametrize("log_blowup", BLOWUPS)
@pytest.mark.parametrize("log_max", LOG_MAXES)
def test_is_first_lde_equals_coefficients_then_evaluate(ctx, log_max, log_blowup):
    sizes = range(LOG_MIN, log_max + 1)
    ptrs = [ctx.malloc(4 << (n + log_blowup)) for n in sizes]
    try:
        ctx.is_first_lde(LOG_MIN, log_max, log_blowup, ptrs)
        for n, p in zip(sizes, ptrs):
            got = ctx.download(p, 1 << (n + log_blowup))
            assert got.max() < (1 << 31) - 1, "IsFirst(%d): a word outside [0, p)" % n
            want = reference_lde(ctx, n, log_blowup)
            assert np.array_equal(got, want), "IsFirst(%d) at log_blowup %d: %s" % (n, log_blowup, first_difference(got, want))
    finally:
        for p in ptrs:
            ctx.free(p)


def test_is_first_lde_skips_a_null_pointer_in_the_middle(ctx):
    log_max, log_blowup, hole = 13, 1, 8
    sizes = list(range(LOG_MIN, log_max + 1))
    ptrs = [ctx.malloc(4 << (n + log_blowup)) for n in sizes]
    # the skipped size's storage stays as it was, and so does what lies around the written columns
    marker = np.full(1 << (hole + log_blowup), 0x5A5A5A5A, dtype=np.uint32)
    keep = ctx.upload(marker)
    try:
        ctx.is_first_lde(LOG_MIN, log_max, log_blowup, [None if n == hole else p for n, p in zip(sizes, ptrs)])
        assert np.array_equal(ctx.download(keep, marker.size), marker)
        for n, p in zip(sizes, ptrs):
            if n == hole:
                continue
            got = ctx.download(p, 1 << (n + log_blowup))
            want = reference_lde(ctx, n, log_blowup)
            assert np.array_equal(got, want), "IsFirst(%d) beside the skipped size: %s" % (n, first_difference(got, want))
    finally:
        for p in ptrs + [keep]:
            ctx.free(p)


def test_is_first_lde_refuses_what_is_first_coeffs_refuses(ctx):
    # below 4, reversed, 28 sizes or more, past any twiddle tree by size and by blowup. Every pointer is null: a call that got through would write nothing
    for lo, hi, b in ((3, 5, 1), (6, 5, 1), (4, 32, 1), (4, 30, 1), (4, 5, 40)):
        with pytest.raises(Exception):
            ctx.is_first_lde(lo, hi, b, [None] * max(1, hi - lo + 1))


# two points with all four QM31 coordinates of x and of y non-zero (the product form is an identity in (x, y): the points need not lie on the circle)
POINTS = (
    [0x12345678, 0x0FEDCBA9, 0x2468ACE1, 0x13579BDF, 0x7654321, 0x1ABCDEF0, 0x3C3C3C3C, 0x55AA55AA],
    [0x7FFFFFFE, 1, 0x40000000, 0x3FFFFFFF, 2, 0x7FFFFFFD, 0x00010001, 0x7FFF0000],
)


@pytest.mark.parametrize("n", (4, 5, 12, 20))
def test_is_first_sample_closed_form_equals_eval_at_point(ctx, n):
    coeffs = ctx.malloc(4 << n)
    try:
        ctx.is_first_coeffs(n, n, [coeffs])
        for point in POINTS:
            want = ctx.eval_at_point(coeffs, n, point)
            got = ctx.is_first_eval_at_point(n, point)
            assert got == want, "IsFirst(%d) at %s: got %s, want %s" % (n, point, got, want)
    finally:
        ctx.free(coeffs)
