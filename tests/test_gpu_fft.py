"""-m gpu parity: circle iFFT / FFT through the C ABI against the oracle, bit-exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fft_plan_model as fm
import field_inputs as fi
from conftest import ROOT, splitmix_column, P

pytestmark = pytest.mark.gpu

# Index-only mutations of the column loop, each built on a scratch copy and run on an MI355X, one at a time, against the tests of the section
# "many columns per workgroup" below and tests/test_gpu_pcs_commit_large.py ("new") and against the op-level modules as they were before
# ("old": the other tests of this module, tests/test_gpu_field_edges.py). Every mutant stays inside the buffers of its launch: it reads another
# column of the same size or writes fewer columns.
MUTATIONS = """
1 k_fft_tile12, column loop: the next column's tile is fetched from a.src[col0] instead of a.src[col + 1]
    new: caught by test_many_columns_per_workgroup at all six rows (every second column of a block of 2, columns 1, 2 and 4 of 5 under blocks of 3 / 5:
         "first difference at (column, index) = (1, 0) of the max column"; at (23, 2) column 1, the edge column), by both
         test_many_columns_under_larger_blowups cases, and by every session of test_gpu_pcs_commit_large.py (an LDE column of the largest class;
         b1_top22 already at the coefficients)
    old: caught at the one shape where a block walks 2 columns — the evaluate to 2^23 of test_fft_matches_oracle_at_proof_sizes[22-2] and of
         test_gpu_field_edges.py::test_interpolate_then_evaluate[22] (2048 tiles: cols_per_block = ncols = 2, "evaluate mismatch at log 22", no column
         named) — and by the linearity check of test_three_strided_pass_plan_identity_and_linearity (3 columns of 2^27 in one block); 76 + 225 others passed
2 k_fft_stridedK, column loop: src = a.src[col0] instead of a.src[col]
    new: caught by test_many_columns_per_workgroup[20-17], [21-9], [22-5] (K = 8, 9, 10; interpolate, column 1 = the max column named) and by
         test_gpu_pcs_commit_large.py[b1_top22] (coefficients of a 2^21 column); the other sessions pass: no trace of theirs runs 20 layers
    old: caught at the same one shape as mutant 1 (evaluate 2^22 -> 2^23 with 2 columns, K = 10), in the same two tests; K = 8 and 9 and every
         inverse stridedK pass: missed
3 fft_plan, fast path: gy = ncols / cpb instead of the ceiling (the shorter last column block is never launched)
    new: caught by test_many_columns_per_workgroup at the five rows with a shorter last block ("(64, 0) of the edge column ... 1 of 65 columns differ";
         (22, 5): columns 3 and 4), passes at (23, 2) as it must (one block, no shorter one); by both larger-blowup cases; by every session of
         test_gpu_pcs_commit_large.py; and by test_library_launches_what_the_plan_model_says (b2048 against the model's b2112 at (18, 65))
    old: missed (78 + 226 passed)
"""


def _roundtrip(ctx, oracle, log, ncols, seed):
    cols = np.stack([splitmix_column(0x5EED0000 + seed + c, 1 << log) for c in range(ncols)])
    ptrs = [ctx.upload(cols[c]) for c in range(ncols)]
    ctx.interpolate(ptrs, ptrs, log)
    got = np.stack([ctx.download(p, 1 << log) for p in ptrs])
    want = oracle.interpolate(cols, log)
    assert np.array_equal(got, want), f"interpolate mismatch at log {log}"
    lde = [ctx.malloc(4 << (log + 1)) for _ in range(ncols)]
    ctx.evaluate(ptrs, lde, log, log + 1)
    got2 = np.stack([ctx.download(p, 1 << (log + 1)) for p in lde])
    want2 = oracle.evaluate(want, log, log + 1)
    assert np.array_equal(got2, want2), f"evaluate mismatch at log {log}"
    for p in ptrs + lde:
        ctx.free(p)


@pytest.mark.parametrize("log", [3, 4, 5, 6, 7, 9, 11, 12, 13, 14, 16, 19, 20, 21])
def test_fft_matches_oracle(ctx, oracle, log):
    _roundtrip(ctx, oracle, log, 3 if log < 19 else 2, seed=log * 16)


def test_fft_large_identity(ctx):
    """Size-independent property at a large size: evaluate(interpolate(f)) on the same domain == f."""
    log = 23
    col = splitmix_column(0x5EED0000, 1 << log)
    p = ctx.upload(col)
    q = ctx.malloc(4 << log)
    ctx.interpolate([p], [q], log)
    ctx.evaluate([q], [q], log, log)
    assert np.array_equal(ctx.download(q, 1 << log), col)
    ctx.free(p); ctx.free(q)


@pytest.mark.parametrize("log", [4, 5, 6, 8, 10, 13, 17, 20])
def test_replicated_column_matches_full_transform(ctx, oracle, log):
    """A row-granular ("replicated") transform equals the full circle transform of the 16x-broadcast column (memory/table.rs:95-104)."""
    rows = splitmix_column(0xABC0 + log, 1 << (log - 4))
    full = np.repeat(rows, 16)[None, :]
    want_coeffs = oracle.interpolate(full, log)[0]
    p = ctx.upload(rows)
    ctx.interpolate([p], [p], log, replicated=True)
    got = ctx.download(p, 1 << (log - 4))
    assert np.array_equal(got, want_coeffs[::16])
    assert not np.any(want_coeffs.reshape(-1, 16)[:, 1:])  # all other coefficients vanish
    q = ctx.malloc(4 << (log - 3))
    ctx.evaluate([p], [q], log, log + 1, replicated=True)
    got_lde = ctx.download(q, 1 << (log - 3))
    want_lde = oracle.evaluate(want_coeffs[None, :], log, log + 1)[0]
    assert np.array_equal(np.repeat(got_lde, 16), want_lde)
    ctx.free(p); ctx.free(q)


@pytest.mark.single_conv
@pytest.mark.parametrize("log,ncols", [(22, 2), (24, 1)])
def test_fft_matches_oracle_at_proof_sizes(pkg, _oracle, log, ncols):
    """Op-level parity at the sizes of the benchmark proof (2^22, and one column at 2^24 -> LDE 2^25): bit-exact vs the oracle's CPU
    transform (seconds per column), not only through the proof digest."""
    c = pkg.Context(0, max_log_domain=log + 1)
    try:
        _roundtrip(c, _oracle, log, ncols, seed=log * 16 + 1)
    finally:
        c.close()


@pytest.mark.single_conv
def test_three_strided_pass_plan_identity_and_linearity(pkg):
    """A context with max_log_domain 29 and one column of 2^27 cells: the plan with three strided passes (only reached above 2^26) —
    evaluate(interpolate(f)) == f on the same domain, and interpolate is linear: interpolate(f + g) == interpolate(f) + interpolate(g)."""
    log = 27
    c = pkg.Context(0, max_log_domain=29)
    try:
        f = splitmix_column(0x5EED0001, 1 << log); g = splitmix_column(0x5EED0002, 1 << log)
        fg = ((f.astype(np.uint64) + g) % P).astype(np.uint32)
        pf, pg, pfg = c.upload(f), c.upload(g), c.upload(fg)
        q = c.malloc(4 << log)
        c.interpolate([pf], [q], log)
        c.evaluate([q], [q], log, log)
        assert np.array_equal(c.download(q, 1 << log), f)
        c.interpolate([pf, pg, pfg], [pf, pg, pfg], log)
        cf, cg, cfg_ = c.download(pf, 1 << log), c.download(pg, 1 << log), c.download(pfg, 1 << log)
        assert np.array_equal(((cf.astype(np.uint64) + cg) % P).astype(np.uint32), cfg_)
        # LDE to 2^28 and back: the low half of interpolate(evaluate_2N(coeffs)) are the coefficients, the high half is zero
        lde = c.malloc(4 << (log + 1))
        c.evaluate([pf], [lde], log, log + 1)
        c.interpolate([lde], [lde], log + 1)
        back = c.download(lde, 1 << (log + 1))
        assert np.array_equal(back[: 1 << log], cf) and not back[1 << log:].any()
        for p_ in (pf, pg, pfg, q, lde):
            c.free(p_)
    finally:
        c.close()


def test_is_first_coefficients_closed_form(ctx, oracle):
    """bfhip_is_first_coeffs (one launch, no transform) == interpolate(gen_is_first(n)) (mod.rs:497): against the oracle's transform of the
    one-hot column for the small sizes and against this library's own transform of it for every size up to the context's limit."""
    lo, hi = 4, 21
    ptrs = [ctx.malloc(4 << n) for n in range(lo, hi + 1)]
    ctx.is_first_coeffs(lo, hi, ptrs)
    for n in range(lo, hi + 1):
        got = ctx.download(ptrs[n - lo], 1 << n)
        one_hot = np.zeros(1 << n, dtype=np.uint32); one_hot[0] = 1
        if n <= 16:
            assert np.array_equal(got, oracle.interpolate(one_hot[None, :], n)[0]), n
        p = ctx.upload(one_hot)
        ctx.interpolate([p], [p], n)
        assert np.array_equal(got, ctx.download(p, 1 << n)), n
        ctx.free(p)
    # a skipped size stays untouched
    keep = ctx.upload(np.full(1 << 6, 7, dtype=np.uint32))
    ctx.is_first_coeffs(5, 7, [ptrs[1], None, ptrs[3]])
    assert (ctx.download(keep, 1 << 6) == 7).all()
    for p in ptrs + [keep]:
        ctx.free(p)


def test_transform_batches_with_many_sizes_in_one_call(pkg, oracle):
    """fft_plan packs the passes of every size group of a call into one launch per pass and kernel kind: a proof with 13 components of 10
    distinct sizes exercises it end to end (test_gpu_prove); here the planner's group table is driven directly through two contexts'
    worth of sizes — each size alone must equal the same size inside a mixed batch (results may not depend on the batch composition)."""
    c = pkg.Context(0, max_log_domain=22)
    try:
        for log in (5, 9, 12, 13, 18, 20):
            cols = np.stack([splitmix_column(0x77000 + log * 8 + k, 1 << log) for k in range(3)])
            ptrs = [c.upload(cols[k]) for k in range(3)]
            c.interpolate(ptrs, ptrs, log)
            got = np.stack([c.download(p, 1 << log) for p in ptrs])
            if log <= 18:
                assert np.array_equal(got, oracle.interpolate(cols, log)), log
            for p in ptrs:
                c.free(p)
    finally:
        c.close()


# ---- many columns per workgroup ------------------------------------------------------------------------------------------------------------
# One workgroup of k_fft_tile12 / k_fft_strided7 / k_fft_stridedK stages a tile's twiddles once and walks cols_per_block columns through the
# same LDS buffer; fft_plan gives cols_per_block >= 2 only when the tiles alone are fewer than 2048 workgroups' worth for the column count
# (tests/fft_plan_model.py restates the rule; tests/test_fft_plan_model_cpu.py holds every case below to the path it is named for).
@pytest.fixture(scope="module")
def big_ctx(pkg):
    c = pkg.Context(0, max_log_domain=24)
    yield c
    c.close()


def _labelled_columns(seed, ncols, n):
    """Columns that can be told apart: column c is uniform with a seed of its own (seeds further apart than any column is long), but for one
    column of all P - 1 in the first column block (column 1; column 0 of a pair) and one edge column at the end of the last block.
    Returns (columns, family of every column)."""
    fams = ["uniform"] * ncols
    fams[1 if ncols > 2 else 0] = "max"
    fams[ncols - 1] = "edge"
    return np.stack([fi.column(f, seed + (c << 32), n) for c, f in enumerate(fams)]), fams


def _assert_columns_equal(got, want, fams, what):
    if np.array_equal(got, want):
        return
    cols = np.nonzero((got != want).any(axis=1))[0]
    c = int(cols[0])
    i = int(np.nonzero(got[c] != want[c])[0][0])
    raise AssertionError("%s: first difference at (column, index) = (%d, %d) of the %s column: %d against %d; %d of %d columns differ: %s" % (
        what, c, i, fams[c], got[c][i], want[c][i], cols.size, got.shape[0], cols[:12].tolist()))


def _interpolate(ctx, oracle, cols, fams, log, what):
    """(device pointers holding the coefficients, the oracle's coefficients)"""
    ptrs = [ctx.upload(c) for c in cols]
    ctx.interpolate(ptrs, ptrs, log)
    got = np.stack([ctx.download(p, 1 << log) for p in ptrs])
    want = oracle.interpolate(cols, log)
    _assert_columns_equal(got, want, fams, "interpolate %s" % (what,))
    m = fams.index("max")         # closed form, independent of the oracle: a constant column has one coefficient
    assert got[m][0] == P - 1 and not got[m][1:].any(), what
    return ptrs, want


def _evaluate(ctx, oracle, ptrs, coeffs, fams, log, log_eval, what):
    lde = [ctx.malloc(4 << log_eval) for _ in ptrs]
    ctx.evaluate(ptrs, lde, log, log_eval)
    got = np.stack([ctx.download(p, 1 << log_eval) for p in lde])
    for p in ptrs + lde:
        ctx.free(p)
    _assert_columns_equal(got, oracle.evaluate(coeffs, log, log_eval), fams, "evaluate %s" % (what,))
    return got


@pytest.mark.single_conv
@pytest.mark.parametrize("log,ncols", list(fm.MANY_COLUMNS), ids=lambda v: str(v))
def test_many_columns_per_workgroup(big_ctx, oracle, log, ncols):
    """The rows of fft_plan_model.MANY_COLUMNS: cols_per_block 2, 3 and 5 with a shorter last block, and every column in one block, under
    tile12 with k0 = 9, 11 and 12, the narrow and the wide strided7, stridedK<8>, <9> and <10> and the plan with two strided passes —
    interpolate, then evaluate to the next level, each against the oracle."""
    cols, fams = _labelled_columns(0x6C0000 + log, ncols, 1 << log)
    ptrs, coeffs = _interpolate(big_ctx, oracle, cols, fams, log, (log, ncols))
    got = _evaluate(big_ctx, oracle, ptrs, coeffs, fams, log, log + 1, (log, log + 1, ncols))
    assert (got[fams.index("max")] == P - 1).all()


@pytest.mark.single_conv
@pytest.mark.parametrize("log,log_eval,ncols", list(fm.LARGER_BLOWUPS), ids=lambda v: str(v))
def test_many_columns_under_larger_blowups(big_ctx, oracle, log, log_eval, ncols):
    """The shapes log_blowup_factor 4 gives a tree of many columns: the wide strided7 pass over layers [9, 16) and [11, 18) of a transform whose
    upper layers only duplicate, with a shorter last column block."""
    coeffs, fams = _labelled_columns(0x6D0000 + log, ncols, 1 << log)
    ptrs = [big_ctx.upload(c) for c in coeffs]
    _evaluate(big_ctx, oracle, ptrs, coeffs, fams, log, log_eval, (log, log_eval, ncols))


@pytest.mark.single_conv
@pytest.mark.parametrize("log", fm.BETWEEN_SIZES)
def test_sizes_between_the_visited_ones(big_ctx, oracle, log):
    """k0 = 8, 10 and 11 in front of one strided pass: the inverse sizes no other test compares with the oracle."""
    cols, fams = _labelled_columns(0x6E0000 + log, fm.BETWEEN_COLUMNS, 1 << log)
    ptrs, coeffs = _interpolate(big_ctx, oracle, cols, fams, log, (log, len(cols)))
    _evaluate(big_ctx, oracle, ptrs, coeffs, fams, log, log + 1, (log, log + 1, len(cols)))


@pytest.mark.single_conv
@pytest.mark.parametrize("log,ncols", [(log, n) for log in fm.TINY_LOGS for n in fm.tiny_column_counts(log)])
def test_tiny_transforms_over_several_workgroups(big_ctx, oracle, log, ncols):
    """k_fft_tiny packs 256 >> log columns into a workgroup: two and three workgroups, the last one with a partly filled last wave."""
    cols, fams = _labelled_columns(0x6F0000 + log, ncols, 1 << log)
    ptrs, coeffs = _interpolate(big_ctx, oracle, cols, fams, log, (log, ncols))
    _evaluate(big_ctx, oracle, ptrs, coeffs, fams, log, log + 1, (log, log + 1, ncols))


PLAN_CHILD = os.path.join(ROOT, "tests", "fft_plan_child.py")


@pytest.mark.single_conv
def test_library_launches_what_the_plan_model_says():
    """The library's own account of its launches (BFHIP_FFT_PROF_DETAIL=1: the profiler's kernel names carry /b<workgroups>/g<groups>) for
    every transform of MANY_COLUMNS and LARGER_BLOWUPS against tests/fft_plan_model.py. The switch is read once per process, at the first
    transform: a fresh child process runs the transforms (tests/fft_plan_child.py) under a time limit of its own."""
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, PLAN_CHILD], capture_output=True, text=True,
                       env=dict(os.environ, BFHIP_FFT_PROF_DETAIL="1"))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    got = json.loads(r.stdout.strip().splitlines()[-1])
    jobs = [(True, log, log, n) for log, n in fm.MANY_COLUMNS] + [(False, log + 1, log, n) for log, n in fm.MANY_COLUMNS]
    jobs += [(False, log_eval, log, n) for log, log_eval, n in fm.LARGER_BLOWUPS]
    assert len(got) == len(jobs)
    for job, rec in zip(jobs, got):
        assert tuple(rec["job"]) == tuple(int(v) for v in job)
        want = fm.launch_names(job[0], fm.plan(*job))
        assert rec["launches"] == want, "tests/fft_plan_model.py is stale for (inverse, log, src_log, ncols) = %r: the library launched %r, the model says %r" % (job, rec["launches"], want)
