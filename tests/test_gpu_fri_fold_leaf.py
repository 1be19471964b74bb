"""GPU: the FRI commit step that folds a layer inside the leaf launch of its Merkle tree (bfhip_fri_fold_leaf, merkle.hip k_fri_fold_leaf).

Op level: the fused launch against the launches it replaces — bfhip_fold_line, then bfhip_fold_circle_into_line on the result when a circle
evaluation is folded in (the first line layer: bfhip_fold_circle_into_line into a zeroed destination), then bfhip_merkle_commit_layer over
the four folded columns. Folded columns and all leaf hashes must be equal word for word, in the three modes, under every hashing convention,
on uniform columns and on the saturated families of field_inputs.py (the lazily reduced QM31 products are where a rewrite goes wrong).
The entry takes whole layers only: row ranges are not supported, so there is no partial-layer case.

Proof level: a program whose FRI line has layers of 2^19 rows (circle fold alone), 2^18 and 2^17 rows (line fold + the quotient of that
size), all produced by the fused launch; the proof must be the CPU oracle's, byte for byte."""
import functools
import os

import numpy as np
import pytest

import field_inputs as fi
from conftest import P

pytestmark = pytest.mark.gpu

MODES = ("line", "line_circle", "circle")
# 6: less than one workgroup; 8: exactly one; 17: the smallest layer the prover folds this way; 22: 2^14 workgroups, several rows per lane
LOGS = (6, 8, 17, 22)


def _zero_or_max(seed, n):
    """Every cell 0 or P - 1."""
    return np.where(fi.uniform(seed ^ 0x5A7, n) & 1, np.uint32(P - 1), np.uint32(0)).astype(np.uint32)


# (columns, alpha): pseudo-random canonical values, then 0 / P - 1 in every coordinate of source, circle evaluation and alpha, the edge set,
# and the two constants that drive q_const's kept negations to P itself
CASES = {
    "uniform": ("uniform", "uniform"),
    "max": ("max", "max"),
    "zero_or_max": (_zero_or_max, "max"),
    "zero_or_max_alpha": ("max", _zero_or_max),
    "edge": ("edge", "edge"),
    "nc_is_p": ("max", "nc_is_p"),
    "ne_is_p": ("max", "ne_is_p"),
}
BIG_CASES = ("uniform", "max", "zero_or_max", "edge")       # 2^22 rows: bounds the upload time


def _cols(fam, seed, k, n):
    return [fam(seed + 8 * j, n) for j in range(k)] if callable(fam) else fi.columns(fam, seed, k, n)


@functools.lru_cache(maxsize=None)
def _inputs(case, log):
    """(line source, circle evaluation, alpha) of a layer of 2^log rows: both sources have 2^(log + 1) rows."""
    cols_f, alpha_f = CASES[case]
    n = 2 << log
    src, quot = _cols(cols_f, 700 + log, 4, n), _cols(cols_f, 800 + log, 4, n)
    alpha = alpha_f(9, 4) if callable(alpha_f) else fi.const(alpha_f, 9, 4)
    for a in src + quot + [alpha]:
        a.setflags(write=False)
        assert a.dtype == np.uint32 and int(a.max()) < P
    return src, quot, alpha


@pytest.fixture(scope="module", autouse=True)
def _drop_inputs():
    yield
    _inputs.cache_clear()      # the 2^23-row columns of the largest case: 256 MB per family


@pytest.mark.parametrize("log", LOGS)
@pytest.mark.parametrize("mode", MODES)
def test_fused_fold_and_leaves_equal_the_separate_launches(ctx, mode, log):
    n = 1 << log
    for case in (BIG_CASES if log >= 20 else CASES):
        src, quot, alpha = _inputs(case, log)
        ds = [ctx.upload(s) for s in src] if mode != "circle" else None
        dq = [ctx.upload(q) for q in quot] if mode != "line" else None
        zeros = np.zeros(n, dtype=np.uint32)
        want_d = [ctx.upload(zeros) for _ in range(4)]
        got_d = [ctx.upload(np.full(n, 0xDEADBEEF, dtype=np.uint32)) for _ in range(4)]      # nothing of the destination's old contents survives
        want_h, got_h = ctx.malloc(32 * n), ctx.malloc(32 * n)
        try:
            if ds is not None:
                ctx.fold_line(ds, want_d, log + 1, alpha)
            if dq is not None:
                ctx.fold_circle_into_line(want_d, dq, log + 1, alpha)
            ctx.merkle_commit_layer(log, 0, want_d, want_h)
            ctx.fri_fold_leaf(ds, dq, got_d, log, alpha, got_h)
            want = np.stack([ctx.download(p, n) for p in want_d])
            got = np.stack([ctx.download(p, n) for p in got_d])
            wh, gh = ctx.download(want_h, 8 * n), ctx.download(got_h, 8 * n)
        finally:
            for p in (ds or []) + (dq or []) + want_d + got_d + [want_h, got_h]:
                ctx.free(p)
        assert int(want.max()) < P
        bad = np.nonzero(got != want)
        assert bad[0].size == 0, (mode, case, log, "folded columns: first differing (coordinate, row)", int(bad[0][0]), int(bad[1][0]))
        bad = np.nonzero(gh != wh)[0]
        assert bad.size == 0, (mode, case, log, "leaf hashes: first differing row", int(bad[0]) // 8)
        assert gh.any()


def test_entry_rejects_what_it_cannot_do(ctx, pkg):
    d = [ctx.malloc(4 << 6) for _ in range(4)]
    h = ctx.malloc(32 << 6)
    try:
        with pytest.raises(pkg.BfhipError, match="neither a line source nor a circle evaluation"):
            ctx.fri_fold_leaf(None, None, d, 6, [1, 0, 0, 0], h)
        with pytest.raises(pkg.BfhipError, match="twiddle tree"):
            ctx.fri_fold_leaf(d, None, d, ctx.max_log_domain - 1, [1, 0, 0, 0], h)      # a line source of 2^max_log_domain rows
        with pytest.raises(pkg.BfhipError, match="twiddle tree"):
            ctx.fri_fold_leaf(None, d, d, 1, [1, 0, 0, 0], h)
    finally:
        for p in d + [h]:
            ctx.free(p)


def _prog(name):
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "programs", name)).read()


# 29 x 29 passes of "move one unit two cells to the right": 5222 VM steps over three live memory cells
NESTED_LOOPS = "+" * 29 + "[>" + "+" * 29 + "[>+<-]<-]"


def test_proof_with_fused_fri_layers_matches_the_oracle(ctx, pkg, oracle):
    """NESTED_LOOPS at LOG_MAX_ROWS 18: the FRI line starts at 2^19 rows (circle fold alone) and its layers of 2^19, 2^18 and 2^17 rows are
    fused launches; everything below keeps its own kernels. A column of 2^s cells has a quotient of 2^(s + 2) cells that folds into the line
    layer of 2^(s + 1) rows: the 2^18-row layer takes the quotient of the 2^17-cell components. No component has 2^16 cells, but the
    2^17-row layer is still a line fold PLUS a circle fold: the preprocessed trace holds an IsFirst column of every size from 2^4 to
    2^LOG_MAX_ROWS cells, so every line layer of a proof has a quotient of its size folded in. A layer without one cannot occur in a proof
    (the plain line fold is covered at op level above); what can be asserted here is the component sizes and that the fused path ran."""
    tr = pkg.Trace(ctx, NESTED_LOOPS)
    try:
        assert tr.log_sizes == [18, 17, 11, 17, 14, 9, 4, 14, 14, 4, 15, 14, 4]
        sizes = set(tr.log_sizes)
        assert max(sizes) == 18 and 17 in sizes and 16 not in sizes
        got, _ = tr.prove(18)
    finally:
        tr.close()
    assert ctx.last_proof_flags()["fri_fold_leaf"]
    want, _, _ = oracle.prove(NESTED_LOOPS, b"", log_max_rows=18)
    assert got == want
    assert pkg.verify_brainfuck(got, 18) == (True, "")


@pytest.mark.single_conv
def test_small_proofs_keep_the_separate_launches(ctx, pkg):
    """hello1 at LOG_MAX_ROWS 15: the first line layer has 2^16 rows — below the threshold, nothing is fused and the flag says so."""
    pkg.prove_brainfuck(_prog("hello1.bf"), b"", ctx=ctx, log_max_rows=15)
    assert not ctx.last_proof_flags()["fri_fold_leaf"]
