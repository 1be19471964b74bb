"""GPU: the commit path of a commitment-scheme session (bfhip_pcs_commit, csrc/pcs.hip) ABOVE LDE level 18, column by column against the CPU
oracle. bfhip_pcs_tree_columns hands back the coefficients and the LDE of every committed column, so the path is checked without proving
anything: mixed-size batches in one fft_plan (small groups riding in the tile launch), both commit forms, many columns per workgroup in the
largest size class, and the Merkle plan over many columns per level. One session per entry of fft_plan_model.SESSIONS: log_blowup_factor 1, 2
and 4 with top LDE level 20, 21 and 22, and log_blowup_factor 1 at top level 22 — the one whose traces (2^21 rows) run k_fft_stridedK.

Per column: coefficients == oracle.interpolate(input) (form 0) or the input itself (form 1); LDE == oracle.evaluate(coefficients, log, log + b).
Per tree: the root == the root of the oracle's Merkle commitment over the oracle's LDE columns, and is what the channel was given.
Integers and bytes only. tests/test_fft_plan_model_cpu.py holds the trees to what this text says of them.

Oracle time per session on a 16-core host: see the printed line of each case (pytest -s)."""
import ctypes
import random
import time

import numpy as np
import pytest

import fft_plan_model as fm
import pcs_generic_cases as gc
from conftest import P

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

MAX_LOG_DOMAIN = 22
FORMS = (0, 1)          # tree 0 commits evaluations, tree 1 coefficients


def session_trees(name):
    """[tree] = [(log, family, seed)] in caller order: the largest size class of fft_plan_model.SESSIONS (one column of all P - 1, one edge
    column), and in shuffled order between them one tiny column (2^4 or 2^5), one single-pass column (2^6 .. 2^11), two sizes of
    2^12 .. 2^19 below the largest, one of the sizes twice, one zero and one constant column."""
    b, top, nbig = fm.SESSIONS[name]
    big = top - b
    small = ([(5, "uniform"), (9, "uniform"), (13, "uniform"), (16, "edge"), (13, "max"), (9, "zero"), (16, "const")],
             [(4, "const"), (11, "uniform"), (12, "uniform"), (17, "uniform"), (12, "edge"), (17, "zero"), (7, "max")])
    trees = []
    for t in range(2):
        cols = [(big, "uniform")] * nbig + small[t]
        cols[1], cols[nbig - 1] = (big, "max"), (big, "edge")
        rng = random.Random(1000 * top + 10 * b + t)
        rng.shuffle(cols)
        trees.append([(log, fam, 0x9C0000 + (top << 12) + (t << 8) + k + ((k + 1) << 32)) for k, (log, fam) in enumerate(cols)])
    return trees


@pytest.fixture(scope="module")
def lctx(pkg):
    c = pkg.Context(0, max_log_domain=MAX_LOG_DOMAIN)
    yield c
    c.close()


def _same(got, want, what, tree, k, col):
    if not np.array_equal(got, want):
        i = int(np.nonzero(got != want)[0][0])
        raise AssertionError("%s of tree %d column %d (2^%d, %s): first difference at index %d: %d against %d" % (what, tree, k, col[0], col[1], i, got[i], want[i]))


def _oracle_root(oracle, lde, logs):
    ptrs = (ctypes.c_void_p * len(lde))(*[c.ctypes.data for c in lde])
    root = (ctypes.c_ubyte * 32)()
    assert oracle.L.orc_merkle_commit(ptrs, (ctypes.c_uint32 * len(logs))(*logs), ctypes.c_size_t(len(logs)), root, None) == 0
    return bytes(root)


def _run_session(pkg, ctx, oracle, name, conv):
    b = fm.SESSIONS[name][0]
    trees = session_trees(name)
    ctx.set_conventions(*conv)
    ctx.set_pcs_config(pkg.PcsConfig(pow_bits=4, log_blowup_factor=b, n_queries=6))
    oracle.set_conventions(*conv)
    ch, ch_ref = pkg.Channel(conv), pkg.Channel(conv)
    dev, t_oracle = [], 0.0
    try:
        ctx.profile_enable(1)
        ctx.profile_reset()
        with pkg.PcsSession(ctx) as s:
            for t, tree in enumerate(trees):
                logs = [c[0] for c in tree]
                cols = [gc.column(*c) for c in tree]
                ptrs = [ctx.upload(c) for c in cols]
                dev += ptrs
                root = s.commit(ch, ptrs, logs, form=FORMS[t])
                co, ev = s.tree_columns(t)
                assert len(co) == len(ev) == len(tree)
                lde = [None] * len(tree)
                for log in sorted(set(logs)):          # the oracle per size class, the columns in caller order
                    idx = [k for k, l in enumerate(logs) if l == log]
                    inp = np.stack([cols[k] for k in idx])
                    t0 = time.perf_counter()
                    coeffs = oracle.interpolate(inp, log) if FORMS[t] == 0 else inp
                    ext = oracle.evaluate(coeffs, log, log + b)
                    t_oracle += time.perf_counter() - t0
                    for j, k in enumerate(idx):
                        _same(ctx.download(co[k], 1 << log), coeffs[j], "coefficients", t, k, tree[k])
                        _same(ctx.download(ev[k], 1 << (log + b)), ext[j], "LDE", t, k, tree[k])
                        if tree[k][1] in ("max", "const") and FORMS[t] == 0:      # closed form: a constant column is its value everywhere
                            assert (ext[j] == cols[k][0]).all()
                        lde[k] = ext[j]
                t0 = time.perf_counter()
                want_root = _oracle_root(oracle, lde, [l + b for l in logs])
                t_oracle += time.perf_counter() - t0
                assert root == want_root, "tree %d: root %s against the oracle's %s" % (t, root.hex(), want_root.hex())
                ch_ref.mix_root(want_root)
                assert ch.state() == ch_ref.state(), "tree %d: the channel was not given the root" % t
        ctx.sync()
        rep = ctx.profile_report()
    finally:
        ctx.profile_enable(0)
        ctx.sync()
        for p in dev:
            ctx.free(p)
        ctx.set_conventions(*gc.STWO)
        ctx.set_pcs_config(None)
        oracle.set_conventions(0, 0, 0, 0)
        ch.close()
        ch_ref.close()
    print("%-9s %s oracle %.2f s" % (name, conv, t_oracle))
    # the launches the session is there for
    want = fm.session_kernels(b, [[c[0] for c in tree] for tree in trees], FORMS)
    calls = {k: v["calls"] for k, v in rep.items() if k.startswith("k_fft")}
    for kernel in sorted(want):
        assert calls.get(kernel, 0) > 0, (name, kernel, calls)
    assert set(calls) == want, (name, calls)


@pytest.mark.parametrize("name", list(fm.SESSIONS))
def test_committed_columns_and_roots_are_the_oracles(pkg, lctx, _oracle, name):
    _run_session(pkg, lctx, _oracle, name, gc.STWO)


def test_committed_columns_and_roots_under_rfc7693_nodes(pkg, lctx, _oracle):
    """The log_blowup_factor 1 session once more under the RFC 7693 node hash, on the context and on the oracle."""
    _run_session(pkg, lctx, _oracle, "b1", gc.RFC7693)


assert P == (1 << 31) - 1
