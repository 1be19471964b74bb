"""GPU: the commitment-scheme session (bfhip_pcs_*, csrc/pcs.hip) — stwo's CommitmentSchemeProver over arbitrary columns on the fused
launches of a Brainfuck proof. Everything is compared as integers and bytes:
 1. the four trees of a Brainfuck proof, captured as plain coefficient columns (bfhip_test_capture_polys, test-hooks build) and pushed
    through a session by a Python replay of the protocol (tests/pcs_replay.py), give the proof's own "proof" member byte for byte;
 2. committing evaluations (form 0) and coefficients (form 1) of the same polynomials gives the same root;
 3. columns without any Brainfuck structure: roots against a chain of single operations (the only check of roots against them), sampled values
    against bfhip_eval_at_point, the proof against the generic verifier, which rejects a flipped queried or sampled value. The bytes of
    such proofs — quotients, FRI layers, nonce, queried values, decommitments — are held to the CPU oracle's generic prover in
    tests/test_gpu_pcs_generic_oracle.py, over the matrix of tests/pcs_generic_cases.py (LDE levels 5 to 20, up to 302 columns, 64 points);
 4. a tree whose largest column makes line layers from 2^17 down: k_fri_fold_leaf, k_fri_layer and k_fri_tail in one commit phase;
 5. what is refused, and that a destroyed session leaves the context as it was."""
import ctypes
import json

import numpy as np
import pytest

import field_inputs as fi
import pcs_replay
from conftest import P

pytestmark = pytest.mark.gpu

CODE, INP, LMR = "+++>,<[>+.<-]", b"\x01", 17      # of tests/test_gpu_pcs_config.py
STWO, RFC7693, POSEIDON = (0, 0, 0, 0), (1, 0, 0, 0), (0, 0, 0, 1)
MAX_LOG_DOMAIN = 20                                 # log_max_rows 17 at log_blowup_factor 2: 17 + 2 + 1


@pytest.fixture(scope="module")
def _hctx(hooks_pkg):
    c = hooks_pkg.Context(0, max_log_domain=MAX_LOG_DOMAIN)
    yield c
    c.close()


@pytest.fixture
def hctx(_hctx):
    yield _hctx
    _hctx.set_conventions(*STWO)
    _hctx.set_pcs_config(None)


class Dev:
    """Device buffers of one test, freed together."""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint32)
        assert int(arr.max(initial=0)) < P
        self.ptrs.append(self.ctx.upload(arr))
        return self.ptrs[-1]

    def empty(self, n_words):
        self.ptrs.append(self.ctx.malloc(4 * n_words))
        return self.ptrs[-1]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.sync()
        for p in self.ptrs:
            self.ctx.free(p)


def _capture(hp, ctx, conv, cfg):
    """(the proof bfhip_prove_brainfuck returned, its parsed form, [tree][column] = coefficient column) — one proof with the capture on."""
    L = hp.lib()
    ctx.set_conventions(*conv)
    ctx.set_pcs_config(cfg)
    hp._check(L.bfhip_test_capture_polys(ctx._h, 1))
    try:
        raw = hp.prove_brainfuck(CODE, INP, ctx=ctx, log_max_rows=LMR)
        full = json.loads(raw)
        logs = pcs_replay.tree_log_sizes(hp, [full["claim"][n]["log_size"] for n in pcs_replay.NAMES], LMR)
        trees = []
        for t in range(4):
            cols = []
            for c, log in enumerate(logs[t]):
                got = ctypes.c_uint32()
                out = np.empty(1 << log, dtype=np.uint32)
                hp._check(L.bfhip_test_captured_poly(ctx._h, t, c, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.size), ctypes.byref(got)))
                assert got.value == log, (t, c)
                cols.append(out)
            # no column beyond the ones the claim describes
            assert L.bfhip_test_captured_poly(ctx._h, t, len(logs[t]), None, ctypes.c_size_t(0), ctypes.byref(ctypes.c_uint32())) == -1
            trees.append(cols)
    finally:
        hp._check(L.bfhip_test_capture_polys(ctx._h, 0))
    return raw, full, logs, trees


def _prove_replay(hp, ctx, dev, full, logs, trees, conv):
    """prove_brainfuck's commitment-scheme half through a session: the claim and the claimed sums are the sweep's results (taken from
    the proof, whose sweep is not what is under test); every root, challenge and opening is the session's."""
    log_sizes = [full["claim"][n]["log_size"] for n in pcs_replay.NAMES]
    claimed = [pcs_replay.flat_q(full["interaction_claim"][n]["claimed_sum"]) for n in pcs_replay.NAMES]
    ch = hp.Channel(conv)
    with hp.PcsSession(ctx) as s:
        ptrs = [[dev.up(col) for col in tree] for tree in trees]
        roots = [s.commit(ch, ptrs[0], logs[0], form=1)]
        for l in log_sizes:
            ch.mix_u64(l)
        roots.append(s.commit(ch, ptrs[1], logs[1], form=1))
        for _ in range(3):
            ch.draw_felts(2)
        for c in claimed:
            ch.mix_felts([c])
        roots.append(s.commit(ch, ptrs[2], logs[2], form=1))
        ch.draw_felts(1)
        roots.append(s.commit(ch, ptrs[3], logs[3], form=1))
        oods = ch.draw_point()
        points, samples = pcs_replay.mask_of(hp, log_sizes, LMR, oods, conv[2])
        proof = s.prove_values(ch, points, samples)
    assert roots == [pcs_replay.root_bytes(h) for h in full["proof"]["commitments"]]
    return proof


@pytest.mark.parametrize("name,cv,cfg", [("default", STWO, None), ("b2_q10_pow16", STWO, dict(pow_bits=16, log_blowup_factor=2, n_queries=10)),
                                           ("rfc7693", RFC7693, None), ("poseidon252", POSEIDON, None)])
def test_session_reproduces_the_brainfuck_proof_byte_for_byte(hooks_pkg, hctx, name, cv, cfg):
    hp, conv = hooks_pkg, cv
    cfg = None if cfg is None else hp.PcsConfig(**cfg)
    raw, full, logs, trees = _capture(hp, hctx, conv, cfg)
    assert hp.verify_brainfuck(raw, LMR, conv, cfg) == (True, "")
    # the capture expands row-granular polynomials: every main-trace coefficient sits at an index that is 0 mod 16
    assert all(not col.reshape(-1, 16)[:, 1:].any() for col in trees[1]) and any(col.any() for col in trees[1])
    with Dev(hctx) as dev:
        proof = _prove_replay(hp, hctx, dev, full, logs, trees, conv)
    want = pcs_replay.proof_member(raw)
    assert len(proof) == len(want) and proof == want, name
    assert hp.prove_brainfuck(CODE, INP, ctx=hctx, log_max_rows=LMR) == raw      # and the context proves as before


def test_evaluations_and_coefficients_commit_to_the_same_root(hooks_pkg, hctx):
    hp = hooks_pkg
    _, full, logs, trees = _capture(hp, hctx, STWO, None)
    with Dev(hctx) as dev:
        coeffs = [dev.up(col) for col in trees[1]]
        evals = [dev.empty(1 << log) for log in logs[1]]
        for log in sorted(set(logs[1])):
            idx = [k for k, l in enumerate(logs[1]) if l == log]
            hctx.evaluate([coeffs[k] for k in idx], [evals[k] for k in idx], log, log)
        before = [hctx.download(p, 1 << log) for p, log in zip(evals, logs[1])]
        with hp.PcsSession(hctx) as s:
            root1 = s.commit(hp.Channel(STWO), coeffs, logs[1], form=1)
        with hp.PcsSession(hctx) as s:
            root0 = s.commit(hp.Channel(STWO), evals, logs[1], form=0)
            co, _ = s.tree_columns(0)
            assert all(np.array_equal(hctx.download(p, 1 << log), want) for p, log, want in zip(co, logs[1], trees[1]))
        assert root0 == root1 == bytes(full["proof"]["commitments"][1])
        # the caller's columns are borrowed, not modified
        assert all(np.array_equal(hctx.download(p, 1 << log), b) for p, log, b in zip(evals, logs[1], before))


ARBITRARY = ([6, 4, 4], [10, 10, 7, 5], [11])


def _arbitrary_columns():
    """Random canonical columns, one all p - 1, one all zero, one of edge values."""
    cols, seed = [], 7001
    for t, logs in enumerate(ARBITRARY):
        tree = []
        for c, log in enumerate(logs):
            seed += 1
            family = {(0, 1): "max", (1, 2): "zero", (1, 3): "edge"}.get((t, c), "uniform")
            tree.append(np.zeros(1 << log, dtype=np.uint32) if family == "zero" else fi.column(family, seed, 1 << log))
        cols.append(tree)
    return cols


def _chain_root(ctx, dev, eval_ptrs, logs, blowup):
    """The root of one tree by single operations: bfhip_interpolate + bfhip_evaluate per size, then bfhip_merkle_commit_layer per level."""
    lde = {}
    for log in set(logs):
        idx = [k for k, l in enumerate(logs) if l == log]
        co = [dev.empty(1 << log) for _ in idx]
        ev = [dev.empty(1 << (log + blowup)) for _ in idx]
        ctx.interpolate([eval_ptrs[k] for k in idx], co, log)
        ctx.evaluate(co, ev, log, log + blowup)
        for k, p in zip(idx, ev):
            lde[k] = p
    top = max(logs) + blowup
    prev = None
    for level in range(top, -1, -1):
        here = [lde[k] for k, l in enumerate(logs) if l + blowup == level]
        out = dev.empty(8 << level)
        ctx.merkle_commit_layer(level, prev, here, out)
        prev = out
    return ctx.download(prev, 8).tobytes()


@pytest.mark.parametrize("blowup", [1, 2])
def test_arbitrary_columns_commit_open_and_verify(hooks_pkg, hctx, blowup):
    hp = hooks_pkg
    cfg = hp.PcsConfig(pow_bits=6, log_blowup_factor=blowup, n_queries=5)
    hctx.set_pcs_config(cfg)
    data = _arbitrary_columns()
    with Dev(hctx) as dev:
        ptrs = [[dev.up(col) for col in tree] for tree in data]
        ch = hp.Channel(STWO)
        with hp.PcsSession(hctx) as s:
            roots = [s.commit(ch, ptrs[t], ARBITRARY[t], form=0) for t in range(3)]
            oods = ch.draw_point()
            points = [oods, hp.circle_point_offset(oods, 10, -1)]
            # the two 2^10 columns are opened at both points, in either order; one column has no sample at all
            samples = [[[0], [0], []], [[0, 1], [1, 0], [0], [0]], [[0]]]
            proof, sampled = s.prove_values(ch, points, samples, with_sampled=True)
            # sampled values = bfhip_eval_at_point of the session's own coefficients, in the order of the description
            want, k = [], 0
            for t in range(3):
                co, ev = s.tree_columns(t)
                assert len(co) == len(ev) == len(ARBITRARY[t])
                for c, log in enumerate(ARBITRARY[t]):
                    for i in samples[t][c]:
                        want.append(hctx.eval_at_point(co[c], log, points[i]))
            assert sampled == want and len(sampled) == 9
        # the roots by single operations
        for t in range(3):
            assert roots[t] == _chain_root(hctx, dev, ptrs[t], ARBITRARY[t], blowup), t
    pf = json.loads(proof)
    assert [bytes(h) for h in pf["commitments"]] == roots
    assert [[pcs_replay.flat_q(q) for col in tree for q in col] for tree in pf["sampled_values"]] == [sampled[:2], sampled[2:8], sampled[8:]]
    assert pf["sampled_values"][0][2] == [] and len(pf["fri_proof"]["inner_layers"]) == 10      # line layers 2^(10 + b) .. 2^(1 + b)

    def verify(js):
        vch, v = hp.Channel(STWO), hp.PcsVerifier(STWO, cfg)
        for t in range(3):
            v.commit(vch, roots[t], ARBITRARY[t])
        assert vch.draw_point() == oods
        return v.verify_values(vch, points, samples, js)

    assert verify(proof) == (True, "")
    bad = json.loads(proof)
    bad["queried_values"][1][0] ^= 1
    assert verify(pcs_replay.compact(bad))[1].startswith("MerkleVerification tree 1")
    bad = json.loads(proof)
    bad["sampled_values"][1][1][1][0][0] ^= 1
    ok, why = verify(pcs_replay.compact(bad))
    assert not ok and why
    # another description of the same openings (the second point dropped from one column) does not verify either
    vch, v = hp.Channel(STWO), hp.PcsVerifier(STWO, cfg)
    for t in range(3):
        v.commit(vch, roots[t], ARBITRARY[t])
    vch.draw_point()
    assert v.verify_values(vch, points, [[[0], [0], []], [[0], [1, 0], [0], [0]], [[0]]], proof) == (False, "InvalidStructure: sampled_values")


def test_line_layers_from_2_to_the_17_take_every_fri_launch_path(hooks_pkg, hctx):
    """One tree whose largest column has 2^17 rows at log_blowup_factor 1: the first line layer has 2^17 rows (k_fri_fold_leaf), the layers
    2^16 .. 2^11 are k_fri_layer's, the rest k_fri_tail's; the smaller columns' quotients fold in on the way down."""
    hp = hooks_pkg
    logs = [17, 12, 9, 5]
    cfg = hp.PcsConfig(pow_bits=5, log_blowup_factor=1, n_queries=4)
    hctx.set_pcs_config(cfg)
    with Dev(hctx) as dev:
        ptrs = [dev.up(fi.column("uniform", 8100 + k, 1 << log)) for k, log in enumerate(logs)]
        ch = hp.Channel(STWO)
        with hp.PcsSession(hctx) as s:
            root = s.commit(ch, ptrs, logs, form=0)
            oods = ch.draw_point()
            samples = [[[0], [0], [0], [0]]]
            proof = s.prove_values(ch, [oods], samples)
            assert hctx.last_proof_flags()["fri_fold_leaf"]
    pf = json.loads(proof)
    assert len(pf["fri_proof"]["inner_layers"]) == 16 and len(pf["fri_proof"]["last_layer_poly"]["coeffs"]) == 1
    vch, v = hp.Channel(STWO), hp.PcsVerifier(STWO, cfg)
    v.commit(vch, root, logs)
    assert vch.draw_point() == oods
    assert v.verify_values(vch, [oods], samples, proof) == (True, "")
    assert vch.state() == ch.state()                      # prover and verifier leave the channel in the same state


def test_refusals_and_nothing_left_behind(hooks_pkg, hctx, _oracle):
    hp = hooks_pkg
    _oracle.set_conventions(*STWO)
    want = _oracle.prove(CODE, INP, log_max_rows=LMR)[0]
    assert hp.prove_brainfuck(CODE, INP, ctx=hctx, log_max_rows=LMR) == want
    in_use = hctx.memory()["arena_in_use"]
    assert in_use > 0
    with Dev(hctx) as dev:
        col = dev.up(fi.column("uniform", 9001, 1 << 6))
        ch = hp.Channel(STWO)
        s = hp.PcsSession(hctx)
        try:
            with pytest.raises(hp.BfhipError, match="a commitment-scheme session is open"):
                hp.PcsSession(hctx)
            with pytest.raises(hp.BfhipError, match="a commitment-scheme session is open"):
                hp.prove_brainfuck(CODE, INP, ctx=hctx, log_max_rows=LMR)
            with pytest.raises(hp.BfhipError, match="a commitment-scheme session is open"):
                hp.Trace(hctx, CODE, INP)
            with pytest.raises(hp.BfhipError, match="a commitment-scheme session is open"):
                hctx.set_pcs_config(hp.PcsConfig(n_queries=4))
            g = hp.LocalGroup(2)
            with pytest.raises(hp.BfhipError, match="a commitment-scheme session is open"):
                hctx.join_local_group(g, 0)
            g.close()
            for bad in (3, MAX_LOG_DOMAIN):               # [4, max_log_domain - log_blowup_factor] = [4, 19]
                with pytest.raises(hp.BfhipError, match=r"outside \[4, max_log_domain - log_blowup_factor\] = \[4, 19\]"):
                    s.commit(ch, [col], [bad], form=0)
            with pytest.raises(hp.BfhipError, match="form must be"):
                s.commit(ch, [col], [6], form=2)
            with pytest.raises(hp.BfhipError, match="at least one column"):
                s.commit(ch, [], [], form=0)
            with pytest.raises(hp.BfhipError, match="nothing was committed"):
                s.prove_values(ch, [], [])
            with pytest.raises(hp.BfhipError, match="other conventions"):
                s.commit(hp.Channel(POSEIDON), [col], [6], form=0)
            state = ch.state()
            s.commit(ch, [col, col], [6, 6], form=0)        # repeats are allowed
            assert ch.state() != state
            p = ch.draw_point()
            with pytest.raises(hp.BfhipError, match="point index 1 out of range"):
                s.prove_values(ch, [p], [[[0], [1]]])
            with pytest.raises(hp.BfhipError, match="at most 2 per column"):        # a cap of the quotient tables
                s.prove_values(ch, [p], [[[0, 0, 0], [0]]])
            with pytest.raises(hp.BfhipError, match=r"more than BFHIP_PCS_MAX_POINTS \(64\)"):
                s.prove_values(ch, [p] * 65, [[[0], [0]]])
            with pytest.raises(hp.BfhipError, match="canonical"):
                s.prove_values(ch, [[P] + p[1:]], [[[0], [0]]])
            # a refused description leaves the session usable; the single operations a sweep needs keep working meanwhile
            co, ev = s.tree_columns(0)
            assert hctx.eval_at_point(co[0], 6, p) == hctx.eval_at_point(co[1], 6, p)
            proof = s.prove_values(ch, [p], [[[0], [0]]])
            assert json.loads(proof)["sampled_values"][0][0] == json.loads(proof)["sampled_values"][0][1]
            with pytest.raises(hp.BfhipError, match="already called"):
                s.prove_values(ch, [p], [[[0], [0]]])
            with pytest.raises(hp.BfhipError, match="ended this session"):
                s.commit(ch, [col], [6], form=0)
            assert len(s.tree_columns(0)[0]) == 2
            assert hctx.memory()["arena_in_use"] != in_use
        finally:
            s.close()
    assert hctx.memory()["arena_in_use"] == in_use
    assert hp.prove_brainfuck(CODE, INP, ctx=hctx, log_max_rows=LMR) == want
    # a member of a shard group
    g = hp.LocalGroup(2)
    c = hp.Context(0, max_log_domain=16)
    try:
        c.join_local_group(g, 0)
        with pytest.raises(hp.BfhipError, match="shard group"):
            hp.PcsSession(c)
        c.leave_group()
        hp.PcsSession(c).close()
    finally:
        c.close()
        g.close()
    # a pool's sub-context: idle is fine, refused while a job is outstanding
    pool = hp.Pool(0, n_in_flight=1, max_log_domain=MAX_LOG_DOMAIN)
    try:
        hp.PcsSession(pool.ctx(0)).close()
        ticket = pool.submit_program(CODE, INP, log_max_rows=LMR)
        with pytest.raises(hp.BfhipError, match="jobs are outstanding"):      # queued, running or finished and not yet taken
            hp.PcsSession(pool.ctx(0))
        r = pool.wait()
        assert r.ticket == ticket and r.ok and r.proof == want
        hp.PcsSession(pool.ctx(0)).close()
    finally:
        pool.close()
