"""GPU: the commitment-scheme session (bfhip_pcs_*, csrc/pcs.hip) over ARBITRARY columns against the CPU oracle, byte for byte. For every case
of tests/pcs_generic_cases.py the session's proof is the proof orc::Prover::prove_values gives for the same columns, config, conventions,
points and sample lists (tests/native/oracle_pcs_generic.cpp): same length, same bytes — roots, sampled values, quotients (through the
first FRI layer's root), every FRI layer, the last layer, the nonce, queried values, decommitments and witnesses. On a mismatch the test
names the first member, in the order the prover produces them, that differs. The sampled values the session returns and the state it leaves
the channel in are the oracle's too. Integers and bytes only; there is no tolerance anywhere.
The shim itself is anchored to bytes the oracle's full prover is known to produce: the four trees of a Brainfuck proof, captured as
coefficient columns (bfhip_test_capture_polys, test-hooks build), go through the shim under the replay of tests/pcs_replay.py and give the
proof's own "proof" member.
Measured on an MI355X host with 16 cores, oracle / session per case: 1 to 10 ms / 1 to 9 ms for every case but sub17, ladder, deep_b1 and
deep_b2 (39 to 50 ms / 2 ms), wide20 (0.29 s / 42 ms) and conv_poseidon252 (0.49 s / 25 ms); the module takes 5 s, 3.6 s of which build the shim."""
import ctypes
import json
import time

import numpy as np
import pytest

import oracle_pcs_generic
import pcs_generic_cases as gc
import pcs_replay
from conftest import P

pytestmark = pytest.mark.gpu

CODE, INP = "+++>,<[>+.<-]", b"\x01"
ANCHOR_LMR = 15      # log_max_rows 15 at log_blowup_factor 2 needs max_log_domain 15 + 2 + 1 = 18: within the context of the matrix (20)


@pytest.fixture(scope="module")
def gshim(tmp_path_factory):
    return oracle_pcs_generic.build(tmp_path_factory.mktemp("oracle_pcs_generic"))


@pytest.fixture(scope="module")
def oracle_proofs(gshim, pkg):
    """The oracle's proof of a case, computed once."""
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = oracle_pcs_generic.prove_case(gshim, pkg, case)
        return cache[case.name]
    return get


def _context(pk):
    return pk.Context(0, max_log_domain=gc.MAX_LOG_DOMAIN)


@pytest.fixture(scope="module")
def _gctx(pkg):
    c = _context(pkg)
    yield c
    c.close()


@pytest.fixture
def gctx(_gctx):
    yield _gctx
    _gctx.set_conventions(*gc.STWO)
    _gctx.set_pcs_config(None)


@pytest.fixture(scope="module")
def _hctx(hooks_pkg):
    c = _context(hooks_pkg)
    yield c
    c.close()


@pytest.fixture
def hctx(_hctx):
    yield _hctx
    _hctx.set_conventions(*gc.STWO)
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

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.sync()
        for p in self.ptrs:
            self.ctx.free(p)


def session_prove(pk, ctx, case, columns=None, form=None, inside=None):
    """The case through a PcsSession of `ctx`: (roots, drawn point, points, proof, sampled values, channel state, device pointers).
    One array object is uploaded once: a column the case holds twice is one device column passed twice. inside(session): called before
    the session is closed; its result is appended."""
    ctx.set_conventions(*case.conv)
    ctx.set_pcs_config(pk.PcsConfig(**case.cfg))
    columns = case.columns() if columns is None else columns
    ch = pk.Channel(case.conv)
    with Dev(ctx) as dev:
        up = {}
        for tree in columns:
            for col in tree:
                if id(col) not in up:
                    up[id(col)] = dev.up(col)
        ptrs = [[up[id(col)] for col in tree] for tree in columns]
        with pk.PcsSession(ctx) as s:
            out = gc.prove(case, pk, s, ch, ptrs, form=form)
            extra = () if inside is None else (inside(s),)
    return out + (ch.state(), ptrs) + extra


def assert_same_proof(case, got, want):
    roots, oods, points, proof, sampled = got[:5]
    w_roots, w_oods, w_points, w_proof, w_sampled = want[:5]
    for t, (a, b) in enumerate(zip(roots, w_roots)):
        assert a == b, "%s: commitments[%d]: %s against %s" % (case.name, t, a.hex(), b.hex())
    assert oods == w_oods and points == w_points, case.name
    diff = gc.first_difference(proof, w_proof)
    assert diff is None, "%s: first difference at %s" % (case.name, diff)
    assert len(proof) == len(w_proof) and proof == w_proof, case.name
    assert sampled == w_sampled, case.name
    assert got[5] == want[5], case.name                  # the channel after prove_values


@pytest.mark.parametrize("case", gc.CASES, ids=repr)
def test_session_proof_is_the_oracles_byte_for_byte(pkg, gctx, oracle_proofs, case):
    want = oracle_proofs(case)
    deep = case.name.startswith("deep")
    if deep:
        # the path flags are those of the last proof; a session only adds to them. A small Brainfuck proof clears them first.
        gctx.set_conventions(*gc.STWO)
        gctx.set_pcs_config(None)
        pkg.prove_brainfuck(CODE, INP, ctx=gctx, log_max_rows=10)
        assert not gctx.last_proof_flags()["fri_fold_leaf"]
    t0 = time.perf_counter()
    got = session_prove(pkg, gctx, case)
    print("%-18s oracle %.3f s, session %.3f s, proof %d bytes" % (case.name, want[6], time.perf_counter() - t0, len(got[3])))
    assert_same_proof(case, got, want)
    if deep:
        assert gctx.last_proof_flags()["fri_fold_leaf"], case.name      # the first line layer has 2^17 rows: folded inside its leaf launch


BY_LAUNCHES, BY_FOLD_LEAF, BY_LAYER_KERNEL, BY_TAIL, QUOTIENT, NO_TREE = 0, 1, 2, 3, 4, 15      # HipProver::FriCommitted::path (csrc/prover.h)


@pytest.mark.parametrize("name", ["tiny", "ladder", "deep_b1", "deep_b2"])
def test_session_reaches_the_fri_launch_paths_its_case_is_there_for(hooks_pkg, hctx, oracle_proofs, name):
    """Which launch folded and which hashed each line layer of the session's FRI commit phase (bfhip_test_pcs_fri_path, test-hooks build):
    word k = who folded layer k | QUOTIENT when a circle evaluation was folded in | who hashed its tree << 4."""
    hp, case = hooks_pkg, gc.BY_NAME[name]

    def fri_path(s):
        n = ctypes.c_uint32()
        hp._check(hp.lib().bfhip_test_pcs_fri_path(s._h, None, 0, ctypes.byref(n)))
        out = (ctypes.c_uint32 * n.value)()
        hp._check(hp.lib().bfhip_test_pcs_fri_path(s._h, out, n.value, ctypes.byref(n)))
        return list(out)

    got = session_prove(hp, hctx, case, inside=fri_path)
    assert_same_proof(case, got, oracle_proofs(case))
    path, b = got[7], case.cfg["log_blowup_factor"]
    print(name, [hex(w) for w in path])
    top = case.max_log + b - 1                                  # layer k has 2^(top - k) rows; the last one (2^b rows) has no tree
    assert len(path) == top - b + 1
    folded, hashed = [w & 3 for w in path], [w >> 4 for w in path]
    # the circle evaluation of 2^(L + 1) rows folds into the line layer of 2^L rows: a quotient where, and only where, the case has the size
    sizes = {l + b for t in case.logs for l in t}
    assert [bool(w & QUOTIENT) for w in path] == [top - k + 1 in sizes for k in range(len(path))]
    assert hashed[-1] == NO_TREE and NO_TREE not in hashed[:-1]
    for k in range(len(path)):
        log = top - k
        want_hash = NO_TREE if k == len(path) - 1 else BY_FOLD_LEAF if log >= 17 else BY_LAYER_KERNEL if 11 <= log <= 16 and k >= 1 else BY_TAIL if log <= 10 else BY_LAUNCHES
        assert hashed[k] == want_hash, (k, log, hex(path[k]))
        # layer 0 is folded from the largest quotient alone, a layer of 2^10 rows from one of 2^11 by a launch of its own (the tail starts
        # with its tree), everything below by the tail
        want_fold = BY_FOLD_LEAF if log >= 17 else BY_LAUNCHES if k == 0 or log == 10 else BY_LAYER_KERNEL if log >= 11 else BY_TAIL
        assert folded[k] == want_fold, (k, log, hex(path[k]))
    if name == "ladder":
        assert {BY_LAYER_KERNEL, BY_TAIL} <= set(hashed) and {BY_LAYER_KERNEL, BY_TAIL} <= set(folded) and all(w & QUOTIENT for w in path[:13])
    if name.startswith("deep"):
        assert path[0] == BY_FOLD_LEAF | QUOTIENT | BY_FOLD_LEAF << 4 and {BY_LAYER_KERNEL, BY_TAIL} <= set(hashed)
        assert hctx.last_proof_flags()["fri_fold_leaf"]
    if name == "tiny":
        assert set(hashed[:-1]) == {BY_TAIL}


def test_both_commit_forms_give_the_oracles_proof(pkg, gctx, _oracle, oracle_proofs):
    """The `forms` case commits coefficients (form 1). The evaluations of the same polynomials (the oracle's circle_evaluate), committed as
    form 0 in a second session, give the same bytes; the column the case holds twice is one device column passed twice."""
    case = gc.BY_NAME["forms"]
    want = oracle_proofs(case)
    as_coeffs = session_prove(pkg, gctx, case)
    assert as_coeffs[6][0][0] == as_coeffs[6][0][4]
    assert_same_proof(case, as_coeffs, want)
    evals, made = [], {}
    for tree, logs in zip(case.columns(), case.logs):
        evals.append([made.setdefault(id(col), _oracle.evaluate(col[None, :], log, log)[0]) for col, log in zip(tree, logs)])
    assert evals[0][0] is evals[0][4]
    as_evals = session_prove(pkg, gctx, case, columns=evals, form=0)
    assert as_evals[6][0][0] == as_evals[6][0][4]
    assert_same_proof(case, as_evals, want)


def _capture(hp, ctx, conv, cfg):
    """(the proof bfhip_prove_brainfuck returned, its parsed form, the trees' log sizes, [tree][column] = coefficient column)"""
    L = hp.lib()
    ctx.set_conventions(*conv)
    ctx.set_pcs_config(cfg)
    hp._check(L.bfhip_test_capture_polys(ctx._h, 1))
    try:
        raw = hp.prove_brainfuck(CODE, INP, ctx=ctx, log_max_rows=ANCHOR_LMR)
        full = json.loads(raw)
        logs = pcs_replay.tree_log_sizes(hp, [full["claim"][n]["log_size"] for n in pcs_replay.NAMES], ANCHOR_LMR)
        trees = []
        for t in range(4):
            cols = []
            for c, log in enumerate(logs[t]):
                got = ctypes.c_uint32()
                out = np.empty(1 << log, dtype=np.uint32)
                hp._check(L.bfhip_test_captured_poly(ctx._h, t, c, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.size), ctypes.byref(got)))
                assert got.value == log, (t, c)
                cols.append(out)
            trees.append(cols)
    finally:
        hp._check(L.bfhip_test_capture_polys(ctx._h, 0))
    return raw, full, logs, trees


@pytest.mark.parametrize("name,cfg", [("default", None), ("blowup2", dict(pow_bits=8, log_blowup_factor=2, n_queries=10))])
def test_shim_reproduces_the_brainfuck_proof_from_its_captured_trees(hooks_pkg, hctx, gshim, name, cfg):
    """The anchor of the shim: its commit, its prove_values and its serialisation, run over the four trees of a Brainfuck proof under the
    protocol of tests/pcs_replay.py and the shim's own channel, give the "proof" member of that proof — bytes of the oracle's full prover
    (tests/test_gpu_pcs_config.py, tests/test_gpu_prove.py hold the product to them)."""
    hp = hooks_pkg
    kw = cfg or dict(pow_bits=5, log_blowup_factor=1, n_queries=3)
    raw, full, logs, trees = _capture(hp, hctx, gc.STWO, None if cfg is None else hp.PcsConfig(**cfg))
    assert hp.verify_brainfuck(raw, ANCHOR_LMR, gc.STWO, hp.PcsConfig(**kw)) == (True, "")
    log_sizes = [full["claim"][n]["log_size"] for n in pcs_replay.NAMES]
    claimed = [pcs_replay.flat_q(full["interaction_claim"][n]["claimed_sum"]) for n in pcs_replay.NAMES]
    gshim.set_conventions(*gc.STWO)
    ch = gshim.Channel()
    with gshim.Session(max_log_size=max(l for t in logs for l in t), **kw) as s:
        roots = [s.commit(ch, trees[0], logs[0], form=1)]
        for l in log_sizes:
            ch.mix_u64(l)
        roots.append(s.commit(ch, trees[1], logs[1], form=1))
        for _ in range(3):
            ch.draw_felts(2)
        for c in claimed:
            ch.mix_felts([c])
        roots.append(s.commit(ch, trees[2], logs[2], form=1))
        ch.draw_felts(1)
        roots.append(s.commit(ch, trees[3], logs[3], form=1))
        oods = ch.draw_point()
        points, samples = pcs_replay.mask_of(hp, log_sizes, ANCHOR_LMR, oods, 0)
        proof = s.prove_values(ch, points, samples)
    assert roots == [pcs_replay.root_bytes(h) for h in full["proof"]["commitments"]]
    want = pcs_replay.proof_member(raw)
    diff = gc.first_difference(proof, want)
    assert diff is None, "%s: first difference at %s" % (name, diff)
    assert len(proof) == len(want) and proof == want, name
