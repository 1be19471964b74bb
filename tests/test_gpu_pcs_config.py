"""-m gpu: proofs under a configurable PcsConfig (include/bfhip.h `bfhip_pcs_config`). Every non-default config must give the bytes of the CPU
oracle proving under the same config (tests/native/oracle_pcs.cpp), through a single context, a pool and a kept preprocessed tree, in either
launch order; the proof-of-work search must find GrindOps' smallest nonce at the larger pow_bits; and what the device prover does not
support must fail with a clear error and leave the context usable. That holds above log_blowup_factor 1 too (there the oracle evaluates the
constraints on CanonicCoset(log_size + 1) from its committed polynomials, as the device prover does): every proof made here at b > 1 is
compared byte for byte, and tap for tap, with the oracle's, on top of both verifiers, single-flip corruptions and the comparisons across
contexts, pools and launch orders (fib19 at full size with the digest of the oracle's proof, a committed fixture)."""
import ctypes
import hashlib
import json
import os

import pytest

import oracle_pcs
from bf_fuzz import random_program

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CODE, INP = "+++>,<[>+.<-]", b"\x01"
P = (1 << 31) - 1
B1_CONFIGS = [(0, 1), (12, 20), (20, 70), (8, 256)]      # (pow_bits, n_queries) at log_blowup_factor 1


def _prog(name):
    return open(os.path.join(HERE, "golden", "programs", name)).read()


@pytest.fixture(scope="module")
def _shim(tmp_path_factory):
    return oracle_pcs.build(tmp_path_factory.mktemp("oracle_pcs"))


@pytest.fixture
def shim(_shim, conv):
    _shim.set_conventions(*conv)
    yield _shim
    _shim.set_conventions()


@pytest.fixture
def stwo_shim(_shim):
    """The shim under the default conventions, for the tests that are not parametrised over `conv`."""
    _shim.set_conventions()
    yield _shim
    _shim.set_conventions()


_SHIM_PROOFS = {}     # the oracle's (proof, taps) per (conventions, program, input, log_max_rows, config): each CPU proof is made once per module run


def _want(shim, conv, code, inp, lmr, cfg):
    """The oracle's (proof bytes, taps) under cfg; `shim` is set to `conv` already (the `shim` and `stwo_shim` fixtures)."""
    key = (tuple(conv), code, inp, lmr, cfg.pow_bits, cfg.log_blowup_factor, cfg.n_queries)
    if key not in _SHIM_PROOFS:
        _SHIM_PROOFS[key] = shim.prove(code, inp, lmr, pow_bits=cfg.pow_bits, log_blowup_factor=cfg.log_blowup_factor, n_queries=cfg.n_queries)
    return _SHIM_PROOFS[key]


def _assert_oracle_bytes(got, taps, want, want_taps, what=""):
    """Taps first: the first one that differs names the phase (root3: composition; sampled: OODS; fri_commit: quotients or folds; equal taps
    and different bytes: proof of work or decommitment)."""
    assert set(want_taps) == {"root0", "root1", "root2", "root3", "sampled", "fri_commit"}
    for k in ("root0", "root1", "root2", "root3", "sampled", "fri_commit"):
        assert taps[k] == want_taps[k], (k, what)
    assert got == want, what


@pytest.fixture(scope="module")
def _pctx(pkg):
    c = pkg.Context(0, max_log_domain=22)
    yield c
    c.close()


@pytest.fixture
def pctx(_pctx, conv, pkg):
    _pctx.set_conventions(*conv)
    yield _pctx
    _pctx.set_pcs_config(None)
    _pctx.set_mailbox(-1)


def _cfg(pkg, pw, q):
    return pkg.PcsConfig(pow_bits=pw, log_blowup_factor=1, n_queries=q)


@pytest.mark.parametrize("lmr", [17, 20])
def test_explicit_default_config_gives_the_oracle_bytes(pkg, oracle, pctx, lmr):
    pctx.set_pcs_config(pkg.PcsConfig())
    assert pctx.pcs_config() == pkg.PcsConfig()
    got = pkg.prove_brainfuck(CODE, INP, ctx=pctx, log_max_rows=lmr)
    assert got == oracle.prove(CODE, INP, log_max_rows=lmr)[0]


@pytest.mark.parametrize("lmr", [17, 20])
@pytest.mark.parametrize("pw,q", B1_CONFIGS)
def test_blowup_1_configs_give_the_shim_oracle_bytes(pkg, shim, pctx, conv, lmr, pw, q):
    cfg = _cfg(pkg, pw, q)
    got, taps = pkg.prove_brainfuck(CODE, INP, ctx=pctx, log_max_rows=lmr, with_transcript=True, pcs_config=cfg)
    assert pctx.pcs_config() == cfg
    want, want_taps = shim.prove(CODE, INP, lmr, pow_bits=pw, n_queries=q)
    assert {k: taps.get(k) for k in want_taps} == want_taps
    assert got == want
    assert pkg.verify_brainfuck(got, lmr, conventions=conv, pcs_config=cfg) == (True, "")
    assert shim.verify(got, lmr, pow_bits=pw, n_queries=q) == (True, "")
    if (pw, q) != (5, 3):
        assert not pkg.verify_brainfuck(got, lmr, conventions=conv)[0]          # not a default-config proof


@pytest.mark.single_conv
def test_prove_brainfuck_sizes_its_own_context(pkg, shim):
    cfg = _cfg(pkg, 12, 20)
    assert pkg.prove_brainfuck(CODE, INP, log_max_rows=17, pcs_config=cfg) == shim.prove(CODE, INP, 17, pow_bits=12, n_queries=20)[0]


@pytest.fixture(scope="module")
def _bctx(pkg):
    c = pkg.Context(0, max_log_domain=25)      # log_max_rows 20 + blowup 4 + 1
    yield c
    c.close()


@pytest.fixture
def bctx(_bctx, conv):
    _bctx.set_conventions(*conv)
    yield _bctx
    _bctx.set_pcs_config(None)
    _bctx.set_mailbox(-1)


def _flip_first_value(proof, *path):
    """The proof with the first integer under proof[path...] changed (an M31 word + 1 mod p)."""
    d = json.loads(proof)
    node = d
    for k in path:
        node = node[k]

    def flip(x):
        for i, y in enumerate(x):
            if isinstance(y, int):
                x[i] = (y + 1) % P
                return True
            if isinstance(y, list) and flip(y):
                return True
        return False
    assert flip(node)
    return json.dumps(d, separators=(",", ":")).encode()


@pytest.mark.parametrize("lmr", [17, 20])
@pytest.mark.parametrize("b,pw,q", [(2, 12, 20), (3, 8, 24), (4, 10, 20)])
def test_blowup_above_1_gives_the_shim_oracle_bytes(pkg, shim, bctx, conv, lmr, b, pw, q):
    """At log_max_rows 17 and b >= 2 the first FRI line layers have 2^17 rows or more: the fused fold-and-leaf launch runs under these configs."""
    cfg = pkg.PcsConfig(pow_bits=pw, log_blowup_factor=b, n_queries=q)
    got, taps = pkg.prove_brainfuck(CODE, INP, ctx=bctx, log_max_rows=lmr, with_transcript=True, pcs_config=cfg)
    _assert_oracle_bytes(got, taps, *_want(shim, conv, CODE, INP, lmr, cfg))
    assert pkg.verify_brainfuck(got, lmr, conventions=conv, pcs_config=cfg) == (True, "")
    assert shim.verify(got, lmr, pow_bits=pw, log_blowup_factor=b, n_queries=q) == (True, "")
    assert not pkg.verify_brainfuck(got, lmr, conventions=conv)[0]
    assert not pkg.verify_brainfuck(got, lmr, conventions=conv, pcs_config=pkg.PcsConfig(pow_bits=pw, log_blowup_factor=b - 1, n_queries=q))[0]
    for path in (("proof", "queried_values", 1), ("proof", "fri_proof", "last_layer_poly", "coeffs")):
        bad = _flip_first_value(got, *path)
        assert not pkg.verify_brainfuck(bad, lmr, conventions=conv, pcs_config=cfg)[0], path
        assert not shim.verify(bad, lmr, pow_bits=pw, log_blowup_factor=b, n_queries=q)[0], path


@pytest.mark.single_conv
@pytest.mark.parametrize("b,lmr,code,inp", [(5, 12, CODE, INP), (6, 12, CODE, INP), (6, 12, "++[-]+.", b""), (8, 12, CODE, INP), (16, 8, "+>+<-.", b"")],
                         ids=["b5", "b6", "b6_with_a_32_row_component", "b8", "b16"])
def test_large_blowups_the_config_promises(pkg, shim, conv, b, lmr, code, inp):
    """bfhip_pcs_config advertises 1 <= log_blowup_factor <= 16. From 6 up (5 with a 2^5-row component) the row-granular columns of the 2^4- and
    2^5-row components are polynomials of ONE or TWO coefficients extended past 32 cells, which the transform planner used to refuse: every
    such proof failed. Same assertions as above, whole proofs and all taps against the oracle included (b = 16 at log_max_rows 8 too: its CPU
    proof, on domains of 2^24 and more cells, took 50 s on 8 cores when this was written)."""
    pw, q = 8, 6
    cfg = pkg.PcsConfig(pow_bits=pw, log_blowup_factor=b, n_queries=q)
    c = pkg.Context(0, max_log_domain=lmr + b + 1)
    try:
        got, taps = pkg.prove_brainfuck(code, inp, ctx=c, log_max_rows=lmr, with_transcript=True, pcs_config=cfg)
    finally:
        c.close()
    _assert_oracle_bytes(got, taps, *_want(shim, conv, code, inp, lmr, cfg))
    assert pkg.verify_brainfuck(got, lmr, conventions=conv, pcs_config=cfg) == (True, "")
    assert shim.verify(got, lmr, pow_bits=pw, log_blowup_factor=b, n_queries=q) == (True, "")
    assert not pkg.verify_brainfuck(got, lmr, conventions=conv)[0]
    assert not pkg.verify_brainfuck(got, lmr, conventions=conv, pcs_config=pkg.PcsConfig(pow_bits=pw, log_blowup_factor=b - 1, n_queries=q))[0]
    bad = _flip_first_value(got, "proof", "queried_values", 1)
    assert not pkg.verify_brainfuck(bad, lmr, conventions=conv, pcs_config=cfg)[0]
    assert not shim.verify(bad, lmr, pow_bits=pw, log_blowup_factor=b, n_queries=q)[0]


def _ten_sizes_program():
    return random_program(40402, 6000, min_steps=300)[:2]      # tests/test_gpu_fuzz.py::test_program_with_ten_distinct_component_sizes


SMALL_SHAPES = {
    "ten_component_sizes": (_ten_sizes_program, 17),      # its memory table has 2^17 rows: the one shape here above 2^14
    "a-bc": (lambda: (_prog("a-bc.bf"), b"a"), 12),
    "32_row_component": (lambda: ("++[-]+.", b""), 12),
    "empty_loops": (lambda: ("[][]+[-]", b""), 14),
}
SMALL_SHAPES.update({"fuzz_seed_%d" % s: (lambda s=s: random_program(s, 400, min_steps=20)[:2], 12 + s % 3) for s in range(701, 707)})


@pytest.mark.parametrize("b", [2, 3])
@pytest.mark.parametrize("shape", list(SMALL_SHAPES))
def test_small_shapes_at_blowup_2_and_3_give_the_shim_oracle_bytes(pkg, shim, bctx, conv, shape, b):
    """Other component-size patterns than the sweep program's, at log_max_rows 12 to 14: components of 16 and 32 rows under preprocessed
    columns of 2^12 rows and more, loops that never run, six generated programs — and ten distinct component sizes (ten composition
    accumulators, each evaluated on its own domain), whose program needs log_max_rows 17."""
    make, lmr = SMALL_SHAPES[shape]
    code, inp = make()
    cfg = pkg.PcsConfig(pow_bits=8, log_blowup_factor=b, n_queries=12)
    got, taps = pkg.prove_brainfuck(code, inp, ctx=bctx, log_max_rows=lmr, with_transcript=True, pcs_config=cfg)
    if shape == "ten_component_sizes":
        assert len({c["log_size"] for c in json.loads(got)["claim"].values()}) >= 10
    _assert_oracle_bytes(got, taps, *_want(shim, conv, code, inp, lmr, cfg), what=code)
    assert pkg.verify_brainfuck(got, lmr, conventions=conv, pcs_config=cfg) == (True, "")


@pytest.mark.single_conv
def test_unsupported_settings_fail_clearly(pkg, oracle, pctx):
    want = oracle.prove(CODE, INP, log_max_rows=17)[0]
    for bad in (pkg.PcsConfig(n_queries=0), pkg.PcsConfig(n_queries=257), pkg.PcsConfig(log_blowup_factor=0), pkg.PcsConfig(log_blowup_factor=17),
                pkg.PcsConfig(log_last_layer_degree_bound=1), pkg.PcsConfig(pow_bits=33)):
        with pytest.raises(pkg.BfhipError, match="bfhip_pcs_config"):
            pctx.set_pcs_config(bad)
    r = pkg.PcsConfig()
    r.reserved[0] = 7
    with pytest.raises(pkg.BfhipError, match="reserved"):
        pctx.set_pcs_config(r)
    assert pctx.pcs_config() == pkg.PcsConfig()         # a refused config changes nothing
    assert pkg.prove_brainfuck(CODE, INP, ctx=pctx, log_max_rows=17) == want
    # Poseidon252 channel: its nonce search runs on the host — more than 12 bits are refused when the proof starts
    pctx.set_conventions(0, 0, 0, 1)
    pctx.set_pcs_config(_cfg(pkg, 13, 10))
    with pytest.raises(pkg.BfhipError, match="Poseidon252 channel: pow_bits > 12"):
        pkg.prove_brainfuck(CODE, INP, ctx=pctx, log_max_rows=17)
    pctx.set_conventions(0, 0, 0, 0)
    assert pkg.prove_brainfuck(CODE, INP, ctx=pctx, log_max_rows=17) != want       # still the 13-bit config, now on Blake2s
    # a twiddle tree too small for log_max_rows + log_blowup_factor + 1 names the size it needs (pctx: max_log_domain 22)
    pctx.set_pcs_config(pkg.PcsConfig(log_blowup_factor=3, n_queries=20))
    with pytest.raises(pkg.BfhipError, match="max_log_domain >= 23"):
        pkg.prove_brainfuck(CODE, INP, ctx=pctx, log_max_rows=19)
    pctx.set_pcs_config(None)
    with pytest.raises(pkg.BfhipError, match="max_log_domain >= 23"):
        pkg.prove_brainfuck(CODE, INP, ctx=pctx, log_max_rows=21)
    assert pkg.prove_brainfuck(CODE, INP, ctx=pctx, log_max_rows=17) == want


@pytest.mark.single_conv
def test_shard_group_keeps_the_default_config(pkg, oracle):
    want = oracle.prove(CODE, INP, log_max_rows=17)[0]
    g = pkg.LocalGroup(2)
    c = pkg.Context(0, max_log_domain=20)
    try:
        c.set_pcs_config(_cfg(pkg, 12, 20))
        with pytest.raises(pkg.BfhipError, match="non-default PcsConfig cannot join a shard group"):
            c.join_local_group(g, 0)
        c.set_pcs_config(None)
        assert pkg.prove_brainfuck(CODE, INP, ctx=c, log_max_rows=17) == want
    finally:
        c.close()
        g.close()


def test_pool_batch_gives_the_single_context_bytes(pkg, shim, bctx, conv):
    cfg = pkg.PcsConfig(pow_bits=12, log_blowup_factor=2, n_queries=20)
    progs = [(CODE, INP), ("++[-]+.", b""), (_prog("a-bc.bf"), b"a"), ("[][]+[-]", b"")]
    bctx.set_pcs_config(cfg)
    want = [pkg.prove_brainfuck(c, i, ctx=bctx, log_max_rows=18) for c, i in progs]
    assert want == [_want(shim, conv, c, i, 18, cfg)[0] for c, i in progs]      # ... which are the oracle's: the pool is pinned through them
    pool = pkg.Pool(0, n_in_flight=2, max_log_domain=21)
    try:
        pool.set_conventions(*conv)
        pool.set_pcs_config(cfg)
        assert pool.ctx(1).pcs_config() == cfg
        proofs, _ = pool.prove_batch_brainfuck(progs, log_max_rows=18)
        assert proofs == want
    finally:
        pool.close()


def _fresh_proof(pkg, cfg, lmr=18):
    c = pkg.Context(0, max_log_domain=lmr + cfg.log_blowup_factor + 1)
    try:
        return pkg.prove_brainfuck(CODE, INP, ctx=c, log_max_rows=lmr, pcs_config=cfg)
    finally:
        c.close()


@pytest.mark.single_conv
def test_kept_preprocessed_trees_follow_the_blowup(pkg, stwo_shim):
    """Pool mode 2 and a context that keeps its preprocessed tree, alternating b = 1 -> 2 -> 1 -> 2: every proof is a fresh context's bytes
    (the IsFirst LDE depends on the blowup: a tree kept from the other blowup must not serve the proof), and those are the oracle's."""
    seq = [pkg.PcsConfig(pow_bits=8, log_blowup_factor=b, n_queries=20) for b in (1, 2, 1, 2)]
    want = {cfg.log_blowup_factor: _fresh_proof(pkg, cfg) for cfg in seq[:2]}
    for cfg in seq[:2]:
        assert want[cfg.log_blowup_factor] == _want(stwo_shim, (0, 0, 0, 0), CODE, INP, 18, cfg)[0], cfg
    c = pkg.Context(0, max_log_domain=21)
    pool = pkg.Pool(0, n_in_flight=2, max_log_domain=21, preprocessed=2)
    try:
        pkg.lib().bfhip_ctx_reuse_preprocessed(c._h, 1)
        for n, cfg in enumerate(seq):
            b = cfg.log_blowup_factor
            assert pkg.prove_brainfuck(CODE, INP, ctx=c, log_max_rows=18, pcs_config=cfg) == want[b], (n, b)
            assert not c.last_proof_flags()["kept_preprocessed"]      # the kept tree is always the other blowup's: rebuilt
            pool.set_pcs_config(cfg)
            proofs, _ = pool.prove_batch_brainfuck([(CODE, INP)] * 2, log_max_rows=18)
            assert proofs == [want[b]] * 2, (n, b)
        assert pkg.prove_brainfuck(CODE, INP, ctx=c, log_max_rows=18, pcs_config=seq[-1]) == want[2]
        assert c.last_proof_flags()["kept_preprocessed"]              # same blowup again: the kept tree serves
    finally:
        pkg.lib().bfhip_ctx_reuse_preprocessed(c._h, 0)
        c.close()
        pool.close()


@pytest.mark.single_conv
def test_mailbox_order_on_and_off_give_the_same_bytes(pkg, stwo_shim):
    code = _prog("collatz.bf")
    c = pkg.Context(0, max_log_domain=24)
    try:
        got = []
        c.set_pcs_config(pkg.PcsConfig(pow_bits=20, log_blowup_factor=2, n_queries=35))
        for mode in (1, 0):
            c.set_mailbox(mode)
            got.append(pkg.prove_brainfuck(code, b"7\n", ctx=c, log_max_rows=21))
            assert c.last_proof_flags()["mailbox_order"] == (mode == 1)
        assert got[0] == got[1]
        assert got[0] == _want(stwo_shim, (0, 0, 0, 0), code, b"7\n", 21, c.pcs_config())[0]
        assert pkg.verify_brainfuck(got[0], 21, pcs_config=c.pcs_config()) == (True, "")
    finally:
        c.close()


@pytest.mark.single_conv
def test_256_queries_split_the_decommitment_gather(pkg):
    """fib19 at 256 queries builds more gather requests than a quarter of the staging ring holds: the split path runs and the proof verifies."""
    cfg = _cfg(pkg, 8, 256)
    c = pkg.Context(0, max_log_domain=26)
    try:
        tr = pkg.Trace(c, _prog("fib19.bf"))
        c.set_pcs_config(cfg)
        proof, _ = tr.prove(24)
        assert c.last_proof_flags()["split_gather"]
        tr.close()
    finally:
        c.close()
    assert pkg.verify_brainfuck(proof, 24, pcs_config=cfg) == (True, "")


def test_grind_finds_the_smallest_nonce_at_pow_16_to_22(pkg, oracle, pctx):
    oracle.L.orc_grind_digest.restype = ctypes.c_uint64
    for i in range(16):
        pow_bits = 16 + i % 7
        digest = hashlib.blake2s(b"bfhip pcs grind %d" % i).digest()
        assert pctx.grind(digest, pow_bits) == oracle.L.orc_grind_digest(digest, pow_bits), (i, pow_bits)


@pytest.mark.single_conv
def test_poseidon252_with_a_non_default_config_verifies(pkg, shim, pctx):
    pctx.set_conventions(0, 0, 0, 1)
    shim.set_conventions(0, 0, 0, 1)
    cfg = pkg.PcsConfig(pow_bits=8, log_blowup_factor=2, n_queries=10)
    got, taps = pkg.prove_brainfuck(CODE, INP, ctx=pctx, log_max_rows=17, with_transcript=True, pcs_config=cfg)
    _assert_oracle_bytes(got, taps, *_want(shim, (0, 0, 0, 1), CODE, INP, 17, cfg))
    assert pkg.verify_brainfuck(got, 17, conventions=(0, 0, 0, 1), pcs_config=cfg) == (True, "")
    assert shim.verify(got, 17, pow_bits=8, log_blowup_factor=2, n_queries=10) == (True, "")
    assert not pkg.verify_brainfuck(got, 17, conventions=(0, 0, 0, 1))[0]


@pytest.mark.single_conv
def test_fib19_full_size_at_b2_pow20_q20_verifies(pkg):
    """The oracle's proof at this size takes minutes and 56 GiB: its size and SHA-256 are a fixture (tests/golden/make_fib19_b2_proof_digest.py)."""
    golden = json.load(open(os.path.join(HERE, "golden", "fib19_lmr24_b2_pow20_q20_oracle_proof.json")))["stwo"]
    cfg = pkg.PcsConfig(pow_bits=20, log_blowup_factor=2, n_queries=20)
    c = pkg.Context(0, max_log_domain=27)
    try:
        c.set_pcs_config(cfg)
        tr = pkg.Trace(c, _prog("fib19.bf"))
        proof, _ = tr.prove(24)
        tr.close()
    finally:
        c.close()
    assert golden["pcs_config"] == {"pow_bits": cfg.pow_bits, "log_blowup_factor": cfg.log_blowup_factor, "n_queries": cfg.n_queries}
    assert (len(proof), hashlib.sha256(proof).hexdigest()) == (golden["proof_bytes"], golden["sha256"])
    assert pkg.verify_brainfuck(proof, 24, pcs_config=cfg) == (True, "")
    assert not pkg.verify_brainfuck(proof, 24)[0]
    bad = proof.replace(b'"proof_of_work":', b'"proof_of_work":1', 1)
    assert not pkg.verify_brainfuck(bad, 24, pcs_config=cfg)[0]
