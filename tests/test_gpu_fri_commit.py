"""GPU: the FRI commit phase at op level (HipProver::fri_commit, csrc/prover_fri.hip) through bfhip_test_fri_commit of libbfhip_testhooks.so.

The driver picks one of four paths per layer — the fold inside the leaf launch (k_fri_fold_leaf, 2^17 rows and above), k_fri_layer (2^11 .. 2^16:
fold, subtrees, ticket counter, channel step), k_fri_tail (2^10 and below: everything left in one workgroup) and separate launches (the plain folds,
merkle_run with the channel step in k_merkle_top). Whole proofs compare bytes with the oracle, which sees what a proof reads: n_queries paths per
tree, layers that all take a quotient, a channel that has never rejected a draw. Here the real driver runs on the test's columns and EVERYTHING
it leaves in HBM is compared, bit for bit, with tests/fri_commit_model.py: every layer, every node of every tree (the nodes go to LDS and to HBM
separately: a node stored at a wrong index still gives the right root), alpha || alpha^2 of every channel step, the final channel, and which path
produced each layer, taken from the driver's own decisions. A mismatch names the first differing (layer, coordinate, row) or (tree, level, node).

The rejected draw (a word >= 2P, 2^-28 per draw) is reached through tests/golden/channel_redraw.json: initial digests found by search for which
a chosen step redraws — in k_merkle_top (R1), k_fri_layer (R2) and k_fri_tail (R3, R4), each also with the layer chain cut so that the redrawing
step is the last one and its n_sent = 2 is what stays in the device channel. The one-lane copy (channel_step / k_channel_mix_root_draw) runs only
for a tree without a fused top (fused_top == 0: replicated small levels, or Poseidon252 whose channel is on the host); an FRI tree never is one.

Mutation runs (value-only changes on a scratch copy, one GPU run each): see MUTATIONS below."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import field_inputs as fi
import fri_commit_model as model
from conftest import P

pytestmark = pytest.mark.gpu

MUTATIONS = """
Each mutant: csrc/merkle.hip changed in one place on a scratch copy, both libraries rebuilt, this module run, then the whole-proof parity tests from before
(test_gpu_prove.py, test_gpu_fri_fold_leaf.py, test_gpu_pcs_config.py -k oracle -x; for 1 to 6 also test_gpu_fuzz.py). new: of the 33 tests here.
1 k_fri_layer   two `sel` cases swapped (yinv)                  new: caught, 11 tests (every case with a quotient at 2^11 .. 2^16, none of the "largest" ones)   old: caught by the first proof
2 k_fri_tail    k_alpha_sq -> k_alpha in the quotient fold-in    new: caught, 16 tests                                                               old: caught by the first proof
3 k_fri_layer   the `- P31` of a drawn word dropped              new: caught, 17 tests (alpha || alpha^2 of the step is named)                      old: caught by the first proof
4 k_fri_layer   hash_to_hbm at j instead of node0 + j            new: caught, 17 tests (tree, level, node named; roots and layers agree)            old: caught by the first proof
5 k_fri_tail    a narrow inner level stored at tree[lg + 1]      new: caught, 29 tests ("tree of layer 0: first differing (level, node) 4, 0")      old: caught by the first proof
6 k_fri_tail    ONE node (300) of the wide levels stored at 301  new: caught, 25 tests (every case with a tree of 2^9 rows or more)                  old: 29 proofs pass, the 30th (hello1.bf) opens that node
7 k_fri_tail    fold WITHOUT a quotient doubled (else branch)    new: caught, 29 tests                                                               old: caught by the first proof (the layers below 2^(3+b) rows of a proof have no quotient)
8 k_fri_tail    alpha's words rotated ONLY behind a rejected draw  new: caught, exactly R3-1, R3-9, R4-1, R4-8                                       old: missed (195 passed): no proof has ever redrawn
9 k_fri_layer   fold WITHOUT a quotient doubled (else branch)    new: caught, 11 tests ("largest" / "every_other" at 12, 17, 18, log_blowup 3, R2)   old: missed (195 passed): at 2^11 .. 2^16 rows a proof always has a quotient
Not mutated, on purpose: loop conditions, barriers, the ticket counter, n_sent (a mutant that may not terminate is not run).
"""

HERE = os.path.dirname(os.path.abspath(__file__))
BY_LAUNCHES, BY_FOLD_LEAF, BY_LAYER_KERNEL, BY_TAIL, QUOTIENT, NO_TREE = 0, 1, 2, 3, 4, 15      # HipProver::FriCommitted::path (csrc/prover.h)
LINE_LOGS = (4, 10, 11, 12, 17, 18)
PATTERNS = ("every", "largest", "every_other")
STWO, RFC7693, POSEIDON = (0, 0, 0, 0), (1, 0, 0, 0), (0, 0, 0, 1)


def _zero_or_max(seed, n):
    """Every cell 0 or P - 1."""
    return np.where(fi.uniform(seed ^ 0x5A7, n) & 1, np.uint32(P - 1), np.uint32(0)).astype(np.uint32)


FAMILIES = dict({k: fi.FAMILIES[k] for k in ("uniform", "max", "edge", "complement1", "complement2", "equal1", "equal2")}, zero_or_max=_zero_or_max)
BIG_FAMILIES = ("uniform", "max", "edge")      # line_log >= 17


def _families(line_log):
    return BIG_FAMILIES if line_log >= 17 else tuple(FAMILIES)


@functools.lru_cache(maxsize=None)
def _data(family, line_log, pattern, log_blowup):
    q = model.quotient_columns(FAMILIES[family], tuple(model.pattern_sizes(pattern, line_log, log_blowup)))
    for _, cols in q:
        for c in cols:
            c.setflags(write=False)
            assert c.dtype == np.uint32 and int(c.max()) < P
    return q


def _constant(line_log, value):
    return [(line_log + 1, [np.full(2 << line_log, c, dtype=np.uint32) for c in value])]


def _want(L, conv, family, line_log, pattern, log_blowup):
    """The model's result, computed once per case and left unchanged (kept for the module where a case is used twice; the trees of a 2^18-row
    case are 64 MB). L: the oracle, switched to `conv` for the call."""
    keep = line_log < 17 or (line_log == 17 and pattern == "every" and conv == STWO)
    return (_want_kept if keep else _want_once)(L, conv, family, line_log, pattern, log_blowup)


def _want_once(L, conv, family, line_log, pattern, log_blowup):
    with L.conventions(conv):
        return model.commit(L.lib, _data(family, line_log, pattern, log_blowup), log_blowup, bytes(32), oracle_channel=conv[3] == 1)


_want_kept = functools.lru_cache(maxsize=None)(_want_once)


class _Lib:
    """The oracle library with a scoped convention switch (the switch is process-wide: always put back)."""

    def __init__(self, oracle):
        self.oracle, self.lib = oracle, oracle.L

    def conventions(self, conv):
        o = self.oracle

        class Scope:
            def __enter__(self):
                o.set_conventions(*conv)

            def __exit__(self, *exc):
                o.set_conventions(0, 0, 0, 0)
        return Scope()


@pytest.fixture(scope="module")
def orc(_oracle):
    return _Lib(_oracle)


@pytest.fixture(scope="module")
def _hctx(hooks_pkg):
    c = hooks_pkg.Context(0, max_log_domain=20)
    yield c
    c.close()


@pytest.fixture
def hctx(_hctx):
    """The module's context on libbfhip_testhooks.so, at the default conventions and PcsConfig before and after every test."""
    _hctx.set_conventions(*STWO); _hctx.set_pcs_config(None)
    yield _hctx
    _hctx.set_conventions(*STWO); _hctx.set_pcs_config(None)


@pytest.fixture(scope="module", autouse=True)
def _drop_cached():
    yield
    _data.cache_clear(); _want_kept.cache_clear()


def _level_offset(max_log, lg):
    return (2 << max_log) - (2 << lg)      # nodes of the levels max_log .. lg + 1, stored in front of level lg


def run_hook(hooks_pkg, c, quotients, digest=bytes(32)):
    """bfhip_test_fri_commit on context c (its conventions and PcsConfig as set). Returns what fri_commit_model.commit returns, plus "paths"."""
    log_blowup = c.pcs_config().log_blowup_factor
    sizes = [lg for lg, _ in quotients]
    line_log = sizes[0] - 1
    n_inner = max(line_log - log_blowup, 0)
    layer_logs = [line_log - k for k in range(n_inner + 1)]
    tree_logs = [sizes[0]] + layer_logs[:-1]
    layers = np.full(sum(4 << lg for lg in layer_logs), 0xDEADBEEF, dtype=np.uint32)
    trees = np.full((sum((2 << lg) - 1 for lg in tree_logs), 8), 0xDEADBEEF, dtype=np.uint32)
    roots, alphas = np.zeros((n_inner + 1, 8), dtype=np.uint32), np.zeros((n_inner + 1, 8), dtype=np.uint32)
    chan, paths = np.zeros(9, dtype=np.uint32), np.zeros(n_inner + 1, dtype=np.uint32)
    cols = [np.ascontiguousarray(a, dtype=np.uint32) for _, four in quotients for a in four]
    for (lg, _), k in zip(quotients, range(len(quotients))):
        assert all(a.size == 1 << lg for a in cols[4 * k:4 * k + 4])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = hooks_pkg.lib().bfhip_test_fri_commit(c._h, bytes(digest), ctypes.c_uint32(len(sizes)), (ctypes.c_uint32 * len(sizes))(*sizes),
                                               (ctypes.c_void_p * len(cols))(*[a.ctypes.data for a in cols]), p(layers), p(trees), p(roots), p(alphas), p(chan), p(paths))
    if rc != 0:
        raise hooks_pkg.BfhipError(hooks_pkg.lib().bfhip_last_error().decode())
    out = {"layers": [], "trees": [], "roots": [r.tobytes() for r in roots], "alphas": alphas, "digest": chan[:8].tobytes(), "n_sent": int(chan[8]), "paths": [int(x) for x in paths]}
    o = 0
    for lg in layer_logs:
        out["layers"].append(layers[o:o + (4 << lg)].reshape(4, 1 << lg)); o += 4 << lg
    o = 0
    for lg in tree_logs:
        out["trees"].append(trees[o:o + (2 << lg) - 1]); o += (2 << lg) - 1
    return out


def compare(got, want, tag):
    """Bit-exact, in the order of the data flow; names the first difference."""
    assert len(got["layers"]) == len(want["layers"]) and len(got["trees"]) == len(want["trees"]), tag
    assert got["roots"][0] == want["roots"][0], (tag, "root of the first-layer tree")
    for k in range(len(want["layers"])):
        g, w = got["layers"][k], want["layers"][k]
        assert g.shape == w.shape, (tag, "layer", k)
        assert got["alphas"][k].tolist() == want["alphas"][k].tolist(), (tag, "alpha || alpha^2 of channel step %d (drawn behind %s)" % (k, "the first-layer tree" if k == 0 else "layer %d" % (k - 1)))
        bad = np.nonzero(g != w)
        assert bad[0].size == 0, (tag, "layer %d (2^%d rows): first differing (coordinate, row)" % (k, w.shape[1].bit_length() - 1), int(bad[0][0]), int(bad[1][0]),
                                  "path", got["paths"][k])
    for t in range(len(want["trees"])):
        g, w = got["trees"][t], want["trees"][t]
        assert g.shape == w.shape, (tag, "tree", t)
        bad = np.nonzero(np.any(g != w, axis=1))[0]
        if bad.size:
            max_log = (w.shape[0] + 1).bit_length() - 2
            lg = next(l for l in range(max_log, -1, -1) if bad[0] < _level_offset(max_log, l) + (1 << l))
            name = "first-layer tree" if t == 0 else "tree of layer %d" % (t - 1)
            assert False, (tag, name + ": first differing (level, node)", lg, int(bad[0]) - _level_offset(max_log, lg), "path", None if t == 0 else got["paths"][t - 1])
        assert got["roots"][t] == want["roots"][t] == w[-1].tobytes(), (tag, "root of tree", t)
    assert got["digest"] == want["digest"], (tag, "final channel digest")
    assert want["n_sent"] is None or got["n_sent"] == want["n_sent"], (tag, "final n_sent", got["n_sent"])


def expected_paths(line_log, sizes, log_blowup):
    """What the driver's thresholds give under the device channel (the issue's table): checks the report, not the driver."""
    out = []
    for k in range(line_log - log_blowup + 1):
        lg = line_log - k
        fold = BY_FOLD_LEAF if lg >= 17 and lg > log_blowup else BY_LAYER_KERNEL if 11 <= lg <= 16 and 1 <= k and lg > log_blowup else BY_TAIL if lg < 10 and k >= 1 else BY_LAUNCHES
        tree = NO_TREE if lg == log_blowup else BY_FOLD_LEAF if lg >= 17 else BY_LAYER_KERNEL if 11 <= lg <= 16 and k >= 1 else BY_TAIL if lg <= 10 else BY_LAUNCHES
        out.append(fold | (QUOTIENT if lg + 1 in sizes else 0) | tree << 4)
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("line_log", LINE_LOGS)
def test_commit_phase_equals_the_model(hooks_pkg, hctx, orc, line_log, pattern):
    sizes = model.pattern_sizes(pattern, line_log, 1)
    for family in _families(line_log):
        got = run_hook(hooks_pkg, hctx, _data(family, line_log, pattern, 1))
        assert got["paths"] == expected_paths(line_log, sizes, 1), (line_log, pattern, got["paths"])
        compare(got, _want(orc, STWO, family, line_log, pattern, 1), (line_log, pattern, family))


@pytest.mark.parametrize("line_log", (12, 17))
def test_rfc7693_node_hashes(hooks_pkg, hctx, orc, line_log):
    """The other node-hash convention (rfc = 0xFFFFFFFF in k_fri_layer / k_fri_tail, the RFC leaf and node shapes of the layer kernels)."""
    hctx.set_conventions(*RFC7693)
    for pattern in PATTERNS:
        for family in BIG_FAMILIES:
            got = run_hook(hooks_pkg, hctx, _data(family, line_log, pattern, 1))
            want = _want(orc, RFC7693, family, line_log, pattern, 1)
            assert line_log != 12 or want["roots"] != _want(orc, STWO, family, line_log, pattern, 1)["roots"]
            compare(got, want, (line_log, pattern, family, "rfc7693"))


def test_log_blowup_3_ends_the_tail_at_8_rows(hooks_pkg, hctx, orc):
    hctx.set_pcs_config(hooks_pkg.PcsConfig(log_blowup_factor=3))
    for pattern in PATTERNS:
        sizes = model.pattern_sizes(pattern, 12, 3)
        assert min(sizes) >= 7
        for family in ("uniform", "edge", "zero_or_max"):
            got = run_hook(hooks_pkg, hctx, _data(family, 12, pattern, 3))
            assert got["layers"][-1].shape == (4, 8) and got["paths"] == expected_paths(12, sizes, 3)
            compare(got, _want(orc, STWO, family, 12, pattern, 3), (12, pattern, family, "log_blowup 3"))


def test_repeated_commits_on_one_context(hooks_pkg, hctx, orc):
    """Six k_fri_layer launches per 2^17 commit share one ticket counter, which every last workgroup puts back to zero: twice in a row, and
    after a commit of another shape."""
    for line_log, family in ((17, "uniform"), (17, "uniform"), (12, "edge"), (17, "max"), (17, "uniform")):
        got = run_hook(hooks_pkg, hctx, _data(family, line_log, "every", 1))
        compare(got, _want(orc, STWO, family, line_log, "every", 1), (line_log, family, "repeated"))


def test_poseidon252_host_channel(hooks_pkg, hctx, orc):
    """merkle_channel 1: nothing is fused — every fold is k_fold_line_circle (or the circle fold of layer 0), every tree a merkle_commit of the
    Poseidon252 layer kernel, the channel stepped on the host by commit_step at every layer size."""
    hctx.set_conventions(*POSEIDON)
    for family in ("uniform", "edge"):
        got = run_hook(hooks_pkg, hctx, _data(family, 12, "every", 1))
        sizes = model.pattern_sizes("every", 12, 1)
        assert got["paths"] == [BY_LAUNCHES | (QUOTIENT if 13 - k in sizes else 0) | (NO_TREE if k == 11 else BY_LAUNCHES) << 4 for k in range(12)]
        assert got["n_sent"] == 1
        compare(got, _want(orc, POSEIDON, family, 12, "every", 1), (12, family, "poseidon252"))


def test_every_path_ran(hooks_pkg, hctx):
    """From the driver's own report: all four paths, and the three folds without a quotient (FF_LINE in the leaf launch, k_fri_layer and
    k_fold_line_circle with a null quotient), over the cases of this module."""
    seen, trees = set(), set()
    for line_log in LINE_LOGS:
        for pattern in PATTERNS:
            paths = run_hook(hooks_pkg, hctx, _data("uniform", line_log, pattern, 1))["paths"]
            seen |= {(p & 3, bool(p & QUOTIENT), k == 0) for k, p in enumerate(paths)}
            trees |= {p >> 4 for p in paths}
    folds = {(who, quot) for who, quot, _ in seen}
    assert folds == {(who, quot) for who in (BY_LAUNCHES, BY_FOLD_LEAF, BY_LAYER_KERNEL, BY_TAIL) for quot in (False, True)}, folds
    assert (BY_FOLD_LEAF, False, False) in seen          # FF_LINE
    assert (BY_LAYER_KERNEL, False, False) in seen       # k_fri_layer, a.quot[0] == nullptr
    assert (BY_LAUNCHES, False, False) in seen           # k_fold_line_circle, q == nullptr
    assert trees == {BY_LAUNCHES, BY_FOLD_LEAF, BY_LAYER_KERNEL, BY_TAIL, NO_TREE}, trees


@pytest.mark.single_conv
def test_a_proof_after_a_hook_call_is_the_oracles(hooks_pkg, hctx, oracle, orc):
    """The hook resets the proof arena and leaves the staging ring, the ticket counter and the pinned blocks as a proof would find them."""
    got = run_hook(hooks_pkg, hctx, _data("uniform", 12, "every", 1))
    compare(got, _want(orc, STWO, "uniform", 12, "every", 1), (12, "before the proof"))
    code = "++>+++[<+>-]<."
    assert hooks_pkg.prove_brainfuck(code, b"", ctx=hctx, log_max_rows=16) == oracle.prove(code, b"", log_max_rows=16)[0]
    got = run_hook(hooks_pkg, hctx, _data("edge", 12, "every", 1))
    compare(got, _want(orc, STWO, "edge", 12, "every", 1), (12, "after the proof"))


def test_hook_refuses_what_it_cannot_run(hooks_pkg, hctx):
    """(more layers than the driver allows — 40 — would need a column of 2^42 rows: that refusal has no case.)"""
    col = lambda lg: [np.zeros(1 << lg, dtype=np.uint32) for _ in range(4)]
    for sizes, msg in (((6, 6), "distinct and descending"), ((5, 6), "distinct and descending"), ((6, 1), "below log_blowup_factor \\+ 1"), ((6, 2), "at least 8 rows"),
                       ((20,), "twiddle tree")):      # 2^20 rows on a context whose twiddle tree ends at 2^19
        with pytest.raises(hooks_pkg.BfhipError, match=msg):
            run_hook(hooks_pkg, hctx, [(lg, col(lg)) for lg in sizes])
    hctx.set_pcs_config(hooks_pkg.PcsConfig(log_blowup_factor=6))
    with pytest.raises(hooks_pkg.BfhipError, match="below log_blowup_factor \\+ 1"):
        run_hook(hooks_pkg, hctx, [(9, col(9)), (6, col(6))])
    hctx.set_pcs_config(None)
    assert run_hook(hooks_pkg, hctx, [(6, col(6))])["paths"] == [BY_LAUNCHES | QUOTIENT | BY_TAIL << 4, BY_TAIL | BY_TAIL << 4, BY_TAIL | BY_TAIL << 4, BY_TAIL | BY_TAIL << 4,
                                                                  BY_TAIL | NO_TREE << 4]      # the context is usable afterwards


# ---- the rejected draw ----------------------------------------------------------------------------------------------------------------------
CONSTANT = (1234567, 7654321, P - 1, 5)      # make_channel_redraw_fixtures.py: the constant column of R2 .. R4
# fixture, log_blowup values: 1 = the whole chain behind the redrawn alpha; the other cuts the chain so that the redrawing step is the LAST one
# and its n_sent = 2 stays in the device channel (R2: the layers 2^12, 2^11 and a last layer of 2^10 rows; R3: 2^10 | 2^9; R4: 2^10, 2^9 | 2^8)
REDRAWS = [("R1", 1), ("R2", 1), ("R2", 10), ("R3", 1), ("R3", 9), ("R4", 1), ("R4", 8)]


@pytest.mark.parametrize("name,log_blowup", REDRAWS)
def test_rejected_draw_is_redrawn_on_the_device(hooks_pkg, hctx, orc, name, log_blowup):
    """The step's alpha must be the SECOND draw's words (counter 1) mod P, every later layer is folded with it, and the host's replay of the channel
    (which the driver compares with the device's, digest and n_sent) must agree: a diverged channel raises from the hook."""
    fx = json.load(open(os.path.join(HERE, "golden", "channel_redraw.json")))[name]
    line_log, step, digest = fx["line_log"], fx["step"], bytes.fromhex(fx["digest"])
    data = _data("uniform", line_log, "every", 1) if name == "R1" else _constant(line_log, CONSTANT)
    hctx.set_pcs_config(hooks_pkg.PcsConfig(log_blowup_factor=log_blowup))
    want = model.commit(orc.lib, data, log_blowup, digest)
    last = len(want["draws"]) - 1
    assert want["draws"] == [2 if k == step else 1 for k in range(last + 1)] and want["alphas"][step].tolist() == fx["alpha"] and fx["n_sent"] == 2
    words = model.draw_words(want["digest"] if step == last else _digest_after(digest, want["roots"][:step + 1]), 0)
    assert any(w >= 2 * P for w in words), "the fixture's first draw at this step is not rejected"
    if log_blowup == 1:
        assert want["digest"].hex() == fx["final_digest"] and want["n_sent"] == fx["final_n_sent"] == 1
    else:
        assert step == last and want["n_sent"] == 2
    got = run_hook(hooks_pkg, hctx, data, digest)
    who = {"R1": BY_LAUNCHES, "R2": BY_LAYER_KERNEL, "R3": BY_TAIL, "R4": BY_TAIL}[name]
    assert step == 0 or got["paths"][step - 1] >> 4 == who, got["paths"]          # the kernel that hashed the tree of that step steps the channel
    assert got["alphas"][step].tolist() == fx["alpha"], (name, "alpha || alpha^2 of the redrawing step")
    compare(got, want, (name, log_blowup))


def _digest_after(digest, roots):
    for r in roots:
        digest = model.mix_root(digest, r)
    return digest
