"""-m gpu: every k_merkle_layer instantiation (hashing convention x node shape, merkle.hip MerkleShape) through the C ABI
(Context.merkle_commit_layer) against the CPU oracle, node by node.

Shapes: leaves over 1, 2, 3, 4 columns (one instantiation each), 5, 16, 17 and 33 columns (1, 1, 2 and 3 blocks of the wide-leaf instantiation, the
zero-padding boundaries at 16 / 17), each with and without a replicated column (col_shifts); inner nodes with 0 columns (their own instantiation) and 1, 4, 20
columns (2, 2, 3 blocks), over a plain child layer and over a replicated one. Layer sizes: 2^6 (one partial workgroup), 2^12, and 2^22 stored nodes
(the grid in which a lane hashes several nodes).

The C ABI stores and reads every layer in full (out_shift = prev_shift = 0), so a "replicated child layer" here is the full expansion of one: every
child hash repeated 2^s times, which is exactly what a layer under replicated columns holds. The shifted storage itself belongs to the prover and is
covered by the whole-proof digests of tests/test_gpu_prove.py under both conventions."""
import ctypes

import numpy as np
import pytest

from conftest import splitmix_column

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 1], ids=["stwo", "rfc7693"])
def node_conv(request, _ctx, _oracle, pkg):
    """Both Merkle node-hash conventions, set on the context and on the oracle (process-wide switch); the other switches stay at their defaults."""
    _oracle.set_conventions(request.param, 0, 0, 0)
    _ctx.set_conventions(request.param, 0, 0, 0)
    yield request.param
    _oracle.set_conventions(0, 0, 0, 0)
    _ctx.set_conventions(0, 0, 0, 0)


def _columns(seed, ncols, log, replicated):
    """ncols columns of 2^log cells; with `replicated` the LAST column is row-granular (2^(log-4) cells, shift 4). Returns (arrays, shifts, full views)."""
    cols, shifts, full = [], [], []
    for k in range(ncols):
        sh = 4 if replicated and k == ncols - 1 else 0
        c = splitmix_column(seed + 13 * k, (1 << log) >> sh)
        cols.append(c); shifts.append(sh); full.append(np.repeat(c, 1 << sh))
    return cols, shifts, full


def _hashes(seed, n, repeat_log=0):
    """n pseudo-random 32-byte hashes as [n][8] u32; with repeat_log every hash is repeated 2^repeat_log times (a replicated layer stored in full)."""
    m = n >> repeat_log
    x = (np.arange(8 * m, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29); x *= np.uint64(0xBF58476D1CE4E5B9); x ^= x >> np.uint64(32)
    return np.repeat((x & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(m, 8), 1 << repeat_log, axis=0)


def _run(ctx, log, prev, cols, shifts):
    dprev = ctx.upload(prev) if prev is not None else 0
    dcols = [ctx.upload(c) for c in cols]
    out = ctx.malloc(32 << log)
    ctx.merkle_commit_layer(log, dprev, dcols, out, col_shifts=shifts if any(shifts) else None)
    got = ctx.download(out, 8 << log).view(np.uint8).reshape(-1, 32)
    for p in dcols + [out] + ([dprev] if dprev else []):
        ctx.free(p)
    return got


def _check_nodes(oracle, got, prev, full, nodes):
    pb = prev.view(np.uint8).reshape(-1, 32) if prev is not None else None
    for i in nodes:
        i = int(i)
        l, r = (bytes(pb[2 * i]), bytes(pb[2 * i + 1])) if pb is not None else (None, None)
        assert bytes(got[i]) == oracle.hash_node(l, r, [c[i] for c in full]), f"node {i}"


@pytest.mark.parametrize("log", [6, 12])
@pytest.mark.parametrize("replicated", [False, True], ids=["plain", "replicated_col"])
@pytest.mark.parametrize("ncols", [1, 2, 3, 4, 5, 16, 17, 33])
def test_leaf_shapes_match_oracle(_ctx, _oracle, node_conv, ncols, replicated, log):
    cols, shifts, full = _columns(1000 + ncols, ncols, log, replicated)
    got = _run(_ctx, log, None, cols, shifts)
    _check_nodes(_oracle, got, None, full, range(1 << log))


@pytest.mark.parametrize("log", [6, 12])
@pytest.mark.parametrize("child_repeat", [0, 3], ids=["plain_children", "replicated_children"])
@pytest.mark.parametrize("ncols", [0, 1, 4, 20])
def test_inner_shapes_match_oracle(_ctx, _oracle, node_conv, ncols, child_repeat, log):
    prev = _hashes(77 + ncols, 2 << log, child_repeat)
    # over a replicated child layer the columns of a real tree are replicated too (else the layer would not be): take the last one row-granular
    cols, shifts, full = _columns(2000 + ncols, ncols, log, replicated=bool(child_repeat))
    got = _run(_ctx, log, prev, cols, shifts)
    _check_nodes(_oracle, got, prev, full, range(1 << log))


def test_tree_of_2p22_leaves_matches_oracle_commit(_ctx, _oracle, node_conv):
    """2^22 stored nodes (several nodes per lane): a 4-column leaf layer, then an inner layer with one column, then a column-less inner layer, each
    compared in full with the layers of the oracle's MerkleProver::commit."""
    logs = [22, 22, 22, 22, 21]
    cols = [splitmix_column(400 + i, 1 << l) for i, l in enumerate(logs)]
    ptrs_h = (ctypes.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
    want = np.zeros(sum(32 << l for l in range(23)), dtype=np.uint8); root = (ctypes.c_ubyte * 32)()
    assert _oracle.L.orc_merkle_commit(ptrs_h, (ctypes.c_uint32 * len(logs))(*logs), ctypes.c_size_t(len(logs)), root, want.ctypes.data_as(ctypes.c_void_p)) == 0
    dev = [_ctx.upload(c) for c in cols]
    prev, off, outs = 0, 0, []
    for log in (22, 21, 20):
        out = _ctx.malloc(32 << log); outs.append(out)
        _ctx.merkle_commit_layer(log, prev, [d for d, l in zip(dev, logs) if l == log], out)
        got = _ctx.download(out, 8 << log).view(np.uint8)
        assert np.array_equal(got, want[off: off + (32 << log)]), f"layer {log}"
        off += 32 << log
        prev = out
    for p in dev + outs:
        _ctx.free(p)


def test_inner_layer_of_2p22_nodes_matches_oracle_on_sampled_nodes(_ctx, _oracle, node_conv):
    """The column-less inner instantiation in the several-nodes-per-lane grid. 2^22 nodes are too many for one oracle call each: the first and last
    workgroups, the nodes around every grid-stride boundary (a lane's 2nd, 3rd and 4th node start at multiples of 2^20) and 2048 pseudo-random nodes."""
    log = 22
    prev = _hashes(9, 2 << log)
    got = _run(_ctx, log, prev, [], [])
    edges = [k * (1 << 20) + d for k in range(1, 4) for d in range(-64, 64)]
    nodes = np.unique(np.concatenate([np.arange(256), np.arange((1 << log) - 256, 1 << log), np.array(edges), splitmix_column(5, 2048).astype(np.int64) % (1 << log)]))
    _check_nodes(_oracle, got, prev, [], nodes)
    assert len({bytes(h) for h in got[nodes]}) == len(nodes)          # distinct inputs, distinct hashes: no slot was left unwritten or written twice
