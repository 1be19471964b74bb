"""-m gpu: bfhip_witness_program_generate (include/bfhip.h "Witness programs", csrc/witness_program.hip). In every case generate followed by
rows_from_columns must equal bfhip_witness_program_eval_table bit for bit: domains below one wave, of exactly one, of two, on the tiled path
of the ingest and of many workgroups; the program at every cap; a bit decomposition; the Processor table from device-ingested registers
against the uploaded host table; columns derived on the device accepted by bfhip_air_check (an is-zero gadget, a "next" column) and a
corrupted one named by it; the call inside an open session without touching the arena; every refusal word for word, writing nothing."""
import ctypes
import os

import numpy as np
import pytest

import witness_model as model
from conftest import P, ROOT
from witness_model import ARG, M_ADD, M_COL, ROW, STORE

pytestmark = pytest.mark.gpu

STWO = (0, 0, 0, 0)
FILL = 0xA5A5A5A5
COLLATZ = open(os.path.join(ROOT, "tests", "golden", "programs", "collatz.bf")).read()
EDGES = np.array([0, 0, 1, P - 1, P - 2, 255], dtype=np.uint32)


def _table(seed, log_size, n_cols):
    """(2^log_size, n_cols) canonical words, a third of them field edges and zeros"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, P, size=(1 << log_size, n_cols), dtype=np.uint32)
    pick = rng.integers(0, 3 * len(EDGES), size=t.shape)
    return np.where(pick < len(EDGES), EDGES[pick % len(EDGES)], t).astype(np.uint32)


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _generate(ctx, prog, log_size, table, args=()):
    """The program over the ingested table, read back in row order."""
    with ctx.columns_from_rows(table, log_size) as cols, ctx.witness_program_generate(prog, log_size, cols, args) as out:
        return ctx.rows_from_columns(out, log_size)


@pytest.fixture(scope="module")
def random_case(pkg):
    """One random program with every opcode and offsets up to +-16, shared by the sizes."""
    rng = model.random.Random(2)
    code = model.random_program(rng, 4, 3, 2, 60, offsets=(0, 0, 1, -1, 2, -2, 16, -16))
    assert set(range(6)) | set(range(ARG, STORE + 1)) == set(code[0::4])
    assert {code[i + 3] for i in range(0, len(code), 4) if code[i] == M_COL} == {o & 0xFFFFFFFF for o in (0, 1, -1, 2, -2, 16, -16)}
    return pkg.WitnessProgram(code, 4, 3, 2), [P - 1, 12345]


@pytest.mark.parametrize("log_size", [1, 5, 6, 7, 10, 16])
def test_generate_equals_eval_table_at_every_size(_ctx, pkg, random_case, log_size):
    prog, args = random_case
    table = _table(log_size, log_size, 4)
    want = prog.eval_table(table, args)
    if log_size <= 6:      # the plain-Python model behind eval_table, where it is quick
        assert want.tolist() == model.eval_table(prog.code, table.tolist(), args, 3)
    _same(_generate(_ctx, prog, log_size, table, args), want)


def test_program_at_every_cap(_ctx, pkg):
    """96 registers, 256 input columns, 256 outputs, offsets from -16 to 16, at one wave."""
    log_size = 6
    code = [ROW, 95, 0, 0]
    for k in range(256):
        r = k % 95
        code += [M_COL, r, k, (k % 33 - 16) & 0xFFFFFFFF, M_ADD, r, r, 95, STORE, 255 - k, r, 0]
    prog = pkg.WitnessProgram(code, 256, 256, 0)
    assert prog.shape()["m_regs"] == 96 and (prog.shape()["min_offset"], prog.shape()["max_offset"]) == (-16, 16)
    table = _table(9, log_size, 256)
    n = 1 << log_size
    want = prog.eval_table(table)
    rows = np.arange(n)
    for k in (0, 16, 255):
        assert want[:, 255 - k].tolist() == ((table[(rows + (k % 33 - 16)) % n, k].astype(np.uint64) + rows) % P).tolist()
    _same(_generate(_ctx, prog, log_size, table), want)


def test_bit_decomposition(_ctx, pkg):
    """8 outputs of AND / SHR whose weighted sum is the input byte."""
    log_size = 8
    b = pkg.AirBuilder()
    x = b.col(0)
    for i in range(8):
        b.store(i, b.bit_and(b.shr(x, i), 1))
    prog = b.witness_program(8)
    table = np.random.default_rng(4).permutation(256).astype(np.uint32).reshape(256, 1)
    got = _generate(_ctx, prog, log_size, table)
    _same(got, prog.eval_table(table))
    assert set(got.ravel().tolist()) == {0, 1} and ((got.astype(np.uint64) << np.arange(8, dtype=np.uint64)).sum(axis=1) == table[:, 0]).all()


def _host_processor_table(pkg, regs7, code_words):
    L = pkg.lib()
    words = np.ascontiguousarray(code_words, dtype=np.uint32)
    nr, nc = ctypes.c_size_t(), ctypes.c_size_t()
    args = (regs7.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(regs7.shape[0]), words.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(words.size), 3)
    assert L.bfhip_host_table(*args, None, ctypes.c_size_t(0), ctypes.byref(nr), ctypes.byref(nc)) == 0
    t = np.zeros((nr.value, nc.value), dtype=np.uint32)
    assert L.bfhip_host_table(*args, t.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(t.size), ctypes.byref(nr), ctypes.byref(nc)) == 0
    return t


def test_processor_table_from_device_ingested_registers(_ctx, pkg):
    """The six register columns ingested with repeat_last, the Processor program over them: the storage-order columns of the uploaded
    bfhip_host_table, byte for byte."""
    regs = np.ascontiguousarray(pkg.host_run(COLLATZ, bytes([55, 10]))[1], dtype=np.uint32)
    want = _host_processor_table(pkg, regs, pkg.host_compile(COLLATZ))
    log_size = want.shape[0].bit_length() - 1
    assert want.shape == (1 << log_size, 9) and regs.shape[0] < want.shape[0] and want[:, 7].any()
    prog = pkg.brainfuck_witness_program("processor")[0]
    with _ctx.columns_from_rows(np.ascontiguousarray(regs[:, :6]), log_size, repeat_last=True) as inputs, \
            _ctx.witness_program_generate(prog, log_size, inputs, [regs.shape[0]]) as out, _ctx.columns_from_rows(want, log_size) as uploaded:
        _same(out.download(), uploaded.download())
        _same(_ctx.rows_from_columns(out, log_size), want)


def test_is_zero_gadget_end_to_end(_ctx, pkg):
    """Columns a, a_inv, z with a z = 0 and a a_inv = 1 - z; a_inv and z are derived on the device and bfhip_air_check accepts them; one
    overwritten word of a_inv is named."""
    log_size = 9
    n = 1 << log_size
    a = _table(21, log_size, 1)
    assert (a == 0).any() and (a != 0).any()
    w = pkg.AirBuilder()
    w.store(0, w.inv0(w.col(0)))
    w.store(1, w.is_zero(w.col(0)))
    witness = w.witness_program(2)
    c = pkg.AirBuilder()
    ca, ca_inv, cz = c.col(0), c.col(1), c.col(2)
    c.constraint(ca * cz)
    c.constraint(ca * ca_inv - (1 - cz))
    air = c.program()
    with _ctx.columns_from_rows(a, log_size) as cols, _ctx.witness_program_generate(witness, log_size, cols) as derived:
        rep = _ctx.air_check(air, log_size, [cols[0], derived[0], derived[1]], [])
        assert rep.as_dict()["n_bad_cells"] == 0 and pkg.format_air_check(rep) == "air check: ok"
        row = int(np.flatnonzero(a[:, 0])[3])      # a row with a != 0: a a_inv = 1 pins a_inv
        cell = pkg.cell_of_row(log_size, row)
        broken = _ctx.download(derived[0], n).copy()
        broken[cell] = (int(broken[cell]) + 1) % P
        ptr = _ctx.upload(broken)
        try:
            rep = _ctx.air_check(air, log_size, [cols[0], ptr, derived[1]], []).as_dict()
        finally:
            _ctx.free(ptr)
        assert rep["n_bad_cells"] == 1 and rep["first_bad_cell"] == cell and rep["first_bad_constraint"] == 1, rep


@pytest.mark.parametrize("log_size", [4, 11])
def test_next_column_satisfies_an_air_that_reads_it_at_offset_zero(_ctx, pkg, log_size):
    a = _table(33 + log_size, log_size, 1)
    w = pkg.AirBuilder()
    w.store(0, w.col(0, 1))
    witness = w.witness_program(1)
    c = pkg.AirBuilder()
    c.constraint(c.col(1) - c.col(0, 1))
    air = c.program()
    with _ctx.columns_from_rows(a, log_size) as cols, _ctx.witness_program_generate(witness, log_size, cols) as nxt:
        assert _ctx.air_check(air, log_size, [cols[0], nxt[0]], []).as_dict()["n_bad_cells"] == 0
        _same(_ctx.rows_from_columns(nxt, log_size)[:, 0], np.roll(a[:, 0], -1))


def test_inside_an_open_session_without_touching_the_arena(_ctx, pkg, random_case):
    ctx, log_size = _ctx, 11
    prog, args = random_case
    ctx.set_conventions(*STWO)
    ctx.set_pcs_config(None)
    table = _table(44, log_size, 4)
    want = prog.eval_table(table, args)
    with ctx.columns_from_rows(table, log_size) as cols:
        with pkg.Channel(STWO) as ch, pkg.PcsSession(ctx) as s:
            before = ctx.memory()["arena_in_use"]
            with ctx.witness_program_generate(prog, log_size, cols, args) as out:
                assert ctx.memory()["arena_in_use"] == before
                _same(ctx.rows_from_columns(out, log_size), want)
                assert ctx.memory()["arena_in_use"] == before
                assert len(s.commit(ch, cols.ptrs + out.ptrs, [log_size] * 7, form=0)) == 32
        outside = ctx.memory()["arena_in_use"]
        with ctx.witness_program_generate(prog, log_size, cols, args) as out:
            assert ctx.memory()["arena_in_use"] == outside


def _raw(pkg, ctx, prog, log_size, cols, args, n_args, outs, n_out):
    """(return code, bfhip_last_error()) of the C call itself"""
    ptrs = lambda ps: None if ps is None else (ctypes.c_void_p * max(1, len(ps)))(*ps)
    words = None if args is None else (ctypes.c_uint32 * max(1, len(args)))(*args)
    rc = pkg.lib().bfhip_witness_program_generate(ctx._h if ctx is not None else None, prog._h if prog is not None else None, ctypes.c_uint32(log_size), ptrs(cols), words,
                                                  ctypes.c_uint32(n_args), ptrs(outs), ctypes.c_uint32(n_out))
    return rc, pkg.lib().bfhip_last_error().decode()


def test_every_refusal_word_for_word_writes_nothing(_ctx, pkg, random_case):
    ctx, log_size = _ctx, 7
    n = 1 << log_size
    prog, args = random_case
    table = _table(5, log_size, 4)
    want = prog.eval_table(table, args)
    who = "bfhip_witness_program_generate: "
    with ctx.columns_from_rows(table, log_size) as cols:
        ins, inputs_before = cols.ptrs, cols.download()
        sentinel = np.full(n + 1, FILL, dtype=np.uint32)
        outs = [ctx.upload(sentinel) for _ in range(3)]
        try:
            cases = [
                ((ctx, None, log_size, ins, args, 2, outs, 3), who + "null argument"),
                ((ctx, prog, log_size, None, args, 2, outs, 3), who + "null argument"),
                ((ctx, prog, log_size, ins, None, 2, outs, 3), who + "null argument"),
                ((ctx, prog, log_size, ins, args, 2, None, 3), who + "null argument"),
                ((None, prog, log_size, ins, args, 2, outs, 3), "null context"),
                ((ctx, prog, 0, ins, args, 2, outs, 3), who + "log_size must be in [1, max_log_domain = 24], got 0"),
                ((ctx, prog, 25, ins, args, 2, outs, 3), who + "log_size must be in [1, max_log_domain = 24], got 25"),
                ((ctx, prog, log_size, ins, args, 2, outs[:2], 2), who + "2 output columns, the program has 3"),
                ((ctx, prog, log_size, ins, args + [0], 3, outs, 3), who + "3 args, the program has 2"),
                ((ctx, prog, log_size, ins, args[:1], 1, outs, 3), who + "1 args, the program has 2"),
                ((ctx, prog, log_size, ins, [0, P], 2, outs, 3), who + "arg 1: 2147483647 is not a canonical M31 value"),
                ((ctx, prog, log_size, ins[:2] + [0] + ins[3:], args, 2, outs, 3), who + "input column 2 is a null pointer"),
                ((ctx, prog, log_size, ins, args, 2, [outs[0], 0, outs[2]], 3), who + "output column 1 is a null pointer"),
                ((ctx, prog, log_size, ins, args, 2, [outs[0], ins[3], outs[2]], 3), who + "output column 1 overlaps input column 3"),
                ((ctx, prog, log_size, ins, args, 2, [outs[0], outs[1], ins[0] + 4 * (n - 1)], 3), who + "output column 2 overlaps input column 0"),
                ((ctx, prog, log_size, ins, args, 2, [outs[0], outs[1], outs[0] + 4], 3), who + "output column 2 overlaps output column 0"),
            ]
            for call, message in cases:
                assert _raw(pkg, *call) == (-1, message)
            # a context in a shard group
            group, member = pkg.LocalGroup(2), pkg.Context(0, max_log_domain=10)
            try:
                member.join_local_group(group, 0)
                assert _raw(pkg, member, prog, log_size, ins, args, 2, outs, 3) == (-1, who + "a context in a shard group is not supported (bfhip_ctx_leave_group first)")
                member.leave_group()
            finally:
                member.close(); group.close()
            for p in outs:
                _same(ctx.download(p, n + 1), sentinel)
            _same(cols.download(), inputs_before)
            # the context still runs the good case, to the same bytes, and writes 2^log_size words of each output and no more
            assert _raw(pkg, ctx, prog, log_size, ins, args, 2, outs, 3)[0] == 0
            _same(ctx.rows_from_columns(outs, log_size), want)
            assert all(int(ctx.download(p, n + 1)[n]) == FILL for p in outs)
        finally:
            for p in outs:
                ctx.free(p)
