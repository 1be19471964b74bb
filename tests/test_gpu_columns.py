"""-m gpu: bfhip_columns_from_rows / bfhip_rows_from_columns (include/bfhip.h "Row order", csrc/rows.hip) against the numpy model of
tests/columns_model.py, byte for byte: every log_size from 1 to 16 in both layouts, column counts around the 8 and 16 columns of an LDS pass, row
counts and both paddings, strides, misaligned bases and column maps, non-canonical words, every refusal, the round trip, tables of many
workgroups, and what the order MEANS — an offset-reading AIR accepts an ingested row-order trace, air_prove gives the bytes it gives on the
numpy helper's columns, and the call works inside an open session without touching the arena."""
import ctypes

import numpy as np
import pytest

import columns_model as model
from conftest import P
from test_gpu_air_prove import STWO, _is_first, _lookup_statement, _lookup_trace, _storage_of_coset_order

pytestmark = pytest.mark.gpu

PASS_COLS = (8, 16)  # csrc/rows.hip: columns per LDS pass, up to 8 output columns and beyond; the tiled kernels start at log_size 10 (csrc/rows_index.h)
FILL = 0xA5A5A5A5


class Dev:
    """device buffers freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, arr):
        self.ptrs.append(self.ctx.upload(np.ascontiguousarray(arr, dtype=np.uint32)))
        return self.ptrs[-1]

    def filled(self, n_words, value=FILL):
        return self.up(np.full(n_words, value, dtype=np.uint32))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.free(p)


def _table(seed, n_rows, n_cols):
    return np.random.default_rng(seed).integers(0, P, size=(n_rows, n_cols), dtype=np.uint32)


def _device_table(pkg, dev, table, layout, row_stride=None, offset_words=0):
    """The table on the device: row-major (optionally with a larger stride and a base offset_words into its allocation) or column-major."""
    n_rows, n_cols = table.shape
    if layout == "columns":
        return pkg.DeviceRowColumns([dev.up(np.concatenate([np.full(offset_words, FILL, dtype=np.uint32), table[:, c]])) + 4 * offset_words for c in range(n_cols)], n_rows)
    stride = n_cols if row_stride is None else row_stride
    wide = np.full((n_rows, stride), FILL, dtype=np.uint32)
    wide[:, :n_cols] = table
    base = dev.up(np.concatenate([np.full(offset_words, FILL, dtype=np.uint32), wide.ravel(), np.zeros(1, dtype=np.uint32)]))
    return pkg.DeviceRows(base + 4 * offset_words, n_rows, n_cols, stride)


def _run(pkg, ctx, table, log_size, layout="rows", columns=None, pad=None, repeat_last=False, row_stride=None, offset_words=0):
    with Dev(ctx) as dev:
        src = _device_table(pkg, dev, table, layout, row_stride, offset_words)
        with ctx.columns_from_rows(src, log_size, columns=columns, pad=pad, repeat_last=repeat_last) as cols:
            return cols.download()


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("layout", ["rows", "columns"])
@pytest.mark.parametrize("log_size", range(1, 17))
def test_every_log_size_both_layouts(_ctx, pkg, log_size, layout):
    for n_out in (1, 3):
        table = _table(100 * log_size + n_out, 1 << log_size, n_out)
        _same(_run(pkg, _ctx, table, log_size, layout), model.columns_from_rows(table, log_size))


@pytest.mark.parametrize("layout", ["rows", "columns"])
@pytest.mark.parametrize("log_size", [10, 14])
def test_column_counts_around_the_lds_pass(_ctx, pkg, log_size, layout):
    counts = sorted({1, 2, 7, 8, 9, 16, 17, 31, 32, 33, 65} | {c + d for c in PASS_COLS for d in (-1, 0, 1)})
    table = _table(7 + log_size, 1 << log_size, max(counts))
    want = model.columns_from_rows(table, log_size)
    with Dev(_ctx) as dev:
        src = _device_table(pkg, dev, table, layout)
        for n_out in counts:
            with _ctx.columns_from_rows(src, log_size, columns=list(range(n_out))) as cols:
                _same(cols.download(), want[:n_out])


@pytest.mark.parametrize("layout", ["rows", "columns"])
@pytest.mark.parametrize("log_size", [1, 5, 12])
def test_row_counts_and_both_paddings(_ctx, pkg, log_size, layout):
    n = 1 << log_size
    pad = [0, P - 1, 12345]
    for n_rows in sorted({0, 1, 2, n // 2 - 1, n // 2, n // 2 + 1, n - 1} & set(range(n + 1))):
        table = _table(31 * log_size + n_rows, n_rows, 3)
        _same(_run(pkg, _ctx, table, log_size, layout, pad=pad), model.columns_from_rows(table, log_size, pad=pad))
        _same(_run(pkg, _ctx, table, log_size, layout), model.columns_from_rows(table, log_size))
        if n_rows:
            _same(_run(pkg, _ctx, table, log_size, layout, repeat_last=True), model.columns_from_rows(table, log_size, repeat_last=True))
        else:
            with pytest.raises(pkg.BfhipError) as e:
                _run(pkg, _ctx, table, log_size, layout, repeat_last=True)
            assert str(e.value) == "bfhip_columns_from_rows: BFHIP_ROWS_REPEAT_LAST needs at least one row"


@pytest.mark.parametrize("log_size", [6, 11])
def test_strides_misaligned_bases_and_column_maps(_ctx, pkg, log_size):
    n_rows = (1 << log_size) - 3
    table = _table(900 + log_size, n_rows, 7)
    for stride in (7, 8, 9):
        for offset in (0, 1):      # one word into the allocation: nothing is 16-byte aligned
            _same(_run(pkg, _ctx, table, log_size, row_stride=stride, offset_words=offset), model.columns_from_rows(table, log_size))
    _same(_run(pkg, _ctx, table, log_size, "columns", offset_words=1), model.columns_from_rows(table, log_size))
    maps = {"permutation": [3, 0, 6, 5, 1, 2, 4], "subset": [5, 2], "repeats": [1, 1, 4, 1, 0, 0, 0, 0, 6, 1]}
    for layout in ("rows", "columns"):
        for columns in maps.values():
            pad = [(11 * k) % P for k in range(len(columns))]
            _same(_run(pkg, _ctx, table, log_size, layout, columns=columns, pad=pad, row_stride=9 if layout == "rows" else None, offset_words=1),
                  model.columns_from_rows(table, log_size, columns=columns, pad=pad))


@pytest.mark.parametrize("layout", ["rows", "columns"])
@pytest.mark.parametrize("log_size", [4, 12])
def test_bad_words_name_the_lowest_row_then_the_lowest_column(_ctx, pkg, log_size, layout):
    n = 1 << log_size
    all_max = np.full((n, 9), P - 1, dtype=np.uint32)
    _same(_run(pkg, _ctx, all_max, log_size, layout), model.columns_from_rows(all_max, log_size))
    good = _table(5, n, 9)
    cases = [((n - 1, 0, P), (n // 2 + 1, 8, 0xFFFFFFFF), (n // 2 + 1, 8, 0xFFFFFFFF)),      # lowest row wins over lowest column
             ((7, 6, 0xFFFFFFFF), (7, 2, P), (7, 2, P)),                                     # same row: lowest column
             ((0, 0, P), (n - 1, 8, 0xFFFFFFFF), (0, 0, P))]
    for a, b, (row, col, value) in cases:
        bad = good.copy()
        bad[a[0], a[1]], bad[b[0], b[1]] = a[2], b[2]
        with pytest.raises(pkg.BfhipError) as e:
            _run(pkg, _ctx, bad, log_size, layout)
        assert str(e.value) == "bfhip_columns_from_rows: row %d, column %d: %d is not a canonical M31 value" % (row, col, value)
        # the context stays usable: a correct call right behind it
        _same(_run(pkg, _ctx, good, log_size, layout), model.columns_from_rows(good, log_size))
    # the column named is the OUTPUT column: source column 6 is output column 1 under this map; a bad word in an unmapped column is not read
    bad = good.copy()
    bad[3, 6], bad[2, 0] = P, P
    with pytest.raises(pkg.BfhipError) as e:
        _run(pkg, _ctx, bad, log_size, layout, columns=[4, 6])
    assert str(e.value) == "bfhip_columns_from_rows: row 3, column 1: %d is not a canonical M31 value" % P


def _raw(pkg, ctx, table, log_size, src_cols, pad, outs, n_out):
    rc = pkg.lib().bfhip_columns_from_rows(ctx._h, ctypes.byref(table) if table is not None else None, ctypes.c_uint32(log_size),
                                           None if src_cols is None else (ctypes.c_uint32 * len(src_cols))(*src_cols),
                                           None if pad is None else (ctypes.c_uint32 * len(pad))(*pad),
                                           None if outs is None else (ctypes.c_void_p * len(outs))(*outs), ctypes.c_uint32(n_out))
    return rc, pkg.lib().bfhip_last_error().decode() if rc else ""


def test_refusals_name_their_rule_and_write_nothing(_ctx, pkg):
    ctx, log_size = _ctx, 10
    n = 1 << log_size
    T = pkg.RowsTable
    u32p = lambda p: ctypes.cast(ctypes.c_void_p(p), ctypes.POINTER(ctypes.c_uint32))
    with Dev(ctx) as dev:
        table = _table(1, n, 4)
        rows = dev.up(table)
        src_cols = [dev.up(table[:, c]) for c in range(4)]
        cols_h = (ctypes.c_void_p * 4)(*src_cols)
        cols_pp = ctypes.cast(cols_h, ctypes.POINTER(ctypes.c_void_p))
        big = dev.filled(3 * n)
        outs = [big, big + 4 * n, big + 8 * n]
        rm = lambda **kw: T(**{**dict(layout=0, n_cols=4, rows_d=u32p(rows), cols_h=None, n_rows=n, row_stride=4, flags=0, reserved=0), **kw})
        cm = lambda **kw: T(**{**dict(layout=1, n_cols=4, rows_d=None, cols_h=cols_pp, n_rows=n, row_stride=0, flags=0, reserved=0), **kw})
        who = "bfhip_columns_from_rows: "
        cases = [
            ((None, log_size, None, None, outs, 3), who + "null argument"),
            ((rm(), log_size, None, None, None, 3), who + "null argument"),
            ((rm(rows_d=None), log_size, None, None, outs, 3), who + "null table pointer"),
            ((cm(cols_h=None), log_size, None, None, outs, 3), who + "null table pointer"),
            ((rm(), log_size, None, None, [outs[0], None, outs[2]], 3), who + "output column 1 is a null pointer"),
            ((rm(), 0, None, None, outs, 3), who + "log_size 0 is outside 1..30"),
            ((rm(), 31, None, None, outs, 3), who + "log_size 31 is outside 1..30"),
            ((rm(n_rows=n + 1), log_size, None, None, outs, 3), who + "n_rows %d exceeds 2^%d" % (n + 1, log_size)),
            ((rm(row_stride=3), log_size, None, None, outs, 3), who + "row_stride 3 is below n_cols 4"),
            ((rm(), log_size, [0, 4, 1], None, outs, 3), who + "column index 4 is not below n_cols 4"),
            ((cm(), log_size, [0, 1, 7], None, outs, 3), who + "column index 7 is not below n_cols 4"),
            ((rm(n_cols=2), log_size, None, None, outs, 3), who + "column index 2 is not below n_cols 2"),
            ((rm(), log_size, None, None, outs, 0), who + "n_out 0 is outside 1..256 (BFHIP_AIR_MAX_COLUMNS)"),
            ((rm(), log_size, None, None, outs, 257), who + "n_out 257 is outside 1..256 (BFHIP_AIR_MAX_COLUMNS)"),
            ((rm(layout=2), log_size, None, None, outs, 3), who + "unknown layout 2"),
            ((rm(flags=2), log_size, None, None, outs, 3), who + "unknown flag bits 2"),
            ((rm(flags=3), log_size, None, None, outs, 3), who + "unknown flag bits 3"),
            ((rm(reserved=1), log_size, None, None, outs, 3), who + "reserved must be 0"),
            ((rm(), log_size, None, [0, P, 0], outs, 3), who + "pad value %d of output column 1 is not a canonical M31 value" % P),
            ((rm(n_rows=0, flags=1), log_size, None, None, outs, 3), who + "BFHIP_ROWS_REPEAT_LAST needs at least one row"),
            ((rm(), log_size, None, None, [outs[0], outs[1], outs[0] + 4 * (n - 1)], 3), who + "output column 2 overlaps output column 0"),
            ((rm(), log_size, None, None, [outs[0], rows + 16 * n - 4, outs[2]], 3), who + "output column 1 overlaps the source table"),
            ((cm(), log_size, None, None, [outs[0], outs[1], src_cols[0] + 4 * (n - 1)], 3), who + "output column 2 overlaps source column 0"),
        ]
        for args, message in cases:
            assert _raw(pkg, ctx, *args) == (-1, message)
        # a context in a shard group
        group, member = pkg.LocalGroup(2), pkg.Context(0, max_log_domain=10)
        try:
            member.join_local_group(group, 0)
            assert _raw(pkg, member, rm(), log_size, None, None, outs, 3) == (-1, who + "a context in a shard group is not supported (bfhip_ctx_leave_group first)")
            rc = pkg.lib().bfhip_rows_from_columns(member._h, (ctypes.c_void_p * 3)(*outs), ctypes.c_uint32(3), ctypes.c_uint32(log_size), ctypes.c_void_p(rows),
                                                   ctypes.c_uint64(n), ctypes.c_uint64(4), ctypes.c_uint32(0))
            assert rc == -1 and pkg.lib().bfhip_last_error().decode() == "bfhip_rows_from_columns: a context in a shard group is not supported (bfhip_ctx_leave_group first)"
            member.leave_group()
        finally:
            member.close(); group.close()
        # the inverse, in its own name
        inv = lambda cols, n_cols, log, dst, n_rows, stride, reserved=0: (
            pkg.lib().bfhip_rows_from_columns(ctx._h, None if cols is None else (ctypes.c_void_p * len(cols))(*cols), ctypes.c_uint32(n_cols), ctypes.c_uint32(log),
                                              ctypes.c_void_p(dst), ctypes.c_uint64(n_rows), ctypes.c_uint64(stride), ctypes.c_uint32(reserved)),
            pkg.lib().bfhip_last_error().decode())
        who = "bfhip_rows_from_columns: "
        scratch = dev.filled(4 * n)
        assert inv(None, 3, log_size, scratch, n, 4) == (-1, who + "null argument")
        assert inv(outs, 3, log_size, None, n, 4) == (-1, who + "null argument")
        assert inv([outs[0], None, outs[2]], 3, log_size, scratch, n, 4) == (-1, who + "column 1 is a null pointer")
        assert inv(outs, 3, log_size, scratch, n, 4, 9) == (-1, who + "reserved must be 0")
        assert inv(outs, 3, 31, scratch, n, 4) == (-1, who + "log_size 31 is outside 1..30")
        assert inv(outs, 3, log_size, scratch, n + 1, 4) == (-1, who + "n_rows %d exceeds 2^%d" % (n + 1, log_size))
        assert inv(outs, 3, log_size, scratch, n, 2) == (-1, who + "row_stride 2 is below n_cols 3")
        assert inv(outs, 0, log_size, scratch, n, 4) == (-1, who + "n_cols 0 is outside 1..256 (BFHIP_AIR_MAX_COLUMNS)")
        assert inv(outs, 3, log_size, outs[1] + 4 * (n - 1), n, 4) == (-1, who + "column 1 overlaps the table")
        # nothing was written, and the context computes
        assert (ctx.download(big, 3 * n) == FILL).all() and (ctx.download(scratch, 4 * n) == FILL).all()
        with ctx.columns_from_rows(pkg.DeviceRows(rows, n, 4), log_size, out=outs, columns=[3, 1, 0]) as cols:
            _same(cols.download(), model.columns_from_rows(table, log_size, columns=[3, 1, 0]))
        with pytest.raises(TypeError):
            ctx.columns_from_rows(table.astype(np.int64), log_size)


@pytest.mark.parametrize("log_size", [1, 7, 13])
def test_round_trip_leaves_the_rest_of_each_row_alone(_ctx, pkg, log_size):
    n, n_cols, stride = 1 << log_size, 5, 8
    for n_rows in sorted({1, n // 2 + 1, n} & set(range(1, n + 1))):
        x = _table(77 + log_size + n_rows, n_rows, n_cols)
        with _ctx.columns_from_rows(x, log_size, pad=[9] * n_cols) as cols, Dev(_ctx) as dev:
            _same(_ctx.rows_from_columns(cols, log_size, n_rows), x)
            _same(_ctx.rows_from_columns(cols.ptrs, log_size), model.rows_from_columns(model.columns_from_rows(x, log_size, pad=[9] * n_cols), log_size, n))
            dst = dev.filled(n * stride + 1)
            rc = pkg.lib().bfhip_rows_from_columns(_ctx._h, (ctypes.c_void_p * n_cols)(*cols.ptrs), ctypes.c_uint32(n_cols), ctypes.c_uint32(log_size),
                                                   ctypes.c_void_p(dst + 4), ctypes.c_uint64(n_rows), ctypes.c_uint64(stride), ctypes.c_uint32(0))
            assert rc == 0, pkg.lib().bfhip_last_error()
            got = _ctx.download(dst, n * stride + 1)
            want = np.full(n * stride + 1, FILL, dtype=np.uint32)
            wide = want[1:].reshape(n, stride)
            wide[:n_rows, :n_cols] = x
            _same(got, want)


@pytest.mark.parametrize("layout,log_size,n_cols", [("rows", 20, 7), ("columns", 22, 3)])
def test_many_workgroups(_ctx, pkg, layout, log_size, n_cols):
    table = _table(log_size, (1 << log_size) - 5, n_cols)
    _same(_run(pkg, _ctx, table, log_size, layout, pad=[P - 1] * n_cols), model.columns_from_rows(table, log_size, pad=[P - 1] * n_cols))
    if layout == "rows":
        with _ctx.columns_from_rows(table, log_size) as cols:
            _same(_ctx.rows_from_columns(cols, log_size, table.shape[0]), table)


@pytest.mark.parametrize("log_size", [4, 9])
def test_an_offset_reading_air_accepts_the_ingested_row_order_trace(_ctx, pkg, log_size):
    """What the order means, without the numpy helper: NXT[r] = A[(r + 1) mod n] written by row; a program that reads A at offset +1 against
    NXT holds on every cell, and a corrupted row r is reported at cell_of_row(r)."""
    n = 1 << log_size
    a = _table(3 + log_size, n, 1)[:, 0]
    trace = np.stack([a, np.roll(a, -1)], axis=1)
    b = pkg.AirBuilder()
    b.constraint(b.col(1) - b.col(0, 1))
    program = b.program()
    with _ctx.columns_from_rows(trace, log_size) as cols:
        rep = _ctx.air_check(program, log_size, cols.ptrs, []).as_dict()
        assert rep["n_bad_cells"] == 0, rep
    for r in (0, 5, n - 1):
        broken = trace.copy()
        broken[r, 1] = (int(broken[r, 1]) + 1) % P
        with _ctx.columns_from_rows(broken, log_size) as cols:
            rep = _ctx.air_check(program, log_size, cols.ptrs, []).as_dict()
        assert rep["n_bad_cells"] == 1 and rep["first_bad_cell"] == pkg.cell_of_row(log_size, r), (r, rep)
        assert pkg.row_of_cell(log_size, rep["first_bad_cell"]) == r


def test_air_prove_gives_the_bytes_it_gives_on_the_numpy_helpers_columns(_ctx, pkg):
    ctx, log_size = _ctx, 6
    ctx.set_conventions(*STWO)
    ctx.set_pcs_config(None)
    st = _lookup_statement(pkg, log_size)
    by_row = np.concatenate([_lookup_trace(log_size, 51), _is_first(log_size)[None]]).T.copy()      # (n, 4): a, t, mult, IsFirst — row 0 is cell 0
    proofs = []
    with Dev(ctx) as dev:
        helper = [dev.up(_storage_of_coset_order(by_row[:, c], log_size)) for c in range(4)]
        with ctx.columns_from_rows(by_row, log_size) as cols:
            _same(cols.download(), np.stack([ctx.download(p, 1 << log_size) for p in helper]))
            for tree in (helper, cols.ptrs):
                with pkg.Channel(STWO) as ch:
                    proofs.append(ctx.air_prove(st, [tree], ch))
    assert proofs[0] == proofs[1] and len(proofs[0]) > 1000
    with pkg.Channel(STWO) as ch:
        assert pkg.air_verify(st, proofs[1], ch, STWO, None) == (True, "")


def test_inside_an_open_session_without_touching_the_arena(_ctx, pkg):
    ctx, log_size = _ctx, 11
    ctx.set_conventions(*STWO)
    ctx.set_pcs_config(None)
    table = _table(44, (1 << log_size) - 1, 9)
    want = model.columns_from_rows(table, log_size, repeat_last=True)
    with pkg.Channel(STWO) as ch, pkg.PcsSession(ctx) as s:
        before = ctx.memory()["arena_in_use"]
        with ctx.columns_from_rows(table, log_size, repeat_last=True) as cols:
            assert ctx.memory()["arena_in_use"] == before
            _same(cols.download(), want)
            _same(ctx.rows_from_columns(cols, log_size, table.shape[0]), table)
            assert ctx.memory()["arena_in_use"] == before
            root = s.commit(ch, cols.ptrs, [log_size] * 9, form=0)
            assert len(root) == 32
    outside = ctx.memory()["arena_in_use"]
    with ctx.columns_from_rows(table, log_size) as cols:
        assert ctx.memory()["arena_in_use"] == outside
