"""-m gpu: bfhip_rows_fill (include/bfhip.h "Row filling", csrc/rows_fill.hip) held to bfhip_rows_fill_host word for word — the columns
(downloaded in storage order and compared with the host's rows placed by tests/columns_model.py's map) and the count: the plain and the tiled
form and the tile seams, output widths at the pass boundaries of the gather, both layouts and a stride above n_cols, gaps that end and begin
at the seams of a run and of a tile, a gap and a tail longer than a tile, offsets across the end of the domain, an order written by
bfhip_rows_select, T at the edges of the domain and above 2^32, non-canonical words, a bad order word, an open session, the scratch reserve,
every device-side refusal, and the three Brainfuck tables on real traces with bfhip_air_check over the device-built Memory table."""
import ctypes
import os

import numpy as np
import pytest

import rows_fill_cases as cases
import rows_fill_model as model
from conftest import P, ROOT
from rows_fill_cases import GROUP, STEP
from test_gpu_air_prove import STWO
from test_gpu_columns import FILL, Dev, _device_table

pytestmark = pytest.mark.gpu

WHO = "bfhip_rows_fill: "
GAPS = dict(group=(GROUP,), step=STEP, gaps=True)
ALL_KINDS = [("keep", STEP), ("keep", 2), ("set", 3, 7), ("mark", 1), ("keep", STEP, 1), ("set", 2, P - 1, 16), ("mark", 5, 16), ("keep", 4, 1)]


def _check(pkg, ctx, table, layout="rows", row_stride=None, src=None, order=None, **kw):
    """ctx.rows_fill on the device table == rows_fill_host on the host table: columns and count. Returns the host result."""
    want = pkg.rows_fill_host(table, order=order, **kw)
    log_size = want.rows.shape[0].bit_length() - 1
    with Dev(ctx) as dev:
        src = _device_table(pkg, dev, np.asarray(table), layout, row_stride, 1) if src is None else src      # one word into its allocation
        with ctx.rows_fill(src, order=order, **kw) as cols:
            assert cols.log_size == log_size and cols.n_filled == want.n_filled
            got = cols.download()
            assert got.shape == (want.rows.shape[1], 1 << log_size) and got.tobytes() == model.storage(want.rows, log_size).tobytes()
    return want


@pytest.mark.parametrize("layout", ["rows", "columns"])
@pytest.mark.parametrize("log_size", [1, 5, 9, 10, 11, 12])
def test_sizes_plain_form_one_tile_and_tile_seams(_ctx, pkg, log_size, layout):
    n = 1 << log_size
    # about a third of the domain are entries, a few short gaps between them, the tail fills the rest; then T = 2^log_size exactly
    n_entries = max(2, n // 3)
    gaps_at = [] if n_entries < 8 else [(3, 2), (n_entries // 2 + 4, 5), (n_entries + 6, 1)]
    t = cases.stepped(n_entries + 3, 6, gaps_at, group_len=None if n_entries < 8 else n_entries // 2 + 3)
    got = _check(pkg, _ctx, t, layout, 8, rows=(1, 1 + n_entries), columns=ALL_KINDS, log_size=log_size, **GAPS)
    assert n_entries <= got.n_filled <= n
    full = cases.stepped(n - 4, 6, [(1, 4)]) if n >= 8 else cases.stepped(n, 6)
    assert _check(pkg, _ctx, full, layout, columns=ALL_KINDS, log_size=log_size, **GAPS).n_filled == n
    _check(pkg, _ctx, full, layout, columns=ALL_KINDS, log_size=log_size, step=STEP)      # no gaps asked for: the tail alone


@pytest.mark.parametrize("layout", ["rows", "columns"])
@pytest.mark.parametrize("n_out", [1, 8, 9, 16, 17])
def test_output_widths_at_the_pass_boundaries(_ctx, pkg, n_out, layout):
    t = cases.stepped(700, 6, [(5, 40), (300, 3), (600, 90)], group_len=450)
    kinds = [("keep", (5 * k) % 6, k % 17) if k % 3 == 0 else ("set", (5 * k) % 6, (k * 77) % P, k % 17) if k % 3 == 1 else ("mark", k + 1, (3 * k) % 17) for k in range(n_out)]
    for log_size in (11, 10):      # two workgroups, one
        _check(pkg, _ctx, t, layout, 9, columns=kinds, log_size=log_size, **GAPS)
    _check(pkg, _ctx, t[:100], layout, 9, columns=kinds, log_size=9, **GAPS)      # plain


@pytest.mark.parametrize("gaps_at", [[(20, 12), (1000, 24)], [(32, 7), (1024, 9)], [(31, 1), (33, 1), (1023, 1), (1025, 2)], [(31, 2), (1023, 2)]],
                         ids=["ending at 31 and 1023", "beginning at 32 and 1024", "of one row around the seams", "across the seams"])
def test_gaps_at_the_seams_of_a_run_and_of_a_tile(_ctx, pkg, gaps_at):
    t = cases.stepped(1500, 5, gaps_at)
    for layout in ("rows", "columns"):
        got = _check(pkg, _ctx, t, layout, columns=ALL_KINDS, log_size=11, **GAPS)
        assert got.n_filled == 1500 + sum(g for _, g in gaps_at)
        for start, length in gaps_at:      # the d column: the gap's rows and no other around it
            assert (got.rows[start:start + length, 3] == 1).all() and got.rows[start - 1, 3] == 0 and got.rows[start + length, 3] == 0


def test_whole_tiles_of_inserted_rows_a_gap_before_the_last_entry_and_a_long_tail(_ctx, pkg):
    for layout in ("rows", "columns"):
        # one gap of 3000 rows in a 2^12 domain: output rows 500 .. 3499, tiles that hold nothing but inserted rows of entry 499
        got = _check(pkg, _ctx, cases.stepped(900, 5, [(500, 3000)]), layout, columns=ALL_KINDS, log_size=12, **GAPS)
        assert got.n_filled == 3900 and (got.rows[500:3500, 3] == 1).all() and (got.rows[500:3500, 0] == got.rows[499, 0] + 1 + np.arange(3000)).all()
        # a gap directly in front of the last entry, which is the last row of the domain
        got = _check(pkg, _ctx, cases.stepped(600, 5, [(599, 1448)]), layout, columns=ALL_KINDS, log_size=11, **GAPS)
        assert got.n_filled == 2048 and got.rows[2047, 3] == 0 and got.rows[2046, 3] == 1
        # a tail longer than a tile: 40 entries in a 2^12 domain; and one that wraps past p - 1
        got = _check(pkg, _ctx, cases.stepped(40, 5, [(7, 3)]), layout, columns=ALL_KINDS, log_size=12, **GAPS)
        assert got.n_filled == 43 and (got.rows[43:, 3] == 1).all()
        got = _check(pkg, _ctx, cases.stepped(40, 5, first_step=P - 41), layout, columns=ALL_KINDS, log_size=11, **GAPS)
        assert got.rows[39, 0] == P - 2 and got.rows[40:43, 0].tolist() == [P - 1, 0, 1]


def test_offsets_across_the_end_of_the_domain(_ctx, pkg):
    t = cases.stepped(1020, 5, [(1010, 3)])      # T = 1023: offset 1 of the last row is the pairing dummy, offset 16 reaches 15 rows further
    outs = [("keep", STEP, 0), ("keep", STEP, 1), ("keep", STEP, 16), ("set", 2, 9, 1), ("set", 2, 9, 16), ("mark", 1, 1), ("mark", 1, 16)]
    for layout in ("rows", "columns"):
        got = _check(pkg, _ctx, t, layout, columns=outs, log_size=10, **GAPS)
        assert (got.rows[:, 1] == (got.rows[:, 0].astype(np.int64) + 1) % P).all() and got.rows[1023, 2] == (int(got.rows[1023, 0]) + 16) % P
        _check(pkg, _ctx, t[:500], layout, columns=outs, log_size=9, **GAPS)
        full = cases.stepped(1024, 5)      # T = 2^log_size: every element past the last row is tail
        got = _check(pkg, _ctx, full, layout, columns=outs, log_size=10, **GAPS)
        assert got.rows[1023, 5] == 1 and got.rows[1007, 6] == 0 and got.rows[1008, 6] == 1


def test_order_from_rows_select_and_a_row_range(_ctx, pkg):
    rng = np.random.default_rng(11)
    t = rng.integers(0, P, size=(2000, 5), dtype=np.uint32)
    t[:, 0] = rng.integers(0, 5, size=2000)              # the group
    t[:, 1] = rng.permutation(6000)[:2000]               # the step: distinct, so that gaps appear once sorted
    want_order = pkg.rows_select_host(t, order_by=(0, 1), count_only=True, want_order=True).order
    for layout in ("rows", "columns"):
        with Dev(_ctx) as dev:
            src = _device_table(pkg, dev, t, layout, 7, 1)
            order_d = dev.filled(2000)
            assert _ctx.rows_select_count(src, order_by=(0, 1), order_out=order_d) == (2000, None)
            assert (_ctx.download(order_d, 2000) == want_order).all()
            want = pkg.rows_fill_host(t, order=want_order, columns=ALL_KINDS, **GAPS)
            assert want.n_filled > 2000
            with _ctx.rows_fill(src, order=order_d, n_order=2000, columns=ALL_KINDS, **GAPS) as cols:
                assert cols.n_filled == want.n_filled and cols.download().tobytes() == model.storage(want.rows, cols.log_size).tobytes()
        # no order: the rows of a range that does not start at 0 (the unsorted steps: ascents are gaps, descents are not)
        _check(pkg, _ctx, t[:200], layout, 7, rows=(13, 150), columns=ALL_KINDS, log_size=None, step=1, gaps=True)


def test_count_at_the_edges_of_the_domain_and_above_2_to_32(_ctx, pkg):
    t = cases.stepped(500, 4, [(100, 12)])      # T = 512
    with Dev(_ctx) as dev:
        src = _device_table(pkg, dev, t, "rows")
        assert _ctx.rows_fill_count(src, **GAPS) == 512 and _ctx.rows_fill_count(src, step=STEP) == 500
        out = [dev.filled(512), dev.filled(512)]
        with _ctx.rows_fill(src, 9, columns=[0, ("mark", 1)], out=out, **GAPS) as cols:
            assert cols.n_filled == 512 and (_ctx.rows_from_columns(cols, 9)[:, 1] == np.r_[np.zeros(100), np.ones(12), np.zeros(400)]).all()
        more = _device_table(pkg, dev, cases.stepped(500, 4, [(100, 13)]), "rows")
        out = [dev.filled(512), dev.filled(512)]
        with pytest.raises(pkg.BfhipError) as e:
            _ctx.rows_fill(more, 9, columns=[0, ("mark", 1)], out=out, **GAPS)
        assert str(e.value) == WHO + "513 rows after filling, the domain has 512"
        # three gaps of 1431655765 rows between six entries: T = 2^32 + 5, which a 32-bit total would take for 5
        g = 1431655765
        big = np.zeros((6, 3), dtype=np.uint32)
        big[:, STEP] = [0, g + 1] * 3
        assert model.count(big, (GROUP,), STEP, True) == (1 << 32) + 5
        wide = _device_table(pkg, dev, big, "rows")
        with pytest.raises(pkg.BfhipError) as e:
            _ctx.rows_fill(wide, 9, columns=[0, ("mark", 1)], out=out, **GAPS)
        assert str(e.value) == WHO + "4294967301 rows after filling, the domain has 512"
        assert _ctx.rows_fill_count(wide, **GAPS) == (1 << 32) + 5
        assert all((_ctx.download(p, 512) == FILL).all() for p in out)
        _check(pkg, _ctx, t, columns=[0, ("mark", 1)], log_size=9, **GAPS)      # and the context works afterwards


@pytest.mark.parametrize("layout", ["rows", "columns"])
def test_non_canonical_words_are_named_lowest_first_and_the_context_works_afterwards(_ctx, pkg, layout):
    base = cases.stepped(1500, 6, [(40, 30), (900, 200)], group_len=800)
    kw = dict(columns=[("keep", 2), ("set", 3, 1, 1), ("mark", 1), ("keep", 5, 16)], rows=(2, 1400), **GAPS)
    plants = {"a group word": [(700, GROUP, P), (1200, GROUP, P + 5)], "a step word": [(800, STEP, 0xFFFFFFFF)],      # the first entry of its group, and the next step descends: no gap of 2^32 rows
              "an output word": [(60, 2, P), (1000, 5, P)], "several": [(1100, 3, 0x80000000), (1030, 5, P), (1030, 2, P), (1080, GROUP, P)]}
    for log_size in (11, 9):      # tiled; plain over fewer entries
        if log_size == 9:
            kw = dict(kw, rows=(2, 200))
            plants = {"a group word and an output word": [(150, GROUP, P), (120, 5, P)], "an output word": [(199, 3, P), (180, 2, P + 1)]}
        for what, words in plants.items():
            t = base.copy()
            for r, c, v in words:
                t[r, c] = v
            with pytest.raises(pkg.BfhipError) as e:
                _check(pkg, _ctx, t, layout, 8, log_size=log_size, **kw)
            host = str(e.value)
            want = model.lowest_bad_word(t, log_size, (GROUP,), STEP, True, kw["columns"], rows=kw["rows"])
            assert host == "bfhip_rows_fill_host: row %d, column %d: %d is not a canonical M31 value" % want, what
            with Dev(_ctx) as dev, pytest.raises(pkg.BfhipError) as e:
                _ctx.rows_fill(_device_table(pkg, dev, t, layout, 8), log_size=log_size, **kw)
            assert str(e.value) == host.replace("bfhip_rows_fill_host: ", WHO), what
        _check(pkg, _ctx, base, layout, 8, log_size=log_size, **kw)      # the context works afterwards
    # words nobody reads may hold anything: in front of and behind the entries, and in a column that nothing names
    t = base.copy()
    t[210:, :] = 0xFFFFFFFF
    t[:2, :] = 0xFFFFFFFF
    t[5, 4] = P + 9
    _check(pkg, _ctx, t, layout, 8, log_size=9, **kw)


def test_a_bad_order_word_is_named_and_nothing_is_read_through_it(_ctx, pkg):
    t = cases.stepped(1200, 4, [(30, 5)])      # the table is the first 1000 rows of an allocation of 1200
    order = np.arange(1000, dtype=np.uint32)
    order[[400, 777]] = [1000, 1100]
    with Dev(_ctx) as dev:
        for layout in ("rows", "columns"):
            whole = _device_table(pkg, dev, t, layout)
            src = pkg.DeviceRows(whole.ptr, 1000, 4, 4) if layout == "rows" else pkg.DeviceRowColumns(whole.ptrs, 1000)
            out = [dev.filled(2048), dev.filled(2048)]
            for kw in (GAPS, dict(step=STEP)):
                with pytest.raises(pkg.BfhipError) as e:
                    _ctx.rows_fill(src, 11, order=order, columns=[STEP, ("mark", 1)], out=out, **kw)
                assert str(e.value) == WHO + "order[400] = 1000 is not a row of the table (1000 rows)"
                assert all((_ctx.download(p, 2048) == FILL).all() for p in out)
            with pytest.raises(pkg.BfhipError) as e:
                _ctx.rows_fill_count(src, order=order, **GAPS)
            assert str(e.value) == WHO + "order[400] = 1000 is not a row of the table (1000 rows)"
            good = np.arange(1000, dtype=np.uint32)[::-1].copy()
            want = pkg.rows_fill_host(t[:1000], order=good, columns=[STEP, ("mark", 1)], log_size=11, **GAPS)
            with _ctx.rows_fill(src, 11, order=good, columns=[STEP, ("mark", 1)], **GAPS) as cols:      # the context works afterwards
                assert cols.n_filled == want.n_filled == 1000 and cols.download().tobytes() == model.storage(want.rows, 11).tobytes()
    with pytest.raises(pkg.BfhipError) as e:
        pkg.rows_fill_host(t[:1000], order=order, columns=[STEP], log_size=11, **GAPS)
    assert str(e.value) == "bfhip_rows_fill_host: order[400] = 1000 is not a row of the table (1000 rows)"


def test_inside_an_open_session_without_touching_the_arena(_ctx, pkg):
    ctx = _ctx
    ctx.set_conventions(*STWO)
    ctx.set_pcs_config(None)
    t = cases.stepped(1500, 5, [(100, 700), (1900, 40)], group_len=900)
    kw = dict(columns=ALL_KINDS[:4], log_size=12, **GAPS)
    outside = _check(pkg, ctx, t, **kw)
    with pkg.Channel(STWO) as ch, pkg.PcsSession(ctx) as s:
        before = ctx.memory()["arena_in_use"]
        inside = _check(pkg, ctx, t, **kw)
        assert ctx.memory()["arena_in_use"] == before
        assert (inside.rows == outside.rows).all() and inside.n_filled == outside.n_filled
        with ctx.rows_fill(np.asarray(t), **kw) as cols:
            assert ctx.memory()["arena_in_use"] == before
            assert len(s.commit(ch, cols.ptrs, [12] * 4, form=0)) == 32


def test_second_call_of_a_shape_allocates_nothing_with_a_scratch_reserve(pkg):
    t = cases.stepped(1500, 5, [(100, 700), (1900, 40)], group_len=900)
    kw = dict(columns=ALL_KINDS, log_size=12, **GAPS)
    ctx = pkg.Context(0, max_log_domain=14)
    try:
        ctx.set_scratch_reserve(8 << 20)
        with Dev(ctx) as dev:
            src = _device_table(pkg, dev, np.asarray(t), "rows")
            _check(pkg, ctx, t, src=src, **kw)
            first = ctx.scratch_stats()
            _check(pkg, ctx, t, src=src, **kw)
            second = ctx.scratch_stats()
        assert second["device_allocations"] == first["device_allocations"] and second["served"] > first["served"] and first["high_water"] > 0
    finally:
        ctx.close()


def test_every_device_side_refusal_leaves_the_columns_alone(_ctx, pkg):
    ctx, n = _ctx, 16
    t = np.arange(40, dtype=np.uint32).reshape(10, 4)
    L = pkg.lib()
    Out, Desc, Table = pkg.FillOut, pkg.RowsFillDesc, pkg.RowsTable
    U32P = ctypes.POINTER(ctypes.c_uint32)
    with Dev(ctx) as dev:
        rows_d = dev.up(np.concatenate([t.ravel(), np.zeros(8, dtype=np.uint32)]))
        big = dev.filled(3 * n)
        order_d = dev.up(np.arange(10))
        col_ptrs = [dev.up(t[:, c]) for c in range(4)]
        cols_h = (ctypes.c_void_p * 4)(*col_ptrs)
        outs = (Out * 2)(Out(0, 0, 0, 0), Out(1, 0, 0, 1))
        n_filled = ctypes.c_uint64(77)
        group1 = (ctypes.c_uint32 * 5)(2, 2, 2, 2, 2)

        def table(layout=0, n_cols=4, rows=rows_d, cols=None, n_rows=10, stride=4, flags=0, reserved=0):
            return Table(layout, n_cols, ctypes.cast(rows, U32P), cols, n_rows, stride, flags, reserved)

        def desc(group=None, n_group=0, step=0, order=None, n_entries=10, row_begin=0, flags=0, reserved=0):
            return Desc(ctypes.cast(group, U32P) if group is not None else None, n_group, step, ctypes.cast(order, U32P) if order else None, n_entries, row_begin, flags, reserved)

        def call(tab, fill, log_size=4, outs_=outs, out_ptrs=(big, big + 4 * n), n_out=2, nf=n_filled, handle=ctx._h):
            ptrs = None if out_ptrs is None else (ctypes.c_void_p * max(1, len(out_ptrs)))(*out_ptrs)
            rc = L.bfhip_rows_fill(handle, None if tab is None else ctypes.byref(tab), None if fill is None else ctypes.byref(fill), ctypes.c_uint32(log_size), outs_, ptrs,
                                   ctypes.c_uint32(n_out), None if nf is None else ctypes.byref(nf))
            return rc, L.bfhip_last_error().decode() if rc else ""

        col_major = table(layout=1, rows=None, cols=ctypes.cast(cols_h, ctypes.POINTER(ctypes.c_void_p)))
        holed = (ctypes.c_void_p * 4)(col_ptrs[0], None, col_ptrs[2], col_ptrs[3])
        refusals = [
            ((None, desc()), {}, "null argument"), ((table(), None), {}, "null argument"), ((table(), desc()), dict(nf=None), "null argument"),
            ((table(), desc()), dict(outs_=None), "null argument"),
            ((table(reserved=1), desc()), {}, "reserved must be 0"), ((table(layout=2), desc()), {}, "unknown layout 2"), ((table(flags=2), desc()), {}, "unknown flag bits 2"),
            ((table(flags=1), desc()), {}, "BFHIP_ROWS_REPEAT_LAST does not apply: the tail is this call's padding"),
            ((table(stride=3), desc()), {}, "row_stride 3 is below n_cols 4"), ((table(n_cols=0, stride=0), desc()), {}, "the table has no columns"),
            ((table(rows=None), desc()), {}, "null table pointer"), ((table(layout=1, rows=None), desc()), {}, "null table pointer"),
            ((table(layout=1, rows=None, cols=ctypes.cast(holed, ctypes.POINTER(ctypes.c_void_p))), desc()), {}, "source column 1 is a null pointer"),
            ((table(), desc()), dict(log_size=0), "log_size 0 is outside 1..30"), ((table(), desc()), dict(log_size=31), "log_size 31 is outside 1..30"),
            ((table(), desc()), dict(n_out=0), "n_out 0 is outside 1..256 (BFHIP_AIR_MAX_COLUMNS)"),
            ((table(), desc()), dict(out_ptrs=None), "the count-only form takes null outputs, n_out 0 and log_size 0 together"),
            ((table(), desc()), dict(out_ptrs=None, n_out=0), "the count-only form takes null outputs, n_out 0 and log_size 0 together"),
            ((table(), desc()), dict(out_ptrs=(big, None)), "output column 1 is a null pointer"),
            ((table(), desc()), dict(outs_=(Out * 2)(Out(0, 0, 0, 0), Out(1, 3, 0, 0))), "output 1: unknown kind 3"),
            ((table(), desc()), dict(outs_=(Out * 2)(Out(0, 0, 0, 0), Out(4, 1, 0, 0))), "output 1: column index 4 is not below n_cols 4"),
            ((table(), desc()), dict(outs_=(Out * 2)(Out(0, 1, P, 0), Out(1, 0, 0, 0))), "output 0: value 2147483647 is not a canonical M31 value"),
            ((table(), desc()), dict(outs_=(Out * 2)(Out(0, 0, 0, 0), Out(9, 2, P, 0))), "output 1: value 2147483647 is not a canonical M31 value"),
            ((table(), desc()), dict(outs_=(Out * 2)(Out(0, 0, 0, 17), Out(1, 0, 0, 0))), "output 0: offset 17 exceeds 16 (BFHIP_FILL_MAX_OFFSET)"),
            ((table(), desc(reserved=3)), {}, "reserved must be 0"), ((table(), desc(flags=2)), {}, "unknown flag bits 2"),
            ((table(), desc(group=group1, n_group=5)), {}, "n_group 5 exceeds 4 (BFHIP_FILL_MAX_GROUP)"),
            ((table(), desc(n_group=1)), {}, "n_group 1 with a null group_cols array"),
            ((table(), desc(group=(ctypes.c_uint32 * 2)(1, 4), n_group=2)), {}, "group 1: column index 4 is not below n_cols 4"),
            ((table(), desc(step=4)), {}, "step: column index 4 is not below n_cols 4"),
            ((table(), desc(step=0xFFFFFFFF, flags=1)), {}, "BFHIP_FILL_GAPS needs a step column"),
            ((table(), desc(n_entries=0)), {}, "needs at least one entry"),
            ((table(n_rows=1 << 31), desc(n_entries=(1 << 30) + 1)), {}, "1073741825 entries exceed 2^30"),
            ((table(), desc(n_entries=8, row_begin=3)), {}, "row_begin 3 + n_entries 8 exceeds n_rows 10"),
            ((table(), desc(order=order_d, n_entries=5, row_begin=1)), {}, "row_begin 1 must be 0 when an order is given"),
            ((table(n_rows=(1 << 40) + 1), desc()), {}, "n_rows 1099511627777 exceeds 2^40"),
            ((table(), desc()), dict(out_ptrs=(big, big + 4 * n - 4)), "output column 1 overlaps output column 0"),
            ((table(), desc()), dict(out_ptrs=(big, rows_d + 4 * 39)), "output column 1 overlaps the source table"),
            ((col_major, desc()), dict(out_ptrs=(big, col_ptrs[2] + 36)), "output column 1 overlaps source column 2"),
            ((table(), desc(order=order_d)), dict(out_ptrs=(order_d + 36, big)), "output column 0 overlaps the order"),
            ((table(), desc()), dict(log_size=3), "10 rows after filling, the domain has 8"),
            ((table(), desc(flags=1)), dict(log_size=3), "37 rows after filling, the domain has 8"),      # column 0 steps by 4: nine gaps of 3
        ]
        for (tab, fill), kw, rule in refusals:
            assert call(tab, fill, **kw) == (-1, WHO + rule), rule
            assert (ctx.download(big, 3 * n) == FILL).all() and (ctx.download(order_d, 10) == np.arange(10)).all(), rule
        assert call(table(), desc(), handle=None) == (-1, "null context")
        # a context in a shard group
        group, member = pkg.LocalGroup(2), pkg.Context(0, max_log_domain=10)
        try:
            member.join_local_group(group, 0)
            for tab in (table(), col_major):
                assert call(tab, desc(), handle=member._h) == (-1, WHO + "a context in a shard group is not supported (bfhip_ctx_leave_group first)")
                assert (ctx.download(big, 3 * n) == FILL).all()
            member.leave_group()
            assert call(table(), desc(n_entries=8, row_begin=1), handle=member._h) == (0, "") and n_filled.value == 8      # and works once it has left
        finally:
            member.close(); group.close()
        # the good call on the same context, both layouts, with and without the order
        for tab in (table(), col_major):
            for fill in (desc(n_entries=8, row_begin=1), desc(order=order_d + 4, n_entries=8)):
                assert call(tab, fill) == (0, "") and n_filled.value == 8
                got = ctx.download(big, 3 * n).reshape(3, n)
                rows = np.zeros((16, 2), dtype=np.uint32)
                rows[:8, 0] = t[1:9, 0]
                rows[8:, 0] = (t[8, 0] + 1 + np.arange(8)) % P      # column 0 is the step: the tail counts on
                rows[:7, 1] = t[2:9, 1]
                rows[7:, 1] = t[8, 1]
                assert (got[:2] == model.storage(rows, 4)).all() and (got[2] == FILL).all()


@pytest.mark.parametrize("program,inp", [("hello_kakarot.bf", b""), ("collatz.bf", bytes([55, 10]))])
def test_brainfuck_tables_on_a_real_trace(_ctx, pkg, program, inp):
    """The Memory, Instruction and Processor tables built whole on the device by rows_select and rows_fill equal bfhip_host_table in every row
    and column; the Memory table's non-logUp constraints (memory/component.rs:81-122 without is_first: d and next_d boolean, mp rises by 0 or
    1, clk by 1 where mp stays, next_mv = 0 where mp rises, a dummy keeps mp and mv), stated directly, hold on every row of the device-built
    columns by bfhip_air_check — the inserted rows and the dummies behind the entries included."""
    code = open(os.path.join(ROOT, "tests", "golden", "programs", program)).read()
    regs, words = pkg.host_run(code, inp)[1], pkg.host_compile(code)
    assert regs.shape[0] > 500
    kept = {}

    def select_device(src, **kw):
        with Dev(_ctx) as dev:
            order_d = dev.filled(src.shape[0])
            assert _ctx.rows_select_count(src, order_out=order_d, **{k: v for k, v in kw.items() if k != "want_order"}) == (src.shape[0], None)
            return _ctx.download(order_d, src.shape[0])

    def fill_device(src, order, **kw):
        cols = _ctx.rows_fill(src, order=order, **kw)
        kept["cols"] = cols
        host = pkg.rows_fill_host(src, order=order, **kw)
        assert cols.n_filled == host.n_filled and cols.log_size == host.rows.shape[0].bit_length() - 1
        return _ctx.rows_from_columns(cols, cols.log_size), cols.n_filled

    for name in ("memory", "instruction", "processor"):
        T, n_entries = cases.brainfuck_table(pkg, regs, words, name, select_device, fill_device)
        assert T > n_entries if name == "memory" else T == n_entries
        with kept.pop("cols") as cols:
            if name == "memory":
                c = pkg.AirBuilder()
                clk, mp, mv, d, n_clk, n_mp, n_mv, n_d = (c.col(j) for j in range(8))
                c.constraint(d * (d - 1))
                c.constraint(n_d * (n_d - 1))
                c.constraint((n_mp - mp) * (n_mp - mp - 1))
                c.constraint((n_mp - mp - 1) * (n_clk - clk - 1))
                c.constraint((n_mp - mp) * n_mv)
                c.constraint(d * (n_mp - mp))
                c.constraint(d * (n_mv - mv))
                rep = _ctx.air_check(c.program(), cols.log_size, cols.ptrs, [])
                assert rep.as_dict()["n_bad_cells"] == 0 and pkg.format_air_check(rep) == "air check: ok"
