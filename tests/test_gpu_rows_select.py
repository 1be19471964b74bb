"""-m gpu: bfhip_rows_select (include/bfhip.h "Row selection", csrc/rows_select.hip) held to bfhip_rows_select_host word for word — the columns
(downloaded in storage order and compared with the host's rows placed by tests/columns_model.py's map, or read back with
bfhip_rows_from_columns), the order and the count: the plain and the tiled form and the tile seams, candidate counts at the scan's tile and
block seams, output widths at the pass boundaries of the gather, both layouts and a stride above n_cols, S at the edges of the domain, one
to four keys, offsets, paddings, non-canonical words, an open session, the scratch reserve, every device-side refusal, and the Brainfuck
example on a real trace."""
import ctypes
import os

import numpy as np
import pytest

import rows_select_cases as cases
import rows_select_model as model
from conftest import P, ROOT
from test_gpu_air_prove import STWO
from test_gpu_columns import FILL, Dev, _device_table

pytestmark = pytest.mark.gpu

WHO = "bfhip_rows_select: "
_TABLES = {}


def _table(n_rows, n_cols, seed=1):
    """One seeded table per shape, shared by the tests and never modified (a test that plants words copies it)."""
    key = (n_rows, n_cols, seed)
    if key not in _TABLES:
        t = model.random_table(np.random.default_rng(1000 * seed + n_cols), n_rows, n_cols, small=8)
        t.setflags(write=False)
        _TABLES[key] = t
    return _TABLES[key]


def _check(pkg, ctx, table, layout="rows", row_stride=None, src=None, **kw):
    """ctx.rows_select on the device table == rows_select_host on the host table: columns, count and order. Returns the host result."""
    want = pkg.rows_select_host(table, want_order=True, **kw)
    log_size = want.rows.shape[0].bit_length() - 1
    with Dev(ctx) as dev:
        src = _device_table(pkg, dev, np.asarray(table), layout, row_stride, 1) if src is None else src      # one word into its allocation
        with ctx.rows_select(src, want_order=True, **kw) as cols:
            assert cols.log_size == log_size and cols.n_selected == want.n_selected
            assert cols.order.dtype == np.uint32 and (cols.order == want.order).all()
            got = cols.download()
            assert got.shape == (want.rows.shape[1], 1 << log_size) and got.tobytes() == model.storage(want.rows, log_size).tobytes()
    return want


@pytest.mark.parametrize("layout", ["rows", "columns"])
@pytest.mark.parametrize("log_size", [1, 5, 9, 10, 11, 12])
def test_sizes_plain_form_one_tile_and_tile_seams(_ctx, pkg, log_size, layout):
    n = 1 << log_size
    t = _table(n + 9, 5)
    # every row of the domain selected (S = 2^log_size), in sorted order, read at an offset; then about half of them, padded
    _check(pkg, _ctx, t, layout, 7, rows=(3, n + 3), order_by=(0, (1, "desc")), columns=[2, (3, 6), (4, -3), 0], log_size=log_size)
    got = _check(pkg, _ctx, t, layout, None, rows=(3, n + 3), where=[(0, "<", 4)], order_by=((2, "desc"),), columns=[2, (3, 6), (4, -3)], pad=[1, P - 1, 0], log_size=log_size)
    assert got.n_selected <= n
    if got.n_selected:
        _check(pkg, _ctx, t, layout, None, rows=(3, n + 3), where=[(0, "<", 4)], columns=[2, (3, 6)], repeat_last=True, log_size=log_size)


@pytest.mark.parametrize("n_cand", [1, 255, 2048, 2049, 4097, 1 << 12])
def test_candidate_counts_at_the_scan_seams(_ctx, pkg, n_cand):
    t = _table(4100, 5)
    for layout in ("rows", "columns"):
        _check(pkg, _ctx, t, layout, rows=(1, 1 + n_cand), where=[(0, "!=", 3)], order_by=(3, 0), columns=[2, (4, -1)], log_size=13)
    # the count-only form over the same candidates, with and without the order
    S, order = _ctx.rows_select_count(t, where=[(0, "!=", 3)], rows=(1, 1 + n_cand), order_by=(3, 0), want_order=True)
    want = pkg.rows_select_host(t, where=[(0, "!=", 3)], rows=(1, 1 + n_cand), order_by=(3, 0), count_only=True, want_order=True)
    assert S == want.n_selected and (order == want.order).all()
    assert _ctx.rows_select_count(t, where=[(0, "!=", 3)], rows=(1, 1 + n_cand))[0] == S
    # log_size None: the smallest domain that holds the selection
    with _ctx.rows_select(t, where=[(0, "!=", 3)], rows=(1, 1 + n_cand), columns=[2]) as cols:
        assert cols.n_selected == S and cols.log_size == max(1, (S - 1).bit_length()) and cols.order is None


@pytest.mark.parametrize("layout", ["rows", "columns"])
@pytest.mark.parametrize("n_out", [1, 8, 9, 16, 17])
def test_output_widths_at_the_pass_boundaries(_ctx, pkg, n_out, layout):
    t = _table(3000, 6)
    columns = [((5 * k) % 6, (k % 5) - 2) for k in range(n_out)]
    pad = [(k * 77) % P for k in range(n_out)]
    for log_size in (11, 9):      # tiled (two workgroups), plain
        n = 1 << log_size
        _check(pkg, _ctx, t, layout, 9, rows=(2, 2 + n + 20), where=[(0, ">=", 1)], order_by=((3, "desc"), 1), columns=columns, pad=pad, log_size=log_size)


def test_count_at_the_edges_of_the_domain(_ctx, pkg):
    t = np.array(_table(1100, 4))
    t[:, 0] = (np.arange(1100) % 2)                       # 550 ones; 1025 candidates hold 512 or 513 of them
    for layout in ("rows", "columns"):
        assert _check(pkg, _ctx, t, layout, where=[(0, "==", 7)], log_size=10, pad=[4, 3, 2, 1]).n_selected == 0
        assert _check(pkg, _ctx, t, layout, where=[(0, "==", 7)], log_size=3, pad=[4, 3, 2, 1]).n_selected == 0
        assert _check(pkg, _ctx, t, layout, where=[(1, ">=", 0)], rows=(5, 6), log_size=10, order_by=(1,)).n_selected == 1
        assert _check(pkg, _ctx, t, layout, where=[(1, ">=", 0)], rows=(5, 6), log_size=1, repeat_last=True).n_selected == 1
        assert _check(pkg, _ctx, t, layout, where=[(0, "==", 1)], rows=(0, 1024), log_size=9, order_by=(2,)).n_selected == 512      # S = 2^log_size
        assert _check(pkg, _ctx, t, layout, rows=(0, 1024), log_size=10, order_by=((3, "desc"),), columns=[(1, 76), 0]).n_selected == 1024
    # S = 2^log_size + 1: refused after the count, the columns untouched
    with Dev(_ctx) as dev:
        src = _device_table(pkg, dev, t, "rows")
        out = [dev.filled(512), dev.filled(512)]
        for kw, rule in ((dict(where=[(0, "==", 1)], rows=(1, 1026), log_size=9), "513 rows selected, the domain has 512"),
                         (dict(where=[(0, "==", 7)], log_size=9, repeat_last=True), "BFHIP_ROWS_REPEAT_LAST needs at least one selected row")):
            with pytest.raises(pkg.BfhipError) as e:
                _ctx.rows_select(src, columns=[1, 2], out=out, **kw)
            assert str(e.value) == WHO + rule
            assert all((_ctx.download(p, 512) == FILL).all() for p in out)


@pytest.mark.parametrize("order_by", [(0,), ((1, "desc"),), (0, 3), (0, (3, "desc"), 1), ((3, "desc"), 0, (1, "desc"), 2), (3, 3, 3)],
                         ids=["1 key", "1 key desc over 0 and p - 1", "2 keys", "3 keys", "4 keys", "3 equal keys"])
def test_sorts(_ctx, pkg, order_by):
    t = np.array(_table(2500, 5))
    t[:, 3] = np.arange(2500) % 3
    for layout in ("rows", "columns"):
        _check(pkg, _ctx, t, layout, order_by=order_by, log_size=12, columns=[2, 4])
        _check(pkg, _ctx, t, layout, order_by=order_by, where=[(0, "<=", 5), (1, "!=", 1)], log_size=12, columns=[2, (4, 0)])      # a filter and a sort
    same = np.array(_table(2500, 5))
    same[:, 0] = 5
    got = _check(pkg, _ctx, same, order_by=(0, (0, "desc"), 0), log_size=12, columns=[2])
    assert (got.order == np.arange(2500)).all()      # all keys equal: the order is the source's


def test_offsets_repeat_last_and_pads(_ctx, pkg):
    t = _table(3000, 6)
    kw = dict(rows=(100, 2500), where=[(0, "!=", 0)], order_by=(3,), log_size=12)      # offsets -100 .. +500 are what the range admits
    for layout in ("rows", "columns"):
        _check(pkg, _ctx, t, layout, columns=[(2, -1), (2, 1), (5, -100), (5, 500), 4], pad=[0, 1, P - 1, 7, 8], **kw)
        _check(pkg, _ctx, t, layout, columns=[(2, -1), (2, 1), (5, -100), (5, 500), 4], repeat_last=True, **kw)
        _check(pkg, _ctx, t, layout, columns=[(1, -7)], rows=(7, 8), repeat_last=True, log_size=4)
    for off, rows, text in ((-101, (100, 2500), "reads in front of the table from row_begin 100"), (501, (100, 2500), "reads behind the table's 3000 rows from row_end 2500")):
        with pytest.raises(pkg.BfhipError) as e:
            _ctx.rows_select(np.asarray(t), log_size=12, columns=[0, (1, off)], rows=rows)
        assert str(e.value) == WHO + "output 1: offset %d %s" % (off, text)


def test_read_back_by_rows_from_columns(_ctx, pkg):
    t = _table(3000, 6)
    kw = dict(where=[(0, ">", 2)], order_by=((1, "desc"), 0), columns=[5, (2, 3), 0], rows=(0, 2900), pad=[9, 8, 7], log_size=12)
    want = pkg.rows_select_host(t, **kw)
    with _ctx.rows_select(np.asarray(t), **kw) as cols:
        assert (_ctx.rows_from_columns(cols, 12) == want.rows).all()


@pytest.mark.parametrize("layout", ["rows", "columns"])
def test_non_canonical_words_are_named_lowest_first_and_the_context_works_afterwards(_ctx, pkg, layout):
    base = np.array(_table(3000, 6))
    base[:, 0] = np.arange(3000) % 4
    kw = dict(where=[(0, "!=", 3), (3, ">=", 0)], order_by=((1, "desc"), 2), columns=[(4, -2), 5, (4, 3)], rows=(2, 2900))
    plants = {"a term word of an unselected candidate": [(7, 3, P), (2001, 3, P + 5)],
              "a key word": [(1500, 2, 0xFFFFFFFF), (1500, 1, P), (2600, 4, P)],
              "an output word at an offset": [(0, 4, P), (1600, 5, P)],
              "an output word behind the candidates": [(2901, 4, P + 1)],      # row 2898 at offset +3
              "several": [(2100, 0, 0x80000000), (1030, 5, P), (1030, 4, P), (1080, 3, P)]}
    for log_size in (12, 9):      # tiled; plain over fewer candidates
        if log_size == 9:
            kw = dict(kw, rows=(2, 600))
            plants = {"a key word and a term word": [(300, 2, P), (301, 3, P)], "an output word at an offset": [(0, 4, P), (500, 5, P)]}
        for what, words in plants.items():
            t = base.copy()
            for r, c, v in words:
                t[r, c] = v
            want = model.lowest_bad_word(t, log_size=log_size, **kw)
            with pytest.raises(pkg.BfhipError) as e:
                _check(pkg, _ctx, t, layout, 8, log_size=log_size, **kw)
            assert str(e.value) == "bfhip_rows_select_host: row %d, column %d: %d is not a canonical M31 value" % want, what
            with Dev(_ctx) as dev, pytest.raises(pkg.BfhipError) as e:
                _ctx.rows_select(_device_table(pkg, dev, t, layout, 8), log_size=log_size, **kw)
            assert str(e.value) == WHO + "row %d, column %d: %d is not a canonical M31 value" % want, what
        _check(pkg, _ctx, base, layout, 8, log_size=log_size, **kw)      # the context works afterwards
    # words nobody reads may hold anything
    t = base.copy()
    t[7, 1] = t[7, 2] = t[7, 5] = P + 9      # row 7 is not selected: its key words and its own output word
    t[610:, :] = 0xFFFFFFFF                  # behind every read: candidates end at 599, the largest offset is +3
    _check(pkg, _ctx, t, layout, 8, log_size=9, **kw)


def test_inside_an_open_session_without_touching_the_arena(_ctx, pkg):
    ctx = _ctx
    ctx.set_conventions(*STWO)
    ctx.set_pcs_config(None)
    t = _table(3000, 6)
    kw = dict(where=[(0, "!=", 1)], order_by=(3, (1, "desc")), columns=[2, (4, 1), 5], rows=(0, 2999), log_size=12)
    outside = _check(pkg, ctx, t, **kw)
    with pkg.Channel(STWO) as ch, pkg.PcsSession(ctx) as s:
        before = ctx.memory()["arena_in_use"]
        inside = _check(pkg, ctx, t, **kw)
        assert ctx.memory()["arena_in_use"] == before
        assert (inside.rows == outside.rows).all() and (inside.order == outside.order).all()
        with ctx.rows_select(np.asarray(t), **kw) as cols:
            assert ctx.memory()["arena_in_use"] == before
            assert len(s.commit(ch, cols.ptrs, [12] * 3, form=0)) == 32


def test_second_call_of_a_shape_allocates_nothing_with_a_scratch_reserve(pkg):
    t = _table(3000, 6)
    kw = dict(where=[(0, "!=", 1)], order_by=(3, (1, "desc"), 0), columns=[2, (4, 1), 5], rows=(0, 2999), log_size=12)
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
    Out, Desc, Table, Term, Key = pkg.SelectOut, pkg.RowsSelectDesc, pkg.RowsTable, pkg.SelectTerm, pkg.SelectKey
    with Dev(ctx) as dev:
        rows_d = dev.up(np.concatenate([t.ravel(), np.zeros(8, dtype=np.uint32)]))
        big = dev.filled(3 * n)
        order_d = dev.filled(16)
        col_ptrs = [dev.up(t[:, c]) for c in range(4)]
        cols_h = (ctypes.c_void_p * 4)(*col_ptrs)
        outs = (Out * 2)(Out(0, 0, 0), Out(1, 0, 0))
        n_sel = ctypes.c_uint64(77)

        def table(layout=0, n_cols=4, rows=rows_d, cols=None, n_rows=10, stride=4, flags=0, reserved=0):
            return Table(layout, n_cols, ctypes.cast(rows, ctypes.POINTER(ctypes.c_uint32)), cols, n_rows, stride, flags, reserved)

        def desc(begin=0, end=10, reserved=(0, 0), terms=(), keys=(), n_terms=None, n_keys=None):
            ta, ka = (Term * max(1, len(terms)))(*terms), (Key * max(1, len(keys)))(*keys)
            d = Desc(ctypes.cast(ta, ctypes.c_void_p) if terms else None, ctypes.cast(ka, ctypes.c_void_p) if keys else None, len(terms) if n_terms is None else n_terms,
                     len(keys) if n_keys is None else n_keys, begin, end, (ctypes.c_uint32 * 2)(*reserved))
            d._keep = (ta, ka)
            return d

        def call(tab, sel, log_size=4, outs_=outs, out_ptrs=(big, big + 4 * n), n_out=2, order=None, ns=n_sel, handle=ctx._h):
            ptrs = None if out_ptrs is None else (ctypes.c_void_p * max(1, len(out_ptrs)))(*out_ptrs)
            rc = L.bfhip_rows_select(handle, None if tab is None else ctypes.byref(tab), None if sel is None else ctypes.byref(sel), ctypes.c_uint32(log_size), outs_, ptrs,
                                     ctypes.c_uint32(n_out), ctypes.c_void_p(order), None if ns is None else ctypes.byref(ns))
            return rc, L.bfhip_last_error().decode() if rc else ""

        col_major = table(layout=1, rows=None, cols=ctypes.cast(cols_h, ctypes.POINTER(ctypes.c_void_p)))
        holed = (ctypes.c_void_p * 4)(col_ptrs[0], None, col_ptrs[2], col_ptrs[3])
        refusals = [
            ((None, desc()), {}, "null argument"), ((table(), None), {}, "null argument"), ((table(), desc()), dict(ns=None), "null argument"),
            ((table(), desc()), dict(outs_=None), "null argument"),
            ((table(reserved=1), desc()), {}, "reserved must be 0"), ((table(layout=2), desc()), {}, "unknown layout 2"), ((table(flags=2), desc()), {}, "unknown flag bits 2"),
            ((table(stride=3), desc()), {}, "row_stride 3 is below n_cols 4"), ((table(n_cols=0, stride=0), desc()), {}, "the table has no columns"),
            ((table(rows=None), desc()), {}, "null table pointer"), ((table(layout=1, rows=None), desc()), {}, "null table pointer"),
            ((table(layout=1, rows=None, cols=ctypes.cast(holed, ctypes.POINTER(ctypes.c_void_p))), desc()), {}, "source column 1 is a null pointer"),
            ((table(), desc()), dict(log_size=0), "log_size 0 is outside 1..30"), ((table(), desc()), dict(n_out=0), "n_out 0 is outside 1..256 (BFHIP_AIR_MAX_COLUMNS)"),
            ((table(), desc()), dict(out_ptrs=None), "the count-only form takes null outputs, n_out 0 and log_size 0 together"),
            ((table(), desc()), dict(out_ptrs=None, n_out=0), "the count-only form takes null outputs, n_out 0 and log_size 0 together"),
            ((table(), desc()), dict(out_ptrs=(big, None)), "output column 1 is a null pointer"),
            ((table(), desc()), dict(outs_=(Out * 2)(Out(0, 0, 0), Out(1, 0, P))), "output 1: pad value 2147483647 is not a canonical M31 value"),
            ((table(), desc()), dict(outs_=(Out * 2)(Out(0, 0, 0), Out(4, 0, 0))), "output 1: column index 4 is not below n_cols 4"),
            ((table(), desc()), dict(outs_=(Out * 2)(Out(0, 1, 0), Out(1, 0, 0))), "output 0: offset 1 reads behind the table's 10 rows from row_end 10"),
            ((table(), desc(reserved=(0, 3))), {}, "reserved must be 0"), ((table(), desc(begin=3, end=2)), {}, "row_begin 3 is above row_end 2"),
            ((table(), desc(end=11)), {}, "row_end 11 exceeds n_rows 10"),
            ((table(), desc()), dict(out_ptrs=(big, big + 4 * n - 4)), "output column 1 overlaps output column 0"),
            ((table(), desc()), dict(out_ptrs=(big, rows_d + 4 * 39)), "output column 1 overlaps the source table"),
            ((col_major, desc()), dict(out_ptrs=(big, col_ptrs[2] + 36)), "output column 1 overlaps source column 2"),
            ((table(), desc()), dict(order=big + 4 * n + 36), "output column 1 overlaps the order"),
            ((table(), desc()), dict(order=rows_d), "the order overlaps the source table"),
            # the rules of the shared validator (csrc/rows_select.h), through the device entry point
            ((table(), desc(terms=[Term(0, 0, 0)] * 9)), {}, "n_terms 9 exceeds 8 (BFHIP_SELECT_MAX_TERMS)"),
            ((table(), desc(keys=[Key(0, 0)] * 5)), {}, "n_keys 5 exceeds 4 (BFHIP_SELECT_MAX_KEYS)"),
            ((table(), desc(n_terms=1)), {}, "n_terms 1 with a null terms array"), ((table(), desc(n_keys=2)), {}, "n_keys 2 with a null keys array"),
            ((table(), desc(terms=[Term(0, 5, 0), Term(1, 6, 0)])), {}, "term 1: unknown op 6"),
            ((table(), desc(terms=[Term(0, 0, P)])), {}, "term 0: value 2147483647 is not a canonical M31 value"),
            ((table(), desc(terms=[Term(4, 0, 0)])), {}, "term 0: column index 4 is not below n_cols 4"),
            ((table(), desc(keys=[Key(0, 1), Key(1, 2)])), {}, "key 1: unknown flag bits 2"),
            ((col_major, desc(keys=[Key(7, 0)])), {}, "key 0: column index 7 is not below n_cols 4"),
            ((table(n_rows=1 << 31), desc(end=(1 << 30) + 1)), {}, "1073741825 candidate rows exceed 2^30"),
            ((table(n_rows=1 << 33), desc(begin=1 << 32, end=(1 << 32) + 1)), dict(order=order_d), "the order holds 32-bit rows: row_end 4294967297 exceeds 2^32"),
            ((table(n_rows=(1 << 40) + 1), desc()), {}, "n_rows 1099511627777 exceeds 2^40"),
            ((table(), desc(end=10)), dict(log_size=3), "10 rows selected, the domain has 8"),
        ]
        for (tab, sel), kw, rule in refusals:
            assert call(tab, sel, **kw) == (-1, WHO + rule), rule
            assert (ctx.download(big, 3 * n) == FILL).all() and (ctx.download(order_d, 16) == FILL).all(), rule
        assert call(table(), desc(), handle=None) == (-1, "null context")
        # a context in a shard group
        group, member = pkg.LocalGroup(2), pkg.Context(0, max_log_domain=10)
        try:
            member.join_local_group(group, 0)
            for tab in (table(), col_major):
                assert call(tab, desc(), order=order_d, handle=member._h) == (-1, WHO + "a context in a shard group is not supported (bfhip_ctx_leave_group first)")
                assert (ctx.download(big, 3 * n) == FILL).all() and (ctx.download(order_d, 16) == FILL).all()
            member.leave_group()
            assert call(table(), desc(begin=1, end=9), handle=member._h) == (0, "") and n_sel.value == 8      # and works once it has left
        finally:
            member.close(); group.close()
        # the good call on the same context, both layouts; the order beside the last output column
        for tab in (table(), col_major):
            assert call(tab, desc(begin=1, end=9), order=order_d) == (0, "") and n_sel.value == 8
            got = ctx.download(big, 3 * n).reshape(3, n)
            want = model.storage(np.concatenate([t[1:9, :2], np.zeros((8, 2), dtype=np.uint32)]), 4)
            assert (got[:2] == want).all() and (got[2] == FILL).all()
            assert (ctx.download(order_d, 16) == np.concatenate([np.arange(1, 9), np.full(8, FILL)])).all()


@pytest.mark.parametrize("program,inp", [("hello_kakarot.bf", b""), ("collatz.bf", bytes([55, 10]))])
def test_brainfuck_example_on_a_real_trace(_ctx, pkg, program, inp):
    """The sub-table and (mp, clk) selections of brainfuck_rows_select, run on the device over a real register trace, equal
    bfhip_host_table. bfhip_air_check of the component's brainfuck_air_program is NOT run on the result: that program holds the component's
    logUp constraint, which reads the interaction column over the whole padded domain, and its is_first and transition constraints take the
    dummy rows behind the real ones for granted (d = 1 with a continued clk — row-by-row work and, for Memory, inserted rows), so no
    statement about the real rows alone can be made with it. The real rows' transition constraints are stated here directly instead."""
    code = open(os.path.join(ROOT, "tests", "golden", "programs", program)).read()
    regs, words = pkg.host_run(code, inp)[1], pkg.host_compile(code)
    assert regs.shape[0] > 500
    with Dev(_ctx) as dev:
        src = pkg.DeviceRows(dev.up(regs), regs.shape[0], 7, 7)
        for name in ("plus_instruction", "left_instruction", "jump_if_zero", "jump_if_not_zero"):
            kw, names = pkg.brainfuck_rows_select(name, regs.shape[0])
            with _ctx.rows_select(src, want_order=True, **kw) as cols:
                got, S = _ctx.rows_from_columns(cols, cols.log_size), cols.n_selected
                cases.check_brainfuck_sub_table(pkg, regs, words, name, got, S)
                assert (got == pkg.rows_select_host(regs, **kw).rows).all() and (got[S:] == 0).all()
                assert (regs[cols.order, 2] == ord({"plus_instruction": "+", "left_instruction": "<", "jump_if_zero": "[", "jump_if_not_zero": "]"}[name])).all()
                real = {n_: got[:S, k].astype(np.int64) for k, n_ in enumerate(names)}
                if name == "plus_instruction":      # n_ip = ip + 1, n_mp = mp, n_mv = mv + 1 (mod p)
                    assert S and (real["next_ip"] == real["ip"] + 1).all() and (real["next_mp"] == real["mp"]).all() and (real["next_mv"] == (real["mv"] + 1) % P).all()
                elif name == "left_instruction":
                    assert (real["next_ip"] == real["ip"] + 1).all() and (real["next_mp"] == real["mp"] - 1).all()
                else:
                    assert (real["next_mp"] == real["mp"]).all() and (real["next_mv"] == real["mv"]).all()
        kw, _ = pkg.brainfuck_rows_select("memory", regs.shape[0])
        with _ctx.rows_select(src, **kw) as cols:
            got = _ctx.rows_from_columns(cols, cols.log_size)
            cases.check_brainfuck_memory(pkg, regs, words, got, cols.n_selected)
            assert (got == pkg.rows_select_host(regs, **kw).rows).all()
