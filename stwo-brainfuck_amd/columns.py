"""Row order <-> storage order (include/bfhip.h "Row order"): the host map cell_of_row / row_of_cell, the two ways to name a device table
in row order (DeviceRows, DeviceRowColumns), and Columns — the handle that owns what Context.columns_from_rows wrote."""
import collections
import ctypes

import numpy as np

from ._abi import _check, _ptr_array, _u32s, abi, struct_fields
from ._abi_gen import (BFHIP_FILL_GAPS as FILL_GAPS, BFHIP_FILL_KEEP as FILL_KEEP, BFHIP_FILL_MARK as FILL_MARK, BFHIP_FILL_MAX_GROUP as FILL_MAX_GROUP,
                       BFHIP_FILL_MAX_OFFSET as FILL_MAX_OFFSET, BFHIP_FILL_NO_STEP as FILL_NO_STEP, BFHIP_FILL_SET as FILL_SET,
                       BFHIP_ROWS_COLUMN_MAJOR as ROWS_COLUMN_MAJOR, BFHIP_ROWS_REPEAT_LAST as ROWS_REPEAT_LAST, BFHIP_ROWS_ROW_MAJOR as ROWS_ROW_MAJOR,
                       BFHIP_SELECT_DESCENDING as SELECT_DESCENDING, BFHIP_SELECT_EQ, BFHIP_SELECT_GE, BFHIP_SELECT_GT, BFHIP_SELECT_LE, BFHIP_SELECT_LT,
                       BFHIP_SELECT_MAX_KEYS as SELECT_MAX_KEYS, BFHIP_SELECT_MAX_TERMS as SELECT_MAX_TERMS, BFHIP_SELECT_NE)


class RowsTable(ctypes.Structure):
    """include/bfhip.h `bfhip_rows_table`."""
    _fields_ = struct_fields("bfhip_rows_table")


# A row-major device table: word (r, c) at ptr[r * row_stride + c]; row_stride in words, None = n_cols
DeviceRows = collections.namedtuple("DeviceRows", "ptr n_rows n_cols row_stride", defaults=(None,))
# A column-major one: one device pointer per source column, each to n_rows words in row order
DeviceRowColumns = collections.namedtuple("DeviceRowColumns", "ptrs n_rows")


def cell_of_row(log_size, row):
    """bfhip_cell_of_row: the storage index of coset index `row` on CanonicCoset(log_size).circle_domain(), bit-reversed."""
    out = ctypes.c_uint64()
    _check(abi().bfhip_cell_of_row(int(log_size), int(row), ctypes.byref(out)))
    return out.value


def row_of_cell(log_size, cell):
    """bfhip_row_of_cell: its inverse — the row an author wrote for the cell that air_check or a logUp generation reports."""
    out = ctypes.c_uint64()
    _check(abi().bfhip_row_of_cell(int(log_size), int(cell), ctypes.byref(out)))
    return out.value


class Columns:
    """Storage-order device columns of 2^log_size words each: .ptrs is what every entry point that takes column pointers accepts (the object
    itself is a sequence of them). close() frees the columns it owns — those columns_from_rows allocated, not the caller's `out`."""

    def __init__(self, ctx, ptrs, log_size, owned):
        self._ctx, self.ptrs, self.log_size, self._owned = ctx, list(ptrs), log_size, list(owned)

    def __len__(self):
        return len(self.ptrs)

    def __getitem__(self, k):
        return self.ptrs[k]

    def __iter__(self):
        return iter(self.ptrs)

    def download(self):
        """The columns as a (n_cols, 2^log_size) uint32 array, storage order."""
        return np.stack([self._ctx.download(p, 1 << self.log_size) for p in self.ptrs])

    def close(self):
        owned, self._owned = self._owned, []
        for p in owned:
            self._ctx.free(p)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            if self._ctx._h:
                self.close()
        except Exception:
            pass


def _rows_table(table, repeat_last):
    """The bfhip_rows_table of a DeviceRows / DeviceRowColumns and what it points into."""
    flags = ROWS_REPEAT_LAST if repeat_last else 0
    if isinstance(table, DeviceRowColumns):
        arr = _ptr_array(list(table.ptrs))
        return RowsTable(ROWS_COLUMN_MAJOR, len(table.ptrs), None, ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)), int(table.n_rows), 0, flags, 0), arr
    if isinstance(table, DeviceRows):
        stride = table.n_cols if table.row_stride is None else table.row_stride
        return RowsTable(ROWS_ROW_MAJOR, int(table.n_cols), ctypes.cast(table.ptr, ctypes.POINTER(ctypes.c_uint32)), None, int(table.n_rows), int(stride), flags, 0), None
    raise TypeError("a table is a (n_rows, n_cols) uint32 array, a DeviceRows or a DeviceRowColumns")


def columns_from_rows(ctx, table, log_size, columns=None, pad=None, repeat_last=False, out=None):
    """Context.columns_from_rows (see there)."""
    tmp = None
    if isinstance(table, np.ndarray):
        if table.ndim != 2 or table.dtype != np.uint32:
            raise TypeError("a host table is a (n_rows, n_cols) uint32 array")
        host = np.ascontiguousarray(table)
        tmp = ctx.upload(host) if host.size else None
        table = DeviceRows(tmp, host.shape[0], host.shape[1], host.shape[1])
    try:
        desc, keep = _rows_table(table, repeat_last)
        n_out = len(columns) if columns is not None else len(out) if out is not None else desc.n_cols
        if out is not None and len(out) != n_out:
            raise ValueError("one output pointer per output column")
        if pad is not None and len(pad) != n_out:
            raise ValueError("one pad value per output column")
        owned = []
        try:
            ptrs = list(out) if out is not None else None
            if ptrs is None:
                for _ in range(n_out):
                    owned.append(ctx.malloc(4 << log_size))
                ptrs = owned
            _check(abi().bfhip_columns_from_rows(ctx._h, ctypes.byref(desc), int(log_size), None if columns is None else _u32s(columns),
                                                 None if pad is None else _u32s(pad), _ptr_array(ptrs), n_out))
        except Exception:
            for p in owned:
                ctx.free(p)
            raise
        del keep
        return Columns(ctx, ptrs, log_size, owned)
    finally:
        if tmp is not None:
            ctx.free(tmp)


def witness_program_generate(ctx, program, log_size, col_ptrs, args=(), out=None):
    """Context.witness_program_generate (see there)."""
    col_ptrs, args = list(col_ptrs), [int(a) for a in args]
    n_out = program.shape()["n_out"] if out is None else len(out)
    owned = []
    try:
        ptrs = list(out) if out is not None else None
        if ptrs is None:
            for _ in range(n_out):
                owned.append(ctx.malloc(4 << log_size))
            ptrs = owned
        _check(abi().bfhip_witness_program_generate(ctx._h, program._h, int(log_size), _ptr_array(col_ptrs) if col_ptrs else None,
                                                    _u32s(args) if args else None, len(args), _ptr_array(ptrs) if ptrs else None, n_out))
    except Exception:
        for p in owned:
            ctx.free(p)
        raise
    return Columns(ctx, ptrs, log_size, owned)


def rows_from_columns(ctx, col_ptrs, log_size, n_rows=None):
    """Context.rows_from_columns (see there)."""
    col_ptrs = list(col_ptrs)
    n_rows = (1 << log_size) if n_rows is None else int(n_rows)
    n_cols = len(col_ptrs)
    if n_rows == 0 or n_cols == 0:
        return np.zeros((n_rows, n_cols), dtype=np.uint32)
    dst = ctx.malloc(4 * n_rows * n_cols)
    try:
        _check(abi().bfhip_rows_from_columns(ctx._h, _ptr_array(col_ptrs), n_cols, int(log_size), dst, n_rows, n_cols, 0))
        return ctx.download(dst, n_rows * n_cols).reshape(n_rows, n_cols)
    finally:
        ctx.free(dst)


# ---- bfhip_rows_select (include/bfhip.h "Row selection") -------------------------------------------------------------------------------
SELECT_OPS = {"==": BFHIP_SELECT_EQ, "!=": BFHIP_SELECT_NE, "<": BFHIP_SELECT_LT, "<=": BFHIP_SELECT_LE, ">": BFHIP_SELECT_GT, ">=": BFHIP_SELECT_GE}


class SelectTerm(ctypes.Structure):
    """include/bfhip.h `bfhip_select_term`."""
    _fields_ = struct_fields("bfhip_select_term")


class SelectKey(ctypes.Structure):
    """include/bfhip.h `bfhip_select_key`."""
    _fields_ = struct_fields("bfhip_select_key")


class SelectOut(ctypes.Structure):
    """include/bfhip.h `bfhip_select_out`."""
    _fields_ = struct_fields("bfhip_select_out")


class RowsSelectDesc(ctypes.Structure):
    """include/bfhip.h `bfhip_rows_select_desc`."""
    _fields_ = struct_fields("bfhip_rows_select_desc")


# What rows_select_host returns: rows = (2^log_size, n_out) uint32 in ROW order (None in the count-only form), order = the source rows of the
# selected rows (None unless asked for)
SelectedRows = collections.namedtuple("SelectedRows", "rows n_selected order")


def _select_desc(where, order_by, rows, n_rows):
    """The bfhip_rows_select_desc of (where, order_by, rows) and the arrays it points into."""
    for _, op, _ in where:
        if isinstance(op, str) and op not in SELECT_OPS:
            raise ValueError('a where entry is (column, "==" | "!=" | "<" | "<=" | ">" | ">=", value)')
    terms = (SelectTerm * max(1, len(where)))(*[SelectTerm(int(c), SELECT_OPS[op] if isinstance(op, str) else int(op), int(v)) for c, op, v in where])
    keys = (SelectKey * max(1, len(order_by)))()
    for i, k in enumerate(order_by):
        col, how = (k, "asc") if isinstance(k, (int, np.integer)) else k
        if how not in ("asc", "desc"):
            raise ValueError('an order_by entry is a column or (column, "asc" | "desc")')
        keys[i] = SelectKey(int(col), SELECT_DESCENDING if how == "desc" else 0)
    begin, end = (0, n_rows) if rows is None else rows
    desc = RowsSelectDesc(ctypes.cast(terms, ctypes.c_void_p) if len(where) else None, ctypes.cast(keys, ctypes.c_void_p) if len(order_by) else None,
                          len(where), len(order_by), int(begin), int(end), (ctypes.c_uint32 * 2)(0, 0))
    return desc, (terms, keys)


def _select_outs(columns, pad, n_cols):
    columns = list(range(n_cols)) if columns is None else list(columns)
    if pad is not None and len(pad) != len(columns):
        raise ValueError("one pad value per output column")
    outs = (SelectOut * max(1, len(columns)))()
    for k, c in enumerate(columns):
        col, off = (c, 0) if isinstance(c, (int, np.integer)) else c
        outs[k] = SelectOut(int(col), int(off), 0 if pad is None else int(pad[k]))
    return outs, len(columns)


def _domain_for(n_selected):
    """The smallest log_size whose domain holds n_selected rows, at least 1."""
    return max(1, int(n_selected - 1).bit_length()) if n_selected > 1 else 1


def _as_device_table(ctx, table):
    """(table as DeviceRows / DeviceRowColumns, the temporary upload to free or None)."""
    if isinstance(table, np.ndarray):
        if table.ndim != 2 or table.dtype != np.uint32:
            raise TypeError("a host table is a (n_rows, n_cols) uint32 array")
        host = np.ascontiguousarray(table)
        tmp = ctx.upload(host) if host.size else None
        return DeviceRows(tmp, host.shape[0], host.shape[1], host.shape[1]), tmp
    return table, None


def rows_select_count(ctx, table, where=(), order_by=(), rows=None, want_order=False, order_out=None):
    """Context.rows_select_count (see there)."""
    table, tmp = _as_device_table(ctx, table)
    order_d = None
    try:
        tdesc, keep = _rows_table(table, False)
        sel, keep2 = _select_desc(list(where), list(order_by), rows, tdesc.n_rows)
        n_cand = max(0, sel.row_end - sel.row_begin)
        if want_order and order_out is None:
            order_d = ctx.malloc(4 * max(1, n_cand))
        n_sel = ctypes.c_uint64()
        _check(abi().bfhip_rows_select(ctx._h, ctypes.byref(tdesc), ctypes.byref(sel), 0, None, None, 0, order_d if order_out is None else order_out, ctypes.byref(n_sel)))
        del keep, keep2
        order = None
        if want_order and order_out is None:
            order = ctx.download(order_d, n_sel.value) if n_sel.value else np.zeros(0, dtype=np.uint32)
        return n_sel.value, order
    finally:
        if order_d is not None:
            ctx.free(order_d)
        if tmp is not None:
            ctx.free(tmp)


def rows_select(ctx, table, log_size=None, where=(), order_by=(), columns=None, rows=None, pad=None, repeat_last=False, out=None, want_order=False):
    """Context.rows_select (see there)."""
    table, tmp = _as_device_table(ctx, table)
    order_d, owned = None, []
    try:
        tdesc, keep = _rows_table(table, repeat_last)
        where, order_by = list(where), list(order_by)
        sel, keep2 = _select_desc(where, order_by, rows, tdesc.n_rows)
        outs, n_out = _select_outs(columns, pad, tdesc.n_cols)
        if out is not None and len(out) != n_out:
            raise ValueError("one output pointer per output column")
        if log_size is None:
            log_size = _domain_for(rows_select_count(ctx, table, where, (), rows)[0])
        n_cand = max(0, sel.row_end - sel.row_begin)
        if want_order:
            order_d = ctx.malloc(4 * max(1, n_cand))
        ptrs = list(out) if out is not None else None
        if ptrs is None:
            for _ in range(n_out):
                owned.append(ctx.malloc(4 << log_size))
            ptrs = owned
        n_sel = ctypes.c_uint64()
        _check(abi().bfhip_rows_select(ctx._h, ctypes.byref(tdesc), ctypes.byref(sel), int(log_size), outs, _ptr_array(ptrs) if ptrs else None, n_out, order_d,
                                       ctypes.byref(n_sel)))
        del keep, keep2
        order = None
        if want_order:
            order = ctx.download(order_d, n_sel.value) if n_sel.value else np.zeros(0, dtype=np.uint32)
        cols = Columns(ctx, ptrs, log_size, owned)      # from here on the handle owns the columns
        owned = []
        cols.n_selected, cols.order = n_sel.value, order
        return cols
    finally:
        for p in owned:
            ctx.free(p)
        if order_d is not None:
            ctx.free(order_d)
        if tmp is not None:
            ctx.free(tmp)


def rows_select_host(table, log_size=None, where=(), order_by=(), columns=None, rows=None, pad=None, repeat_last=False, want_order=False, n_cols=None,
                     count_only=False):
    """bfhip_rows_select_host: the definition of a selection, on the host and without a GPU. table: a (n_rows, row_stride) uint32 array of
    which the first n_cols words of a row are the table (None = all). The other arguments are rows_select's. Returns SelectedRows(rows,
    n_selected, order): rows in ROW order, (2^log_size, n_out). count_only: the count (and the order, if wanted) without rows; log_size
    None takes the smallest domain that holds the count, at least 1."""
    table = np.ascontiguousarray(table, dtype=np.uint32)
    if table.ndim != 2:
        raise TypeError("a host table is a (n_rows, row_stride) uint32 array")
    n_rows, stride = table.shape
    n_cols = stride if n_cols is None else int(n_cols)
    where, order_by = list(where), list(order_by)
    sel, keep = _select_desc(where, order_by, rows, n_rows)
    n_sel = ctypes.c_uint64()
    order = np.zeros(max(1, sel.row_end - sel.row_begin), dtype=np.uint32) if want_order else None
    data = table.ctypes.data if table.size else None

    def call(log, outs, n_out, rows_out):
        _check(abi().bfhip_rows_select_host(data, n_rows, n_cols, stride, int(bool(repeat_last)), ctypes.byref(sel), log, outs, n_out,
                                            None if rows_out is None else rows_out.ctypes.data, None if order is None else order.ctypes.data, ctypes.byref(n_sel)))
    if count_only or log_size is None:
        call(0, None, 0, None)
        if count_only:
            return SelectedRows(None, n_sel.value, None if order is None else order[:n_sel.value].copy())
        log_size = _domain_for(n_sel.value)
    outs, n_out = _select_outs(columns, pad, n_cols)
    rows_out = np.zeros((1 << log_size, n_out), dtype=np.uint32)
    call(int(log_size), outs, n_out, rows_out)
    del keep
    return SelectedRows(rows_out, n_sel.value, None if order is None else order[:n_sel.value].copy())


# ---- bfhip_rows_fill (include/bfhip.h "Row filling") ------------------------------------------------------------------------------------
FILL_KINDS = {"keep": FILL_KEEP, "set": FILL_SET, "mark": FILL_MARK}


class FillOut(ctypes.Structure):
    """include/bfhip.h `bfhip_fill_out`."""
    _fields_ = struct_fields("bfhip_fill_out")


class RowsFillDesc(ctypes.Structure):
    """include/bfhip.h `bfhip_rows_fill_desc`."""
    _fields_ = struct_fields("bfhip_rows_fill_desc")


# What rows_fill_host returns: rows = (2^log_size, n_out) uint32 in ROW order (None in the count-only form), n_filled = T
FilledRows = collections.namedtuple("FilledRows", "rows n_filled")


def _fill_outs(columns):
    """columns: ("keep", col[, offset]) | ("set", col, value[, offset]) | ("mark", value[, offset]) | a bare column (keep, offset 0)."""
    columns = list(columns)
    outs = (FillOut * max(1, len(columns)))()
    for k, c in enumerate(columns):
        if isinstance(c, (int, np.integer)):
            c = ("keep", c)
        kind, rest = c[0], [int(v) for v in c[1:]]
        want = {"keep": (1, 2), "set": (2, 3), "mark": (1, 2)}.get(kind)
        if want is None or len(rest) not in want:
            raise ValueError('an output is ("keep", col[, offset]), ("set", col, value[, offset]) or ("mark", value[, offset])')
        off = rest.pop() if len(rest) == want[1] else 0
        col, value = (0, rest[0]) if kind == "mark" else (rest[0], rest[1] if kind == "set" else 0)
        outs[k] = FillOut(col, FILL_KINDS[kind], value, off)
    return outs, len(columns)


def _fill_desc(group, step, gaps, order_ptr, n_entries, row_begin):
    """The bfhip_rows_fill_desc and the array it points into."""
    group = [int(g) for g in group]
    garr = _u32s(group) if group else None
    desc = RowsFillDesc(ctypes.cast(garr, ctypes.POINTER(ctypes.c_uint32)) if group else None, len(group), FILL_NO_STEP if step is None else int(step),
                        ctypes.cast(order_ptr, ctypes.POINTER(ctypes.c_uint32)) if order_ptr else None, int(n_entries), int(row_begin), FILL_GAPS if gaps else 0, 0)
    return desc, garr


def _fill_entries(order, n_order, rows, n_rows):
    """(n_entries, row_begin) of the (order, rows) arguments."""
    if order is not None:
        if rows is not None:
            raise ValueError("give an order or a row range, not both")
        return n_order, 0
    begin, end = (0, n_rows) if rows is None else rows
    return max(0, int(end) - int(begin)), int(begin)


def _fill_call(ctx, table, log_size, group, step, gaps, columns, order, n_order, rows, out):
    table, tmp = _as_device_table(ctx, table)
    order_tmp, owned = None, []
    try:
        tdesc, keep = _rows_table(table, False)
        if isinstance(order, np.ndarray):
            n_order = order.size
            if not order.size:
                raise ValueError("an order has at least one entry")
            order_tmp = order = ctx.upload(np.ascontiguousarray(order, dtype=np.uint32))
        elif order is not None and n_order is None:
            raise ValueError("a device order needs n_order, the number of entries")
        n_entries, row_begin = _fill_entries(order, n_order, rows, tdesc.n_rows)
        fill, keep2 = _fill_desc(group, step, gaps, order, n_entries, row_begin)
        n_filled = ctypes.c_uint64()
        if columns is None:
            _check(abi().bfhip_rows_fill(ctx._h, ctypes.byref(tdesc), ctypes.byref(fill), 0, None, None, 0, ctypes.byref(n_filled)))
            return n_filled.value
        outs, n_out = _fill_outs(columns)
        if out is not None and len(out) != n_out:
            raise ValueError("one output pointer per output column")
        if log_size is None:
            _check(abi().bfhip_rows_fill(ctx._h, ctypes.byref(tdesc), ctypes.byref(fill), 0, None, None, 0, ctypes.byref(n_filled)))
            log_size = _domain_for(n_filled.value)
        ptrs = list(out) if out is not None else None
        if ptrs is None:
            for _ in range(n_out):
                owned.append(ctx.malloc(4 << log_size))
            ptrs = owned
        _check(abi().bfhip_rows_fill(ctx._h, ctypes.byref(tdesc), ctypes.byref(fill), int(log_size), outs, _ptr_array(ptrs) if ptrs else None, n_out, ctypes.byref(n_filled)))
        del keep, keep2
        cols = Columns(ctx, ptrs, log_size, owned)      # from here on the handle owns the columns
        owned = []
        cols.n_filled = n_filled.value
        return cols
    finally:
        for p in owned:
            ctx.free(p)
        if order_tmp is not None:
            ctx.free(order_tmp)
        if tmp is not None:
            ctx.free(tmp)


def rows_fill(ctx, table, log_size=None, group=(), step=None, gaps=False, columns=None, order=None, n_order=None, rows=None, out=None):
    """Context.rows_fill (see there)."""
    if columns is None:
        raise ValueError("rows_fill needs its output columns (rows_fill_count is the count-only form)")
    return _fill_call(ctx, table, log_size, group, step, gaps, columns, order, n_order, rows, out)


def rows_fill_count(ctx, table, group=(), step=None, gaps=False, order=None, n_order=None, rows=None):
    """Context.rows_fill_count (see there)."""
    return _fill_call(ctx, table, None, group, step, gaps, None, order, n_order, rows, None)


def rows_fill_host(table, log_size=None, group=(), step=None, gaps=False, columns=None, order=None, rows=None, n_cols=None, count_only=False):
    """bfhip_rows_fill_host: the definition of a filled table, on the host and without a GPU. table: a (n_rows, row_stride) uint32 array of
    which the first n_cols words of a row are the table (None = all); order: None or a uint32 array of source rows. The other arguments are
    rows_fill's. Returns FilledRows(rows, n_filled): rows in ROW order, (2^log_size, n_out). count_only: the count without rows; log_size None
    takes the smallest domain that holds the count, at least 1."""
    table = np.ascontiguousarray(table, dtype=np.uint32)
    if table.ndim != 2:
        raise TypeError("a host table is a (n_rows, row_stride) uint32 array")
    n_rows, stride = table.shape
    n_cols = stride if n_cols is None else int(n_cols)
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.uint32)
    n_entries, row_begin = _fill_entries(order, None if order is None else order.size, rows, n_rows)
    fill, keep = _fill_desc(group, step, gaps, order.ctypes.data if order is not None and order.size else None, n_entries, row_begin)
    n_filled = ctypes.c_uint64()
    data = table.ctypes.data if table.size else None

    def call(log, outs, n_out, rows_out):
        _check(abi().bfhip_rows_fill_host(data, n_rows, n_cols, stride, ctypes.byref(fill), log, outs, n_out, None if rows_out is None else rows_out.ctypes.data,
                                          ctypes.byref(n_filled)))
    if count_only or log_size is None:
        call(0, None, 0, None)
        if count_only:
            return FilledRows(None, n_filled.value)
        log_size = _domain_for(n_filled.value)
    outs, n_out = _fill_outs(columns if columns is not None else range(n_cols))
    rows_out = np.zeros((1 << log_size, n_out), dtype=np.uint32)
    call(int(log_size), outs, n_out, rows_out)
    del keep
    return FilledRows(rows_out, n_filled.value)
