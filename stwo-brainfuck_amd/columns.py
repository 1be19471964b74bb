"""Row order <-> storage order (include/bfhip.h "Row order"): the host map cell_of_row / row_of_cell, the two ways to name a device table
in row order (DeviceRows, DeviceRowColumns), and Columns — the handle that owns what Context.columns_from_rows wrote."""
import collections
import ctypes

import numpy as np

from ._abi import _check, _ptr_array, _u32s, abi, struct_fields
from ._abi_gen import (BFHIP_ROWS_COLUMN_MAJOR as ROWS_COLUMN_MAJOR, BFHIP_ROWS_REPEAT_LAST as ROWS_REPEAT_LAST, BFHIP_ROWS_ROW_MAJOR as ROWS_ROW_MAJOR)


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
