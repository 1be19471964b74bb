"""The numpy model of bfhip_rows_select / bfhip_rows_select_host (include/bfhip.h "Row selection"), restated from the header's normative
text and from nothing in the library: a boolean mask, numpy.lexsort (stable), a gather at offsets, padding, and — for the storage-order
side — the cell placement of tests/columns_model.py."""
import numpy as np

import columns_model

P = (1 << 31) - 1
OPS = {"==": np.equal, "!=": np.not_equal, "<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal}


def split(entry):
    """col or (col, second) -> (col, second or None)"""
    return (int(entry), None) if isinstance(entry, (int, np.integer)) else (int(entry[0]), entry[1])


def select(table, log_size=None, where=(), order_by=(), columns=None, rows=None, pad=None, repeat_last=False):
    """table: (n_rows, n_cols) uint32 in row order. Returns (rows of the output in ROW order, (2^log_size, n_out) or None when log_size is
    None; S; the source rows of the selected rows, in order). The caller keeps the arguments inside what the library admits."""
    table = np.asarray(table, dtype=np.uint32)
    n_rows, n_cols = table.shape
    begin, end = (0, n_rows) if rows is None else rows
    cand = np.arange(begin, end, dtype=np.int64)
    mask = np.ones(len(cand), dtype=bool)
    for col, op, value in where:
        mask &= OPS[op](table[cand, col].astype(np.int64), int(value))
    order = cand[mask]
    if len(order_by) and len(order):
        keys = []
        for entry in order_by:
            col, how = split(entry)
            v = table[order, col].astype(np.int64)
            keys.append(P - 1 - v if how == "desc" else v)
        order = order[np.lexsort(keys[::-1])]      # lexsort: the LAST key is the primary one; stable
    S = len(order)
    if log_size is None:
        return None, S, order
    n = 1 << log_size
    assert S <= n
    outs = [split(c) for c in (range(n_cols) if columns is None else columns)]
    pad = [0] * len(outs) if pad is None else list(pad)
    out = np.empty((n, len(outs)), dtype=np.uint32)
    for k, (col, off) in enumerate(outs):
        out[:S, k] = table[order + (off or 0), col]
        out[S:, k] = out[S - 1, k] if repeat_last else pad[k]
    return out, S, order


def storage(rows_out, log_size):
    """The (n_out, 2^log_size) storage-order columns of an output in row order."""
    return np.ascontiguousarray(np.asarray(rows_out)[columns_model.rows_of_cells(log_size)].T)


def lowest_bad_word(table, where=(), order_by=(), columns=None, rows=None, repeat_last=False, log_size=None, sorts=True):
    """(row, col, value) of the lowest non-canonical word among the checked ones, or None: the term words of every candidate, the key words
    (where the sort runs) and the output words, offsets applied, of every selected row."""
    table = np.asarray(table, dtype=np.uint32)
    _, S, order = select(table, None, where, order_by if sorts else (), None, rows)
    begin, end = (0, table.shape[0]) if rows is None else rows
    seen = [(r, col) for r in range(begin, end) for col, _, _ in where]
    if sorts:
        seen += [(int(r), split(e)[0]) for r in order for e in order_by]
    if log_size is not None:
        outs = [split(c) for c in (range(table.shape[1]) if columns is None else columns)]
        seen += [(int(r) + (off or 0), col) for r in order for col, off in outs]
    bad = sorted((r, c) for r, c in seen if table[r, c] >= P)
    return (bad[0][0], bad[0][1], int(table[bad[0]])) if bad else None


def random_table(rng, n_rows, n_cols, small=4):
    """Columns alternate between few distinct values (ties for the sort, hits for the filter), the field's edges, and anything canonical."""
    t = rng.integers(0, P, size=(n_rows, n_cols), dtype=np.uint32)
    for c in range(n_cols):
        if c % 3 == 0:
            t[:, c] = rng.integers(0, small, size=n_rows)
        elif c % 3 == 1:
            t[:, c] = rng.choice(np.array([0, 1, P - 2, P - 1], dtype=np.uint32), size=n_rows)
    return t
