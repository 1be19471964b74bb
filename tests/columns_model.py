"""The numpy model of bfhip_columns_from_rows / bfhip_rows_from_columns (include/bfhip.h "Row order"): the map, the padding and the
column map, restated from the header's normative text and from nothing in the library."""
import numpy as np

P = (1 << 31) - 1


def bit_reverse(x, bits):
    x = np.asarray(x, dtype=np.uint64)
    r = np.zeros_like(x)
    for k in range(bits):
        r |= ((x >> np.uint64(k)) & np.uint64(1)) << np.uint64(bits - 1 - k)
    return r.astype(np.int64)


def rows_of_cells(log_size):
    """rows[s] = the row (coset index) that cell s holds: d = bit_reverse(s); 2 d if d < n / 2, else 2 (n - 1 - d) + 1."""
    n = 1 << log_size
    d = bit_reverse(np.arange(n), log_size)
    return np.where(d < n // 2, 2 * d, 2 * (n - 1 - d) + 1)


def cells_of_rows(log_size):
    rows = rows_of_cells(log_size)
    cells = np.empty_like(rows)
    cells[rows] = np.arange(len(rows))
    return cells


def columns_from_rows(table, log_size, columns=None, pad=None, repeat_last=False):
    """table: (n_rows, n_src) in row order -> (n_out, 2^log_size) in storage order."""
    table = np.asarray(table, dtype=np.uint32)
    n, (n_rows, n_src) = 1 << log_size, table.shape
    columns = list(range(n_src)) if columns is None else list(columns)
    pad = [0] * len(columns) if pad is None else list(pad)
    full = np.empty((n, len(columns)), dtype=np.uint32)
    full[:n_rows] = table[:, columns]
    full[n_rows:] = table[n_rows - 1, columns] if repeat_last else np.asarray(pad, dtype=np.uint32)
    return np.ascontiguousarray(full[rows_of_cells(log_size)].T)


def rows_from_columns(cols, log_size, n_rows):
    """(n_cols, 2^log_size) in storage order -> the first n_rows rows, (n_rows, n_cols)."""
    cols = np.asarray(cols, dtype=np.uint32)
    return np.ascontiguousarray(cols[:, cells_of_rows(log_size)[:n_rows]].T)
