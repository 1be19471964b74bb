"""The numpy model of bfhip_rows_fill / bfhip_rows_fill_host (include/bfhip.h "Row filling"), restated from the header's normative text and
from nothing in the library: the repeat counts 1 + g_i, numpy.repeat for the entries with their inserted rows in front, the tail behind
them, the value rule per kind, and — for the storage-order side — the cell placement of tests/columns_model.py."""
import numpy as np

import columns_model

P = (1 << 31) - 1
MAX_OFFSET = 16


def entries(table, order=None, rows=None):
    """The source rows of the entries, in order."""
    if order is not None:
        return np.asarray(order, dtype=np.int64)
    begin, end = (0, np.asarray(table).shape[0]) if rows is None else rows
    return np.arange(begin, end, dtype=np.int64)


def gaps(table, src, group=(), step=None, use_gaps=False):
    """g_i per entry, as Python-exact int64: step(i) - step(prev) - 1 where positive and every group word agrees, else 0; g_0 = 0."""
    table = np.asarray(table, dtype=np.uint32)
    g = np.zeros(len(src), dtype=np.int64)
    if use_gaps and len(src) > 1:
        s = table[src, step].astype(np.int64)
        same = np.ones(len(src) - 1, dtype=bool)
        for c in group:
            same &= table[src[1:], c] == table[src[:-1], c]
        d = s[1:] - s[:-1] - 1
        g[1:] = np.where(same & (d > 0), d, 0)
    return g


def count(table, group=(), step=None, gaps_=False, order=None, rows=None):
    """T, exact."""
    src = entries(table, order, rows)
    return int(len(src)) + int(gaps(table, src, group, step, gaps_).sum())


def normalise(c):
    """An output as (kind, col, value, offset)."""
    if isinstance(c, (int, np.integer)):
        return "keep", int(c), 0, 0
    kind = c[0]
    if kind == "keep":
        return kind, int(c[1]), 0, int(c[2]) if len(c) > 2 else 0
    if kind == "set":
        return kind, int(c[1]), int(c[2]), int(c[3]) if len(c) > 3 else 0
    return kind, 0, int(c[1]), int(c[2]) if len(c) > 2 else 0


def fill(table, log_size, group=(), step=None, gaps_=False, columns=None, order=None, rows=None):
    """table: (n_rows, n_cols) uint32 in row order. Returns (the output in ROW order, (2^log_size, n_out); T). The caller keeps the
    arguments inside what the library admits (T <= 2^log_size)."""
    table = np.asarray(table, dtype=np.uint32)
    src = entries(table, order, rows)
    g = gaps(table, src, group, step, gaps_)
    T = len(src) + int(g.sum())
    n = 1 << log_size
    assert T <= n
    need = n + MAX_OFFSET
    # element -> (the entry whose words it shows, t): an entry's inserted rows show its predecessor, the tail shows the last entry
    shown = np.repeat(np.arange(len(src)), g + 1)
    first = np.cumsum(g + 1) - (g + 1)
    t = np.arange(T) - first[shown] + 1
    real = t == g[shown] + 1
    t = np.where(real, 0, t)
    shown = np.where(real, shown, shown - 1)
    shown = np.concatenate([shown, np.full(need - T, len(src) - 1)])
    t = np.concatenate([t, np.arange(1, need - T + 1)])
    outs = [normalise(c) for c in (range(table.shape[1]) if columns is None else columns)]
    out = np.empty((n, len(outs)), dtype=np.uint32)
    for k, (kind, col, value, off) in enumerate(outs):
        e_shown, e_t = shown[off:off + n], t[off:off + n]
        if kind == "mark":
            out[:, k] = np.where(e_t > 0, value, 0)
            continue
        w = table[src[e_shown], col].astype(np.int64)
        if kind == "set":
            out[:, k] = np.where(e_t > 0, value, w)
        else:
            out[:, k] = (w + e_t) % P if col == step else w
    return out, T


def storage(rows_out, log_size):
    """The (n_out, 2^log_size) storage-order columns of an output in row order (section 9q's cell placement)."""
    return np.ascontiguousarray(np.asarray(rows_out)[columns_model.rows_of_cells(log_size)].T)


def lowest_bad_word(table, log_size, group=(), step=None, gaps_=False, columns=None, order=None, rows=None):
    """(row, col, value) of the lowest non-canonical word among the checked ones, or None: with gaps the group and step words of every entry,
    and every source word an output reads (an inserted row of a set column and a mark column read nothing)."""
    table = np.asarray(table, dtype=np.uint32)
    src = entries(table, order, rows)
    seen = set()
    if gaps_:
        seen |= {(int(r), int(c)) for r in src for c in tuple(group) + (step,)}
    g = gaps(table, src, group, step, gaps_)
    T = len(src) + int(g.sum())
    n = 1 << log_size
    shown = np.repeat(np.arange(len(src)), g + 1)
    first = np.cumsum(g + 1) - (g + 1)
    t = np.arange(T) - first[shown] + 1
    real = t == g[shown] + 1
    t = np.where(real, 0, t)
    shown = np.where(real, shown, shown - 1)
    shown = np.concatenate([shown, np.full(n + MAX_OFFSET - T, len(src) - 1)])
    t = np.concatenate([t, np.arange(1, n + MAX_OFFSET - T + 1)])
    for kind, col, _, off in [normalise(c) for c in (range(table.shape[1]) if columns is None else columns)]:
        if kind == "mark":
            continue
        rows_read = src[shown[off:off + n]] if kind == "keep" else src[shown[off:off + n][t[off:off + n] == 0]]
        seen |= {(int(r), col) for r in np.unique(rows_read)}
    bad = sorted((r, c) for r, c in seen if table[r, c] >= P)
    return (bad[0][0], bad[0][1], int(table[bad[0]])) if bad else None
