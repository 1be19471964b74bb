"""relation_aggregate's contract (csrc/relations.hip steps 2 to 5) on numpy arrays, for sizes where the Counter models of relation_model.py
and relation_program_model.py take seconds: sort the entries by tuple (np.lexsort), find the segment heads by comparing neighbours, take every
tuple's net from a uint64 cumulative sum (n p < 2^52 for n <= 2^21 entries: exact without a reduction on the way), its three counts and its
first yield / first use from reductions over the segment, and list the tuples with net != 0 in lexicographic order. It shares no code with
the product and nothing but P with the Counter models; tests/test_relation_model_np_cpu.py pins it to both of them field for field.

The front halves — which column is which word — are relation_program_model.run / table_rows for program tables (already vectorised) and
PARTS below for the 13 Brainfuck tables, a restatement of relation_model.PARTS as arrays."""
import numpy as np

import relation_program_model

P = (1 << 31) - 1
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
# component -> [(relation, word columns, d column or None = always -1, sign of (1 - d))]: relation_model.PARTS, written out
PARTS = {0: [(0, (0, 1, 2), 3, -1)], 1: [(1, (0, 1, 2), 3, -1)], 2: [(1, (0, 1, 2), 3, +1)],
         3: [(0, (0, 4, 5), 7, +1), (1, (1, 2, 3), 7, +1), (2, (0, 1, 2, 3, 4, 5, 6), 7, +1)],
         4: [(2, (0, 1, 2, 3, 4, 5, 6), 11, -1)], 5: [(2, (0, 1, 2, 3, 4, 5, 6), 11, -1)], 12: [(2, (0, 1, 2, 3, 4, 5, 6), None, -1)]}
for _k in range(6, 12):
    PARTS[_k] = [(2, (0, 1, 2, 3, 4, 5, 6), 7, -1)]


def aggregate(words, mult, table, row):
    """The entries of one relation in (table, row, program order): words = one array per tuple word, mult = canonical multiplicities (zeros
    are dropped here), table / row = where each entry comes from. Returns {"n_entries", "n_tuples", "entries": the unbalanced tuples in
    lexicographic order, each {"tuple", "net", "n_yield", "n_use", "n_other", "first_yield", "first_use"} with first_* = (table, row) or
    None, "start", "end": every tuple's [start, end) among the sorted entries, "mult": the multiplicities in sorted order, "unbalanced": the
    ranks of the unbalanced tuples}."""
    mult = np.asarray(mult, dtype=np.uint64)
    keep = np.flatnonzero(mult)
    mult = mult[keep]
    words = [np.asarray(w)[keep].astype(np.uint32) for w in words]
    origin = (np.asarray(table, dtype=np.uint64)[keep] << np.uint64(32)) | np.asarray(row, dtype=np.uint64)[keep]
    n = len(mult)
    empty = np.zeros(0, dtype=np.int64)
    if n == 0:
        return {"n_entries": 0, "n_tuples": 0, "entries": [], "start": empty, "end": empty, "mult": mult, "unbalanced": empty}
    assert n * P < 1 << 52 and int(mult.max()) < P
    order = np.lexsort([origin] + words[::-1])          # the last key is the most significant: word 0
    words, mult, origin = [w[order] for w in words], mult[order], origin[order]
    head = np.zeros(n, dtype=bool)
    head[0] = True
    for w in words:
        head[1:] |= w[1:] != w[:-1]
    start = np.flatnonzero(head)
    end = np.append(start[1:], n)
    run = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(mult, dtype=np.uint64)])
    net = (run[end] - run[start]) % np.uint64(P)
    is_yield, is_use = mult == 1, mult == P - 1
    n_yield = np.add.reduceat(is_yield.astype(np.int64), start)
    n_use = np.add.reduceat(is_use.astype(np.int64), start)
    n_other = (end - start) - n_yield - n_use
    first_yield = np.minimum.reduceat(np.where(is_yield, origin, NONE), start)
    first_use = np.minimum.reduceat(np.where(is_use, origin, NONE), start)
    at = lambda v: None if v == NONE else (int(v) >> 32, int(v) & 0xFFFFFFFF)
    unb = np.flatnonzero(net)
    entries = [{"tuple": tuple(int(w[start[s]]) for w in words), "net": int(net[s]), "n_yield": int(n_yield[s]), "n_use": int(n_use[s]), "n_other": int(n_other[s]),
                "first_yield": at(first_yield[s]), "first_use": at(first_use[s])} for s in unb]
    return {"n_entries": n, "n_tuples": len(start), "entries": entries, "start": start, "end": end, "mult": mult, "unbalanced": unb}


def _concat(parts, n_words):
    """parts: [(words, mult, table, row)] in table order"""
    if not parts:
        return aggregate([np.zeros(0)] * n_words, np.zeros(0), np.zeros(0), np.zeros(0))
    return aggregate([np.concatenate([p[0][k] for p in parts]) for k in range(n_words)], np.concatenate([p[1] for p in parts]),
                     np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts]))


def relations(tables):
    """relation_model.relations: tables = [(component, (n_main, n_rows) array)]; one aggregate() result per Brainfuck relation."""
    out = []
    for rel, n_words in enumerate((3, 3, 7)):
        parts = []
        for t, (comp, cols) in enumerate(tables):
            for r, wcols, d, sign in PARTS[comp]:
                if r != rel:
                    continue
                rows = cols.shape[1]
                if d is None:
                    num = np.full(rows, P - 1, dtype=np.uint64)
                else:
                    one_minus_d = (np.uint64(P + 1) - cols[d].astype(np.uint64) % np.uint64(P)) % np.uint64(P)
                    num = one_minus_d if sign > 0 else (np.uint64(P) - one_minus_d) % np.uint64(P)
                parts.append(([cols[w] for w in wcols], num, np.full(rows, t, dtype=np.uint64), np.arange(rows, dtype=np.uint64)))
        out.append(_concat(parts, n_words))
    return out


def summary(tables, relation_words):
    """relation_program_model.summary: tables = [(code, log_size, row_shift, columns, col_shifts or None)]; one aggregate() result per
    relation, with "n_words". A row's entries of one relation stand in program order."""
    per_table = [relation_program_model.run(code, relation_program_model.table_rows(log_size, row_shift, columns, shifts))
                 for code, log_size, row_shift, columns, shifts in tables]
    out = []
    for rel, n_words in enumerate(relation_words):
        parts = []
        for t, entries in enumerate(per_table):
            mine = [(mult, words) for r, mult, words in entries if r == rel]
            if not mine:
                continue
            rows, k = len(mine[0][0]), len(mine)
            assert all(len(words) == n_words for _, words in mine)
            flat = lambda arrs: np.stack(arrs, axis=1).reshape(rows * k)          # (row, program order)
            parts.append(([flat([words[j] for _, words in mine]) for j in range(n_words)], flat([mult for mult, _ in mine]),
                          np.full(rows * k, t, dtype=np.uint64), np.repeat(np.arange(rows, dtype=np.uint64), k)))
        out.append(dict(_concat(parts, n_words), n_words=n_words))
    return out
