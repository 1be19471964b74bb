"""Relation programs (include/bfhip.h "Relation programs") in plain Python with a Counter: the model bfhip_relation_program_eval_row and
bfhip_relation_program_summary are compared against. It shares no code with the product: the interpreter below copies a value when WORD names
it (the product keeps the register and reads it at the ENTRY; the validator makes the two the same thing), runs all rows of a table at once
on uint64 numpy arrays, and the summary is a Counter per relation. Column words are canonical (< p)."""
from collections import Counter, defaultdict

import numpy as np

P = (1 << 31) - 1
M_COL, M_CONST, M_ADD, M_SUB, M_MUL, M_NEG = range(6)
WORD, ENTRY = 17, 18


def run(code, columns):
    """code: flat u32 words; columns: one uint array per program column, all of one length (the value of the column at every evaluated row).
    Returns the entries in program order: [(relation, multiplicity array, [word arrays])], every array over the rows."""
    n = len(columns[0]) if len(columns) else 1
    m, pending, out = {}, [], []
    for i in range(0, len(code), 4):
        op, dst, a, b = (int(w) for w in code[i: i + 4])
        if op == M_COL:
            assert b == 0
            m[dst] = np.asarray(columns[a], dtype=np.uint64)
        elif op == M_CONST:
            m[dst] = np.full(n, a, dtype=np.uint64)
        elif op == M_ADD:
            m[dst] = (m[a] + m[b]) % P
        elif op == M_SUB:
            m[dst] = (m[a] + P - m[b]) % P
        elif op == M_MUL:
            m[dst] = (m[a] * m[b]) % P
        elif op == M_NEG:
            m[dst] = (P - m[a]) % P
        elif op == WORD:
            pending.append(m[a].copy())
        elif op == ENTRY:
            out.append((dst, m[a].copy(), pending))
            pending = []
        else:
            raise AssertionError("opcode %d is not a relation program's" % op)
    assert not pending
    return out


def eval_row(code, col_values):
    """One row: [(relation, multiplicity, tuple)] in program order, zero multiplicities included."""
    return [(rel, int(mult[0]), tuple(int(w[0]) for w in words)) for rel, mult, words in run(code, [np.array([v], dtype=np.uint64) for v in col_values])]


def table_rows(log_size, row_shift, columns, col_shifts=None):
    """The value of every column at every evaluated row: row r of 2^(log_size - row_shift) reads column k at (r << row_shift) >> s_k."""
    r = np.arange(1 << (log_size - row_shift), dtype=np.uint64)
    shifts = [row_shift] * len(columns) if col_shifts is None else col_shifts
    out = []
    for col, s in zip(columns, shifts):
        col = np.asarray(col, dtype=np.uint64)
        assert len(col) == 1 << (log_size - s)
        out.append(col[((r << np.uint64(row_shift)) >> np.uint64(s)).astype(np.int64)])
    return out


def summary(tables, relation_words):
    """tables: [(code, log_size, row_shift, columns, col_shifts or None)]. Per relation {"n_words", "n_entries", "n_tuples", "entries": the
    unbalanced tuples sorted, each {"tuple", "net", "n_yield", "n_use", "n_other", "first_yield", "first_use"}}, first_* = (table, row) or
    None — the shape of relation_model.relations."""
    per_table = [run(code, table_rows(log_size, row_shift, columns, shifts)) for code, log_size, row_shift, columns, shifts in tables]
    out = []
    for rel, n_words in enumerate(relation_words):
        net, kinds, first = Counter(), defaultdict(Counter), {}
        for t, entries in enumerate(per_table):
            mine = [(mult, words) for r, mult, words in entries if r == rel]
            if not mine:
                continue
            assert all(len(words) == n_words for _, words in mine)
            for row in range(len(mine[0][0])):
                for mult, words in mine:          # (table, row, program order)
                    num = int(mult[row])
                    if num == 0:
                        continue
                    tup = tuple(int(w[row]) for w in words)
                    kind = "n_yield" if num == 1 else "n_use" if num == P - 1 else "n_other"
                    net[tup] = (net[tup] + num) % P
                    kinds[tup][kind] += 1
                    first.setdefault((tup, kind), (t, row))
        entries = [{"tuple": tup, "net": net[tup], "n_yield": kinds[tup]["n_yield"], "n_use": kinds[tup]["n_use"], "n_other": kinds[tup]["n_other"],
                    "first_yield": first.get((tup, "n_yield")), "first_use": first.get((tup, "n_use"))} for tup in sorted(net) if net[tup]]
        out.append({"n_words": n_words, "n_entries": sum(sum(k.values()) for k in kinds.values()), "n_tuples": len(net), "entries": entries})
    return out
