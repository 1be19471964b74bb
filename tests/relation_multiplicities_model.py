"""bfhip_relation_program_multiplicities (include/bfhip.h "Lookup multiplicities") in plain Python with Counters: the model the device result
is compared against, word for word and count for count. Built on relation_program_model.run and table_rows; it shares no code with the
product. The target is the `target_entry`-th ENTRY of `relation`, in program order, of table `target_table`: its tuple at every row, its
multiplicity operand ignored. Every other entry of the relation with a non-zero multiplicity counts."""
from collections import Counter, defaultdict

import numpy as np

from relation_program_model import P, run, table_rows


def multiplicities(tables, relation, target_table, target_entry):
    """tables: [(code, log_size, row_shift, columns, col_shifts or None)]. Returns (out, report, missing): out = the column as a uint32 array,
    one word per evaluated row of the target table; report = {"n_rows", "n_row_tuples", "n_entries", "n_tuples", "n_filled", "n_missing"};
    missing = the tuples with net != 0 that no target row holds, sorted, each {"tuple", "net", "n_yield", "n_use", "n_other", "first_yield",
    "first_use"} over the other entries — the shape of relation_program_model.summary's entries."""
    net, kinds, first = Counter(), defaultdict(Counter), {}
    lowest = {}          # tuple -> lowest target row holding it
    n_rows = None
    for t, (code, log_size, row_shift, columns, shifts) in enumerate(tables):
        mine = [(mult.tolist(), [w.tolist() for w in words]) for r, mult, words in run(code, table_rows(log_size, row_shift, columns, shifts)) if r == relation]
        if t == target_table:
            assert target_entry < len(mine)
            n_rows = 1 << (log_size - row_shift)
        for row in range(1 << (log_size - row_shift)):
            for ordinal, (mult, words) in enumerate(mine):          # (table, row, program order)
                tup = tuple(w[row] for w in words)
                if t == target_table and ordinal == target_entry:
                    lowest.setdefault(tup, row)
                    continue
                num = mult[row]
                if num == 0:
                    continue
                kind = "n_yield" if num == 1 else "n_use" if num == P - 1 else "n_other"
                net[tup] = (net[tup] + num) % P
                kinds[tup][kind] += 1
                first.setdefault((tup, kind), (t, row))
    assert n_rows is not None
    out = np.zeros(n_rows, dtype=np.uint32)
    for tup, row in lowest.items():
        out[row] = net.get(tup, 0)
    missing = [{"tuple": tup, "net": net[tup], "n_yield": kinds[tup]["n_yield"], "n_use": kinds[tup]["n_use"], "n_other": kinds[tup]["n_other"],
                "first_yield": first.get((tup, "n_yield")), "first_use": first.get((tup, "n_use"))} for tup in sorted(net) if net[tup] and tup not in lowest]
    report = {"n_rows": n_rows, "n_row_tuples": len(lowest), "n_entries": sum(sum(k.values()) for k in kinds.values()), "n_tuples": len(net),
              "n_filled": int(np.count_nonzero(out)), "n_missing": len(missing)}
    return out, report, missing
