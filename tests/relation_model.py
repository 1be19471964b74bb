"""The three lookup relations of the Brainfuck AIRs over numpy tables, with a Counter: the model bfhip_relation_summary / bfhip_trace_relations
are compared against. Restates the `add_to_relation` calls of the reference and shares no code with the product:
memory/component.rs:62-137 (uses Memory, d - 1), instruction/component.rs:65-142 (uses Instruction, d - 1), program/component.rs:60-104
(yields Instruction, 1 - d), processor/component.rs:79-153 (yields Processor, Instruction, Memory, 1 - d), jump/jump_if_{not_,}zero_component.rs:61-130
and instructions/*_component.rs:62-122 (use Processor, d - 1), end_of_execution/component.rs:61-90 (uses Processor, -1)."""
from collections import Counter, defaultdict

P = (1 << 31) - 1
# component -> [(relation, word columns, d column or None = always -1, sign of (1 - d))]
PARTS = {0: [(0, (0, 1, 2), 3, -1)], 1: [(1, (0, 1, 2), 3, -1)], 2: [(1, (0, 1, 2), 3, +1)],
         3: [(0, (0, 4, 5), 7, +1), (1, (1, 2, 3), 7, +1), (2, tuple(range(7)), 7, +1)],
         4: [(2, tuple(range(7)), 11, -1)], 5: [(2, tuple(range(7)), 11, -1)], 12: [(2, tuple(range(7)), None, -1)]}
PARTS.update({k: [(2, tuple(range(7)), 7, -1)] for k in range(6, 12)})


def relations(tables):
    """tables: [(component, (n_main, n_rows) array)]. Returns per relation {"n_entries", "n_tuples", "entries": the unbalanced tuples sorted,
    each {"tuple", "net", "n_yield", "n_use", "n_other", "first_yield", "first_use"} with first_* = (table index, row) or None}."""
    out = []
    for rel in range(3):
        net, kinds, first = Counter(), defaultdict(Counter), {}
        for t, (comp, cols) in enumerate(tables):
            for r, words, d, sign in PARTS[comp]:
                if r != rel:
                    continue
                for row in range(cols.shape[1]):
                    num = (P - 1) if d is None else sign * (1 - int(cols[d, row])) % P
                    if num == 0:
                        continue
                    tup = tuple(int(cols[w, row]) for w in words)
                    kind = "n_yield" if num == 1 else "n_use" if num == P - 1 else "n_other"
                    net[tup] = (net[tup] + num) % P
                    kinds[tup][kind] += 1
                    first.setdefault((tup, kind), (t, row))          # tables and rows are visited in ascending order
        entries = [{"tuple": tup, "net": net[tup], "n_yield": kinds[tup]["n_yield"], "n_use": kinds[tup]["n_use"], "n_other": kinds[tup]["n_other"],
                    "first_yield": first.get((tup, "n_yield")), "first_use": first.get((tup, "n_use"))} for tup in sorted(net) if net[tup]]
        out.append({"n_entries": sum(sum(k.values()) for k in kinds.values()), "n_tuples": len(net), "entries": entries})
    return out
