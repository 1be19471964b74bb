"""The reference of bfhip_air_check (include/bfhip.h "Constraint programs asserted on the trace domain") in numpy: the model of
tests/air_model.py run once per constraint with a one-hot coefficient over the trace domain itself (log_expand = 0, where offset_rows is a
move in coset order), reduced to the report's fields. tests/test_air_check_cpu.py anchors it to the CPU oracle's AssertEvaluator on the 13
Brainfuck programs; tests/test_gpu_air_check.py compares the kernel with it. one_pass() gives the same report from a single run (pinned to
report() in tests/test_air_check_cpu.py): what tests/air_check_cases.py and tests/test_gpu_air_check_edges.py use."""
import numpy as np

import air_model

ONE, ZERO = [1, 0, 0, 0], [0, 0, 0, 0]
FIELDS = ("log_size", "n_constraints", "n_bad_cells", "first_bad_cell", "first_bad_constraint", "first_bad_value", "bad_per_constraint", "first_cell_per_constraint")


def n_constraints_of(code):
    return sum(1 for i in range(0, len(code), 4) if code[i] in (air_model.C_BASE, air_model.C_EXT))


def report(code, cols, params, log_size):
    """cols: full-size columns (n_cols, 2^log_size) in storage order. The dict AirCheckReport.as_dict() gives, without "ok"."""
    n, k = 1 << log_size, n_constraints_of(code)
    read = air_model.domain_reader(np.asarray(cols), log_size, 0)
    values = [air_model.run(code, read, params, [ONE if i == j else ZERO for i in range(k)], n) for j in range(k)]
    bad = np.stack([v.any(axis=0) for v in values])          # (k, n)
    cells = np.nonzero(bad.any(axis=0))[0]
    out = {"log_size": log_size, "n_constraints": k, "n_bad_cells": int(len(cells)), "first_bad_cell": None, "first_bad_constraint": -1,
           "first_bad_value": [0, 0, 0, 0], "bad_per_constraint": [int(b.sum()) for b in bad],
           "first_cell_per_constraint": [int(np.argmax(b)) if b.any() else None for b in bad]}
    if len(cells):
        c = int(cells[0])
        j = int(np.argmax(bad[:, c]))
        out.update(first_bad_cell=c, first_bad_constraint=j, first_bad_value=[int(w) for w in values[j][:, c]])
    return out


def one_pass(code, cols, params, log_size):
    """(the report, bad) from ONE run of the interpreter (air_model.constraint_values hands out every constraint's value as the program
    reaches it) instead of report()'s run per constraint: what keeps 64 constraints and 2^20 cells cheap. bad: (k, n) bool, bad[j, c] =
    constraint j is non-zero at cell c — what the tests read the shape of a case from (counts per wave, lowest lanes). Only a constraint's
    value at its own first bad cell is kept: the first bad cell overall is the lowest of those, and its lowest failing constraint is the
    lowest j whose own first cell it is. tests/test_air_check_cpu.py pins it to report()."""
    n = 1 << log_size
    read = air_model.domain_reader(np.asarray(cols), log_size, 0)
    bad, firsts = [], []
    for _, value in air_model.constraint_values(code, read, params, n):
        b = value.any(axis=0)
        c = int(np.argmax(b)) if b.any() else None
        bad.append(b)
        firsts.append((c, None if c is None else [int(w) for w in value[:, c]]))
    bad, k = np.stack(bad), len(bad)
    out = {"log_size": log_size, "n_constraints": k, "n_bad_cells": int(np.count_nonzero(bad.any(axis=0))), "first_bad_cell": None,
           "first_bad_constraint": -1, "first_bad_value": [0, 0, 0, 0], "bad_per_constraint": [int(b.sum()) for b in bad],
           "first_cell_per_constraint": [c for c, _ in firsts]}
    failing = [(c, j) for j, (c, _) in enumerate(firsts) if c is not None]
    if failing:
        c, j = min(failing)
        out.update(first_bad_cell=c, first_bad_constraint=j, first_bad_value=firsts[j][1])
    return out, bad


def report_one_pass(code, cols, params, log_size):
    return one_pass(code, cols, params, log_size)[0]


def same(got, want):
    """got: AirCheckReport.as_dict(); want: report(). Every field, exactly."""
    return all(got[f] == want[f] for f in FIELDS)
