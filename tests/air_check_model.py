"""The reference of bfhip_air_check (include/bfhip.h "Constraint programs asserted on the trace domain") in numpy: the model of
tests/air_model.py run once per constraint with a one-hot coefficient over the trace domain itself (log_expand = 0, where offset_rows is a
move in coset order), reduced to the report's fields. tests/test_air_check_cpu.py anchors it to the CPU oracle's AssertEvaluator on the 13
Brainfuck programs; tests/test_gpu_air_check.py compares the kernel with it."""
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


def same(got, want):
    """got: AirCheckReport.as_dict(); want: report(). Every field, exactly."""
    return all(got[f] == want[f] for f in FIELDS)
