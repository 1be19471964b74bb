"""No GPU: the numpy reference of tests/relation_model_np.py pinned field for field to the two Counter models it stands in for at sizes they are
too slow for (tests/test_gpu_relation_scale.py) — on the tables of two GPU tests and on one random case per model with multiplicities from
{1, p - 1, 2, p - 2}."""
import numpy as np
import pytest

import relation_model
import relation_model_np
import relation_program_model
from conftest import P, splitmix_column
from test_gpu_relation_program import one_entry_program, three_table_specs
from test_gpu_relations import opcode_table, processor_table, sort_order_tables

FIELDS = ("n_words", "n_entries", "n_tuples", "entries")
MULTS = np.array([1, P - 1, 2, P - 2], dtype=np.uint32)


def assert_pinned(got, want):
    """Every field of the Counter model's result, and the segments the numpy reference adds: they tile [0, n_entries) in order, and the
    unbalanced ranks are those of the listed tuples among all tuples."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        print({k: g[k] for k in FIELDS if k in g and k != "entries"}, len(g["entries"]), g["entries"][:4])
        assert {k: g[k] for k in w} == w
        start, end = g["start"], g["end"]
        assert len(start) == len(end) == g["n_tuples"] and len(g["unbalanced"]) == len(g["entries"])
        if g["n_tuples"]:
            assert start[0] == 0 and end[-1] == g["n_entries"] and (start[1:] == end[:-1]).all() and (end > start).all()
            assert [int(end[s] - start[s]) for s in g["unbalanced"]] == [e["n_yield"] + e["n_use"] + e["n_other"] for e in g["entries"]]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_compiled_path_on_the_sort_order_tables(seed):
    tables = sort_order_tables(seed)
    want = relation_model.relations(tables)
    assert want[2]["n_tuples"] > len(want[2]["entries"]) > 0
    assert_pinned(relation_model_np.relations(tables), want)


def test_program_path_on_the_three_table_case(pkg):
    widths, specs = three_table_specs(pkg)
    tables = [(prog.code, log, rs, cols, shifts) for prog, log, rs, cols, shifts in specs]
    want = relation_program_model.summary(tables, widths)
    assert [w["n_entries"] > 0 for w in want] == [True, False, True, False]
    assert_pinned(relation_model_np.summary(tables, widths), want)


def test_compiled_path_on_random_tables():
    """About 5 000 entries: a Processor table (d from {0, 2, p - 1, 3}: numerators 1, p - 1, 2, p - 2 — relation_model takes 1 - d), two opcode
    tables and a Memory table over a few hundred distinct tuples, plus dummy rows (d = 1)."""
    def words(seed, rows, k):
        return np.stack([splitmix_column(seed + j, rows) % np.uint32(3 + j) for j in range(k)])

    def d_column(seed, rows, sign):      # numerator sign * (1 - d) drawn from MULTS, one row in nine a dummy
        num = MULTS[splitmix_column(seed, rows) % np.uint32(4)].astype(np.int64)
        d = (1 - sign * num) % P
        d[splitmix_column(seed + 1, rows) % np.uint32(9) == 0] = 1
        return d.astype(np.uint32)

    proc = np.zeros((9, 2048), dtype=np.uint32)
    proc[:7], proc[7] = words(10, 2048, 7), d_column(20, 2048, +1)
    jnz = np.zeros((13, 512), dtype=np.uint32)
    jnz[:7], jnz[11] = words(10, 512, 7), d_column(30, 512, -1)
    right = np.zeros((11, 1024), dtype=np.uint32)
    right[:7], right[7] = words(10, 1024, 7)[:, ::-1], d_column(40, 1024, -1)
    mem = np.zeros((8, 1024), dtype=np.uint32)
    mem[:3], mem[3] = words(10, 1024, 7)[[0, 4, 5]], d_column(50, 1024, -1)
    eoe = words(10, 4, 7)
    tables = [(4, jnz), (3, proc), (0, mem), (11, right), (12, eoe)]
    want = relation_model.relations(tables)
    assert sum(w["n_entries"] for w in want) > 5000 and all(0 < len(w["entries"]) < w["n_tuples"] for w in want)
    assert any(e["n_other"] and e["n_yield"] and e["n_use"] for e in want[2]["entries"])
    assert_pinned(relation_model_np.relations(tables), want)


def test_program_path_on_random_tables(pkg):
    """About 5 000 entries of a 3-word relation from two tables, the first with two entries per row; some multiplicities are zero."""
    widths = [3, 1]
    two, one = one_entry_program(pkg, widths, 0, n_entries=2), one_entry_program(pkg, widths, 0)
    draw = lambda seed, n, k: splitmix_column(seed, n) % np.uint32(k)

    def mult(seed, n):
        m = MULTS[draw(seed, n, 4)].copy()
        m[draw(seed + 1, n, 11) == 0] = 0
        return m

    tables = [(two.code, 11, 0, [draw(1, 2048, 5), draw(2, 2048, 7), draw(3, 2048, 3), mult(4, 2048), draw(6, 2048, 7), draw(7, 2048, 5), draw(8, 2048, 3), mult(9, 2048)], None),
              (one.code, 10, 0, [draw(11, 1024, 5), draw(12, 1024, 7), draw(13, 1024, 3), mult(14, 1024)], None)]
    want = relation_program_model.summary(tables, widths)
    assert 4500 < want[0]["n_entries"] < 5120 and 0 < len(want[0]["entries"]) < want[0]["n_tuples"] and want[1]["n_entries"] == 0
    assert any(e["n_other"] and e["n_yield"] and e["n_use"] for e in want[0]["entries"])
    assert_pinned(relation_model_np.summary(tables, widths), want)
