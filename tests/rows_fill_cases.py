"""What tests/test_rows_fill_cpu.py and tests/test_gpu_rows_fill.py share beside the model (tests/rows_fill_model.py): tables whose gaps lie
at chosen OUTPUT rows, and the three Brainfuck tables of the worked example (brainfuck_rows_fill) beside bfhip_host_table."""
import numpy as np

from rows_select_cases import host_table

P = (1 << 31) - 1
BF_TABLES = {"memory": 0, "instruction": 1, "processor": 3}      # name -> component index of bfhip_host_table
GROUP, STEP = 0, 1                                              # the group and step columns of stepped()


def stepped(n_entries, n_cols, gaps_at=(), group_len=None, seed=3, first_step=0):
    """A table of n_entries rows: column 0 the group word (it changes every group_len entries; None = one group), column 1 the step —
    it rises by 1 from entry to entry, and by 1 + length in front of the entry that sits behind each gap of gaps_at = [(first output
    row of the gap, length), ...] (ascending, not adjacent: an entry lies between two gaps) —, the other columns canonical random words."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, P, size=(n_entries, n_cols), dtype=np.uint32)
    t[:, GROUP] = 0 if group_len is None else np.arange(n_entries) // group_len
    delta = np.ones(n_entries, dtype=np.int64)
    inserted = 0
    for start, length in gaps_at:
        entry = start - inserted      # the entry that the gap precedes
        assert 1 <= entry < n_entries and (group_len is None or entry % group_len), (start, length)
        delta[entry] += length
        inserted += length
    t[:, STEP] = (first_step + np.cumsum(delta) - 1) % P
    return t


def brainfuck_table(pkg, regs, words, name, select_host, fill):
    """One table of the worked example: `select_host(src, **kw)` -> the order (host side), `fill(src, order, **kw)` -> the rows of the
    filled table in ROW order and T. Asserts equality with bfhip_host_table in every row and column; returns (T, n_entries)."""
    src = pkg.brainfuck_instruction_rows(words, regs) if name == "instruction" else regs
    select_kw, fill_kw, names = pkg.brainfuck_rows_fill(name, src.shape[0])
    order = None if select_kw is None else select_host(src, **select_kw)
    rows, T = fill(src, order, **fill_kw)
    want = host_table(pkg, regs, words, BF_TABLES[name])
    assert rows.shape == want.shape == (want.shape[0], len(names)) and (np.asarray(rows) == want).all(), name
    return T, src.shape[0]
