"""What tests/test_rows_select_cpu.py and tests/test_gpu_rows_select.py share beside the model (tests/rows_select_model.py): bfhip_host_table of
one Brainfuck component, and the comparison of the worked example's selections (brainfuck_rows_select) with it."""
import ctypes

import numpy as np


def host_table(pkg, regs7, code_words, component):
    """bfhip_host_table of one component: (n_rows, n_cols) uint32, row-major."""
    L = pkg.lib()
    regs7 = np.ascontiguousarray(regs7, dtype=np.uint32)
    words = np.ascontiguousarray(code_words, dtype=np.uint32)
    nr, nc = ctypes.c_size_t(), ctypes.c_size_t()
    args = (regs7.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(regs7.shape[0]), words.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(words.size), component)
    assert L.bfhip_host_table(*args, None, ctypes.c_size_t(0), ctypes.byref(nr), ctypes.byref(nc)) == 0
    want = np.zeros((nr.value, nc.value), dtype=np.uint32)
    assert L.bfhip_host_table(*args, want.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(want.size), ctypes.byref(nr), ctypes.byref(nc)) == 0
    return want


# the sub-table components of the Brainfuck example: name -> (component index, is a jump table)
BF_SUB_TABLES = {"jump_if_not_zero": (4, True), "jump_if_zero": (5, True), "input_instruction": (6, False), "left_instruction": (7, False),
                 "minus_instruction": (8, False), "output_instruction": (9, False), "plus_instruction": (10, False), "right_instruction": (11, False)}


def check_brainfuck_sub_table(pkg, regs, code_words, name, got_rows, S):
    """The selection's S rows against the first S rows of the component's host table: clk .. mvi are columns 0..6 of both sub-table layouts
    and next_ip, next_mp, next_mv columns 8, 9, 10; every host row past S is a dummy (d = 1: column 7, or 11 of a jump table)."""
    component, jump = BF_SUB_TABLES[name]
    want = host_table(pkg, regs, code_words, component)
    d = want[:, 11 if jump else 7]
    assert S == int((d == 0).sum()) and (d[:S] == 0).all() and S <= want.shape[0]
    assert (np.asarray(got_rows)[:S] == want[:S][:, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10]]).all()
    return want


def check_brainfuck_memory(pkg, regs, code_words, got_rows, S):
    """The (mp, clk)-sorted selection against the Memory host table: its real entries (d = 0: column 3) in table order are exactly the sorted
    register rows — clk, mp, mv are columns 0, 1, 2. One entry per table row in this layout, so the last real entry is among them too."""
    want = host_table(pkg, regs, code_words, 0)
    real = want[want[:, 3] == 0][:, :3]
    assert S == regs.shape[0] == real.shape[0]
    assert (np.asarray(got_rows)[:S] == real).all()
