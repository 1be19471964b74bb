"""ctypes view of tests/native/oracle_air_check.cpp: the CPU oracle's AssertEvaluator looped over EVERY cell of a caller-supplied table — the
full report bfhip_check_constraints / bfhip_trace_check return (counts per constraint, first bad cell, first failing constraint and value).
Built with g++ into a temporary directory by the `air_check` fixtures of tests/test_trace_check_cpu.py and tests/test_gpu_trace_check.py."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "oracle_air_check.cpp")
NO_CELL = (1 << 64) - 1
# what a report is compared on: every field of bfhip_check_report but component / log_size / reserved
FIELDS = ("n_bad_cells", "first_bad_cell", "first_bad_constraint", "first_bad_value", "bad_per_constraint", "claimed_sum")


def build(directory):
    path = os.path.join(str(directory), "liboracle_air_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-I", os.path.join(ROOT, "oracle"), "-o", path, SRC,
                           os.path.join(ROOT, "oracle", "simd_port.cpp"), "-lpthread"])
    return OracleAirCheck(path)


class OracleAirCheck:
    def __init__(self, path):
        self.L = ctypes.CDLL(path)
        self.L.oac_last_error.restype = ctypes.c_char_p

    def check(self, component, rows, elems24, inter=None, claimed=None):
        """rows: (n_main, n_rows) row-granular columns. inter: None = generated from rows, else (4 * n_logup, 16 * n_rows) full-size logUp
        columns (then `claimed` is required). Returns the report as a dict with the fields FIELDS; first_bad_cell is None without violations."""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        if inter is not None:
            inter = np.ascontiguousarray(inter, dtype=np.uint32)
            assert inter.shape == ((12 if component == 3 else 4), 16 * rows.shape[1]) and claimed is not None
        n_bad, first, con = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int(-1)
        val, per, cl = (ctypes.c_uint32 * 4)(), (ctypes.c_uint64 * 16)(), (ctypes.c_uint32 * 4)()
        rc = self.L.oac_check(component, p(rows), ctypes.c_size_t(rows.shape[1]), (ctypes.c_uint32 * 24)(*[int(v) for v in elems24]),
                              None if inter is None else p(inter), None if claimed is None else (ctypes.c_uint32 * 4)(*[int(v) for v in claimed]),
                              ctypes.byref(n_bad), ctypes.byref(first), ctypes.byref(con), val, per, cl)
        if rc != 0:
            raise RuntimeError(self.L.oac_last_error().decode())
        return {"n_bad_cells": n_bad.value, "first_bad_cell": None if first.value == NO_CELL else first.value, "first_bad_constraint": con.value,
                "first_bad_value": list(val), "bad_per_constraint": list(per), "claimed_sum": list(cl)}


def table_from_registers(oracle, trace, code, component):
    """(n_rows, n_main) table of one component built by the oracle from an explicit register trace and program words."""
    tr = np.ascontiguousarray(trace, dtype=np.uint32).reshape(-1, 7)
    cw = np.ascontiguousarray(code, dtype=np.uint32)
    nr, nc = ctypes.c_size_t(), ctypes.c_size_t()
    args = (tr.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(tr.shape[0]), cw.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cw.size), component)
    oracle._chk(oracle.L.orc_table_from_registers(*args, None, ctypes.c_size_t(0), ctypes.byref(nr), ctypes.byref(nc)))
    out = np.zeros((nr.value, nc.value), dtype=np.uint32)
    oracle._chk(oracle.L.orc_table_from_registers(*args, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.size), ctypes.byref(nr), ctypes.byref(nc)))
    return out


def same_report(got, want):
    """got: a product report (CheckReport.as_dict()); want: OracleAirCheck.check(). Every compared field, exactly."""
    return all(got[f] == want[f] for f in FIELDS)
