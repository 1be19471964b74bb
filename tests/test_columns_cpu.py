"""No GPU: the row-order map of include/bfhip.h "Row order" — bfhip_cell_of_row / bfhip_row_of_cell against the numpy model
(tests/columns_model.py) and the formula the GPU tests' own helper uses, the complement identity, the refusals; the shared index header
(csrc/rows_index.h: the map, the tile decomposition of the tiled kernels, 64-bit source offsets) walked by a stand-alone program under
AddressSanitizer + UBSan; and the new prototypes in the header, the Python mirror and the Rust FFI block. All comparisons are between integers."""
import os
import re
import subprocess

import numpy as np
import pytest

import air_model
import columns_model
from conftest import ROOT

NEW = ("bfhip_columns_from_rows", "bfhip_rows_from_columns", "bfhip_cell_of_row", "bfhip_row_of_cell")


def _helper_formula(log_size):
    """tests/test_gpu_air_program.py: _storage_of_coset_order's index, restated (that file is GPU-only)"""
    n = 1 << log_size
    d = air_model.bit_reverse(np.arange(n), log_size)
    return np.where(d < n // 2, 2 * d, 2 * (n - 1 - d) + 1)


@pytest.mark.parametrize("log_size", range(1, 17))
def test_cell_of_row_and_row_of_cell_are_inverse_bijections_and_the_model(pkg, log_size):
    n = 1 << log_size
    rows = np.array([pkg.row_of_cell(log_size, s) for s in range(n)])
    cells = np.array([pkg.cell_of_row(log_size, r) for r in range(n)])
    assert sorted(rows.tolist()) == list(range(n)) and sorted(cells.tolist()) == list(range(n))
    assert (cells[rows] == np.arange(n)).all() and (rows[cells] == np.arange(n)).all()
    assert (rows == columns_model.rows_of_cells(log_size)).all() and (cells == columns_model.cells_of_rows(log_size)).all()
    assert (rows == _helper_formula(log_size)).all()
    # the complement identity: with s = bit_reverse(d), row 2 d lives in cell s and row 2 d + 1 in cell ~s & (n - 1)
    d = np.arange(n // 2)
    s = columns_model.bit_reverse(d, log_size)
    assert (cells[2 * d] == s).all() and (cells[2 * d + 1] == (~s & (n - 1))).all()


def test_out_of_range_arguments_are_refused(pkg):
    for name, fn in (("bfhip_cell_of_row", pkg.cell_of_row), ("bfhip_row_of_cell", pkg.row_of_cell)):
        for log_size in (0, 31, 32):
            with pytest.raises(pkg.BfhipError) as e:
                fn(log_size, 0)
            assert str(e.value) == "%s: log_size %d is outside 1..30" % (name, log_size)
        for log_size, index in ((1, 2), (5, 32), (30, 1 << 30), (30, 1 << 40)):
            with pytest.raises(pkg.BfhipError) as e:
                fn(log_size, index)
            assert str(e.value) == "%s: index %d is not below 2^%d" % (name, index, log_size)
        assert fn(30, (1 << 30) - 1) < 1 << 30
        assert getattr(pkg.lib(), name)(4, 0, None) == -1
        assert pkg.lib().bfhip_last_error().decode() == name + ": null argument"


@pytest.mark.parametrize("sanitize", [False, True])
def test_index_header_walked_by_a_stand_alone_program(tmp_path, sanitize):
    """tests/native/rows_index_host.cpp (its own main) includes csrc/rows_index.h as plain C++: every cell of every tiled log_size up to 14 is
    produced exactly once with the model's row, and source offsets beyond 2^32 words are what 64-bit arithmetic gives. Run as a process."""
    exe = str(tmp_path / "rows_index_host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "native", "rows_index_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "rows_index_host ok" and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])


def _params(text):
    return [" ".join(p.split()) for p in text.split(",")]


def test_header_python_mirror_and_rust_agree_on_the_new_prototypes(pkg):
    import ctypes
    import sys
    gen = sys.modules[pkg.__name__ + "._abi_gen"]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bfhip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    width = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    for name in NEW:
        m = re.search(r"^int32_t %s\s*\((.*?)\)\s*;" % name, header, flags=re.S | re.M)
        assert m, name
        params = _params(m.group(1))
        restype, argtypes = gen.FUNCTIONS[name]
        assert restype is ctypes.c_int32 and len(argtypes) == len(params), name
        for p, t in zip(params, argtypes):
            ctype = p.rsplit(" ", 1)[0]
            assert t is (ctypes.c_void_p if "*" in p else width[ctype]), (name, p)
        r = re.search(r"pub fn %s\((.*?)\) -> i32;" % name, rust, flags=re.S)
        assert r, name + " is missing from bfhip_sys.rs"
        assert len(_params(r.group(1))) == len(params), name
        assert hasattr(pkg.lib(), name)
    # the by-value struct: 48 bytes in the header's stated layout, the same fields in the Rust block
    fields = gen.STRUCTS["bfhip_rows_table"]
    assert [f for f, _ in fields] == ["layout", "n_cols", "rows_d", "cols_h", "n_rows", "row_stride", "flags", "reserved"]
    assert ctypes.sizeof(pkg.RowsTable) == 48
    assert [getattr(pkg.RowsTable, f).offset for f, _ in fields] == [0, 4, 8, 16, 24, 32, 40, 44]
    body = re.search(r"pub struct BfhipRowsTable \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == [f for f, _ in fields]
    assert (gen.BFHIP_ROWS_ROW_MAJOR, gen.BFHIP_ROWS_COLUMN_MAJOR, gen.BFHIP_ROWS_REPEAT_LAST) == (0, 1, 1)
    for c in ("BFHIP_ROWS_ROW_MAJOR", "BFHIP_ROWS_COLUMN_MAJOR", "BFHIP_ROWS_REPEAT_LAST"):
        assert c in rust


def test_model_against_itself():
    """The model's two directions are inverse, padding and maps included (what the GPU tests compare with)."""
    rng = np.random.default_rng(5)
    for log_size, n_rows in ((1, 2), (4, 11), (9, 512), (10, 1000)):
        table = rng.integers(0, columns_model.P, size=(n_rows, 5), dtype=np.uint32)
        cols = columns_model.columns_from_rows(table, log_size, columns=[4, 0, 0], pad=[7, 0, columns_model.P - 1])
        assert cols.shape == (3, 1 << log_size)
        back = columns_model.rows_from_columns(cols, log_size, 1 << log_size)
        assert (back[:n_rows] == table[:, [4, 0, 0]]).all() and (back[n_rows:] == [7, 0, columns_model.P - 1]).all()
        rep = columns_model.rows_from_columns(columns_model.columns_from_rows(table, log_size, repeat_last=True), log_size, 1 << log_size)
        assert (rep[n_rows:] == table[-1]).all()
