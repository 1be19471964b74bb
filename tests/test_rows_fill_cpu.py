"""No GPU: bfhip_rows_fill_host (include/bfhip.h "Row filling") — the definition the kernels are held to — against the numpy model of
tests/rows_fill_model.py: no gaps, one gap, adjacent gaps, a gap of exactly 1, equal and descending steps, a group change, 0 to 4 group
columns, no step column, every kind, offsets 0, 1 and 16, a tail that wraps past p - 1, T = 2^log_size and one more, a total above 2^32
refused without a wrap, an order given and none, a row stride above n_cols, the count-only form; every refusal word for word; the lowest
(row, column) among several planted non-canonical words; a bad order word; the struct layouts of the generated ABI against the header's
comment; the Brainfuck example against bfhip_host_table; and the host code under AddressSanitizer + UBSan in a stand-alone program
(tests/native/rows_fill_host_sanitize.cpp). All comparisons are between integers."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rows_fill_cases as cases
import rows_fill_model as model
from conftest import ROOT
from rows_fill_cases import GROUP, STEP

P = model.P
WHO = "bfhip_rows_fill_host: "
PROGRAMS = os.path.join(ROOT, "tests", "golden", "programs")
GAPS = dict(group=(GROUP,), step=STEP, gaps=True)
ALL_KINDS = [("keep", STEP), ("keep", 2), ("set", 3, 7), ("mark", 1), ("keep", STEP, 1), ("set", 2, P - 1, 16), ("mark", 5, 16), ("keep", 3, 1), ("set", STEP, 0, 1)]


def _same(pkg, table, n_cols=None, order=None, **kw):
    """rows_fill_host == the model, the count included; returns the host's result."""
    t = np.asarray(table, dtype=np.uint32)
    got = pkg.rows_fill_host(t, order=order, n_cols=n_cols, **kw)
    want_rows, T = model.fill(t if n_cols is None else t[:, :n_cols], got.rows.shape[0].bit_length() - 1, kw.get("group", ()), kw.get("step"), kw.get("gaps", False),
                              kw.get("columns"), order, kw.get("rows"))
    assert got.n_filled == T and got.rows.shape == want_rows.shape and (got.rows == want_rows).all()
    assert pkg.rows_fill_host(t, order=order, n_cols=n_cols, count_only=True, **{k: v for k, v in kw.items() if k not in ("columns", "log_size")}) == (None, T)
    return got


def _steps(steps, groups=None, n_cols=4, seed=5):
    """A table with the given step column (1) and group column (0), the rest canonical random words."""
    t = np.random.default_rng(seed).integers(0, P, size=(len(steps), n_cols), dtype=np.uint32)
    t[:, STEP] = steps
    t[:, GROUP] = 0 if groups is None else groups
    return t


def test_gaps_against_the_model(pkg):
    cases_ = {"no gaps": ([3, 4, 5, 6, 7], None, 5), "one gap": ([3, 4, 9, 10], None, 8), "adjacent gaps": ([0, 3, 7, 8], None, 9),
              "a gap of exactly 1": ([5, 7, 8, 10], None, 6), "equal steps": ([4, 4, 4, 9], None, 8), "descending steps": ([9, 2, 1, 5], None, 7),
              "a group change between entries": ([1, 2, 30, 31, 40], [0, 0, 1, 1, 1], 13), "one entry": ([77], None, 1)}
    for what, (steps, groups, T) in cases_.items():
        got = _same(pkg, _steps(steps, groups), columns=ALL_KINDS, log_size=4, **GAPS)
        assert got.n_filled == T, what
        assert _same(pkg, _steps(steps, groups), columns=ALL_KINDS, log_size=4, step=STEP).n_filled == len(steps), what      # no gaps asked for
    got = _same(pkg, _steps([3, 4, 9, 10]), columns=[("keep", STEP), ("mark", 1), ("keep", 2), ("set", 3, 8)], log_size=3, **GAPS)
    t = _steps([3, 4, 9, 10])
    assert got.rows[:, 0].tolist() == [3, 4, 5, 6, 7, 8, 9, 10] and got.rows[:, 1].tolist() == [0, 0, 1, 1, 1, 1, 0, 0]
    assert got.rows[:, 2].tolist() == [t[0, 2]] + [t[1, 2]] * 5 + [t[2, 2], t[3, 2]] and got.rows[:, 3].tolist() == [t[0, 3], t[1, 3], 8, 8, 8, 8, t[2, 3], t[3, 3]]


@pytest.mark.parametrize("n_group", [0, 1, 2, 3, 4])
def test_group_columns(pkg, n_group):
    rng = np.random.default_rng(20 + n_group)
    t = rng.integers(0, P, size=(300, 7), dtype=np.uint32)
    t[:, 2:6] = rng.integers(0, 2, size=(300, 4))
    t[:, 2:6] = t[np.lexsort((t[:, 5], t[:, 4], t[:, 3], t[:, 2])), 2:6]      # the rows sorted by the four group words
    t[:, 6] = np.cumsum(rng.integers(0, 4, size=300))      # ascents of 0 .. 3: gaps of 0, 1, 2
    group = (2, 3, 4, 5)[:n_group]
    got = _same(pkg, t, columns=[("keep", 6), 0, ("mark", 1), ("keep", 6, 1)] + [("keep", c) for c in group], log_size=10, group=group, step=6, gaps=True)
    assert got.n_filled > 300
    if n_group == 0:      # every consecutive pair is one group: the step column has no holes left
        assert (np.diff(got.rows[:got.n_filled, 0].astype(np.int64)) <= 1).all()


def test_no_step_column_an_order_a_row_range_and_a_stride(pkg):
    rng = np.random.default_rng(7)
    t = rng.integers(0, P, size=(90, 9), dtype=np.uint32)
    t[:, 1] = np.sort(rng.integers(0, 400, size=90))
    outs = [("keep", 1), ("set", 2, 5), ("mark", P - 1), ("keep", 1, 1), ("set", 2, 5, 16), ("mark", 3, 1)]
    _same(pkg, t, columns=outs, log_size=7)                                        # no step: the tail repeats the last entry's words
    _same(pkg, t, columns=outs, log_size=7, rows=(17, 60))
    _same(pkg, t, n_cols=6, columns=outs, log_size=9, rows=(17, 60), step=1, gaps=True)      # a stride of 9 over 6 columns
    order = rng.permutation(90)[:50].astype(np.uint32)
    _same(pkg, t, order=order, columns=outs, log_size=None, step=1, gaps=True)     # an unsorted order: ascents are gaps, descents are not
    _same(pkg, t, order=np.sort(order), columns=outs, log_size=None, group=(0,), step=1, gaps=True)
    _same(pkg, t, order=np.array([4, 4, 4], dtype=np.uint32), columns=outs, log_size=2, step=1, gaps=True)      # the same row more than once
    with pytest.raises(ValueError):
        pkg.rows_fill_host(t, order=order, rows=(0, 5), columns=outs, log_size=7)


def test_the_tail_wraps_past_p_minus_1(pkg):
    t = _steps([P - 4, P - 2])
    got = _same(pkg, t, columns=[("keep", STEP), ("keep", STEP, 1), ("keep", STEP, 16), ("mark", 1)], log_size=3, **GAPS)
    assert got.n_filled == 3 and got.rows[:, 0].tolist() == [P - 4, P - 3, P - 2, P - 1, 0, 1, 2, 3] and got.rows[7, 2] == 19 and got.rows[:, 3].tolist() == [0, 1, 0, 1, 1, 1, 1, 1]


def test_count_at_the_edges_of_the_domain_and_above_2_to_32(pkg):
    assert _same(pkg, _steps([0, 1, 6, 7]), columns=ALL_KINDS, log_size=3, **GAPS).n_filled == 8      # T = 2^log_size
    with pytest.raises(pkg.BfhipError) as e:
        pkg.rows_fill_host(_steps([0, 1, 7, 8]), columns=ALL_KINDS, log_size=3, **GAPS)
    assert str(e.value) == WHO + "9 rows after filling, the domain has 8"
    # The largest gap between canonical steps is p - 2 rows (0 -> p - 1) and the steps of one ascent add up to less than p, so a total
    # above 2^32 takes more than two ascents: six entries of one group, steps 0, g + 1 three times over, three gaps of g = (2^32 - 1) / 3
    # rows. T = 6 + 3 g = 2^32 + 5 exactly — a total kept in 32 bits would be 5 and fit the domain.
    g = 1431655765
    t = _steps([0, g + 1] * 3)
    assert model.count(t, (GROUP,), STEP, True) == (1 << 32) + 5 == 6 + 3 * g
    assert pkg.rows_fill_host(t, count_only=True, **GAPS).n_filled == (1 << 32) + 5
    with pytest.raises(pkg.BfhipError) as e:
        pkg.rows_fill_host(t, columns=[0], log_size=3, **GAPS)
    assert str(e.value) == WHO + "4294967301 rows after filling, the domain has 8"
    # and the two largest gaps there are: 0 -> p - 1 twice, T = 4 + 2 (p - 2) = 2^32 - 2
    t = _steps([0, P - 1, 0, P - 1])
    assert pkg.rows_fill_host(t, count_only=True, **GAPS).n_filled == (1 << 32) - 2 == model.count(t, (GROUP,), STEP, True)
    with pytest.raises(pkg.BfhipError) as e:
        pkg.rows_fill_host(t, columns=[0], log_size=20, **GAPS)
    assert str(e.value) == WHO + "4294967294 rows after filling, the domain has 1048576"


def _raw(pkg, t, fill, log_size, outs, n_out, rows_out, n_filled, n_rows=None, n_cols=None, stride=None):
    return pkg.lib().bfhip_rows_fill_host(ctypes.c_void_p(t.ctypes.data), ctypes.c_uint64(t.shape[0] if n_rows is None else n_rows), ctypes.c_uint32(t.shape[1] if n_cols is None else n_cols),
                                          ctypes.c_uint64(t.shape[1] if stride is None else stride), fill, ctypes.c_uint32(log_size), outs, ctypes.c_uint32(n_out),
                                          ctypes.c_void_p(rows_out), n_filled)


def test_every_refusal_word_for_word(pkg):
    t = np.arange(40, dtype=np.uint32).reshape(10, 4)
    Out, Desc = pkg.FillOut, pkg.RowsFillDesc
    U32P = ctypes.POINTER(ctypes.c_uint32)
    out = np.full(32, 0xABABABAB, dtype=np.uint32)
    outs = (Out * 2)(Out(0, 0, 0, 0), Out(1, 0, 0, 1))
    n_filled = ctypes.c_uint64(77)
    order = np.arange(10, dtype=np.uint32)

    def desc(group=None, n_group=0, step=0, order_=None, n_entries=10, row_begin=0, flags=0, reserved=0):
        d = Desc(ctypes.cast(group, U32P) if group is not None else None, n_group, step, ctypes.cast(ctypes.c_void_p(order_.ctypes.data), U32P) if order_ is not None else None,
                 n_entries, row_begin, flags, reserved)
        d._keep = (group, order_)
        return d

    def refused(rule, fill=None, log_size=4, outs_=outs, n_out=2, rows_out=out.ctypes.data, nf=n_filled, **kw):
        fill = desc() if fill is None else fill
        rc = _raw(pkg, t, None if fill == "null" else ctypes.byref(fill), log_size, outs_, n_out, rows_out, None if nf is None else ctypes.byref(nf), **kw)
        assert rc == -1 and pkg.lib().bfhip_last_error().decode() == WHO + rule, pkg.lib().bfhip_last_error().decode()
        assert (out == 0xABABABAB).all()

    refused("null argument", fill="null")
    refused("null argument", nf=None)
    refused("null argument", outs_=None)
    refused("row_stride 3 is below n_cols 4", stride=3)
    refused("the count-only form takes null outputs, n_out 0 and log_size 0 together", rows_out=None)
    refused("the count-only form takes null outputs, n_out 0 and log_size 0 together", rows_out=None, n_out=0)
    refused("the count-only form takes null outputs, n_out 0 and log_size 0 together", rows_out=None, log_size=0)
    refused("log_size 0 is outside 1..30", log_size=0)
    refused("log_size 31 is outside 1..30", log_size=31)
    refused("n_out 0 is outside 1..256 (BFHIP_AIR_MAX_COLUMNS)", n_out=0)
    refused("n_out 257 is outside 1..256 (BFHIP_AIR_MAX_COLUMNS)", n_out=257)
    refused("reserved must be 0", fill=desc(reserved=1))
    refused("the table has no columns", n_cols=0)
    refused("n_cols 16777217 exceeds 2^24", n_cols=(1 << 24) + 1, stride=1 << 25)
    refused("n_rows 1099511627777 exceeds 2^40", n_rows=(1 << 40) + 1)
    refused("unknown flag bits 2", fill=desc(flags=2))
    refused("unknown flag bits 3", fill=desc(flags=3))
    refused("n_group 5 exceeds 4 (BFHIP_FILL_MAX_GROUP)", fill=desc(group=(ctypes.c_uint32 * 5)(), n_group=5))
    refused("n_group 2 with a null group_cols array", fill=desc(n_group=2))
    refused("group 1: column index 4 is not below n_cols 4", fill=desc(group=(ctypes.c_uint32 * 2)(3, 4), n_group=2))
    refused("step: column index 4 is not below n_cols 4", fill=desc(step=4))
    refused("BFHIP_FILL_GAPS needs a step column", fill=desc(step=0xFFFFFFFF, flags=1))
    refused("needs at least one entry", fill=desc(n_entries=0))
    refused("1073741825 entries exceed 2^30", fill=desc(n_entries=(1 << 30) + 1), n_rows=1 << 31)
    refused("row_begin 1 must be 0 when an order is given", fill=desc(order_=order, n_entries=5, row_begin=1))
    refused("row_begin 3 + n_entries 8 exceeds n_rows 10", fill=desc(n_entries=8, row_begin=3))
    refused("row_begin 11 + n_entries 1 exceeds n_rows 10", fill=desc(n_entries=1, row_begin=11))
    refused("output 1: unknown kind 3", outs_=(Out * 2)(Out(0, 0, 0, 0), Out(1, 3, 0, 0)))
    refused("output 1: column index 4 is not below n_cols 4", outs_=(Out * 2)(Out(3, 0, 0, 0), Out(4, 1, 0, 0)))
    refused("output 0: value 4294967295 is not a canonical M31 value", outs_=(Out * 2)(Out(0, 1, 0xFFFFFFFF, 0), Out(1, 0, 0, 0)))
    refused("output 1: value 2147483647 is not a canonical M31 value", outs_=(Out * 2)(Out(0, 0, P, 0), Out(77, 2, P, 0)))      # KEEP ignores its value, MARK its column
    refused("output 0: offset 17 exceeds 16 (BFHIP_FILL_MAX_OFFSET)", outs_=(Out * 2)(Out(0, 0, 0, 17), Out(1, 0, 0, 0)))
    bad_order = order.copy()
    bad_order[[3, 6]] = [10, 99]
    refused("order[3] = 10 is not a row of the table (10 rows)", fill=desc(order_=bad_order))
    refused("order[3] = 10 is not a row of the table (10 rows)", fill=desc(order_=bad_order), rows_out=None, n_out=0, log_size=0)
    refused("10 rows after filling, the domain has 8", log_size=3)
    assert n_filled.value == 10      # the count is known when the domain turns out too small
    refused("37 rows after filling, the domain has 32", fill=desc(flags=1), log_size=5, rows_out=np.full(64, 0xABABABAB, dtype=np.uint32).ctypes.data)
    assert n_filled.value == 37
    # the good call: column 0 is the step, so the tail counts on; column 1 at offset 1
    assert _raw(pkg, t, ctypes.byref(desc(n_entries=8, row_begin=1)), 4, outs, 2, out.ctypes.data, ctypes.byref(n_filled)) == 0 and n_filled.value == 8
    got = out.reshape(16, 2)
    assert got[:, 0].tolist() == t[1:9, 0].tolist() + [t[8, 0] + 1 + i for i in range(8)] and got[:, 1].tolist() == t[2:9, 1].tolist() + [t[8, 1]] * 9


def test_the_lowest_non_canonical_word_is_named(pkg):
    base = cases.stepped(120, 6, [(10, 4), (70, 9)], group_len=50)
    kw = dict(columns=[("keep", 2), ("set", 3, 1, 1), ("mark", 1), ("keep", 5, 16)], rows=(2, 110), log_size=7, **GAPS)
    plants = {"a group word": [(60, GROUP, P), (90, GROUP, P + 5)], "a step word": [(50, STEP, 0xFFFFFFFF)],      # row 50 opens its group and row 51 descends: no gap
              "an output word": [(30, 2, P), (80, 5, P)], "a set column's word of a real row": [(40, 3, P)],
              "several": [(100, 3, 0x80000000), (33, 5, P), (33, 2, P), (80, GROUP, P)]}
    for what, words in plants.items():
        t = base.copy()
        for r, c, v in words:
            t[r, c] = v
        want = model.lowest_bad_word(t, 7, (GROUP,), STEP, True, kw["columns"], rows=kw["rows"])
        assert want is not None, what
        with pytest.raises(pkg.BfhipError) as e:
            pkg.rows_fill_host(t, **kw)
        assert str(e.value) == WHO + "row %d, column %d: %d is not a canonical M31 value" % want, what
    # what is not checked: the rows in front of and behind the entries, a column nothing names, and — without gaps — the group and step words
    t = base.copy()
    t[:2, :] = t[110:, :] = 0xFFFFFFFF
    t[5, 4] = P + 9
    _same(pkg, t, **kw)
    t[7, GROUP] = t[9, STEP] = P
    _same(pkg, t, columns=kw["columns"], rows=kw["rows"], log_size=7)
    # a set column's word of an entry that no output row shows as a real row is not read: offset 16 alone skips entries 0 .. 15
    t = base.copy()
    t[2 + 3, 3] = P
    _same(pkg, t, columns=[("set", 3, 1, 16), ("mark", 1)], rows=(2, 110), log_size=7)
    # the refusal by the count comes first
    t = base.copy()
    t[60, STEP] = 0xFFFFFFFF
    with pytest.raises(pkg.BfhipError) as e:
        pkg.rows_fill_host(t, **kw)
    assert "rows after filling, the domain has 128" in str(e.value)


def test_struct_layouts_equal_the_header_comment_and_both_bindings_declare_the_calls(pkg):
    gen = sys.modules[pkg.__name__ + "._abi_gen"]
    text = open(os.path.join(ROOT, "include", "bfhip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")).read()
    classes = {"bfhip_fill_out": pkg.FillOut, "bfhip_rows_fill_desc": pkg.RowsFillDesc}
    for name, cls in classes.items():
        m = re.search(r"\* +%s +(\d+) bytes: ([^\n*]+)" % name, text)
        assert m, name
        stated = [(f.rsplit(" ", 1)[0], int(f.rsplit(" ", 1)[1])) for f in m.group(2).strip().split(", ")]
        assert ctypes.sizeof(cls) == int(m.group(1)), name
        assert [(f, getattr(cls, f).offset) for f, _ in gen.STRUCTS[name]] == stated, name
        body = re.search(r"pub struct %s \{(.*?)\}" % "".join(w.capitalize() for w in name.split("_")), rust, flags=re.S).group(1)
        assert re.findall(r"pub (\w+):", body) == [f for f, _ in stated]
    assert (gen.BFHIP_FILL_KEEP, gen.BFHIP_FILL_SET, gen.BFHIP_FILL_MARK, gen.BFHIP_FILL_GAPS) == (0, 1, 2, 1)
    assert (gen.BFHIP_FILL_NO_STEP, gen.BFHIP_FILL_MAX_GROUP, gen.BFHIP_FILL_MAX_OFFSET) == (0xFFFFFFFF, 4, 16)
    assert "pub const BFHIP_FILL_NO_STEP: u32 = 4294967295;" in rust
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("bfhip_rows_fill", "bfhip_rows_fill_host"):
        m = re.search(r"^int32_t %s\s*\((.*?)\)\s*;" % name, header, flags=re.S | re.M)
        restype, argtypes = gen.FUNCTIONS[name]
        assert m and restype is ctypes.c_int32 and len(argtypes) == len(m.group(1).split(",")), name
        r = re.search(r"pub fn %s\((.*?)\) -> i32;" % name, rust, flags=re.S)
        assert r and len(r.group(1).split(",")) == len(argtypes), name
        assert hasattr(pkg.lib(), name)
    assert hasattr(pkg.Context, "rows_fill") and hasattr(pkg.Context, "rows_fill_count")
    assert "pub fn rows_fill" in open(os.path.join(ROOT, "bindings", "rust", "lib.rs")).read()


@pytest.mark.parametrize("program,inp", [("hello1.bf", b""), ("collatz.bf", bytes([55, 10]))])
def test_brainfuck_example_equals_the_host_tables(pkg, program, inp):
    code = open(os.path.join(PROGRAMS, program)).read()
    regs, words = pkg.host_run(code, inp)[1], pkg.host_compile(code)

    def select_host(src, **kw):
        return pkg.rows_select_host(src, count_only=True, **kw).order

    def fill_host(src, order, **kw):
        got = pkg.rows_fill_host(src, order=order, **kw)
        want, T = model.fill(src, got.rows.shape[0].bit_length() - 1, kw.get("group", ()), kw.get("step"), kw.get("gaps", False), kw["columns"], order, kw.get("rows"))
        assert T == got.n_filled and (want == got.rows).all()
        return got.rows, got.n_filled

    for name in ("memory", "processor", "instruction"):
        T, n_entries = cases.brainfuck_table(pkg, regs, words, name, select_host, fill_host)
        assert T > n_entries if name == "memory" else T == n_entries      # both programs leave clk gaps inside an address
    with pytest.raises(ValueError):
        pkg.brainfuck_rows_fill("plus_instruction", 5)


def test_host_code_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/rows_fill_host_sanitize.cpp (its own main) compiled together with csrc/rows_fill_host.hip as plain C++ under g++
    -fsanitize=address,undefined and run directly: the validator, the gap count and the value rule of csrc/rows_fill.h and the host function
    over exactly fitting buffers — random fillings against an independent walk, the edges of this file, every refusal."""
    exe = str(tmp_path / "rows_fill_host_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "rows_fill_host_sanitize.cpp"),
                           "-x", "c++", os.path.join(ROOT, "stwo-brainfuck_amd", "csrc", "rows_fill_host.hip")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    out = r.stdout.strip().splitlines()
    assert re.fullmatch(r"random: \d+ fillings, \d+ with gaps, \d+ with an order, \d+ refused by the count, \d+ non-canonical", out[0]) and out[-1] == "rows_fill_host_sanitize ok", out
