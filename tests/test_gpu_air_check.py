"""-m gpu: the constraint program asserted on the trace domain (bfhip_air_check, csrc/air_check.hip) — the 13 Brainfuck programs against
bfhip_check_constraints on valid and corrupted tables, seeded random programs with offsets up to +-16 against the numpy reference of
tests/air_check_model.py (anchored to the oracle in tests/test_air_check_cpu.py) from fewer cells than a wave to many waves, violations
placed at wave edges of a synthetic AIR, the edges of the 64-bit lane mask, determinism, the contract and refusals, and the lookup example of
INTEGRATION.md section 2e. Every field of the report is an integer: every comparison is exact."""
import ctypes

import numpy as np
import pytest

import air_check_model
import air_model
from conftest import splitmix_column, P

pytestmark = pytest.mark.gpu

HELLO = ("++++++++++[>+++++++>++++++++++>+++>+<<<<-]>++.>+.+++++++..+++.>++.<<+++++++++++++++.>.+++.------.--------.>+.>.", b"")
NAMES = ["memory", "instruction", "program", "processor", "jnz", "jz", "input", "left", "minus", "output", "plus", "right", "end_of_execution"]
ONE = [1, 0, 0, 0]
SHARED = ("n_bad_cells", "first_bad_cell", "first_bad_constraint", "first_bad_value")      # what bfhip_check_report also has


def _elems(seed):
    e = splitmix_column(seed, 24)
    e[e == 0] = 1
    return e.tolist()


def _quads(seed, n):
    return splitmix_column(seed, 4 * n).reshape(n, 4).tolist()


class Dev:
    """device buffers freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, arr):
        self.ptrs.append(self.ctx.upload(np.ascontiguousarray(arr, dtype=np.uint32)))
        return self.ptrs[-1]

    def empty(self, n):
        self.ptrs.append(self.ctx.malloc(4 * n))
        return self.ptrs[-1]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.free(p)


def _check(ctx, program, log_size, cols, params, shifts=None):
    """AirCheckReport of one call on host columns (column k holds 2^(log_size - shifts[k]) cells)"""
    with Dev(ctx) as dev:
        return ctx.air_check(program, log_size, [dev.up(c) for c in cols], params, col_shifts=shifts)


def _show(tag, rep):
    """Every figure is printed before it is asserted on (visible with -s / in a captured failure)."""
    print(tag, {f: rep[f] for f in air_check_model.FIELDS})


# ---- 1. the 13 Brainfuck programs against the compiled-in check ---------------------------------------------------------------------------------
def _brainfuck_reports(ctx, pkg, comp, rows, elems, patch_logup=None):
    """(bfhip_check_constraints' report, air_check on the same row-granular buffers, air_check on every column expanded to full size).
    Main columns row-granular (shift 4); the logUp columns are bfhip_logup_generate's, shift 4 on all but the last four; IsFirst is passed.
    patch_logup: (column, cell) of the generated logUp columns to add 1 to before the checks."""
    n_main, M = rows.shape
    log_size, n_logup = int(np.log2(M)) + 4, 3 if comp == 3 else 1
    n = 1 << log_size
    program, _, _ = pkg.brainfuck_air_program(comp)
    with Dev(ctx) as dev:
        main = [dev.up(r) for r in rows]
        sizes = [M] * (4 * (n_logup - 1)) + [n] * 4
        logup = [dev.empty(s) for s in sizes]
        claimed = ctx.logup_generate(comp, log_size, main, elems, logup)
        host = [ctx.download(p, s) for p, s in zip(logup, sizes)]
        if patch_logup is not None:
            k, cell = patch_logup
            host[k][cell] = (int(host[k][cell]) + 1) % P
            logup[k] = dev.up(host[k])
        is_first = np.zeros(n, dtype=np.uint32); is_first[0] = 1
        want = ctx.check_constraints(comp, log_size, main, logup, elems, claimed)
        params = pkg.brainfuck_air_params(elems, claimed)
        shifts = [4] * (n_main + 4 * (n_logup - 1)) + [0] * 5
        shifted = ctx.air_check(program, log_size, main + logup + [dev.up(is_first)], params, col_shifts=shifts)
        full = [np.repeat(c, n // c.size) for c in list(rows) + host] + [is_first]
        expanded = ctx.air_check(program, log_size, [dev.up(c) for c in full], params)
    return want, shifted, expanded


def _assert_same_as_compiled(want, rep, tag):
    got = rep.as_dict()
    _show(tag, got)
    assert all(got[f] == want[f] for f in SHARED), (tag, want)
    assert list(rep.bad_per_constraint[:12]) == want["bad_per_constraint"][:12] and not any(rep.bad_per_constraint[12:]), (tag, want)
    assert got["ok"] == want["ok"] and got["log_size"] == want["log_size"]


def test_brainfuck_programs_equal_check_constraints(_ctx, pkg, _oracle):
    """hello: the 13 programs on valid tables; Processor with one main cell changed; Memory with the last logUp column changed at cell 0, the
    cell whose predecessor wraps (coset index 0: its row at offset -1 is the last coset element). Row-granular and full-size storage."""
    elems = _elems(77)
    logs = set()
    for comp in range(13):
        rows = np.ascontiguousarray(_oracle.table(*HELLO, comp).T)
        want, shifted, expanded = _brainfuck_reports(_ctx, pkg, comp, rows, elems)
        assert want["ok"] and pkg.format_air_check(shifted) == "air check: ok"
        for rep, storage in ((shifted, "shift 4"), (expanded, "full size")):
            _assert_same_as_compiled(want, rep, "%s valid %s" % (NAMES[comp], storage))
            assert bytes(rep) == bytes(shifted)
        logs.add(want["log_size"])
    assert min(logs) == 4 and max(logs) >= 9      # 16 cells: less than a wave; 512 cells and more: many

    rows = np.ascontiguousarray(_oracle.table(*HELLO, 3).T)
    rows[5, 5] = (int(rows[5, 5]) + 1) % P      # mv of table row 5
    want, shifted, expanded = _brainfuck_reports(_ctx, pkg, 3, rows, elems)
    assert want["n_bad_cells"] >= 16 and want["first_bad_cell"] >> 4 == 5      # the 16 cells of the changed row at least
    for rep, storage in ((shifted, "shift 4"), (expanded, "full size")):
        _assert_same_as_compiled(want, rep, "processor main cell %s" % storage)

    rows = np.ascontiguousarray(_oracle.table(*HELLO, 0).T)
    want, shifted, expanded = _brainfuck_reports(_ctx, pkg, 0, rows, elems, patch_logup=(0, 0))
    n = 16 * rows.shape[1]
    successor = int(air_model.offset_rows(want["log_size"], 0, 1)[0])
    assert want["n_bad_cells"] == 2 and want["bad_per_constraint"][11] == 2 and want["first_bad_cell"] == 0 and 0 < successor < n
    for rep, storage in ((shifted, "shift 4"), (expanded, "full size")):
        _assert_same_as_compiled(want, rep, "memory logUp cell 0 %s" % storage)
        assert rep.as_dict()["first_cell_per_constraint"] == [None] * 11 + [0]


# ---- 2. seeded random programs against the numpy reference ---------------------------------------------------------------------------------------
def _columns_read_at_an_offset(code, n_cols):
    out = [False] * n_cols
    for i in range(0, len(code), 4):
        op, _, a, b = code[i: i + 4]
        if op in (air_model.M_COL, air_model.Q_COL) and b != 0:
            for c in range(a, a + (4 if op == air_model.Q_COL else 1)):
                out[c] = True
    return out


_RANDOM = {}


def _random_case(seed, log_size):
    """(code, n_cols, n_params, stored columns, shifts or None, params, the reference's report), computed once. Offsets up to +-16; columns
    that the program reads at offset 0 only are stored at shift 2 where the domain allows it, the others full size."""
    if (seed, log_size) not in _RANDOM:
        code, n_cols, n_params, _ = air_model.random_program(seed, n_cols=14, n_ops=150, max_off=16, max_cons=64)
        n = 1 << log_size
        full = [splitmix_column((seed << 8) + 16 * log_size + k, n) for k in range(n_cols)]
        shifts = None
        if log_size >= 2:
            shifts = [0 if offset else 2 for offset in _columns_read_at_an_offset(code, n_cols)]
            full = [np.repeat(c[:: 1 << s], 1 << s) for c, s in zip(full, shifts)]
        params = _quads(seed + 1000, n_params)
        want = air_check_model.report(code, full, params, log_size)
        stored = [c[:: 1 << s] for c, s in zip(full, shifts)] if shifts else full
        _RANDOM[(seed, log_size)] = (code, n_cols, n_params, stored, shifts, params, want)
    return _RANDOM[(seed, log_size)]


@pytest.mark.parametrize("log_size", [1, 2, 5, 6, 7, 10])
@pytest.mark.parametrize("seed", [4, 34])      # 34 and 29 constraints: both halves of the lane mask; 2 and 3 columns at a shift
def test_random_programs_match_the_reference(_ctx, pkg, seed, log_size):
    """Every field, first_cell_per_constraint included: 2 and 4 cells (offsets wrap several times), half a wave, exactly one wave, two waves,
    16 waves. Random columns: nearly every cell violates nearly every constraint — the all-bad path, where counts reach the number of cells."""
    code, n_cols, n_params, stored, shifts, params, want = _random_case(seed, log_size)
    got = _check(_ctx, pkg.AirProgram(code, n_cols, n_params), log_size, stored, params, shifts).as_dict()
    _show("seed %d log_size %d" % (seed, log_size), got)
    assert air_check_model.same(got, want), want
    n = 1 << log_size
    assert want["n_bad_cells"] == n and want["first_bad_cell"] == 0 and max(want["bad_per_constraint"]) == n
    signed = lambda w: w - (1 << 32) if w >= 1 << 31 else w
    assert any(abs(signed(code[i + 3])) > 8 for i in range(0, len(code), 4) if code[i] in (air_model.M_COL, air_model.Q_COL))


def test_two_runs_give_byte_identical_reports(_ctx, pkg):
    code, n_cols, n_params, stored, shifts, params, _ = _random_case(4, 10)
    program = pkg.AirProgram(code, n_cols, n_params)
    first, second = _check(_ctx, program, 10, stored, params, shifts), _check(_ctx, program, 10, stored, params, shifts)
    assert bytes(first) == bytes(second) and len(bytes(first)) == 1088 and first.n_bad_cells == 1 << 10


# ---- 3. violations placed at wave edges of a synthetic AIR ---------------------------------------------------------------------------------------
A, B, OUT, NXT, PRV, NXT2, PRV2 = range(7)


def _synthetic_program(pkg):
    """tests/test_gpu_air_program.py's AIR at d = 2: out = a * b and four shifted copies of a: nxt = a[+1], prv = a[-1], nxt2 = a[+2], prv2 = a[-2]."""
    b = pkg.AirBuilder()
    b.constraint(b.col(OUT) - b.col(A) * b.col(B))
    b.constraint(b.col(NXT) - b.col(A, 1))
    b.constraint(b.col(PRV) - b.col(A, -1))
    b.constraint(b.col(NXT2) - b.col(A, 2))
    b.constraint(b.col(PRV2) - b.col(A, -2))
    return b.program()


_SYNTHETIC = {}


def _synthetic_trace(log_size):
    """The 7 columns in storage order, valid by construction: built in coset order (where the row at offset k is k places on, cyclically) and
    moved to bit-reversed circle-domain order — cell s holds coset index 2 d (d < n / 2) or 2 (n - 1 - d) + 1, d the bit reversal of s."""
    if log_size not in _SYNTHETIC:
        n = 1 << log_size
        a, b = splitmix_column(90 + log_size, n).astype(np.uint64), splitmix_column(190 + log_size, n).astype(np.uint64)
        coset = [a, b, a * b % np.uint64(P), np.roll(a, -1), np.roll(a, 1), np.roll(a, -2), np.roll(a, 2)]
        d = air_model.bit_reverse(np.arange(n), log_size)
        _SYNTHETIC[log_size] = np.stack(coset).astype(np.uint32)[:, np.where(d < n // 2, 2 * d, 2 * (n - 1 - d) + 1)]
    return _SYNTHETIC[log_size]


@pytest.mark.parametrize("log_size", [7, 16])
def test_placed_violations_are_named_with_their_cells(_ctx, pkg, log_size):
    """One cell of `a` changed — cell 0, 63, 64 (the two sides of a wave's edge) or n - 1: each of the five constraints reads it once, the
    four copies through their offsets from another cell, so each fails at exactly one cell, the one the reference gives."""
    program, trace, n = _synthetic_program(pkg), _synthetic_trace(log_size), 1 << log_size
    with Dev(_ctx) as dev:
        cols = [dev.up(c) for c in trace]
        valid = _ctx.air_check(program, log_size, cols, [])
        assert valid.as_dict()["ok"] and valid.first_bad_constraint == -1 and pkg.format_air_check(valid) == "air check: ok"
        for cell in (0, 63, 64, n - 1):
            bad = trace[A].copy()
            bad[cell] = (int(bad[cell]) + 1) % P
            got = _ctx.air_check(program, log_size, [dev.up(bad)] + cols[1:], []).as_dict()
            want = air_check_model.report(program.code, np.concatenate([bad[None], trace[1:]]), [], log_size)
            _show("log_size %d cell %d" % (log_size, cell), got)
            assert air_check_model.same(got, want), want
            reach = lambda off: int(np.nonzero(air_model.offset_rows(log_size, 0, off) == cell)[0][0])      # the cell whose row at `off` is `cell`
            assert want["first_cell_per_constraint"] == [cell, reach(1), reach(-1), reach(2), reach(-2)]
            assert want["bad_per_constraint"] == [1] * 5 and want["n_bad_cells"] == 5


# ---- 4. the edges of the lane mask ------------------------------------------------------------------------------------------------------------------
def _mask_edges(ctx, pkg):
    """64 constraints, constraint j = column j, log_size 8 (four waves); only columns 31, 32 and 63 are non-zero, at one cell each, in waves
    1, 0 and 3. Returns (report, the reference's)."""
    b = pkg.AirBuilder()
    for j in range(64):
        b.constraint(b.col(j))
    program = b.program()
    cols = np.zeros((64, 256), dtype=np.uint32)
    cols[31, 70], cols[32, 9], cols[63, 255] = 5, P - 1, 123456
    with Dev(ctx) as dev:
        zero = dev.up(cols[0])
        rep = ctx.air_check(program, 8, [dev.up(c) if c.any() else zero for c in cols], [])
    return rep, air_check_model.report(program.code, cols, [], 8)


def _assert_mask_edges(ctx, pkg):
    rep, want = _mask_edges(ctx, pkg)
    got = rep.as_dict()
    _show("mask edges", got)
    assert air_check_model.same(got, want), want
    assert want["bad_per_constraint"] == [1 if j in (31, 32, 63) else 0 for j in range(64)] and want["n_bad_cells"] == 3
    assert (want["first_bad_cell"], want["first_bad_constraint"], want["first_bad_value"]) == (9, 32, [P - 1, 0, 0, 0])
    assert [want["first_cell_per_constraint"][j] for j in (31, 32, 63)] == [70, 9, 255]
    assert pkg.format_air_check(rep) == ("air check: 3 of 256 cells violate 3 of 64 constraints\nconstraint 31: 1 cells, first at cell 70\n"
                                         "constraint 32: 1 cells, first at cell 9, value (%d, 0, 0, 0)\nconstraint 63: 1 cells, first at cell 255" % (P - 1))


def test_mask_bits_31_32_and_63(_ctx, pkg):
    _assert_mask_edges(_ctx, pkg)


# ---- 6. the contract ----------------------------------------------------------------------------------------------------------------------------------
def test_valid_trace_returns_zero_and_leaves_the_error_text(_ctx, pkg):
    program, trace = _synthetic_program(pkg), _synthetic_trace(7)
    L = pkg.lib()
    with Dev(_ctx) as dev:
        cols = [dev.up(c) for c in trace]
        with pytest.raises(pkg.BfhipError, match="log_size"):
            _ctx.air_check(program, 0, cols, [])
        text = L.bfhip_last_error()
        rep = pkg.AirCheckReport()
        assert L.bfhip_air_check(_ctx._h, program._h, 7, _ctx._ptr_array(cols), None, None, 0, ctypes.byref(rep)) == 0
        assert rep.n_bad_cells == 0 and L.bfhip_last_error() == text and b"bfhip_air_check: log_size" in text
        # violations are a result too: 0, and the text stays
        bad = trace[OUT].copy()
        bad[100] = (int(bad[100]) + 1) % P
        assert L.bfhip_air_check(_ctx._h, program._h, 7, _ctx._ptr_array(cols[:OUT] + [dev.up(bad)] + cols[OUT + 1:]), None, None, 0, ctypes.byref(rep)) == 0
        assert rep.n_bad_cells == 1 and rep.first_bad_cell == 100 and rep.first_bad_constraint == 0 and L.bfhip_last_error() == text


def test_works_inside_an_open_session_without_touching_the_arena(_ctx, pkg):
    log_size = 7
    _ctx.set_pcs_config(pkg.PcsConfig())
    program, trace = _synthetic_program(pkg), _synthetic_trace(log_size)
    bad = trace.copy()
    bad[PRV, 64] = (int(bad[PRV, 64]) + 1) % P
    with Dev(_ctx) as dev:
        ch = pkg.Channel((0, 0, 0, 0))
        with pkg.PcsSession(_ctx) as s:
            cols = [dev.up(c) for c in bad]
            s.commit(ch, cols, [log_size] * 7, form=0)
            lde = s.tree_columns(0)[1]
            before, in_use = [_ctx.download(p, 2 << log_size) for p in lde], _ctx.memory()["arena_in_use"]
            got = _ctx.air_check(program, log_size, cols, []).as_dict()
            assert _ctx.memory()["arena_in_use"] == in_use and in_use > 0
            after = [_ctx.download(p, 2 << log_size) for p in lde]
    assert air_check_model.same(got, air_check_model.report(program.code, bad, [], log_size))
    assert got["bad_per_constraint"] == [0, 0, 1, 0, 0] and got["first_bad_cell"] == 64
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def test_refusals_name_the_rule_and_leave_the_context_usable(_ctx, pkg):
    ctx = _ctx
    program = _synthetic_program(pkg)
    b = pkg.AirBuilder()
    b.constraint(b.secure_col(0) * b.param(0))
    with_param = b.program()
    with Dev(ctx) as dev:
        col = dev.up(np.zeros(1 << 7, dtype=np.uint32))
        cols = [col] * 7
        for kwargs, what in ((dict(col_shifts=[4, 0, 0, 0, 0, 0, 0]), "column 0 is stored with shift 4 and read at a non-zero offset"),
                             (dict(col_shifts=[0, 1, 0, 0, 0, 0, 0]), "column 1 has shift 1"),
                             (dict(col_shifts=[0, 6, 0, 0, 0, 0, 0]), r"column 1 has shift 6 \(0, or 2 .. log_size\)"),
                             (dict(params=[ONE]), "the program takes 0 parameters, got 1"),
                             (dict(program=with_param, cols=cols[:4], params=[]), "the program takes 1 parameters, got 0"),
                             (dict(program=with_param, cols=cols[:4], params=[[0, P, 0, 0]]), "a parameter word is not a canonical M31"),
                             (dict(log_size=0), r"log_size must be in \[1, max_log_domain = %d\], got 0" % ctx.max_log_domain),
                             (dict(log_size=ctx.max_log_domain + 1), "log_size must be in"),
                             (dict(cols=cols[:3] + [0] + cols[4:]), r"null column pointer \(column 3\)")):
            args = dict(program=program, log_size=5, cols=cols, params=[], col_shifts=None)
            args.update(kwargs)
            with pytest.raises(pkg.BfhipError, match="bfhip_air_check: " + what):
                ctx.air_check(args["program"], args["log_size"], args["cols"], args["params"], col_shifts=args["col_shifts"])
            _assert_mask_edges(ctx, pkg)      # after each refusal the context still computes
        # a column stored with a shift and read at offset 0 only is fine, up to shift = log_size
        assert ctx.air_check(program, 5, cols, [], col_shifts=[0, 5, 2, 0, 0, 0, 0]).as_dict()["ok"]


# ---- 7. the lookup example of INTEGRATION.md section 2e ------------------------------------------------------------------------------------------
def test_integration_lookup_example(_ctx, pkg):
    """`ctx.air_check(prog, log_size, trace_cols + inter_cols, [z, alpha, claimed])` before the first commit: ok on the honest trace; with one
    mult cell changed behind the interaction trace's back it names logup_last (constraint 1) at the cell the reference gives."""
    log_size, ctx = 6, _ctx
    n = 1 << log_size
    f = pkg.AirBuilder()                                   # the fractions: columns a, t, mult; parameters z, alpha
    a, t, mult, z, alpha = f.col(0), f.col(1), f.col(2), f.param(0), f.param(1)
    f.frac(1, alpha * a - z); f.end_column()
    f.frac(-mult, alpha * t - z); f.end_column()
    fractions = f.logup_program()
    b = pkg.AirBuilder()                                   # the constraints: a, t, mult, IsFirst, then the 8 interaction coordinate columns
    a, t, mult, is_first = b.col(0), b.col(1), b.col(2), b.col(3)
    z, alpha, total = b.param(0), b.param(1), b.param(2)
    cur0, cur1, prev1 = b.secure_col(4), b.secure_col(8), b.secure_col(8, -1)
    b.constraint(cur0 * (alpha * a - z) - b._to_q(b.const(1)))
    b.constraint((cur1 - (prev1 - total * is_first) - cur0) * (alpha * t - z) - b._to_q(-mult))
    prog = b.program()
    table = splitmix_column(51, n)                         # t distinct, a drawn from t, mult[i] = how often t[i] occurs in a
    assert len(set(table.tolist())) == n
    pick = splitmix_column(52 << 32, n) % np.uint32(n // 4)
    first = np.zeros(n, dtype=np.uint32); first[0] = 1
    trace = np.stack([table[pick], table, np.bincount(pick, minlength=n).astype(np.uint32), first])
    zq, alphaq = _quads(61, 2)
    with Dev(ctx) as dev:
        trace_cols, inter_cols = [dev.up(c) for c in trace], [dev.empty(n) for _ in range(8)]
        claimed = ctx.logup_program_generate(fractions, log_size, trace_cols[:3], [zq, alphaq], inter_cols)
        assert claimed == [0, 0, 0, 0]
        report = ctx.air_check(prog, log_size, trace_cols + inter_cols, [zq, alphaq, claimed])
        assert report.as_dict()["ok"] and pkg.format_air_check(report) == "air check: ok"
        bad = trace[2].copy()
        bad[3] = (int(bad[3]) + 1) % P
        report = ctx.air_check(prog, log_size, trace_cols[:2] + [dev.up(bad), trace_cols[3]] + inter_cols, [zq, alphaq, claimed])
        inter = np.stack([ctx.download(p, n) for p in inter_cols])
    got = report.as_dict()
    want = air_check_model.report(prog.code, np.concatenate([trace[:2], bad[None], trace[3:], inter]), [zq, alphaq, claimed], log_size)
    _show("lookup, mult[3] changed", got)
    assert air_check_model.same(got, want), want
    assert want["bad_per_constraint"] == [0, 1] and want["first_cell_per_constraint"] == [None, 3] and want["first_bad_constraint"] == 1
    assert pkg.format_air_check(report).startswith("air check: 1 of 64 cells violate 1 of 2 constraints\nconstraint 1: 1 cells, first at cell 3, value (")
