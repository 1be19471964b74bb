"""-m gpu: bfhip_logup_program_generate_batch (csrc/logup_batch.hip) — every component's output columns and claimed sum are, word for word,
what bfhip_logup_program_generate leaves for that component alone (that entry is held to the numpy model and the oracle by
tests/test_gpu_logup_program.py), and `total` is the QM31 sum of the claimed sums computed here. The lists sit on the seams of the three
prefix tables (waves, scan tiles, 256-cell blocks), on the LDS sizing of the shared row-stage launch, on the 2^16 launch threshold and on
the chunking of the tile totals; then shifted inputs, saturated cells, a program that appears three times, the 13 Brainfuck programs against
bfhip_logup_generate, zero denominators, an open session, determinism and every refusal. Integer field arithmetic: every comparison is
exact.

One refusal of the header has no case: a list whose staged blocks do not fit the staging ring. At the caps (64 distinct programs of 4096
instructions = 4 MiB of code, 64 x 256 column descriptors = 256 KiB, the parameters and tables below 100 KiB) a list stages less than
5 MiB of the 8 MiB ring, so no valid list reaches it."""
import ctypes
import sys

import numpy as np
import pytest

import field_inputs
import logup_model
import pcs_replay
from conftest import splitmix_column, P

pytestmark = pytest.mark.gpu

HELLO = ("++++++++++[>+++++++>++++++++++>+++>+<<<<-]>++.>+.+++++++..+++.>++.<<+++++++++++++++.>.+++.------.--------.>+.>.", b"")
NAMES = ["memory", "instruction", "program", "processor", "jnz", "jz", "input", "left", "minus", "output", "plus", "right", "end_of_execution"]
ME = "bfhip_logup_program_generate_batch"
SENTINEL = 0x5A5A5A5A


def _elems(seed):
    e = splitmix_column(seed, 24)
    e[e == 0] = 1
    return e.tolist()


def _quads(seed, n):
    return splitmix_column(seed, 4 * n).reshape(n, 4).tolist()


def _q_sum(values):
    total = [0, 0, 0, 0]
    for v in values:
        total = [(a + b) % P for a, b in zip(total, v)]
    return total


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


def _random_case(n_logup, n_fractions, log_size, column=splitmix_column, seed=0):
    """(code, columns, parameters) of a seeded random fraction program over distinct cells, as tests/test_gpu_logup_program.py builds them"""
    code, n_cols, n_params = logup_model.random_program(1000 * n_fractions + log_size + seed, n_logup, n_fractions)
    if (n_logup, n_fractions) == (1, 1):      # the one-fraction program over 2 columns: params[0] * col 0 / (col 1 + params[1])
        m = logup_model
        code = [m.M_COL, 0, 0, 0, m.M_COL, 1, 1, 0, m.Q_FROM_M, 1, 1, 0, m.Q_PARAM, 0, 1, 0, m.Q_ADD, 1, 1, 0, m.Q_PARAM, 0, 0, 0, m.Q_MULM, 0, 0, 0,
                m.FRAC, 0, 0, 1, m.END_COL, 0, 0, 0]
        n_cols, n_params = 2, 2
    cols = np.stack([column(((k + 1) << 32) + log_size + (seed << 40), 1 << log_size) for k in range(n_cols)])
    return code, cols, _quads(600 + log_size + seed, n_params)


class Item:
    """one component of a list, on the host"""

    def __init__(self, pkg, log_size, n_logup=2, n_fractions=3, seed=0, column=splitmix_column, program=None, case=None, shifts=None, params=None):
        code, cols, pars = case if case else _random_case(n_logup, n_fractions, log_size, column, seed)
        self.code = code
        self.program = program if program is not None else pkg.LogupProgram(code, len(cols), len(pars))
        self.log_size, self.shifts, self.params = log_size, shifts, pars if params is None else params
        self.cols = [c[: 1 << (log_size - s)] for c, s in zip(cols, shifts)] if shifts else list(cols)
        self.n_out = 4 * self.program.shape["n_logup_cols"]


def _both(ctx, items):
    """Runs the list in one batch call and component by component through the single call, on the same device columns. Asserts that every
    output column and claimed sum agree and that total is the sum; returns (the batch's columns per component, claimed sums, total)."""
    with Dev(ctx) as dev:
        entries, refs = [], []
        for it in items:
            src = [dev.up(c) for c in it.cols]
            n = 1 << it.log_size
            entries.append((it.program, it.log_size, src, it.params, [dev.empty(n) for _ in range(it.n_out)], it.shifts))
            refs.append([dev.empty(n) for _ in range(it.n_out)])
        claimed, total = ctx.logup_program_generate_batch(entries)
        got = []
        for k, (it, e, ref) in enumerate(zip(items, entries, refs)):
            want_claimed = ctx.logup_program_generate(it.program, it.log_size, e[2], it.params, ref, col_shifts=it.shifts)
            assert claimed[k] == want_claimed, ("claimed sum of component", k)
            n = 1 << it.log_size
            got.append(np.stack([ctx.download(p, n) for p in e[4]]))
            for j, p in enumerate(ref):
                assert np.array_equal(got[k][j], ctx.download(p, n)), ("component", k, "coordinate column", j)
        assert len(claimed) == len(items) and total == _q_sum(claimed)
        return got, claimed, total


# ---- 1. the seams of the three prefix tables ---------------------------------------------------------------------------------------------------
# log_size 1: 2 cells, N / 2 = 1; 12: two scan tiles, so the totals matter; 6: exactly one wave; 11: exactly one tile; 5: a partial wave
SEAMS = [1, 12, 6, 11, 5, 12]


@pytest.mark.parametrize("order", ["as_listed", "reversed"])
def test_seams_of_the_prefix_tables(_ctx, pkg, order):
    logs = SEAMS if order == "as_listed" else SEAMS[::-1]
    items = [Item(pkg, log, seed=10 * k) for k, log in enumerate(logs)]
    got, claimed, total = _both(_ctx, items)
    assert any(total) and len({tuple(c) for c in claimed}) == len(items)


# ---- 2. every wave guarded; a single component -----------------------------------------------------------------------------------------------------
def test_64_components_of_two_cells(_ctx, pkg):
    program = Item(pkg, 1).program
    items = [Item(pkg, 1, seed=k, program=program if k % 2 else None) for k in range(64)]
    _, claimed, _ = _both(_ctx, items)
    assert len({tuple(c) for c in claimed}) == 64


def test_one_component_of_one_wave(_ctx, pkg):
    _both(_ctx, [Item(pkg, 6)])


# ---- 3. LDS sizing of the shared launch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["caps_first", "caps_last"])
def test_the_shared_launch_is_sized_for_its_largest_program(_ctx, pkg, order):
    """8 logUp columns and 32 fractions beside one fraction, both at log_size 7: the small program's waves get the large program's LDS,
    never the reverse"""
    caps, one = Item(pkg, 7, 8, 32), Item(pkg, 7, 1, 1, seed=1)
    assert caps.program.shape["n_logup_cols"] == 8 and caps.program.shape["n_fractions"] == 32
    assert caps.program.shape["m_regs"] + 4 * caps.program.shape["q_regs"] > one.program.shape["m_regs"] + 4 * one.program.shape["q_regs"]
    _both(_ctx, [caps, one] if order == "caps_first" else [one, caps])


# ---- 4. the launch threshold ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beside", ["a_larger_program", "equal_programs"])
def test_components_around_the_launch_threshold(_ctx, pkg, beside):
    """One-fraction programs over 2 columns at log_size 15, 16 and 17 (2560 bytes of LDS a wave: 32 waves a CU). Beside a log_size 3
    component whose program asks for 5376 bytes (30 waves a CU) the one of 2^15 cells shares that component's launch and the two of 2^16
    cells and more launch alone (csrc/logup_batch_plan.h has the rule); without it the three share one launch that crosses both sizes."""
    items = [Item(pkg, 15, 1, 1), Item(pkg, 16, 1, 1, seed=1), Item(pkg, 17, 1, 1, seed=2)]
    lds = lambda it: 256 * (it.program.shape["m_regs"] + 4 * it.program.shape["q_regs"])
    assert {lds(it) for it in items} == {2560} and len(items[0].cols) == 2
    if beside == "a_larger_program":
        items.insert(2, Item(pkg, 3, seed=3))
        assert 163840 // lds(items[2]) < 32
    _both(_ctx, items)


# ---- 5. more than one chunk of tile totals ----------------------------------------------------------------------------------------------------------
def test_more_than_one_chunk_of_tile_totals(_ctx, pkg):
    """log_size 20: nb = 512 tile totals = two chunks of 256 with a carry, beside a component of 16 cells"""
    _both(_ctx, [Item(pkg, 20, 1, 1), Item(pkg, 4, 1, 1, seed=1)])


# ---- 6. shifted inputs ------------------------------------------------------------------------------------------------------------------------------
def test_mixed_shifts_in_the_middle_of_a_batch(_ctx, pkg):
    log_size = 7
    case = _random_case(2, 3, log_size, seed=5)
    shifts = ([4, 0, 2, 3, log_size, 0, 4, 2] * 4)[: len(case[1])]
    assert 4 in shifts and 0 in shifts
    mixed = Item(pkg, log_size, case=case, shifts=shifts)
    want, want_claimed, zeros = logup_model.generate(case[0], mixed.cols, shifts, case[2], log_size)
    got, claimed, _ = _both(_ctx, [Item(pkg, 5, seed=1), mixed, Item(pkg, 8, seed=2)])
    assert zeros == [] and claimed[1] == want_claimed and np.array_equal(got[1], want)


# ---- 7. saturated cells ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["max", "zero", "edge"])
def test_saturated_cells(_ctx, pkg, family):
    log_size = 6
    column = {"max": lambda seed, n: np.full(n, P - 1, dtype=np.uint32), "zero": lambda seed, n: np.zeros(n, dtype=np.uint32), "edge": field_inputs.edge}[family]
    items = [Item(pkg, log_size, seed=1, column=column), Item(pkg, log_size, seed=2, column=column)]
    items[1].params = [[P - 1] * 4] * len(items[1].params)
    for it in items:
        assert logup_model.generate(it.code, it.cols, [0] * len(it.cols), it.params, log_size)[2] == [], "the test's parameters must keep every denominator non-zero"
    _both(_ctx, items)


# ---- 8. equal programs staged once -------------------------------------------------------------------------------------------------------------------
def test_one_program_three_times(_ctx, pkg):
    first = Item(pkg, 9, seed=0)
    items = [first, Item(pkg, 5, seed=7, program=first.program), Item(pkg, 9, seed=8, program=first.program)]
    items[1].params, items[2].params = _quads(71, len(first.params)), first.params
    _, claimed, _ = _both(_ctx, items)
    assert claimed[0] != claimed[2]


# ---- 9. the 13 Brainfuck programs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["shift_4", "full_size"])
def test_brainfuck_programs_match_logup_generate(_ctx, pkg, _oracle, storage):
    """The 13 brainfuck_logup_programs on `hello`'s tables in ONE batch: every earlier column == the 16-fold broadcast of
    bfhip_logup_generate's row-granular output, the last column and the claimed sum == bfhip_logup_generate's; the 13 claimed sums of a valid
    trace add up to zero."""
    ctx, elems = _ctx, _elems(77)
    params = pkg.brainfuck_air_params(elems, [0, 0, 0, 0])[:24]
    with Dev(ctx) as dev:
        entries, compiled, compiled_claimed = [], [], []
        for comp in range(13):
            rows = np.ascontiguousarray(_oracle.table(HELLO[0], HELLO[1], comp).T)
            n_main, M = rows.shape
            log_size, n_logup = int(np.log2(M)) + 4, 3 if comp == 3 else 1
            sizes = [M] * (4 * (n_logup - 1)) + [16 * M] * 4
            dst = [dev.empty(s) for s in sizes]
            compiled_claimed.append(ctx.logup_generate(comp, log_size, [dev.up(r) for r in rows], elems, dst))
            compiled.append(np.stack([np.repeat(ctx.download(p, s), 16 * M // s) for p, s in zip(dst, sizes)]))
            program, _ = pkg.brainfuck_logup_program(comp)
            cols, shifts = (rows, [4] * n_main) if storage == "shift_4" else (np.repeat(rows, 16, axis=1), None)
            entries.append((program, log_size, [dev.up(c) for c in cols], params, [dev.empty(16 * M) for _ in range(4 * n_logup)], shifts))
        claimed, total = ctx.logup_program_generate_batch(entries)
        assert claimed == compiled_claimed and total == [0, 0, 0, 0] and any(any(c) for c in claimed)
        for comp, e in enumerate(entries):
            got = np.stack([ctx.download(p, 1 << e[1]) for p in e[4]])
            assert np.array_equal(got, compiled[comp]), NAMES[comp]
        assert min(e[1] for e in entries) == 4 and max(e[1] for e in entries) >= 9


# ---- 10. zero denominators ------------------------------------------------------------------------------------------------------------------------
def _lookup_fractions(pkg):
    """Columns a (0), t (1), mult (2); parameters z (0), alpha (1). Column 0: 1 / (alpha t - z) + 1 / (alpha a - z) + alpha / (alpha a - z);
    column 1: -mult / (alpha t - z): fractions 0, 1, 2; then 3."""
    b = pkg.AirBuilder()
    a, t, mult, z, alpha = b.col(0), b.col(1), b.col(2), b.param(0), b.param(1)
    b.frac(1, alpha * t - z)
    b.frac(1, alpha * a - z)
    b.frac(b.param(1), alpha * a - z)
    b.end_column()
    b.frac(-mult, alpha * t - z)
    b.end_column()
    return b.logup_program()


def test_zero_denominators_name_the_lowest_component_cell_and_fraction(_ctx, pkg):
    """z = alpha * a[37] where `a` also holds that value at cell 50: fractions 1 and 2 vanish at cells 37 and 50. First in component 1 of 3
    only, then in components 1 and 2 (there at cells 12 and 37): the message names component 1, cell 37, fraction 1 both times. The next
    call on the context is exact."""
    ctx, log_size, n = _ctx, 6, 64
    program = _lookup_fractions(pkg)
    alpha = _quads(21, 1)[0]

    def columns(seed, cells):
        a, t, mult = splitmix_column(seed << 32, n), splitmix_column((seed + 1) << 32, n), splitmix_column((seed + 2) << 32, n)
        for c in cells[1:]:
            a[c] = a[cells[0]]
        assert int(a[cells[0]]) not in [int(v) for v in t]
        return [a, t, mult], pcs_replay.q_mul(alpha, [int(a[cells[0]]), 0, 0, 0])

    cols1, z1 = columns(11, [37, 50])
    cols2, z2 = columns(31, [12, 37])
    assert logup_model.generate(program.code, cols1, [0, 0, 0], [z1, alpha], log_size)[2] == [(37, 1), (37, 2), (50, 1), (50, 2)]
    good = _quads(22, 1)[0]
    mk = lambda cols, z: Item(pkg, log_size, program=program, case=(program.code, np.stack(cols), [z, alpha]))
    with Dev(ctx) as dev:
        def run(items):
            entries = [(it.program, it.log_size, [dev.up(c) for c in it.cols], it.params, [dev.empty(n) for _ in range(8)]) for it in items]
            return ctx.logup_program_generate_batch(entries)
        for items in ([mk(cols2, good), mk(cols1, z1), mk(cols2, good)], [mk(cols2, good), mk(cols1, z1), mk(cols2, z2)]):
            with pytest.raises(pkg.BfhipError) as e:
                run(items)
            assert str(e.value) == ME + ": component 1: fraction 1 has a zero denominator at cell 37"
            assert pkg.lib().bfhip_last_error().decode() == str(e.value)
        with pytest.raises(pkg.BfhipError) as e:
            run([mk(cols2, z2), mk(cols1, z1)])
        assert str(e.value) == ME + ": component 0: fraction 1 has a zero denominator at cell 12"
    _both(ctx, [mk(cols2, good), mk(cols1, good), mk(cols2, _quads(23, 1)[0])])


# ---- 11. while a session is open -------------------------------------------------------------------------------------------------------------------
def test_batch_inside_an_open_session(_ctx, pkg):
    """Between a session's commit and its prove_values: bfhip_ctx_memory out[3] (arena bytes in use) does not move, the batch is exact, and
    the session's proof is byte for byte that of a run without the batch in between."""
    ctx, log_size = _ctx, 8
    ctx.set_pcs_config(pkg.PcsConfig())
    items = [Item(pkg, log_size, seed=9), Item(pkg, 5, seed=10), Item(pkg, log_size, 1, 1, seed=11)]
    trace = items[0].cols

    def session(between):
        with Dev(ctx) as dev:
            ch = pkg.Channel((0, 0, 0, 0))
            with pkg.PcsSession(ctx) as s:
                s.commit(ch, [dev.up(c) for c in trace], [log_size] * len(trace), form=0)
                seen = between()
                oods = ch.draw_point()
                return s.prove_values(ch, [oods], [[[0]] * len(trace)]), seen

    def batch():
        before = ctx.memory()["arena_in_use"]
        _both(ctx, items)
        return before, ctx.memory()["arena_in_use"]

    plain, _ = session(lambda: None)
    proof, (before, after) = session(batch)
    assert before == after and before > 0
    assert len(proof) > 0 and proof == plain


# ---- 12. determinism --------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_leave_identical_bytes(_ctx, pkg):
    ctx = _ctx
    items = [Item(pkg, log, seed=3 * k) for k, log in enumerate([12, 3, 7, 12])]
    with Dev(ctx) as dev:
        src = [[dev.up(c) for c in it.cols] for it in items]
        runs = []
        for fill in (0, 0xFFFFFFFF):
            outs = [[dev.up(np.full(1 << it.log_size, fill, dtype=np.uint32)) for _ in range(it.n_out)] for it in items]
            res = ctx.logup_program_generate_batch([(it.program, it.log_size, s, it.params, o) for it, s, o in zip(items, src, outs)])
            runs.append((res, [ctx.download(p, 1 << it.log_size).tobytes() for it, o in zip(items, outs) for p in o]))
    assert runs[0] == runs[1]


# ---- 13. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_and_the_context_as_they_were(_ctx, pkg):
    ctx, log_size, n = _ctx, 5, 32
    abi = sys.modules[pkg.__name__ + "._abi"].abi
    b = pkg.AirBuilder()
    a, t, mult, z, alpha = b.col(0), b.col(1), b.col(2), b.param(0), b.param(1)
    b.frac(1, alpha * a - z); b.end_column(); b.frac(-mult, alpha * t - z); b.end_column()
    program = b.logup_program()
    cols = [splitmix_column((31 + k) << 32, n) for k in range(3)]
    params = _quads(33, 2)
    with Dev(ctx) as dev:
        src = [[dev.up(c) for c in cols] for _ in range(2)]
        dst = [[dev.up(np.full(n, SENTINEL, dtype=np.uint32)) for _ in range(8)] for _ in range(2)]
        big = dev.up(np.full(2 * n, SENTINEL, dtype=np.uint32))      # 256 bytes: an input over its first half, an output over its middle
        g = [(program, log_size, src[k], params, dst[k]) for k in range(2)]

        def with_(k=0, **kw):
            d = dict(log_size=log_size, cols=src[k], params=params, dst=dst[k], shifts=None)
            d.update(kw)
            return (program, d["log_size"], d["cols"], d["params"], d["dst"], d["shifts"])

        def untouched():
            assert all((ctx.download(p, n) == SENTINEL).all() for k in range(2) for p in dst[k]) and (ctx.download(big, 2 * n) == SENTINEL).all()

        why = r" \(every output column is written while other components still read and write theirs\)$"
        for entries, what in (
                ([], r"^%s: 1 to BFHIP_LOGUP_BATCH_MAX_COMPONENTS \(64\) components, got 0$" % ME),
                ([g[0]] * 65, r"^%s: 1 to BFHIP_LOGUP_BATCH_MAX_COMPONENTS \(64\) components, got 65$" % ME),
                ([g[0], with_(1, log_size=0)], r"^%s: component 1: log_size must be in \[1, max_log_domain = %d\], got 0$" % (ME, ctx.max_log_domain)),
                ([with_(log_size=ctx.max_log_domain + 1)], r"^%s: component 0: log_size must be in \[1, max_log_domain = %d\], got %d$" % (ME, ctx.max_log_domain, ctx.max_log_domain + 1)),
                ([with_(shifts=[0, 1, 0])], r"^%s: component 0: column 1 has shift 1 \(0, or 2 \.\. log_size\)$" % ME),
                ([g[0], with_(1, shifts=[0, 6, 0])], r"^%s: component 1: column 1 has shift 6 \(0, or 2 \.\. log_size\)$" % ME),
                ([with_(params=params[:1])], r"^%s: component 0: the program takes 2 parameters, got 1$" % ME),
                ([g[0], with_(1, params=[params[0], [P, 0, 0, 0]])], r"^%s: component 1: a parameter word is not a canonical M31$" % ME),
                ([with_(dst=dst[0][:7] + [0])], r"^%s: component 0: null output column pointer \(coordinate column 7\)$" % ME),
                ([g[0], with_(1, cols=[src[1][0], 0, src[1][2]])], r"^%s: component 1: null column pointer \(column 1\)$" % ME),
                # an output of component 0 is an input of component 1; is an output of component 1 too; is given twice by component 0
                ([g[0], with_(1, cols=[src[1][0], dst[0][3], src[1][2]])], r"^%s: an output column of component 0 overlaps an input column of component 1" % ME + why),
                ([g[0], with_(1, dst=dst[1][:5] + [dst[0][2]] + dst[1][6:])], r"^%s: an output column of component 0 overlaps an output column of component 1" % ME + why),
                ([with_(dst=dst[0][:7] + [dst[0][0]])], r"^%s: an output column of component 0 overlaps an output column of component 0" % ME + why),
                # ranges that share 64 bytes, not a pointer: an input [0, 128) of component 0, an output [64, 192) of component 1
                ([with_(cols=[big, src[0][1], src[0][2]]), with_(1, dst=[big + 64] + dst[1][1:])], r"^%s: an input column of component 0 overlaps an output column of component 1" % ME + why),
                # the same input and an output 32 bytes into it (the accepted twin of this case, at shift 2, closes the test)
                ([with_(cols=[big, src[0][1], src[0][2]]), with_(1, dst=[big + 32] + dst[1][1:])], r"^%s: an input column of component 0 overlaps an output column of component 1" % ME + why)):
            with pytest.raises(pkg.BfhipError, match=what):
                ctx.logup_program_generate_batch(entries)
            assert pkg.lib().bfhip_last_error().decode().startswith(ME + ": ")
            untouched()

        # the struct itself: reserved, null members, null arguments
        entry, claimed, total = abi().bfhip_logup_program_generate_batch, (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 4)()
        pars = (ctypes.c_uint32 * 8)(*[w for q in params for w in q])
        cp = [(ctypes.c_void_p * 3)(*src[k]) for k in range(2)]
        op = [(ctypes.c_void_p * 8)(*dst[k]) for k in range(2)]
        vpp = lambda arr: ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
        make = lambda k=0, **kw: pkg.LogupComponent(**{**dict(program=program._h.value, log_size=log_size, n_params=2, cols_h=vpp(cp[k]), col_shifts_h=None, params_h=pars,
                                                              out_cols_h=vpp(op[k]), reserved=0), **kw})
        arr = lambda *cs: (pkg.LogupComponent * len(cs))(*cs)

        def refused(rc, what):
            assert rc == -1 and abi().bfhip_last_error().decode() == what, abi().bfhip_last_error().decode()
            untouched()

        refused(entry(ctx._h, arr(make(), make(1, reserved=1)), 2, claimed, total), ME + ": component 1: reserved must be 0")
        refused(entry(ctx._h, arr(make(reserved=1 << 32)), 1, claimed, total), ME + ": component 0: reserved must be 0")
        refused(entry(ctx._h, arr(make(program=None)), 1, claimed, total), ME + ": component 0: null argument")
        refused(entry(ctx._h, arr(make(), make(1, cols_h=None)), 2, claimed, total), ME + ": component 1: null argument")
        refused(entry(ctx._h, arr(make(params_h=None)), 1, claimed, total), ME + ": component 0: null argument")
        refused(entry(ctx._h, arr(make(out_cols_h=None)), 1, claimed, total), ME + ": component 0: null argument")
        refused(entry(ctx._h, None, 1, claimed, total), ME + ": null argument")
        refused(entry(ctx._h, arr(make()), 1, None, total), ME + ": null argument")
        refused(entry(ctx._h, arr(make()), 0, claimed, total), ME + ": 1 to BFHIP_LOGUP_BATCH_MAX_COMPONENTS (64) components, got 0")
        refused(entry(ctx._h, arr(make()), 65, claimed, total), ME + ": 1 to BFHIP_LOGUP_BATCH_MAX_COMPONENTS (64) components, got 65")      # on the count alone
        # a member of a shard group
        group, member = pkg.LocalGroup(2), pkg.Context(0, max_log_domain=10)
        try:
            member.join_local_group(group, 0)
            with pytest.raises(pkg.BfhipError, match=r"^%s: a context in a shard group is not supported \(bfhip_ctx_leave_group first\)$" % ME):
                member.logup_program_generate_batch(g)
            member.leave_group()
        finally:
            member.close(); group.close()
        untouched()
        # more than 2^31 cells: 33 components of 2^26. Refused before anything is read or enqueued, so the columns are addresses only.
        wide, one = pkg.Context(0, max_log_domain=26), Item(pkg, 4, 1, 1)
        try:
            at = lambda k, j: (1 << 44) + ((6 * k + j) << 30)
            many = [(one.program, 26, [at(k, 0), at(k, 1)], one.params, [at(k, 2 + j) for j in range(4)]) for k in range(33)]
            with pytest.raises(pkg.BfhipError, match=r"^%s: the list has %d cells, a call takes at most 2\^31 = 2147483648$" % (ME, 33 << 26)):
                wide.logup_program_generate_batch(many)
        finally:
            wide.close()

        # total_h may be NULL; an input at shift 2 that ends at the byte where an output begins is accepted. Both are the single call's words.
        want = [dev.empty(n) for _ in range(8)]
        assert entry(ctx._h, arr(make()), 1, claimed, None) == 0
        assert list(claimed)[:4] == ctx.logup_program_generate(program, log_size, src[0], params, want)
        assert all(np.array_equal(ctx.download(p, n), ctx.download(w, n)) for p, w in zip(dst[0], want))
        stored = cols[0][: n >> 2]
        edge = dev.up(np.concatenate([stored, np.full(2 * n - len(stored), SENTINEL, dtype=np.uint32)]))      # input: bytes [0, 32); output: [32, 160)
        got_claimed, got_total = ctx.logup_program_generate_batch([(program, log_size, [edge] + src[0][1:], params, [edge + 32] + dst[0][1:], [2, 0, 0])])
        want_claimed = ctx.logup_program_generate(program, log_size, [dev.up(stored)] + src[0][1:], params, want, col_shifts=[2, 0, 0])
        assert got_claimed == [want_claimed] and got_total == want_claimed
        assert np.array_equal(ctx.download(edge + 32, n), ctx.download(want[0], n)) and np.array_equal(ctx.download(edge, len(stored)), stored)
        assert all(np.array_equal(ctx.download(p, n), ctx.download(w, n)) for p, w in zip(dst[0][1:], want[1:]))
