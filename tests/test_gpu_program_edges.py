"""-m gpu: the two program interpreters (k_air_program of csrc/air_program.hip, k_logup_program of csrc/logup_program.hip) at the inputs the
parity modules test_gpu_air_program.py / test_gpu_logup_program.py never feed them: random programs of tests/air_model.py with offsets up to
+-16 on domains of 4 to 4096 rows, storage shifts 0, 2, 3, 4 and log_size + log_expand (a one-cell column), four different shifts under one
Q_COL, saturated cells / parameters / coefficients, the lazy-reduction schedule of C_BASE driven to its bound, the final m_add at
acc + r == P, the register files at their caps (96 M + 24 Q = 48 KiB of LDS) and with one file absent, 64 interleaved constraints on the one
coefficient index; for the fraction program the longest fold chain (32 fractions in one column) and eight columns of one fraction.

Every comparison is bit-exact. The expected accumulator is (acc0 + model.run(...) * domain_denominators) mod P from tests/air_model.py (numpy
and Python integers, pinned on the CPU by tests/test_air_program_cpu.py against the host evaluator), or tests/logup_model.py, or a closed form;
never a launch of the code under test. Columns are plain full-size arrays: the kernel is row-local, so no LDE is needed.

Mutation runs (arithmetic-only changes on a scratch copy, one at a time): see MUTATIONS below."""
import numpy as np
import pytest

import air_model
import field_inputs as fi
import logup_model
from air_model import M_COL, Q_COL, Q_PARAM, Q_MUL, C_BASE, C_EXT
from conftest import splitmix_column, P

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

# Arithmetic-only mutations (a value or a condition on values; never an address, an index, a bound or a launch shape), each built on a scratch
# copy and run once on an MI355X against this module ("new") and the older module of that kernel ("old": test_gpu_air_program.py /
# test_gpu_logup_program.py):
MUTATIONS = """
1 air_program.hip AIR_C_BASE        pending == 4 -> 5    new: caught, test_base_constraint_dot_products_at_their_bound in all 12 cases (k = 5, 9, 64 and
  5, 9, 32 with C_EXT between, coefficients max and heavy_powers) and test_saturated_values_match_the_model x max, edge columns at both shapes
  (zero and sparse columns pass: their products are small)                                                                       old: missed (35 passed)
2 air_program.hip final m_add x 4   a local add returning P at sum == P    new: caught, test_accumulator_sums_of_exactly_p_and_p_minus_one at both
  shapes, and by nothing else: no other input, saturated ones included, makes acc + r land on exactly P                          old: missed (35 passed)
3 logup_program.hip LOGUP_FRAC      fd = q_mul(fd, den) -> q_mul(den, den)    new: caught, test_fraction_fold_chain_extremes_match_the_model 1x32 at both
  sizes and test_fraction_fold_chain_of_32_at_saturated_values at both (8x1 passes, as it must: a column of one fraction never folds)
  old: caught too, by 16 tests (every column of two or more fractions differs: after the second fraction fd is den2^2, not den1 den2)
"""

_P = np.uint64(P)
_DEN = {}


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


def _den(log_size, log_expand):
    if (log_size, log_expand) not in _DEN:
        _DEN[(log_size, log_expand)] = air_model.from_m(air_model.domain_denominators(log_size, log_expand))
    return _DEN[(log_size, log_expand)]


def _quads(family, seed, n):
    """n QM31 values (4 words each) of a constant family of tests/field_inputs.py"""
    return fi.const(family, seed, 4 * n).reshape(n, 4).tolist() if n else []


def _cols(family, seed, k, n):
    if family == "zero":
        return np.zeros((k, n), dtype=np.uint32)
    return np.stack(fi.columns(family, seed, k, n))


def _acc0(family, seed, n):
    return np.stack([fi.column(family, seed + 1000 * k, n) for k in range(4)])


def _model_sum(code, full_cols, log_size, log_expand, params, coeffs):
    """(sum_j coeff_j C_j) / vanishing per row as (4, n) uint64"""
    n = 1 << (log_size + log_expand)
    r = air_model.run(code, air_model.domain_reader(full_cols, log_size, log_expand), params, coeffs, n)
    return air_model.q_mul(r, _den(log_size, log_expand))


def _expected(code, full_cols, log_size, log_expand, params, coeffs, acc0):
    return ((_model_sum(code, full_cols, log_size, log_expand, params, coeffs) + acc0.astype(np.uint64)) % _P).astype(np.uint32)


class Launch:
    """One program's columns on the device, stored at `shifts` (column k holds every 2^shift-th cell of its full-size expansion: the model
    reads the np.repeat expansion, the kernel the stored cells); run() launches from an accumulator and returns the (4, n) result."""

    def __init__(self, ctx, pkg, code, n_cols, n_params, log_size, log_expand, stored, shifts=None):
        self.ctx, self.program = ctx, pkg.AirProgram(code, n_cols, n_params)
        self.log_size, self.log_expand, self.n = log_size, log_expand, 1 << (log_size + log_expand)
        self.stored, self.shifts = stored, shifts
        for k, c in enumerate(stored):
            assert len(c) == self.n >> (shifts[k] if shifts else 0)

    def run(self, params, coeffs, acc0):
        with Dev(self.ctx) as dev:
            cols = [dev.up(c) for c in self.stored]
            acc = [dev.up(acc0[k]) for k in range(4)]
            self.ctx.air_eval_domain(self.program, self.log_size, self.log_expand, cols, params, coeffs, acc, col_shifts=self.shifts)
            return np.stack([self.ctx.download(p, self.n) for p in acc])


def _check(got, want, what):
    d = np.nonzero(got != want)
    assert d[0].size == 0, (what, "first differing (word, row)", (int(d[0][0]), int(d[1][0])), "got", int(got[d[0][0], d[1][0]]), "want", int(want[d[0][0], d[1][0]]))


# ---- a. random programs at the shapes where paths change ----------------------------------------------------------------------------------
# (log_size, log_expand): 4 rows = the smallest domain; (1, 3): 16 rows of a 2-row trace, every offset wraps several times; 64 rows = exactly one
# wave; 32 = half a wave; 128 = two workgroups; 4096 = 64 workgroups
SHAPES = [(1, 1), (1, 3), (2, 2), (3, 3), (4, 1), (5, 2), (9, 3)]
SEEDS = [301, 340, 362]           # random_program(seed, max_off=16): offsets -12 .. 16, -16 .. 16, -16 .. 16
WIDE = (303, 24)                  # 24 columns: a Q_COL at offset 0 whose four coordinate columns are read at no other offset


def _random_program(seed, n_cols=9):
    return air_model.random_program(seed, n_cols=n_cols, max_off=16)


def test_the_random_programs_reach_both_extreme_offsets(pkg):
    shapes = [pkg.AirProgram(*_random_program(seed)[:3]).shape for seed in SEEDS]
    assert min(s["min_offset"] for s in shapes) == -16 and max(s["max_offset"] for s in shapes) == 16
    assert any(s["min_offset"] == -16 and s["max_offset"] == 16 for s in shapes)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("log_size,log_expand", SHAPES, ids=["%d+%d" % s for s in SHAPES])
def test_random_programs_match_the_model(_ctx, pkg, log_size, log_expand, seed):
    code, n_cols, n_params, n_cons = _random_program(seed)
    n = 1 << (log_size + log_expand)
    cols = _cols("uniform", (seed << 32) + n, n_cols, n)
    params, coeffs, acc0 = _quads("uniform", seed + 1, n_params), _quads("uniform", seed + 2, n_cons), _acc0("uniform", seed + 3, n)
    assert acc0.any()
    got = Launch(_ctx, pkg, code, n_cols, n_params, log_size, log_expand, cols).run(params, coeffs, acc0)
    _check(got, _expected(code, cols, log_size, log_expand, params, coeffs, acc0), (seed, log_size, log_expand))


# ---- b. storage shifts ---------------------------------------------------------------------------------------------------------------------
def _shifted_storage(program, full_cols, el, phase):
    """Every column program.mask() reads at offset 0 only gets the next shift of the cycle 0, 2, 3, 4, el (starting at `phase`); a column read
    at a non-zero offset stays at shift 0. Returns (stored columns, shifts, the full-size columns the model reads)."""
    at_offset = {c for c, off in program.mask() if off != 0}
    cycle, shifts, k = [0, 2, 3, 4, el], [], phase
    for c in range(len(full_cols)):
        if c in at_offset:
            shifts.append(0)
        else:
            shifts.append(cycle[k % 5])
            k += 1
    stored = [col[: len(col) >> s] for col, s in zip(full_cols, shifts)]      # distinct cells; the expansion repeats each 2^s times
    expanded = np.stack([np.repeat(c, 1 << s) for c, s in zip(stored, shifts)])
    return stored, shifts, expanded


@pytest.mark.parametrize("seed,n_cols", [(s, 9) for s in SEEDS] + [WIDE])
@pytest.mark.parametrize("log_size,log_expand", [(3, 3), (5, 2)], ids=["3+3", "5+2"])
def test_storage_shifts_match_the_model(_ctx, pkg, log_size, log_expand, seed, n_cols):
    code, n_cols, n_params, n_cons = _random_program(seed, n_cols)
    el = log_size + log_expand
    n = 1 << el
    full = _cols("uniform", (seed << 32) + 77 + n, n_cols, n)
    params, coeffs, acc0 = _quads("uniform", seed + 4, n_params), _quads("uniform", seed + 5, n_cons), _acc0("uniform", seed + 6, n)
    program = pkg.AirProgram(code, n_cols, n_params)
    seen = set()
    for phase in range(5):          # every shiftable column meets every shift of the cycle
        stored, shifts, expanded = _shifted_storage(program, full, el, phase)
        seen |= set(shifts)
        if (seed, n_cols) == WIDE:
            q_cols = [code[i + 2] for i in range(0, len(code), 4) if code[i] == Q_COL and code[i + 3] == 0]
            four = [sorted(shifts[a: a + 4]) for a in q_cols]
            assert any(len(set(f)) == 4 for f in four), "a Q_COL over four different shifts"
            assert phase != 0 or [2, 3, 4, el] in four
        got = Launch(_ctx, pkg, code, n_cols, n_params, log_size, log_expand, stored, shifts).run(params, coeffs, acc0)
        _check(got, _expected(code, expanded, log_size, log_expand, params, coeffs, acc0), (seed, phase, shifts))
    if (seed, n_cols) in ((301, 9), WIDE):
        assert seen == {0, 2, 3, 4, el}


# ---- c. saturated values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["max", "zero", "edge", "sparse"])
@pytest.mark.parametrize("log_size,log_expand", [(3, 3), (5, 2)], ids=["3+3", "5+2"])
def test_saturated_values_match_the_model(_ctx, pkg, log_size, log_expand, family):
    """Cells all P - 1, all zero, the edge set, one-hot; parameters max / edge / uniform crossed with coefficients max / edge / uniform / heavy
    (every coefficient (HEAVY_ROOT, 0, 0, 0)); the starting accumulator uniform and all P - 1."""
    n = 1 << (log_size + log_expand)
    for seed in SEEDS[1:]:
        code, n_cols, n_params, n_cons = _random_program(seed)
        cols = _cols(family, seed, n_cols, n)
        launch = Launch(_ctx, pkg, code, n_cols, n_params, log_size, log_expand, cols)
        accs = {f: _acc0(f, seed + 7, n) for f in ("uniform", "max")}
        for fp in ("max", "edge", "uniform"):
            params = _quads(fp, seed + 8, n_params)
            for fc in ("max", "edge", "uniform", "heavy"):
                coeffs = _quads(fc, seed + 9, n_cons)
                r = _model_sum(code, cols, log_size, log_expand, params, coeffs)
                for fa, acc0 in accs.items():
                    _check(launch.run(params, coeffs, acc0), ((r + acc0) % _P).astype(np.uint32), (seed, family, fp, fc, fa))


# ---- d. the fold schedule of C_BASE, directed -----------------------------------------------------------------------------------------------
def _base_chain(k, with_ext):
    """k base constraints, constraint j = column j (M_COL into a register of its own, C_BASE); with_ext: C_EXT of parameter 0 after every
    base constraint but the last — the base products that share the 64-bit accumulators are the same, the coefficient index interleaves."""
    code = []
    for j in range(k):
        code += [M_COL, j, j, 0, C_BASE, 0, j, 0]
        if with_ext and j + 1 < k:
            code += [Q_PARAM, j % 24, 0, 0, C_EXT, 0, j % 24, 0]
    return code, k, 1 if with_ext else 0, k + (k - 1 if with_ext else 0)


def _heavy_powers(n):
    """(HEAVY_ROOT^(j + 1), 0, 0, 0): r .. r^5 all exceed 0.85 P (tests/field_inputs.py), so five products with cells P - 1 pass 2^64"""
    return [[pow(fi.HEAVY_ROOT, j + 1, P), 0, 0, 0] for j in range(n)]


# Without C_EXT k reaches the cap of 64 constraints; with one between every two base constraints 32 + 31 = 63 is the longest that fits it.
CHAINS = [(5, False), (9, False), (64, False), (5, True), (9, True), (32, True)]


@pytest.mark.parametrize("coeff_family", ["max", "heavy_powers"])
@pytest.mark.parametrize("k,with_ext", CHAINS, ids=["%d%s" % (k, "_ext" if e else "") for k, e in CHAINS])
def test_base_constraint_dot_products_at_their_bound(_ctx, pkg, k, with_ext, coeff_family):
    """Cells P - 1 under coefficient words P - 1: every product is (P - 1)^2, four of them on a folded accumulator are the most 64 bits
    hold (4 (P - 1)^2 + 2^34 < 2^64 < 5 (P - 1)^2), so a fold that comes one product late is wrong on every row. k = 5 is the first length
    with a fold, 9 the first with two, 64 the cap."""
    log_size, log_expand = 3, 3
    n = 1 << (log_size + log_expand)
    assert 4 * (P - 1) ** 2 + (1 << 34) < 1 << 64 < 5 * (P - 1) ** 2
    code, n_cols, n_params, n_cons = _base_chain(k, with_ext)
    cols = _cols("max", 0, n_cols, n)
    coeffs = _quads("max", 0, n_cons) if coeff_family == "max" else _heavy_powers(n_cons)
    params = _quads("max", 0, n_params)
    acc0 = _acc0("uniform", 40 + k, n)
    got = Launch(_ctx, pkg, code, n_cols, n_params, log_size, log_expand, cols).run(params, coeffs, acc0)
    _check(got, _expected(code, cols, log_size, log_expand, params, coeffs, acc0), (k, with_ext, coeff_family))
    if not with_ext:
        # closed form over Python integers: (P - 1) c = -c, so the sum is -(c_0 + .. + c_(k-1)) word by word (the cell is a base-field value)
        den = air_model.domain_denominators(log_size, log_expand).tolist()
        total = [(-sum(c[w] for c in coeffs)) % P for w in range(4)]
        want = np.array([[(int(acc0[w][row]) + total[w] * den[row]) % P for row in range(n)] for w in range(4)], dtype=np.uint32)
        _check(got, want, ("closed form", k, coeff_family))


# ---- e. exact cancellation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_size,log_expand", [(3, 3), (5, 2)], ids=["3+3", "5+2"])
def test_accumulator_sums_of_exactly_p_and_p_minus_one(_ctx, pkg, log_size, log_expand):
    """From a zero accumulator the launch leaves r; from (P - r) mod P the final m_add meets acc + r == P on every row with r != 0 and must
    leave the zero word, not P; from (P - 1 - r) mod P every word is P - 1."""
    seed = SEEDS[1]
    code, n_cols, n_params, n_cons = _random_program(seed)
    n = 1 << (log_size + log_expand)
    cols = _cols("uniform", (seed << 32) + 5 + n, n_cols, n)
    params, coeffs = _quads("uniform", seed + 11, n_params), _quads("uniform", seed + 12, n_cons)
    r = _model_sum(code, cols, log_size, log_expand, params, coeffs)
    assert np.count_nonzero(r) > 3 * n      # the sum that is exactly P needs r != 0
    launch = Launch(_ctx, pkg, code, n_cols, n_params, log_size, log_expand, cols)
    _check(launch.run(params, coeffs, np.zeros((4, n), dtype=np.uint32)), r.astype(np.uint32), "from zero")
    got = launch.run(params, coeffs, ((_P - r) % _P).astype(np.uint32))
    assert not got.any(), ("acc + r == P must give 0", np.unique(got).tolist()[:4])
    got = launch.run(params, coeffs, ((_P - np.uint64(1) + _P - r) % _P).astype(np.uint32))
    assert np.all(got == P - 1), ("acc + r == P - 1", np.unique(got).tolist()[:4])


# ---- f. caps and degenerate register files --------------------------------------------------------------------------------------------------
_CAPS = {}


def _caps_program():
    if not _CAPS:
        _CAPS["p"] = air_model.random_program(7, n_cols=256, n_params=64, n_ops=3900, m_pool=96, q_pool=24, max_off=16, max_cons=64)
    return _CAPS["p"]


@pytest.mark.parametrize("log_size,log_expand", [(4, 2), (4, 3)], ids=["4+2", "4+3"])
def test_register_files_at_their_caps(_ctx, pkg, log_size, log_expand):
    """96 M + 24 Q registers = 48 KiB of LDS (the last Q word of lane 63 is word 12287 of 12288), 256 columns, 64 parameters, 64 constraints
    of both kinds on the one coefficient index, some 3400 instructions, offsets -16 .. 16; on one full wave and on two workgroups."""
    code, n_cols, n_params, n_cons = _caps_program()
    n = 1 << (log_size + log_expand)
    cols = _cols("uniform", (9 << 32) + n, n_cols, n)
    params, coeffs, acc0 = _quads("uniform", 21, n_params), _quads("uniform", 22, n_cons), _acc0("uniform", 23, n)
    launch = Launch(_ctx, pkg, code, n_cols, n_params, log_size, log_expand, cols)
    s = launch.program.shape
    assert s["m_regs"] == 96 and s["q_regs"] == 24 and s["n_constraints"] == 64 and 3000 <= s["n_instr"] <= 4096, s
    assert (s["min_offset"], s["max_offset"]) == (-16, 16)
    kinds = [code[i] for i in range(0, len(code), 4) if code[i] >= C_BASE]
    assert C_BASE in kinds and C_EXT in kinds and any(a != b for a, b in zip(kinds, kinds[1:]))      # interleaved
    _check(launch.run(params, coeffs, acc0), _expected(code, cols, log_size, log_expand, params, coeffs, acc0), "caps")


DEGENERATE = {
    # no Q register: the Q file has no words; the last M register of the 96
    "no_q": ([M_COL, 0, 0, 3, C_BASE, 0, 0, 0, M_COL, 95, 1, (-5) & 0xFFFFFFFF, C_BASE, 0, 95, 0], 2, 0),
    # no M register: the Q file starts at LDS word 0; the last Q register of the 24
    "no_m": ([Q_PARAM, 0, 1, 0, Q_COL, 23, 0, 7, Q_MUL, 1, 0, 23, C_EXT, 0, 1, 0, Q_COL, 0, 1, 0, C_EXT, 0, 0, 0, C_EXT, 0, 23, 0], 5, 2),
}


@pytest.mark.parametrize("which", list(DEGENERATE))
@pytest.mark.parametrize("log_size,log_expand", [(4, 2), (4, 3)], ids=["4+2", "4+3"])
def test_a_program_with_one_register_file_only(_ctx, pkg, log_size, log_expand, which):
    code, n_cols, n_params = DEGENERATE[which]
    n = 1 << (log_size + log_expand)
    n_cons = sum(1 for i in range(0, len(code), 4) if code[i] >= C_BASE)
    for family in ("uniform", "max"):
        cols = _cols(family, (3 << 32) + n, n_cols, n)
        params, coeffs, acc0 = _quads(family, 31, n_params), _quads(family, 32, n_cons), _acc0("uniform", 33, n)
        launch = Launch(_ctx, pkg, code, n_cols, n_params, log_size, log_expand, cols)
        s = launch.program.shape
        assert (s["m_regs"], s["q_regs"]) == ((96, 0) if which == "no_q" else (0, 24)), s
        _check(launch.run(params, coeffs, acc0), _expected(code, cols, log_size, log_expand, params, coeffs, acc0), (which, family))


# ---- the fraction program: the longest fold chain, and eight columns of one fraction -------------------------------------------------------
def _generate(ctx, program, log_size, cols, params):
    n = 1 << log_size
    with Dev(ctx) as dev:
        src = [dev.up(c) for c in cols]
        dst = [dev.empty(n) for _ in range(4 * program.shape["n_logup_cols"])]
        claimed = ctx.logup_program_generate(program, log_size, src, params, dst)
        return np.stack([ctx.download(p, n) for p in dst]), claimed


LOGUP_SHAPES = [(1, 32), (8, 8)]


@pytest.mark.parametrize("log_size", [6, 7])
@pytest.mark.parametrize("n_logup,n_fractions", LOGUP_SHAPES, ids=["1x32", "8x1"])
def test_fraction_fold_chain_extremes_match_the_model(_ctx, pkg, n_logup, n_fractions, log_size):
    """All 32 fractions in one column: fn / fd is folded 31 times before the column's single inversion. Eight columns of one fraction each:
    no fold at all, an inversion per column."""
    code, n_cols, n_params = logup_model.random_program(1000 * n_fractions + log_size, n_logup, n_fractions)
    cols = np.stack([splitmix_column(((k + 1) << 32) + log_size, 1 << log_size) for k in range(n_cols)])
    params = _quads("uniform", 600 + log_size, n_params)
    program = pkg.LogupProgram(code, n_cols, n_params)
    assert (program.shape["n_logup_cols"], program.shape["n_fractions"]) == (n_logup, n_fractions)
    per_col = [c.count(logup_model.FRAC) for c in _split_columns(code)]
    assert per_col == ([32] if n_logup == 1 else [1] * 8)
    want, want_claimed, zeros = logup_model.generate(code, cols, [0] * n_cols, params, log_size)
    assert zeros == []
    got, claimed = _generate(_ctx, program, log_size, cols, params)
    assert claimed == want_claimed
    _check(got, want, (n_logup, n_fractions, log_size))


def _split_columns(code):
    """opcodes per logUp column"""
    out, cur = [], []
    for i in range(0, len(code), 4):
        cur.append(code[i])
        if code[i] == logup_model.END_COL:
            out.append(cur)
            cur = []
    return out


@pytest.mark.parametrize("log_size", [6, 7])
def test_fraction_fold_chain_of_32_at_saturated_values(_ctx, pkg, log_size):
    """The 32-fraction column on cells of the edge set with every parameter word P - 1; seed 0 of this family has no zero denominator."""
    code, n_cols, n_params = logup_model.random_program(32000, 1, 32)
    cols = np.stack([fi.edge(k, 1 << log_size) for k in range(n_cols)])
    params = [[P - 1] * 4] * n_params
    want, want_claimed, zeros = logup_model.generate(code, cols, [0] * n_cols, params, log_size)
    assert zeros == [], "the test's seed must keep every denominator non-zero"
    got, claimed = _generate(_ctx, pkg.LogupProgram(code, n_cols, n_params), log_size, cols, params)
    assert claimed == want_claimed
    _check(got, want, ("edge", log_size))
