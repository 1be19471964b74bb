"""Shared by tests/test_air_check_cpu.py and tests/test_gpu_air_check_edges.py: the cases that put bfhip_air_check (csrc/air_check.hip) where
its wave reduction, its sink and its row policy can go wrong — "defect" programs whose constraints fail at chosen cells (partial ballots),
the register caps, storage shifts with violations inside a shift group, algebraic identities at saturated field values with their
off-by-one twins, extension values that are non-zero in one coordinate, and a first violation whose lowest failing constraint is not
constraint 0. Programs are plain bytecode (include/bfhip.h "Constraint programs"), traces are numpy arrays, and the expected report is
tests/air_check_model.py's: nothing here needs the library or a GPU. The CPU module asserts, on the model alone, that each case contains
what it was built for; the GPU module compares the kernel with the model on the same objects.

A Case is built once per process and keeps its model report."""
import random

import numpy as np

import air_check_model
import air_codegen_cases
import air_model
import field_inputs as fi
from air_model import (M_COL, M_CONST, M_ADD, M_SUB, M_MUL, M_NEG, Q_COL, Q_PARAM, Q_FROM_M, Q_ADD, Q_SUB, Q_MUL, Q_MULM, C_BASE, C_EXT)
from conftest import splitmix_column, P

M32 = 0xFFFFFFFF
WAVE = 64
_CACHE = {}


def _cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


class Case:
    """A program, its trace and parameters. full: (n_cols, 2^log_size), what the model reads; stored: what the kernel is given, column k
    holding every 2^shifts[k]-th cell (full must be its expansion). notes: what the builder knows about the case."""

    def __init__(self, code, n_params, log_size, full, params, shifts=None, **notes):
        self.code, self.n_cols, self.n_params, self.log_size = [int(w) & M32 for w in code], len(full), n_params, log_size
        self.full = np.ascontiguousarray(full, dtype=np.uint32)
        assert self.full.shape == (self.n_cols, 1 << log_size) and int(self.full.max(initial=0)) < P
        self.params, self.shifts, self.notes = [[int(w) for w in q] for q in params], shifts, notes
        assert len(self.params) == n_params
        self.stored = [c[:: 1 << s] for c, s in zip(self.full, shifts)] if shifts else list(self.full)
        if shifts:
            assert all(np.array_equal(np.repeat(c, 1 << s), f) for c, s, f in zip(self.stored, shifts, self.full))
        self._model = None

    def _run(self):
        if self._model is None:
            self._model = air_check_model.one_pass(self.code, self.full, self.params, self.log_size)
        return self._model

    @property
    def want(self):
        """the model's report"""
        return self._run()[0]

    @property
    def bad(self):
        """(k, n) bool: constraint j is non-zero at cell c, in the model"""
        return self._run()[1]

    def kinds(self):
        return [self.code[i] for i in range(0, len(self.code), 4) if self.code[i] in (C_BASE, C_EXT)]


def nonzero_column(seed, n):
    v = splitmix_column(seed, n)
    v[v == 0] = 1
    return v


def wave_profile(bad):
    """Of a (k, n) bad matrix, per wave of 64 cells (one wave of n cells below 64): counts[j, w] = cells of wave w at which constraint j
    fails (what popcll of its ballot must give), lowest[j, w] = its lowest failing lane or -1 (ffsll), wave_lowest[w] = the lowest lane
    with any failing constraint or -1."""
    k, n = bad.shape
    per = bad.reshape(k, -1, min(n, WAVE))
    counts = per.sum(axis=2)
    lowest = np.where(counts > 0, per.argmax(axis=2), -1)
    any_bad = per.any(axis=0)
    return counts, lowest, np.where(any_bad.any(axis=1), any_bad.argmax(axis=1), -1)


# ---- 1. defect programs: constraint j = d[c_j][off_j] * g_j ---------------------------------------------------------------------------------
def defect_program(cons):
    """cons: [(C_BASE or C_EXT, defect column, offset, g)], g = ("const", v) or ("col", column, offset) for a base constraint and
    ("param", index) for an extension one; g is non-zero everywhere, so the constraint fails exactly where the defect column, read at the
    offset, is non-zero. Registers walk both files."""
    code = []
    for j, (kind, c, off, g) in enumerate(cons):
        r = (3 * j) % 93
        code += [M_COL, r, c, off & M32]
        if kind == C_BASE:
            code += [M_CONST, r + 1, g[1], 0] if g[0] == "const" else [M_COL, r + 1, g[1], g[2] & M32]
            code += [M_MUL, r + 2, r, r + 1, C_BASE, 0, r + 2, 0]
        else:
            qa = (2 * j) % 23
            code += [Q_PARAM, qa, g[1], 0, Q_MULM, qa + 1, qa, r, C_EXT, 0, qa + 1, 0]
    return code


DEFECT_PARAMS = [[P - 1] * 4, [0, 0, 0, 5], [1, 0, 0, 0], [123456789, 0, P - 2, 7]]      # each non-zero as a QM31 value
N_DEFECT_COLS, N_G_COLS = 8, 4


def defect_columns(log_size, seed):
    """Eight sparse columns. W = the number of waves; with one wave every pattern below sits in it.
    0: all zero                                  1: one cell, lane 37 of the last wave
    2: lanes 5 and 63 of wave 0, and cell 64     3: 33 cells, lanes 31..63 of wave W / 2
    4: 63 cells, lanes 1..63 of wave 0           5: 64 cells, the whole last wave (cell n - 1 included)
    6: every cell with probability 1 / 8         7: every cell with probability 1 / 2
    Non-zero cells hold 1, P - 1 or a random non-zero value."""
    n = 1 << log_size
    waves = max(1, n // WAVE)
    last = (waves - 1) * WAVE
    d = np.zeros((N_DEFECT_COLS, n), dtype=bool)
    d[1, last + 37] = True
    d[2, [5, 63]] = True
    if n > WAVE:
        d[2, 64] = True
    d[3, (waves // 2) * WAVE + 31: (waves // 2) * WAVE + 64] = True
    d[4, 1: 64] = True
    d[5, last: last + 64] = True
    d[6] = splitmix_column(seed + 6, n) % np.uint32(8) == 0
    d[7] = splitmix_column(seed + 7, n) % np.uint32(2) == 0
    values = np.stack([nonzero_column(seed + 100 + k, n) for k in range(N_DEFECT_COLS)])
    pick = np.stack([splitmix_column(seed + 200 + k, n) % np.uint32(4) for k in range(N_DEFECT_COLS)])
    values = np.where(pick == 0, np.uint32(1), np.where(pick == 1, np.uint32(P - 1), values))
    return np.where(d, values, np.uint32(0)).astype(np.uint32)


def defect_cons_64(seed):
    """64 constraints: the first eight read the eight defect columns at offset 0 (the counts of defect_columns reach the waves as they
    are), the other 56 read a random one at every offset of -16..16 but 0 at least once; both kinds interleaved."""
    rng = random.Random(seed)
    offs = [o for o in range(-16, 17) if o] + [rng.randrange(-16, 17) for _ in range(24)]
    rng.shuffle(offs)
    offs = [0] * N_DEFECT_COLS + offs
    cons = []
    for j in range(64):
        kind = C_EXT if rng.random() < 0.5 else C_BASE
        c = j if j < N_DEFECT_COLS else rng.randrange(N_DEFECT_COLS)
        if kind == C_EXT:
            g = ("param", rng.randrange(len(DEFECT_PARAMS)))
        elif rng.random() < 0.5:
            g = ("const", rng.choice([1, P - 1, rng.randrange(1, P)]))
        else:
            g = ("col", N_DEFECT_COLS + rng.randrange(N_G_COLS), rng.choice([0, 0, 1, -3, 16]))
        cons.append((kind, c, offs[j], g))
    return cons


def defect_case(log_size):
    def build():
        n = 1 << log_size
        cons = defect_cons_64(500 + log_size)
        full = np.concatenate([defect_columns(log_size, 1000 * log_size), np.stack([nonzero_column(70 + k + 10 * log_size, n) for k in range(N_G_COLS)])])
        return Case(defect_program(cons), len(DEFECT_PARAMS), log_size, full, DEFECT_PARAMS, cons=cons)
    return _cached(("defect", log_size), build)


BIG_LOG = 20
# (kind, offset, the cells at which the constraint is to fail): each constraint has a defect column of its own, non-zero at the rows those
# cells read. Every cell lies above 2^16; constraint 0 fails once, in the last wave; constraints 3 and 5 share a cell.
BIG_SPEC = [(C_BASE, 0, [(1 << BIG_LOG) - 64 + 17]), (C_EXT, -16, [70001, 70002, 900000]), (C_BASE, 16, [(1 << BIG_LOG) - 1, 65600]),
            (C_EXT, 1, [1 << 19, (1 << 19) + 63, (1 << 19) + 64]), (C_BASE, -1, []), (C_EXT, 5, [(1 << BIG_LOG) - 64, (1 << 19) + 63])]


def defect_case_big():
    def build():
        n = 1 << BIG_LOG
        full = np.zeros((len(BIG_SPEC) + 1, n), dtype=np.uint32)
        full[len(BIG_SPEC)] = nonzero_column(20, n)
        cons = []
        for j, (kind, off, cells) in enumerate(BIG_SPEC):
            rows = air_model.offset_rows(BIG_LOG, 0, off)[cells] if off and cells else np.array(cells, dtype=np.int64)
            full[j, rows] = [(P - 1, 1, 77777)[i % 3] for i in range(len(cells))]
            cons.append((kind, j, off, ("param", j % len(DEFECT_PARAMS)) if kind == C_EXT else ("col", len(BIG_SPEC), 0) if j else ("const", P - 1)))
        return Case(defect_program(cons), len(DEFECT_PARAMS), BIG_LOG, full, DEFECT_PARAMS, cons=cons)
    return _cached("defect_big", build)


def defect_closed_form(case):
    """(bad_per_constraint, first_cell_per_constraint) without an interpreter: the offset map is a permutation, so constraint j fails at as
    many cells as its defect column has non-zero cells, first at the lowest cell whose row at off_j is one of them."""
    maps, counts, firsts = {}, [], []
    for _, c, off, _ in case.notes["cons"]:
        if off not in maps:
            maps[off] = air_model.offset_rows(case.log_size, 0, off) if off else np.arange(1 << case.log_size)
        hit = case.full[c][maps[off]] != 0
        counts.append(int(np.count_nonzero(case.full[c])))
        firsts.append(int(np.argmax(hit)) if hit.any() else None)
    return counts, firsts


def assert_defect_conditions(case):
    """What a 64-constraint defect case must contain, in the model alone, for the kernel's reduction to be exercised: see the asserts."""
    want, bad, n = case.want, case.bad, 1 << case.log_size
    counts, lowest, wave_lowest = wave_profile(bad)
    waves = counts.shape[1]
    kinds = case.kinds()
    offs = [off for _, _, off, _ in case.notes["cons"]]
    assert len(kinds) == 64 and C_BASE in kinds[:32] and C_EXT in kinds[:32] and C_BASE in kinds[32:] and C_EXT in kinds[32:]
    assert any(a != b for a, b in zip(kinds, kinds[1:])) and min(offs) == -16 and max(offs) == 16
    failing = [j for j in range(64) if want["bad_per_constraint"][j]]
    assert min(failing) < 32 <= max(failing) and {kinds[j] for j in failing} == {C_BASE, C_EXT}      # both halves of the lane mask
    assert {1, 2, 33, 63, 64} <= set(counts.ravel().tolist())                                       # partial and full ballots
    assert any(0 in counts[:, w].tolist() for w in range(waves) if wave_lowest[w] >= 0)            # a constraint that fails nowhere in a bad wave
    for w in range(waves):      # in some wave the constraints' lowest lanes differ from each other and from the wave's lowest bad lane
        lows = {int(l) for l in lowest[:, w] if l >= 0}
        if len(lows) >= 3 and any(l != wave_lowest[w] for l in lows):
            break
    else:
        raise AssertionError("no wave with three different lowest lanes")
    assert 0 < want["n_bad_cells"] < sum(want["bad_per_constraint"])      # n_bad_cells is the ballot of the union, not a sum
    assert len(set(want["bad_per_constraint"])) >= 6               # counts differ from constraint to constraint
    firsts = [c for c in want["first_cell_per_constraint"] if c is not None]
    assert None in want["first_cell_per_constraint"]
    assert bad[:, 63].any() and bad[:, n - 1].any()
    if waves > 1:
        assert min(firsts) < WAVE and max(firsts) >= n - WAVE     # one first cell in wave 0, another in the last wave
        assert any(np.count_nonzero(counts[j]) == waves for j in range(64))      # a count that adds up over every wave
        assert bad[:, 64].any()                                    # both sides of a wave's edge


# ---- 2. the caps, and a program with one register file only ----------------------------------------------------------------------------------
CAPS_SEED = 0      # most seeds multiply a zero register into a constraint or two, which then never fail; 0, 8 and 11 are the first that do not


def caps_case(log_size):
    def build():
        code, n_cols, n_params, _ = _cached("caps_program", lambda: air_codegen_cases.caps_program(CAPS_SEED))
        n = 1 << log_size
        full = np.stack(fi.columns("uniform", (11 << 32) + n, n_cols, n))
        params = fi.const("uniform", 12, 4 * n_params).reshape(n_params, 4).tolist()
        return Case(code, n_params, log_size, full, params)
    return _cached(("caps", log_size), build)


# tests/test_gpu_program_edges.py DEGENERATE: (code, n_cols, n_params). no_q: the q file has no words, the last of the 96 m registers is
# used; no_m: the q file starts at LDS word 0, the last of the 24 q registers is used.
ONE_FILE = {
    "no_q": ([M_COL, 0, 0, 3, C_BASE, 0, 0, 0, M_COL, 95, 1, (-5) & M32, C_BASE, 0, 95, 0], 2, 0),
    "no_m": ([Q_PARAM, 0, 1, 0, Q_COL, 23, 0, 7, Q_MUL, 1, 0, 23, C_EXT, 0, 1, 0, Q_COL, 0, 1, 0, C_EXT, 0, 0, 0, C_EXT, 0, 23, 0], 5, 2),
}


def one_file_case(which, log_size):
    """Column k is non-zero where a hash of the row is k mod 8: a row has at most one non-zero column (a Q_COL value is then non-zero in
    one coordinate), and three rows in eight have none."""
    def build():
        code, n_cols, n_params = ONE_FILE[which]
        n = 1 << log_size
        h = splitmix_column(31 + log_size, n) % np.uint32(8)
        full = np.stack([np.where(h == k, nonzero_column(40 + k, n), np.uint32(0)) for k in range(n_cols)])
        return Case(code, n_params, log_size, full, [[P - 1, 1, 0, 5], [3, 0, P - 1, 2]][:n_params])
    return _cached((which, log_size), build)


# ---- 3. storage shifts -------------------------------------------------------------------------------------------------------------------------
def shift_case(log_size):
    """Columns 0..3: base columns stored at shifts 2, 3, 4 and log_size (one cell); 4..7: the coordinates of one Q_COL at four different
    shifts; 8..15: full-size copies of the expansions of 0..7, 16: of the product of columns 0 and 1 — each copy changed at a few cells.
    Constraints: column k minus its copy (k < 4), the Q_COL minus the Q_COL of the copies, column 0 times column 1 minus the product's
    copy. Every stored cell is random, so an index other than cell >> shift fails nearly everywhere; with the right index a constraint
    fails at the changed cells only, which lie inside shift groups whose other cells pass."""
    def build():
        n = 1 << log_size
        shifts = [2, 3, 4, log_size] + ([0, 2, 3, 4] if log_size == 4 else [2, 3, 4, log_size]) + [0] * 9
        expanded = [np.repeat(splitmix_column(900 + 16 * log_size + k, n >> s), 1 << s) for k, s in enumerate(shifts[:8])]
        copies = [e.copy() for e in expanded] + [(expanded[0].astype(np.uint64) * expanded[1] % np.uint64(P)).astype(np.uint32)]
        changed = []
        for k, c in enumerate(copies):
            g = 1 << shifts[k % 8] if shifts[k % 8] else 4
            cells = sorted({v for v in [0, g - 1, g + 1, 63, 64, n - 2, n - 1][k % 2:: 2] if 0 <= v < n})
            c[cells] = (c[cells].astype(np.uint64) + np.uint64(1)) % np.uint64(P)
            changed.append(cells)
        code = []
        for k in range(4):
            code += [M_COL, 3 * k, k, 0, M_COL, 3 * k + 1, 8 + k, 0, M_SUB, 3 * k + 2, 3 * k, 3 * k + 1, C_BASE, 0, 3 * k + 2, 0]
        code += [Q_COL, 0, 4, 0, Q_COL, 1, 12, 0, Q_SUB, 2, 0, 1, C_EXT, 0, 2, 0]
        code += [M_COL, 20, 0, 0, M_COL, 21, 1, 0, M_MUL, 22, 20, 21, M_COL, 23, 16, 0, M_SUB, 24, 22, 23, C_BASE, 0, 24, 0]
        return Case(code, 0, log_size, np.stack(expanded + copies), [], shifts=shifts, changed=changed)
    return _cached(("shift", log_size), build)


def assert_shift_conditions(case):
    want, bad, changed, shifts = case.want, case.bad, case.notes["changed"], case.shifts
    q_cells = sorted(set().union(*changed[4:8]))
    assert len(set(shifts[4:8])) == 4 and shifts[0] != shifts[1] and shifts[3] == case.log_size and set(shifts[:4]) >= {2, 3, 4}
    assert all(len(c) == 1 << (case.log_size - s) and (len(c) == 1 or len(np.unique(c)) > 1) for c, s in zip(case.stored, shifts))      # non-constant
    assert [np.nonzero(b)[0].tolist() for b in bad] == changed[:4] + [q_cells, changed[8]]
    assert bad[0, 0] and want["first_bad_cell"] == 0      # cell 0 fails: below a wave the lanes past the end evaluate it too
    for j, s in zip(range(6), shifts[:4] + [max(shifts[4:8]), shifts[0]]):      # inside a shift group some cells fail and others pass
        groups = bad[j].reshape(-1, 1 << s).sum(axis=1)
        assert any(0 < g < 1 << s for g in groups), j


# ---- 4. field edges ------------------------------------------------------------------------------------------------------------------------------
class Asm:
    """Bytecode from calls; destination registers walk the two files round and round (an identity below keeps far fewer than 24 values)."""

    def __init__(self):
        self.code, self._m, self._q = [], 0, 0

    def m(self, op, a=0, b=0):
        r, self._m = self._m, (self._m + 1) % 96
        self.code += [op, r, a, b & M32]
        return r

    def q(self, op, a=0, b=0):
        r, self._q = self._q, (self._q + 1) % 24
        self.code += [op, r, a, b & M32]
        return r

    def base(self, r):
        self.code += [C_BASE, 0, r, 0]

    def ext(self, r):
        self.code += [C_EXT, 0, r, 0]


A, B, C, X, Y, Z = 0, 1, 2, 3, 7, 11          # columns: three base ones and the coordinates of three extension ones
N_IDENTITY_COLS = 15
IDENTITY_PARAMS = [[P - 1] * 4, [P - 1] * 4, [0, 0, 0, 1]]      # the third: what the extension twin is off by


def _base_identities():
    """E - E' for rearrangements E' of E in M31: (name, f(asm) -> m register)"""
    col, add, sub, mul, neg = (lambda s, c: s.m(M_COL, c)), (lambda s, a, b: s.m(M_ADD, a, b)), (lambda s, a, b: s.m(M_SUB, a, b)), (lambda s, a, b: s.m(M_MUL, a, b)), (lambda s, a: s.m(M_NEG, a))
    const = lambda s, v: s.m(M_CONST, v)

    def distribute(s):
        a, b, c = col(s, A), col(s, B), col(s, C)
        return sub(s, mul(s, add(s, a, b), c), add(s, mul(s, a, c), mul(s, b, c)))

    def antisymmetry(s):
        a, b = col(s, A), col(s, B)
        return sub(s, sub(s, a, b), neg(s, sub(s, b, a)))

    def plus_negation(s):
        a = col(s, A)
        return add(s, a, neg(s, a))

    def associate(s):
        a, b, c = col(s, A), col(s, B), col(s, C)
        return sub(s, mul(s, a, mul(s, b, c)), mul(s, mul(s, a, b), c))

    def double_negation(s):
        a = col(s, A)
        return sub(s, neg(s, neg(s, a)), a)

    def minus_itself(s):
        return sub(s, col(s, A), col(s, A))

    def times_minus_one(s):
        a = col(s, A)
        return add(s, mul(s, a, const(s, P - 1)), a)

    def neutral_elements(s):
        a = col(s, A)
        return sub(s, mul(s, add(s, a, const(s, 0)), const(s, 1)), a)

    def difference_of_squares(s):
        a, b = col(s, A), col(s, B)
        return sub(s, mul(s, sub(s, a, b), add(s, a, b)), sub(s, mul(s, a, a), mul(s, b, b)))

    def negation_of_zero(s):      # the one identity whose last operation is a negation: the zero it negates must stay the canonical one
        return neg(s, sub(s, col(s, B), col(s, B)))

    return [distribute, antisymmetry, plus_negation, associate, double_negation, minus_itself, times_minus_one, neutral_elements, difference_of_squares,
            negation_of_zero]


def _ext_identities():
    """the same in QM31, and across the two files: (name, f(asm) -> q register)"""
    col, qcol, par, lift = (lambda s, c: s.m(M_COL, c)), (lambda s, c: s.q(Q_COL, c)), (lambda s, i: s.q(Q_PARAM, i)), (lambda s, r: s.q(Q_FROM_M, r))
    add, sub, mul, mulm = (lambda s, a, b: s.q(Q_ADD, a, b)), (lambda s, a, b: s.q(Q_SUB, a, b)), (lambda s, a, b: s.q(Q_MUL, a, b)), (lambda s, a, b: s.q(Q_MULM, a, b))

    def distribute(s):
        x, y, z = qcol(s, X), qcol(s, Y), qcol(s, Z)
        return sub(s, mul(s, add(s, x, y), z), add(s, mul(s, x, z), mul(s, y, z)))

    def mulm_is_mul_of_the_lift(s):
        x, a = qcol(s, X), col(s, A)
        return sub(s, mulm(s, x, a), mul(s, x, lift(s, a)))

    def antisymmetry(s):
        x, y = qcol(s, X), qcol(s, Y)
        return add(s, sub(s, x, y), sub(s, y, x))

    def plus_negation(s):
        x = qcol(s, X)
        return add(s, x, mulm(s, x, s.m(M_CONST, P - 1)))

    def associate(s):
        x, y, z = qcol(s, X), qcol(s, Y), qcol(s, Z)
        return sub(s, mul(s, mul(s, x, y), z), mul(s, x, mul(s, y, z)))

    def commute_with_a_parameter(s):
        x, p = qcol(s, X), par(s, 0)
        return sub(s, mul(s, p, x), mul(s, x, p))

    def lift_of_a_sum(s):
        a, b = col(s, A), col(s, B)
        return sub(s, add(s, lift(s, a), lift(s, b)), lift(s, s.m(M_ADD, a, b)))

    def lift_of_a_product(s):
        a, b = col(s, A), col(s, B)
        return sub(s, lift(s, s.m(M_MUL, a, b)), mul(s, lift(s, a), lift(s, b)))

    def parameter_there_and_back(s):
        x, p = qcol(s, X), par(s, 1)
        return sub(s, add(s, sub(s, x, p), p), x)

    def difference_of_squares(s):
        x, y = qcol(s, X), qcol(s, Y)
        return sub(s, sub(s, mul(s, x, x), mul(s, y, y)), mul(s, sub(s, x, y), add(s, x, y)))

    return [distribute, mulm_is_mul_of_the_lift, antisymmetry, plus_negation, associate, commute_with_a_parameter, lift_of_a_sum, lift_of_a_product,
            parameter_there_and_back, difference_of_squares]


def identity_program(twin=None):
    """Base and extension identities interleaved: every constraint is identically zero. twin = j: constraint j is off by one — a base
    constraint by the constant 1, an extension constraint by parameter 2 = (0, 0, 0, 1). Returns (code, the constraints' kinds)."""
    base, ext = _base_identities(), _ext_identities()
    order = [f for pair in zip(base, ext) for f in pair] + ext[len(base):]
    s, kinds = Asm(), []
    for j, f in enumerate(order):
        r = f(s)
        if f in base:
            s.base(s.m(M_ADD, r, s.m(M_CONST, 1)) if twin == j else r)
        else:
            s.ext(s.q(Q_ADD, r, s.q(Q_PARAM, 2)) if twin == j else r)
        kinds.append(C_BASE if f in base else C_EXT)
    return s.code, kinds


def complement_program():
    """Zero only where column B is P - A and Y is P - X coordinate by coordinate (a zero cell stays zero): every sum is exactly P."""
    s = Asm()
    a, b = s.m(M_COL, A), s.m(M_COL, B)
    s.base(s.m(M_ADD, a, b))
    x, y = s.q(Q_COL, X), s.q(Q_COL, Y)
    s.ext(s.q(Q_ADD, x, y))
    s.ext(s.q(Q_ADD, s.q(Q_FROM_M, a), s.q(Q_FROM_M, b)))
    s.base(s.m(M_MUL, s.m(M_ADD, b, a), s.m(M_COL, C)))
    s.ext(s.q(Q_MULM, s.q(Q_ADD, y, x), a))
    return s.code


IDENTITY_FAMILIES = ("max", "edge", "zero", "uniform", "complement")
IDENTITY_LOG = 7


def _swap_neighbours(v):
    return v.reshape(-1, 2)[:, ::-1].reshape(-1)


def identity_columns(family, log_size=IDENTITY_LOG):
    """15 columns of a tests/field_inputs.py family. "complement": A, C, X and Z are complement1 columns (cells i and i ^ 1 sum to exactly
    P), B and Y are A and X with the two cells of each pair swapped, so A + B and X + Y are P in every cell that is not zero."""
    n = 1 << log_size
    if family == "zero":
        return np.zeros((N_IDENTITY_COLS, n), dtype=np.uint32)
    if family != "complement":
        return np.stack(fi.columns(family, 77, N_IDENTITY_COLS, n))
    cols = fi.columns("complement1", 78, N_IDENTITY_COLS, n)
    cols[B] = _swap_neighbours(cols[A])
    for k in range(4):
        cols[Y + k] = _swap_neighbours(cols[X + k])
    return np.stack(cols)


def identity_case(family, twin=None):
    def build():
        code, kinds = identity_program(twin)
        return Case(code, 3, IDENTITY_LOG, identity_columns(family), IDENTITY_PARAMS, kinds=kinds, twin=twin)
    return _cached(("identity", family, twin), build)


def complement_case():
    return _cached("complement", lambda: Case(complement_program(), 0, IDENTITY_LOG, identity_columns("complement"), []))


def twin_report(case):
    """The closed form of an off-by-one twin: every cell fails constraint `twin` alone, with value 1 in the first coordinate (base) or the
    fourth (extension)."""
    n, j, kinds = 1 << case.log_size, case.notes["twin"], case.notes["kinds"]
    k = len(kinds)
    return {"log_size": case.log_size, "n_constraints": k, "n_bad_cells": n, "first_bad_cell": 0, "first_bad_constraint": j,
            "first_bad_value": [1, 0, 0, 0] if kinds[j] == C_BASE else [0, 0, 0, 1], "bad_per_constraint": [n if i == j else 0 for i in range(k)],
            "first_cell_per_constraint": [0 if i == j else None for i in range(k)]}


ONE_COORDINATE_LOG = 7
ONE_COORDINATE_DELTA = [5, 1, P - 1, 123456]


def one_coordinate_case(lowest):
    """Columns 0..3: X, random; 4 + 4 k .. 7 + 4 k: X again with coordinate k lowered by ONE_COORDINATE_DELTA[k] at one cell. Constraint k
    = X minus copy k (C_EXT): non-zero at that cell only, in coordinate k only. Coordinate `lowest` gets the lowest cell. Returns the case;
    notes: cells, and the closed-form report."""
    def build():
        n = 1 << ONE_COORDINATE_LOG
        cells = [100, 37, 64, 63]
        cells[lowest] = 5
        x = np.stack(fi.columns("uniform", 55, 4, n))
        full, code = [x], []
        for k in range(4):
            y = x.copy()
            y[k, cells[k]] = (int(y[k, cells[k]]) - ONE_COORDINATE_DELTA[k]) % P
            full.append(y)
            code += [Q_COL, 6 * k, 0, 0, Q_COL, 6 * k + 1, 4 + 4 * k, 0, Q_SUB, 6 * k + 2, 6 * k, 6 * k + 1, C_EXT, 0, 6 * k + 2, 0]
        report = {"log_size": ONE_COORDINATE_LOG, "n_constraints": 4, "n_bad_cells": 4, "first_bad_cell": 5, "first_bad_constraint": lowest,
                  "first_bad_value": [ONE_COORDINATE_DELTA[lowest] if w == lowest else 0 for w in range(4)], "bad_per_constraint": [1] * 4,
                  "first_cell_per_constraint": cells}
        return Case(code, 0, ONE_COORDINATE_LOG, np.concatenate(full), [], report=report)
    return _cached(("one_coordinate", lowest), build)


FIRST_LOG, FIRST_CELL, LATER_CELL, FIRST_CONSTRAINT = 8, 77, 200, 41
FIRST_VALUE = [11, P - 1, 33, 44]


def first_constraint_case(kind):
    """44 constraints on 256 cells. Constraint 0 (column 0) fails at cell 200 only. Constraints 1..40 are products with an all-zero
    column, base and extension alternating. Constraint 41 reads columns 1..4 as one Q_COL (kind C_EXT) or column 1 alone (C_BASE): FIRST_VALUE
    at cell 77, something else at cell 150. Constraints 42 (base) and 43 (extension) read column 6, non-zero at cell 77 too. So the first
    bad cell is 77, where the lowest failing constraint is 41 and later ones fail as well."""
    def build():
        n = 1 << FIRST_LOG
        full = np.zeros((7, n), dtype=np.uint32)
        full[0, LATER_CELL] = 9
        full[1:5, FIRST_CELL] = FIRST_VALUE
        full[1, 150] = 5
        full[6, FIRST_CELL] = 3
        s = Asm()
        s.base(s.m(M_MUL, s.m(M_COL, 0), s.m(M_CONST, 7)))
        for j in range(1, FIRST_CONSTRAINT):
            z = s.m(M_COL, 5)
            if j % 2:
                s.ext(s.q(Q_MULM, s.q(Q_PARAM, 0), z))
            else:
                s.base(s.m(M_MUL, z, s.m(M_CONST, P - j)))
        if kind == C_EXT:
            s.ext(s.q(Q_COL, 1))
        else:
            s.base(s.m(M_COL, 1))
        c = s.m(M_COL, 6)
        s.base(c)
        s.ext(s.q(Q_MULM, s.q(Q_PARAM, 0), c))
        value = FIRST_VALUE if kind == C_EXT else [FIRST_VALUE[0], 0, 0, 0]
        k = FIRST_CONSTRAINT + 3
        count = lambda j: 1 if j in (0, 42, 43) else 2 if j == FIRST_CONSTRAINT else 0
        report = {"log_size": FIRST_LOG, "n_constraints": k, "n_bad_cells": 3, "first_bad_cell": FIRST_CELL, "first_bad_constraint": FIRST_CONSTRAINT,
                  "first_bad_value": value, "bad_per_constraint": [count(j) for j in range(k)],
                  "first_cell_per_constraint": [LATER_CELL if j == 0 else FIRST_CELL if count(j) else None for j in range(k)]}
        return Case(s.code, 1, FIRST_LOG, full, [[2, 0, 0, P - 3]], report=report)
    return _cached(("first", kind), build)
