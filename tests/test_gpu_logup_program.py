"""-m gpu: the fraction program on the trace domain (bfhip_logup_program_generate, csrc/logup_program.hip) — bit-exact parity with
bfhip_logup_generate and the oracle for the 13 Brainfuck components written as fraction programs, seeded random programs over distinct cells
against the numpy model of tests/logup_model.py at the sizes where the kernels change path, saturated values, the zero-denominator report, a
lookup AIR proved and verified end to end through the commitment-scheme session, and the call inside an open session. Integer field
arithmetic: every comparison is exact."""
import numpy as np
import pytest

import field_inputs
import logup_model
import pcs_replay
from conftest import splitmix_column, P

pytestmark = pytest.mark.gpu

ALL_OPS = ("+++>,<[>+.<-]", b"\x01")       # tests/test_gpu_air_program.py
HELLO = ("++++++++++[>+++++++>++++++++++>+++>+<<<<-]>++.>+.+++++++..+++.>++.<<+++++++++++++++.>.+++.------.--------.>+.>.", b"")
PROGS = {"all_ops": ALL_OPS, "hello": HELLO}
NAMES = ["memory", "instruction", "program", "processor", "jnz", "jz", "input", "left", "minus", "output", "plus", "right", "end_of_execution"]
ONE = [1, 0, 0, 0]


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


def _generate(ctx, program, log_size, cols, shifts, params):
    """(the 4 * n_logup full-size output columns, claimed sum) of one call on host columns"""
    n = 1 << log_size
    with Dev(ctx) as dev:
        src = [dev.up(c) for c in cols]
        dst = [dev.empty(n) for _ in range(4 * program.shape["n_logup_cols"])]
        claimed = ctx.logup_program_generate(program, log_size, src, params, dst, col_shifts=shifts)
        return np.stack([ctx.download(p, n) for p in dst]), claimed


# ---- 1. the 13 Brainfuck components -----------------------------------------------------------------------------------------------------------
_ORACLE_CASES = {}


def _oracle_case(oracle, name, comp):
    if (name, comp) not in _ORACLE_CASES:
        code, inp = PROGS[name]
        rows = np.ascontiguousarray(oracle.table(code, inp, comp).T)
        _ORACLE_CASES[(name, comp)] = (rows,) + oracle.logup_generate(comp, rows, _elems(77))
    return _ORACLE_CASES[(name, comp)]


@pytest.mark.parametrize("storage", ["shift_4", "full_size"])
@pytest.mark.parametrize("name", ["all_ops", "hello"])
def test_brainfuck_programs_match_logup_generate_and_the_oracle(_ctx, pkg, _oracle, name, storage):
    """bfhip_logup_program_generate of the 13 brainfuck_logup_programs on the row-granular main columns at shift 4 (and on the same columns
    expanded to full size at shift 0): every earlier column == the 16-fold broadcast of bfhip_logup_generate's row-granular output, the last
    column and the claimed sum == bfhip_logup_generate's, and all of it == the oracle's."""
    ctx, elems = _ctx, _elems(77)
    logs = set()
    for comp in range(13):
        rows, want, want_claimed = _oracle_case(_oracle, name, comp)
        n_main, M = rows.shape
        log_size, n_logup = int(np.log2(M)) + 4, 3 if comp == 3 else 1
        with Dev(ctx) as dev:
            sizes = [M] * (4 * (n_logup - 1)) + [16 * M] * 4
            dst = [dev.empty(s) for s in sizes]
            compiled_claimed = ctx.logup_generate(comp, log_size, [dev.up(r) for r in rows], elems, dst)
            compiled = np.stack([np.repeat(ctx.download(p, s), 16 * M // s) for p, s in zip(dst, sizes)])
        program, _ = pkg.brainfuck_logup_program(comp)
        params = pkg.brainfuck_air_params(elems, [0, 0, 0, 0])[:24]
        cols, shifts = (rows, [4] * n_main) if storage == "shift_4" else (np.repeat(rows, 16, axis=1), [0] * n_main)
        got, claimed = _generate(ctx, program, log_size, cols, shifts, params)
        assert claimed == compiled_claimed == want_claimed, NAMES[comp]
        assert np.array_equal(got, compiled) and np.array_equal(got, want), NAMES[comp]
        logs.add(log_size)
    assert min(logs) == 4 and max(logs) >= 9


# ---- 2. generic shapes against the model ----------------------------------------------------------------------------------------------------
# The constants a size crosses (csrc/logup_program.hip: 64 lanes per row-stage workgroup; the scan covers the N / 2 sums w[q] in tiles of
# LP_TILE = 1024, and the totals pass takes LP_CHUNK = 256 tile totals per chunk):
#   1   two cells: N / 2 = 1, a single w, the smallest domain there is
#   4   16 cells: below one wave; a workgroup with idle lanes
#   6   64 cells: one wave exactly
#   11  N / 2 = 1024: exactly one full scan tile
#   12  N / 2 = 2048: two tiles, so the totals pass and its carry into the second tile matter
#   20  N / 2 = 2^19 = 512 tiles: the smallest size at which the totals pass takes more than one chunk of 256 (one fraction only)
SHAPES = [("small", 2, 3, 1), ("small", 2, 3, 4), ("small", 2, 3, 6), ("small", 2, 3, 11), ("small", 2, 3, 12),
          ("caps", 8, 32, 1), ("caps", 8, 32, 4), ("caps", 8, 32, 6), ("caps", 8, 32, 11), ("caps", 8, 32, 12), ("one_fraction", 1, 1, 20)]


def _random_case(n_logup, n_fractions, log_size, column=splitmix_column, seed=0):
    code, n_cols, n_params = logup_model.random_program(1000 * n_fractions + log_size + seed, n_logup, n_fractions)
    if log_size >= 16:      # the model's time goes with cells x QM31 products: the large domain gets the shortest program, params[0] / (col 2 + params[1])
        assert (n_logup, n_fractions) == (1, 1)
        code = [logup_model.M_COL, 0, 2, 0, logup_model.Q_FROM_M, 1, 0, 0, logup_model.Q_PARAM, 0, 1, 0, logup_model.Q_ADD, 1, 1, 0, logup_model.Q_PARAM, 0, 0, 0,
                logup_model.FRAC, 0, 0, 1, logup_model.END_COL, 0, 0, 0]
    cols = np.stack([column(((k + 1) << 32) + log_size, 1 << log_size) for k in range(n_cols)])      # every cell distinct, no column a shift of another
    return code, cols, _quads(600 + log_size + seed, n_params)


@pytest.mark.parametrize("kind,n_logup,n_fractions,log_size", SHAPES, ids=["%s-log%d" % (s[0], s[3]) for s in SHAPES])
def test_random_programs_on_distinct_cells_match_the_model(_ctx, pkg, kind, n_logup, n_fractions, log_size):
    code, cols, params = _random_case(n_logup, n_fractions, log_size)
    program = pkg.LogupProgram(code, len(cols), len(params))
    assert (program.shape["n_logup_cols"], program.shape["n_fractions"]) == (n_logup, n_fractions)
    want, want_claimed, zeros = logup_model.generate(code, cols, [0] * len(cols), params, log_size)
    assert zeros == []
    got, claimed = _generate(_ctx, program, log_size, cols, None, params)
    assert claimed == want_claimed
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k]), ("coordinate column", k)
    # the claimed sum is the sum of the last column's per-cell values: the last column minus the one before, summed over the coset — here
    # read off the prefix sum itself: its value at the last coset position
    last = int(np.nonzero(logup_model.coset_position(log_size) == (1 << log_size) - 1)[0][0])
    assert [int(got[-4 + k][last]) for k in range(4)] == claimed


def test_mixed_shifts_match_the_model(_ctx, pkg):
    """Columns stored at shifts 0, 2, 3 and log_size in one call (log_size 7: two row-stage workgroups)."""
    log_size = 7
    code, cols, params = _random_case(2, 3, log_size, seed=5)
    shifts = [0, 2, 3, log_size, 0, 2]
    stored = [c[: 1 << (log_size - s)] for c, s in zip(cols, shifts)]
    want, want_claimed, zeros = logup_model.generate(code, stored, shifts, params, log_size)
    assert zeros == []
    got, claimed = _generate(_ctx, pkg.LogupProgram(code, len(cols), len(params)), log_size, stored, shifts, params)
    assert claimed == want_claimed and np.array_equal(got, want)


# ---- 3. saturated values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["max", "zero", "edge"])
def test_saturated_cells_match_the_model(_ctx, pkg, family):
    """All cells p - 1, all cells zero, and the edge set of tests/field_inputs.py (0, 1, p - 1, 2^30, 2^16 ... drawn per cell), under
    parameters for which the model finds no vanishing denominator; also with every parameter word p - 1."""
    log_size = 7
    column = {"max": lambda seed, n: np.full(n, P - 1, dtype=np.uint32), "zero": lambda seed, n: np.zeros(n, dtype=np.uint32), "edge": field_inputs.edge}[family]
    for seed, params_of in ((1, None), (2, lambda n: [[P - 1] * 4] * n)):
        code, cols, params = _random_case(2, 3, log_size, column=column, seed=seed)
        if params_of:
            params = params_of(len(params))
        want, want_claimed, zeros = logup_model.generate(code, cols, [0] * len(cols), params, log_size)
        assert zeros == [], "the test's parameters must keep every denominator non-zero"
        got, claimed = _generate(_ctx, pkg.LogupProgram(code, len(cols), len(params)), log_size, cols, None, params)
        assert claimed == want_claimed and np.array_equal(got, want), (family, seed)


# ---- 4. a zero denominator ---------------------------------------------------------------------------------------------------------------------
def _lookup_fractions(pkg, extra=False):
    """Columns a (0), t (1), mult (2); parameters z (0), alpha (1). Column 0: 1 / (alpha a - z); column 1: -mult / (alpha t - z). extra: a
    fraction 1 / (alpha t - z) in front of column 0's and a second copy of column 0's behind it (fractions 0, 1, 2; then 3)."""
    b = pkg.AirBuilder()
    a, t, mult, z, alpha = b.col(0), b.col(1), b.col(2), b.param(0), b.param(1)
    if extra:
        b.frac(1, alpha * t - z)
    b.frac(1, alpha * a - z)
    if extra:
        b.frac(b.param(1), alpha * a - z)
    b.end_column()
    b.frac(-mult, alpha * t - z)
    b.end_column()
    return b.logup_program()


def test_zero_denominator_names_the_lowest_cell_and_fraction(_ctx, pkg):
    """z = alpha * a[37] on a log_size 6 trace whose `a` also holds that value at cell 50: fractions 1 and 2 (the two over alpha a - z) vanish
    at cells 37 and 50; the call returns -1 naming fraction 1 at cell 37. The next valid call on the context is bit-exact."""
    log_size, n = 6, 64
    program = _lookup_fractions(pkg, extra=True)
    a, t, mult = splitmix_column(11 << 32, n), splitmix_column(12 << 32, n), splitmix_column(13 << 32, n)
    a[50] = a[37]
    alpha = _quads(21, 1)[0]
    z = pcs_replay.q_mul(alpha, [int(a[37]), 0, 0, 0])
    assert int(a[37]) not in [int(v) for v in t]
    _, _, zeros = logup_model.generate(program.code, [a, t, mult], [0, 0, 0], [z, alpha], log_size)
    assert zeros == [(37, 1), (37, 2), (50, 1), (50, 2)]
    with pytest.raises(pkg.BfhipError) as e:
        _generate(_ctx, program, log_size, [a, t, mult], None, [z, alpha])
    assert str(e.value) == "bfhip_logup_program_generate: fraction 1 has a zero denominator at cell 37"
    assert pkg.lib().bfhip_last_error().decode() == str(e.value)
    z = _quads(22, 1)[0]
    want, want_claimed, zeros = logup_model.generate(program.code, [a, t, mult], [0, 0, 0], [z, alpha], log_size)
    got, claimed = _generate(_ctx, program, log_size, [a, t, mult], None, [z, alpha])
    assert zeros == [] and claimed == want_claimed and np.array_equal(got, want)


def test_refusals_leave_the_context_usable(_ctx, pkg):
    ctx, log_size = _ctx, 5
    program = _lookup_fractions(pkg)
    cols = [splitmix_column((31 + k) << 32, 32) for k in range(3)]
    params = _quads(33, 2)
    with Dev(ctx) as dev:
        src, dst = [dev.up(c) for c in cols], [dev.empty(32) for _ in range(8)]
        for kwargs, what in ((dict(log_size=0), "log_size must be in"), (dict(log_size=ctx.max_log_domain + 1), "log_size must be in"),
                             (dict(col_shifts=[0, 1, 0]), "shift 1"), (dict(col_shifts=[0, 6, 0]), "shift 6"),
                             (dict(params=params[:1]), "takes 2 parameters, got 1"), (dict(params=[params[0], [P, 0, 0, 0]]), "canonical"),
                             (dict(dst=dst[:7] + [0]), "null output column pointer")):
            args = dict(log_size=log_size, params=params, col_shifts=None, dst=dst)
            args.update(kwargs)
            with pytest.raises(pkg.BfhipError, match=what):
                ctx.logup_program_generate(program, args["log_size"], src, args["params"], args["dst"], col_shifts=args["col_shifts"])
            assert pkg.lib().bfhip_last_error().decode().startswith("bfhip_logup_program_generate: ")
    want, want_claimed, _ = logup_model.generate(program.code, cols, [0, 0, 0], params, log_size)
    got, claimed = _generate(ctx, program, log_size, cols, None, params)
    assert claimed == want_claimed and np.array_equal(got, want)


# ---- 5. a lookup AIR end to end through the session ---------------------------------------------------------------------------------------
A, T, MULT, IS_FIRST, LOGUP0, LOGUP1 = 0, 1, 2, 3, 4, 8


def _lookup_constraints(pkg):
    """The two degree-2 logUp constraints of the fraction program above, built the way logup_mid / logup_last of brainfuck_air_program build
    them. Columns a, t, mult, IsFirst, then the 8 interaction coordinate columns; parameters z, alpha, the claimed sum."""
    b = pkg.AirBuilder()
    a, t, mult, is_first = b.col(A), b.col(T), b.col(MULT), b.col(IS_FIRST)
    z, alpha, total = b.param(0), b.param(1), b.param(2)
    cur0 = b.secure_col(LOGUP0)
    b.constraint(cur0 * (alpha * a - z) - b._to_q(b.const(1)))
    cur1, prev_row = b.secure_col(LOGUP1), b.secure_col(LOGUP1, -1)
    diff = cur1 - (prev_row - total * is_first) - cur0
    b.constraint(diff * (alpha * t - z) - b._to_q(-mult))
    return b.program()


def _lookup_trace(log_size, seed):
    """a, t, mult, IsFirst in storage order: t distinct, a drawn from t, mult[i] = how often t[i] occurs in a."""
    n = 1 << log_size
    t = splitmix_column(seed, n)
    assert len(set(t.tolist())) == n
    pick = splitmix_column((seed + 1) << 32, n) % np.uint32(n // 4)      # a quarter of the table is looked up, several times each
    a = t[pick]
    mult = np.bincount(pick, minlength=n).astype(np.uint32)
    is_first = np.zeros(n, dtype=np.uint32); is_first[0] = 1
    return np.stack([a, t, mult, is_first])


def _prove_lookup(ctx, pkg, trace, log_size, corrupt_interaction=False):
    """(claimed sum, verifier's verdict, sampled composition value, the constraint program at the sampled mask values)"""
    fractions, program = _lookup_fractions(pkg), _lookup_constraints(pkg)
    n, mask = 1 << log_size, program.mask()
    with Dev(ctx) as dev:
        ch = pkg.Channel((0, 0, 0, 0))
        with pkg.PcsSession(ctx) as s:
            cols = [dev.up(c) for c in trace]
            root0 = s.commit(ch, cols, [log_size] * 4, form=0)
            z, alpha = ch.draw_felts(2)
            inter = [dev.empty(n) for _ in range(8)]
            claimed = ctx.logup_program_generate(fractions, log_size, cols[:3], [z, alpha], inter)      # while the session is open
            if corrupt_interaction:
                bad = ctx.download(inter[5], n)
                bad[9] = (int(bad[9]) + 1) % P
                inter[5] = dev.up(bad)
            ch.mix_felts([claimed])
            root1 = s.commit(ch, inter, [log_size] * 8, form=0)
            random_coeff = ch.draw_felt()
            coeffs = [random_coeff, ONE]                              # stwo's accumulator order: constraint j gets r^(N - 1 - j)
            params = [z, alpha, claimed]
            lde = s.tree_columns(0)[1] + s.tree_columns(1)[1]         # the session's own LDE columns: blowup 2 = the constraint domain
            acc = [dev.up(np.zeros(2 * n, dtype=np.uint32)) for _ in range(4)]
            ctx.air_eval_domain(program, log_size, 1, lde, params, coeffs, acc)
            comp = [dev.empty(2 * n) for _ in range(4)]
            ctx.interpolate(acc, comp, log_size + 1)
            root2 = s.commit(ch, comp, [log_size + 1] * 4, form=1)
            oods = ch.draw_point()
            points = [oods, pkg.circle_point_offset(oods, log_size, -1)]
            per_col = [[{0: 0, -1: 1}[off] for c, off in mask if c == col] for col in range(12)]
            samples = [per_col[:4], per_col[4:], [[0]] * 4]
            proof, sampled = s.prove_values(ch, points, samples, with_sampled=True)
    vch, v = pkg.Channel((0, 0, 0, 0)), pkg.PcsVerifier((0, 0, 0, 0))
    v.commit(vch, root0, [log_size] * 4)
    assert vch.draw_felts(2) == [z, alpha]
    vch.mix_felts([claimed])
    v.commit(vch, root1, [log_size] * 8)
    assert vch.draw_felt() == random_coeff
    v.commit(vch, root2, [log_size + 1] * 4)
    assert vch.draw_point() == oods
    verdict = v.verify_values(vch, points, samples, proof)
    assert len(sampled) == len(mask) + 4
    return claimed, verdict, pcs_replay.from_partial_evals(sampled[-4:]), program.eval_at_point(log_size, oods, sampled[: len(mask)], params, coeffs)


def test_lookup_air_proved_and_verified_through_the_session(_ctx, pkg):
    """Commit the trace, draw z and alpha, generate the interaction trace from the fraction program, mix the claimed sum, commit the 8
    interaction columns, sweep the two logUp constraints over the session's LDE, commit the composition, open with the constraint
    program's mask; a verifier session replays it. The claimed sum is zero (every looked-up value is in the table as often as mult says),
    the proof verifies and the sampled composition value is the program at the sampled mask values. One mult cell changed: the claimed sum
    is not zero. One interaction cell changed after generation: the openings still verify, and the out-of-domain equality fails."""
    log_size = 6
    _ctx.set_pcs_config(pkg.PcsConfig())      # blowup 2: the session's LDE domain is the constraint domain of a degree-2 AIR
    program = _lookup_constraints(pkg)
    assert program.shape["n_constraints"] == 2 and sorted(set(program.mask())) == sorted([(c, 0) for c in range(12)] + [(c, -1) for c in range(8, 12)])
    trace = _lookup_trace(log_size, 51)
    claimed, verdict, sampled_value, at_point = _prove_lookup(_ctx, pkg, trace, log_size)
    assert claimed == [0, 0, 0, 0] and verdict == (True, "") and sampled_value == at_point and any(sampled_value)
    bad = trace.copy()
    bad[MULT, 3] = (int(bad[MULT, 3]) + 1) % P
    _, bad_claimed = _generate(_ctx, _lookup_fractions(pkg), log_size, bad[:3], None, _quads(61, 2))
    assert bad_claimed != [0, 0, 0, 0]
    assert _generate(_ctx, _lookup_fractions(pkg), log_size, trace[:3], None, _quads(61, 2))[1] == [0, 0, 0, 0]
    claimed, verdict, sampled_value, at_point = _prove_lookup(_ctx, pkg, trace, log_size, corrupt_interaction=True)
    assert claimed == [0, 0, 0, 0] and verdict == (True, "") and sampled_value != at_point


# ---- 6. while a session is open ---------------------------------------------------------------------------------------------------------------
def test_generate_works_while_a_session_is_open(_ctx, pkg):
    """The call on a context whose PcsSession is open and holds a committed tree: same bytes as the model, the session's arena untouched
    (its LDE columns read the same before and after)."""
    ctx, log_size = _ctx, 8
    code, cols, params = _random_case(2, 3, log_size, seed=9)
    want, want_claimed, _ = logup_model.generate(code, cols, [0] * len(cols), params, log_size)
    with Dev(ctx) as dev:
        ch = pkg.Channel((0, 0, 0, 0))
        with pkg.PcsSession(ctx) as s:
            s.commit(ch, [dev.up(c) for c in cols], [log_size] * len(cols), form=0)
            lde = s.tree_columns(0)[1]
            before = [ctx.download(p, 2 << log_size) for p in lde]
            got, claimed = _generate(ctx, pkg.LogupProgram(code, len(cols), len(params)), log_size, cols, None, params)
            after = [ctx.download(p, 2 << log_size) for p in lde]
    assert claimed == want_claimed and np.array_equal(got, want)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
