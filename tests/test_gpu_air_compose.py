"""-m gpu: the composition polynomial of any AIR in one call (bfhip_air_compose, csrc/air_compose.hip).
 1. The 13 Brainfuck programs over the captured polynomials of a real proof give the proof's own composition tree word for word, and the
    proof byte for byte when committed in its place — interpreted, compiled, and mixed; both logUp mask orders and log_blowup_factor 2.
 2. Seeded random and hand-written programs against the sequence of single operations a caller had before (bfhip_air_eval_domain per
    component under bfhip_air_compose_coeffs' slices into zeroed accumulators, bfhip_interpolate per size, bfhip_accumulate per smaller
    size), at the smallest shapes where a bucketed one-launch sweep can go wrong. bfhip_interpolate starts at 8 cells: a 4-cell bucket is
    interpolated here by solving the 4 x 4 system over the domain's points.
 3. The numpy model of tests/air_model.py with its own denominators, the oracle's interpolate and zero extension: independent of the
    library's sweep and finalize.
 4. At a channel-drawn point the host evaluator on the columns' sampled values equals the result evaluated at the point.
 5. Refusals leave the destination untouched and the context usable; nothing is taken from an open session's arena; a shard-group member
    is refused.
Integer field arithmetic: every comparison is exact."""
import ctypes
import sys

import numpy as np
import pytest

import air_model
import pcs_replay
from air_model import C_BASE, C_EXT, M_ADD, M_COL, M_MUL, M_NEG, M_SUB, Q_ADD, Q_COL, Q_FROM_M, Q_MUL, Q_MULM, Q_PARAM, Q_SUB
from conftest import P, splitmix_column
from test_gpu_air_program import _synthetic_program, _synthetic_trace
from test_gpu_pcs_session import LMR, STWO, Dev, _capture, _hctx, hctx      # noqa: F401 (the two fixtures)

pytestmark = pytest.mark.gpu

R = [0x1234567, P - 1, 0, 0x7654321]
NEG = lambda v: (-v) & 0xFFFFFFFF

# ---- programs ---------------------------------------------------------------------------------------------------------------------------------
# 2 columns, 3 constraints of both kinds
SMALL = ([M_COL, 0, 0, 0, M_COL, 1, 1, NEG(1), M_MUL, 2, 0, 1, C_BASE, 0, 2, 0, M_SUB, 3, 0, 1, Q_FROM_M, 0, 3, 0, Q_PARAM, 1, 0, 0, Q_MUL, 0, 0, 1, C_EXT, 0, 0, 0,
          M_ADD, 0, 0, 0, C_BASE, 0, 0, 0], 2, 1)
BASE_ONLY = ([M_COL, 0, 0, 1, M_COL, 1, 1, 0, M_SUB, 2, 0, 1, C_BASE, 0, 2, 0, M_MUL, 2, 2, 2, C_BASE, 0, 2, 0, M_NEG, 0, 1, 0, C_BASE, 0, 0, 0, C_BASE, 0, 1, 0, C_BASE, 0, 2, 0], 2, 0)
EXT_ONLY = ([Q_COL, 0, 0, 0, Q_PARAM, 1, 1, 0, Q_SUB, 2, 0, 1, C_EXT, 0, 2, 0, Q_COL, 3, 1, NEG(1), Q_ADD, 3, 3, 2, C_EXT, 0, 3, 0, M_COL, 0, 4, 0, Q_MULM, 3, 3, 0, C_EXT, 0, 3, 0], 5, 2)
TINY3 = ([M_COL, 0, 0, 0, M_NEG, 1, 0, 0, C_BASE, 0, 1, 0], 1, 0)      # 3 instructions, 2 m registers: 512 bytes of LDS
OFFSETS = ([M_COL, 0, 0, 2, M_COL, 1, 0, NEG(2), M_COL, 2, 0, 16, M_COL, 3, 0, NEG(16), M_MUL, 4, 0, 1, C_BASE, 0, 4, 0, M_SUB, 4, 2, 3, C_BASE, 0, 4, 0,
            Q_COL, 0, 0, NEG(16), Q_COL, 1, 0, 16, Q_MUL, 0, 0, 1, C_EXT, 0, 0, 0, M_COL, 5, 4, 0, C_BASE, 0, 5, 0], 5, 0)
_PROGRAMS = {}


def _program(pkg, name):
    """(AirProgram, code, n_cols, n_params), one per name for the module: "caps" and "r<seed>" come from air_model.random_program"""
    if name not in _PROGRAMS:
        if name == "caps":      # 96 m and 24 q registers = 48 KiB of LDS, 256 columns, 64 parameters, 64 constraints, offsets -16 .. 16
            code, n_cols, n_params, _ = air_model.random_program(7, n_cols=256, n_params=64, n_ops=3900, m_pool=96, q_pool=24, max_off=16, max_cons=64)
        elif name.startswith("r"):
            code, n_cols, n_params, _ = air_model.random_program(int(name[1:]), max_off=2)
        else:
            code, n_cols, n_params = {"small": SMALL, "base": BASE_ONLY, "ext": EXT_ONLY, "tiny3": TINY3, "offsets": OFFSETS}[name]
        _PROGRAMS[name] = (pkg.AirProgram(code, n_cols, n_params), code, n_cols, n_params)
    return _PROGRAMS[name]


def test_the_programs_are_what_the_cases_say(pkg):
    s = _program(pkg, "caps")[0].shape
    assert s["m_regs"] == 96 and s["q_regs"] == 24 and s["n_constraints"] == 64 and s["n_cols"] == 256 and s["n_params"] == 64
    s = _program(pkg, "small")[0].shape
    assert s["n_cols"] == 2 and s["n_constraints"] == 3
    assert _program(pkg, "tiny3")[0].shape["n_instr"] == 3
    kinds = lambda name: {_program(pkg, name)[1][i] for i in range(0, len(_program(pkg, name)[1]), 4)} & {C_BASE, C_EXT}
    assert kinds("base") == {C_BASE} and kinds("ext") == {C_EXT} and kinds("small") == {C_BASE, C_EXT}
    s = _program(pkg, "offsets")[0].shape
    assert (s["min_offset"], s["max_offset"]) == (-16, 16) and {off for _, off in _program(pkg, "offsets")[0].mask()} == {0, 2, -2, 16, -16}


# ---- one component: its columns on the device and on the host -----------------------------------------------------------------------------------
class Comp:
    def __init__(self, pkg, dev, name, log_size, log_expand, seed, cells="random", shifts=None):
        self.program, self.code, n_cols, n_params = _program(pkg, name)
        self.log_size, self.log_expand, self.el = log_size, log_expand, log_size + log_expand
        n = 1 << self.el
        self.shifts = shifts
        fill = {"random": lambda k: splitmix_column((seed << 16) + k, n), "max": lambda k: np.full(n, P - 1, dtype=np.uint32), "zero": lambda k: np.zeros(n, dtype=np.uint32)}[cells]
        self.cols = np.stack([fill(k) for k in range(n_cols)]).astype(np.uint32)
        if shifts is not None:      # a column of shift s holds one cell per 2^s rows: the full-size view repeats it
            for k, s in enumerate(shifts):
                self.cols[k] = np.repeat(self.cols[k][:: 1 << s], 1 << s)
        self.ptrs = [dev.up(c if shifts is None else c[:: 1 << shifts[k]]) for k, c in enumerate(self.cols)]
        self.params = [] if not n_params else (np.full((n_params, 4), P - 1, dtype=np.uint32) if cells == "max" else splitmix_column(seed + 99, 4 * n_params).reshape(n_params, 4)).tolist()

    def entry(self, program=None):
        e = (program or self.program, self.log_size, self.log_expand, self.ptrs, self.params)
        return e if self.shifts is None else e + (self.shifts,)


def _interpolate4(acc):
    """The coefficients (c0, c1, c2, c3) of c0 + c1 y + c2 x + c3 x y from its values on CanonicCoset(2).circle_domain() in bit-reversed
    order: the 4 x 4 system over the domain's points (air_model.domain_group_indices), solved by elimination over Python integers."""
    def point(index):
        mul = lambda p, q: ((p[0] * q[0] - p[1] * q[1]) % P, (p[0] * q[1] + p[1] * q[0]) % P)
        res, cur = (1, 0), air_model.CIRCLE_GEN
        while index:
            if index & 1:
                res = mul(res, cur)
            cur, index = mul(cur, cur), index >> 1
        return res
    pts = [point(g) for g in air_model.domain_group_indices(1, 1).tolist()]
    out = []
    for col in acc:
        rows = [[1, y, x, x * y % P, int(v)] for (x, y), v in zip(pts, col)]
        for i in range(4):
            piv = next(r for r in range(i, 4) if rows[r][i] % P)
            rows[i], rows[piv] = rows[piv], rows[i]
            inv = pow(rows[i][i], P - 2, P)
            rows[i] = [v * inv % P for v in rows[i]]
            for r in range(4):
                if r != i:
                    rows[r] = [(a - rows[r][i] * b) % P for a, b in zip(rows[r], rows[i])]
        out.append([rows[i][4] for i in range(4)])
    return np.array(out, dtype=np.uint32)


def _sequence(pkg, ctx, comps, r):
    """What a caller did before this entry: the coefficients sliced per component, bfhip_air_eval_domain per component into zeroed
    accumulators (one per log_size + log_expand), bfhip_interpolate per size, bfhip_accumulate per smaller size. Returns (4, 2^max el)."""
    coeffs = pkg.air_compose_coeffs([c.program.shape["n_constraints"] for c in comps], r)
    with Dev(ctx) as dev:
        accs, g = {}, 0
        for c in comps:
            if c.el not in accs:
                accs[c.el] = [dev.up(np.zeros(1 << c.el, dtype=np.uint32)) for _ in range(4)]
            n = c.program.shape["n_constraints"]
            ctx.air_eval_domain(c.program, c.log_size, c.log_expand, c.ptrs, c.params, coeffs[g: g + n], accs[c.el], col_shifts=c.shifts)
            g += n
        top = max(accs)
        for el, acc in accs.items():
            if el >= 3:
                ctx.interpolate(acc, acc, el)
            else:
                co = _interpolate4(np.stack([ctx.download(p, 4) for p in acc]))
                accs[el] = acc = [dev.up(co[w]) for w in range(4)]
            if el == top:
                top_acc = acc
        for el, acc in accs.items():
            if el != top:
                for w in range(4):
                    ctx.accumulate(top_acc[w], accs[el][w], 1 << el)
        return np.stack([ctx.download(p, 1 << top) for p in top_acc])


def _compose(ctx, dev, entries, r, dst_log, poison=0x5A5A5A5A):
    """air_compose into a destination that holds no field element before the call: it is overwritten, not accumulated"""
    dst = [dev.up(np.full(1 << dst_log, poison, dtype=np.uint32)) for _ in range(4)]
    ctx.air_compose(entries, r, dst, dst_log)
    return np.stack([ctx.download(p, 1 << dst_log) for p in dst])


# (name, log_size, log_expand) lists; the ids say what each is there for
SHAPES = {
    "el2_guarded_wave": [("small", 1, 1)],
    "el6_one_wave": [("small", 5, 1)],
    "el7_two_workgroups": [("small", 4, 3)],
    "el6_random_program": [("r11", 4, 2)],
    "bucket_of_three_middle_ext_only": [("small", 5, 1), ("ext", 5, 1), ("base", 5, 1)],
    "one_bucket_three_log_sizes": [("r12", 6, 1), ("r13", 5, 2), ("small", 4, 3)],
    "list_order_is_not_size_order": [("small", 7, 1), ("base", 4, 1), ("r11", 10, 2), ("ext", 5, 2)],       # el 8, 5, 12, 7
    "caps_beside_three_instructions": [("caps", 4, 2), ("tiny3", 3, 1)],
    "three_instructions_beside_caps": [("tiny3", 6, 2), ("caps", 3, 3)],
    "fourteen_sizes": [("small" if k % 2 else "base", k, 1) for k in range(1, 15)],                         # el 2 .. 15: a second accumulate_sizes launch
    "sixty_four_components": [(("small", "base", "ext", "tiny3")[k % 4], 4 - k % 3, 1 + k % 3) for k in range(64)],      # all el = 5
    # buckets of 2^16 rows and more are launched alone, the smaller ones together: el 17, 16 (two components), 7, 5
    "large_buckets_beside_small_ones": [("small", 4, 1), ("r11", 15, 2), ("small", 15, 1), ("tiny3", 6, 1), ("base", 15, 1)],
    "offsets_expand_1": [("offsets", 5, 1)], "offsets_expand_2": [("offsets", 5, 2), ("offsets", 4, 2)], "offsets_expand_3": [("offsets", 3, 3), ("offsets", 5, 3)],
}


@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_compose_is_the_sequence_of_single_operations(_ctx, pkg, shape):
    ctx = _ctx
    with Dev(ctx) as dev:
        comps = [Comp(pkg, dev, name, ls, le, 1000 + 7 * k) for k, (name, ls, le) in enumerate(SHAPES[shape])]
        dst_log = max(c.el for c in comps)
        got = _compose(ctx, dev, [c.entry() for c in comps], R, dst_log)
        want = _sequence(pkg, ctx, comps, R)
    if shape == "fourteen_sizes":
        assert len({c.el for c in comps}) == 14
    if shape == "sixty_four_components":
        assert {c.el for c in comps} == {5} and len({(c.log_size, c.log_expand) for c in comps}) == 3
    assert got.max() < P and got.any()
    assert np.array_equal(got, want), shape


@pytest.mark.parametrize("cells", ["max", "zero"])
def test_saturated_and_zero_cells(_ctx, pkg, cells):
    """all cells and parameters p - 1 (and r = (p - 1) x 4), all cells zero"""
    ctx, r = _ctx, [P - 1] * 4 if cells == "max" else R
    with Dev(ctx) as dev:
        comps = [Comp(pkg, dev, name, ls, le, 50 + k, cells=cells) for k, (name, ls, le) in enumerate([("r11", 4, 2), ("small", 4, 2), ("ext", 3, 1), ("base", 6, 1)])]
        got = _compose(ctx, dev, [c.entry() for c in comps], r, 7)
        want = _sequence(pkg, ctx, comps, r)
    assert np.array_equal(got, want) and got.max() < P


def test_a_column_at_shift_4_read_at_offset_0(_ctx, pkg):
    ctx = _ctx
    with Dev(ctx) as dev:
        # "offsets" reads column 4 at offset 0 only; "small" reads column 0 at offset 0 only
        comps = [Comp(pkg, dev, "offsets", 5, 2, 5, shifts=[0, 0, 0, 0, 4]), Comp(pkg, dev, "small", 6, 1, 6, shifts=[4, 0]), Comp(pkg, dev, "tiny3", 4, 1, 7, shifts=[5])]
        got = _compose(ctx, dev, [c.entry() for c in comps], R, 7)
        want = _sequence(pkg, ctx, comps, R)
    assert np.array_equal(got, want) and got.any()


def test_single_component_is_eval_domain_from_zero_interpolated(_ctx, pkg, _oracle):
    """for a single component the bucket holds bfhip_air_eval_domain's value from a zero accumulator: its oracle interpolation is the result"""
    ctx = _ctx
    with Dev(ctx) as dev:
        c = Comp(pkg, dev, "r12", 5, 2, 3)
        got = _compose(ctx, dev, [c.entry()], R, 7)
        acc = [dev.up(np.zeros(128, dtype=np.uint32)) for _ in range(4)]
        ctx.air_eval_domain(c.program, 5, 2, c.ptrs, c.params, pkg.air_compose_coeffs([c.program.shape["n_constraints"]], R), acc)
        want = _oracle.interpolate(np.stack([ctx.download(p, 128) for p in acc]), 7)
    assert np.array_equal(got, want)


def test_against_the_numpy_model_and_the_oracles_interpolate(_ctx, pkg, _oracle):
    """(6, 1), (5, 2) and (4, 3) in one bucket plus a smaller and a larger bucket: each bucket's accumulator from air_model.run times
    air_model.domain_denominators, interpolated by the oracle, added by zero extension — no kernel and no finalize of the library."""
    ctx, spec = _ctx, [("r12", 6, 1), ("small", 3, 2), ("r13", 5, 2), ("small", 4, 3), ("base", 7, 1)]
    with Dev(ctx) as dev:
        comps = [Comp(pkg, dev, name, ls, le, 300 + k) for k, (name, ls, le) in enumerate(spec)]
        got = _compose(ctx, dev, [c.entry() for c in comps], R, 8)
    coeffs = pkg.air_compose_coeffs([c.program.shape["n_constraints"] for c in comps], R)
    buckets, g = {}, 0
    for c in comps:
        n, rows = c.program.shape["n_constraints"], 1 << c.el
        value = air_model.run(c.code, air_model.domain_reader(c.cols, c.log_size, c.log_expand), c.params, coeffs[g: g + n], rows)
        value = air_model.q_mul(value, air_model.from_m(air_model.domain_denominators(c.log_size, c.log_expand)))
        buckets[c.el] = air_model.q_add(buckets[c.el], value) if c.el in buckets else value
        g += n
    assert sorted(buckets) == [5, 7, 8]
    want = np.zeros((4, 256), dtype=np.uint64)
    for el, acc in buckets.items():
        want[:, : 1 << el] = (want[:, : 1 << el] + _oracle.interpolate(acc.astype(np.uint32), el)) % np.uint64(P)
    assert np.array_equal(got, want.astype(np.uint32))


def test_point_and_domain_agree(_ctx, pkg, _oracle):
    """Three satisfied AIRs of three sizes (degrees 2, 3, 5 at blowups 2, 4, 8): at a channel-drawn point, air_compose_at_point on the
    columns' polynomials at the mask points equals the result's four coordinate polynomials at the point, combined."""
    ctx, spec = _ctx, [(4, 2, 1), (6, 5, 3), (5, 3, 2)]      # (log_size, degree, log_expand): el 5, 9, 7
    ch = pkg.Channel((0, 0, 0, 0))
    ch.mix_u64(77)
    point = ch.draw_point()
    with Dev(ctx) as dev:
        entries, at_point = [], []
        for k, (log_size, d, log_expand) in enumerate(spec):
            program = _synthetic_program(pkg, d)
            polys = _oracle.interpolate(_synthetic_trace(log_size, d, 60 + k), log_size)
            lde = _oracle.evaluate(polys, log_size, log_size + log_expand)
            entries.append((program, log_size, log_expand, [dev.up(c) for c in lde], []))
            co = [dev.up(c) for c in polys]
            mask_values = [ctx.eval_at_point(co[col], log_size, pkg.circle_point_offset(point, log_size, off)) for col, off in program.mask()]
            at_point.append((program, log_size, mask_values, []))
        got = _compose(ctx, dev, entries, R, 9)
        # a polynomial: the quotient of the largest size (odd degree) has no coefficient in the upper half (tests/test_gpu_air_program.py)
        assert got.any() and not got[:, 256:].any()
        value = pcs_replay.from_partial_evals([ctx.eval_at_point(dev.up(c), 9, point) for c in got])
    assert pkg.air_compose_at_point(at_point, point, R) == value


# ---- the Brainfuck composition polynomial ---------------------------------------------------------------------------------------------------------
_COMPILED = {}


def _brainfuck_program(hp, ctx, k, order, compiled):
    program = hp.brainfuck_air_program(k, order)[0]
    if not compiled:
        return program
    if (k, order) not in _COMPILED:
        _COMPILED[(k, order)] = ctx.air_compile(program)
    return _COMPILED[(k, order)]


def _brainfuck_compose_in_session(hp, ctx, dev, full, logs, trees, conv, which):
    """tests/test_gpu_pcs_session.py::_prove_replay with tree 3 computed by air_compose inside the open session, from trees 0 .. 2
    evaluated on each component's CanonicCoset(log + 1). which(k) -> whether component k runs as its compiled kernel.
    Returns (the composition columns, the session's proof, arena bytes in use before and after the call)."""
    log_sizes = [full["claim"][n]["log_size"] for n in pcs_replay.NAMES]
    claimed = [pcs_replay.flat_q(full["interaction_claim"][n]["claimed_sum"]) for n in pcs_replay.NAMES]
    ch = hp.Channel(conv)
    with hp.PcsSession(ctx) as s:
        ptrs = [[dev.up(col) for col in tree] for tree in trees[:3]]
        roots = [s.commit(ch, ptrs[0], logs[0], form=1)]
        for l in log_sizes:
            ch.mix_u64(l)
        roots.append(s.commit(ch, ptrs[1], logs[1], form=1))
        lookup = [w for _ in range(3) for q in ch.draw_felts(2) for w in q]
        for c in claimed:
            ch.mix_felts([c])
        roots.append(s.commit(ch, ptrs[2], logs[2], form=1))
        random_coeff = ch.draw_felts(1)[0]
        entries, m0, i0 = [], 0, 0
        for k, (n_main, n_logup) in enumerate(pcs_replay.component_shapes(hp)):
            log = log_sizes[k]
            where = [(1, m0 + j) for j in range(n_main)] + [(2, i0 + j) for j in range(4 * n_logup)] + [(0, LMR - log)]
            assert all(logs[t][c] == log for t, c in where), k
            src = [dev.up(trees[t][c]) for t, c in where]      # copies: the session owns what it was given
            cols = [dev.empty(2 << log) for _ in where]
            ctx.evaluate(src, cols, log, log + 1)
            entries.append((_brainfuck_program(hp, ctx, k, conv[2], which(k)), log, 1, cols, hp.brainfuck_air_params(lookup, claimed[k])))
            m0, i0 = m0 + n_main, i0 + 4 * n_logup
        dst_log = max(log_sizes) + 1
        assert logs[3] == [dst_log] * 4
        dst = [dev.up(np.full(1 << dst_log, 0x5A5A5A5A, dtype=np.uint32)) for _ in range(4)]
        before = ctx.memory()["arena_in_use"]
        ctx.air_compose(entries, random_coeff, dst, dst_log)
        after = ctx.memory()["arena_in_use"]
        got = np.stack([ctx.download(p, 1 << dst_log) for p in dst])
        roots.append(s.commit(ch, dst, logs[3], form=1))
        oods = ch.draw_point()
        points, samples = pcs_replay.mask_of(hp, log_sizes, LMR, oods, conv[2])
        proof = s.prove_values(ch, points, samples)
    assert roots == [pcs_replay.root_bytes(h) for h in full["proof"]["commitments"]]
    return got, proof, before, after


BRAINFUCK = {"default": (STWO, None, "interpreted"), "prev_cur": ((0, 0, 1, 0), None, "interpreted"),
             "b2_q10_pow16": (STWO, dict(pow_bits=16, log_blowup_factor=2, n_queries=10), "interpreted"),
             "compiled": (STWO, None, "compiled"), "odd_components_compiled": (STWO, None, "mixed")}


@pytest.mark.parametrize("case", BRAINFUCK, ids=list(BRAINFUCK))
def test_brainfuck_composition_polynomial_and_proof(hooks_pkg, hctx, case):
    hp = hooks_pkg
    conv, cfg, how = BRAINFUCK[case]
    cfg = None if cfg is None else hp.PcsConfig(**cfg)
    raw, full, logs, trees = _capture(hp, hctx, conv, cfg)
    which = {"interpreted": lambda k: False, "compiled": lambda k: True, "mixed": lambda k: k % 2 == 1}[how]
    with Dev(hctx) as dev:
        got, proof, before, after = _brainfuck_compose_in_session(hp, hctx, dev, full, logs, trees, conv, which)
    assert len({full["claim"][n]["log_size"] for n in pcs_replay.NAMES}) > 1      # several buckets
    for w in range(4):
        assert np.array_equal(got[w], trees[3][w]), (case, w)
    assert before == after and before > 0      # the session's arena is not touched
    want = pcs_replay.proof_member(raw)
    assert len(proof) == len(want) and proof == want, case


# ---- refusals and state -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_and_the_context_as_they_were(_ctx, pkg):
    ctx = _ctx
    abi = sys.modules[pkg.__name__ + "._abi"].abi
    with Dev(ctx) as dev:
        good = Comp(pkg, dev, "small", 5, 1, 1)
        off = Comp(pkg, dev, "offsets", 5, 1, 2)
        dst = [dev.up(np.full(64, 0x5A5A5A5A, dtype=np.uint32)) for _ in range(4)]
        g = good.entry()

        def with_(**kw):
            d = dict(program=g[0], log_size=5, log_expand=1, cols=g[3], params=g[4], shifts=None)
            d.update(kw)
            return (d["program"], d["log_size"], d["log_expand"], d["cols"], d["params"], d["shifts"])

        bad_param = [[P, 0, 0, 0]]
        for entries, r, dst_log, what in (
                ([], R, 6, r"^bfhip_air_compose: 1 to BFHIP_AIR_COMPOSE_MAX_COMPONENTS \(64\) components, got 0$"),
                ([g] * 65, R, 6, r"^bfhip_air_compose: 1 to BFHIP_AIR_COMPOSE_MAX_COMPONENTS \(64\) components, got 65$"),
                ([g, with_(log_expand=0)], R, 6, r"^bfhip_air_compose: component 1: log_expand must be in \[1, 3\], got 0$"),
                ([with_(log_expand=4)], R, 9, r"^bfhip_air_compose: component 0: log_expand must be in \[1, 3\], got 4$"),
                ([g, g, with_(log_size=0)], R, 6, "^bfhip_air_compose: component 2: log_size must be at least 1"),
                ([with_(log_size=ctx.max_log_domain - 1, log_expand=2)], R, ctx.max_log_domain + 1, "^bfhip_air_compose: component 0: log_size \\+ log_expand = %d exceeds the context's max_log_domain" % (ctx.max_log_domain + 1)),
                ([with_(shifts=[0, 1])], R, 6, "^bfhip_air_compose: component 0: column 1 has shift 1 "),
                ([with_(shifts=[0, 7])], R, 6, "^bfhip_air_compose: component 0: column 1 has shift 7 "),
                ([g, (off.program, 5, 1, off.ptrs, [], [4, 0, 0, 0, 0])], R, 6, "^bfhip_air_compose: component 1: column 0 is stored with shift 4 and read at a non-zero offset$"),
                ([with_(params=[])], R, 6, "^bfhip_air_compose: component 0: the program takes 1 parameters, got 0$"),
                ([with_(params=bad_param)], R, 6, "^bfhip_air_compose: component 0: a parameter word is not a canonical M31$"),
                ([g], [0, 0, P, 0], 6, "^bfhip_air_compose: random_coeff: a word is not a canonical M31$"),
                ([g], R, 5, "^bfhip_air_compose: dst_log must be the largest log_size \\+ log_expand of the list, 6, got 5$"),
                ([g, with_(log_size=4)], R, 7, "^bfhip_air_compose: dst_log must be the largest log_size \\+ log_expand of the list, 6, got 7$")):
            with pytest.raises(pkg.BfhipError, match=what):
                ctx.air_compose(entries, r, dst, dst_log)

        # the struct itself: reserved, neither program nor kernel, null pointers, a kernel of another context
        entry, r4, dst4 = abi().bfhip_air_compose, (ctypes.c_uint32 * 4)(*R), (ctypes.c_void_p * 4)(*dst)
        cols, pars = (ctypes.c_void_p * 2)(*good.ptrs), (ctypes.c_uint32 * 4)(*good.params[0])
        make = lambda **kw: pkg.AirComponent(**{**dict(program=good.program._h.value, kernel=None, log_size=5, log_expand=1, cols_h=ctypes.cast(cols, ctypes.POINTER(ctypes.c_void_p)),
                                                       col_shifts_h=None, params_h=pars, n_params=1, reserved=0), **kw})
        arr = lambda *cs: (pkg.AirComponent * len(cs))(*cs)

        def refused(rc, what):
            assert rc == -1 and abi().bfhip_last_error().decode() == what, abi().bfhip_last_error().decode()

        refused(entry(ctx._h, arr(make(), make(reserved=1)), 2, r4, 6, dst4), "bfhip_air_compose: component 1: reserved must be 0")
        refused(entry(ctx._h, arr(make(program=None)), 1, r4, 6, dst4), "bfhip_air_compose: component 0: neither program nor kernel is set")
        refused(entry(ctx._h, arr(make(cols_h=None)), 1, r4, 6, dst4), "bfhip_air_compose: component 0: null argument")
        refused(entry(ctx._h, arr(make(params_h=None)), 1, r4, 6, dst4), "bfhip_air_compose: component 0: null argument")
        refused(entry(ctx._h, None, 1, r4, 6, dst4), "bfhip_air_compose: null argument")
        refused(entry(ctx._h, arr(make()), 1, None, 6, dst4), "bfhip_air_compose: null argument")
        refused(entry(ctx._h, arr(make()), 1, r4, 6, None), "bfhip_air_compose: null argument")
        refused(entry(ctx._h, arr(make()), 1, r4, 6, (ctypes.c_void_p * 4)(dst[0], dst[1], None, dst[3])), "bfhip_air_compose: null destination pointer")
        other = pkg.Context(0, max_log_domain=10)
        try:
            foreign = other.air_compile(good.program)
            refused(entry(ctx._h, arr(make(), make(program=None, kernel=foreign._h.value)), 2, r4, 6, dst4),
                    "bfhip_air_compose: component 1: the kernel was compiled by another context (a module belongs to the context that loaded it)")
            foreign.close()
        finally:
            other.close()
        # a member of a shard group
        group, member = pkg.LocalGroup(2), pkg.Context(0, max_log_domain=10)
        try:
            member.join_local_group(group, 0)
            with pytest.raises(pkg.BfhipError, match=r"^bfhip_air_compose: a context in a shard group is not supported \(bfhip_ctx_leave_group first\)$"):
                member.air_compose([g], R, dst, 6)
            member.leave_group()
        finally:
            member.close(); group.close()

        # nothing was written, and the context computes: one parity case again
        assert all((ctx.download(p, 64) == 0x5A5A5A5A).all() for p in dst)
        assert entry(ctx._h, arr(make()), 1, r4, 6, dst4) == 0
        comps = [Comp(pkg, dev, name, ls, le, 1000 + 7 * k) for k, (name, ls, le) in enumerate(SHAPES["one_bucket_three_log_sizes"])]
        assert np.array_equal(_compose(ctx, dev, [c.entry() for c in comps], R, 7), _sequence(pkg, ctx, comps, R))
        assert np.array_equal(np.stack([ctx.download(p, 64) for p in dst]), _sequence(pkg, ctx, [good], R))
