"""-m gpu: the constraint program on the constraint domain (bfhip_air_eval_domain, csrc/air_program.hip) — bit-exact parity with the oracle's
evaluate_constraint_quotients_on_domain for the 13 Brainfuck components written as programs, a synthetic AIR with offsets -2 .. +2 at blowups
2, 4 and 8 against its own quotient's degree, the out-of-domain evaluator and the numpy model of tests/air_model.py, the same AIR proved and
verified end to end through the commitment-scheme session, and the refusals. Integer field arithmetic: every comparison is exact."""
import numpy as np
import pytest

import air_model
import pcs_replay
from conftest import splitmix_column, P

pytestmark = pytest.mark.gpu

ALL_OPS = ("+++>,<[>+.<-]", b"\x01")       # tests/test_gpu_components.py
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


_CASES = {}


def _component_case(oracle, name, comp):
    """Inputs and the oracle's result for one component of one program, computed once: full-size LDE columns in the program's column order
    (main, logUp coordinates, IsFirst), lookup elements, claimed sum, coefficients, starting accumulator, expected accumulator."""
    if (name, comp) not in _CASES:
        code, inp = PROGS[name]
        elems = _elems(77)
        rows = np.ascontiguousarray(oracle.table(code, inp, comp).T)
        n_main, M = rows.shape
        log = int(np.log2(M)) + 4
        n = 1 << (log + 1)
        lde = lambda cols: oracle.evaluate(oracle.interpolate(cols, log), log, log + 1)
        inter, claimed = oracle.logup_generate(comp, rows, elems)
        main_lde, inter_lde = lde(np.repeat(rows, 16, axis=1)), lde(inter)
        one_hot = np.zeros((1, 1 << log), dtype=np.uint32); one_hot[0, 0] = 1
        is_first = lde(one_hot)[0]
        n_cons = [12, 11, 5, 10, 9, 9, 7, 7, 8, 8, 8, 7, 2][comp]
        coeffs = splitmix_column(500 + comp, 4 * n_cons)
        acc0 = np.stack([splitmix_column(900 + k, n) for k in range(4)])      # non-zero start: the operation accumulates
        want = oracle.eval_constraints(comp, log, is_first, main_lde, inter_lde, elems, claimed, coeffs, acc0)
        _CASES[(name, comp)] = dict(log=log, cols=np.concatenate([main_lde, inter_lde, is_first[None]]), n_main=n_main, n_logup=inter.shape[0] // 4, elems=elems,
                                    claimed=claimed, coeffs=coeffs.reshape(n_cons, 4).tolist(), acc0=acc0, want=want)
    return _CASES[(name, comp)]


def _run_component(ctx, pkg, case, comp, shifted):
    program, _, _ = pkg.brainfuck_air_program(comp)
    n_rep = case["n_main"] + 4 * (case["n_logup"] - 1)
    shifts = [4 if shifted and k < n_rep else 0 for k in range(len(case["cols"]))]
    n = 2 << case["log"]
    with Dev(ctx) as dev:
        cols = [dev.up(c[:: 1 << s]) for c, s in zip(case["cols"], shifts)]
        acc = [dev.up(case["acc0"][k]) for k in range(4)]
        ctx.air_eval_domain(program, case["log"], 1, cols, pkg.brainfuck_air_params(case["elems"], case["claimed"]), case["coeffs"], acc, col_shifts=shifts)
        return np.stack([ctx.download(p, n) for p in acc])


def _denominators(ctx, pkg, log_size, log_expand):
    """1 / vanishing per row, from a launch of the one-constraint program const(1) with coefficient 1 into a zero accumulator."""
    b = pkg.AirBuilder()
    b.constraint(b.const(1))
    n = 1 << (log_size + log_expand)
    with Dev(ctx) as dev:
        acc = [dev.up(np.zeros(n, dtype=np.uint32)) for _ in range(4)]
        ctx.air_eval_domain(b.program(), log_size, log_expand, [], [], [ONE], acc)
        got = np.stack([ctx.download(p, n) for p in acc])
    assert not got[1:].any()
    return got[0]


@pytest.mark.parametrize("storage", ["full_size", "shift_4"])
@pytest.mark.parametrize("name", ["all_ops", "hello"])
def test_brainfuck_programs_match_the_oracle(_ctx, pkg, _oracle, name, storage):
    """air_eval_domain(log_expand = 1) of the 13 programs == oracle.eval_constraints bit for bit, from a non-zero accumulator: full-size
    columns, and the main columns and the earlier logUp columns at shift 4 (the last logUp column and IsFirst full size). log_size 4 .. 15:
    domains below one 64-lane workgroup (32 rows) and of 2 to 1024 workgroups; the synthetic AIR below adds the domain of exactly one."""
    logs = set()
    for comp in range(13):
        case = _component_case(_oracle, name, comp)
        got = _run_component(_ctx, pkg, case, comp, storage == "shift_4")
        assert np.array_equal(got, case["want"]), NAMES[comp]
        logs.add(case["log"])
        if storage == "full_size":
            # the same through the numpy model times the denominators a const(1) launch shows: pins those denominators to the oracle's
            program, _, _ = pkg.brainfuck_air_program(comp)
            n = 2 << case["log"]
            den = _denominators(_ctx, pkg, case["log"], 1)
            assert np.array_equal(den, np.repeat(den[:: 1 << case["log"]], 1 << case["log"])) and den[0] != den[-1]
            model = air_model.run(program.code, air_model.domain_reader(case["cols"], case["log"], 1), pkg.brainfuck_air_params(case["elems"], case["claimed"]), case["coeffs"], n)
            model = air_model.q_mul(model, air_model.from_m(den.astype(np.uint64)))
            assert np.array_equal((model + case["acc0"]) % np.uint64(P), case["want"]), NAMES[comp]
    print(name, storage, "log sizes", sorted(logs))
    assert min(logs) == 4 and max(logs) >= 9      # 32 rows: less than one workgroup; 2^10 rows and more: many


# ---- a synthetic AIR written with AirBuilder ----------------------------------------------------------------------------------------------
A, B, OUT, NXT, PRV, NXT2, PRV2 = range(7)


def _synthetic_program(pkg, d):
    """out = a * b^(d - 1) (degree d) and four shifted copies of a: nxt = a[+1], prv = a[-1], nxt2 = a[+2], prv2 = a[-2]."""
    b = pkg.AirBuilder()
    a, bb, out = b.col(A), b.col(B), b.col(OUT)
    prod = a
    for _ in range(d - 1):
        prod = prod * bb
    b.constraint(out - prod)
    b.constraint(b.col(NXT) - b.col(A, 1))
    b.constraint(b.col(PRV) - b.col(A, -1))
    b.constraint(b.col(NXT2) - b.col(A, 2))
    b.constraint(b.col(PRV2) - b.col(A, -2))
    return b.program()


def _storage_of_coset_order(col, log_size):
    """Coset order -> bit-reversed circle-domain order: cell s holds the value of coset index 2 d (d < n / 2) or 2 (n - 1 - d) + 1, d = the
    bit reversal of s — the index map prev_trace_cell of csrc/air.h walks, inverted."""
    n = 1 << log_size
    d = air_model.bit_reverse(np.arange(n), log_size)
    return col[np.where(d < n // 2, 2 * d, 2 * (n - 1 - d) + 1)]


def _synthetic_trace(log_size, d, seed):
    """The 7 columns in storage order; the shifted copies close cyclically, so no IsFirst is needed."""
    n = 1 << log_size
    a, b = splitmix_column(seed, n).astype(np.uint64), splitmix_column(seed + 1, n).astype(np.uint64)
    out = a.copy()
    for _ in range(d - 1):
        out = out * b % np.uint64(P)
    coset = [a, b, out, np.roll(a, -1), np.roll(a, 1), np.roll(a, -2), np.roll(a, 2)]
    return np.stack([_storage_of_coset_order(c, log_size) for c in coset]).astype(np.uint32)


def _sweep(ctx, program, log_size, log_expand, lde, coeffs):
    n = 1 << (log_size + log_expand)
    with Dev(ctx) as dev:
        cols = [dev.up(c) for c in lde]
        acc = [dev.up(np.zeros(n, dtype=np.uint32)) for _ in range(4)]
        ctx.air_eval_domain(program, log_size, log_expand, cols, [], coeffs, acc)
        return np.stack([ctx.download(p, n) for p in acc])


_circle_x = air_model.circle_x      # x coordinate of G^index, G the generator of the M31 circle group


@pytest.mark.parametrize("log_size", [4, 9])
@pytest.mark.parametrize("d,log_expand", [(2, 1), (3, 2), (5, 3)])
def test_synthetic_air_on_larger_blowups(_ctx, pkg, _oracle, d, log_expand, log_size):
    ctx, el = _ctx, log_size + log_expand
    n = 1 << el
    program = _synthetic_program(pkg, d)
    assert program.mask() == [(A, 0), (A, 1), (A, -1), (A, 2), (A, -2), (B, 0), (OUT, 0), (NXT, 0), (PRV, 0), (NXT2, 0), (PRV2, 0)]
    trace = _synthetic_trace(log_size, d, 40 + d)
    coeffs_of = lambda cols: _oracle.interpolate(cols, log_size)
    lde = _oracle.evaluate(coeffs_of(trace), log_size, el)
    coeffs = _quads(300 + d, 5)
    acc = _sweep(ctx, program, log_size, log_expand, lde, coeffs)

    # (a) the quotient is a polynomial: the upper half of its coefficients is zero. Coefficient j belongs to y^(j & 1) * prod_i pi^(i-1)(x)^(bit i
    # of j); a trace polynomial's top term is y x^(2^log_size / 2 - 1). For odd d the quotient's top term is y x^(n / 4 - 1), the last basis
    # function of the lower half. For even d, y^d = (1 - x^2)^(d / 2) leaves the x-only term x^(n / 4) = the basis function of index n / 2 —
    # the one dimension by which a degree-2 quotient exceeds half of a blowup-2 domain (why stwo commits it at log_size + 1). So for d = 2
    # the first coefficient of the upper half is free and everything above it is zero. (tests/air_model.py alone, no kernel, shows the same.)
    acc_coeffs = _oracle.interpolate(acc, el)
    upper = n // 2 + (1 if d % 2 == 0 else 0)
    print("d", d, "log_expand", log_expand, "log_size", log_size, "non-zero coefficients at or above n / 2:", np.nonzero(acc_coeffs[:, n // 2:].any(axis=0))[0].tolist())
    assert acc.any() and not acc_coeffs[:, upper:].any()

    # (c) row by row against the numpy model; denominators from a const(1) launch: 2^log_expand distinct values indexed by row >> log_size,
    # equal to 1 / (x of the domain point doubled log_size - 1 times) at the first point of each class
    den = _denominators(ctx, pkg, log_size, log_expand)
    table = den[:: 1 << log_size]
    assert len(table) == 1 << log_expand == len(set(table.tolist())) and np.array_equal(den, np.repeat(table, 1 << log_size))
    for i, v in enumerate(table.tolist()):
        dd = int(air_model.bit_reverse([i << log_size], el)[0])      # circle-domain index of storage row i << log_size
        half = n // 2
        x = _circle_x((1 << (30 - el)) + (dd % half) * (1 << (32 - el)))
        for _ in range(log_size - 1):
            x = (2 * x * x - 1) % P
        assert v * x % P == 1, (i, v, x)
    assert np.array_equal(den, air_model.domain_denominators(log_size, log_expand))      # the same for every row, from the model
    model = air_model.run(program.code, air_model.domain_reader(lde, log_size, log_expand), [], coeffs, n)
    assert np.array_equal(air_model.q_mul(model, air_model.from_m(den.astype(np.uint64))), acc)

    # (b) at a channel-drawn point: the mask values are the columns' polynomials at the shifted points; the point evaluator on them equals the
    # interpolated accumulator at the point
    ch = pkg.Channel((0, 0, 0, 0))
    ch.mix_u64(1000 * d + log_size)
    point = ch.draw_point()
    with Dev(ctx) as dev:
        co = [dev.up(c) for c in coeffs_of(trace)]
        mask_values = [ctx.eval_at_point(co[col], log_size, pkg.circle_point_offset(point, log_size, off)) for col, off in program.mask()]
        acc_at = [ctx.eval_at_point(dev.up(c), el, point) for c in acc_coeffs]
    assert program.eval_at_point(log_size, point, mask_values, [], coeffs) == pcs_replay.from_partial_evals(acc_at)

    # (d) one trace cell changed: no polynomial quotient any more
    bad = trace.copy()
    bad[PRV, 3] = (int(bad[PRV, 3]) + 1) % P
    bad_acc = _sweep(ctx, program, log_size, log_expand, _oracle.evaluate(coeffs_of(bad), log_size, el), coeffs)
    assert _oracle.interpolate(bad_acc, el)[:, upper:].any()


# ---- end to end through the commitment-scheme session --------------------------------------------------------------------------------------
def _session_program(pkg):
    """The synthetic AIR (d = 2) over the same trace with each shift read from the copy's side: nxt[-1] = a, prv[+1] = a, nxt2[-2] = a,
    prv2[+2] = a. The same five statements about the same seven columns, and no column is opened at more than two points, which is what a
    session accepts (BFHIP_PCS_MAX_SAMPLES_PER_COLUMN = 2; the form of the test above opens `a` at five)."""
    b = pkg.AirBuilder()
    a = b.col(A)
    b.constraint(b.col(OUT) - a * b.col(B))
    b.constraint(b.col(NXT, -1) - a)
    b.constraint(b.col(PRV, 1) - a)
    b.constraint(b.col(NXT2, -2) - a)
    b.constraint(b.col(PRV2, 2) - a)
    return b.program()


def _prove_and_verify(ctx, pkg, program, trace, log_size):
    """(verifier's verdict, sampled composition value, point evaluator on the sampled mask values)"""
    n_cols, mask = len(trace), program.mask()
    offsets = sorted({off for _, off in mask}, key=lambda o: (o != 0, o))
    with Dev(ctx) as dev:
        ch = pkg.Channel((0, 0, 0, 0))
        with pkg.PcsSession(ctx) as s:
            root0 = s.commit(ch, [dev.up(c) for c in trace], [log_size] * n_cols, form=0)
            random_coeff = ch.draw_felt()
            powers = [ONE]
            for _ in range(program.shape["n_constraints"] - 1):
                powers.append(pcs_replay.q_mul(powers[-1], random_coeff))
            coeffs = powers[::-1]                                     # stwo's accumulator order: constraint j gets r^(N - 1 - j)
            _, lde = s.tree_columns(0)                                # the session's own LDE columns: blowup 2 = the constraint domain
            n = 2 << log_size
            acc = [dev.up(np.zeros(n, dtype=np.uint32)) for _ in range(4)]
            ctx.air_eval_domain(program, log_size, 1, lde, [], coeffs, acc)      # works while the session is open
            comp = [dev.empty(n) for _ in range(4)]
            ctx.interpolate(acc, comp, log_size + 1)
            root1 = s.commit(ch, comp, [log_size + 1] * 4, form=1)
            oods = ch.draw_point()
            points = [pkg.circle_point_offset(oods, log_size, off) for off in offsets]
            assert points[0] == oods
            samples = [[[offsets.index(off) for c, off in mask if c == col] for col in range(n_cols)], [[0]] * 4]
            proof, sampled = s.prove_values(ch, points, samples, with_sampled=True)
    vch, v = pkg.Channel((0, 0, 0, 0)), pkg.PcsVerifier((0, 0, 0, 0))
    v.commit(vch, root0, [log_size] * n_cols)
    assert vch.draw_felt() == random_coeff
    v.commit(vch, root1, [log_size + 1] * 4)
    assert vch.draw_point() == oods
    verdict = v.verify_values(vch, points, samples, proof)
    assert len(sampled) == len(mask) + 4
    return verdict, pcs_replay.from_partial_evals(sampled[-4:]), program.eval_at_point(log_size, oods, sampled[: len(mask)], [], coeffs)


def test_synthetic_air_proved_and_verified_through_the_session(_ctx, pkg):
    """Commit the trace, draw the coefficient, sweep with the program, commit the composition polynomial's four coordinate columns (form 1),
    open everything with AirProgram.mask() as the sample description; a verifier session accepts, and the sampled composition value is the
    program at the sampled mask values. A corrupted trace still opens correctly — and fails that equality."""
    log_size = 6
    _ctx.set_pcs_config(pkg.PcsConfig())      # blowup 2: the session's LDE domain is the constraint domain of a degree-2 AIR
    program = _session_program(pkg)
    assert max(sum(1 for c, _ in program.mask() if c == col) for col in range(7)) <= pkg.PCS_MAX_SAMPLES_PER_COLUMN
    assert {off for _, off in program.mask()} == {0, -1, 1, -2, 2}
    trace = _synthetic_trace(log_size, 2, 71)
    verdict, sampled_value, at_point = _prove_and_verify(_ctx, pkg, program, trace, log_size)
    assert verdict == (True, "") and sampled_value == at_point and any(sampled_value)
    bad = trace.copy()
    bad[OUT, 17] = (int(bad[OUT, 17]) + 1) % P
    verdict, sampled_value, at_point = _prove_and_verify(_ctx, pkg, program, bad, log_size)
    assert verdict == (True, "") and sampled_value != at_point


def test_refusals_leave_the_context_usable(_ctx, pkg, _oracle):
    ctx = _ctx
    program = _synthetic_program(pkg, 2)
    coeffs = _quads(1, 5)
    with Dev(ctx) as dev:
        col = dev.up(np.zeros(1 << 7, dtype=np.uint32))
        cols, acc = [col] * 7, [dev.up(np.zeros(1 << 7, dtype=np.uint32)) for _ in range(4)]
        for kwargs, what in ((dict(log_expand=0), "log_expand must be in"), (dict(log_expand=4), "log_expand must be in"),
                             (dict(log_size=ctx.max_log_domain - 1, log_expand=2), "max_log_domain"), (dict(log_size=0), "log_size"),
                             (dict(col_shifts=[4, 0, 0, 0, 0, 0, 0]), "column 0 is stored with shift 4 and read at a non-zero offset"),
                             (dict(col_shifts=[0, 1, 0, 0, 0, 0, 0]), "shift 1"),
                             (dict(coeffs=coeffs[:4]), "has 5 constraints, got 4 coefficients"), (dict(coeffs=coeffs + [ONE]), "got 6 coefficients"),
                             (dict(params=[ONE]), "takes 0 parameters, got 1"), (dict(coeffs=coeffs[:4] + [[P, 0, 0, 0]]), "canonical")):
            args = dict(log_size=5, log_expand=2, params=[], coeffs=coeffs, col_shifts=None)
            args.update(kwargs)
            with pytest.raises(pkg.BfhipError, match=what):
                ctx.air_eval_domain(program, args["log_size"], args["log_expand"], cols, args["params"], args["coeffs"], acc, col_shifts=args["col_shifts"])
            # the C ABI's own answer: -1 with the message
            assert what.split(" must")[0] in pkg.lib().bfhip_last_error().decode()
        # a column stored with a shift and read at offset 0 only is fine
        ctx.air_eval_domain(program, 5, 2, cols, [], coeffs, acc, col_shifts=[0, 4, 4, 0, 0, 0, 0])
        assert not np.stack([ctx.download(p, 1 << 7) for p in acc]).any()
    # the context still computes: one case of the parity test again
    case = _component_case(_oracle, "all_ops", 3)
    assert np.array_equal(_run_component(ctx, pkg, case, 3, False), case["want"])
