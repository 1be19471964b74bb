"""-m gpu: constraint programs compiled to their own gfx950 kernel at run time (bfhip_air_compile / bfhip_air_kernel_eval_domain,
csrc/air_codegen.hip + csrc/air_compile.hip) held to the interpreter (bfhip_air_eval_domain) and, for the 13 Brainfuck components, to the
built-in kernels (bfhip_eval_constraints), bit for bit: below one workgroup and over several, full-size and shifted columns, offsets up to
+-16 at blowups 2, 4 and 8, the lazy reduction's seams at saturated values, a program at the caps, the interpreter's refusals, the cache,
an open session, a destroyed context, and a lookup AIR proved twice to the same bytes. Integer field arithmetic: every comparison is exact.
Kernels are compiled once per module. A failure to find or drive libhiprtc fails these tests with the library's message."""
import numpy as np
import pytest

import air_codegen_cases as cases
import pcs_replay
import test_gpu_air_program as synthetic
import test_gpu_logup_program as lookup
from conftest import splitmix_column, P
from test_gpu_air_program import Dev, ONE, NAMES

pytestmark = pytest.mark.gpu

N_CONS = [12, 11, 5, 10, 9, 9, 7, 7, 8, 8, 8, 7, 2]


def _quads(seed, n):
    return splitmix_column(seed, 4 * n).reshape(n, 4).tolist()


@pytest.fixture(scope="module")
def compiled(_ctx, pkg):
    """name -> (AirProgram, CompiledAir on the session's context); each program goes through the compiler once for the whole module"""
    progs = {NAMES[k]: pkg.brainfuck_air_program(k)[0] for k in range(13)}
    progs["synthetic_pm2"] = synthetic._synthetic_program(pkg, 3)
    progs["synthetic_pm16"] = cases.synthetic_wide_program(pkg)
    for n_base in (4, 5, 8, 9, 64):
        progs["run_%d" % n_base] = cases.constraint_run_program(pkg, n_base)
    progs["run_interleaved"] = cases.constraint_run_program(pkg, 40, interleave_ext=True)
    # the caps program of the CPU suite, all 4096 instructions: its compile takes two to three seconds of this fixture, once per module
    code, n_cols, n_params, _ = cases.caps_program(2024)
    progs["caps"] = pkg.AirProgram(code, n_cols, n_params)
    out = {name: (prog, _ctx.air_compile(prog)) for name, prog in progs.items()}
    yield out
    for _, kernel in out.values():
        kernel.close()


def _sweep(ctx, what, log_size, log_expand, cols, shifts, params, coeffs, acc0):
    n = 1 << (log_size + log_expand)
    with Dev(ctx) as dev:
        ptrs = [dev.up(c) for c in cols]
        acc = [dev.up(acc0[k]) for k in range(4)]
        ctx.air_eval_domain(what, log_size, log_expand, ptrs, params, coeffs, acc, col_shifts=shifts)
        return np.stack([ctx.download(p, n) for p in acc])


def _acc0(n, seed=900):
    return np.stack([splitmix_column(seed + k, n) for k in range(4)])      # a non-zero start: the sweep accumulates


# ---- 1. the 13 components: compiled == interpreter == built-in -------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["full_size", "shift_4"])
@pytest.mark.parametrize("log_size", [5, 9])
def test_components_equal_the_interpreter_and_the_builtin_kernels(_ctx, pkg, compiled, log_size, storage):
    """log_size 5: 64 rows, fewer than one 256-lane workgroup (the tail guard); log_size 9: 1024 rows, four workgroups. Random cells (the
    sweep does not care whether a trace satisfies its AIR); shift_4: the main columns and the earlier logUp columns hold one cell per 16 rows."""
    ctx, n = _ctx, 2 << log_size
    elems = splitmix_column(77, 24)
    elems[elems == 0] = 1
    elems, claimed = elems.tolist(), splitmix_column(78, 4).tolist()
    acc0 = _acc0(n)
    for comp in range(13):
        program, kernel = compiled[NAMES[comp]]
        n_cols = program.shape["n_cols"]
        n_logup = 3 if comp == 3 else 1
        n_main = n_cols - 4 * n_logup - 1
        n_rep = n_main + 4 * (n_logup - 1)
        shifts = [4 if storage == "shift_4" and k < n_rep else 0 for k in range(n_cols)]
        cols = [splitmix_column(1000 * comp + k, n >> s) for k, s in enumerate(shifts)]
        coeffs = _quads(500 + comp, N_CONS[comp])
        params = pkg.brainfuck_air_params(elems, claimed)
        got = _sweep(ctx, kernel, log_size, 1, cols, shifts, params, coeffs, acc0)
        interpreted = _sweep(ctx, program, log_size, 1, cols, shifts, params, coeffs, acc0)
        with Dev(ctx) as dev:
            ptrs = [dev.up(c) for c in cols]
            acc = [dev.up(acc0[k]) for k in range(4)]
            ctx.eval_constraints(comp, log_size, ptrs[-1], ptrs[:n_main], ptrs[n_main:-1], elems, claimed, [w for q in coeffs for w in q], acc,
                                 main_shifts=shifts[:n_main], inter_shifts=shifts[n_main:-1])
            builtin = np.stack([ctx.download(p, n) for p in acc])
        assert np.array_equal(got, interpreted), NAMES[comp]
        assert np.array_equal(got, builtin), NAMES[comp]
        assert not np.array_equal(got, acc0), NAMES[comp]


# ---- 2. offsets and blowups --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_size", [4, 5, 10])
@pytest.mark.parametrize("log_expand", [1, 2, 3])
@pytest.mark.parametrize("name", ["synthetic_pm2", "synthetic_pm16"])
def test_offsets_and_blowups_equal_the_interpreter(_ctx, compiled, name, log_expand, log_size):
    """Offsets -2 .. +2 and +-16 at blowups 2, 4 and 8. At log_size 4 offset 16 is a whole turn of the trace coset: the row itself, which the
    second assertion states without the interpreter."""
    program, kernel = compiled[name]
    n = 1 << (log_size + log_expand)
    cols = [splitmix_column(40 + 7 * log_size + k, n) for k in range(program.shape["n_cols"])]
    coeffs = _quads(300 + log_expand, program.shape["n_constraints"])
    acc0 = _acc0(n, 910)
    got = _sweep(_ctx, kernel, log_size, log_expand, cols, None, [], coeffs, acc0)
    assert np.array_equal(got, _sweep(_ctx, program, log_size, log_expand, cols, None, [], coeffs, acc0))
    assert not np.array_equal(got, acc0)
    if name == "synthetic_pm16" and log_size == 4:
        # nxt - a[+16] and prv - a[-16] read a at the row itself: with nxt = prv = a both vanish, and the product constraint with out = a b
        a, b = cols[0].astype(np.uint64), cols[1].astype(np.uint64)
        closed = [cols[0], cols[1], (a * b % np.uint64(P)).astype(np.uint32), cols[0], cols[0]]
        assert np.array_equal(_sweep(_ctx, kernel, log_size, log_expand, closed, None, [], coeffs, acc0), acc0)


# ---- 3. the lazy reduction's seams, saturated ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", ["p_minus_1", "random"])
@pytest.mark.parametrize("name", ["run_4", "run_5", "run_8", "run_9", "run_64", "run_interleaved"])
def test_lazy_reduction_seams_equal_the_interpreter(_ctx, compiled, name, cells):
    """4, 5, 8, 9 and 64 base-field constraints in a row (the fold comes before every fifth product), and base and extension constraints
    interleaved; every cell, parameter word and coefficient word p - 1 (each 64-bit dot product reaches 4 (p - 1)^2 on top of a folded
    accumulator), and random."""
    program, kernel = compiled[name]
    s, log_size, log_expand = program.shape, 7, 1
    n = 1 << (log_size + log_expand)
    if cells == "p_minus_1":
        cols = [np.full(n, P - 1, dtype=np.uint32) for _ in range(s["n_cols"])]
        params, coeffs = [[P - 1] * 4] * s["n_params"], [[P - 1] * 4] * s["n_constraints"]
    else:
        cols = [splitmix_column(60 + k, n) for k in range(s["n_cols"])]
        params, coeffs = _quads(61, s["n_params"]), _quads(62, s["n_constraints"])
    acc0 = _acc0(n, 920)
    got = _sweep(_ctx, kernel, log_size, log_expand, cols, None, params, coeffs, acc0)
    assert np.array_equal(got, _sweep(_ctx, program, log_size, log_expand, cols, None, params, coeffs, acc0))
    assert not np.array_equal(got, acc0)


# ---- 4. the caps -----------------------------------------------------------------------------------------------------------------------------------
def test_program_at_the_register_caps_equals_the_interpreter(_ctx, compiled):
    program, kernel = compiled["caps"]
    s = program.shape
    assert (s["m_regs"], s["q_regs"], s["n_constraints"], s["n_instr"], s["min_offset"], s["max_offset"]) == (96, 24, 64, 4096, -16, 16)
    print("caps", kernel.info())      # scratch above 0 is reported, not refused
    log_size, log_expand = 6, 2
    n = 1 << (log_size + log_expand)
    cols = [splitmix_column(5000 + k, n) for k in range(s["n_cols"])]
    params, coeffs = _quads(71, s["n_params"]), _quads(72, s["n_constraints"])
    acc0 = _acc0(n, 930)
    got = _sweep(_ctx, kernel, log_size, log_expand, cols, None, params, coeffs, acc0)
    assert np.array_equal(got, _sweep(_ctx, program, log_size, log_expand, cols, None, params, coeffs, acc0))
    assert not np.array_equal(got, acc0)


# ---- 5. the contract -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_the_interpreters(_ctx, pkg, compiled):
    """Each bad argument gives the same message from the compiled kernel's entry point as from bfhip_air_eval_domain."""
    ctx = _ctx
    program, kernel = compiled["synthetic_pm2"]
    coeffs = _quads(1, 5)
    with Dev(ctx) as dev:
        col = dev.up(np.zeros(1 << 7, dtype=np.uint32))
        cols, acc = [col] * 7, [dev.up(np.zeros(1 << 7, dtype=np.uint32)) for _ in range(4)]
        for kwargs in (dict(coeffs=coeffs[:4]), dict(coeffs=coeffs + [ONE]), dict(params=[ONE]), dict(coeffs=coeffs[:4] + [[P, 0, 0, 0]]),
                       dict(col_shifts=[4, 0, 0, 0, 0, 0, 0]), dict(col_shifts=[0, 1, 0, 0, 0, 0, 0]), dict(log_expand=0), dict(log_expand=4),
                       dict(log_size=0), dict(log_size=ctx.max_log_domain - 1, log_expand=2)):
            args = dict(log_size=5, log_expand=2, params=[], coeffs=coeffs, col_shifts=None)
            args.update(kwargs)
            messages = []
            for what in (program, kernel):
                with pytest.raises(pkg.BfhipError) as e:
                    ctx.air_eval_domain(what, args["log_size"], args["log_expand"], cols, args["params"], args["coeffs"], acc, col_shifts=args["col_shifts"])
                messages.append(str(e.value))
            print(messages[1])
            assert messages[0] == messages[1] and messages[0].startswith("bfhip_air_eval_domain: "), messages
        # still usable, and a shifted column read at offset 0 only is fine
        ctx.air_eval_domain(kernel, 5, 2, cols, [], coeffs, acc, col_shifts=[0, 4, 4, 0, 0, 0, 0])
        assert not np.stack([ctx.download(p, 1 << 7) for p in acc]).any()


def test_kernel_outlives_its_program_and_reports_the_cache(_ctx, pkg):
    """The program is destroyed before the kernel is used; a second compile of an equal program is served by the context's cache; after the
    last kernel of a source is gone the next compile builds again."""
    ctx = _ctx
    b = pkg.AirBuilder()
    b.constraint(b.col(0) * b.col(1) - b.col(2, 1) + 12345)
    program = b.program()
    code, log_size = list(program.code), 6
    n = 2 << log_size
    cols, coeffs, acc0 = [splitmix_column(80 + k, n) for k in range(3)], _quads(81, 1), _acc0(n, 940)
    want = _sweep(ctx, program, log_size, 1, cols, None, [], coeffs, acc0)
    first = ctx.air_compile(program)
    program.close()
    info = first.info()
    print(info)
    assert not info["from_cache"] and info["compile_us"] > 0 and info["vgprs"] > 0 and info["scratch_bytes"] == 0 and info["lds_bytes"] == 0
    assert info["code_object_bytes"] > 0 and info["source_bytes"] == len(pkg.AirProgram(code, 3, 0).source().encode())
    assert np.array_equal(_sweep(ctx, first, log_size, 1, cols, None, [], coeffs, acc0), want)
    with ctx.air_compile(pkg.AirProgram(code, 3, 0)) as second:
        again = second.info()
        assert again["from_cache"] and {k: v for k, v in again.items() if k != "from_cache"} == {k: v for k, v in info.items() if k != "from_cache"}
        first.close()      # the module stays: the second kernel uses it
        assert np.array_equal(_sweep(ctx, second, log_size, 1, cols, None, [], coeffs, acc0), want)
    with ctx.air_compile(pkg.AirProgram(code, 3, 0)) as third:
        assert not third.info()["from_cache"]
        assert np.array_equal(_sweep(ctx, third, log_size, 1, cols, None, [], coeffs, acc0), want)


def test_kernel_is_bound_to_its_context_and_survives_its_destruction(_ctx, pkg, compiled):
    """A kernel used with a second context is refused. bfhip_ctx_destroy with a live kernel cleans up: it unloads the module, and the kernel
    object can afterwards only be destroyed (info and eval_domain return -1)."""
    program, kernel = compiled["synthetic_pm2"]
    other = pkg.Context(0, max_log_domain=12)
    try:
        with Dev(other) as dev:
            cols = [dev.up(np.zeros(1 << 6, dtype=np.uint32)) for _ in range(7)]
            acc = [dev.up(np.zeros(1 << 6, dtype=np.uint32)) for _ in range(4)]
            with pytest.raises(pkg.BfhipError, match="compiled by another context"):
                other.air_eval_domain(kernel, 5, 1, cols, [], _quads(1, 5), acc)
            mine = other.air_compile(program)
            other.air_eval_domain(mine, 5, 1, cols, [], _quads(1, 5), acc)
            assert not np.stack([other.download(p, 1 << 6) for p in acc]).any()      # zero cells satisfy the synthetic AIR
    finally:
        other.close()
    with pytest.raises(pkg.BfhipError, match="context has been destroyed"):
        mine.info()
    with pytest.raises(pkg.BfhipError, match="compiled by another context"):
        _ctx.air_eval_domain(mine, 5, 1, [0] * 7, [], _quads(1, 5), [0] * 4)
    assert pkg.lib().bfhip_air_kernel_destroy(mine._h) == 0
    mine._h = None
    assert kernel.info()["vgprs"] > 0      # the first context's kernels are untouched


def test_components_take_no_scratch(compiled):
    """The 13 components keep at most 17 m and 6 q values live: straight-line code of that size fits the VGPR file by a wide
    margin, so any private segment would be a defect of the generated code."""
    for comp in range(13):
        info = compiled[NAMES[comp]][1].info()
        print(NAMES[comp], info)
        assert info["scratch_bytes"] == 0 and info["lds_bytes"] == 0 and 0 < info["vgprs"] <= 128, (NAMES[comp], info)


# ---- 6. inside a session, end to end -----------------------------------------------------------------------------------------------------------
def _prove_lookup(ctx, pkg, trace, log_size, sweep):
    """tests/test_gpu_logup_program.py's lookup AIR (a, t, mult, IsFirst, 8 interaction columns) through a
    session, the constraint sweep done by `sweep` (the program or its compiled kernel). Returns (proof bytes, roots, points, samples, what
    the verifier needs to replay the channel, arena in use before and after the sweep)."""
    fractions, program = lookup._lookup_fractions(pkg), lookup._lookup_constraints(pkg)
    n, mask = 1 << log_size, program.mask()
    with Dev(ctx) as dev:
        ch = pkg.Channel((0, 0, 0, 0))
        with pkg.PcsSession(ctx) as s:
            cols = [dev.up(c) for c in trace]
            roots = [s.commit(ch, cols, [log_size] * 4, form=0)]
            z, alpha = ch.draw_felts(2)
            inter = [dev.empty(n) for _ in range(8)]
            claimed = ctx.logup_program_generate(fractions, log_size, cols[:3], [z, alpha], inter)
            ch.mix_felts([claimed])
            roots.append(s.commit(ch, inter, [log_size] * 8, form=0))
            random_coeff = ch.draw_felt()
            lde = s.tree_columns(0)[1] + s.tree_columns(1)[1]
            acc = [dev.up(np.zeros(2 * n, dtype=np.uint32)) for _ in range(4)]
            before = ctx.memory()["arena_in_use"]
            ctx.air_eval_domain(sweep, log_size, 1, lde, [z, alpha, claimed], [random_coeff, ONE], acc)      # while the session is open
            after = ctx.memory()["arena_in_use"]
            comp = [dev.empty(2 * n) for _ in range(4)]
            ctx.interpolate(acc, comp, log_size + 1)
            roots.append(s.commit(ch, comp, [log_size + 1] * 4, form=1))
            oods = ch.draw_point()
            points = [oods, pkg.circle_point_offset(oods, log_size, -1)]
            per_col = [[{0: 0, -1: 1}[off] for c, off in mask if c == col] for col in range(12)]
            samples = [per_col[:4], per_col[4:], [[0]] * 4]
            proof = s.prove_values(ch, points, samples)
    return proof, roots, points, samples, claimed, (before, after)


def test_lookup_air_proved_with_either_sweep_gives_the_same_bytes(_ctx, pkg):
    """The lookup AIR at log_size 6 proved once with the interpreter's sweep and once with the compiled kernel's: the two proofs are
    byte-identical, the sweep leaves the arena's bookkeeping (bfhip_ctx_memory out[3]) alone inside the open session, and a verifier session
    accepts."""
    log_size = 6
    _ctx.set_pcs_config(pkg.PcsConfig())      # blowup 2: the session's LDE domain is the constraint domain of a degree-2 AIR
    program = lookup._lookup_constraints(pkg)
    trace = lookup._lookup_trace(log_size, 51)
    with _ctx.air_compile(program) as kernel:
        interpreted = _prove_lookup(_ctx, pkg, trace, log_size, program)
        compiled_run = _prove_lookup(_ctx, pkg, trace, log_size, kernel)
    assert bytes(compiled_run[0]) == bytes(interpreted[0]) and compiled_run[1] == interpreted[1] and compiled_run[4] == interpreted[4] == [0, 0, 0, 0]
    assert compiled_run[5][0] == compiled_run[5][1] and interpreted[5][0] == interpreted[5][1] and compiled_run[5][0] > 0
    proof, roots, points, samples, claimed, _ = compiled_run
    vch, v = pkg.Channel((0, 0, 0, 0)), pkg.PcsVerifier((0, 0, 0, 0))
    v.commit(vch, roots[0], [log_size] * 4)
    vch.draw_felts(2)
    vch.mix_felts([claimed])
    v.commit(vch, roots[1], [log_size] * 8)
    vch.draw_felt()
    v.commit(vch, roots[2], [log_size + 1] * 4)
    assert vch.draw_point() == points[0]
    assert v.verify_values(vch, points, samples, proof) == (True, "")
