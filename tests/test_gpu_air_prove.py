"""-m gpu: bfhip_air_prove / bfhip_air_verify (include/bfhip.h "Proving an AIR given as programs", csrc/air_prove.hip) — the driver against the
same protocol made call by call from Python over the entry points it is built of (PcsSession, Channel, logup_program_generate_batch,
evaluate, air_compose), byte for byte: the lookup AIR of INTEGRATION.md section 2e, the Brainfuck AIR over the captured polynomials of a real
proof (the proof member of bfhip_prove_brainfuck's result), the shapes a driver can get wrong, the failures and what they leave behind. All
comparisons are between bytes and integers."""
import json

import numpy as np
import pytest

import air_model
import pcs_replay
from conftest import P, splitmix_column
from test_gpu_pcs_session import LMR, MAX_LOG_DOMAIN, Dev, _capture

pytestmark = pytest.mark.gpu

STWO = (0, 0, 0, 0)
B2 = dict(pow_bits=5, log_blowup_factor=2, n_queries=3)


@pytest.fixture
def cctx(_ctx, pkg):
    yield _ctx
    _ctx.set_conventions(*STWO)
    _ctx.set_pcs_config(None)


# ---- the protocol, call by call: what INTEGRATION.md section 2e had a caller write before bfhip_air_prove ---------------------------------
def _resolve(pkg, rules, lookup, claimed):
    out = []
    for kind, relation, power, value in rules:
        if kind == 0:
            out.append(list(value))
        elif kind == 1:
            out.append(lookup[relation][0])
        elif kind == 3:
            out.append(claimed)
        else:
            cur = [1, 0, 0, 0]
            for _ in range(power):
                cur = pcs_replay.q_mul(cur, lookup[relation][1])
            out.append(cur)
    return out


def _describe(pkg, st, oods):
    """(points, samples, per component [(tree, column, position)]) from the programs' masks, in plain Python"""
    S = pkg.AirStatement
    frac = st.fraction_components
    it = len(st.trees)
    n_inter = {k: 4 * st.components[k][5].shape["n_logup_cols"] for k in frac}
    first, at = {}, 0
    for k in frac:
        first[k] = at
        at += n_inter[k]
    samples = [[[] for _ in t[0]] for t in st.trees] + ([[[] for _ in range(at)]] if frac else []) + [[[0] for _ in range(4)]]
    keys, points, refs = [(0, 0)], [list(oods)], []
    for k, (program, log_size, _, columns, _, _, _) in enumerate(st.components):
        refs.append([])
        for col, off in program.mask():
            key = (0, 0) if off == 0 else (log_size, off)
            if key not in keys:
                keys.append(key)
                points.append(pkg.circle_point_offset(oods, log_size, off))
            t, c = columns[col]
            if t == S.INTERACTION:
                t, c = it, first[k] + c
            if keys.index(key) not in samples[t][c]:
                samples[t][c].append(keys.index(key))
            refs[-1].append((t, c, samples[t][c].index(keys.index(key))))
    return points, samples, refs


def _hand_prove(pkg, ctx, st, tree_cols, ch, kernels=None):
    """(roots, claimed sums of the components with fractions, the CommitmentSchemeProof bytes, sampled composition value, composition at the point)"""
    S = pkg.AirStatement
    blowup = ctx.pcs_config().log_blowup_factor
    frac, it = st.fraction_components, len(st.trees)
    with Dev(ctx) as dev, pkg.PcsSession(ctx) as s:
        roots = []
        for t, (logs, form, mix) in enumerate(st.trees):
            for v in mix:
                ch.mix_u64(v)
            roots.append(s.commit(ch, tree_cols[t], logs, form=form))
        lookup = [ch.draw_felts(2) for _ in range(st.n_relations)]
        claimed, inter, inter_logs = {}, [], []
        if frac:
            batch = []
            for k in frac:
                _, log_size, _, _, rules, fractions, fcols = st.components[k]
                out = [dev.empty(1 << log_size) for _ in range(4 * fractions.shape["n_logup_cols"])]
                batch.append((fractions, log_size, [tree_cols[t][c] for t, c in fcols], _resolve(pkg, rules[: fractions.shape["n_params"]], lookup, None), out))
                inter += out
                inter_logs += [log_size] * len(out)
            sums, _ = ctx.logup_program_generate_batch(batch)
            for k, c in zip(frac, sums):
                claimed[k] = c
                ch.mix_felts([c])
            roots.append(s.commit(ch, inter, inter_logs, form=0))
        r = ch.draw_felt()
        session = [s.tree_columns(t) for t in range(len(roots))]
        first, at = {}, 0
        for k in frac:
            first[k] = at
            at += 4 * st.components[k][5].shape["n_logup_cols"]
        expanded, comps = {}, []
        for k, (program, log_size, log_expand, columns, rules, _, _) in enumerate(st.components):
            cols = []
            for t, c in columns:
                if t == S.INTERACTION:
                    t, c = it, first[k] + c
                if log_expand == blowup:
                    cols.append(session[t][1][c])
                    continue
                if (t, c, log_expand) not in expanded:
                    expanded[(t, c, log_expand)] = dev.empty(1 << (log_size + log_expand))
                    ctx.evaluate([session[t][0][c]], [expanded[(t, c, log_expand)]], log_size, log_size + log_expand)
                cols.append(expanded[(t, c, log_expand)])
            runner = kernels[k] if kernels and kernels[k] is not None else program
            comps.append((runner, log_size, log_expand, cols, _resolve(pkg, rules, lookup, claimed.get(k))))
        dst_log = max(c[1] + c[2] for c in comps)
        comp = [dev.empty(1 << dst_log) for _ in range(4)]
        ctx.air_compose(comps, r, comp, dst_log)
        roots.append(s.commit(ch, comp, [dst_log] * 4, form=1))
        oods = ch.draw_point()
        points, samples, refs = _describe(pkg, st, oods)
        proof, sampled = s.prove_values(ch, points, samples, with_sampled=True)
    nested, at = [], 0
    for t in samples:
        nested.append([])
        for c in t:
            nested[-1].append(sampled[at: at + len(c)])
            at += len(c)
    at_point = pkg.air_compose_at_point([(st.components[k][0], st.components[k][1], [nested[t][c][i] for t, c, i in refs[k]], comps[k][4]) for k in range(len(comps))], oods, r)
    return roots, [claimed[k] for k in frac], proof, pcs_replay.from_partial_evals([c[0] for c in nested[-1]]), at_point


def _split(raw):
    """air_prove's result -> (claimed sums as 4-word lists, the bytes of the proof member)"""
    head = b'{"claimed_sums":'
    assert raw.startswith(head) and raw.endswith(b"}")
    at = raw.index(b',"proof":')
    return [pcs_replay.flat_q(q) for q in json.loads(raw[len(head): at])], raw[at + len(b',"proof":'):-1]


def _both(pkg, ctx, st, tree_cols, conv=STWO, kernels=None, cfg=None):
    """The driver and the hand-made sequence on the same columns: equal bytes, equal sums, equal roots; the verifier accepts. Returns the bytes."""
    before = ctx.memory()["arena_in_use"]
    with pkg.Channel(conv) as ch:
        ch.mix_u64(77)      # the caller's channel may already carry mixes
        raw = ctx.air_prove(st, tree_cols, ch, kernels=kernels)
        after = ch.state()
    assert ctx.memory()["arena_in_use"] == before
    with pkg.Channel(conv) as ch:
        ch.mix_u64(77)
        roots, sums, proof, sampled_value, at_point = _hand_prove(pkg, ctx, st, tree_cols, ch, kernels)
        assert ch.state() == after
    got_sums, member = _split(raw)
    assert sampled_value == at_point and got_sums == sums
    assert len(member) == len(proof) and member == proof
    assert [pcs_replay.root_bytes(h) for h in json.loads(member)["commitments"]] == roots
    with pkg.Channel(conv) as ch:
        ch.mix_u64(77)
        assert pkg.air_verify(st, raw, ch, conv, cfg) == (True, "")
    with pkg.Channel(conv) as ch:      # a channel that does not carry the caller's mix: other draws
        ok, why = pkg.air_verify(st, raw, ch, conv, cfg)
        assert not ok and why
    return raw


# ---- 1. the lookup AIR of INTEGRATION.md section 2e ---------------------------------------------------------------------------------------
def _lookup_programs(pkg):
    f = pkg.AirBuilder()
    a, t, mult, z, alpha = f.col(0), f.col(1), f.col(2), f.param(0), f.param(1)
    f.frac(1, alpha * a - z); f.end_column()
    f.frac(-mult, alpha * t - z); f.end_column()
    b = pkg.AirBuilder()
    a, t, mult, is_first = b.col(0), b.col(1), b.col(2), b.col(3)
    z, alpha, total = b.param(0), b.param(1), b.param(2)
    cur0, cur1, prev1 = b.secure_col(4), b.secure_col(8), b.secure_col(8, -1)
    b.constraint(cur0 * (alpha * a - z) - b._to_q(b.const(1)))
    b.constraint((cur1 - (prev1 - total * is_first) - cur0) * (alpha * t - z) - b._to_q(-mult))
    return b.program(), f.logup_program()


def _lookup_trace(log_size, seed):
    """a, t, mult in storage order: t distinct, a drawn from t, mult[i] = how often t[i] occurs in a"""
    n = 1 << log_size
    t = splitmix_column(seed, n)
    assert len(set(t.tolist())) == n
    pick = splitmix_column((seed + 1) << 32, n) % np.uint32(n // 4)
    return np.stack([t[pick], t, np.bincount(pick, minlength=n).astype(np.uint32)])


def _is_first(log_size):
    c = np.zeros(1 << log_size, dtype=np.uint32)
    c[0] = 1
    return c


def _lookup_rules(pkg, relation=0):
    S = pkg.AirStatement
    return [S.z(relation), S.alpha_pow(relation, 1), S.claimed_sum()]


def _lookup_statement(pkg, log_size):
    """a, t, mult, IsFirst in one tree; one component"""
    S = pkg.AirStatement
    program, fractions = _lookup_programs(pkg)
    st = S(n_relations=1)
    t0 = st.tree([log_size] * 4)
    st.component(program, log_size, 1, [(t0, c) for c in range(4)] + [(S.INTERACTION, j) for j in range(8)], _lookup_rules(pkg), fractions=fractions,
                 fraction_columns=[(t0, 0), (t0, 1), (t0, 2)])
    return st


def test_lookup_air_equals_the_hand_made_sequence(cctx, pkg):
    """log_size 6 under the default config (the constraint domain is the session's LDE), at log_blowup_factor 2 (it is evaluated from
    coefficients), and with the component given as its compiled kernel: per config the same bytes, which are the hand-made sequence's."""
    ctx, log_size = cctx, 6
    st = _lookup_statement(pkg, log_size)
    trace = np.concatenate([_lookup_trace(log_size, 51), _is_first(log_size)[None]])
    kernel = ctx.air_compile(st.components[0][0])
    try:
        with Dev(ctx) as dev:
            cols = [[dev.up(c) for c in trace]]
            for cfg in (None, pkg.PcsConfig(**B2)):
                ctx.set_pcs_config(cfg)
                raw = _both(pkg, ctx, st, cols, cfg=cfg)
                assert _split(raw)[0] == [[0, 0, 0, 0]]
                assert _both(pkg, ctx, st, cols, kernels=[kernel], cfg=cfg) == raw
                with pkg.Channel(STWO) as ch:
                    ch.mix_u64(77)
                    assert ctx.air_prove(st, cols, ch, check=True) == raw
    finally:
        kernel.close()


# ---- 2. the Brainfuck AIR over the captured polynomials of a real proof -------------------------------------------------------------------
@pytest.fixture(scope="module")
def _hctx(hooks_pkg):
    c = hooks_pkg.Context(0, max_log_domain=MAX_LOG_DOMAIN)
    yield c
    c.close()


@pytest.mark.parametrize("name,cv,cfg,compiled", [("default", STWO, None, False), ("mask_order_1", (0, 0, 1, 0), None, False),
                                                      ("b2_q10_pow16", STWO, dict(pow_bits=16, log_blowup_factor=2, n_queries=10), False), ("odd_compiled", STWO, None, True)])
def test_brainfuck_statement_reproduces_the_proof_byte_for_byte(hooks_pkg, _hctx, name, cv, cfg, compiled):
    """The four trees of bfhip_prove_brainfuck's proof, captured as coefficients; tree 0 is given as it is (form 1), tree 1 evaluated onto
    the trace domain (form 0). air_prove under brainfuck_air_statement returns the proof's own proof member and its 13 claimed sums."""
    hp, ctx, conv = hooks_pkg, _hctx, cv
    cfg = None if cfg is None else hp.PcsConfig(**cfg)
    try:
        raw, full, logs, trees = _capture(hp, ctx, conv, cfg)
        log_sizes = [full["claim"][n]["log_size"] for n in pcs_replay.NAMES]
        st = hp.brainfuck_air_statement(log_sizes, LMR, conv[2])
        kernels = [ctx.air_compile(st.components[k][0]) if k % 2 else None for k in range(13)] if compiled else None
        with Dev(ctx) as dev:
            t0 = [dev.up(c) for c in trees[0]]
            t1 = []
            for col, log in zip(trees[1], logs[1]):
                t1.append(dev.empty(1 << log))
                ctx.evaluate([dev.up(col)], [t1[-1]], log, log)
            before = ctx.memory()["arena_in_use"]
            with hp.Channel(conv) as ch:
                got = ctx.air_prove(st, [t0, t1], ch, kernels=kernels)
            assert ctx.memory()["arena_in_use"] == before
        sums, member = _split(got)
        want = pcs_replay.proof_member(raw)
        assert len(member) == len(want) and member == want, name
        assert sums == [pcs_replay.flat_q(full["interaction_claim"][n]["claimed_sum"]) for n in pcs_replay.NAMES]
        with hp.Channel(conv) as ch:
            assert hp.air_verify(st, got, ch, conv, cfg) == (True, "")
        for k in kernels or []:
            if k is not None:
                k.close()
    finally:
        ctx.set_conventions(*STWO)
        ctx.set_pcs_config(None)


# ---- 3. shapes the driver can get wrong ---------------------------------------------------------------------------------------------------
A, B, OUT, NXT, PRV, NXT2, PRV2 = range(7)


def _storage_of_coset_order(col, log_size):
    """tests/test_gpu_air_program.py: coset order -> bit-reversed circle-domain order"""
    n = 1 << log_size
    d = air_model.bit_reverse(np.arange(n), log_size)
    return col[np.where(d < n // 2, 2 * d, 2 * (n - 1 - d) + 1)]


def _shift_program(pkg):
    """Degree 3 (out = a b b) and offsets -2 .. +2 read from the shifted copies' side, so that no column is opened at more than two points"""
    b = pkg.AirBuilder()
    a, bb = b.col(A), b.col(B)
    b.constraint(b.col(OUT) - a * bb * bb)
    b.constraint(b.col(NXT, -1) - a)
    b.constraint(b.col(PRV, 1) - a)
    b.constraint(b.col(NXT2, -2) - a)
    b.constraint(b.col(PRV2, 2) - a)
    return b.program()


def _shift_trace(log_size, seed):
    n = 1 << log_size
    a, b = splitmix_column(seed, n).astype(np.uint64), splitmix_column(seed + 1, n).astype(np.uint64)
    out = a * b % np.uint64(P) * b % np.uint64(P)
    coset = [a, b, out, np.roll(a, -1), np.roll(a, 1), np.roll(a, -2), np.roll(a, 2)]
    return np.stack([_storage_of_coset_order(c, log_size) for c in coset]).astype(np.uint32)


def _shapes(pkg, ctx, dev, L):
    """(statement, tree columns). Tree 0, as coefficients: IsFirst(L), IsFirst(L + 1) and a column nobody binds. Tree 1 behind two mixed
    words: lookup A (L) and the seven columns of the shift AIR (L). Tree 2 behind one: lookup B (L + 1), lookup C (L). Components: A (relation
    0), the shift AIR (degree 3 at log_expand 2, no fractions, between two that have them), B (relation 1, the larger size), C (relation 0,
    A's size, sharing IsFirst(L) with A: one sample for both)."""
    S = pkg.AirStatement
    program, fractions = _lookup_programs(pkg)
    st = S(n_relations=2)
    t0 = st.tree([L, L + 1, L], form=1)
    t1 = st.tree([L] * 10, mix_u64=[7, (1 << 40) + 3])
    t2 = st.tree([L + 1] * 3 + [L] * 3, mix_u64=[11])
    inter = [(S.INTERACTION, j) for j in range(8)]
    st.component(program, L, 1, [(t1, 0), (t1, 1), (t1, 2), (t0, 0)] + inter, _lookup_rules(pkg, 0), fractions=fractions, fraction_columns=[(t1, 0), (t1, 1), (t1, 2)])
    st.component(_shift_program(pkg), L, 2, [(t1, 3 + c) for c in range(7)], [])
    st.component(program, L + 1, 1, [(t2, 0), (t2, 1), (t2, 2), (t0, 1)] + inter, _lookup_rules(pkg, 1), fractions=fractions, fraction_columns=[(t2, 0), (t2, 1), (t2, 2)])
    st.component(program, L, 1, [(t2, 3), (t2, 4), (t2, 5), (t0, 0)] + inter, _lookup_rules(pkg, 0), fractions=fractions, fraction_columns=[(t2, 3), (t2, 4), (t2, 5)])
    pre = [dev.empty(1 << L), dev.empty(2 << L), dev.up(splitmix_column(901 + L, 1 << L))]
    ctx.is_first_coeffs(L, L + 1, pre[:2])
    main = [dev.up(c) for c in _lookup_trace(L, 61)] + [dev.up(c) for c in _shift_trace(L, 71)]
    more = [dev.up(c) for c in _lookup_trace(L + 1, 81)] + [dev.up(c) for c in _lookup_trace(L, 91)]
    return st, [pre, main, more]


@pytest.mark.parametrize("blowup", [1, 2])
@pytest.mark.parametrize("L", [4, 9])
def test_shapes_equal_the_hand_made_sequence(cctx, pkg, L, blowup):
    ctx = cctx
    cfg = pkg.PcsConfig(log_blowup_factor=blowup)
    ctx.set_pcs_config(cfg)
    with Dev(ctx) as dev:
        st, cols = _shapes(pkg, ctx, dev, L)
        pts, samples = st.samples(cfg)
        assert pts == [(0, 0), (L, -1), (L, 1), (L, -2), (L, 2), (L + 1, -1)]
        assert samples[0] == [[0], [0], []] and len(samples) == 5 and [len(t) for t in samples] == [3, 10, 6, 24, 4]
        raw = _both(pkg, ctx, st, cols, cfg=cfg)
        assert _split(raw)[0] == [[0, 0, 0, 0]] * 3 and len(json.loads(_split(raw)[1])["commitments"]) == 5


@pytest.mark.parametrize("L", [4, 9])
def test_no_relation_and_no_fraction_program_gives_three_roots(cctx, pkg, L):
    """n_relations = 0 and no fraction program anywhere: no draw, no interaction tree — two caller trees and the composition tree"""
    ctx = cctx
    st = pkg.AirStatement()
    t0, t1 = st.tree([L] * 3), st.tree([L] * 4, mix_u64=[5])
    st.component(_shift_program(pkg), L, 2, [(t0, c) for c in range(3)] + [(t1, c) for c in range(4)], [])
    with Dev(ctx) as dev:
        trace = _shift_trace(L, 33)
        raw = _both(pkg, ctx, st, [[dev.up(c) for c in trace[:3]], [dev.up(c) for c in trace[3:]]])
    sums, member = _split(raw)
    assert sums == [] and len(json.loads(member)["commitments"]) == 3


# ---- 4. failures, and what they leave behind ----------------------------------------------------------------------------------------------
def _mul_program(pkg):
    b = pkg.AirBuilder()
    b.constraint(b.col(2) - b.col(0) * b.col(1))
    return b.program()


def _failure_statement(pkg, log_size):
    """The lookup component and, behind it, out = a x over three more columns of the same tree"""
    S = pkg.AirStatement
    st = _lookup_statement(pkg, log_size)
    st.trees[0] = ([log_size] * 7, 0, [])
    st.component(_mul_program(pkg), log_size, 1, [(0, 4), (0, 5), (0, 6)], [])
    return st


def test_failures_are_named_and_leave_the_context_as_it_was(cctx, pkg):
    ctx, log_size, n = cctx, 6, 64
    st = _failure_statement(pkg, log_size)
    x, y = splitmix_column(5 << 32, n).astype(np.uint64), splitmix_column(6 << 32, n).astype(np.uint64)
    trace = np.concatenate([_lookup_trace(log_size, 51), _is_first(log_size)[None], np.stack([x, y, x * y % np.uint64(P)]).astype(np.uint32)])

    def prove(t, check=False):
        with Dev(ctx) as dev, pkg.Channel(STWO) as ch:
            return ctx.air_prove(st, [[dev.up(c) for c in t]], ch, check=check)

    def verify(raw):
        with pkg.Channel(STWO) as ch:
            return pkg.air_verify(st, raw, ch, STWO)

    good = prove(trace)
    assert verify(good) == (True, "") and prove(trace, check=True) == good
    in_use = ctx.memory()["arena_in_use"]

    def afterwards():
        assert ctx.memory()["arena_in_use"] == in_use
        with pkg.PcsSession(ctx):      # no session was left open
            pass
        assert prove(trace) == good

    # one trace cell changed: the sanity check of prover::prove; with check=True the component, the constraint and the cell
    bad = trace.copy()
    bad[6, 3] = (int(bad[6, 3]) + 1) % P
    with pytest.raises(pkg.BfhipError) as e:
        prove(bad)
    assert str(e.value) == "bfhip_air_prove: ConstraintsNotSatisfied"
    afterwards()
    with pytest.raises(pkg.BfhipError) as e:
        prove(bad, check=True)
    with Dev(ctx) as dev:
        report = ctx.air_check(_mul_program(pkg), log_size, [dev.up(c) for c in bad[4:7]], [])
    lines = pkg.format_air_check(report).splitlines()
    assert lines[1].startswith("constraint 0: 1 cells, first at cell 3, value (1, 0, 0, 0)")
    assert str(e.value) == "bfhip_air_prove: component 1: " + lines[1]
    afterwards()
    # one mult cell changed: every constraint still holds, the proof is produced, and the lookup does not balance
    bad = trace.copy()
    bad[2, 3] = (int(bad[2, 3]) + 1) % P
    raw = prove(bad)
    assert _split(raw)[0] != [[0, 0, 0, 0]] and verify(raw) == (False, "InvalidLookup: Invalid LogUp sum")
    afterwards()
    # a zero denominator: the batch's own message, prefixed. The denominator a - a[37] does not depend on the drawn elements.
    S = pkg.AirStatement
    v = int(trace[0, 37])
    f = pkg.AirBuilder()
    f.frac(1, f.col(0) - f.const(v)); f.end_column()
    b = pkg.AirBuilder()
    cur, prev = b.secure_col(2), b.secure_col(2, -1)
    b.constraint((cur - (prev - b.param(0) * b.col(1))) * b._to_q(b.col(0) - b.const(v)) - b._to_q(b.const(1)))
    zero = S()
    zero.tree([log_size] * 7)
    zero.component(b.program(), log_size, 1, [(0, 0), (0, 3)] + [(S.INTERACTION, j) for j in range(4)], [S.claimed_sum()], fractions=f.logup_program(), fraction_columns=[(0, 0)])
    cell = min(i for i in range(n) if int(trace[0, i]) == v)
    with Dev(ctx) as dev, pkg.Channel(STWO) as ch:
        with pytest.raises(pkg.BfhipError) as e:
            ctx.air_prove(zero, [[dev.up(c) for c in trace]], ch)
    assert str(e.value) == "bfhip_air_prove: bfhip_logup_program_generate_batch: component 0: fraction 0 has a zero denominator at cell %d" % cell
    afterwards()
    # a refusal of the validator, and of the driver's own checks: before the session opens
    with Dev(ctx) as dev, pkg.Channel(STWO) as ch:
        cols = [dev.up(c) for c in trace]
        state = ch.state()
        st.components[1] = st.components[1][:2] + (4,) + st.components[1][3:]
        st._built = None
        with pytest.raises(pkg.BfhipError) as e:
            ctx.air_prove(st, [cols], ch)
        assert str(e.value) == "bfhip_air_prove: component 1: log_expand must be 1, 2 or 3, got 4"
        st.components[1] = st.components[1][:2] + (1,) + st.components[1][3:]
        st._built = None
        with pytest.raises(pkg.BfhipError) as e:
            ctx.air_prove(st, [cols[:6] + [0]], ch)
        assert str(e.value) == "bfhip_air_prove: tree 0: null column pointer"
        assert ch.state() == state
    afterwards()


def test_open_session_and_shard_group_are_refused_by_name(cctx, pkg):
    ctx, log_size = cctx, 6
    st = _lookup_statement(pkg, log_size)
    trace = np.concatenate([_lookup_trace(log_size, 51), _is_first(log_size)[None]])
    with Dev(ctx) as dev, pkg.Channel(STWO) as ch:
        cols = [dev.up(c) for c in trace]
        with pkg.PcsSession(ctx):
            with pytest.raises(pkg.BfhipError) as e:
                ctx.air_prove(st, [cols], ch)
            assert str(e.value) == "bfhip_air_prove: a commitment-scheme session is open on this context (bfhip_pcs_destroy first)"
        good = ctx.air_prove(st, [cols], ch)
        assert _split(good)[0] == [[0, 0, 0, 0]]
    group, member = pkg.LocalGroup(2), pkg.Context(0, max_log_domain=10)
    try:
        member.join_local_group(group, 0)
        with Dev(member) as dev, pkg.Channel(STWO) as ch:
            with pytest.raises(pkg.BfhipError) as e:
                member.air_prove(st, [[dev.up(c) for c in trace]], ch)
            assert str(e.value) == "bfhip_air_prove: a context in a shard group is not supported (bfhip_ctx_leave_group first)"
        member.leave_group()
    finally:
        member.close(); group.close()
