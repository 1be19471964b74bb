"""-m gpu: op-level parity at SATURATED field values and at kernel shapes no other op-level test visits. Every comparison is bit-exact, against the
CPU oracle (pinned at these inputs by test_field_inputs_cpu.py) or against exact integers; the inputs are the families of tests/field_inputs.py
(all cells P - 1, the edge set, butterfly partners summing to exactly P or differing by 0, one-hot columns) crossed with constants of the same
families plus the three that drive m31.h q_mul_const to its bound. What this pins: the fold schedules of the lazily reduced accumulators
(quotient.hip stage 1: 4 (p-1)^2 + 2^34 < 2^64; mac3; air.hip DomainEval / GroupEval: 4 products between folds; air.h combine_base: every third
term), the m_add / m_sub edges at s == P, m_mul_pre2's multiplicand bound, and the shapes: every evaluate extension the PCS config promises,
the six-column double buffer of k_quotients in all residue classes, the paired and unpaired row-group constraint kernels, the two-pass plans.

Mutation runs (arithmetic-only changes on a scratch copy, one at a time): see MUTATIONS below."""
import ctypes

import numpy as np
import pytest

import field_inputs as fi
from conftest import P

pytestmark = [pytest.mark.gpu, pytest.mark.single_conv]

# Arithmetic-only mutations, each built on a scratch copy and run on an MI355X against this module ("new") and the older module of that op
# ("old": test_gpu_components.py / test_gpu_ops.py / test_gpu_fft.py):
MUTATIONS = """
1 air.hip DomainEval::constraint  pending == 4 -> 5   new: caught, test_eval_constraints_kernel_variants per_row_* x (uniform, max), (edge, max)   old: missed
  (twin) air.hip GroupEval::dot   pending == 4 -> 5   new: caught, row_group / paired_and_unpaired x (uniform, max), (edge, max), (uniform, heavy)     old: missed
2 quotient.hip stage 1            idx % 4 -> idx % 5  new: caught, test_eval_at_point at 10 of 11 shapes                                             old: caught at one shape (log 17)
3 quotient.hip k_quotients full-column mac3 without its m_fold   new: caught, both accumulate_quotients tests, every family pair                      old: missed
4 m31.h m_add returning P at a + b == P               new: caught, test_interpolate_then_evaluate, test_replicated_.., test_fold_line, test_accumulate   old: missed (201 passed)
5 air.h combine_base              i % 3 -> i % 5      missed by both, and by construction: the mutant computes the same values. alpha^0 = 1, so the
  first five terms are v0 + four products <= (p - 1) + 4 (p - 1)^2 < 2^64 on an EMPTY accumulator, and two products follow the fold at i = 5.
  The nearest schedule that can overflow, i % 6 (v0 + five products), is caught: test_eval_constraints_kernel_variants x (max, heavy) in every
  variant, reported at the processor component (the first of the ten combine7 users — processor, jnz, jz, the six instruction components,
  end_of_execution — that the loop reaches) — field_inputs.HEAVY_ROOT exists for this; old: missed.
"""

N_MAIN = [8, 8, 4, 9, 13, 13, 11, 11, 11, 11, 11, 11, 7]
N_CONS = [12, 11, 5, 10, 9, 9, 7, 7, 8, 8, 8, 7, 2]
NAMES = ["memory", "instruction", "program", "processor", "jnz", "jz", "input", "left", "minus", "output", "plus", "right", "end_of_execution"]
FAMS = list(fi.FAMILIES)
# (column family, constant family): the crossing of field_inputs.CROSS, then every other column family against max and edge constants
PAIRS = fi.CROSS + [(f, c) for f in FAMS if f not in fi.BIG_FAMILIES for c in ("max", "edge")]
BIG = 20        # from 2^20 cells up only the crossings of uniform / max / edge columns (bounds the oracle's CPU time)


def _pairs(log):
    return fi.CROSS if log >= BIG else PAIRS


def _ids(p):
    return f"{p[0]}-{p[1]}" if isinstance(p, tuple) else None


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _ptrs(arrs):
    return (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


def _u32s(v):
    return (ctypes.c_uint32 * len(v))(*[int(x) for x in v])


def _first_diff(got, want):
    d = np.nonzero(np.asarray(got) != np.asarray(want))
    return None if d[0].size == 0 else tuple(int(x[0]) for x in d)


def _assert_equal(got, want, what):
    assert np.array_equal(got, want), (what, "first differing index", _first_diff(got, want))


# ---- transforms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [3, 5, 6, 11, 12, 13, 19, 20, 22])
def test_interpolate_then_evaluate(ctx, oracle, log):
    """tiny / generic / tile12 / strided7 / two-pass plans. complement / equal partners at strides 1, 2 and n / 2 are the butterfly partners of the
    first two layers and of the last one."""
    n = 1 << log
    for fam in (fi.BIG_FAMILIES if log >= BIG else FAMS):
        cols = np.stack(fi.columns(fam, log, 2, n))
        ptrs = [ctx.upload(c) for c in cols]
        ctx.interpolate(ptrs, ptrs, log)
        got = np.stack([ctx.download(p, n) for p in ptrs])
        want = oracle.interpolate(cols, log)
        _assert_equal(got, want, ("interpolate", fam, log))
        lde = [ctx.malloc(8 * n) for _ in ptrs]
        ctx.evaluate(ptrs, lde, log, log + 1)
        got2 = np.stack([ctx.download(p, 2 * n) for p in lde])
        _assert_equal(got2, oracle.evaluate(want, log, log + 1), ("evaluate", fam, log))
        if fam == "max":      # closed form, independent of the oracle: a constant column has one non-zero coefficient
            assert (got[:, 0] == P - 1).all() and not got[:, 1:].any() and (got2 == P - 1).all()
        for p in ptrs + lde:
            ctx.free(p)


@pytest.mark.parametrize("log", [4, 5, 10, 16, 20])
def test_replicated_interpolate_then_evaluate(ctx, oracle, log):
    m = 1 << (log - 4)
    for fam in (fi.BIG_FAMILIES if log >= BIG else FAMS):
        rows = fi.column(fam, 0xAB0 + log, m)
        want = oracle.interpolate(np.repeat(rows, 16)[None, :], log)
        p = ctx.upload(rows)
        ctx.interpolate([p], [p], log, replicated=True)
        _assert_equal(ctx.download(p, m), want[0][::16], ("interpolate", fam, log))
        assert not want[0].reshape(-1, 16)[:, 1:].any()
        q = ctx.malloc(8 * m)
        ctx.evaluate([p], [q], log, log + 1, replicated=True)
        _assert_equal(np.repeat(ctx.download(q, 2 * m), 16), oracle.evaluate(want, log, log + 1)[0], ("evaluate", fam, log))
        ctx.free(p); ctx.free(q)


# ---- evaluate: every extension, and the ones the PCS config promises (log_blowup_factor up to 16) ---------------------------------------------
EXTENSIONS = [(3, 3), (4, 8), (4, 12), (4, 20), (5, 13), (6, 22), (8, 24), (11, 12), (11, 15), (12, 20), (13, 21), (16, 24), (20, 24)]
REPLICATED_EXTENSIONS = [(4, 5), (4, 9), (4, 10), (5, 10), (5, 11), (6, 12), (8, 24), (20, 24)]


@pytest.mark.parametrize("fam", ["uniform", "edge"])
@pytest.mark.parametrize("log_size,log_eval", EXTENSIONS)
def test_evaluate_extension(ctx, oracle, log_size, log_eval, fam):
    coeffs = fi.column(fam, 31 * log_size + log_eval, 1 << log_size)
    p, q = ctx.upload(coeffs), ctx.malloc(4 << log_eval)
    ctx.evaluate([p], [q], log_size, log_eval)
    got = ctx.download(q, 1 << log_eval)
    ctx.free(p); ctx.free(q)
    _assert_equal(got, oracle.evaluate(coeffs[None, :], log_size, log_eval)[0], (log_size, log_eval))


@pytest.mark.parametrize("fam", ["uniform", "edge"])
@pytest.mark.parametrize("log_size,log_eval", REPLICATED_EXTENSIONS)
def test_evaluate_extension_replicated(ctx, oracle, log_size, log_eval, fam):
    """(4, 10) is the one-call form of a proof under log_blowup_factor 6: the row-granular columns of a 2^4-row component are ONE coefficient
    extended to 64 cells (a 2^5-row component: two) — fft_plan used to refuse it."""
    m = 1 << (log_size - 4)
    coeffs = fi.column(fam, 37 * log_size + log_eval, m)
    full = np.zeros(1 << log_size, dtype=np.uint32); full[::16] = coeffs
    p, q = ctx.upload(coeffs), ctx.malloc(4 << (log_eval - 4))
    ctx.evaluate([p], [q], log_size, log_eval, replicated=True)
    got = ctx.download(q, 1 << (log_eval - 4))
    ctx.free(p); ctx.free(q)
    _assert_equal(np.repeat(got, 16), oracle.evaluate(full[None, :], log_size, log_eval)[0], (log_size, log_eval))


def test_evaluate_rejects_what_it_cannot_do_and_extends_two_coefficients(ctx, pkg, oracle):
    p, q = ctx.upload(fi.edge(1, 64)), ctx.malloc(4 << 6)
    with pytest.raises(pkg.BfhipError, match="log_eval < log_size"):
        ctx.evaluate([p], [q], 6, 5)
    with pytest.raises(pkg.BfhipError, match="twiddle tree"):
        ctx.evaluate([p], [q], 6, ctx.max_log_domain + 1)
    with pytest.raises(pkg.BfhipError, match="log_size >= 4"):
        ctx.evaluate([p], [q], 3, 6, replicated=True)
    # a polynomial of 2 coefficients (and of 1) on 64 cells: supported since the planner zero-pads to the 4 cells a lane loads
    for log_size in (1, 0):
        coeffs = fi.edge(5, 64)[: 1 << log_size].copy(); coeffs[0] = P - 1
        c = ctx.upload(coeffs)
        ctx.evaluate([c], [q], log_size, 6)
        _assert_equal(ctx.download(q, 64), oracle.evaluate(coeffs[None, :], log_size, 6)[0], ("evaluate", log_size, 6))
        ctx.free(c)
    ctx.free(p); ctx.free(q)


# ---- FRI folds and point evaluation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [1, 2, 5, 11, 16, 20, 22])
def test_fold_line(ctx, oracle, log):
    n = 1 << log
    for cols_f, const_f in _pairs(log):
        src = fi.columns(cols_f, 300 + log, 4, n)
        alpha = fi.const(const_f, 3, 4)
        want = [np.zeros(n // 2, dtype=np.uint32) for _ in range(4)]
        assert oracle.L.orc_fold_line(_ptrs(src), log, _u32s(alpha), _ptrs(want)) == 0
        ds = [ctx.upload(s) for s in src]; dd = [ctx.malloc(2 * n) for _ in range(4)]
        ctx.fold_line(ds, dd, log, alpha)
        got = [ctx.download(d, n // 2) for d in dd]
        for p in ds + dd:
            ctx.free(p)
        _assert_equal(np.stack(got), np.stack(want), (cols_f, const_f, log))


@pytest.mark.parametrize("log", [3, 6, 12, 17, 20, 22])
def test_fold_circle_into_line(ctx, oracle, log):
    n = 1 << log
    for cols_f, const_f in _pairs(log):
        src = fi.columns(cols_f, 400 + log, 4, n)
        dst = fi.columns(cols_f, 500 + log, 4, n // 2)          # the destination's old contents take the family too
        alpha = fi.const(const_f, 4, 4)
        want = [d.copy() for d in dst]
        assert oracle.L.orc_fold_circle_into_line(_ptrs(want), _ptrs(src), log, _u32s(alpha)) == 0
        ds = [ctx.upload(s) for s in src]; dd = [ctx.upload(d) for d in dst]
        ctx.fold_circle_into_line(dd, ds, log, alpha)
        got = [ctx.download(d, n // 2) for d in dd]
        for p in ds + dd:
            ctx.free(p)
        _assert_equal(np.stack(got), np.stack(want), (cols_f, const_f, log))


@pytest.mark.parametrize("log,replicated", [(4, False), (9, False), (13, False), (17, False), (21, False), (22, False), (24, False),
                                            (5, True), (12, True), (18, True), (24, True)])
def test_eval_at_point(ctx, oracle, log, replicated):
    """The weights are derived from the point (stage 1: four products on a folded accumulator, a fold every 4th term; above 2^20 coefficients
    stage 2 folds sequentially)."""
    n = 1 << (log - 4 if replicated else log)
    for cols_f, const_f in _pairs(log):
        coeffs = fi.column(cols_f, 100 + log, n)
        full = coeffs
        if replicated:
            full = np.zeros(1 << log, dtype=np.uint32); full[::16] = coeffs
        point = fi.const(const_f, 7, 8)
        out = (ctypes.c_uint32 * 4)()
        oracle.L.orc_eval_at_point(_vp(full), log, _u32s(point), out)
        p = ctx.upload(coeffs)
        got = ctx.eval_at_point(p, log, point, replicated)
        ctx.free(p)
        assert got == list(out), (cols_f, const_f, log, replicated)


# ---- batch inverses, accumulate -----------------------------------------------------------------------------------------------------------
BATCH_INVERSE_SIZES = [1, 3, 4, 7, 8, 1000, 1001, 1 << 16]


def batch_inverse_operands(fam, n):
    """(M31 column, four QM31 coordinate columns) without a zero operand: a zero cell becomes 1 (M31) / a zero first coordinate becomes 1."""
    m = fi.column(fam, 9, n).copy(); m[m == 0] = 1
    q = [c.copy() for c in fi.columns(fam, 20, 4, n)]
    q[0][q[0] == 0] = 1
    return m, q


@pytest.mark.parametrize("n", BATCH_INVERSE_SIZES)
def test_batch_inverses(ctx, oracle, n):
    for fam in FAMS:
        m, q = batch_inverse_operands(fam, n)
        p, r = ctx.upload(m), ctx.malloc(4 * n)
        ctx.batch_inverse_m31(p, r, n)
        got = ctx.download(r, n)
        ctx.free(p); ctx.free(r)
        assert int(got.max()) < P and np.all((got.astype(np.uint64) * m.astype(np.uint64)) % np.uint64(P) == 1), (fam, n)   # exact: < 2^62
        flat = np.ascontiguousarray(np.stack(q, axis=1).reshape(-1))
        want = np.zeros_like(flat)
        assert oracle.L.orc_qm31_op(3, _vp(flat), None, _vp(want), ctypes.c_size_t(n)) == 0
        src = [ctx.upload(c) for c in q]
        ctx.batch_inverse_qm31(src, src, n)
        gotq = np.stack([ctx.download(s, n) for s in src], axis=1).reshape(-1)
        for s in src:
            ctx.free(s)
        _assert_equal(gotq, want, (fam, n))


@pytest.mark.parametrize("n", [1, 5000, (1 << 16) + 1])
def test_accumulate(ctx, n):
    for fa in FAMS:
        a = fi.column(fa, 1, n)
        others = [fi.column(fb, 2, n) for fb in FAMS] + [((P - a.astype(np.int64)) % P).astype(np.uint32)]      # the last: every sum is exactly P
        for b in others:
            pa, pb = ctx.upload(a), ctx.upload(b)
            ctx.accumulate(pa, pb, n)
            got = ctx.download(pa, n)
            ctx.free(pa); ctx.free(pb)
            _assert_equal(got, ((a.astype(np.uint64) + b) % np.uint64(P)).astype(np.uint32), (fa, n))


# ---- logUp generation on arbitrary rows ---------------------------------------------------------------------------------------------------
LOGUP_ROWS = [1, 4, 1024]


def lookup_elements(const_f, seed):
    """24 words = (z, alpha) of the three lookup relations; a zero first coordinate becomes 1 so that no element is zero. The last coordinate
    of every z is lowered by one: with z == alpha (the max family) the denominator v0 + v1 alpha + v2 alpha^2 - z vanishes at the edge
    values (0, 1, 0) — such rows would be zero denominators, which logUp does not allow (test_field_inputs_cpu.py asserts there is none)."""
    e = fi.const(const_f, seed, 24).astype(np.int64)
    e[::4][e[::4] == 0] = 1
    e[3::8] = (e[3::8] + P - 1) % P
    return e.tolist()


def logup_inputs(comp, cols_f, const_f, rows):
    return np.stack(fi.columns(cols_f, 40 + comp, N_MAIN[comp], rows)), lookup_elements(const_f, 31)


LOGUP_PAIRS = PAIRS + fi.LOOKUP_CROSS          # every column family of section 1 reaches the logUp kernels


@pytest.mark.parametrize("pair", LOGUP_PAIRS, ids=_ids)
@pytest.mark.parametrize("rows", LOGUP_ROWS)
def test_logup_generate(ctx, oracle, rows, pair):
    from test_gpu_components import _logup_gpu
    for comp in range(13):
        r, elems = logup_inputs(comp, pair[0], pair[1], rows)
        want, want_claimed = oracle.logup_generate(comp, r, elems)
        got, claimed = _logup_gpu(ctx, comp, r, elems)
        assert claimed == want_claimed, (NAMES[comp], pair)
        n_rep = len(got) - 4
        for k in range(n_rep):
            _assert_equal(np.repeat(got[k], 16), want[k], (NAMES[comp], k))
        for k in range(4):
            _assert_equal(got[n_rep + k], want[n_rep + k], (NAMES[comp], k))


# ---- accumulate_quotients: the column-layout matrix ----------------------------------------------------------------------------------------
QUOTIENT_LOGS = [3, 10, 18]
LAYOUTS = sorted({l for nf in range(14) for l in ((nf, 0), (0, nf), (nf, nf), (nf, 13 - nf))} - {(0, 0)})


def quotient_points(const_f):
    """Three distinct sample points of one constant family (a saturated family stays saturated: one coordinate moves to P - 2)."""
    p0 = fi.const(const_f, 7, 8).tolist()
    p1, p2 = list(p0), list(p0)
    p1[0] = P - 2 if p0[0] != P - 2 else P - 3
    p2[4] = P - 2 if p0[4] != P - 2 else P - 3
    return [p0, p1, p2]


def _quotient_case(ctx, oracle, log, nf, nr, n_points, shift, cols_f, const_f):
    """nf full-size and nr replicated (2^shift-fold) columns sampled at point 0, interleaved; with 2 points the last column is sampled at
    point 1 as well (a "last logUp column"); with 3 one more full-size column is sampled at point 2 only."""
    n = 1 << log
    shifts, f, r = [], nf, nr
    while f or r:
        if f:
            shifts.append(0); f -= 1
        if r:
            shifts.append(shift); r -= 1
    which = [[0] for _ in shifts]
    if n_points >= 2:
        which[-1] = [0, 1]
    if n_points >= 3:
        shifts.append(0); which.append([2])
    pts = quotient_points(const_f)
    stored = [fi.column(cols_f, 40 + k, max(1, n >> s)) for k, s in enumerate(shifts)]
    cols = np.stack([np.repeat(c, 1 << s)[:n] for c, s in zip(stored, shifts)])
    n_samples, points, values, seed = [], [], [], 1000
    for w in which:
        n_samples.append(len(w))
        for k in w:
            points += pts[k]
            values += fi.const(const_f, seed, 4).tolist(); seed += 1
    coeff = fi.const(const_f, 3, 4).tolist()
    want = oracle.accumulate_quotients(log, cols, n_samples, points, values, coeff)
    p_cols = [ctx.upload(c) for c in stored]
    p_out = [ctx.malloc(4 * n) for _ in range(4)]
    ctx.accumulate_quotients(log, p_cols, n_samples, points, values, coeff, p_out, col_shifts=shifts)
    got = np.stack([ctx.download(p, n) for p in p_out])
    for p in p_cols + p_out:
        ctx.free(p)
    _assert_equal(got, want, (log, nf, nr, n_points, shift, cols_f, const_f))


@pytest.mark.parametrize("pair", [("uniform", "uniform"), ("max", "max")], ids=_ids)
def test_accumulate_quotients_layout_matrix(ctx, oracle, pair):
    """Every (full, replicated) column count of the diagonal-plus-edges set: all 6 x 6 residue classes of the six-column double buffer on
    both sides, the empty side included; 1..3 sample points and shifts 2..5 walk along the layouts so that each meets every residue."""
    for k, (nf, nr) in enumerate(LAYOUTS):
        for n_points in (1, 2, 3):
            _quotient_case(ctx, oracle, 10, nf, nr, n_points, 2 + (k + n_points) % 4, *pair)


@pytest.mark.parametrize("pair", fi.CROSS, ids=_ids)
def test_accumulate_quotients_crossed_families(ctx, oracle, pair):
    """Quotient coefficients are derived from the random coefficient and the sample points: crossed column / constant families, a few layouts
    with every point count and every shift, and the smallest and a large domain."""
    for nf, nr in ((7, 6), (6, 6), (13, 0), (0, 13), (1, 1)):
        for n_points in (1, 2, 3):
            for shift in (2, 3, 4, 5):
                _quotient_case(ctx, oracle, 10, nf, nr, n_points, shift, *pair)
    _quotient_case(ctx, oracle, 3, 4, 3, 3, 2, *pair)
    _quotient_case(ctx, oracle, 18, 4, 3, 3, 4, *pair)


# ---- eval_constraints: every kernel variant on synthetic columns ---------------------------------------------------------------------------
CONSTRAINT_FAMILIES = [("uniform", "uniform"), ("max", "max"), ("edge", "edge"), ("uniform", "max"), ("max", "uniform"), ("edge", "max")] + fi.LOOKUP_CROSS


def constraint_inputs(comp, log_size, cols_f, const_f, replicated=False):
    """Arbitrary columns (they need not satisfy the AIR) on the LDE domain of 2^(log_size + 1) cells. replicated: main columns and the non-last
    logUp columns are row-granular (`stored` holds n / 16 cells; the oracle's full-size input is their 16-fold repeat)."""
    n = 2 << log_size
    n_logup = 3 if comp == 3 else 1
    inter_rep = [replicated and k < 4 * (n_logup - 1) for k in range(4 * n_logup)]
    main_st = fi.columns(cols_f, 600 + comp, N_MAIN[comp], n >> 4 if replicated else n)
    inter_st = [fi.column(cols_f, 700 + 8 * k + comp, n >> 4 if r else n) for k, r in enumerate(inter_rep)]
    full = lambda c, r: np.repeat(c, 16) if r else c
    return {
        "main_stored": main_st, "inter_stored": inter_st, "inter_rep": inter_rep,
        "main": np.stack([full(c, replicated) for c in main_st]), "inter": np.stack([full(c, r) for c, r in zip(inter_st, inter_rep)]),
        "is_first": fi.column(cols_f, 55, n), "elems": lookup_elements(const_f, 77), "claimed": fi.const(const_f, 5, 4).tolist(),
        "coeffs": fi.const(const_f, 500 + comp, 4 * N_CONS[comp]).tolist(),
        "acc": np.stack(fi.columns(cols_f, 900, 4, n)),          # non-zero start: the operation accumulates
    }


def _constraints_gpu(ctx, comp, log_size, a, replicated):
    n = 2 << log_size
    p_first = ctx.upload(a["is_first"])
    p_main = [ctx.upload(c) for c in a["main_stored"]]
    p_inter = [ctx.upload(c) for c in a["inter_stored"]]
    p_acc = [ctx.upload(a["acc"][k]) for k in range(4)]
    ctx.eval_constraints(comp, log_size, p_first, p_main, p_inter, a["elems"], a["claimed"], a["coeffs"], p_acc,
                         main_shifts=[4 if replicated else 0] * N_MAIN[comp], inter_shifts=[4 if r else 0 for r in a["inter_rep"]])
    got = np.stack([ctx.download(p, n) for p in p_acc])
    for p in [p_first] + p_main + p_inter + p_acc:
        ctx.free(p)
    return got


# (id, log_size, replicated storage, {BFHIP_CONSTRAINT_GROUP_MIN_LOG value (None = unset): the kernel that must run — 0 per row, 16 row group, 32 paired})
CONSTRAINT_VARIANTS = [
    ("per_row_full_size", 6, False, {None: 0}),
    ("per_row_replicated", 6, True, {None: 0}),
    ("row_group_256_rows", 7, True, {"5": 16}),
    ("paired_and_unpaired_8192_rows", 12, True, {"5": 32, "11": 16}),       # 8192 >= 8 << 5: paired (32 rows per group); < 8 << 11: unpaired (16)
    ("paired_and_unpaired_16384_rows", 13, True, {"5": 32, "12": 16}),
]


@pytest.mark.parametrize("pair", CONSTRAINT_FAMILIES, ids=_ids)
@pytest.mark.parametrize("variant", CONSTRAINT_VARIANTS, ids=lambda v: v[0])
def test_eval_constraints_kernel_variants(ctx, oracle, hooks_pkg, monkeypatch, variant, pair):
    """With max columns every row sees the same few values, so the accumulators are loaded by derived values against P - 1 given ones: a window
    of 4 products then exceeds 3 * 2^62 in about one window of 24 — in every run. Which kernel runs is asserted, not assumed."""
    _, log_size, replicated, min_logs = variant
    for comp in range(13):
        a = constraint_inputs(comp, log_size, pair[0], pair[1], replicated)
        want = oracle.eval_constraints(comp, log_size, a["is_first"], a["main"], a["inter"], a["elems"], a["claimed"], a["coeffs"], a["acc"])
        for min_log, kernel in min_logs.items():
            if min_log is None:
                monkeypatch.delenv("BFHIP_CONSTRAINT_GROUP_MIN_LOG", raising=False)
            else:
                monkeypatch.setenv("BFHIP_CONSTRAINT_GROUP_MIN_LOG", min_log)
            # the library's own choice for this layout (the test-hooks build runs the same constraint_group_rows and reads the same variable)
            assert hooks_pkg.lib().bfhip_test_constraint_group_rows(comp, log_size, 4 if replicated else 0) == kernel, (NAMES[comp], variant[0], min_log)
            _assert_equal(_constraints_gpu(ctx, comp, log_size, a, replicated), want, (NAMES[comp], pair, variant[0], min_log))


# ---- the device half of m31.h (test-hooks build only) ---------------------------------------------------------------------------------------
OPS = {"m_add": 0, "m_sub": 1, "m_mul": 2, "m_mul_pre2": 3, "m_mul_pow2": 4, "m_inv": 5, "m_red4": 6, "m_canon": 7, "q_mul": 8, "q_mul_const": 9, "q_inv": 10}
Pu = np.uint64(P)


def _mulmod(a, b):
    return (a.astype(np.uint64) * b.astype(np.uint64)) % Pu          # exact: operands < 2^31


def _qmul_exact(x, y):
    """(n, 4) x (n, 4) -> (n, 4) by the definition i^2 = -1, u^2 = 2 + i; every product reduced, every sum below 2^35: exact in 64 bits."""
    a0, a1, a2, a3 = (x[:, k] for k in range(4)); b0, b1, b2, b3 = (y[:, k] for k in range(4))
    cm = lambda p, q, r, s: ((_mulmod(p, r) + Pu - _mulmod(q, s)) % Pu, (_mulmod(p, s) + _mulmod(q, r)) % Pu)
    aa, bb, ab, ba = cm(a0, a1, b0, b1), cm(a2, a3, b2, b3), cm(a0, a1, b2, b3), cm(a2, a3, b0, b1)
    rb = ((2 * bb[0] + Pu - bb[1]) % Pu, (bb[0] + 2 * bb[1]) % Pu)
    return np.stack([(aa[0] + rb[0]) % Pu, (aa[1] + rb[1]) % Pu, (ab[0] + ba[0]) % Pu, (ab[1] + ba[1]) % Pu], axis=1).astype(np.uint32)


def _powmod(a, e):
    r = np.ones_like(a, dtype=np.uint64); b = a.astype(np.uint64)
    while e:
        if e & 1:
            r = (r * b) % Pu
        b = (b * b) % Pu
        e >>= 1
    return r.astype(np.uint32)


@pytest.fixture(scope="module")
def hooks_ctx(hooks_pkg):
    c = hooks_pkg.Context(0, max_log_domain=10)
    yield c
    c.close()


def _field_op(hooks_pkg, c, op, a, b):
    """a, b: (n, 4) uint32. Returns (n, 4)."""
    n = a.shape[0]
    pa, pb, po = c.upload(a.reshape(-1)), c.upload(b.reshape(-1)), c.malloc(16 * n)
    L = hooks_pkg.lib()
    rc = L.bfhip_test_field_op(c._h, ctypes.c_uint32(OPS[op]), ctypes.c_void_p(pa), ctypes.c_void_p(pb), ctypes.c_void_p(po), ctypes.c_size_t(n))
    assert rc == 0, op
    out = c.download(po, 4 * n).reshape(n, 4)
    for p in (pa, pb, po):
        c.free(p)
    return out


def _scalar_operands():
    """Word 0 of a and b: the edge cross product, then 2^20 uniform pairs."""
    import itertools
    pairs = np.array(list(itertools.product(fi.EDGE_SET, fi.EDGE_SET)), dtype=np.uint32)
    n = 1 << 20
    a = np.zeros((pairs.shape[0] + n, 4), dtype=np.uint32); b = np.zeros_like(a)
    a[:, 0] = np.concatenate([pairs[:, 0], fi.uniform(11, n)]); b[:, 0] = np.concatenate([pairs[:, 1], fi.uniform(12, n)])
    return a, b


def test_device_m31_primitives_match_exact_integers(hooks_pkg, hooks_ctx):
    a, b = _scalar_operands()
    a0, b0 = a[:, 0].astype(np.uint64), b[:, 0].astype(np.uint64)
    run = lambda op, x=a, y=b: _field_op(hooks_pkg, hooks_ctx, op, x, y)
    pow2 = (np.uint64(1) << (b0 % np.uint64(31))) % Pu                # m_mul_pow2(a, b % 31) = a * 2^(b % 31)
    for op, want in (("m_add", (a0 + b0) % Pu), ("m_sub", (a0 + Pu - b0) % Pu), ("m_mul", (a0 * b0) % Pu), ("m_mul_pre2", (a0 * b0) % Pu),
                     ("m_mul_pow2", (a0 * pow2) % Pu)):
        got = run(op)
        _assert_equal(got[:, 0], want.astype(np.uint32), op)
        assert not got[:, 1:].any()
    k = a.shape[0] - (1 << 20)                                         # the edge part once more against Python integers
    assert run("m_add")[:k, 0].tolist() == [(int(x) + int(y)) % P for x, y in zip(a[:k, 0], b[:k, 0])]
    assert run("m_mul_pre2")[:k, 0].tolist() == [(int(x) * int(y)) % P for x, y in zip(a[:k, 0], b[:k, 0])]
    nz = a.copy(); nz[nz[:, 0] == 0, 0] = 1
    inv = run("m_inv", nz)
    _assert_equal(inv[:, 0], _powmod(nz[:, 0], P - 2), "m_inv")
    assert np.all(_mulmod(inv[:, 0], nz[:, 0]) == 1)
    # 64-bit operands: every pair of words of the wide edge set (word 0 + 2^32 word 1), then the uniform pairs with full 32-bit words
    import itertools
    wide = [0, 1, 2, P - 1, P, P + 1, 1 << 31, (1 << 31) + 1, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFF, 0x10000, (1 << 30), 3 * (1 << 30)]
    w = np.array(list(itertools.product(wide, wide)), dtype=np.uint32)
    x = np.zeros((w.shape[0] + (1 << 20), 4), dtype=np.uint32)
    mix = fi._splitmix_u64(77, 1 << 20)
    x[:, 0] = np.concatenate([w[:, 0], (mix & np.uint64(0xFFFFFFFF)).astype(np.uint32)])
    x[:, 1] = np.concatenate([w[:, 1], (mix >> np.uint64(32)).astype(np.uint32)])
    want64 = (((x[:, 1].astype(np.uint64) << np.uint64(32)) | x[:, 0].astype(np.uint64)) % Pu).astype(np.uint32)
    assert want64[: w.shape[0]].tolist() == [(int(lo) + (int(hi) << 32)) % P for lo, hi in w]       # the numpy form against Python integers
    for op in ("m_red4", "m_canon"):
        _assert_equal(run(op, x, x)[:, 0], want64, op)


def test_device_qm31_primitives_match_exact_integers(hooks_pkg, hooks_ctx):
    """q_mul_const at its bound: the kept entries nc1 / nc3 / ne1 are P itself for three of the constants, against x with the edge set in every
    coordinate (four products of values <= P in one u64)."""
    import itertools
    xs = np.array(list(itertools.product(fi.EDGE_SET, repeat=4)), dtype=np.uint32)
    ys = [(P - 1,) * 4, (P - 1, 0, P - 1, 0), (P - 1, P - 1, P - 2, 1), (0, 0, 0, 0), (1, 0, 0, 0), (0, 0, 1, 0), (0, P - 1, 0, P - 1)]
    ys += [tuple(fi.edge(s, 4).tolist()) for s in range(4)] + [tuple(fi.uniform(s, 4).tolist()) for s in range(2)]
    n = 1 << 20
    ux = np.stack([fi.uniform(50 + k, n) for k in range(4)], axis=1); uy = np.stack([fi.uniform(60 + k, n) for k in range(4)], axis=1)
    x = np.concatenate([np.tile(xs, (len(ys), 1)), ux]); y = np.concatenate([np.repeat(np.array(ys, dtype=np.uint32), xs.shape[0], axis=0), uy])
    want = _qmul_exact(x, y)
    for k in range(0, xs.shape[0] * len(ys), 4099):          # the 64-bit form against Python integers
        assert want[k].tolist() == fi.qm31_mul_int(x[k], y[k])
    for op in ("q_mul", "q_mul_const"):
        _assert_equal(_field_op(hooks_pkg, hooks_ctx, op, x, y), want, op)
    nz = x[np.any(x != 0, axis=1)]
    inv = _field_op(hooks_pkg, hooks_ctx, "q_inv", nz, nz)
    assert int(inv.max()) < P
    one = np.zeros_like(nz); one[:, 0] = 1
    _assert_equal(_qmul_exact(nz, inv), one, "q_inv")          # the inverse is unique
