"""CPU: the oracle becomes the expected value of test_gpu_field_edges.py at saturated inputs it was never pinned at (its m31_reduce is
"valid for x in [0, P^2)"). Before it is trusted there: its field operations, FRI folds, point evaluation and transforms on every input
family of tests/field_inputs.py against exact Python integers / algebraic identities, and the preconditions of the GPU matrix (no zero
denominator anywhere) asserted once."""
import ctypes
import itertools

import numpy as np
import pytest

import field_inputs as fi
from conftest import P
from test_oracle_math import m31, qm31

pytestmark = pytest.mark.single_conv
FAMS = list(fi.FAMILIES)


# ---- circle group restated over Python integers (generator (2, 1268011823) of order 2^31) ------------------------------------------------
def _padd(p, q):
    return ((p[0] * q[0] - p[1] * q[1]) % P, (p[0] * q[1] + p[1] * q[0]) % P)


def point_of_index(idx):
    res, cur = (1, 0), (2, 1268011823)
    idx &= (1 << 31) - 1
    while idx:
        if idx & 1:
            res = _padd(res, cur)
        cur = _padd(cur, cur)
        idx >>= 1
    return res


def half_odds_points(log):
    """Coset::half_odds(log): initial index 2^(31 - log - 2), step 2^(31 - log)."""
    p, s = point_of_index(1 << (31 - log - 2)), point_of_index(1 << (31 - log))
    out = []
    for _ in range(1 << log):
        out.append(p)
        p = _padd(p, s)
    return out


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def test_generator_has_order_2_31():
    assert point_of_index(1 << 30) == (P - 1, 0) and point_of_index(1 << 29)[0] == 0 and point_of_index(0) == (1, 0)


# ---- field operations at the edge values ----------------------------------------------------------------------------------------------
def test_m31_ops_on_the_edge_cross_product(oracle):
    pairs = list(itertools.product(fi.EDGE_SET, fi.EDGE_SET))
    a = np.array([p[0] for p in pairs], dtype=np.uint32); b = np.array([p[1] for p in pairs], dtype=np.uint32)
    assert m31(oracle, 0, a, b).tolist() == [(x + y) % P for x, y in pairs]
    assert m31(oracle, 1, a, b).tolist() == [(x - y) % P for x, y in pairs]
    assert m31(oracle, 2, a, b).tolist() == [(x * y) % P for x, y in pairs]
    nz = np.array([v for v in fi.EDGE_SET if v], dtype=np.uint32)
    assert m31(oracle, 3, nz).tolist() == [pow(int(v), P - 2, P) for v in nz]


def _qm31_operands():
    """x: the edge set in every coordinate (13^4); y: the constants that drive q_mul_const to its bound, the edge set on the diagonal and draws."""
    xs = np.array(list(itertools.product(fi.EDGE_SET, repeat=4)), dtype=np.uint32)
    ys = [(P - 1,) * 4, (P - 1, 0, P - 1, 0), (P - 1, P - 1, P - 2, 1), (0, 0, 0, 0), (1, 0, 0, 0), (0, 0, 1, 0), (0, P - 1, 0, P - 1)]
    ys += [tuple(int(v) for v in fi.edge(s, 4)) for s in range(4)] + [tuple(int(v) for v in fi.uniform(s, 4)) for s in range(2)]
    return xs, ys


def test_qm31_ops_with_edge_values_in_every_coordinate(oracle):
    """Product by the definition u^2 = 2 + i, i^2 = -1 written out over Python integers (field_inputs.qm31_mul_int), never by the oracle."""
    xs, ys = _qm31_operands()
    xo = xs.astype(object)
    for y in ys:
        yb = np.tile(np.array(y, dtype=np.uint32), xs.shape[0])
        a0, a1, a2, a3 = (xo[:, k] for k in range(4)); b0, b1, b2, b3 = y
        aa = (a0 * b0 - a1 * b1, a0 * b1 + a1 * b0); bb = (a2 * b2 - a3 * b3, a2 * b3 + a3 * b2)
        ab = (a0 * b2 - a1 * b3, a0 * b3 + a1 * b2); ba = (a2 * b0 - a3 * b1, a2 * b1 + a3 * b0)
        want = np.stack([(aa[0] + 2 * bb[0] - bb[1]) % P, (aa[1] + bb[0] + 2 * bb[1]) % P, (ab[0] + ba[0]) % P, (ab[1] + ba[1]) % P], axis=1)
        assert np.array_equal(qm31(oracle, 2, xs.reshape(-1), yb).reshape(-1, 4).astype(object), want), y
        assert np.array_equal(qm31(oracle, 0, xs.reshape(-1), yb).reshape(-1, 4).astype(object), (xo + np.array(y, dtype=object)) % P), y
        assert np.array_equal(qm31(oracle, 1, xs.reshape(-1), yb).reshape(-1, 4).astype(object), (xo - np.array(y, dtype=object)) % P), y
    # the scalar restatement used by the other tests agrees with the vectorised one on the small full cross product
    small = list(itertools.product([0, 1, P - 1, P - 2, 1 << 30], repeat=4))
    for x in small[::7]:
        for y in small[::11]:
            assert qm31(oracle, 2, np.array(x, dtype=np.uint32), np.array(y, dtype=np.uint32)).tolist() == fi.qm31_mul_int(x, y)


def test_qm31_inverse_with_edge_values_in_every_coordinate(oracle):
    xs, _ = _qm31_operands()
    xs = xs[np.any(xs != 0, axis=1)]
    inv = qm31(oracle, 3, xs.reshape(-1)).reshape(-1, 4)
    assert int(inv.max()) < P
    for k in range(0, xs.shape[0], 37):            # exact product over Python integers: x * x^-1 = 1, and the norm-tower inverse agrees
        assert fi.qm31_mul_int(xs[k], inv[k]) == [1, 0, 0, 0]
        assert fi.qm31_inv_int(xs[k]) == inv[k].tolist()
    one = np.tile(np.array([1, 0, 0, 0], dtype=np.uint32), xs.shape[0])
    assert np.array_equal(qm31(oracle, 2, xs.reshape(-1), inv.reshape(-1)), one)      # every element (the product itself is pinned above)


# ---- FRI folds and point evaluation, restated over Python integers ---------------------------------------------------------------------
def _q(cols, i):
    return [int(c[i]) for c in cols]


def _ibutterfly(f0, f1, t):
    return fi.qm31_add_int(f0, f1), [v * t % P for v in fi.qm31_sub_int(f0, f1)]


def py_fold_line(src, log, alpha):
    xs = half_odds_points(log)
    out = []
    for i in range(1 << (log - 1)):
        f0, f1 = _ibutterfly(_q(src, 2 * i), _q(src, 2 * i + 1), pow(xs[bitrev(i << 1, log)][0], P - 2, P))
        out.append(fi.qm31_add_int(f0, fi.qm31_mul_int(alpha, f1)))
    return out


def py_fold_circle_into_line(dst, src, log, alpha):
    half = half_odds_points(log - 1)
    a2 = fi.qm31_mul_int(alpha, alpha)
    out = []
    for i in range(1 << (log - 1)):
        f0, f1 = _ibutterfly(_q(src, 2 * i), _q(src, 2 * i + 1), pow(half[bitrev(i, log - 1)][1], P - 2, P))
        out.append(fi.qm31_add_int(fi.qm31_mul_int(_q(dst, i), a2), fi.qm31_add_int(fi.qm31_mul_int(alpha, f1), f0)))
    return out


def py_eval_at_point(coeffs, log, point8):
    """sum_j coeffs[j] * prod over the set bits b of j of m_b, m_0 = y, m_1 = x, m_(b+1) = 2 m_b^2 - 1."""
    x, y = [int(v) for v in point8[:4]], [int(v) for v in point8[4:]]
    maps = [y]
    for _ in range(1, log):
        maps.append(x)
        x = fi.qm31_sub_int([2 * v for v in fi.qm31_mul_int(x, x)], [1, 0, 0, 0])
    cur = [[int(c), 0, 0, 0] for c in coeffs]
    for b in range(log):
        cur = [fi.qm31_add_int(cur[2 * i], fi.qm31_mul_int(cur[2 * i + 1], maps[b])) for i in range(len(cur) // 2)]
    return cur[0]


def _ptrs(arrs):
    return (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


@pytest.mark.parametrize("cf", list(fi.CONST_FAMILIES))
@pytest.mark.parametrize("fam", FAMS)
def test_oracle_folds_and_point_evaluation_match_python_integers(oracle, fam, cf):
    for log in (1, 2, 3, 6):
        n = 1 << log
        src = fi.columns(fam, 300 + log, 4, n)
        alpha = fi.const(cf, 3, 4)
        want = [np.zeros(n // 2, dtype=np.uint32) for _ in range(4)]
        assert oracle.L.orc_fold_line(_ptrs(src), log, (ctypes.c_uint32 * 4)(*alpha.tolist()), _ptrs(want)) == 0
        assert [_q(want, i) for i in range(n // 2)] == py_fold_line(src, log, alpha.tolist()), ("fold_line", log)
    for log in (3, 4, 6):
        n = 1 << log
        src = fi.columns(fam, 400 + log, 4, n); dst = fi.columns(fam, 500 + log, 4, n // 2)
        alpha = fi.const(cf, 4, 4)
        got = [d.copy() for d in dst]
        assert oracle.L.orc_fold_circle_into_line(_ptrs(got), _ptrs(src), log, (ctypes.c_uint32 * 4)(*alpha.tolist())) == 0
        assert [_q(got, i) for i in range(n // 2)] == py_fold_circle_into_line(dst, src, log, alpha.tolist()), ("fold_circle_into_line", log)
    for log in (1, 4, 6):
        coeffs = fi.column(fam, 100 + log, 1 << log)
        point = fi.const(cf, 7, 8)
        out = (ctypes.c_uint32 * 4)()
        oracle.L.orc_eval_at_point(coeffs.ctypes.data_as(ctypes.c_void_p), log, (ctypes.c_uint32 * 8)(*point.tolist()), out)
        assert list(out) == py_eval_at_point(coeffs, log, point.tolist()), ("eval_at_point", log)


# ---- transforms: identities that hold for any input --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMS)
def test_oracle_transform_round_trips_on_every_family(oracle, fam):
    for log in range(3, 13):
        cols = np.stack(fi.columns(fam, log, 2, 1 << log))
        coeffs = oracle.interpolate(cols, log)
        assert int(coeffs.max()) < P
        assert np.array_equal(oracle.evaluate(coeffs, log, log), cols), log
        if fam == "max":          # a constant column has one non-zero coefficient
            assert (coeffs[:, 0] == P - 1).all() and not coeffs[:, 1:].any()
        for ext in (1, 4, 8):
            lde = oracle.evaluate(coeffs, log, log + ext)
            back = oracle.interpolate(lde, log + ext)
            assert np.array_equal(back[:, : 1 << log], coeffs) and not back[:, 1 << log:].any(), (log, ext)


def test_oracle_evaluate_agrees_with_point_evaluation_at_saturated_inputs(oracle):
    """evaluate(coeffs)[bit_reverse(i)] == eval_at_point(coeffs, domain.at(i)), the latter pinned to Python integers above."""
    log, ext = 5, 3
    for fam in FAMS:
        coeffs = fi.column(fam, 9, 1 << log)
        lde = oracle.evaluate(coeffs[None, :], log, log + ext)[0]
        half = half_odds_points(log + ext - 1)
        for i in (0, 1, 77, (1 << (log + ext)) - 1):
            h = 1 << (log + ext - 1)
            x, y = half[i] if i < h else (half[i - h][0], (P - half[i - h][1]) % P)
            assert py_eval_at_point(coeffs, log, [x, 0, 0, 0, y, 0, 0, 0]) == [int(lde[bitrev(i, log + ext)]), 0, 0, 0], (fam, i)


# ---- preconditions of the GPU matrix -----------------------------------------------------------------------------------------------------
def test_families_are_canonical_and_hit_their_edges():
    r = fi.HEAVY_ROOT
    assert sum(pow(r, i, P) for i in range(1, 6)) * (P - 1) >= 1 << 64 and 1 + 4 * (P - 1) ** 2 + (P - 1) < 1 << 64
    cand = np.arange(9 * (P // 10), r + 1, dtype=np.uint64)            # the literal is what its comment says: the smallest such r from 0.9 P up
    ok, pw = np.ones(cand.size, dtype=bool), cand.copy()
    for _ in range(5):
        ok &= pw * np.uint64(100) > np.uint64(85 * P)
        pw = (pw * cand) % np.uint64(P)
    assert int(cand[np.argmax(ok)]) == r and ok[-1]
    for fam in FAMS:
        for n in (1, 2, 8, 1024):
            v = fi.column(fam, 5, n)
            assert v.dtype == np.uint32 and int(v.max()) < P
    n = 1024
    for stride, name in ((1, "complement1"), (2, "complement2"), (n // 2, "complement_half"), (1, "complement1_uniform")):
        v = fi.column(name, 5, n).astype(np.int64)
        i = np.arange(n)
        assert (((v + v[i ^ stride]) % P) == 0).all() and ((v + v[i ^ stride]) == P).sum() > n // 2      # sums are exactly P (0 + 0 aside)
    for stride, name in ((1, "equal1"), (2, "equal2"), (n // 2, "equal_half")):
        v = fi.column(name, 5, n)
        assert np.array_equal(v, v[np.arange(n) ^ stride])
    assert set(np.unique(fi.edge(1, 4096)).tolist()) == set(fi.EDGE_SET)
    cols = fi.columns("sparse", 3, 4, 64)
    assert cols[0][0] == P - 1 and cols[1][63] == P - 1 and all(int(c.astype(np.int64).sum()) == P - 1 for c in cols)


def _cm(p, q):
    return ((p[0] * q[0] - p[1] * q[1]) % P, (p[0] * q[1] + p[1] * q[0]) % P)


def test_no_quotient_denominator_of_the_gpu_matrix_is_zero():
    """(Re(px) - x) Im(py) - (Re(py) - y) Im(px) over CM31 for every sample point the GPU tests use and every point of their domains."""
    from test_gpu_field_edges import QUOTIENT_LOGS, quotient_points
    for log in QUOTIENT_LOGS:
        half = half_odds_points(log - 1)
        xs = np.array([p[0] for p in half], dtype=object); ys = np.array([p[1] for p in half], dtype=object)
        for cf in fi.CONST_FAMILIES:
            for pt in quotient_points(cf):
                prx, pix, pry, piy = (pt[0], pt[1]), (pt[2], pt[3]), (pt[4], pt[5]), (pt[6], pt[7])
                for sign in (1, -1):                           # the domain holds the half coset and its conjugates
                    dx0, dy0 = (prx[0] - xs) % P, (pry[0] - sign * ys) % P
                    d_re = (dx0 * piy[0] - prx[1] * piy[1] - (dy0 * pix[0] - pry[1] * pix[1])) % P
                    d_im = (dx0 * piy[1] + prx[1] * piy[0] - (dy0 * pix[1] + pry[1] * pix[0])) % P
                    assert not ((d_re == 0) & (d_im == 0)).any(), (log, cf, pt)


def test_no_batch_inverse_operand_of_the_gpu_matrix_is_zero():
    from test_gpu_field_edges import BATCH_INVERSE_SIZES, batch_inverse_operands
    for fam in FAMS:
        for n in BATCH_INVERSE_SIZES:
            m, q = batch_inverse_operands(fam, n)
            assert (m != 0).all() and int(m.max()) < P
            qo = np.stack(q).astype(object)
            # a QM31 x is zero iff all coordinates are; its inverse needs the norm chain non-zero, which holds for every non-zero x (a field)
            assert np.any(np.stack(q) != 0, axis=0).all() and int(np.stack(q).max()) < P and qo.shape == (4, n)


def test_no_logup_or_constraint_denominator_of_the_gpu_matrix_is_zero(oracle):
    """The oracle throws on an inverse of zero (field.h inv): every (component, family pair, row count) of the GPU logUp matrix and every
    (component, family pair) of the constraint matrix at log_size 6 runs clean on the CPU."""
    from test_gpu_field_edges import CONSTRAINT_FAMILIES, LOGUP_PAIRS, LOGUP_ROWS, constraint_inputs, logup_inputs
    for comp in range(13):
        for cols_f, const_f in LOGUP_PAIRS:
            for rows in LOGUP_ROWS:
                r, elems = logup_inputs(comp, cols_f, const_f, rows)
                out, claimed = oracle.logup_generate(comp, r, elems)
                assert int(out.max()) < P and max(claimed) < P
        for cols_f, const_f in CONSTRAINT_FAMILIES:
            a = constraint_inputs(comp, 6, cols_f, const_f)
            got = oracle.eval_constraints(comp, 6, a["is_first"], a["main"], a["inter"], a["elems"], a["claimed"], a["coeffs"], a["acc"])
            assert int(got.max()) < P
