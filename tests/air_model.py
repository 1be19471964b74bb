"""A pure-numpy model of the constraint program (include/bfhip.h "Constraint programs"): the bytecode run over QM31 values, written from the
header's table alone. Both register files hold QM31 values as uint64 arrays of shape (4, n): n = 1 at a point (a mask value per (column,
offset)), n = the rows of a domain (an M31 cell v is (v, 0, 0, 0)). The result is sum_j coeffs[j] * C_j WITHOUT the vanishing denominator
(run), or every C_j on its own (constraint_values).
Also here: the row-offset map of a bit-reversed circle domain from first principles (group indices of the M31 circle), the vanishing
polynomial of a canonic coset at a point, its inverse at every row of a constraint domain (domain_denominators), and a seeded generator of
random valid programs that uses every opcode and reuses registers.
Shared by tests/test_air_program_cpu.py, tests/test_gpu_air_program.py and tests/test_gpu_program_edges.py."""
import random

import numpy as np

P = (1 << 31) - 1
(M_COL, M_CONST, M_ADD, M_SUB, M_MUL, M_NEG, Q_COL, Q_PARAM, Q_FROM_M, Q_ADD, Q_SUB, Q_MUL, Q_MULM, C_BASE, C_EXT) = range(15)
_P = np.uint64(P)


def q(v, n=1):
    """4 words -> (4, n) uint64"""
    return np.repeat(np.array([int(w) for w in v], dtype=np.uint64).reshape(4, 1), n, axis=1)


def from_m(col):
    """M31 cells (n,) -> (4, n)"""
    out = np.zeros((4, len(col)), dtype=np.uint64)
    out[0] = col
    return out


def _cmul(a0, a1, b0, b1):
    return (a0 * b0 % _P + (_P - a1 * b1 % _P)) % _P, (a0 * b1 % _P + a1 * b0 % _P) % _P


def q_add(x, y):
    return (x + y) % _P


def q_sub(x, y):
    return (x + (_P - y)) % _P


def q_mul(x, y):
    """(a + b u)(c + d u), u^2 = 2 + i, over CM31 = M31[i]"""
    ac, ad, bc, bd = _cmul(x[0], x[1], y[0], y[1]), _cmul(x[0], x[1], y[2], y[3]), _cmul(x[2], x[3], y[0], y[1]), _cmul(x[2], x[3], y[2], y[3])
    e = _cmul(bd[0], bd[1], np.uint64(2), np.uint64(1))
    return np.stack([(ac[0] + e[0]) % _P, (ac[1] + e[1]) % _P, (ad[0] + bc[0]) % _P, (ad[1] + bc[1]) % _P])


def combine_ef(v0, v1, v2, v3):
    """SecureField::from_partial_evals: v0 + v1 i + v2 u + v3 iu"""
    n = v0.shape[1]
    r = v0
    for v, basis in ((v1, (0, 1, 0, 0)), (v2, (0, 0, 1, 0)), (v3, (0, 0, 0, 1))):
        r = q_add(r, q_mul(v, q(basis, n)))
    return r


def constraint_values(code, read, params, n=1):
    """The interpreter itself: yields (C_BASE or C_EXT, the constraint's value as (4, n)) for every constraint, in program order, in one pass
    over the code. code: flat u32 words; read(col, off) -> (4, n) value of that column at that row offset; params: lists of 4 words."""
    m, qr = {}, {}
    signed = lambda w: w - (1 << 32) if w >= 1 << 31 else w
    for i in range(0, len(code), 4):
        op, dst, a, b = code[i: i + 4]
        if op == M_COL:
            m[dst] = read(a, signed(b))
        elif op == M_CONST:
            m[dst] = q((a, 0, 0, 0), n)
        elif op == M_ADD:
            m[dst] = q_add(m[a], m[b])
        elif op == M_SUB:
            m[dst] = q_sub(m[a], m[b])
        elif op == M_MUL:
            m[dst] = q_mul(m[a], m[b])
        elif op == M_NEG:
            m[dst] = q_sub(np.zeros((4, n), dtype=np.uint64), m[a])
        elif op == Q_COL:
            qr[dst] = combine_ef(*[read(a + k, signed(b)) for k in range(4)])
        elif op == Q_PARAM:
            qr[dst] = q(params[a], n)
        elif op == Q_FROM_M:
            qr[dst] = m[a]
        elif op == Q_ADD:
            qr[dst] = q_add(qr[a], qr[b])
        elif op == Q_SUB:
            qr[dst] = q_sub(qr[a], qr[b])
        elif op == Q_MUL:
            qr[dst] = q_mul(qr[a], qr[b])
        elif op == Q_MULM:
            qr[dst] = q_mul(qr[a], m[b])
        elif op in (C_BASE, C_EXT):
            yield op, (m[a] if op == C_BASE else qr[a])
        else:
            raise ValueError("opcode %d" % op)


def run(code, read, params, coeffs, n=1):
    """code, read, params: as for constraint_values; coeffs: lists of 4 words. Returns sum_j coeffs[j] * C_j as (4, n)."""
    acc, ci = np.zeros((4, n), dtype=np.uint64), 0
    for _, value in constraint_values(code, read, params, n):
        acc = q_add(acc, q_mul(q(coeffs[ci], n), value))
        ci += 1
    assert ci == len(coeffs)
    return acc


def bit_reverse(i, log):
    i = np.asarray(i, dtype=np.int64)
    out = np.zeros_like(i)
    for k in range(log):
        out |= ((i >> k) & 1) << (log - 1 - k)
    return out


def offset_rows(log_size, log_expand, off):
    """For every storage index of CanonicCoset(log_size + log_expand).circle_domain() in bit-reversed order: the storage index of the point
    plus off * CanonicCoset(log_size).step(). From the group indices of the circle (generator of order 2^31): the domain's half coset is
    I + k S with I = 2^(30 - el), S = 2^(32 - el), its second half the conjugates; the trace step is 2^(31 - log_size)."""
    el = log_size + log_expand
    n, half, order = 1 << el, 1 << (el - 1), 1 << 31
    I, S, T = 1 << (30 - el), 1 << (32 - el), 1 << (31 - log_size)
    d = bit_reverse(np.arange(n), el)
    g = np.where(d < half, I + d * S, -(I + (d - half) * S)) % order
    g = (g + off * T) % order
    first = ((g - I) % S == 0) & ((g - I) // S < half) & (g >= I)
    neg = (-g) % order
    dd = np.where(first, (g - I) // S, half + (neg - I) // S)
    assert np.all(np.where(first, True, ((neg - I) % S == 0) & ((neg - I) // S < half)))
    return bit_reverse(dd, el)


def domain_reader(cols, log_size, log_expand):
    """cols: full-size columns (n_cols, 2^(log_size + log_expand)) -> read(col, off) for run()"""
    maps = {}

    def read(col, off):
        if off == 0:
            return from_m(cols[col].astype(np.uint64))
        if off not in maps:
            maps[off] = offset_rows(log_size, log_expand, off)
        return from_m(cols[col][maps[off]].astype(np.uint64))
    return read


def coset_vanishing(log_size, point8):
    """coset_vanishing(CanonicCoset(log_size).coset, point): the x coordinate doubled log_size - 1 times (x -> 2 x^2 - 1); the rotation in
    front of it is by -initial + step / 2 = 0 for a canonic coset. 4 words."""
    x = q(point8[:4])
    for _ in range(1, log_size):
        x2 = q_mul(x, x)
        x = q_sub(q_add(x2, x2), q((1, 0, 0, 0)))
    return [int(v) for v in x[:, 0]]


CIRCLE_GEN = (2, 1268011823)      # the generator of the M31 circle group (order 2^31)


def circle_x(index):
    """x coordinate of G^index over Python integers"""
    mul = lambda p, q: ((p[0] * q[0] - p[1] * q[1]) % P, (p[0] * q[1] + p[1] * q[0]) % P)
    res, cur = (1, 0), CIRCLE_GEN
    while index:
        if index & 1:
            res = mul(res, cur)
        cur, index = mul(cur, cur), index >> 1
    return res[0]


def domain_group_indices(log_size, log_expand):
    """Group index of the point of every storage row of CanonicCoset(log_size + log_expand).circle_domain() in bit-reversed order (the
    indices offset_rows starts from)."""
    el = log_size + log_expand
    n, half, order = 1 << el, 1 << (el - 1), 1 << 31
    I, S = 1 << (30 - el), 1 << (32 - el)
    d = bit_reverse(np.arange(n), el)
    return np.where(d < half, I + d * S, -(I + (d - half) * S)) % order


def domain_denominators(log_size, log_expand):
    """1 / coset_vanishing(CanonicCoset(log_size).coset, p) for the point p of every storage row of the constraint domain, as (n,) uint64:
    the x of G^index doubled log_size - 1 times (x -> 2 x^2 - 1), inverted by Fermat. Exact Python integers, every row on its own: that
    the value depends on row >> log_size only is the kernel's table, not something the model assumes."""
    out = []
    for g in domain_group_indices(log_size, log_expand).tolist():
        x = circle_x(g)
        for _ in range(1, log_size):
            x = (2 * x * x - 1) % P
        assert x != 0, "a point of the constraint domain lies on the trace domain"
        out.append(pow(x, P - 2, P))
    return np.array(out, dtype=np.uint64)


def random_program(seed, n_cols=9, n_params=3, n_ops=60, m_pool=6, q_pool=4, max_off=2, max_cons=60):
    """A random valid program over small register pools (so registers are overwritten and reused all the time). Every opcode appears;
    at most max_cons constraints (64 = BFHIP_AIR_MAX_CONSTRAINTS; the default keeps what every earlier seed generated).
    Returns (code words, n_cols, n_params, n_constraints)."""
    rng = random.Random(seed)
    code, mw, qw, n_cons, used = [], set(), set(), 0, set()
    off = lambda: rng.choice([0, 0, 0] + list(range(-max_off, max_off + 1))) & 0xFFFFFFFF
    value = lambda: rng.choice([0, 1, P - 1, rng.randrange(P)])

    def emit(op):
        nonlocal n_cons
        md, qd = rng.randrange(m_pool), rng.randrange(q_pool)
        if op == M_COL:
            code.extend([op, md, rng.randrange(n_cols), off()]); mw.add(md)
        elif op == M_CONST:
            code.extend([op, md, value(), 0]); mw.add(md)
        elif op in (M_ADD, M_SUB, M_MUL) and mw:
            code.extend([op, md, rng.choice(sorted(mw)), rng.choice(sorted(mw))]); mw.add(md)
        elif op == M_NEG and mw:
            code.extend([op, md, rng.choice(sorted(mw)), rng.getrandbits(32)]); mw.add(md)      # an unused word is ignored
        elif op == Q_COL:
            code.extend([op, qd, rng.randrange(n_cols - 3), off()]); qw.add(qd)
        elif op == Q_PARAM:
            code.extend([op, qd, rng.randrange(n_params), 0]); qw.add(qd)
        elif op == Q_FROM_M and mw:
            code.extend([op, qd, rng.choice(sorted(mw)), 0]); qw.add(qd)
        elif op in (Q_ADD, Q_SUB, Q_MUL) and qw:
            code.extend([op, qd, rng.choice(sorted(qw)), rng.choice(sorted(qw))]); qw.add(qd)
        elif op == Q_MULM and qw and mw:
            code.extend([op, qd, rng.choice(sorted(qw)), rng.choice(sorted(mw))]); qw.add(qd)
        elif op == C_BASE and mw and n_cons < max_cons:
            code.extend([op, rng.getrandbits(32), rng.choice(sorted(mw)), 0]); n_cons += 1
        elif op == C_EXT and qw and n_cons < max_cons:
            code.extend([op, 0, rng.choice(sorted(qw)), 0]); n_cons += 1
        else:
            return
        used.add(op)

    for op in (M_COL, M_CONST, Q_PARAM, Q_COL):
        emit(op)
    for _ in range(n_ops):
        emit(rng.randrange(15))
    for op in range(15):          # whatever chance left out; the two constraint kinds last, so the program ends on constraints
        if op not in used or op >= C_BASE:
            emit(op)
    assert used == set(range(15))
    return code, n_cols, n_params, n_cons
