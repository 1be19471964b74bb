"""A pure-numpy model of the fraction program (include/bfhip.h "Fraction programs"), written from the header's contract alone: the bytecode
run over QM31 values with the arithmetic of tests/air_model.py, a vectorised QM31 inverse, and LogupTraceGenerator::finalize_last's
coset-order prefix sum from the group indices of the M31 circle (no index trick of the kernels). Anchored on the oracle's
gen_interaction_trace by tests/test_logup_program_cpu.py for the 13 Brainfuck programs, and from there the yardstick of every generic shape
of tests/test_gpu_logup_program.py. Also here: a seeded generator of random fraction programs."""
import random

import numpy as np

import air_model
from air_model import (M_COL, M_CONST, M_ADD, M_SUB, M_MUL, M_NEG, Q_COL, Q_PARAM, Q_FROM_M, Q_ADD, Q_SUB, Q_MUL, Q_MULM, P, q, q_add, q_sub,
                       q_mul, from_m, combine_ef)

FRAC, END_COL = 15, 16
_P = np.uint64(P)


def m_pow(x, e):
    """x^e over M31, x a uint64 array"""
    r, b = np.ones_like(x), x.copy()
    while e:
        if e & 1:
            r = r * b % _P
        b = b * b % _P
        e >>= 1
    return r


def q_inv(x):
    """1 / x for (4, n) QM31 values: with x = a + b u (a, b in CM31, u^2 = 2 + i), 1 / x = (a - b u) / (a^2 - (2 + i) b^2); the CM31
    inverse is the conjugate over the norm, the M31 inverse the power p - 2. The inverse of 0 comes out 0: callers look for zeros first."""
    cmul = air_model._cmul
    aa, bb = cmul(x[0], x[1], x[0], x[1]), cmul(x[2], x[3], x[2], x[3])
    rbb = cmul(bb[0], bb[1], np.uint64(2), np.uint64(1))
    n0, n1 = (aa[0] + (_P - rbb[0])) % _P, (aa[1] + (_P - rbb[1])) % _P                   # the norm a^2 - (2 + i) b^2, in CM31
    inv = m_pow((n0 * n0 % _P + n1 * n1 % _P) % _P, P - 2)
    d0, d1 = n0 * inv % _P, (_P - n1) % _P * inv % _P                                    # 1 / norm
    lo, hi = cmul(x[0], x[1], d0, d1), cmul((_P - x[2]) % _P, (_P - x[3]) % _P, d0, d1)
    return np.stack([lo[0], lo[1], hi[0], hi[1]])


def coset_position(log_size):
    """For every storage cell of CanonicCoset(log_size).circle_domain() in bit-reversed order: its index in the coset's own order. Group
    indices of the circle (order 2^31): the coset is I + i T with I = 2^(30 - log_size), T = 2^(31 - log_size); the circle domain's half
    coset is I + d (2 T), d < n / 2, its second half the conjugates -(I + (d - n / 2) (2 T))."""
    n, half, order = 1 << log_size, 1 << (log_size - 1), 1 << 31
    I, T = 1 << (30 - log_size), 1 << (31 - log_size)
    d = air_model.bit_reverse(np.arange(n), log_size)
    g = np.where(d < half, I + d * 2 * T, -(I + (d - half) * 2 * T)) % order
    assert np.all((g - I) % T == 0)
    pos = ((g - I) // T) % n
    assert np.bincount(pos, minlength=n).min() == 1
    return pos


def columns(code, read, params, n):
    """The program over n cells. read(col) -> (n,) cells of that column. Returns ([per logUp column the (4, n) per-cell value: column k - 1 plus
    the sum of column k's fractions], [(cell, fraction) of every zero denominator])."""
    m, qr = {}, {}
    cur, out, zeros, fi = np.zeros((4, n), dtype=np.uint64), [], [], 0
    for i in range(0, len(code), 4):
        op, dst, a, b = code[i: i + 4]
        if op == M_COL:
            assert b == 0
            m[dst] = from_m(read(a).astype(np.uint64))
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
            assert b == 0
            qr[dst] = combine_ef(*[from_m(read(a + k).astype(np.uint64)) for k in range(4)])
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
        elif op == FRAC:
            zeros += [(int(c), fi) for c in np.nonzero(~qr[b].any(axis=0))[0]]
            cur = q_add(cur, q_mul(qr[a], q_inv(qr[b])))
            fi += 1
        elif op == END_COL:
            out.append(cur)
        else:
            raise ValueError("opcode %d" % op)
    return out, zeros


def generate(code, cols, shifts, params, log_size):
    """bfhip_logup_program_generate: cols[k] holds 2^(log_size - shifts[k]) cells. Returns ((4 * n_logup, 2^log_size) uint32 coordinate
    columns, claimed sum as 4 ints, the zero denominators sorted as the entry point names them: lowest cell, then lowest fraction)."""
    n = 1 << log_size
    cell = np.arange(n)
    per_col, zeros = columns(code, lambda k: np.asarray(cols[k])[cell >> shifts[k]], params, n)
    pos = coset_position(log_size)
    order = np.argsort(pos)                                        # storage cells in coset order
    last = per_col[-1][:, order]
    prefix = np.cumsum(last, axis=1) % _P                          # < 2^31 * 2^log_size: no overflow in uint64
    final = np.empty_like(prefix)
    final[:, order] = prefix
    out = np.concatenate(per_col[:-1] + [final]).astype(np.uint32)
    return out, [int(v) for v in prefix[:, -1]], sorted(zeros)


def random_program(seed, n_logup_cols, n_fractions, n_cols=6, n_params=3, m_pool=5, q_pool=4):
    """A seeded random fraction program: n_fractions fractions spread over n_logup_cols columns (each at least one). Every numerator is a sum
    with a QM31 parameter in it (a secure numerator); every denominator is param * (an M31 expression of the columns) - param plus a secure
    column, so that on distinct random cells none vanishes. Register pools are small: registers are overwritten and reused."""
    rng = random.Random(seed)
    assert n_fractions >= n_logup_cols and n_cols >= 5
    code = []
    per_col = [1] * n_logup_cols
    for _ in range(n_fractions - n_logup_cols):
        per_col[rng.randrange(n_logup_cols)] += 1
    for k in range(n_logup_cols):
        for _ in range(per_col[k]):
            m0, m1, m2 = rng.sample(range(m_pool), 3)
            q0, q1, q2 = rng.sample(range(q_pool), 3)
            code += [M_COL, m0, rng.randrange(n_cols), 0, M_COL, m1, rng.randrange(n_cols), 0, M_CONST, m2, rng.choice([1, 2, P - 1, rng.randrange(P)]), 0]
            code += [rng.choice([M_ADD, M_SUB, M_MUL]), m2, m1, m2, M_NEG, m1, m2, rng.getrandbits(32)]       # an unused word is ignored
            # numerator q0 = param * m0 + param (or - param): a QM31 value
            code += [Q_PARAM, q0, rng.randrange(n_params), 0, Q_MULM, q0, q0, m0, Q_PARAM, q1, rng.randrange(n_params), 0, rng.choice([Q_ADD, Q_SUB]), q0, q0, q1]
            # denominator q1 = param * m2 - param + secure column * (m1 lifted)
            code += [Q_PARAM, q1, rng.randrange(n_params), 0, Q_MULM, q1, q1, m2, Q_PARAM, q2, rng.randrange(n_params), 0, Q_SUB, q1, q1, q2]
            code += [Q_COL, q2, rng.randrange(n_cols - 3), 0, Q_FROM_M, (q2 + 1) % q_pool if (q2 + 1) % q_pool not in (q0, q1) else q2, m1, 0]
            code += [Q_MUL, q2, q2, q2, Q_ADD, q1, q1, q2]
            code += [FRAC, 0, q0, q1]
        code += [END_COL, 0, 0, 0]
    return code, n_cols, n_params
