"""Deterministic input families for the field kernels: canonical M31 columns (every cell < P; P itself is never fed) that sit where the
lazily reduced arithmetic of the kernels was cut close — all cells P - 1, the edge set around 0, 2^16, 2^30 and P, butterfly partners whose
sum is exactly P or whose difference is 0 — beside the uniform columns every older test draws. Each family is f(seed, n) -> np.uint32[n].
QM31 constants (points, alphas, lookup elements, coefficients) take the same families at length 4 / 8 / 24, plus three that drive
m31.h q_mul_const to its bound (CONST_FAMILIES). Plain module, shared by test_field_inputs_cpu.py and test_gpu_field_edges.py."""
import numpy as np

from conftest import splitmix_column, P

EDGE_SET = [0, 1, 2, P - 1, P - 2, 1 << 30, (1 << 30) - 1, (1 << 30) + 1, 0xFFFF, 0x10000, P - 0x10000, (P - 1) // 2, (P + 1) // 2]


def _splitmix_u64(seed, n):
    x = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def uniform(seed, n):
    return splitmix_column(seed, n)


def max_(seed, n):
    return np.full(n, P - 1, dtype=np.uint32)


def edge(seed, n):
    idx = (_splitmix_u64(seed ^ 0xED6E, n) % np.uint64(len(EDGE_SET))).astype(np.int64)
    return np.array(EDGE_SET, dtype=np.uint32)[idx]


def _paired(base, stride, partner):
    """v[i ^ stride] = partner(v[i]) for every i whose `stride` bit is clear (stride a power of two; a cell without a partner below n keeps
    the base value)."""
    v = base.copy()
    n = v.size
    if stride < 1 or stride >= n:
        return v
    i = np.arange(n)
    lo = i[((i & stride) == 0) & ((i ^ stride) < n)]
    v[lo ^ stride] = partner(v[lo])
    return v


def complement(stride, base=edge):
    """Butterfly partners at distance `stride` sum to exactly P (m_add at s == P); stride "half" = n / 2."""
    def f(seed, n):
        s = n // 2 if stride == "half" else stride
        return _paired(base(seed, n), s, lambda x: ((P - x.astype(np.int64)) % P).astype(np.uint32))
    f.__name__ = f"complement_{stride}_{base.__name__}"
    return f


def equal(stride, base=edge):
    """Butterfly partners at distance `stride` are equal (m_sub at 0)."""
    def f(seed, n):
        s = n // 2 if stride == "half" else stride
        return _paired(base(seed, n), s, lambda x: x)
    f.__name__ = f"equal_{stride}_{base.__name__}"
    return f


def sparse(seed, n):
    """All zero but one cell P - 1; seeds 0 and 1 put it at cell 0 and cell n - 1."""
    v = np.zeros(n, dtype=np.uint32)
    pos = 0 if seed % 8 == 0 else n - 1 if seed % 8 == 1 else int(_splitmix_u64(seed, 1)[0] % np.uint64(n))
    v[pos] = P - 1
    return v


FAMILIES = {
    "uniform": uniform, "max": max_, "edge": edge,
    "complement1": complement(1), "complement2": complement(2), "complement_half": complement("half"), "complement1_uniform": complement(1, uniform),
    "equal1": equal(1), "equal2": equal(2), "equal_half": equal("half"),
    "sparse": sparse,
}
BIG_FAMILIES = ("uniform", "max", "edge")      # sizes >= 2^20: bounds the oracle's CPU time


def column(family, seed, n):
    v = FAMILIES[family](seed, n)
    assert v.dtype == np.uint32 and v.shape == (n,) and (n == 0 or int(v.max()) < P)
    return v


def columns(family, seed, k, n):
    """k columns; `sparse` walks the seeds so that cells 0 and n - 1 are both hit."""
    return [column(family, seed + 8 * j if family != "sparse" else seed * 8 + j, n) for j in range(k)]


# ---- QM31 constants ---------------------------------------------------------------------------------------------------------------------
def _tile4(q):
    return lambda seed, n: np.array((list(q) * ((n + 3) // 4))[:n], dtype=np.uint32)


CONST_FAMILIES = {
    "uniform": uniform, "max": max_, "edge": edge,
    "nc_is_p": _tile4((P - 1, 0, P - 1, 0)),           # q_const keeps nc1 = P - c1, nc3 = P - c3: both become P itself
    "ne_is_p": _tile4((P - 1, P - 1, P - 2, 1)),       # c2 + 2 c3 = 0 (mod P): e1 = 0 and the kept ne1 = P - e1 becomes P
}


# The smallest r >= 0.9 P whose powers r, r^2, .., r^5 all exceed 0.85 P (a constant of P; test_field_inputs_cpu.py checks the property and the
# minimality): with alpha = r (a real QM31) and cells P - 1 the sum alpha^1 v1 + .. + alpha^5 v5 exceeds 4.25 P (P - 1) > 2^64 — five such
# products can never share a 64-bit accumulator, whatever the fold schedule of air.h combine_base becomes (today: three products between folds).
HEAVY_ROOT = 1932738145
# constants that are only legal as lookup elements / coefficients (a sample point without an imaginary part has a zero quotient denominator)
LOOKUP_FAMILIES = dict(CONST_FAMILIES, heavy=_tile4((HEAVY_ROOT, 0, 0, 0)))
LOOKUP_CROSS = [("max", "heavy"), ("uniform", "heavy")]
# columns x constants, crossed (not tied): derived multiplicands (weights, quotient coefficients, constraint values) meet P - 1 given ones
CROSS = [("uniform", "max"), ("edge", "max"), ("max", "max"), ("max", "uniform"), ("edge", "edge"), ("uniform", "uniform"),
         ("max", "nc_is_p"), ("max", "ne_is_p"), ("edge", "nc_is_p")]


def const(family, seed, n):
    v = LOOKUP_FAMILIES[family](seed, n)
    assert v.dtype == np.uint32 and v.shape == (n,) and int(v.max()) < P
    return v


# ---- exact integer arithmetic (the expected values of the primitive tests) --------------------------------------------------------------
def qm31_mul_int(x, y):
    """(a0 + a1 i + (a2 + a3 i) u)(b0 + b1 i + (b2 + b3 i) u) with i^2 = -1, u^2 = 2 + i, over Python integers."""
    a0, a1, a2, a3 = [int(v) for v in x]
    b0, b1, b2, b3 = [int(v) for v in y]
    cm = lambda p, q, r, s: (p * r - q * s, p * s + q * r)              # (p + q i)(r + s i)
    aa, bb, ab, ba = cm(a0, a1, b0, b1), cm(a2, a3, b2, b3), cm(a0, a1, b2, b3), cm(a2, a3, b0, b1)
    rb = (2 * bb[0] - bb[1], bb[0] + 2 * bb[1])                         # (2 + i) * bb
    return [(aa[0] + rb[0]) % P, (aa[1] + rb[1]) % P, (ab[0] + ba[0]) % P, (ab[1] + ba[1]) % P]


def qm31_add_int(x, y):
    return [(int(a) + int(b)) % P for a, b in zip(x, y)]


def qm31_sub_int(x, y):
    return [(int(a) - int(b)) % P for a, b in zip(x, y)]


def qm31_pow_int(x, e):
    r = [1, 0, 0, 0]
    while e:
        if e & 1:
            r = qm31_mul_int(r, x)
        x = qm31_mul_int(x, x)
        e >>= 1
    return r


def qm31_inv_int(x):
    """x^(P^4 - 2) would be exact but slow; use the norm tower instead: x^-1 = conj(x) / (x conj(x)), the norm lies in CM31, and a CM31
    inverse is conj / (a^2 + b^2) with an M31 inverse by Fermat. Every step over Python integers; checked by x * x^-1 == 1 in the caller."""
    a0, a1, a2, a3 = [int(v) for v in x]
    # x conj(x) = (a0 + a1 i)^2 - (2 + i)(a2 + a3 i)^2
    s0, s1 = a0 * a0 - a1 * a1, 2 * a0 * a1
    t0, t1 = a2 * a2 - a3 * a3, 2 * a2 * a3
    n0, n1 = (s0 - (2 * t0 - t1)) % P, (s1 - (t0 + 2 * t1)) % P
    d = pow((n0 * n0 + n1 * n1) % P, P - 2, P)
    i0, i1 = n0 * d % P, (-n1 * d) % P                                  # 1 / (n0 + n1 i)
    return qm31_mul_int([a0, a1, (-a2) % P, (-a3) % P], [i0, i1, 0, 0])
