"""A witness program (include/bfhip.h "Witness programs") restated in plain Python over a row-order table: what
bfhip_witness_program_eval_table, and through it the kernel, is compared against. Nothing here calls the library."""
import random

P = (1 << 31) - 1
(M_COL, M_CONST, M_ADD, M_SUB, M_MUL, M_NEG) = range(6)
(ARG, ROW, INV0, IS_ZERO, LT, AND, SHR, STORE) = range(19, 27)


def _signed(w):
    return w - (1 << 32) if w >= 1 << 31 else w


def _step(op, a, b, m, table, r, args):
    """The value one register-writing instruction produces at row r."""
    if op == M_COL:
        return table[(r + _signed(b)) % len(table)][a]
    if op == M_CONST:
        return a
    if op == M_ADD:
        return (m[a] + m[b]) % P
    if op == M_SUB:
        return (m[a] - m[b]) % P
    if op == M_MUL:
        return m[a] * m[b] % P
    if op == M_NEG:
        return -m[a] % P
    if op == ARG:
        return args[a]
    if op == ROW:
        return r
    if op == INV0:
        return pow(m[a], P - 2, P)
    if op == IS_ZERO:
        return int(m[a] == 0)
    if op == LT:
        return int(m[a] < m[b])
    if op == AND:
        return m[a] & b
    if op == SHR:
        return m[a] >> b
    raise AssertionError("opcode %d" % op)


def eval_table(code, table, args, n_out, inv0_seen=None):
    """code: flat words {op, dst, a, b}; table: 2^log_size rows of n_cols canonical words, row order; returns the rows of n_out words.
    inv0_seen: a list that receives every value an INV0 reads."""
    n = len(table)
    assert n >= 2 and n & (n - 1) == 0
    out = [[None] * n_out for _ in range(n)]
    for r in range(n):
        m = {}
        for i in range(0, len(code), 4):
            op, dst, a, b = code[i: i + 4]
            if op == STORE:
                assert out[r][dst] is None
                out[r][dst] = m[a]
                continue
            if op == INV0 and inv0_seen is not None:
                inv0_seen.append(m[a])
            m[dst] = _step(op, a, b, m, table, r, args)
    return out


def random_program(rng, n_cols, n_out, n_args, n_instr, offsets=(0,), n_regs=12):
    """A valid random program: every opcode the family admits, column reads at `offsets`, every output stored once at a random place.
    Every INV0 reads a register just loaded from a column, so that the table decides whether it inverts zero."""
    code, written = [], []
    stores = set(rng.sample(range(4, n_instr + n_out), n_out))
    pending = list(range(n_out))
    rng.shuffle(pending)

    def reg():
        return rng.choice(written)

    def emit(op, dst, a=0, b=0):
        code.extend([op, dst, a & 0xFFFFFFFF, b & 0xFFFFFFFF])
        if op != STORE and dst not in written:
            written.append(dst)

    emit(M_COL, 0, rng.randrange(n_cols), rng.choice(offsets))
    emit(M_CONST, 1, rng.choice([0, 1, P - 1, rng.randrange(P)]))
    for k in range(2, n_instr + n_out):
        if k in stores:
            emit(STORE, pending.pop(), reg())
            continue
        dst = rng.randrange(n_regs)
        what = rng.randrange(14)
        if what < 3:
            emit(M_COL, dst, rng.randrange(n_cols), rng.choice(offsets))
        elif what == 3:
            emit(M_CONST, dst, rng.choice([0, 1, P - 1, rng.randrange(P)]))
        elif what < 7:
            emit(rng.choice([M_ADD, M_SUB, M_MUL]), dst, reg(), reg())
        elif what == 7:
            emit(M_NEG, dst, reg())
        elif what == 8 and n_args:
            emit(ARG, dst, rng.randrange(n_args))
        elif what in (8, 9):
            emit(ROW, dst)
        elif what == 10:
            emit(M_COL, dst, rng.randrange(n_cols), rng.choice(offsets))
            emit(INV0, rng.randrange(n_regs), dst)
        elif what == 11:
            emit(rng.choice([IS_ZERO, LT]), dst, reg(), reg())
        elif what == 12:
            emit(AND, dst, reg(), rng.choice([0, 1, 0xFF, 0x7FFFFFFF, rng.randrange(1 << 31)]))
        else:
            emit(SHR, dst, reg(), rng.choice([0, 1, 30, rng.randrange(31)]))
    return code


def random_table(rng, log_size, n_cols, fill=None):
    """2^log_size rows of n_cols canonical words: edge values likely, or every cell `fill`."""
    pick = (lambda: fill) if fill is not None else (lambda: rng.choice([0, 0, 1, P - 1, P - 2, rng.randrange(P), rng.randrange(256)]))
    return [[pick() for _ in range(n_cols)] for _ in range(1 << log_size)]


def processor_registers(rng, n_rows):
    """n_rows synthetic register rows (clk, ip, ci, ni, mp, mv): clk counts up from 0 as the VM's does, the rest are canonical words with
    zeros among mv."""
    return [[r, rng.randrange(1 << 16), rng.randrange(256), rng.randrange(256), rng.randrange(1 << 16), rng.choice([0, 1, P - 1, rng.randrange(256)])] for r in range(n_rows)]


def processor_table(regs):
    """host/tables.h processor_table restated over those rows: 9 columns clk, ip, ci, ni, mp, mv, mvi, d, next_clk of next_pow2(len) rows."""
    n_real, n = len(regs), 1
    while n < len(regs):
        n *= 2
    last = regs[-1]
    clk_at = lambda r: regs[r][0] if r < n_real else (last[0] + r - n_real + 1) % P
    rows = []
    for r in range(n):
        head = regs[r] + [pow(regs[r][5], P - 2, P), 0] if r < n_real else [clk_at(r), last[1], 0, 0, 0, 0, 0, 1]
        rows.append(head + [clk_at(r + 1) if r + 1 < n else (clk_at(n - 1) + 1) % P])
    return rows
