"""-m gpu: register rows as the caller holds them (n x 7 u32, row-major) -> the prover's tables, through the device-side ingestion
(csrc/ingest.hip: one upload, one launch that transposes 256-row tiles through LDS and checks every word against 2^31 - 1).
bfhip_trace_create_from_registers goes through it with the GPU table builder on (the default) and must not move: same tables, same
log_sizes, same error texts. bfhip_prove_registers is prove_brainfuck(&Machine) (mod.rs:471-473) in one call: the bytes of
Trace.from_registers(...).prove(...) and of the CPU oracle, and a non-canonical register named with its (row, register)."""
import ctypes

import numpy as np
import pytest

from test_gpu_pool import MIXED

pytestmark = pytest.mark.gpu

P = (1 << 31) - 1
CODE, INPUT = "+++>,<[>+.<-]", b"\x01"
# one row; a partial tile; around the 64-lane wave; around the 256-row tile; around two tiles; many tiles + 1
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 4097]
N_MAIN = (8, 8, 4, 9, 13, 13, 11, 11, 11, 11, 11, 11, 7)      # csrc/air.h: n_main_cols


@pytest.fixture(scope="module")
def machine(pkg):
    """The executed machine of CODE: its register rows (the last one is the ci = 0 row) and program words."""
    _, rows = pkg.host_run(CODE, INPUT)
    assert rows.shape == (26, 7) and rows[-1, 2] == 0 and np.count_nonzero(rows[:, 2] == 0) == 1
    return rows, pkg.host_compile(CODE)


def make_rows(base, n):
    """base repeated and truncated to n rows with clk renumbered; the one ci = 0 row stays the last (the EndOfExecution table wants exactly one)."""
    body = base[:-1]
    reps = -(-(n - 1) // len(body))
    rows = np.concatenate([np.tile(body, (reps, 1))[: n - 1], base[-1:]]) if n > 1 else base[-1:].copy()
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    rows[:, 0] = np.arange(n, dtype=np.uint32)
    return rows


def host_tables(pkg, rows, words):
    """bfhip_host_table for the 13 components: [(n_rows, n_cols) array] — or the library's error text if a builder refuses the rows."""
    L = pkg.lib()
    words = np.ascontiguousarray(words, dtype=np.uint32)
    out = []
    for comp in range(13):
        nr, nc = ctypes.c_size_t(), ctypes.c_size_t()
        args = (rows.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(rows.shape[0]), words.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(words.size), comp)
        if L.bfhip_host_table(*args, None, ctypes.c_size_t(0), ctypes.byref(nr), ctypes.byref(nc)) != 0:
            return L.bfhip_last_error().decode()
        t = np.zeros((nr.value, nc.value), dtype=np.uint32)
        assert L.bfhip_host_table(*args, t.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(t.size), ctypes.byref(nr), ctypes.byref(nc)) == 0
        out.append(t)
    return out


@pytest.fixture(scope="module")
def expected(pkg, machine):
    """(n, saturated) -> (rows, host tables or error text): computed once, shared, never modified."""
    base, words = machine
    out = {}
    for n in SIZES:
        for saturated in (False, True):
            rows = make_rows(base, n)
            if saturated:
                rows[max(n - 2, 0), :] = P - 1          # every register of one row at the largest canonical value (n = 1: the only row)
            rows.setflags(write=False)
            out[(n, saturated)] = (rows, host_tables(pkg, rows, words))
    return out


@pytest.mark.single_conv
@pytest.mark.parametrize("saturated", [False, True], ids=["vm_values", "one_row_at_p_minus_1"])
@pytest.mark.parametrize("n", SIZES)
def test_tables_from_ingested_rows_equal_the_host_tables(pkg, ctx, machine, expected, n, saturated):
    rows, want = expected[(n, saturated)]
    if isinstance(want, str):                               # n = 1 saturated: no ci = 0 row is left — both builders refuse alike
        assert want == "InvalidEndOfExecution"
        with pytest.raises(pkg.BfhipError, match="^InvalidEndOfExecution$"):
            pkg.Trace.from_registers(ctx, rows, machine[1])
        return
    t = pkg.Trace.from_registers(ctx, rows, machine[1])
    try:
        assert t.log_sizes == [int(np.log2(w.shape[0])) + 4 for w in want]
        for comp in range(13):
            assert want[comp].shape[1] == N_MAIN[comp]
            for col in range(N_MAIN[comp]):
                got = t.column(comp, col)
                assert np.array_equal(got, want[comp][:, col]), f"n={n}: component {comp} column {col} differs from bfhip_host_table"
    finally:
        t.close()


@pytest.mark.single_conv
def test_non_canonical_registers_are_named_by_row_and_register(pkg, ctx, machine):
    """p and 2^32 - 1 in the first row, the last row, the last row of a full tile and the first row of the next tile, each register in turn:
    bfhip_prove_registers names the place, bfhip_trace_create_from_registers keeps its text byte for byte."""
    base, words = machine
    n = 513
    good = make_rows(base, n)
    old_text = "^register value is not a canonical M31$"
    for row in (0, 255, 256, n - 1):
        for reg in range(7):
            for value in (P, 0xFFFFFFFF):
                bad = good.copy()
                bad[row, reg] = value
                with pytest.raises(pkg.BfhipError, match=r"^register value is not a canonical M31 \(row %d, register %d\)$" % (row, reg)):
                    pkg.prove_registers(bad, words, ctx=ctx, log_max_rows=14)
                with pytest.raises(pkg.BfhipError, match=old_text):
                    pkg.Trace.from_registers(ctx, bad, words)
    # two bad words at once: the lowest (row, register) wins — across a tile boundary, and within one row
    for places, first in ((((256, 3), (255, 5)), (255, 5)), (((512, 6), (512, 2)), (512, 2)), (((300, 0), (0, 6)), (0, 6))):
        bad = good.copy()
        for (row, reg), value in zip(places, (P, 0xFFFFFFFF)):
            bad[row, reg] = value
        with pytest.raises(pkg.BfhipError, match=r"\(row %d, register %d\)$" % first):
            pkg.prove_registers(bad, words, ctx=ctx, log_max_rows=14)
        with pytest.raises(pkg.BfhipError, match=old_text):
            pkg.Trace.from_registers(ctx, bad, words)
    # which error wins (bfhip_trace_create_from_registers as before): no rows, then no program, then a bad register, then a bad program word
    bad = good.copy(); bad[7, 1] = P
    bad_words = np.array(words, dtype=np.uint32); bad_words[0] = P
    for entry in (lambda r, w: pkg.Trace.from_registers(ctx, r, w), lambda r, w: pkg.prove_registers(r, w, ctx=ctx, log_max_rows=14)):
        with pytest.raises(pkg.BfhipError, match="^EmptyTrace$"):
            entry(good[:0], words[:0])
        with pytest.raises(pkg.BfhipError, match="^empty program$"):
            entry(bad, words[:0])
        with pytest.raises(pkg.BfhipError, match="^register value is not a canonical M31"):
            entry(bad, bad_words)
        with pytest.raises(pkg.BfhipError, match="^program word is not a canonical M31$"):
            entry(good, bad_words)
    # the host table builder keeps the host path, place included for the one-call entry
    ctx.set_table_builder(False)
    try:
        with pytest.raises(pkg.BfhipError, match=r"^register value is not a canonical M31 \(row 7, register 1\)$"):
            pkg.prove_registers(bad, words, ctx=ctx, log_max_rows=14)
        with pytest.raises(pkg.BfhipError, match=old_text):
            pkg.Trace.from_registers(ctx, bad, words)
    finally:
        ctx.set_table_builder(True)
    # and the context proves as before (the executed machine itself: the repeated rows above are no valid execution)
    t = pkg.Trace.from_registers(ctx, base, words)
    try:
        assert pkg.prove_registers(base, words, ctx=ctx, log_max_rows=14) == t.prove(14)[0]
    finally:
        t.close()


@pytest.fixture(scope="module")
def oracle_proofs():
    return {}


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_prove_registers_equals_the_two_call_path_and_the_oracle(pkg, oracle, ctx, conv, oracle_proofs, which):
    code, inp = MIXED[which]
    lmr = 16
    if (conv, which) not in oracle_proofs:
        oracle_proofs[(conv, which)] = oracle.prove(code, inp, log_max_rows=lmr)[:2]
    want, want_taps = oracle_proofs[(conv, which)]
    _, rows = oracle.run(code, inp)
    words = oracle.compile(code)
    proof, taps = pkg.prove_registers(rows, words, ctx=ctx, log_max_rows=lmr, with_transcript=True)
    t = pkg.Trace.from_registers(ctx, rows, words)
    try:
        two_calls = t.prove(lmr)[0]
    finally:
        t.close()
    assert proof == two_calls, "bfhip_prove_registers differs from bfhip_trace_create_from_registers + bfhip_prove_trace"
    assert proof == want, "bfhip_prove_registers differs from the CPU oracle"
    diverged = next((k for k in want_taps if want_taps[k] != taps.get(k)), None)
    assert diverged is None, f"the transcript diverges from the oracle's at {diverged}"
    # the host table builder gives the same bytes through the same entry
    ctx.set_table_builder(False)
    try:
        assert pkg.prove_registers(rows, words, ctx=ctx, log_max_rows=lmr) == want
    finally:
        ctx.set_table_builder(True)
