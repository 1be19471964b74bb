#!/usr/bin/env python3
"""What deriving a table's dependent columns on the device saves: the Processor witness program (brainfuck_witness_program("processor"): 9
columns from the 6 register columns) beside the route it replaces and beside a copy of the same bytes. In one run on one GPU.

  python3 tools/witness_program_rate.py [--passes 5] [--rounds 5] [--small] [--out FILE]

  cases      2^20 and 2^24 rows of synthetic canonical registers (clk counts up from 0, mv holds zeros), 2^log - 3 of them real so that
             the padding path runs. --small: 2^12 and 2^16 rows (a dry run).
  device     (a) the register table (host, row-major, n_real x 6) uploaded and ingested with repeat_last (bfhip_columns_from_rows), then
             bfhip_witness_program_generate into resident columns, then a wait for the stream. `resident` is the same without the upload:
             the registers already in HBM.
  host       (b) the 9 columns derived with numpy (the inverse by square-and-multiply over uint64 arrays: numpy has no modular inverse),
             the n x 9 table uploaded and ingested. Pageable numpy memory, one host thread. One call per window (it is long).
  copy       (c) hipMemcpyAsync device to device, then a wait for the device, of HALF the bytes the kernel reads and writes (6 + 9 columns:
             a copy reads and writes every byte it moves, so it moves the kernel's 15 words per row). The second read of clk (offset +1) is
             not counted.
  time       ms per call: the paths alternate in windows, `rounds` rounds (at least five) after a warm-up round (tools/ratelib.py). GPU time
             by HIP events (the library's profiler): scopes k_columns_from_rows and k_witness_program of the resident route.
  check      before the timing: the device route's 9 columns equal the ingested numpy table, byte for byte.

No threshold is attached. A run without a GPU fails: nothing here is measured on the host alone."""
import argparse
import ctypes
import statistics

import numpy as np

from ratelib import alternate, cell, emit, events, load_package, require_gpu

P = (1 << 31) - 1
D2D = 3      # hipMemcpyDeviceToDevice


def registers(n_real):
    rng = np.random.default_rng(n_real)
    regs = rng.integers(0, 1 << 16, size=(n_real, 6), dtype=np.uint32)
    regs[:, 0] = np.arange(n_real, dtype=np.uint32)
    regs[:, 5] = np.where(rng.integers(0, 4, size=n_real) == 0, 0, rng.integers(0, P, size=n_real)).astype(np.uint32)
    return regs


def inverse(x):
    """x^(p - 2) over a uint64 array, 0 for 0"""
    x = x.astype(np.uint64)
    r = np.ones_like(x)
    for bit in bin(P - 2)[2:]:
        r = r * r % P
        if bit == "1":
            r = r * x % P
    return r


def processor_numpy(regs, log_size):
    """host/tables.h processor_table over the register rows, as a (2^log_size, 9) uint32 table"""
    n_real, n = regs.shape[0], 1 << log_size
    t = np.zeros((n, 9), dtype=np.uint32)
    t[:n_real, :6] = regs
    t[:n_real, 6] = inverse(regs[:, 5])
    pad = np.arange(n - n_real, dtype=np.uint64)
    t[n_real:, 0] = (int(regs[-1, 0]) + 1 + pad) % P
    t[n_real:, 1] = regs[-1, 1]
    t[n_real:, 7] = 1
    t[:-1, 8] = t[1:, 0]
    t[-1, 8] = (int(t[-1, 0]) + 1) % P
    return t


def measure(pkg, ctx, hip, a, log_size):
    n = 1 << log_size
    n_real = n - 3
    regs = registers(n_real)
    prog = pkg.brainfuck_witness_program("processor")[0]
    ptrs = []
    try:
        ins = [ctx.malloc(4 * n) for _ in range(6)]; ptrs += ins
        outs = [ctx.malloc(4 * n) for _ in range(9)]; ptrs += outs
        host_cols = [ctx.malloc(4 * n) for _ in range(9)]; ptrs += host_cols
        copy_bytes = 4 * n * 15 // 2
        copy_src, copy_dst = ctx.malloc(copy_bytes), ctx.malloc(copy_bytes); ptrs += [copy_src, copy_dst]
        resident_regs = ctx.upload(regs); ptrs.append(resident_regs)
        resident_table = pkg.DeviceRows(resident_regs, n_real, 6, 6)

        def derive(table):
            ctx.columns_from_rows(table, log_size, repeat_last=True, out=ins)
            ctx.witness_program_generate(prog, log_size, ins, [n_real], out=outs)
            ctx.sync()

        device = lambda: derive(regs)
        resident = lambda: derive(resident_table)

        def host():
            ctx.columns_from_rows(processor_numpy(regs, log_size), log_size, out=host_cols)

        def copy():
            assert hip.hipMemcpyAsync(ctypes.c_void_p(copy_dst), ctypes.c_void_p(copy_src), ctypes.c_size_t(copy_bytes), D2D, None) == 0
            assert hip.hipDeviceSynchronize() == 0

        device()
        host()
        for k, (p, q) in enumerate(zip(outs, host_cols)):
            if ctx.download(p, n).tobytes() != ctx.download(q, n).tobytes():
                raise SystemExit("witness_program_rate: the device route and the numpy route disagree in column %d at 2^%d" % (k, log_size))
        ms = alternate(ctx, {"device": device, "resident": resident, "copy": copy}, a.passes, a.rounds)
        ms.update(alternate(ctx, {"host": host}, 1, a.rounds))
        ev = events(ctx, resident, a.passes)
        return ms, ev["k_columns_from_rows"][0], ev["k_witness_program"][0]
    finally:
        for p in ptrs:
            ctx.free(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=5); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--small", action="store_true"); ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("witness_program_rate: at least five rounds")
    pkg = load_package()
    require_gpu(pkg, "witness_program_rate")
    hip = ctypes.CDLL("libamdhip64.so")
    ctx = pkg.Context(0, max_log_domain=16 if a.small else 24)
    lines = [f"The Processor witness program (9 columns from 6 register columns, 2^log - 3 real rows): (a) device = upload of the n x 6 register table, "
             f"bfhip_columns_from_rows with repeat_last, bfhip_witness_program_generate, a wait for the stream; resident = the same with the registers already "
             f"in HBM; (b) host = numpy derivation of the 9 columns, upload of the n x 9 table, ingest; (c) copy = a device-to-device copy moving the "
             f"kernel's 15 words per row (7.5 read, 7.5 written). {a.rounds} alternating rounds of {a.passes} calls (host: 1 call) after a warm-up round, the "
             f"context synchronised around every window; equal bytes (device = host route) checked first.", "",
             "case | path | ms per call: median (min-max)"]
    try:
        for log_size in ((12, 16) if a.small else (20, 24)):
            ms, ev_ingest, ev_kernel = measure(pkg, ctx, hip, a, log_size)
            med = {k: statistics.median(v) for k, v in ms.items()}
            name = "2^%d rows" % log_size
            for path in ("device", "resident", "host", "copy"):
                lines.append(f"{name} | {path} | {cell(ms[path], 4)}")
            traffic = 4.0 * 15 * (1 << log_size)
            lines += [f"{name} | by HIP events (resident route) | k_columns_from_rows {ev_ingest:.4f} ms, k_witness_program {ev_kernel:.4f} ms = "
                      f"{traffic / ev_kernel / 1e6:.0f} GB/s over 15 words per row",
                      f"{name} | k_witness_program / copy | {ev_kernel / med['copy']:.2f}x",
                      f"{name} | host / device (median ms) | {med['host'] / med['device']:.1f}x; host / resident {med['host'] / med['resident']:.1f}x", ""]
    finally:
        ctx.close()
    lines += ["Measured: one MI355X (gfx950), one process, one run of `python3 tools/witness_program_rate.py`; the Processor program only (43 instructions, 7 registers,",
              "one INV0, one read at offset +1), these two sizes, synthetic registers.",
              "Not measured: other programs, other sizes, the call inside an open commitment-scheme session, other boxes, the spread from run to run, hardware counters.", ""]
    emit("\n".join(lines), a.out)


if __name__ == "__main__":
    main()
