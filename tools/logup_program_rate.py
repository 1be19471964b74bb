#!/usr/bin/env python3
"""What generality costs: the fraction-program path (bfhip_logup_program_generate, one interpreter and a scan over distinct cells for every
AIR) beside the compiled, replication-aware path (bfhip_logup_generate) on the same tables, in one run on one GPU.

  python3 tools/logup_program_rate.py [--log-size 20] [--components 0,3] [--calls 50] [--rounds 5] [--out profiles/logup_program_rate.txt] [--note TEXT] [--append]

  tables     row-granular main columns of 2^(log_size - 4) rows, splitmix values. bfhip_logup_generate reads them as rows;
             bfhip_logup_program_generate reads them at shift 4 and writes every logUp column full size. A third row per component runs the
             same program on full-size columns of 2^log_size distinct cells (shift 0), which has no compiled counterpart.
  time       ms per call: the paths alternate in windows of `calls` back-to-back calls, `rounds` windows each (each call allocates its
             scratch, launches, reads its claimed sum back and frees: a call returns with the GPU idle), and cells per second =
             2^log_size / median; the row stage and the scan stage by HIP events (tools/ratelib.py has the scheme).
  check      before the timing: the program's earlier columns are the 16-fold broadcast of the compiled path's, the last column and the
             claimed sum are equal.

The generic path scans 16 times the entries and writes 16 times the cells of the replicated one; no threshold is attached. A run without
a GPU fails: nothing here is measured on the host."""
import argparse
import statistics

import numpy as np

from ratelib import alternate, cell, emit, events, load_package, require_gpu, splitmix_column


def measure(pkg, ctx, comp, log_size, calls, rounds):
    program, _ = pkg.brainfuck_logup_program(comp)
    n_main, n_logup = program.shape["n_cols"], program.shape["n_logup_cols"]
    n, M = 1 << log_size, 1 << (log_size - 4)
    elems = [int(v) or 1 for v in splitmix_column(77, 24)]
    params = pkg.brainfuck_air_params(elems, [0, 0, 0, 0])[:24]
    rows = [ctx.upload(splitmix_column((1000 + 16 * comp + k) << 32, M)) for k in range(n_main)]
    full = [ctx.upload(splitmix_column((2000 + 16 * comp + k) << 32, n)) for k in range(n_main)]
    sizes = [M] * (4 * (n_logup - 1)) + [n] * 4
    out_c, out_p = [ctx.malloc(4 * s) for s in sizes], [ctx.malloc(4 * n) for _ in range(4 * n_logup)]
    compiled = lambda: ctx.logup_generate(comp, log_size, rows, elems, out_c)
    shifted = lambda: ctx.logup_program_generate(program, log_size, rows, params, out_p, col_shifts=[4] * n_main)
    distinct = lambda: ctx.logup_program_generate(program, log_size, full, params, out_p)
    try:
        same = compiled() == shifted() and all(np.array_equal(np.repeat(ctx.download(a, s), n // s), ctx.download(b, n)) for a, b, s in zip(out_c, out_p, sizes))
        if not same:
            raise SystemExit("logup_program_rate: the two paths disagree on component %d" % comp)

        paths = {"compiled": compiled, "program": shifted, "distinct": distinct}
        ms = alternate(ctx, paths, calls, rounds)
        # GPU time of the two stages, per timed scope
        ev = {}
        for name in ("program", "distinct"):
            rep = events(ctx, paths[name], calls)
            ev[name] = tuple(rep[k][0] / rep[k][1] for k in ("k_logup_program", "k_logup_program_scan"))
    finally:
        for p in rows + full + out_c + out_p:
            ctx.free(p)
    return {"component": comp, "name": pkg.COMPONENT_NAMES[comp], "shape": program.shape, "ms": ms, "events_ms": ev}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log-size", type=int, default=20); ap.add_argument("--components", default="0,3")
    ap.add_argument("--calls", type=int, default=50); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--out")
    ap.add_argument("--note", default="", help="a line put in front of the table (which variant of the kernels was built)")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    a = ap.parse_args()
    pkg = load_package()
    require_gpu(pkg, "logup_program_rate")
    ctx = pkg.Context(0, max_log_domain=a.log_size + 1)
    try:
        rows = [measure(pkg, ctx, int(c), a.log_size, a.calls, a.rounds) for c in a.components.split(",")]
    finally:
        ctx.close()
    n = 1 << a.log_size
    lines = ([a.note] if a.note else []) + [
        f"bfhip_logup_program_generate (k_logup_program + the coset-order scan over 2^{a.log_size} distinct cells) beside bfhip_logup_generate (k_logup_rows + the "
        f"scan over 2^{a.log_size - 4} replicated rows) at log_size {a.log_size}; {a.rounds} alternating windows of {a.calls} calls after a warm-up round; same bytes checked first", "",
        "component | logUp columns, instructions, m / q registers | path | ms per call: median (min-max) | 10^6 cells per second | over compiled | "
        "by HIP events: row stage, scan stage (3 launches) ms"]
    for r in rows:
        s, c = r["shape"], statistics.median(r["ms"]["compiled"])
        for path, what in (("compiled", "bfhip_logup_generate, rows"), ("program", "program, the same rows at shift 4"), ("distinct", "program, full-size distinct cells")):
            v = r["ms"][path]
            lines.append(f"{r['name']} | {s['n_logup_cols']}, {s['n_instr']}, {s['m_regs']} / {s['q_regs']} | {what} | {cell(v, 4)} | "
                         f"{n / statistics.median(v) / 1e3:.1f} | {statistics.median(v) / c:.2f}x | " + ("%.4f, %.4f" % r["events_ms"][path] if path in r["events_ms"] else "-"))
    emit("\n".join(lines) + "\n", a.out, a.append)


if __name__ == "__main__":
    main()
