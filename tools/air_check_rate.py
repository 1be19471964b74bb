#!/usr/bin/env python3
"""What generality costs on the trace domain: bfhip_air_check (one interpreter kernel for every AIR) beside bfhip_check_constraints (13
compiled-in kernels) on the same resident tables, in one run on one GPU.

  python3 tools/air_check_rate.py [--program fib19] [--passes 200] [--rounds 5] [--out FILE]

  tables     the 13 component tables of one execution (fib19, or the synthetic 2^k-row trace with --program sweep20 .. sweep22), row-granular
             in HBM; the logUp columns are bfhip_logup_generate's. Both calls read the same buffers: main columns and the earlier logUp
             columns at shift 4, the last logUp column full size; the program also reads an IsFirst column.
  time       ms per pass: the two calls alternate in windows of `passes` back-to-back calls, `rounds` rounds, and by HIP events
             (tools/ratelib.py has the scheme). Every call ends in its own read-back, so a pass is what a caller waits for.
  check      before the timing: both report a valid trace, with the same counters.

The interpreter is expected to be slower; no threshold is attached. A run without a GPU fails: nothing here is measured on the host."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.benchlib.workloads import FIB19, sweep_program                 # noqa: E402
from ratelib import alternate, cell, emit, events, load_package, require_gpu      # noqa: E402


def measure(pkg, ctx, tr, comp, elems, passes, rounds):
    program, _, columns = pkg.brainfuck_air_program(comp)
    n_main, n_logup = len([c for c in columns if c.startswith("main")]), len([c for c in columns if c.startswith("logup")]) // 4
    log_size = tr.log_sizes[comp]
    n = 1 << log_size
    main = [ctx.upload(tr.column(comp, j)) for j in range(n_main)]
    logup = [ctx.malloc(4 * (n >> 4)) for _ in range(4 * (n_logup - 1))] + [ctx.malloc(4 * n) for _ in range(4)]
    is_first = np.zeros(n, dtype=np.uint32); is_first[0] = 1
    first = ctx.upload(is_first)
    try:
        claimed = ctx.logup_generate(comp, log_size, main, elems, logup)
        params = pkg.brainfuck_air_params(elems, claimed)
        shifts = [4] * (n_main + 4 * (n_logup - 1)) + [0] * 5
        compiled = lambda: ctx.check_constraints(comp, log_size, main, logup, elems, claimed)
        interpreted = lambda: ctx.air_check(program, log_size, main + logup + [first], params, col_shifts=shifts)
        want, got = compiled(), interpreted().as_dict()
        if not (want["ok"] and got["ok"] and got["bad_per_constraint"] == want["bad_per_constraint"][: got["n_constraints"]]):
            raise SystemExit("air_check_rate: component %d is not reported valid by both: %r / %r" % (comp, want, got))

        calls = {"compiled": compiled, "program": interpreted}
        ms = alternate(ctx, calls, passes, rounds)
        ev = {}
        for name, scope in (("compiled", "k_check_cells"), ("program", "k_air_check")):
            gpu_ms, timed = events(ctx, calls[name], passes)[scope]
            ev[name] = gpu_ms / timed
    finally:
        for p in main + logup + [first]:
            ctx.free(p)
    return {"name": pkg.COMPONENT_NAMES[comp], "log_size": log_size, "shape": program.shape, "columns": len(columns), "ms": ms, "events_ms": ev}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--program", default="fib19", choices=["fib19", "sweep20", "sweep21", "sweep22"])
    ap.add_argument("--passes", type=int, default=200); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--out")
    a = ap.parse_args()
    pkg = load_package()
    require_gpu(pkg, "air_check_rate")
    code = FIB19 if a.program == "fib19" else sweep_program(int(a.program[5:]))
    ctx = pkg.Context(0, max_log_domain=26)
    try:
        tr = pkg.Trace(ctx, code)
        try:
            rows = [measure(pkg, ctx, tr, comp, pkg.default_check_lookup(), a.passes, a.rounds) for comp in range(13)]
        finally:
            tr.close()
    finally:
        ctx.close()
    lines = [f"bfhip_air_check (k_air_check_cells + k_air_check_first, the interpreter) beside bfhip_check_constraints (k_check_cells<COMP> + k_check_first<COMP>) on the "
             f"13 tables of {a.program}, a valid trace, row-granular columns at shift 4; {a.rounds} alternating rounds of {a.passes} passes after a warm-up round; "
             f"each pass ends in its read-back; same counters checked first", "",
             "component | log_size | columns | instructions, m / q registers, LDS bytes per wave | compiled ms per pass: median (min-max) | program ms per pass: median (min-max) | "
             "program / compiled | by HIP events: compiled, program ms"]
    for r in rows:
        c, p, s = r["ms"]["compiled"], r["ms"]["program"], r["shape"]
        lines.append(f"{r['name']} | {r['log_size']} | {r['columns']} | {s['n_instr']}, {s['m_regs']} / {s['q_regs']}, {256 * (s['m_regs'] + 4 * s['q_regs'])} | "
                     f"{cell(c, 4)} | {cell(p, 4)} | "
                     f"{statistics.median(p) / statistics.median(c):.2f}x | {r['events_ms']['compiled']:.4f}, {r['events_ms']['program']:.4f}")
    emit("\n".join(lines) + "\n", a.out)


if __name__ == "__main__":
    main()
