#!/usr/bin/env python3
"""What generality costs: the constraint-program kernel (bfhip_air_eval_domain, one interpreter for every AIR) beside the compiled
per-component kernels (bfhip_eval_constraints) on the same columns, in one run on one GPU.

  python3 tools/air_program_rate.py [--log-size 20] [--components 0,3] [--launches 500] [--rounds 5] [--out profiles/air_program_rate.txt]

  columns    full size (shift 0: bfhip_eval_constraints then takes its per-row kernel, one lane per row like the interpreter), splitmix values;
             the constraint domain is CanonicCoset(log_size + 1). Both calls accumulate into the same four coordinate columns.
  time       ms per launch: the two kernels alternate in windows of `launches` back-to-back calls, `rounds` rounds, and by HIP events
             (tools/ratelib.py has the scheme).
  check      before the timing: from the same starting accumulator the two calls leave the same bytes.

The interpreter is expected to be slower; no threshold is attached. A run without a GPU fails: nothing here is measured on the host."""
import argparse
import statistics

import numpy as np

from ratelib import alternate, cell, emit, events, load_package, require_gpu, splitmix_column


def measure(pkg, ctx, comp, log_size, launches, rounds):
    program, _, columns = pkg.brainfuck_air_program(comp)
    n_main, n_logup = len([c for c in columns if c.startswith("main")]), len([c for c in columns if c.startswith("logup")]) // 4
    n = 2 << log_size
    elems = [int(v) or 1 for v in splitmix_column(77, 24)]
    claimed = splitmix_column(78, 4).tolist()
    n_cons = program.shape["n_constraints"]
    coeffs = splitmix_column(500 + comp, 4 * n_cons)
    params = pkg.brainfuck_air_params(elems, claimed)
    cols = [ctx.upload(splitmix_column(1000 + 16 * comp + k, n)) for k in range(len(columns))]
    zero = np.zeros(n, dtype=np.uint32)
    acc_a, acc_b = [ctx.upload(zero) for _ in range(4)], [ctx.upload(zero) for _ in range(4)]
    main, inter, first = cols[:n_main], cols[n_main: n_main + 4 * n_logup], cols[-1]
    compiled = lambda acc=acc_a: ctx.eval_constraints(comp, log_size, first, main, inter, elems, claimed, coeffs, acc)
    interpreted = lambda acc=acc_a: ctx.air_eval_domain(program, log_size, 1, cols, params, coeffs.reshape(n_cons, 4).tolist(), acc)
    try:
        compiled(); interpreted(acc_b)
        same = all(np.array_equal(ctx.download(a, n), ctx.download(b, n)) for a, b in zip(acc_a, acc_b))
        if not same:
            raise SystemExit("air_program_rate: the two kernels disagree on component %d" % comp)

        calls = {"compiled": compiled, "program": interpreted}
        ms = alternate(ctx, calls, launches, rounds)
        ev = {}
        for name, scope in (("compiled", "k_constraints"), ("program", "k_air_program")):
            gpu_ms, timed = events(ctx, calls[name], launches)[scope]
            ev[name] = gpu_ms / timed
    finally:
        for p in cols + acc_a + acc_b:
            ctx.free(p)
    return {"component": comp, "name": pkg.COMPONENT_NAMES[comp], "shape": program.shape, "columns": len(columns), "ms": ms, "events_ms": ev}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log-size", type=int, default=20); ap.add_argument("--components", default="0,3")
    ap.add_argument("--launches", type=int, default=500); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--out")
    a = ap.parse_args()
    pkg = load_package()
    require_gpu(pkg, "air_program_rate")
    ctx = pkg.Context(0, max_log_domain=a.log_size + 1)
    try:
        rows = [measure(pkg, ctx, int(c), a.log_size, a.launches, a.rounds) for c in a.components.split(",")]
    finally:
        ctx.close()
    lines = [f"bfhip_air_eval_domain (k_air_program, the interpreter) beside bfhip_eval_constraints (k_constraints<COMP>, per-row kernel) at log_size {a.log_size}: "
             f"2^{a.log_size + 1} rows, full-size columns; {a.rounds} alternating rounds of {a.launches} launches after a warm-up round; same bytes checked first", "",
             "component | columns | instructions, m / q registers, LDS bytes per wave | compiled ms per launch: median (min-max) | program ms per launch: median (min-max) | "
             "program / compiled | by HIP events: compiled, program ms"]
    for r in rows:
        c, p, s = r["ms"]["compiled"], r["ms"]["program"], r["shape"]
        lines.append(f"{r['name']} | {r['columns']} | {s['n_instr']}, {s['m_regs']} / {s['q_regs']}, {256 * (s['m_regs'] + 4 * s['q_regs'])} | "
                     f"{cell(c, 4)} | {cell(p, 4)} | "
                     f"{statistics.median(p) / statistics.median(c):.2f}x | {r['events_ms']['compiled']:.4f}, {r['events_ms']['program']:.4f}")
    emit("\n".join(lines) + "\n", a.out)


if __name__ == "__main__":
    main()
