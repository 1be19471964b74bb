#!/usr/bin/env python3
"""What run-time compilation buys: a constraint program as its own kernel (bfhip_air_compile / bfhip_air_kernel_eval_domain) beside the
interpreter (bfhip_air_eval_domain) and the built-in per-component kernels (bfhip_eval_constraints) on the same columns, in one run on one GPU.

  python3 tools/air_compiled_rate.py [--log-size 20] [--components 0,3] [--launches 500] [--rounds 5] [--out profiles/air_compiled_rate.txt]

  columns    full size (shift 0: bfhip_eval_constraints then takes its per-row kernel, one lane per row like the other two), splitmix values;
             the constraint domain is CanonicCoset(log_size + 1). All three calls accumulate into four coordinate columns.
  time       ms per launch: the three kernels alternate in windows of `launches` back-to-back calls, `rounds` rounds, and by HIP events
             (tools/ratelib.py has the scheme).
  check      before the timing: from the same starting accumulator the three calls leave the same bytes.
  compile    once, for each of the 13 programs: generate + compile + load time and bfhip_air_kernel_info's figures.

No threshold is attached. A run without a GPU fails: nothing here is measured on the host."""
import argparse
import statistics

import numpy as np

from ratelib import alternate, cell, emit, events, load_package, require_gpu, splitmix_column

KINDS = ("builtin", "interpreter", "compiled")
SCOPES = {"builtin": "k_constraints", "interpreter": "k_air_program", "compiled": "bfhip_air_generated"}


def measure(pkg, ctx, comp, log_size, launches, rounds):
    program, _, columns = pkg.brainfuck_air_program(comp)
    kernel = ctx.air_compile(program)
    n_main, n_logup = len([c for c in columns if c.startswith("main")]), len([c for c in columns if c.startswith("logup")]) // 4
    n = 2 << log_size
    elems = [int(v) or 1 for v in splitmix_column(77, 24)]
    claimed = splitmix_column(78, 4).tolist()
    n_cons = program.shape["n_constraints"]
    coeffs = splitmix_column(500 + comp, 4 * n_cons)
    quads = coeffs.reshape(n_cons, 4).tolist()
    params = pkg.brainfuck_air_params(elems, claimed)
    cols = [ctx.upload(splitmix_column(1000 + 16 * comp + k, n)) for k in range(len(columns))]
    zero = np.zeros(n, dtype=np.uint32)
    accs = {k: [ctx.upload(zero) for _ in range(4)] for k in KINDS}
    main, inter, first = cols[:n_main], cols[n_main: n_main + 4 * n_logup], cols[-1]
    calls = {"builtin": lambda acc: ctx.eval_constraints(comp, log_size, first, main, inter, elems, claimed, coeffs, acc),
             "interpreter": lambda acc: ctx.air_eval_domain(program, log_size, 1, cols, params, quads, acc),
             "compiled": lambda acc: ctx.air_eval_domain(kernel, log_size, 1, cols, params, quads, acc)}
    try:
        for k in KINDS:
            calls[k](accs[k])
        got = {k: [ctx.download(p, n) for p in accs[k]] for k in KINDS}
        if not all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(*[got[k] for k in KINDS])):
            raise SystemExit("air_compiled_rate: the three kernels disagree on component %d" % comp)

        timed = {k: (lambda k=k: calls[k](accs["builtin"])) for k in KINDS}
        ms = alternate(ctx, timed, launches, rounds)
        ev = {}
        for k in KINDS:
            gpu_ms, n_timed = events(ctx, timed[k], launches)[SCOPES[k]]
            ev[k] = gpu_ms / n_timed
    finally:
        kernel.close()
        for p in cols + [p for k in KINDS for p in accs[k]]:
            ctx.free(p)
    return {"component": comp, "name": pkg.COMPONENT_NAMES[comp], "shape": program.shape, "columns": len(columns), "ms": ms, "events_ms": ev}


def compile_report(pkg, ctx):
    lines = ["program | instructions, m / q registers | compile ms (generate + hiprtc + load) | VGPRs | SGPRs | scratch bytes per lane | LDS bytes | code object bytes | source bytes"]
    for comp in range(13):
        program = pkg.brainfuck_air_program(comp)[0]
        with ctx.air_compile(program) as kernel:
            i, s = kernel.info(), program.shape
        assert not i["from_cache"]
        lines.append(f"{pkg.COMPONENT_NAMES[comp]} | {s['n_instr']}, {s['m_regs']} / {s['q_regs']} | {i['compile_us'] / 1e3:.1f} | {i['vgprs']} | {i['sgprs']} | "
                     f"{i['scratch_bytes']} | {i['lds_bytes']} | {i['code_object_bytes']} | {i['source_bytes']}")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log-size", type=int, default=20); ap.add_argument("--components", default="0,3")
    ap.add_argument("--launches", type=int, default=500); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--out")
    a = ap.parse_args()
    pkg = load_package()
    require_gpu(pkg, "air_compiled_rate")
    ctx = pkg.Context(0, max_log_domain=a.log_size + 1)
    try:
        compiled = compile_report(pkg, ctx)      # first: the first compile of the process also loads libhiprtc and its compiler
        rows = [measure(pkg, ctx, int(c), a.log_size, a.launches, a.rounds) for c in a.components.split(",")]
    finally:
        ctx.close()
    lines = [f"bfhip_air_kernel_eval_domain (a kernel compiled at run time from brainfuck_air_program(k)) beside bfhip_air_eval_domain (k_air_program, the interpreter) and "
             f"bfhip_eval_constraints (k_constraints<COMP>, per-row kernel) at log_size {a.log_size}: 2^{a.log_size + 1} rows, full-size columns; {a.rounds} alternating rounds of "
             f"{a.launches} launches after a warm-up round; same bytes checked first", "",
             "component | columns | ms per launch, median (min-max): built-in | interpreter | compiled | interpreter / compiled | compiled / built-in | by HIP events: built-in, interpreter, compiled ms"]
    for r in rows:
        med = {k: statistics.median(r["ms"][k]) for k in KINDS}
        lines.append(f"{r['name']} | {r['columns']} | {cell(r['ms']['builtin'], 4)} | {cell(r['ms']['interpreter'], 4)} | {cell(r['ms']['compiled'], 4)} | {med['interpreter'] / med['compiled']:.2f}x | "
                     f"{med['compiled'] / med['builtin']:.2f}x | {r['events_ms']['builtin']:.4f}, {r['events_ms']['interpreter']:.4f}, {r['events_ms']['compiled']:.4f}")
    lines += ["", "compiled once each, in this process (the first line includes loading libhiprtc and its compiler):"] + compiled
    emit("\n".join(lines) + "\n", a.out)


if __name__ == "__main__":
    main()
