#!/usr/bin/env python3
"""What generality costs in the relation tracker: bfhip_relation_program_summary (one interpreter kernel for every AIR's add_to_relation
calls) beside bfhip_trace_relations (the three compiled-in Brainfuck relations) on the same resident trace, in one run on one GPU.

  python3 tools/relation_program_rate.py [--program fib19] [--passes 20] [--rounds 5] [--out FILE]

  tables     the 13 component tables of one execution (fib19, or the synthetic 2^k-row trace with --program sweep20 .. sweep22), row-granular
             in HBM. The compiled call reads the resident trace's own columns; the 13 brainfuck_relation_programs read copies of the same
             columns at row_shift 4 (one word per table row, NULL column shifts). Sort, segments, reduction and report are the same launches
             (relation_aggregate) in both: what differs is the extraction.
  time       ms per pass: the two calls alternate in windows of `passes` back-to-back calls, `rounds` rounds (at least five), and by HIP
             events (tools/ratelib.py has the scheme); every call ends in its own read-backs, so a pass is what a caller waits for. By
             events also the extraction launches alone: relations_extract (k_rel_flags + scan; k_rel_emit is timed inside relations_sort)
             against relation_program_count + relation_program_emit (both interpreter launches per table and relation, and the scan).
  check      before the timing: both give the same three reports and the same entries.

The interpreter is expected to be slower; no threshold is attached. A run without a GPU fails: nothing here is measured on the host."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.benchlib.workloads import FIB19, sweep_program                 # noqa: E402
from ratelib import alternate, cell, emit, events, load_package, require_gpu      # noqa: E402

N_MAIN = (8, 8, 4, 9, 13, 13, 11, 11, 11, 11, 11, 11, 7)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--program", default="fib19", choices=["fib19", "sweep20", "sweep21", "sweep22"])
    ap.add_argument("--passes", type=int, default=20); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("relation_program_rate: at least five rounds")
    pkg = load_package()
    require_gpu(pkg, "relation_program_rate")
    code = FIB19 if a.program == "fib19" else sweep_program(int(a.program[5:]))
    ctx = pkg.Context(0, max_log_domain=26)
    ptrs = []
    try:
        tr = pkg.Trace(ctx, code)
        try:
            programs = [pkg.brainfuck_relation_program(k)[0] for k in range(13)]
            tables = []
            for k in range(13):
                cols = [ctx.upload(tr.column(k, j)) for j in range(N_MAIN[k])]
                ptrs += cols
                tables.append((programs[k], tr.log_sizes[k], 4, cols))
            compiled = lambda: tr.relations(4)
            interpreted = lambda: ctx.relation_program_summary(tables, max_entries=4, relation_names=pkg.RELATION_NAMES, table_names=pkg.COMPONENT_NAMES)
            want, got = compiled(), interpreted()
            if not (got.reports == want.reports and got.entries == want.entries):
                raise SystemExit("relation_program_rate: the two paths disagree: %r / %r" % (want.reports, got.reports))

            calls = {"compiled": compiled, "program": interpreted}
            ms = alternate(ctx, calls, a.passes, a.rounds)
            ev = {}
            for name, scopes in (("compiled", ("relations_extract",)), ("program", ("relation_program_count", "relation_program_emit"))):
                rep = events(ctx, calls[name], a.passes)
                ev[name] = {s: rep[s][0] for s in scopes}
                ev[name]["all"] = sum(t for t, _ in rep.values())
            reports, log_sizes = want.reports, list(tr.log_sizes)
        finally:
            tr.close()
    finally:
        for p in ptrs:
            ctx.free(p)
        ctx.close()
    c, p = ms["compiled"], ms["program"]
    shapes = [q.shape for q in programs]
    ext_c, ext_p = ev["compiled"]["relations_extract"], ev["program"]["relation_program_count"] + ev["program"]["relation_program_emit"]
    lines = [f"bfhip_relation_program_summary (k_relation_program, the interpreter: 13 brainfuck_relation_programs at row_shift 4) beside bfhip_trace_relations "
             f"(k_rel_flags + k_rel_emit, compiled) on the 13 tables of {a.program}, a balanced trace, row-granular columns resident in HBM; {a.rounds} alternating "
             f"rounds of {a.passes} passes after a warm-up round, the context synchronised around every window; each pass ends in its read-backs; same reports and "
             f"entries checked first", "",
             f"table log sizes: {log_sizes}",
             f"entries per relation (memory, instruction, processor): {[r['n_entries'] for r in reports]}; distinct tuples: {[r['n_tuples'] for r in reports]}",
             f"programs: {sum(s['n_instr'] for s in shapes)} instructions in all, at most {max(s['m_regs'] for s in shapes)} m registers "
             f"({256 * max(s['m_regs'] for s in shapes)} bytes of LDS per wave), 15 entries; 30 interpreter launches per pass against 6 compiled ones", "",
             "path | ms per pass: median (min-max) | by HIP events per pass: all scopes, extraction alone",
             f"compiled | {cell(c, 4)} | {ev['compiled']['all']:.4f}, {ext_c:.4f} (relations_extract; k_rel_emit is inside relations_sort)",
             f"program | {cell(p, 4)} | {ev['program']['all']:.4f}, {ext_p:.4f} "
             f"(relation_program_count {ev['program']['relation_program_count']:.4f} + relation_program_emit {ev['program']['relation_program_emit']:.4f})",
             f"program / compiled | {statistics.median(p) / statistics.median(c):.2f}x | {ev['program']['all'] / ev['compiled']['all']:.2f}x all scopes"]
    emit("\n".join(lines) + "\n", a.out)


if __name__ == "__main__":
    main()
