#!/usr/bin/env python3
"""What bfhip_trace_relations costs beside bfhip_trace_check and a proof of the same trace: fib19 (LOG_MAX_ROWS 24) and the synthetic
2^22-row trace of tools/benchlib/workloads.py (LOG_MAX_ROWS 22), in one process each workload.

  relations  median of 5 after 2 warm-ups, every call timed on its own (`repeated` of tools/ratelib.py). GPU time by HIP events (one event
             pair around each stage of each of the three relations — extract, sort, reduce, report; the host's three small read-backs per
             relation lie between the pairs) and the wall time of the whole call.
  check      the same protocol for Trace.check(): its two event pairs and its wall time.
  proof      median of 5 after 2 warm-ups of the same resident trace with the profiler off: the total of phase_seconds.

A diagnostic: no threshold. Output: one block of text per workload (--out FILE also writes it to a file)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.benchlib.workloads import FIB19, sweep_program      # noqa: E402
from ratelib import emit, load_package, repeated, require_gpu      # noqa: E402

STAGES = ("relations_extract", "relations_sort", "relations_reduce", "relations_report")


def timed(ctx, call, names, reps, warmup):
    """(GPU ms per stage, wall ms) of `call`, one sample per repetition."""
    kept = repeated(ctx, call, reps, warmup)
    return [[ms.get(n, 0.0) for n in names] for _, ms in kept], [wall for wall, _ in kept]


def measure(pkg, name, code, log_max_rows, reps, warmup):
    ctx = pkg.Context(0, max_log_domain=log_max_rows + 2)
    tr = pkg.Trace(ctx, code)
    res = tr.relations()
    assert res.balanced, res.lines()
    rel_gpu, rel_wall = timed(ctx, lambda: tr.relations(), STAGES, reps, warmup)
    chk_gpu, chk_wall = timed(ctx, lambda: tr.check(), ("trace_check_logup", "k_check_cells"), reps, warmup)
    total = []
    for i in range(warmup + reps):
        _, ph = tr.prove(log_max_rows, want_json=False)
        if i >= warmup:
            total.append(1e3 * ph["total"])
    tr.close(); ctx.close()
    med = statistics.median
    g, w, cg, cw, tt = med(sum(s) for s in rel_gpu), med(rel_wall), med(sum(s) for s in chk_gpu), med(chk_wall), med(total)
    stages = ", ".join("%s %.3f" % (n.split("_")[1], med(s[k] for s in rel_gpu)) for k, n in enumerate(STAGES))
    return [f"{name}: LOG_MAX_ROWS {log_max_rows}, component log sizes {tr.log_sizes}",
            "  relation entries / distinct tuples  " + ", ".join("%s %d / %d" % (r["name"], r["n_entries"], r["n_tuples"]) for r in res.reports),
            f"  relations, GPU time by HIP events   median {g:.3f} ms of {reps} (min {min(sum(s) for s in rel_gpu):.3f}, max {max(sum(s) for s in rel_gpu):.3f}); ms by stage: {stages}",
            f"  relations, wall time of the call    median {w:.3f} ms (min {min(rel_wall):.3f}, max {max(rel_wall):.3f})",
            f"  check, GPU time by HIP events       median {cg:.3f} ms (min {min(sum(s) for s in chk_gpu):.3f}, max {max(sum(s) for s in chk_gpu):.3f})",
            f"  check, wall time of the call        median {cw:.3f} ms (min {min(chk_wall):.3f}, max {max(chk_wall):.3f})",
            f"  proof, total                        median {tt:.3f} ms (min {min(total):.3f}, max {max(total):.3f})",
            f"  relations / check                   {g / cg:.2f} by GPU time, {w / cw:.2f} by wall time",
            f"  relations / proof                   {g / tt:.4f} by GPU time, {w / tt:.4f} by wall time"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--out")
    a = ap.parse_args()
    pkg = load_package()
    require_gpu(pkg, "relations_rate")
    lines = []
    for name, code, lmr in (("fib19", FIB19, 24), ("synthetic 2^22 rows", sweep_program(22), 22)):
        lines += measure(pkg, name, code, lmr, a.reps, a.warmup) + [""]
    emit("\n".join(lines) + "\n", a.out)


if __name__ == "__main__":
    main()
