#!/usr/bin/env python3
"""What bfhip_trace_check costs beside a proof of the same trace: fib19 (LOG_MAX_ROWS 24) and the synthetic 2^22-row trace of
tools/benchlib/workloads.py (LOG_MAX_ROWS 22), in one process each workload.

  check   median of 5 after 2 warm-ups, every call timed on its own (`repeated` of tools/ratelib.py). GPU time by HIP events (one event
          pair around the four logUp launches, one around the 26 check launches) and the wall time of the whole call (staging, two
          read-backs).
  proof   median of 5 after 2 warm-ups of the same resident trace with the profiler off: the `interaction` entry of phase_seconds (logUp
          generation + interaction tree + the round trip) and the total.

The check shares the logUp generation with that phase and adds one read of the row-granular main columns and two reads of the last logUp
column; it does no transform and no hashing. Output: one block of text per workload (--out FILE also writes it to a file)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.benchlib.workloads import FIB19, sweep_program      # noqa: E402
from ratelib import emit, load_package, repeated, require_gpu      # noqa: E402


def measure(pkg, name, code, log_max_rows, reps, warmup):
    ctx = pkg.Context(0, max_log_domain=log_max_rows + 2)
    tr = pkg.Trace(ctx, code)
    results = []
    kept = repeated(ctx, lambda: results.append(tr.check()), reps, warmup)
    for res in results:
        assert res.ok, res.failures()
    wall = [w for w, _ in kept]
    parts = [(ms["trace_check_logup"], ms["k_check_cells"]) for _, ms in kept]
    gpu = [a + b for a, b in parts]
    inter, total = [], []
    for i in range(warmup + reps):
        _, ph = tr.prove(log_max_rows, want_json=False)
        if i >= warmup:
            inter.append(1e3 * ph["interaction"]); total.append(1e3 * ph["total"])
    tr.close(); ctx.close()
    med = statistics.median
    g, w, it, tt = med(gpu), med(wall), med(inter), med(total)
    lines = [f"{name}: LOG_MAX_ROWS {log_max_rows}, component log sizes {tr.log_sizes}, {tr.cells} cells",
             f"  check, GPU time by HIP events   median {g:.3f} ms of {reps} (min {min(gpu):.3f}, max {max(gpu):.3f}); "
             f"logUp generation {med(p[0] for p in parts):.3f} ms + check kernels {med(p[1] for p in parts):.3f} ms",
             f"  check, wall time of the call    median {w:.3f} ms (min {min(wall):.3f}, max {max(wall):.3f})",
             f"  proof, interaction phase        median {it:.3f} ms (min {min(inter):.3f}, max {max(inter):.3f})",
             f"  proof, total                    median {tt:.3f} ms (min {min(total):.3f}, max {max(total):.3f})",
             f"  check / interaction phase       {g / it:.3f} by GPU time, {w / it:.3f} by wall time",
             f"  check / proof                   {g / tt:.4f} by GPU time, {w / tt:.4f} by wall time"]
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--out")
    a = ap.parse_args()
    pkg = load_package()
    require_gpu(pkg, "trace_check_rate")
    lines = []
    for name, code, lmr in (("fib19", FIB19, 24), ("synthetic 2^22 rows", sweep_program(22), 22)):
        lines += measure(pkg, name, code, lmr, a.reps, a.warmup) + [""]
    emit("\n".join(lines) + "\n", a.out)


if __name__ == "__main__":
    main()
