#!/usr/bin/env python3
"""What a proof's preflight (bfhip_ctx_set_preflight) costs and what it saves: fib19 (LOG_MAX_ROWS 24) and the synthetic 2^22- and 2^20-row
traces of tools/benchlib/workloads.py (LOG_MAX_ROWS 22 and 20), one process, one box.

  proof      the same resident trace proved with the preflight off and on, ALTERNATING, median of 5 after 2 warm-ups each: the total of
             phase_seconds, and the preflight's own host wall time (bfhip_preflight_report.seconds).
  preflight  GPU time by HIP events (one event pair around the four logUp launches, one around the launch pair k_check_batch +
             k_check_first_batch), every proof timed on its own (`repeated` of tools/ratelib.py), same counts. 6 launches, ONE host
             synchronisation (the read-back of 13 reports, 13 claimed sums and the total).
  check      the unbatched Trace.check() of the same trace, same protocol: its two event pairs and the wall time of the call. 4 + 26
             launches, TWO host synchronisations (the claimed sums, then the reports).
  rejection  the trace's register rows with one mv altered, as a resident trace: wall time from the call to the TraceRejected (median of 5
             after 2 warm-ups), beside the wall time the same trace takes to fail with ConstraintsNotSatisfied with the preflight off.
  arena      high-water mark of the context's arena after one proof in a fresh context, preflight off and on.

A diagnostic: no threshold. Output: one block of text per workload (--out FILE also writes it to a file)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.benchlib.workloads import FIB19, sweep_program      # noqa: E402
from ratelib import emit, load_package, repeated, require_gpu      # noqa: E402

med = statistics.median


def timed(ctx, call, names, reps, warmup):
    """([GPU ms per name], [wall ms]) of `call`, one sample per repetition."""
    kept = repeated(ctx, call, reps, warmup)
    return [[ms.get(n, 0.0) for n in names] for _, ms in kept], [wall for wall, _ in kept]


def arena_peak(pkg, tr_args, log_max_rows, on):
    ctx = pkg.Context(0, max_log_domain=log_max_rows + 2)
    tr = pkg.Trace.from_registers(ctx, *tr_args)
    ctx.set_preflight(on)
    tr.prove(log_max_rows, want_json=False)
    peak = ctx.memory()["arena_peak"]
    tr.close(); ctx.close()
    return peak


def failing_ms(pkg, tr, log_max_rows, reps, warmup, exc):
    out = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        try:
            tr.prove(log_max_rows, want_json=False)
            raise SystemExit("the altered trace was proved")
        except exc:
            pass
        if i >= warmup:
            out.append(1e3 * (time.perf_counter() - t0))
    return out


def measure(pkg, name, code, log_max_rows, reps, warmup):
    ctx = pkg.Context(0, max_log_domain=log_max_rows + 2)
    _, rows = pkg.host_run(code)
    words = pkg.host_compile(code)
    tr = pkg.Trace.from_registers(ctx, rows, words)
    off, on, pre_wall = [], [], []
    for i in range(warmup + reps):
        ctx.set_preflight(False)
        _, ph0 = tr.prove(log_max_rows, want_json=False)
        ctx.set_preflight(True)
        _, ph1 = tr.prove(log_max_rows, want_json=False)
        assert ctx.last_proof_flags()["preflight"]
        if i >= warmup:
            off.append(1e3 * ph0["total"]); on.append(1e3 * ph1["total"]); pre_wall.append(1e3 * ctx.last_preflight()[0].seconds)
    pre_gpu, _ = timed(ctx, lambda: tr.prove(log_max_rows, want_json=False), ("preflight_logup", "preflight_check"), reps, warmup)
    ctx.set_preflight(False)
    chk_gpu, chk_wall = timed(ctx, lambda: tr.check(), ("trace_check_logup", "k_check_cells"), reps, warmup)
    bad_rows = rows.copy()
    bad_rows[1, 5] = (int(bad_rows[1, 5]) + 4) % ((1 << 31) - 1)
    bad = pkg.Trace.from_registers(ctx, bad_rows, words)
    late = failing_ms(pkg, bad, log_max_rows, reps, warmup, pkg.BfhipError)
    ctx.set_preflight(True)
    early = failing_ms(pkg, bad, log_max_rows, reps, warmup, pkg.TraceRejected)
    first_line = str(ctx.last_preflight()[0].failures()[0])
    ctx.set_preflight(False)
    log_sizes = tr.log_sizes
    bad.close(); tr.close(); ctx.close()
    peak_off, peak_on = arena_peak(pkg, (rows, words), log_max_rows, False), arena_peak(pkg, (rows, words), log_max_rows, True)
    pg, cg = [sum(s) for s in pre_gpu], [sum(s) for s in chk_gpu]
    return [f"{name}: LOG_MAX_ROWS {log_max_rows}, component log sizes {log_sizes}",
            f"  proof, preflight off               median {med(off):.3f} ms of {reps} (min {min(off):.3f}, max {max(off):.3f})",
            f"  proof, preflight on                median {med(on):.3f} ms (min {min(on):.3f}, max {max(on):.3f}); of which the preflight's host wall time {med(pre_wall):.3f} ms",
            f"  preflight, GPU time by HIP events  median {med(pg):.3f} ms (min {min(pg):.3f}, max {max(pg):.3f}): logUp {med(s[0] for s in pre_gpu):.3f} + batched check {med(s[1] for s in pre_gpu):.3f}; "
            "6 launches, 1 host synchronisation",
            f"  Trace.check(), GPU time            median {med(cg):.3f} ms (min {min(cg):.3f}, max {max(cg):.3f}): logUp {med(s[0] for s in chk_gpu):.3f} + 26 check launches {med(s[1] for s in chk_gpu):.3f}; "
            "30 launches, 2 host synchronisations",
            f"  Trace.check(), wall time of call   median {med(chk_wall):.3f} ms (min {min(chk_wall):.3f}, max {max(chk_wall):.3f})",
            f"  batched check / 26 launches        {med(s[1] for s in pre_gpu) / med(s[1] for s in chk_gpu):.2f} by GPU time",
            f"  altered trace, preflight off       ConstraintsNotSatisfied after median {med(late):.3f} ms (min {min(late):.3f}, max {max(late):.3f})",
            f"  altered trace, preflight on        TraceRejected after median {med(early):.3f} ms (min {min(early):.3f}, max {max(early):.3f}): {first_line}",
            f"  arena high-water, one proof        off {peak_off} bytes, on {peak_on} bytes"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--out")
    ap.add_argument("--only", type=int, default=-1, help="one workload only: 0 fib19, 1 synthetic 2^22 rows, 2 synthetic 2^20 rows")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it (one workload per run)")
    a = ap.parse_args()
    pkg = load_package()
    require_gpu(pkg, "preflight_rate")
    loads = (("fib19", FIB19, 24), ("synthetic 2^22 rows", sweep_program(22), 22), ("synthetic 2^20 rows", sweep_program(20), 20))
    lines = []
    for k, (name, code, lmr) in enumerate(loads):
        if a.only in (-1, k):
            lines += measure(pkg, name, code, lmr, a.reps, a.warmup) + [""]
    emit("\n".join(lines) + "\n", a.out, a.append)


if __name__ == "__main__":
    main()
