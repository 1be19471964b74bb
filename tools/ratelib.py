"""How the *_rate.py scripts measure: said once here, used by all of them.

  window     ms per call = host clock around n back-to-back calls, the context synchronised before the clock starts and again before it
             stops, divided by n. Both synchronisations always: a call that ends in its own read-back leaves the second one an idle stream
             to wait for.
  alternate  the paths under comparison take one window each, in a fixed order, round after round; the first round is a warm-up and is
             dropped. A table cell is `median (min-max)` of a path's windows (cell).
  events     GPU time by HIP events: one further window under the library's profiler (Context.profiling, mode 1: an event pair around
             every instrumented launch), per profiler scope and per call. The profiler is off again afterwards, also after an error.
  repeated   for calls timed one by one: every call with the profiler on and reset before it, the first `warmup` calls dropped.

It is also the one module among these scripts that reaches into tests/ for load_package, splitmix_column and Oracle."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import Oracle, load_package, splitmix_column      # noqa: E402,F401


def require_gpu(pkg, name):
    if pkg.device_count() < 1:
        raise SystemExit("%s: no GPU" % name)


def window(ctx, call, n):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0) / n


def alternate(ctx, calls, n, rounds):
    """calls: {name: callable}, measured in that order. Returns {name: [ms per call of each of the `rounds` windows, in the order measured]}."""
    ms = {name: [] for name in calls}
    for r in range(rounds + 1):
        for name, call in calls.items():
            t = window(ctx, call, n)
            if r:
                ms[name].append(t)
    return ms


def _scopes(report):
    return {name: v for name, v in report.items() if isinstance(v, dict) and "total_ms" in v}


def events(ctx, call, n):
    """{scope: (GPU ms per call, timed launches per call)} of one window of n calls."""
    with ctx.profiling(1):
        window(ctx, call, n)
        report = ctx.profile_report()
    return {name: (v["total_ms"] / n, v["calls"] / n) for name, v in _scopes(report).items()}


def repeated(ctx, call, reps, warmup):
    """[(wall ms of the call, {scope: total_ms})] of the last `reps` of warmup + reps calls."""
    kept = []
    with ctx.profiling(1):
        for i in range(warmup + reps):
            ctx.profile_reset()
            t0 = time.perf_counter()
            call()
            wall = 1e3 * (time.perf_counter() - t0)
            gpu = {name: v["total_ms"] for name, v in _scopes(ctx.profile_report()).items()}
            if i >= warmup:
                kept.append((wall, gpu))
    return kept


def cell(xs, digits):
    return "%.*f (%.*f-%.*f)" % (digits, statistics.median(xs), digits, min(xs), digits, max(xs))


def emit(text, out, append=False):
    print(text, end="")
    if out:
        open(out, "a" if append else "w").write(text)
