#!/usr/bin/env python3
"""AIR statements through the pool's queue, and what the scratch reserve changes: bfhip_pool_submit_air beside a loop of bfhip_air_prove,
in one run on one GPU.

  python3 tools/air_pool_rate.py [--program tests/golden/programs/fib19.bf] [--lookup-logs 12 16] [--calls 12] [--rounds 5] [--out profiles/air_pool_rate.txt]

  cases      the lookup AIR of INTEGRATION.md section 2e at every --lookup-logs size (interpreted), and brainfuck_air_statement over the
             resident trace of --program (tools/bfprove.py generic_columns), interpreted and with every component compiled.
  (a)        a loop of Context.air_prove on one context without a reserve: the path before the queue took such jobs, the baseline
  (b)        the same loop on the same context with a scratch reserve set
  (c1..c3)   Pool.submit_air on a pool of three workers with a reserve on every sub-context, at most 1, 2 and 3 jobs outstanding: a new job
             is submitted when a result has been taken
  (d)        the same pool at 3 outstanding WITHOUT the reserve: every proof's call-scoped memory is allocated and released on the device
  reserve    sized per case from a trial proof under a generous reserve: its high-water mark (Context.scratch_stats), rounded up to 1 MiB.
             Setting and clearing it happens between windows, outside the clock.
  check      before the timing every path returns the bytes of (a).
  time       ms per proof by the scheme of tools/ratelib.py: the paths take one window of `calls` proofs each, in a fixed order, round after
             round, the first round dropped; a cell is median (min-max), every window is listed.
  verdict    one path against another only where every window of one lies on one side of every window of the other; otherwise "windows
             overlap" and no ratio.
  counts     device allocations made by call-scoped memory per proof and requests served from the reserve per proof, per path, from
             scratch_stats before and after the measured windows; the high-water marks.

No threshold is attached. A run without a GPU fails: nothing here is measured on the host."""
import argparse
import os
import statistics
import time

import numpy as np

from ratelib import ROOT, cell, emit, load_package, require_gpu, splitmix_column      # first: it puts tests/ on the path
import test_gpu_air_prove as hand                                 # noqa: E402
from bfprove import generic_columns                               # noqa: E402

CONV = (0, 0, 0, 0)
P = (1 << 31) - 1
MIB = 1 << 20
WAIT_S = 600
PATHS = ("a", "b", "c1", "c2", "c3", "d")


class Case:
    """One statement over resident columns, one plain context and one pool of three workers."""

    def __init__(self, pkg, name, max_log_domain, make, compiled):
        self.pkg, self.name = pkg, name
        self.ctx = pkg.Context(0, max_log_domain=max_log_domain)
        self.pool = pkg.Pool(0, n_in_flight=3, max_log_domain=max_log_domain)
        self.st, self.cols, self.ptrs, self.trace = make(self.ctx)
        self.kernels = [self.ctx.air_compile(c[0]) for c in self.st.components] if compiled else None
        self.pool_kernels = [self.pool.air_compile(c[0]) for c in self.st.components] if compiled else None
        self.reserve, self.trial_mark = 0, 0

    def subs(self):
        return [self.pool.ctx(w) for w in range(3)]

    def size_reserve(self, generous):
        """One proof under a generous reserve; the reserve of the measurement is its high-water mark rounded up to 1 MiB."""
        self.ctx.set_scratch_reserve(generous)
        self.loop(1)
        stats = self.ctx.scratch_stats()
        self.ctx.set_scratch_reserve(0)
        if stats["high_water"] == 0 or stats["high_water"] > generous:
            raise SystemExit("air_pool_rate: %s: the trial proof did not fit the generous reserve: %s" % (self.name, stats))
        self.trial_mark = stats["high_water"]
        self.reserve = (stats["high_water"] + MIB - 1) // MIB * MIB

    def prepare(self, path):
        """between windows, outside the clock"""
        self.ctx.set_scratch_reserve(self.reserve if path == "b" else 0)
        self.pool.set_scratch_reserve(self.reserve if path in ("c1", "c2", "c3") else 0)

    def loop(self, n):
        out = []
        for _ in range(n):
            with self.pkg.Channel(CONV) as ch:
                out.append(self.ctx.air_prove(self.st, self.cols, ch, kernels=self.kernels))
        return out

    def queue(self, n, in_flight):
        out, submitted = [], 0
        with self.pkg.Channel(CONV) as ch:
            while len(out) < n:
                while submitted < n and submitted - len(out) < in_flight:
                    self.pool.submit_air(self.st, self.cols, ch, kernels=self.pool_kernels)
                    submitted += 1
                r = self.pool.wait(WAIT_S)
                if not r.ok:
                    raise SystemExit("air_pool_rate: %s: %s" % (self.name, r.error))
                out.append(r.proof)
        return out

    def run(self, path, n):
        return self.loop(n) if path in ("a", "b") else self.queue(n, 3 if path == "d" else int(path[1]))

    def check(self):
        want = None
        for path in PATHS:
            self.prepare(path)
            got = self.run(path, 3)
            want = want or got[0]
            if any(p != want for p in got):
                raise SystemExit("air_pool_rate: %s: path (%s) returns other bytes than (a)" % (self.name, path))
        return len(want)

    def counters(self):
        return [self.ctx.scratch_stats()] + [s.scratch_stats() for s in self.subs()]

    def measure(self, calls, rounds):
        ms = {p: [] for p in PATHS}
        allocs, served = {p: 0 for p in PATHS}, {p: 0 for p in PATHS}
        for r in range(rounds + 1):
            for path in PATHS:
                self.prepare(path)
                before = self.counters()
                self.ctx.sync()
                t0 = time.perf_counter()
                self.run(path, calls)
                self.ctx.sync()
                t = 1e3 * (time.perf_counter() - t0) / calls
                after = self.counters()
                if r:
                    ms[path].append(t)
                    allocs[path] += sum(a["device_allocations"] - b["device_allocations"] for a, b in zip(after, before))
                    served[path] += sum(a["served"] - b["served"] for a, b in zip(after, before))
        per = lambda d: {p: d[p] / (rounds * calls) for p in PATHS}
        return ms, per(allocs), per(served)

    def close(self):
        for k in (self.kernels or []) + (self.pool_kernels or []):
            k.close()
        self.pool.close()
        for p in self.ptrs:
            self.ctx.free(p)
        if self.trace is not None:
            self.trace.close()
        self.ctx.close()


def verdict(x, base):
    """x against base by the rule of DESIGN section 9p: a ratio only where the windows of the two paths do not interleave"""
    if max(x) < min(base):
        return "faster: %.2fx (%.3f vs %.3f ms, no window of either inside the other's range)" % (statistics.median(base) / statistics.median(x), statistics.median(x), statistics.median(base))
    if min(x) > max(base):
        return "slower: %.2fx (%.3f vs %.3f ms, no window of either inside the other's range)" % (statistics.median(x) / statistics.median(base), statistics.median(x), statistics.median(base))
    return "windows overlap: no ratio"


def lookup_trace(log_size, seed):
    """a, t, mult in storage order as tests/test_gpu_air_prove.py makes them, with a table that stays distinct at any size: t[i] = 1000003 i
    + seed mod p"""
    n = 1 << log_size
    t = ((np.arange(n, dtype=np.uint64) * np.uint64(1000003) + np.uint64(seed)) % np.uint64(P)).astype(np.uint32)
    pick = splitmix_column((seed + 1) << 32, n) % np.uint32(n // 4)
    return np.stack([t[pick], t, np.bincount(pick, minlength=n).astype(np.uint32)])


def lookup_maker(pkg, log_size):
    def make(ctx):
        trace = np.concatenate([lookup_trace(log_size, 51), hand._is_first(log_size)[None]])
        ptrs = [ctx.upload(np.ascontiguousarray(c, dtype=np.uint32)) for c in trace]
        return hand._lookup_statement(pkg, log_size), [ptrs], ptrs, None
    return make


def brainfuck_maker(pkg, code, log_max_rows):
    def make(ctx):
        tr = pkg.Trace(ctx, code, b"")
        cols, ptrs = generic_columns(pkg, ctx, tr, log_max_rows)
        return pkg.brainfuck_air_statement(tr.log_sizes, log_max_rows, 0), cols, ptrs, tr
    return make


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--program", default=os.path.join(ROOT, "tests", "golden", "programs", "fib19.bf")); ap.add_argument("--lookup-logs", type=int, nargs="*", default=[12, 16])
    ap.add_argument("--calls", type=int, default=12); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--generous-mib", type=int, default=4096)
    ap.add_argument("--no-brainfuck", action="store_true"); ap.add_argument("--out")
    a = ap.parse_args()
    pkg = load_package()
    require_gpu(pkg, "air_pool_rate")
    cases = [("lookup AIR at log_size %d, interpreted" % l, l + 2, lookup_maker(pkg, l), False) for l in a.lookup_logs]
    if not a.no_brainfuck:
        code = open(a.program).read()
        probe = pkg.Context(0, max_log_domain=24)
        tr = pkg.Trace(probe, code, b"")
        log_sizes, steps = tr.log_sizes, tr.n_steps
        tr.close(); probe.close()
        lmr = max(log_sizes)
        for compiled in (False, True):
            cases.append(("brainfuck, %s (%d steps), log_max_rows %d, %s" % (os.path.basename(a.program), steps, lmr, "compiled" if compiled else "interpreted"), lmr + 2,
                          brainfuck_maker(pkg, code, lmr), compiled))
    lines = [f"bfhip_pool_submit_air beside a loop of bfhip_air_prove: {a.rounds} alternating windows of {a.calls} proofs after a warm-up round, default PcsConfig; one plain context and "
             "one pool of three workers per case; the same proof bytes checked first on every path", "",
             "case | proof bytes | reserve bytes (high-water mark of the trial proof) | ms per proof, median (min-max): (a) air_prove loop | (b) loop with the reserve | (c) queue with the reserve, "
             "1 in flight | 2 in flight | 3 in flight | (d) queue, 3 in flight, no reserve"]
    detail = []
    for name, max_log_domain, make, compiled in cases:
        case = Case(pkg, name, max_log_domain, make, compiled)
        try:
            case.size_reserve(a.generous_mib * MIB)
            n_bytes = case.check()
            ms, allocs, served = case.measure(a.calls, a.rounds)
            case.prepare("c3")
            case.run("c3", 6)
            marks = [s.scratch_stats()["high_water"] for s in case.subs()]
            lines.append(f"{name} | {n_bytes} | {case.reserve} ({case.trial_mark}) | " + " | ".join(cell(ms[p], 3) for p in PATHS))
            short = name.split(",")[0] + (" compiled" if compiled else "")
            for p in PATHS:
                detail.append(f"  {short} ({p}) windows in the order measured, ms per proof: " + ", ".join("%.3f" % t for t in ms[p]) +
                              f"; device allocations by call-scoped memory per proof {allocs[p]:g}, requests served from the reserve per proof {served[p]:g}")
            detail.append(f"  {short} high-water marks of the three sub-contexts after six more jobs at 3 in flight: " + ", ".join(map(str, marks)))
            detail.append(f"  {short} (b) against (a): " + verdict(ms["b"], ms["a"]))
            for p in ("c1", "c2", "c3"):
                detail.append(f"  {short} ({p}) against (a): " + verdict(ms[p], ms["a"]))
            detail.append(f"  {short} (d) against (c3): " + verdict(ms["d"], ms["c3"]))
        finally:
            case.close()
    emit("\n".join(lines + [""] + detail) + "\n", a.out)


if __name__ == "__main__":
    main()
