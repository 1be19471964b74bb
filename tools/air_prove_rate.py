#!/usr/bin/env python3
"""What the protocol driver costs: bfhip_air_prove beside the same protocol made call by call from Python, in one run on one GPU.

  python3 tools/air_prove_rate.py [--program tests/golden/programs/fib19.bf] [--lookup-log 12] [--calls 10] [--rounds 5] [--out profiles/air_prove_rate.txt]

  cases      "brainfuck": brainfuck_air_statement (13 constraint programs, 13 fraction programs, 3 relations) over the resident trace of
             --program: IsFirst as coefficients, the main trace as full-size device columns (tools/bfprove.py generic_columns).
             "lookup": the lookup AIR of INTEGRATION.md section 2e (one component, two logUp columns) at --lookup-log.
  (a)        Context.air_prove, every component interpreted
  (b)        Context.air_prove, every component as its compiled kernel (compiled once, outside the windows)
  (c)        the same protocol call by call over PcsSession, Channel, logup_program_generate_batch, evaluate, air_compose and
             air_compose_at_point: the sequence of INTEGRATION.md section 2e as tests/test_gpu_air_prove.py restates it (_hand_prove), every
             buffer of its own allocated and freed inside the run as a caller would
  (d)        brainfuck only, for orientation: Trace.prove (bfhip_prove_trace), the built-in path on the same trace (row-granular columns,
             compiled-in kernels, its own launch order)
  check      before the timing: (a), (b) and (c) return the same proof bytes, and on the brainfuck case (d)'s proof member is those bytes.
  time       ms per proof: the paths alternate in windows of `calls` back-to-back proofs, `rounds` windows each (every path returns with
             the GPU idle), and by HIP events: GPU ms per proof and timed launches per proof, in all and by kernel (tools/ratelib.py has
             the scheme).

No threshold is attached. A run without a GPU fails: nothing here is measured on the host."""
import argparse
import os
import statistics

import numpy as np

from ratelib import ROOT, alternate, cell, emit, events, load_package, require_gpu      # first: it puts tests/ on the path
import pcs_replay                                                 # noqa: E402
import test_gpu_air_prove as hand                                 # noqa: E402
from bfprove import generic_columns                               # noqa: E402

CONV = (0, 0, 0, 0)


class Case:
    def __init__(self, pkg, ctx, st, cols, ptrs, trace=None, log_max_rows=0):
        self.pkg, self.ctx, self.st, self.cols, self.ptrs, self.trace, self.lmr = pkg, ctx, st, cols, ptrs, trace, log_max_rows
        self.kernels = [ctx.air_compile(c[0]) for c in st.components]
        self.kinds = ["interpreted", "compiled", "by hand"] + (["prove_trace"] if trace is not None else [])

    def call(self, kind):
        with self.pkg.Channel(CONV) as ch:
            if kind == "interpreted":
                return hand._split(self.ctx.air_prove(self.st, self.cols, ch))[1]
            if kind == "compiled":
                return hand._split(self.ctx.air_prove(self.st, self.cols, ch, kernels=self.kernels))[1]
            if kind == "by hand":
                _, _, proof, sampled, at_point = hand._hand_prove(self.pkg, self.ctx, self.st, self.cols, ch)
                assert sampled == at_point
                return proof
        return pcs_replay.proof_member(self.trace.prove(self.lmr)[0])

    def check(self):
        proofs = {k: self.call(k) for k in self.kinds}
        if len(set(proofs.values())) != 1:
            raise SystemExit("air_prove_rate: the paths return different proofs: " + ", ".join("%s %d bytes" % (k, len(v)) for k, v in proofs.items()))
        return len(proofs["interpreted"])

    def measure(self, calls, rounds):
        paths = {k: (lambda k=k: self.call(k)) for k in self.kinds}
        return alternate(self.ctx, paths, calls, rounds), {k: events(self.ctx, paths[k], calls) for k in self.kinds}

    def close(self):
        for k in self.kernels:
            k.close()
        for p in self.ptrs:
            self.ctx.free(p)
        if self.trace is not None:
            self.trace.close()


def brainfuck_case(pkg, ctx, code, log_max_rows):
    tr = pkg.Trace(ctx, code, b"")
    cols, ptrs = generic_columns(pkg, ctx, tr, log_max_rows)
    return Case(pkg, ctx, pkg.brainfuck_air_statement(tr.log_sizes, log_max_rows, 0), cols, ptrs, tr, log_max_rows)


def lookup_case(pkg, ctx, log_size):
    trace = np.concatenate([hand._lookup_trace(log_size, 51), hand._is_first(log_size)[None]])
    ptrs = [ctx.upload(np.ascontiguousarray(c, dtype=np.uint32)) for c in trace]
    return Case(pkg, ctx, hand._lookup_statement(pkg, log_size), [ptrs], ptrs)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--program", default=os.path.join(ROOT, "tests", "golden", "programs", "fib19.bf")); ap.add_argument("--lookup-log", type=int, default=12)
    ap.add_argument("--calls", type=int, default=10); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--out")
    a = ap.parse_args()
    pkg = load_package()
    require_gpu(pkg, "air_prove_rate")
    code = open(a.program).read()
    probe = pkg.Context(0, max_log_domain=24)
    tr = pkg.Trace(probe, code, b"")
    log_sizes, steps = tr.log_sizes, tr.n_steps
    tr.close(); probe.close()
    lmr = max(log_sizes)
    ctx = pkg.Context(0, max_log_domain=max(lmr, a.lookup_log) + 2)
    lines = [f"bfhip_air_prove beside the same protocol call by call from Python: {a.rounds} alternating windows of {a.calls} proofs after a warm-up round, default PcsConfig; "
             "the same proof bytes checked first", "",
             "case | proof bytes | ms per proof, median (min-max): (a) air_prove interpreted | (b) air_prove compiled | (c) call by call | (d) prove_trace | (c) - (a) ms | "
             "GPU ms per proof by HIP events: (a) | (b) | (c) | (d) | timed launches per proof: (a) | (b) | (c) | (d)"]
    detail = []
    try:
        for name, make in (("brainfuck, %s (%d steps), component log sizes %s, log_max_rows %d" % (os.path.basename(a.program), steps, log_sizes, lmr), lambda: brainfuck_case(pkg, ctx, code, lmr)),
                           ("lookup AIR at log_size %d" % a.lookup_log, lambda: lookup_case(pkg, ctx, a.lookup_log))):
            case = make()
            try:
                n_bytes = case.check()
                ms, events = case.measure(a.calls, a.rounds)
                four = case.kinds + [None] * (4 - len(case.kinds))
                path = lambda k: "-" if k is None else cell(ms[k], 3)
                gpu = lambda k: "-" if k is None else "%.3f" % sum(t for t, _ in events[k].values())
                launches = lambda k: "-" if k is None else "%g" % sum(c for _, c in events[k].values())
                lines.append(f"{name} | {n_bytes} | " + " | ".join(path(k) for k in four) + f" | {statistics.median(ms['by hand']) - statistics.median(ms['interpreted']):.3f} | " +
                             " | ".join(gpu(k) for k in four) + " | " + " | ".join(launches(k) for k in four))
                short = name.split(",")[0].split(" at ")[0]
                for k, label in zip(case.kinds, ("(a)", "(b)", "(c)", "(d)")):
                    detail.append(f"  {short} {label} windows in the order measured, ms per proof: " + ", ".join("%.3f" % t for t in ms[k]))
                    detail.append(f"  {short} {label} GPU ms per proof by kernel (timed launches per proof): " +
                                  ", ".join(f"{n} {t:.4f} ({c:g})" for n, (t, c) in sorted(events[k].items(), key=lambda e: -e[1][0])))
            finally:
                case.close()
    finally:
        ctx.close()
    emit("\n".join(lines + [""] + detail) + "\n", a.out)


if __name__ == "__main__":
    main()
