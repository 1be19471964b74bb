#!/usr/bin/env python3
"""What the one-call interaction trace buys: bfhip_logup_program_generate_batch beside the single calls it replaces and beside the frozen
compiled path, on the same tables, in one run on one GPU.

  python3 tools/logup_batch_rate.py [--program tests/golden/programs/fib19.bf] [--equal-log 12] [--calls 50] [--rounds 5] [--out profiles/logup_batch_rate.txt] [--append]

  cases      "brainfuck": the 13 brainfuck_logup_programs at the component sizes of one Brainfuck trace (the CPU oracle runs the program for
             its 13 log sizes). "13 equal": the same 13 programs, every one at --equal-log. "brainfuck and one heavy program": the first
             case plus a 16-cell component whose seeded random program (tests/logup_model.py) keeps 40 KiB of register files a wave, the
             case in which the library launches the large components alone: under BFHIP_LOGUP_BATCH_LAUNCH=one every wave asks for 40 KiB.
             Row-granular main columns of 2^(log_size - 4) rows, splitmix values, not that trace's: no kernel here branches on a cell, and
             the check below needs no valid trace. The programs read them at shift 4 and write every logUp column full size.
  (a)        Context.logup_program_generate_batch: one allocation, k_logup_program_batch (BFHIP_LOGUP_BATCH_LAUNCH=one: one row-stage launch
             for all components; =each: one per component; =size: every component of 2^16 cells and more alone; unset: the library's rule,
             one launch unless the largest program's LDS would lower a large component's occupancy), three scan launches, one read-back
  (b)        Context.logup_program_generate, 13 times: what a caller had before (a)
  (c)        Context.logup_generate, 13 times: the compiled, replication-aware path (row-granular earlier columns, a scan over rows), for
             orientation
  check      before the timing: (a) and (b) leave the same words in every column and the same claimed sums; (c)'s earlier columns broadcast
             16-fold, its last column and its claimed sums are (a)'s.
  time       ms per call of the whole list: the three alternate in windows of `calls` back-to-back runs, `rounds` windows each (every path
             returns with the GPU idle: each call reads its claimed sums back), and by HIP events, by kernel (tools/ratelib.py has the
             scheme).

No threshold is attached. A run without a GPU fails: nothing here is measured on the host."""
import argparse
import os
import statistics

import numpy as np

from ratelib import ROOT, Oracle, alternate, cell, emit, events, load_package, require_gpu, splitmix_column      # first: it puts tests/ on the path
import logup_model

KINDS = ("batch", "singles", "compiled")


class Case:
    def __init__(self, pkg, ctx, log_sizes, heavy=False):
        self.pkg, self.ctx, self.ptrs, self.items = pkg, ctx, [], []
        self.elems = [int(v) or 1 for v in splitmix_column(77, 24)]
        self.params = pkg.brainfuck_air_params(self.elems, [0, 0, 0, 0])[:24]
        for comp, log in enumerate(log_sizes):
            program, _ = pkg.brainfuck_logup_program(comp)
            n_main, n_logup = program.shape["n_cols"], program.shape["n_logup_cols"]
            n, M = 1 << log, 1 << (log - 4)
            rows = [self.up(splitmix_column((1000 + 16 * comp + k) << 32, M)) for k in range(n_main)]
            sizes = [M] * (4 * (n_logup - 1)) + [n] * 4
            self.items.append(dict(comp=comp, program=program, log=log, rows=rows, shifts=[4] * n_main, sizes=sizes,
                                   out={"batch": [self.empty(n) for _ in range(4 * n_logup)], "singles": [self.empty(n) for _ in range(4 * n_logup)],
                                        "compiled": [self.empty(s) for s in sizes]}))
        if heavy:      # a 16-cell component whose seeded random program keeps 40 KiB of register files a wave; it has no compiled counterpart
            code, n_cols, n_params = logup_model.random_program(7, 1, 4, m_pool=90, q_pool=20)
            pars = splitmix_column(601, 4 * n_params).reshape(n_params, 4).tolist()
            self.items.append(dict(comp=None, program=pkg.LogupProgram(code, n_cols, n_params), log=4, rows=[self.up(splitmix_column((3000 + k) << 32, 16)) for k in range(n_cols)],
                                   shifts=None, sizes=[16] * 4, params=pars, out={"batch": [self.empty(16) for _ in range(4)], "singles": [self.empty(16) for _ in range(4)]}))
        self.entries = [(i["program"], i["log"], i["rows"], i.get("params", self.params), i["out"]["batch"], i["shifts"]) for i in self.items]

    def up(self, arr):
        self.ptrs.append(self.ctx.upload(arr))
        return self.ptrs[-1]

    def empty(self, n):
        self.ptrs.append(self.ctx.malloc(4 * n))
        return self.ptrs[-1]

    def call(self, kind):
        ctx = self.ctx
        if kind == "batch":
            return ctx.logup_program_generate_batch(self.entries)[0]
        if kind == "singles":
            return [ctx.logup_program_generate(i["program"], i["log"], i["rows"], i.get("params", self.params), i["out"]["singles"], col_shifts=i["shifts"]) for i in self.items]
        return [ctx.logup_generate(i["comp"], i["log"], i["rows"], self.elems, i["out"]["compiled"]) for i in self.items if i["comp"] is not None]

    def check(self):
        claimed = {k: self.call(k) for k in KINDS}
        if not (claimed["batch"] == claimed["singles"] and claimed["batch"][: len(claimed["compiled"])] == claimed["compiled"]):
            raise SystemExit("logup_batch_rate: the claimed sums of the three paths disagree")
        for k, i in enumerate(self.items):
            n = 1 << i["log"]
            for j, (a, b, s) in enumerate(zip(i["out"]["batch"], i["out"]["singles"], i["sizes"])):
                got = self.ctx.download(a, n)
                same = np.array_equal(got, self.ctx.download(b, n))
                if i["comp"] is not None:
                    same = same and np.array_equal(got, np.repeat(self.ctx.download(i["out"]["compiled"][j], s), n // s))
                if not same:
                    raise SystemExit("logup_batch_rate: the three paths disagree on component %d" % k)

    def measure(self, calls, rounds):
        paths = {k: (lambda k=k: self.call(k)) for k in KINDS}
        return alternate(self.ctx, paths, calls, rounds), {k: events(self.ctx, paths[k], calls) for k in KINDS}

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--program", default=os.path.join(ROOT, "tests", "golden", "programs", "fib19.bf")); ap.add_argument("--input", default="")
    ap.add_argument("--equal-log", type=int, default=12); ap.add_argument("--calls", type=int, default=50); ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out"); ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    a = ap.parse_args()
    pkg = load_package()
    require_gpu(pkg, "logup_batch_rate")
    log_sizes, steps = Oracle().log_sizes(open(a.program).read(), a.input.encode())
    ctx = pkg.Context(0, max_log_domain=max(max(log_sizes), a.equal_log) + 1)
    lines = [f"BFHIP_LOGUP_BATCH_LAUNCH={os.environ.get('BFHIP_LOGUP_BATCH_LAUNCH', '(unset)')}: bfhip_logup_program_generate_batch beside the 13 calls of bfhip_logup_program_generate it replaces and "
             f"the 13 calls of bfhip_logup_generate (compiled, row-granular): {a.rounds} alternating windows of {a.calls} runs of the whole list after a warm-up round; the same words checked first", "",
             "case | cells in all | ms per run of the list, median (min-max): (a) one batch call | (b) 13 single calls | (c) 13 compiled calls | (b) - (a) ms | (b) / (a) | "
             "GPU ms per run by HIP events: (a) | (b) | (c)"]
    detail = []
    try:
        for name, logs, heavy in (("brainfuck, %s (%d steps), component log sizes %s" % (os.path.basename(a.program), steps, log_sizes), log_sizes, False),
                                  ("13 equal: the 13 programs at log_size %d" % a.equal_log, [a.equal_log] * 13, False),
                                  ("brainfuck and one heavy program: the first case and a 14th component of 16 cells with 40960 bytes of register files a wave ((c): the 13)", log_sizes, True)):
            case = Case(pkg, ctx, logs, heavy)
            try:
                case.check()
                ms, events = case.measure(a.calls, a.rounds)
                med = {k: statistics.median(ms[k]) for k in KINDS}
                gpu = {k: "%.3f" % sum(t for t, _ in events[k].values()) if events[k] else "- (its launches are not timed scopes)" for k in KINDS}
                lines.append(f"{name} | {sum(1 << i['log'] for i in case.items)} |{cell(ms['batch'], 3)} | {cell(ms['singles'], 3)} | {cell(ms['compiled'], 3)} | {med['singles'] - med['batch']:.3f} | "
                             f"{med['singles'] / med['batch']:.2f}x | {gpu['batch']} | {gpu['singles']} | {gpu['compiled']}")
                short = name.split(",")[0].split(":")[0]
                for k, label in zip(KINDS, ("(a)", "(b)", "(c)")):
                    detail.append(f"  {short} {label} windows in the order measured, ms per run: " + ", ".join("%.3f" % t for t in ms[k]))
                    if events[k]:
                        detail.append(f"  {short} {label} GPU ms per run by kernel (timed scopes per run): " +
                                      ", ".join(f"{n} {t:.4f} ({c:g})" for n, (t, c) in sorted(events[k].items(), key=lambda e: -e[1][0])))
            finally:
                case.close()
    finally:
        ctx.close()
    emit("\n".join(lines + [""] + detail) + "\n\n", a.out, a.append)


if __name__ == "__main__":
    main()
