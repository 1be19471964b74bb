#!/usr/bin/env python3
"""What the one-call composition buys: bfhip_air_compose beside the sequence of single operations a caller had before it, on the same
columns, in one run on one GPU.

  python3 tools/air_compose_rate.py [--program tests/golden/programs/fib19.bf] [--shrink 0] [--calls 10] [--rounds 5] [--out profiles/air_compose_rate.txt]

  cases      "brainfuck": the 13 brainfuck_air_programs at the component sizes of one Brainfuck trace (the CPU oracle runs the program for
             its 13 log sizes; --shrink s takes s off every size above 4 + s), every column full size on CanonicCoset(log + 1).
             "8 equal": 8 components of the processor program at one size (--equal-log).
             The cells are splitmix values, not that trace's: no kernel here branches on a cell, and the check below needs no valid trace.
  (a)        Context.air_compose over AirPrograms: k_air_compose (BFHIP_AIR_COMPOSE_LAUNCH=one: one launch for all buckets; =bucket: one per
             bucket; unset: the library's rule), one batched inverse transform, accumulate_sizes
  (b)        the same list as CompiledAirs: a zero fill per bucket, one generated kernel per component, the same finalize
  (c)        the sequence: a zero fill of every accumulator, bfhip_air_eval_domain per component under its slice of
             bfhip_air_compose_coeffs, bfhip_interpolate per size, bfhip_accumulate per smaller size and coordinate
  check      before the timing the three leave the same words in all four coefficient columns.
  events     GPU ms per call by kernel, and the LDS bytes per wave of every program beside what the shared launch asks for.
  time       ms per call: the three alternate in windows of `calls` back-to-back calls, `rounds` rounds (tools/ratelib.py has the scheme).
             (a) and (b) end every call with their own wait when the list has more than one bucket (they free their scratch); (c) keeps
             its accumulators allocated across calls.

No threshold is attached. A run without a GPU fails: nothing here is measured on the host."""
import argparse
import ctypes
import os
import statistics

import numpy as np

from ratelib import ROOT, Oracle, alternate, cell, emit, events, load_package, require_gpu, splitmix_column

KINDS = ("compose", "compose_compiled", "sequence")
R = [0x1234567, 0x7654321, 3, 0x2468ACE]


class Case:
    """(component index, log_size) list -> device columns, the three calls, their results"""

    def __init__(self, pkg, ctx, comps, base):
        self.pkg, self.ctx, self.ptrs = pkg, ctx, []
        elems = [int(v) or 1 for v in splitmix_column(77, 24)]
        self.items, at = [], 0
        for k, (comp, log) in enumerate(comps):
            program, _, columns = pkg.brainfuck_air_program(comp)
            n = 2 << log
            cols = []
            for _ in columns:      # distinct buffers of distinct words: slices of one long splitmix column
                at = at + 977 if at + 977 + n <= base.size else 0
                cols.append(self.up(base[at: at + n]))
            self.items.append(dict(program=program, kernel=ctx.air_compile(program), log=log, cols=cols, params=pkg.brainfuck_air_params(elems, splitmix_column(78 + k, 4).tolist())))
        self.dst_log = max(log for _, log in comps) + 1
        self.sizes = sorted({i["log"] + 1 for i in self.items}, reverse=True)
        self.dst = {kind: [self.empty(1 << self.dst_log) for _ in range(4)] for kind in KINDS}
        self.accs = {el: (self.dst["sequence"] if el == self.dst_log else [self.empty(1 << el) for _ in range(4)]) for el in self.sizes}
        self.coeffs = pkg.air_compose_coeffs([i["program"].shape["n_constraints"] for i in self.items], R)
        self.entries = {"compose": [(i["program"], i["log"], 1, i["cols"], i["params"]) for i in self.items],
                        "compose_compiled": [(i["kernel"], i["log"], 1, i["cols"], i["params"]) for i in self.items]}

    def up(self, arr):
        self.ptrs.append(self.ctx.upload(arr))
        return self.ptrs[-1]

    def empty(self, n):
        self.ptrs.append(self.ctx.malloc(4 * n))
        return self.ptrs[-1]

    def call(self, kind):
        ctx, L = self.ctx, self.pkg.lib()
        if kind != "sequence":
            ctx.air_compose(self.entries[kind], R, self.dst[kind], self.dst_log)
            return
        for el, acc in self.accs.items():
            for p in acc:
                assert L.bfhip_memset_zero(ctx._h, ctypes.c_void_p(p), ctypes.c_size_t(4 << el)) == 0
        g = 0
        for i in self.items:
            n = i["program"].shape["n_constraints"]
            ctx.air_eval_domain(i["program"], i["log"], 1, i["cols"], i["params"], self.coeffs[g: g + n], self.accs[i["log"] + 1])
            g += n
        for el, acc in self.accs.items():
            ctx.interpolate(acc, acc, el)
        for el, acc in self.accs.items():
            if el != self.dst_log:
                for w in range(4):
                    ctx.accumulate(self.dst["sequence"][w], acc[w], 1 << el)

    def check(self):
        for kind in KINDS:
            self.call(kind)
        want = [self.ctx.download(p, 1 << self.dst_log) for p in self.dst["sequence"]]
        for kind in KINDS[:2]:
            if not all(np.array_equal(self.ctx.download(p, 1 << self.dst_log), w) for p, w in zip(self.dst[kind], want)):
                raise SystemExit("air_compose_rate: %s and the sequence of single operations disagree" % kind)
        assert any(w.any() for w in want)

    def measure(self, calls, rounds):
        paths = {k: (lambda k=k: self.call(k)) for k in KINDS}
        ms = alternate(self.ctx, paths, calls, rounds)
        # where the GPU time of a call goes
        return ms, {k: {name: t for name, (t, _) in events(self.ctx, paths[k], calls).items()} for k in KINDS}

    def bytes_moved(self):
        """(a)'s and (c)'s HBM bytes of the sweep and the finalize by count: columns read once; accumulator words written (a: once per row;
        c: a zero fill, then read + written per component); transforms and additions are the same for both and left out"""
        cols = sum(4 * (2 << i["log"]) * len(i["cols"]) for i in self.items)
        rows_once = sum(16 << el for el in self.sizes)
        per_comp = sum(2 * (16 * (2 << i["log"])) for i in self.items)
        return cols + rows_once, cols + rows_once + per_comp

    def close(self):
        for i in self.items:
            i["kernel"].close()
        for p in self.ptrs:
            self.ctx.free(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--program", default=os.path.join(ROOT, "tests", "golden", "programs", "fib19.bf")); ap.add_argument("--input", default="")
    ap.add_argument("--shrink", type=int, default=0); ap.add_argument("--equal-log", type=int, default=18)
    ap.add_argument("--calls", type=int, default=10); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--out")
    a = ap.parse_args()
    pkg = load_package()
    require_gpu(pkg, "air_compose_rate")
    log_sizes, steps = Oracle().log_sizes(open(a.program).read(), a.input.encode())
    log_sizes = [l - a.shrink if l >= 4 + a.shrink else l for l in log_sizes]
    top = max(max(log_sizes), a.equal_log) + 1
    base = splitmix_column(4242, (1 << top) + (1 << 16))
    ctx = pkg.Context(0, max_log_domain=top)
    lines = [f"BFHIP_AIR_COMPOSE_LAUNCH={os.environ.get('BFHIP_AIR_COMPOSE_LAUNCH', '(unset)')}: bfhip_air_compose beside the sequence of single operations (bfhip_air_eval_domain per component into zeroed accumulators, bfhip_interpolate per size, "
             f"bfhip_accumulate per smaller size): {a.rounds} alternating rounds of {a.calls} calls after a warm-up round; the same words in all four columns checked first", "",
             "case | components | distinct sizes | largest domain | ms per call, median (min-max): (a) compose, interpreted | (b) compose, compiled kernels | (c) the sequence | "
             "(c) / (a) | (c) / (b) | sweep bytes by count (a), (c)"]
    detail = []
    try:
        for name, comps in (("brainfuck, %s (%d steps), component log sizes %s" % (os.path.basename(a.program), steps, log_sizes), list(enumerate(log_sizes))),
                            ("8 equal: the processor program at log_size %d" % a.equal_log, [(3, a.equal_log)] * 8)):
            case = Case(pkg, ctx, comps, base)
            try:
                case.check()
                ms, events = case.measure(a.calls, a.rounds)
                med = {k: statistics.median(ms[k]) for k in KINDS}
                ba, bc = case.bytes_moved()
                lines.append(f"{name} | {len(comps)} | {len(case.sizes)} | 2^{case.dst_log} | {cell(ms['compose'], 3)} | {cell(ms['compose_compiled'], 3)} | {cell(ms['sequence'], 3)} | "
                             f"{med['sequence'] / med['compose']:.2f}x | {med['sequence'] / med['compose_compiled']:.2f}x | {ba / 2**20:.0f} MiB, {bc / 2**20:.0f} MiB")
                for k, label in zip(KINDS, ("(a)", "(b)", "(c)")):
                    detail.append(f"  {name.split(',')[0].split(':')[0]} {label} GPU ms per call by HIP events (one profiled round): " +
                                  ", ".join(f"{n} {t:.3f}" for n, t in sorted(events[k].items(), key=lambda e: -e[1])) + f"; sum {sum(events[k].values()):.3f}")
                lds = sorted({(256 * (i["program"].shape["m_regs"] + 4 * i["program"].shape["q_regs"]), i["log"]) for i in case.items}, key=lambda e: -e[1])
                detail.append(f"  {name.split(',')[0].split(':')[0]} register files in LDS, bytes per wave (log_size): " + ", ".join(f"{b} ({l})" for b, l in lds) +
                              f"; k_air_compose asks for {max(b for b, _ in lds)} for every wave")
            finally:
                case.close()
    finally:
        ctx.close()
    emit("\n".join(lines + [""] + detail) + "\n", a.out)


if __name__ == "__main__":
    main()
