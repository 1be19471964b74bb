#!/usr/bin/env python3
"""What filling a lookup's multiplicity column on the device costs: bfhip_relation_program_multiplicities beside (a) the relation tracker's
bfhip_relation_program_summary on the same tables with the column filled — the same extraction, sort and scan volume, reporting instead of
writing — and (b) the host route it replaces: download the consumer's and the table's tuple columns, count with numpy, upload the column.
In one run on one GPU.

  python3 tools/relation_multiplicities_rate.py [--log-consumer 20] [--log-table 16] [--passes 10] [--rounds 5] [--out FILE]

  tables     a consumer of 2^20 rows whose every row looks one tuple up (multiplicity 1) in a table of 2^16 distinct tuples, at tuple widths
             1 and 3; full-size columns resident in HBM (row_shift 0). Every table tuple is used, nothing is missing.
  device     Context.relation_program_multiplicities(tables, 0, 1, 0, mult): the column it fills is the one the table side reads.
  summary    Context.relation_program_summary on the same tables, mult filled: balanced, no entry to report.
  host       bfhip_download of the consumer's and the table's word columns, the tuples packed to one key per row (a 4 w-byte void view),
             np.unique(return_counts) over the consumer's keys, np.searchsorted of the table's keys, bfhip_upload of the column into a fresh
             buffer. Pageable numpy memory, one host thread: what a caller without this entry point writes.
  time       ms per call: the three alternate in windows of `passes` back-to-back calls, `rounds` rounds (at least five); the two device
             paths also by HIP events, by profiler scope (tools/ratelib.py has the scheme). Every call ends in its own read-backs or
             copies, so a call is what a caller waits for.
  check      before the timing: the three columns are equal, and the summary says balanced.

No threshold is attached. A run without a GPU fails: nothing here is measured on the host alone."""
import argparse
import statistics

import numpy as np

from ratelib import alternate, cell, emit, events, load_package, require_gpu

P = (1 << 31) - 1


def splitmix(seed, n):
    z = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def keys_of(cols):
    rows = np.ascontiguousarray(np.stack(cols, axis=1))
    return rows.view(np.dtype((np.void, 4 * len(cols)))).ravel()


def measure(pkg, ctx, a, width):
    n, m = 1 << a.log_consumer, 1 << a.log_table
    # 2^log_table distinct tuples: word 0 is a permutation of odd multiples, the other words hang on the row
    ids = np.argsort(splitmix(11 * width, m), kind="stable").astype(np.uint32)
    table = [(ids * np.uint32(2) + np.uint32(1)) % np.uint32(P)] + [(splitmix(100 + k, m) % np.uint64(P)).astype(np.uint32) for k in range(1, width)]
    pick = (splitmix(7 + width, n) % np.uint64(m)).astype(np.int64)
    pick[:m] = np.arange(m)          # every table row is used at least once
    consumer = [c[pick] for c in table]
    b = pkg.AirBuilder()
    b.relation_entry(0, 1, [b.col(k) for k in range(width)])
    consumer_prog = b.relation_program([width])
    b = pkg.AirBuilder()
    b.relation_entry(0, -b.col(width), [b.col(k) for k in range(width)])
    table_prog = b.relation_program([width])
    ptrs = []
    try:
        d_consumer = [ctx.upload(c) for c in consumer]; ptrs += d_consumer
        d_table = [ctx.upload(c) for c in table]; ptrs += d_table
        d_mult = ctx.malloc(4 * m); ptrs.append(d_mult)
        tables = [(consumer_prog, a.log_consumer, 0, d_consumer), (table_prog, a.log_table, 0, d_table + [d_mult])]
        device = lambda: ctx.relation_program_multiplicities(tables, 0, 1, 0, d_mult, max_missing=4)
        summary = lambda: ctx.relation_program_summary(tables, max_entries=4)

        def host():
            got = [ctx.download(p, n) for p in d_consumer]
            tab = [ctx.download(p, m) for p in d_table]
            uniq, counts = np.unique(keys_of(got), return_counts=True)
            tab_keys = keys_of(tab)
            at = np.minimum(np.searchsorted(uniq, tab_keys), len(uniq) - 1)
            mult = np.where(uniq[at] == tab_keys, counts[at], 0).astype(np.uint32)
            fresh = ctx.upload(mult)
            host.last = mult
            ctx.free(fresh)

        res = device()
        on_device = ctx.download(d_mult, m)
        host()
        want = np.bincount(pick, minlength=m).astype(np.uint32)
        if not (res.ok and np.array_equal(on_device, want) and np.array_equal(host.last, want) and summary().balanced):
            raise SystemExit("relation_multiplicities_rate: the paths disagree at width %d: %r" % (width, res.report))

        calls = {"device": device, "summary": summary, "host": host}
        ms = alternate(ctx, calls, a.passes, a.rounds)
        ev = {name: {s: t for s, (t, _) in sorted(events(ctx, calls[name], a.passes).items())} for name in ("device", "summary")}
        return ms, ev, res.report
    finally:
        for p in ptrs:
            ctx.free(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log-consumer", type=int, default=20); ap.add_argument("--log-table", type=int, default=16)
    ap.add_argument("--passes", type=int, default=10); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("relation_multiplicities_rate: at least five rounds")
    pkg = load_package()
    require_gpu(pkg, "relation_multiplicities_rate")
    ctx = pkg.Context(0, max_log_domain=26)
    lines = [f"bfhip_relation_program_multiplicities (device) beside bfhip_relation_program_summary on the same tables with the column filled (summary) and beside "
             f"download + np.unique / np.searchsorted + upload (host): 2^{a.log_consumer} consumer rows, each looking one tuple up with multiplicity 1 in a table of "
             f"2^{a.log_table} distinct tuples, full-size columns resident in HBM; {a.rounds} alternating rounds of {a.passes} calls after a warm-up round, the context "
             f"synchronised around every window; each call ends in its read-backs or copies; equal columns and a balanced summary checked first", ""]
    try:
        for width in (1, 3):
            ms, ev, report = measure(pkg, ctx, a, width)
            med = {k: statistics.median(v) for k, v in ms.items()}
            lines += [f"tuple width {width}: n_entries {report['n_entries']}, n_tuples {report['n_tuples']}, n_rows {report['n_rows']}, n_filled {report['n_filled']}, "
                      f"n_missing {report['n_missing']}",
                      "path | ms per call: median (min-max) | by HIP events per call: all scopes; by scope"]
            for name in ("device", "summary", "host"):
                by_events = "-" if name == "host" else "%.4f; %s" % (sum(ev[name].values()), ", ".join("%s %.4f" % kv for kv in ev[name].items()))
                lines.append(f"{name} | {cell(ms[name], 4)} | {by_events}")
            lines += [f"device / summary | {med['device'] / med['summary']:.2f}x", f"host / device | {med['host'] / med['device']:.2f}x", ""]
    finally:
        ctx.close()
    emit("\n".join(lines), a.out)


if __name__ == "__main__":
    main()
