#!/usr/bin/env python3
"""What building a memory-consistency table from a row-order register trace costs on the device: the Memory pipeline of
brainfuck_rows_fill — bfhip_rows_select sorting the rows by (mp, clk) into a device order, bfhip_rows_fill inserting the clk-gap rows —
beside (a) a device-to-device copy of the OUTPUT's bytes, (b) k_select_gather writing as many columns and rows, and (c) the route an author
had before: download the trace, numpy.lexsort, the repeat counts, numpy.repeat, the storage-order permutation per column, upload. In one run
on one GPU.

  python3 tools/rows_fill_rate.py [--passes 5] [--rounds 5] [--small] [--out FILE]

  shapes     2^24 and 2^20 register rows x 7 words (clk, ip, ci, ni, mp, mv, mvi), row-major and column-major, resident in HBM. clk = the
             row index; every 16 consecutive steps share two cells, mp = 2 (clk / 16) + a pseudo-random bit, so that a cell is left and
             come back to within its block: gaps of 0 to 14 rows, T between n and 2 n. The other columns are random canonical words.
             --small: 2^16 and 2^14 rows (a dry run).
  select     one count-only bfhip_rows_select call ordered by (mp, clk) that leaves the order on the device, its read-backs included.
  fill       one bfhip_rows_fill call through that order — group mp, step clk, BFHIP_FILL_GAPS; clk, mp, mv as KEEP, d as MARK 1 and the same
             four at offset 1 — into 8 resident columns of 2^(log n + 1) words, both read-backs included, on a context with a scratch reserve
             (--reserve-mib). By HIP events (the library's profiler) it splits into counts + scan (k_fill_counts, rows_fill_scan) and
             k_fill_gather; GB/s of the gather = 8 bytes per output word over its time.
  copy       hipMemcpyAsync device to device of 4 x 8 x 2^log_out bytes, then a wait for the device.
  sel.gather k_select_gather alone (by HIP events) inside a bfhip_rows_select call that writes 8 columns of 2^log_out rows from a table of
             2^log_out rows (the trace twice over) ordered by (mp, clk): the same number of words written, a permuted source row per output row.
  numpy      row-major only, one call per window, 2 windows after a warm-up: bfhip_download of the trace, tests/rows_fill_model.py's fill
             over a numpy.lexsort order, per column the storage-order index and bfhip_upload into a fresh buffer, free.
  time       ms per call: select, fill and copy alternate in windows, `rounds` rounds (at least five) after a warm-up round (ratelib).
  check      before the timing: the device's columns equal the numpy route's, byte for byte, and T is the model's.

No threshold is attached. A run without a GPU fails: nothing here is measured on the host alone."""
import argparse
import ctypes
import statistics

import numpy as np

from ratelib import alternate, cell, emit, events, load_package, require_gpu

import columns_model      # tests/ (ratelib put it on the path)
import rows_fill_model as model

P = (1 << 31) - 1
D2D = 3      # hipMemcpyDeviceToDevice
N_COLS, N_OUT = 7, 8
KEEP = [("keep", 0), ("keep", 4), ("keep", 5), ("mark", 1)]
FILL = dict(group=(4,), step=0, gaps=True, columns=KEEP + [c + (1,) for c in KEEP])
SELECT_OUT = [0, 4, 5, 6, (0, 1), (4, 1), (5, 1), (6, 1)]


def make_table(log_n):
    rng = np.random.default_rng(log_n)
    n = 1 << log_n
    t = rng.integers(0, P, size=(n, N_COLS), dtype=np.uint32)
    clk = np.arange(n, dtype=np.uint32)
    t[:, 0] = clk
    t[:, 4] = 2 * (clk // 16) + rng.integers(0, 2, size=n, dtype=np.uint32)
    return t


def measure(pkg, ctx, hip, a, table, src, wide, layout):
    n = table.shape[0]
    log_out = n.bit_length()      # log n + 1: T <= 2 n
    m = 1 << log_out
    index = columns_model.rows_of_cells(log_out)
    ptrs = []
    try:
        cols = [ctx.malloc(4 * m) for _ in range(N_OUT)]; ptrs += cols
        copy_src, copy_dst = ctx.malloc(4 * m * N_OUT), ctx.malloc(4 * m * N_OUT); ptrs += [copy_src, copy_dst]
        order_d = ctx.malloc(4 * n); ptrs.append(order_d)

        def select():
            ctx.rows_select_count(src, order_by=(4, 0), order_out=order_d)

        def fill():
            fill.last = ctx.rows_fill(src, log_out, order=order_d, n_order=n, out=cols, **FILL).n_filled

        def copy():
            assert hip.hipMemcpyAsync(ctypes.c_void_p(copy_dst), ctypes.c_void_p(copy_src), ctypes.c_size_t(4 * m * N_OUT), D2D, None) == 0
            assert hip.hipDeviceSynchronize() == 0

        def select_gather():
            ctx.rows_select(wide, log_out, order_by=(4, 0), columns=SELECT_OUT, rows=(0, m - 1), out=cols)

        def numpy_route():
            t = ctx.download(table_d, n * N_COLS).reshape(n, N_COLS)
            order = np.lexsort((t[:, 0], t[:, 4]))
            rows, numpy_route.T = model.fill(t, log_out, FILL["group"], FILL["step"], True, FILL["columns"], order)
            numpy_route.last = [np.ascontiguousarray(rows[:, c][index]) for c in range(N_OUT)]
            for c in numpy_route.last:
                ctx.free(ctx.upload(c))

        select(); fill()
        ms = alternate(ctx, {"select": select, "fill": fill, "copy": copy}, a.passes, a.rounds)
        ev = events(ctx, fill, a.passes)
        ev_sel = events(ctx, select_gather, 2)
        if layout == "rows":
            table_d = src.ptr
            select(); fill()
            got = np.stack([ctx.download(p, m) for p in cols])
            numpy_route()
            if fill.last != numpy_route.T or got.tobytes() != np.stack(numpy_route.last).tobytes():
                raise SystemExit("rows_fill_rate: the device and the numpy route disagree at 2^%d" % (n.bit_length() - 1))
            ms.update(alternate(ctx, {"numpy": numpy_route}, 1, 2))
        return ms, ev, ev_sel, log_out, fill.last
    finally:
        for p in ptrs:
            ctx.free(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=5); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--small", action="store_true"); ap.add_argument("--out")
    ap.add_argument("--reserve-mib", type=int, default=2048)
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("rows_fill_rate: at least five rounds")
    pkg = load_package()
    require_gpu(pkg, "rows_fill_rate")
    hip = ctypes.CDLL("libamdhip64.so")
    ctx = pkg.Context(0, max_log_domain=16)
    ctx.set_scratch_reserve(a.reserve_mib << 20)
    logs = (16, 14) if a.small else (24, 20)
    lines = [f"The Memory pipeline over 2^{logs[0]} and 2^{logs[1]} register rows x {N_COLS} resident in HBM: bfhip_rows_select ordering them by (mp, clk) into a device order (select), "
             f"bfhip_rows_fill through that order with the clk-gap rows inserted, {N_OUT} columns of twice as many rows (fill), beside a device-to-device copy of the output's bytes "
             f"(copy), k_select_gather writing as many columns and rows from a table of as many rows (sel.gather, by HIP events) and download + numpy + upload (numpy, row-major "
             f"only); a context with a scratch reserve: {a.rounds} alternating rounds of {a.passes} calls (numpy: 2 rounds of 1 call) after a warm-up round, the context synchronised "
             f"around every window; equal bytes (device = numpy route) checked for the row-major cases. fill split by HIP events in one further window: counts = k_fill_counts + "
             f"rows_fill_scan, gather = k_fill_gather with GB/s over 8 bytes per output word.", "",
             "case | path | ms per call: median (min-max)"]
    try:
        for log_n in logs:
            table = make_table(log_n)
            n = 1 << log_n
            twice = np.concatenate([table, table])
            for layout in ("rows", "columns"):
                held = [ctx.upload(table), ctx.upload(twice)] if layout == "rows" else [ctx.upload(t[:, c]) for t in (table, twice) for c in range(N_COLS)]
                src = pkg.DeviceRows(held[0], n, N_COLS, N_COLS) if layout == "rows" else pkg.DeviceRowColumns(held[:N_COLS], n)
                wide = pkg.DeviceRows(held[1], 2 * n, N_COLS, N_COLS) if layout == "rows" else pkg.DeviceRowColumns(held[N_COLS:], 2 * n)
                try:
                    ms, ev, ev_sel, log_out, T = measure(pkg, ctx, hip, a, table, src, wide, layout)
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    name = "2^%d x %d %s -> %d x 2^%d, T = %d" % (log_n, N_COLS, "row-major" if layout == "rows" else "column-major", N_OUT, log_out, T)
                    for path in ("select", "fill", "copy", "numpy"):
                        if path in ms:
                            lines.append(f"{name} | {path} | {cell(ms[path], 4)}")
                    counts = ev.get("k_fill_counts", (0.0, 0))[0] + ev.get("rows_fill_scan", (0.0, 0))[0]
                    gather, sel_gather = ev.get("k_fill_gather", (0.0, 0))[0], ev_sel.get("k_select_gather", (0.0, 0))[0]
                    out_bytes = 8.0 * N_OUT * (1 << log_out)
                    lines.append(f"{name} | by HIP events, ms per call | counts + scan {counts:.4f}, gather {gather:.4f} ({out_bytes / gather / 1e6:.0f} GB/s); "
                                 f"sel.gather {sel_gather:.4f} ({out_bytes / sel_gather / 1e6:.0f} GB/s over the same bytes)")
                    ratios = (f"(select + fill) / copy {(med['select'] + med['fill']) / med['copy']:.2f}x; fill / copy {med['fill'] / med['copy']:.2f}x; "
                              f"fill gather / select gather {gather / sel_gather:.2f}x; fill gather / copy {gather / med['copy']:.2f}x")
                    if "numpy" in med:
                        ratios += f"; numpy / (select + fill) {med['numpy'] / (med['select'] + med['fill']):.0f}x"
                    lines += [f"{name} | ratios of median ms | {ratios}", ""]
                finally:
                    for p in held:
                        ctx.free(p)
        stats = ctx.scratch_stats()
        lines.append(f"scratch reserve {stats['reserve'] >> 20} MiB, high water {stats['high_water'] / 2**20:.0f} MiB, device allocations by call-scoped memory on that context: {stats['device_allocations']}")
    finally:
        ctx.close()
    emit("\n".join(lines), a.out)


if __name__ == "__main__":
    main()
